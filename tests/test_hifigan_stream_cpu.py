"""CPU: the arithmetic tts_hifigan_chunk and tts_hifigan_stream rest on, in the float64 torch restatement (tests/hifigan_ref.py), and the stream driver's
host-side row bookkeeping. A window is decoded from the slice [w0, w1) of the whole utterance's interpolated signal (the interpolation is a function of the
absolute frame and L: exact per frame) as a sequence of its own, zero padding at both ends as the convolutions give it; the kept frames must equal the whole
decode. 1e-12: float64 convolutions of another length may sum in another order (observed differences ~1e-15 on outputs of magnitude <= 1)."""
import numpy as np
import pytest
import torch

import hifigan_ref as R
from test_hifigan_cpu import hifigan_model, inputs  # noqa: F401

HALO = 24  # TTS_HFG_HALO_FRAMES
TOL = 1e-12


@pytest.fixture(scope="module")
def W(hifigan_model):
    return R.load(hifigan_model)


@pytest.fixture(scope="module")
def whole(W):
    """decode of the whole utterance, once per length"""
    memo = {}

    def run(L):
        if L not in memo:
            lat, v = inputs(60)
            memo[L] = R.decode(W, lat[:L], v)
        return memo[L]
    return run


def window_decode(W, lat, v, frame0, n, halo):
    """the samples of frames [frame0, frame0 + n) from the window with `halo` frames of context, as the device evaluates it"""
    T = R.frames(len(lat))
    w0, w1 = max(0, frame0 - halo), min(T, frame0 + n + halo)
    z = R.upsample(torch.as_tensor(lat).to(torch.float64))[..., w0:w1]
    keep = R.upsample
    R.upsample = lambda _lat: z  # decode() on the sliced, absolutely indexed interpolation
    try:
        out = R.decode(W, lat, v)
    finally:
        R.upsample = keep
    assert len(out) == 256 * (w1 - w0)
    return out[256 * (frame0 - w0):256 * (frame0 - w0 + n)]


@pytest.mark.parametrize("L", [20, 60])
def test_window_arithmetic(W, whole, L):
    lat, v = inputs(60)
    lat = lat[:L]
    T = R.frames(L)
    full = whole(L)
    for f0, n in ((30, 20), (0, 10), (T - 5, 5)):
        got = window_decode(W, lat, v, f0, n, HALO)
        err = np.abs(got - full[256 * f0:256 * (f0 + n)]).max()
        print("L = %d window [%d, %d) of %d: max abs %.2e" % (L, f0, f0 + n, T, err))
        assert err <= TOL


def test_halo_must_stay_24(W, whole):
    lat, v = inputs(60)
    got = window_decode(W, lat, v, 30, 20, 8)
    err = np.abs(got - whole(60)[256 * 30:256 * 50]).max()
    print("halo 8, window [30, 50): max abs %.2e" % err)
    assert err > TOL, "a halo of 8 frames reproduces the whole decode: the receptive field is not what the header says"


@pytest.mark.parametrize("Lp", [7, 20, 33])
def test_prefix_property(W, whole, Lp):
    cut = 256 * (R.frames(Lp) - HALO)
    assert cut > 0
    err = np.abs(whole(Lp)[:cut] - whole(60)[:cut]).max()
    print("first %d of 60 rows: max abs %.2e on the %d frames below frames(L') - 24" % (Lp, err, cut // 256))
    assert err <= TOL


def test_row_bookkeeping(pkg):
    """the rows declared final after k codes are a prefix of the utterance's rows however it ends: at any later length, with a stop token or cut"""
    L = pkg.lib()
    rs = np.random.RandomState(3)
    seqs = [rs.randint(0, 8192, 40), rs.randint(0, 8192, 40), rs.randint(0, 8192, 40)]
    seqs[1][10:22] = 83   # the sampler itself produces the run trim_latents cuts at
    seqs[2][31:40] = 83   # ... at the very end
    for codes in seqs:
        codes = np.ascontiguousarray(codes, np.int32)
        ends = {}
        for n in range(41):
            for stop in (False, True):
                end = np.ascontiguousarray(np.append(codes[:n], 8193) if stop else codes[:n], np.int32)
                padded = np.empty(502, np.int32)
                assert L.tts_host_pad_codes(end, len(end), padded) == 0
                ends[n, stop] = (padded, L.tts_host_trimmed_rows(padded))
        last = 0
        for k in range(41):
            r = L.tts_host_stream_final_rows(codes.ctypes.data, k)
            assert last <= r <= k + 1, (k, r)
            last = r
            for n in range(k, 41):
                for stop in (False, True):
                    padded, rows_end = ends[n, stop]
                    assert r <= rows_end, (k, r, n, stop, rows_end)
                    assert np.array_equal(padded[:r], np.concatenate([[8192], codes])[:r])  # the inputs of the final rows are final
        assert L.tts_host_stream_final_rows(codes.ctypes.data, 5) == 6  # and no rows are held back without a reason
    assert L.tts_host_stream_final_rows(None, 0) == 1 and L.tts_host_stream_final_rows(None, 3) == -1 and L.tts_host_stream_final_rows(None, -1) == -1
