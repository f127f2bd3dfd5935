"""GPU: the DVAE decoder through the C ABI (tts_load_dvae_decoder / tts_dvae_decode / tts_dvae_reconstruct, csrc/dvae_dec.h) against the float64 statement
tests/dvae_dec_ref.py on the two smallest configurations at which the kernels can go wrong (A: two k 3 / s 2 layers; B: k 7 / s 4, 64 -> 128 channels) and
1, 2, 31, 32, 33, 63, 64, 65 codes per clip, alone and as neighbours in one ragged batch.

Decoded mel: every element within the propagated bound c U (|b| + sum |w| |x| + |resid|) per layer with c = taps x input channels + 2, U = 2^-24 (n chained
multiply-adds on the f32 MFMA, the bias, one residual add or once-rounded folded weight; carried through sum |w| err_in), AND within the 1e-3 gate of the
project's f32 stages. Reconstruction error: relative 1e-5 against float64 on the codes the engine's own encoder returned. Measured figures: profiles/dvae_decoder.txt."""
import ctypes as C

import numpy as np
import pytest

import dvae_dec_ref as R

pytestmark = pytest.mark.gpu
ARG, STATE = -1, -5
p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(name):
        if name not in made:
            made[name] = pkg.Engine(0)
            made[name].load_dvae_decoder(R.model(name)[0])
            if name == "A":
                made[name].load_dvae(R.model("enc")[0])
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _check(name, n, mel, seed=0):
    ref = R.reference(name, n, seed)
    assert mel.shape == ref["mel"].shape and np.isfinite(mel).all()
    d = np.abs(mel - ref["mel"])
    print("dvae_dec %s n = %d: max abs distance from float64 %.2e (gate %.0e, mel up to %.1f), worst ratio to the bound %.2e"
          % (name, n, d.max(), R.GATE, np.abs(ref["mel"]).max(), (d / ref["bound"]).max()))
    assert (d <= ref["bound"]).all() and d.max() <= R.GATE


@pytest.mark.parametrize("n", R.COUNTS)
@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_single_clip_vs_float64(engines, name, n):
    eng = engines(name)
    cfg = R.CONFIGS[name]
    assert eng.dvae_decode_frames(n) == n * cfg["stride"] ** cfg["layers"]
    _check(name, n, eng.dvae_decode([R.codes_for(name, n)])[0])


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_ragged_batch_planted_edges_and_bit_identities(engines, name):
    """The counts as neighbours: every clip begins with code 0 and ends with tokens - 1 beside a neighbour that ends / begins with the other, so a read across a
    clip boundary or a wrong zero pad shows against float64; one clip of equal codes is constant per phase inside, so a wrong floor((t - pad + j) / s) shows at
    its edges only. Two runs agree and every clip alone is the clip in the batch, bit for bit."""
    eng = engines(name)
    batch = [R.codes_for(name, n, 1 + i) for i, n in enumerate(R.COUNTS)]
    flat = np.full(33, 5, np.int32)
    got = eng.dvae_decode(batch + [flat])
    again = eng.dvae_decode(batch + [flat])
    for i, (n, c) in enumerate(zip(R.COUNTS, batch)):
        _check(name, n, got[i], 1 + i)
        assert np.array_equal(got[i], again[i]), "two runs differ"
        assert np.array_equal(eng.dvae_decode([c])[0], got[i]), "clip %d differs from itself alone" % i
    want = R.decode(R.model(name)[1], flat)
    f = R.CONFIGS[name]["stride"] ** R.CONFIGS[name]["layers"]  # frames per code
    assert np.abs(got[-1] - want["mel"]).max() <= R.GATE and (np.abs(got[-1] - want["mel"]) <= want["bound"]).all()
    assert np.array_equal(got[-1][:, 16 * f:17 * f], got[-1][:, 17 * f:18 * f]), "far from its ends a clip of equal codes repeats every code"


def test_layout_round_trip_and_reconstruct(pkg, engines):
    eng = engines("A")
    codes = [R.codes_for("A", n, 3) for n in (33, 2, 65)]
    mels = eng.dvae_decode(codes)
    back = eng.dvae_codes(mels)  # band-major, no reshaping
    assert [len(b) for b in back] == [eng.dvae_rows(m.shape[1]) for m in mels] == [33, 2, 65]
    # reconstruction error of arbitrary mels, against float64 on the codes the engine's own encoder returned (an encoder tie cannot fail this)
    r = np.random.default_rng(5)
    src = [(0.5 * r.standard_normal((80, T))).astype(np.float32) for T in (130, 7, 257)]
    enc = eng.dvae_codes(src)
    l1, mse, rec = eng.dvae_reconstruct(src, mel_out=True)
    dec = eng.dvae_decode(enc)
    for i, (m, c) in enumerate(zip(src, enc)):
        assert np.array_equal(rec[i], dec[i]), "mel_out is not tts_dvae_decode of the encoder's codes"
        want = R.decode(R.model("A")[1], c)["mel"]
        k = min(m.shape[1], want.shape[1])
        d = m[:, :k].astype(np.float64) - want[:, :k]
        e1, e2 = abs(l1[i] - np.abs(d).mean()) / np.abs(d).mean(), abs(mse[i] - (d * d).mean()) / (d * d).mean()
        print("dvae_dec reconstruct T = %d: %d codes, L1 %.6f MSE %.6f, relative distance from float64 %.2e / %.2e" % (m.shape[1], len(c), l1[i], mse[i], e1, e2))
        assert e1 <= 1e-5 and e2 <= 1e-5
    a1, a2 = eng.dvae_reconstruct(src)
    assert np.array_equal(a1, l1) and np.array_equal(a2, mse)
    for half in ("load_dvae", "load_dvae_decoder"):
        one = pkg.Engine(0)
        getattr(one, half)(R.model("enc" if half == "load_dvae" else "A")[0])
        m, fr, out = src[1].reshape(-1), np.array([7], np.int32), np.full(2, 7, np.float32)
        assert one.L.tts_dvae_reconstruct(one.h, p(m), p(fr), 1, p(out), p(out), None) == STATE and (out == 7).all()
        one.close()


def test_out_of_range_code_and_other_refusals(engines):
    eng = engines("A")
    L, h = eng.L, eng.h
    mel, fr = np.full(80 * 16, 7, np.float32), np.full(1, 7, np.int32)
    call = lambda codes, n=4, k=1, stride=4, cap=mel.size: L.tts_dvae_decode(h, p(np.array(codes, np.int32)), p(np.array([n], np.int32)), k, stride, p(mel), p(fr), cap)  # noqa: E731
    assert call([1, 2, 64, 3]) == ARG and "code 64 at position 2" in L.tts_last_error(h).decode()
    assert call([1, -1, 2, 3]) == ARG and call([1, 2, 3, 4], n=0) == ARG and call([1, 2, 3, 4], n=5) == ARG and call([1, 2, 3, 4], k=0) == ARG
    assert call([1, 2, 3, 4], cap=80 * 16 - 1) == ARG and "mel_out holds" in L.tts_last_error(h).decode()
    assert L.tts_dvae_decode(h, p(np.zeros(4097, np.int32)), p(np.array([4097], np.int32)), 1, 4097, p(mel), p(fr), mel.size) == -6  # 16388 frames
    assert (mel == 7).all() and fr[0] == 7, "a refused call wrote its output"
    assert call([1, 2, 63, 0]) == 0 and fr[0] == 16 and not (mel == 7).any()


def test_a_call_inside_an_open_ar_session(pkg, mid_models, voice):
    """tts_dvae_decode between two steps of an open AR session: every request's codes, rows and latents are the bits of the session without the call"""
    from test_ar_session_gpu import req, run_session
    eng = pkg.Engine(0)
    eng.load(ar=mid_models + "/ggml-model.bin")
    eng.load_dvae_decoder(R.model("A")[0])
    reqs = [req(9, 2, 1, [6, 9]), req(16, 1, 2, [8], at=2)]
    shape = (4, 2, 16, 12)
    base = run_session(eng, reqs, voice, shape=shape)
    got = []
    with_call = run_session(eng, reqs, voice, shape=shape, on_step=lambda step, rid_of, live: got.append(eng.dvae_decode([R.codes_for("A", 33)])[0]) if step == 2 else None)
    assert len(got) == 1 and np.array_equal(got[0], eng.dvae_decode([R.codes_for("A", 33)])[0])
    assert sorted(base) == sorted(with_call)
    for k in base:
        for a, b in zip(base[k], with_call[k]):
            if isinstance(a, (list, tuple)):
                assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
            else:
                assert np.array_equal(a, b)
    eng.close()
