"""No GPU: what tests/test_afe_kernels_gpu.py rests on. The two float64 spellings of the resampler agree; its length, gain and pitch are right; the mel reference
agrees with tts_host_mel_*; the product's tables are the references' tables rounded once; a NumPy float32 restatement of each kernel's operation order stays inside
the derived bounds on the whole case matrix, and nine seeded defects fall outside them; the harness refuses every invalid case before any device call; tts_read_wav
reads hand-written headers."""
import ctypes as C
import struct

import numpy as np
import pytest

import afe_cases as V
from afe_cases import MEL80, MEL100, NONFINITE, RESAMPLE, Case


@pytest.fixture(scope="module")
def res_refs():
    """(case, reference, bound) of the whole resampler matrix, computed once"""
    return [(c,) + V.reference(c)[0] for c in V.res_cases()]


@pytest.fixture(scope="module")
def mel_refs():
    return {b: [(c,) + V.reference(c)[0] for c in V.mel_cases(b)] for b in (80, 100)}


def test_resampler_spellings_agree(res_refs):
    worst = 0.0
    for c, y, _ in res_refs:
        d = V.res_direct(c.clips[0], c.p["orig"], c.p["new"])
        worst = max(worst, float(np.abs(y - d).max() / max(1.0, np.abs(c.clips[0]).max())))
    print("polyphase table against direct evaluation: %.2e" % worst)
    assert worst <= 1e-12


def test_resampler_table_shapes_and_length(res_refs):
    shapes = {(22050, 24000): (160, 161), (44100, 22050): (1, 28), (16000, 22050): (441, 334), (48000, 22050): (147, 348), (8000, 22050): (441, 174)}
    for (a, b), shp in shapes.items():
        assert V.res_table(a, b).shape == shp
        rc, o, n, width, taps = V.geometry(a, b)
        assert rc == 0 and (n, taps) == shp and (o, n, width, taps) == V.res_geometry(a, b)[:4]
    for c, y, _ in res_refs:
        o, n = V.res_geometry(c.p["orig"], c.p["new"])[:2]
        assert len(y) == -(-n * len(c.clips[0]) // o)
    assert V.geometry(*V.LIMIT_PAIR)[0] == V.ERR_LIMIT and V.geometry(22050, 22050)[:3] == (0, 1, 1)


def test_product_tables_are_the_reference_tables_rounded_once():
    L = V.lib()
    for a, b in V.RATE_PAIRS:
        want = V.res_table(a, b)
        got = np.zeros(want.shape, np.float32)
        assert L.tts_afe_test_table(a, b, got.ctypes.data_as(C.c_void_p)) == 0
        assert (np.abs(got - want) <= V.U * np.abs(want) + 2.0 ** -149).all()  # libm and NumPy may differ in the last bit of the double
    t = np.zeros(2048, np.float32)
    L.tts_afe_test_fft_tables(t.ctypes.data_as(C.c_void_p))
    k, i = np.arange(512), np.arange(1024)
    assert np.abs(t[:512] - np.cos(2 * np.pi * k / 1024)).max() <= V.U and np.abs(t[512:1024] + np.sin(2 * np.pi * k / 1024)).max() <= V.U
    assert np.abs(t[1024:] - (0.5 - 0.5 * np.cos(2 * np.pi * i / 1024))).max() <= V.U
    for bands in (80, 100):
        span = np.zeros((bands, 3), np.int32)
        w = np.zeros(4096, np.float32)
        nw = L.tts_afe_test_filterbank(bands, span.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), len(w))
        fb = V.fb_of(bands)
        dense = np.zeros_like(fb)
        for b in range(bands):
            k0, cnt, off = span[b]
            dense[b, k0:k0 + cnt] = w[off:off + cnt]
        assert 0 < nw <= len(w) and span[:, 1].max() < 64  # narrow triangles, not 513-wide rows
        assert (np.abs(dense - fb) <= 2 * V.U * np.abs(fb) + 1e-12).all()


def test_resampler_gain_and_pitch():
    for a, b in V.RATE_PAIRS:
        o, n, width = V.res_geometry(a, b)[:3]
        y, _ = V.res_reference(np.ones(6 * width + 12 * o + 5), a, b)
        edge = -(-n * (width + 1) // o) + 1  # outputs whose taps reach the zero padding
        assert len(y) > 2 * edge + n and np.abs(y[edge:len(y) - edge] - 1.0).max() <= 1e-3, (a, b)
        t = np.arange(a // 2) / a
        z, _ = V.res_reference(0.5 * np.sin(2 * np.pi * 440 * t), a, b)
        k = np.argmax(np.abs(np.fft.rfft(z * np.hanning(len(z)))))
        assert abs(k * b / len(z) - 440) < 3, (a, b)
    x = np.random.RandomState(0).randn(100)
    assert (V.resample64(x, 22050, 22050) == x).all()  # equal rates: the samples pass through


def test_mel_reference_agrees_with_host_mel(pkg):
    rs = np.random.RandomState(3)
    n = 4096 + 77
    t = np.arange(n) / 24000.0
    audio = (0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t + 1) + 0.05 * rs.randn(n)).astype(np.float32)
    norms = V.mel_norms()
    want, _ = V.mel_reference(audio, 0, n, 100)
    got = pkg.host_mel_diffusion100(audio)
    assert got.shape == want.shape and np.abs(got - want).max() < 2e-5 * 11.6  # tests/test_mel_frontend.py's tolerances
    want, _ = V.mel_reference(audio, 0, n, 80, norms)
    got = pkg.host_mel_voice80(audio, norms)
    assert got.shape == want.shape and np.abs(got - want).max() < 2e-5 * max(1.0, np.abs(want).max())


def test_f32_restatement_stays_inside_the_bounds(res_refs, mel_refs):
    worst = {}
    for c, y, b in res_refs + mel_refs[80] + mel_refs[100]:
        e, = V.emulate(c)
        assert e.shape == y.shape, c.name()
        bad, r = V.judge(e, y, b)
        assert bad == 0, (c.name(), bad, r)
        worst[c.kind] = max(worst.get(c.kind, 0.0), r)
    print({V.KIND_NAMES[k]: round(v, 4) for k, v in worst.items()})
    norms = V.mel_norms()
    c = Case(MEL80, [V.mel_input("noise", 900, 1, 80)], "noise", start=[0], win=[900], norms=norms)
    (y, b), = V.reference(c)
    assert V.judge(V.emulate(c)[0], y, b)[0] == 0


def test_zero_input_is_the_floor_exactly():
    norms = V.mel_norms()
    for bands, nm in ((80, None), (80, norms), (100, None)):
        e = V.mel_emulate(np.zeros(700, np.float32), 0, 700, bands, nm)
        want = np.repeat((V.LOG_FLOOR / (nm if nm is not None else np.ones(bands, np.float32)))[:, None], e.shape[1], axis=1).astype(np.float32)
        assert e.dtype == np.float32 and (e.view(np.uint32) == want.view(np.uint32)).all()
        ref, bound = V.mel_reference(np.zeros(700, np.float32), 0, 700, bands, nm)
        assert V.judge(e, ref, bound)[0] == 0


RES_DEFECTS = [("a phase shifted by one tap", dict(phase_shift=1)), ("width one short", dict(width_short=1)), ("truncation to floor", dict(floor=True)),
               ("a missing base / o scale", dict(no_scale=True))]
MEL_DEFECTS = [("reflect index off by one", dict(reflect_off=1)), ("symmetric instead of periodic Hann", dict(symmetric_hann=True)),
               ("power instead of magnitude (and the reverse)", dict(power="swap")), ("HTK and Slaney scales swapped", dict(swap_scale=True)),
               ("the clamp applied after the log", dict(clamp_after_log=True))]


@pytest.mark.parametrize("what,defect", RES_DEFECTS, ids=[d[0] for d in RES_DEFECTS])
def test_seeded_resampler_defects_fall_outside(res_refs, what, defect):
    caught = 0
    for c, y, b in res_refs:
        if c.family != "noise":
            continue
        e, = V.emulate(c, **defect)
        caught += e.shape != y.shape or V.judge(e, y, b)[0] > 0
    assert caught, what


@pytest.mark.parametrize("what,defect", MEL_DEFECTS, ids=[d[0] for d in MEL_DEFECTS])
def test_seeded_mel_defects_fall_outside(mel_refs, what, defect):
    for bands in (80, 100):
        d = dict(defect)
        if d.get("power") == "swap":
            d["power"] = 3 - V.MEL_PARAMS[bands][3]
        caught = 0
        for c, y, b in mel_refs[bands]:
            if c.family == "zeros" and "clamp_after_log" not in d:
                continue
            e, = V.emulate(c, **d)
            with np.errstate(invalid="ignore"):
                caught += V.judge(e, y, b)[0] > 0
        assert caught, (what, bands)


def test_every_invalid_harness_case_is_refused():
    x = np.zeros(600, np.float32)
    ok_r = Case(RESAMPLE, [x], orig=44100, new=22050)
    ok_m = Case(MEL80, [x], start=[0], win=[600])
    assert V.validate(ok_r) == 0 and V.validate(ok_m) == 0 and V.validate(Case(NONFINITE, [x])) == 0
    assert V.validate(Case(RESAMPLE, [x], orig=22050, new=22050)) == 0  # the copy
    assert V.validate(Case(RESAMPLE, [x], orig=V.LIMIT_PAIR[0], new=V.LIMIT_PAIR[1])) == V.ERR_LIMIT
    bad = [
        Case(7, [x]), Case(-1, [x]),
        Case(RESAMPLE, [x], orig=0, new=22050), Case(RESAMPLE, [x], orig=22050, new=-1),
        Case(RESAMPLE, [x] * 4, orig=44100, new=22050),                       # more clips than the harness takes
        Case(RESAMPLE, [np.zeros((1 << 18) + 1, np.float32)], orig=44100, new=22050),
        Case(MEL80, [x], start=[0], win=[512]),                               # reflect padding needs more than 512 samples
        Case(MEL100, [x], start=[0], win=[(1 << 18) + 1]),
        Case(MEL80, [x], start=[-1], win=[600]), Case(MEL80, [x], start=[600], win=[600]),  # the window starts outside the clip
        Case(MEL100, [x], start=[0], win=[600], norms=np.ones(80, np.float32)),             # the product divides the 80-band side only
        Case(MEL80, [x]),                                                      # no start / win
    ]
    for c in bad:
        assert V.validate(c) == V.HIP_INVALID, c.name()
    for field in ("in_", "out", "in_len"):
        assert V.validate(ok_r, **{field: None}) == V.HIP_INVALID, field
    assert V.validate(ok_m, n_clips=0) == V.HIP_INVALID
    c, keep = ok_r.struct()
    assert V.lib().tts_afe_test_run(None) == V.HIP_INVALID  # refused before any HIP call: this test has no device


def _wav(fmt, channels, rate, bits, data, extra=b"", fmt_extra=b""):
    body = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16 + len(fmt_extra), fmt, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits) + fmt_extra
    body += extra + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_read_wav(tmp_path, pkg):
    t = np.arange(800) / 16000.0
    x = (0.5 * np.sin(2 * np.pi * 440 * t)).astype(np.float32)

    def put(name, blob):
        p = str(tmp_path / name)
        open(p, "wb").write(blob)
        return p

    # float32 mono: the inverse of tts_write_wav, bit for bit
    p = str(tmp_path / "w.wav")
    assert pkg.write_wav(p, x, 16000) == 0
    y, rate = pkg.read_wav(p)
    assert rate == 16000 and (y.view(np.uint32) == x.view(np.uint32)).all()
    # PCM16 stereo: the channels are averaged
    l, r = np.round(x * 32767).astype(np.int16), np.round(-0.5 * x * 32767).astype(np.int16)
    y, rate = pkg.read_wav(put("s16.wav", _wav(1, 2, 22050, 16, np.stack([l, r], axis=1).tobytes())))
    assert rate == 22050 and len(y) == len(x) and np.abs(y - (l / 32768.0 + r / 32768.0) / 2).max() < 1e-7
    # PCM24 with negative samples
    v = np.round(x * 8388607).astype(np.int32)
    b24 = b"".join(struct.pack("<i", int(s))[:3] for s in v)
    y, rate = pkg.read_wav(put("s24.wav", _wav(1, 1, 48000, 24, b24)))
    assert rate == 48000 and np.abs(y - v / 8388608.0).max() < 1e-7 and y.min() < -0.4
    # float32 behind an odd-sized unknown chunk (one pad byte follows it) and a LIST chunk
    extra = b"junk" + struct.pack("<I", 3) + b"abc\0" + b"LIST" + struct.pack("<I", 4) + b"INFO"
    y, rate = pkg.read_wav(put("odd.wav", _wav(3, 1, 24000, 32, x.tobytes(), extra=extra)))
    assert rate == 24000 and (y == x).all()
    # errors: truncated data, no file, not RIFF, another format
    L = pkg.lib()
    rate = C.c_int32()
    blob = _wav(3, 1, 24000, 32, x.tobytes())
    assert L.tts_read_wav(put("cut.wav", blob[:-100]).encode(), None, 0, C.byref(rate)) == -2
    assert L.tts_read_wav(put("hdr.wav", blob[:30]).encode(), None, 0, C.byref(rate)) in (-2, -3)
    assert L.tts_read_wav(str(tmp_path / "none.wav").encode(), None, 0, C.byref(rate)) == -2
    assert L.tts_read_wav(put("bad.wav", b"RIFX" + blob[4:]).encode(), None, 0, C.byref(rate)) == -3
    assert L.tts_read_wav(put("alaw.wav", _wav(6, 1, 8000, 8, b"\0" * 64)).encode(), None, 0, C.byref(rate)) == -3
    with pytest.raises(pkg.TtsError):
        pkg.read_wav(str(tmp_path / "cut.wav"))
    out = np.zeros(10, np.float32)
    assert L.tts_read_wav(p.encode(), out.ctypes.data_as(C.c_void_p), 10, C.byref(rate)) == -1  # cap below the sample count
