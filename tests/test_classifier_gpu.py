"""GPU: the synthesized-speech classifier (tts_load_classifier / tts_classify_audio, csrc/classifier.h) against the float64 restatement tests/classifier_ref.py on
synthetic weights, its bit-level properties, the crop, the resampler path, its error statuses, its neighbours, and the path through the C ABI and the CLI.
Unpinned against upstream (no source or weights offline), unjudged on real audio; pinned between independent implementations: see tests/test_classifier_cpu.py.

Gate: 1e-3 absolute on the logits (classifier_ref.GATE), the gate CVVP's scores and both decoders' waveforms are held to; tests/test_classifier_cpu.py holds a
float32 restatement of the whole network within 1e-4 of float64 on every weight and clip pair used here. The stage is f32 throughout, the attention blocks
included.
The measured figures are in DESIGN.md, "What pins the classifier"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import classifier_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = 220000


@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(name):
        if name not in made:
            e = pkg.Engine(0)
            e.load_classifier(R.model(name)[0])
            made[name] = e
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _softmax0(l):
    e = np.exp(l - l.max())
    return e[0] / e.sum()


CASES = [(name, n) for name in ("tiny", "upstream") for n in R.GPU_SAMPLES[name]]


@pytest.mark.parametrize("name,n", CASES, ids=["%s-n%d" % c for c in CASES])
def test_engine_vs_float64(engines, name, n):
    prob, logits = engines(name).classify_audio([R.wave(name, n)], 24000)
    want = R.reference(name, n)
    err = np.abs(logits[0] - want).max()
    print("classifier %s n = %d: logits %s, max abs distance from float64 %.2e (gate %.0e), probability %.6f" % (name, n, logits[0], err, R.GATE, prob[0]))
    assert np.isfinite(logits).all() and err <= R.GATE
    assert abs(prob[0] - _softmax0(want)) <= R.GATE and abs(prob[0] - _softmax0(logits[0].astype(np.float64))) <= 1e-6


def test_ragged_batch_alone_twice_and_reversed(engines):
    eng = engines("tiny")
    clips = [R.wave("tiny", n, k=1 + i) for i, n in enumerate(R.RAGGED + (1000,))]
    pa, la = eng.classify_audio(clips, 24000)
    pb, lb = eng.classify_audio(clips, 24000)
    pr, lr = eng.classify_audio(clips[::-1], 24000)
    assert np.array_equal(la, lb) and np.array_equal(pa, pb), "two calls differ"
    assert np.array_equal(la, lr[::-1]) and np.array_equal(pa, pr[::-1]), "the order of the clips matters"
    for i, c in enumerate(clips):
        p1, l1 = eng.classify_audio([c], 24000)
        assert np.array_equal(l1[0], la[i]) and p1[0] == pa[i], "clip %d differs from itself alone" % i
        want = R.index(R.model("tiny")[1], c)
        assert np.abs(la[i] - want).max() <= R.GATE
    assert not np.array_equal(la[0], la[3])  # same length, another clip


def test_ragged_batch_upstream_configuration(engines):
    eng = engines("upstream")
    ns = (1025, 20000, 1024)
    clips = [R.wave("upstream", n) for n in ns]
    pa, la = eng.classify_audio(clips, 24000)
    for i, n in enumerate(ns):
        assert np.abs(la[i] - R.reference("upstream", n)).max() <= R.GATE
        assert np.array_equal(eng.classify_audio([clips[i]], 24000)[1][0], la[i])


@pytest.mark.parametrize("name", ["tiny", "upstream"])
def test_crop(engines, name):
    """the first 220 000 samples are all the network sees: 220 000, 220 001 and 300 000 samples of one signal give the same bits"""
    eng = engines(name)
    x = R.wave(name, 300000)
    base = eng.classify_audio([x[:CROP]], 24000)
    assert np.isfinite(base[1]).all()
    for n in (CROP + 1, 300000):
        got = eng.classify_audio([x[:n]], 24000)
        assert np.array_equal(got[1], base[1]) and np.array_equal(got[0], base[0]), n
    shorter = eng.classify_audio([x[:CROP - 1]], 24000)
    assert not np.array_equal(shorter[1], base[1])  # and the last of them is seen
    both = eng.classify_audio([x, x[:CROP]], 24000)  # batch equals alone at full length
    assert np.array_equal(both[1][0], base[1][0]) and np.array_equal(both[1][1], base[1][0])


def test_resampler_path(engines):
    """A clip at 24 kHz reaches the network bit for bit whether or not the call runs the resampler for another clip; a clip at another rate is the float64
    network on the float64 resampler's output (tests/afe_cases.py: resample64, one stage to 24 kHz), within the gate."""
    import afe_cases as A
    eng = engines("tiny")
    x24, x22, x48 = R.wave("tiny", 3000), R.wave("tiny", 2500, k=3), R.wave("tiny", 5000, k=4)
    alone = eng.classify_audio([x24], 24000)[1][0]
    p, l = eng.classify_audio([x22, x24, x48, x24], [22050, 24000, 48000, 24000])
    assert np.array_equal(l[1], alone) and np.array_equal(l[3], alone)
    t = R.model("tiny")[1]
    for i, (x, rate) in ((0, (x22, 22050)), (2, (x48, 48000))):
        y = A.resample64(x, rate, 24000)
        want = R.index(t, y)
        err = np.abs(l[i] - want).max()
        print("classifier at %d Hz: %d -> %d samples, logits within %.2e of float64" % (rate, len(x), len(y), err))
        assert err <= R.GATE
        assert np.array_equal(eng.classify_audio([x], rate)[1][0], l[i])
    # the crop applies at 24 kHz: a long clip at 48 kHz is its first 440 000 samples
    long48 = R.wave("tiny", 450000, k=5)
    a = eng.classify_audio([long48], 48000)[1]
    b = eng.classify_audio([long48[:440100]], 48000)[1]  # 440 000 and the resampler's reach behind them
    assert np.array_equal(a, b)


def _raw(eng, audio, n, rates, nc, prob, logits):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return eng.L.tts_classify_audio(eng.h, p(audio), p(n), p(rates), nc, p(prob), p(logits))


def test_errors(pkg, engines):
    eng = engines("tiny")
    S, A, LIM = -5, -1, -6
    x, n, r = R.wave("tiny", 100), np.array([100], np.int64), np.array([24000], np.int32)
    prob, logits = np.full(1, 7.0, np.float32), np.full(2, 7.0, np.float32)
    fresh = pkg.Engine(0)
    assert _raw(fresh, x, n, r, 1, prob, logits) == S and b"tts_load_classifier not called" in fresh.L.tts_last_error(fresh.h)
    assert fresh.L.tts_load_classifier(fresh.h, os.path.join(ROOT, "models", "mol.bin").encode()) < 0
    assert _raw(fresh, x, n, r, 1, prob, logits) == S  # a refused load leaves the context unloaded
    fresh.close()
    bad = lambda *a: (_raw(eng, *a), eng.L.tts_last_error(eng.h).decode())  # noqa: E731
    for args in ((None, n, r, 1, prob, logits), (x, None, r, 1, prob, logits), (x, n, None, 1, prob, logits), (x, n, r, 1, None, logits), (x, n, r, 0, prob, logits)):
        rc, msg = bad(*args)
        assert rc == A and "bad argument" in msg, (rc, msg)
    rc, msg = bad(x, np.array([0], np.int64), r, 1, prob, logits)
    assert rc == A and "0 samples" in msg
    for rate in (0, -24000):
        rc, msg = bad(x, n, np.array([rate], np.int32), 1, prob, logits)
        assert rc == A and "outside the audio front end's range" in msg
    rc, msg = bad(np.zeros(257, np.float32), np.ones(257, np.int64), np.full(257, 24000, np.int32), 257, np.zeros(257, np.float32), None)
    assert rc == LIM and "257 clips" in msg
    for val in (np.nan, np.inf, -np.inf):
        x2 = x.copy()
        x2[50] = val
        rc, msg = bad(x2, n, r, 1, prob, logits)
        assert rc == A and "non-finite" in msg
    assert prob[0] == 7.0 and (logits == 7.0).all(), "a refused call wrote its output"
    assert _raw(eng, x, n, r, 1, prob, None) == 0 and prob[0] != 7.0  # logits_out may be NULL
    assert np.abs(eng.classify_audio([x], 24000)[1][0] - R.index(R.model("tiny")[1], x)).max() <= R.GATE  # and the context still works
    with pytest.raises(pkg.TtsError):
        eng.classify_audio([x, x], [24000])


def test_profiler_families(engines):
    eng = engines("tiny")  # depth 2, one ResBlock per level, one attention block
    eng.prof_reset(True)
    eng.classify_audio([R.wave("tiny", 1000)], 24000)
    conv, gn, attn = (eng.prof_get(f) for f in ("cls_conv", "cls_gn", "cls_attn"))
    eng.prof_reset(False)
    assert conv[1] == 1 + 2 * 2 + 2 + 1 and gn[1] == 2 * 2 + 1 and attn[1] == 1 + 1
    assert conv[0] > 0 and gn[0] > 0 and attn[0] > 0 and conv[2] > 0


def test_neighbours_keep_their_bytes(pkg, small_models):
    """tts_vocoder, tts_bigvgan and tts_hifigan_decode return the bytes they returned before the classifier was loaded and run; a call between two steps of an
    open diffusion session leaves the session's mel bit-equal"""
    import bigvgan_ref as BR
    from test_hifigan_cpu import inputs
    from tortoise_cpp_amd import synth_weights as sw
    hfg = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "hifigan", "ggml-hifigan-model.bin")
    if not os.path.exists(hfg + ".done"):
        os.makedirs(os.path.dirname(hfg), exist_ok=True)
        sw.write_hifigan(hfg, seed=1240)
        open(hfg + ".done", "w").write("ok")
    e = pkg.Engine(0)
    e.load(diffusion=small_models + "/ggml-diffusion-model.bin", vocoder=small_models + "/ggml-vocoder-model.bin")
    e.load_hifigan(hfg)
    e.load_bigvgan(BR.model("tiny")[0])
    lat, v = inputs(9)
    T = e.frames(9)
    rs = np.random.RandomState(1)
    nz, vz = rs.randn(5, 100 * T).astype(np.float32), rs.randn(64, T + 10).astype(np.float32)
    mel0 = e.diffusion([lat], n_steps=4, noise=[nz])[0]
    a0, b0, h0 = e.vocoder([mel0], noise=[vz])[0], e.bigvgan([mel0])[0], e.hifigan_decode([lat], v)[0]

    def session(between):
        e.diff_session_open(1024, 1)
        rid = e.diff_session_admit([lat], n_steps=4, noise=[nz])
        e.diff_session_step()
        between()
        while e.diff_session_step():
            pass
        out = e.diff_session_collect(rid)[0]
        e.diff_session_close()
        return out
    s0 = session(lambda: None)
    e.load_classifier(R.model("tiny")[0])
    clip = h0[:5000]
    c0 = e.classify_audio([clip], 24000)
    assert np.isfinite(c0[1]).all()
    mel1 = e.diffusion([lat], n_steps=4, noise=[nz])[0]
    assert np.array_equal(mel0, mel1) and np.array_equal(a0, e.vocoder([mel1], noise=[vz])[0]) and np.array_equal(b0, e.bigvgan([mel1])[0])
    assert np.array_equal(h0, e.hifigan_decode([lat], v)[0])
    got = []
    s1 = session(lambda: got.append(e.classify_audio([clip, a0[:3000]], [24000, 22050])))
    assert np.array_equal(s0, s1) and np.array_equal(got[0][1][0], c0[1][0])
    e.close()


def test_cli_detect_prints_what_the_call_returns(pkg, engines, tmp_path):
    eng = engines("tiny")
    clips = [R.wave("tiny", 3000, k=7), R.wave("tiny", 2000, k=8)]
    paths = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for p, c, rate in zip(paths, clips, (24000, 22050)):
        assert pkg.lib().tts_write_wav(p.encode(), c, len(c), rate) == 0
    want = eng.classify_audio(clips, [24000, 22050])[0]
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    r = subprocess.run([exe, "--detect", ",".join(paths), "--classifier", R.model("tiny")[0]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("detect: ")]
    assert [row[1] for row in rows] == paths
    assert [np.float32(row[2]) for row in rows] == list(want)
    r = subprocess.run([exe, "--detect", str(tmp_path / "none.wav"), "--classifier", R.model("tiny")[0]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "not a readable RIFF WAV" in r.stderr
