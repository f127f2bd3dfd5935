"""GPU: the wav2vec2 CTC aligner (tts_load_aligner / tts_aligner_ids / tts_align_audio / tts_redact_audio, csrc/aligner.h) against the float64 restatement
tests/aligner_ref.py on synthetic weights, its bit-level properties, the resampler path, its error statuses, an open AR session beside it, and the path through
the C ABI and the CLI. Unpinned against upstream (no source or weights offline); pinned between independent implementations: see tests/test_aligner_cpu.py.

Gate: 1e-3 absolute on the logits (aligner_ref.GATE), the project's gate for f32 stages. The ids must equal the float64 argmax on EVERY frame:
tests/test_aligner_cpu.py asserts that the float64 top-two margin exceeds twice the gate on every frame of every 16 kHz clip used here, so nothing is excluded.
The measured figures are in DESIGN.md, "What pins the aligner", and profiles/aligner.txt."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import aligner_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, A, LIM = -5, -1, -6


@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(name):
        if name not in made:
            e = pkg.Engine(0)
            e.load_aligner(R.model(name)[0])
            made[name] = e
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _vocab(name):
    return R.model(name)[1]["aligner.vocab"].astype(np.int32)


CASES = [(name, n) for name in R.CONFIGS for n in R.GPU_SAMPLES[name]]


@pytest.mark.parametrize("name,n", CASES, ids=["%s-n%d" % c for c in CASES])
def test_engine_vs_float64(engines, name, n):
    ids, logits = engines(name).aligner_ids([R.wave(name, n)], 16000, logits=True)
    want = R.reference(name, n)
    assert logits[0].shape == want.shape and ids[0].shape == (want.shape[0],)
    err = np.abs(logits[0] - want).max()
    print("aligner %s n = %d: %d frames, logits max abs distance from float64 %.2e (gate %.0e, logits up to %.1f, smallest margin %.4f)"
          % (name, n, want.shape[0], err, R.GATE, np.abs(want).max(), R.margin(want).min()))
    assert np.isfinite(logits[0]).all() and err <= R.GATE
    assert np.array_equal(ids[0], want.argmax(1)), "an id differs from the float64 argmax"
    assert np.array_equal(ids[0], logits[0].argmax(1))
    assert np.array_equal(engines(name).aligner_ids([R.wave(name, n)], 16000)[0], ids[0])  # without the logits: the same ids


def test_vocab_frames_and_config(engines, pkg):
    for name, cfg in R.CONFIGS.items():
        v, blank = engines(name).aligner_vocab()
        assert np.array_equal(v, _vocab(name)) and blank == cfg["blank"] and len(v) == cfg["V"]
        for n in R.GPU_SAMPLES[name]:
            assert engines(name).L.tts_aligner_clip_frames(engines(name).h, n, 16000) == R.frames(name, n)
        assert engines(name).L.tts_aligner_clip_frames(engines(name).h, 29, 16000) == A  # below one frame


def test_ragged_batch_alone_twice_and_reversed(engines):
    eng = engines("even")
    clips = [R.wave("even", n, k=1 + i) for i, n in enumerate(R.RAGGED)]
    ia, la = eng.aligner_ids(clips, 16000, logits=True)
    ib, lb = eng.aligner_ids(clips, 16000, logits=True)
    ir, lr = eng.aligner_ids(clips[::-1], 16000, logits=True)
    for i, c in enumerate(clips):
        assert np.array_equal(la[i], lb[i]) and np.array_equal(ia[i], ib[i]), "two calls differ"
        assert np.array_equal(la[i], lr[len(clips) - 1 - i]) and np.array_equal(ia[i], ir[len(clips) - 1 - i]), "the order of the clips matters"
        i1, l1 = eng.aligner_ids([c], 16000, logits=True)
        assert np.array_equal(l1[0], la[i]) and np.array_equal(i1[0], ia[i]), "clip %d differs from itself alone" % i
        want = R.reference("even", R.RAGGED[i], 1 + i)
        assert np.abs(la[i] - want).max() <= R.GATE and np.array_equal(ia[i], want.argmax(1))
    two = eng.aligner_ids([clips[0], clips[2]], 16000, logits=True)
    assert np.array_equal(two[1][0], la[0]) and np.array_equal(two[1][1], la[2])


def test_resampler_path(engines):
    """The identity the resampler allows: a clip at 16 kHz reaches the network bit for bit whether or not the call runs the resampler for another clip; a clip
    at another rate is NOT bit-equal to anything on the host - it is the float64 network on the float64 resampler's output (tests/afe_cases.py: resample64,
    one stage to 16 kHz, the resampler tts_audio_mel's front end uses) within the gate, with the ids equal wherever the float64 margin exceeds twice the gate."""
    import afe_cases as AF
    eng = engines("even")
    x16, x22, x48 = R.wave("even", 1290), R.wave("even", 2500, k=3), R.wave("even", 5000, k=4)
    alone = eng.aligner_ids([x16], 16000, logits=True)
    ids, lg = eng.aligner_ids([x22, x16, x48, x16], [22050, 16000, 48000, 16000], logits=True)
    assert np.array_equal(lg[1], alone[1][0]) and np.array_equal(lg[3], alone[1][0]) and np.array_equal(ids[1], alone[0][0])
    t = R.model("even")[1]
    for i, (x, rate) in ((0, (x22, 22050)), (2, (x48, 48000))):
        y = AF.resample64(x, rate, 16000)
        want = R.index(t, y)
        assert lg[i].shape == want.shape
        err = np.abs(lg[i] - want).max()
        sure = R.margin(want) > 2 * R.GATE
        print("aligner at %d Hz: %d -> %d samples, %d frames, logits within %.2e of float64, %d frames with a margin above twice the gate"
              % (rate, len(x), len(y), want.shape[0], err, sure.sum()))
        assert err <= R.GATE and np.array_equal(ids[i][sure], want.argmax(1)[sure])
        again = eng.aligner_ids([x], rate, logits=True)
        assert np.array_equal(again[1][0], lg[i]) and np.array_equal(again[0][0], ids[i])


def _raw(eng, audio, n, rates, nc, ids, nf, stride, logits):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return eng.L.tts_aligner_ids(eng.h, p(audio), p(n), p(rates), nc, p(ids), p(nf), stride, p(logits))


def test_errors(pkg, engines):
    eng = engines("even")
    x, n, r = R.wave("even", 1290), np.array([1290], np.int64), np.array([16000], np.int32)
    ids, nf, lg = np.full(64, 7, np.int32), np.full(1, 7, np.int32), np.full(64 * 29, 7.0, np.float32)
    off, out = np.full(16, 7, np.int64), np.full(1290, 7.0, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fresh = pkg.Engine(0)
    assert _raw(fresh, x, n, r, 1, ids, nf, 64, lg) == S and b"tts_load_aligner not called" in fresh.L.tts_last_error(fresh.h)
    assert fresh.L.tts_align_audio(fresh.h, p(x), 1290, 16000, b"abc", p(off), 16) == S
    assert fresh.L.tts_redact_audio(fresh.h, p(x), 1290, 16000, b"a[b]c", p(out), 1290) == S
    assert fresh.L.tts_aligner_vocab(fresh.h, None, 0, None) == S
    assert fresh.L.tts_load_aligner(fresh.h, os.path.join(ROOT, "models", "mol.bin").encode()) < 0
    assert _raw(fresh, x, n, r, 1, ids, nf, 64, lg) == S  # a refused load leaves the context unloaded
    fresh.close()
    bad = lambda *a: (_raw(eng, *a), eng.L.tts_last_error(eng.h).decode())  # noqa: E731
    for args in ((None, n, r, 1, ids, nf, 64, lg), (x, None, r, 1, ids, nf, 64, lg), (x, n, None, 1, ids, nf, 64, lg), (x, n, r, 1, None, nf, 64, lg),
                 (x, n, r, 1, ids, None, 64, lg), (x, n, r, 0, ids, nf, 64, lg), (x, n, r, 1, ids, nf, 0, lg)):
        rc, msg = bad(*args)
        assert rc == A and "bad argument" in msg, (rc, msg)
    rc, msg = bad(x, np.array([0], np.int64), r, 1, ids, nf, 64, lg)
    assert rc == A and "0 samples" in msg
    rc, msg = bad(x, np.array([29], np.int64), r, 1, ids, nf, 64, lg)
    assert rc == A and "less than one frame" in msg
    rc, msg = bad(x, n, r, 1, ids, nf, 63, lg)
    assert rc == A and "frame_stride is 63" in msg
    rc, msg = bad(x, np.array([(1 << 26) + 1], np.int64), r, 1, ids, nf, 64, lg)
    assert rc == LIM and "2^26" in msg
    for rate in (0, -16000):
        rc, msg = bad(x, n, np.array([rate], np.int32), 1, ids, nf, 64, lg)
        assert rc == A and "outside the audio front end's range" in msg
    rc, msg = bad(np.zeros(257 * 40, np.float32), np.full(257, 40, np.int64), np.full(257, 16000, np.int32), 257, np.zeros(257, np.int32), np.zeros(257, np.int32), 1, None)
    assert rc == LIM and "257 clips" in msg
    for val in (np.nan, np.inf, -np.inf):
        x2 = x.copy()
        x2[700] = val
        rc, msg = bad(x2, n, r, 1, ids, nf, 64, lg)
        assert rc == A and "non-finite" in msg
        assert eng.L.tts_align_audio(eng.h, p(x2), 1290, 16000, b"abc", p(off), 16) == A
        assert eng.L.tts_redact_audio(eng.h, p(x2), 1290, 16000, b"a[b]c", p(out), 1290) == A
        assert eng.L.tts_redact_audio(eng.h, p(x2), 1290, 16000, b"abc", p(out), 1290) == A
    # the text: too many characters for the room, brackets, '~', no UTF-8; a kept size beyond the room
    assert eng.L.tts_align_audio(eng.h, p(x), 1290, 16000, b"abc", p(off), 2) == A and "room for 2 of 3" in eng.L.tts_last_error(eng.h).decode()
    assert eng.L.tts_align_audio(eng.h, p(x), 1290, 16000, b"a~c", p(off), 16) == A
    assert eng.L.tts_align_audio(eng.h, p(x), 1290, 16000, b"\xff\xfe", p(off), 16) == A
    assert eng.L.tts_align_audio(eng.h, p(x), 1290, 16000, None, p(off), 16) == A and eng.L.tts_align_audio(eng.h, p(x), 1290, 16000, b"abc", None, 16) == A
    for text in (b"a[b", b"a]b", b"a[[b]]c"):
        assert eng.L.tts_redact_audio(eng.h, p(x), 1290, 16000, text, p(out), 1290) == A
    assert eng.L.tts_redact_audio(eng.h, p(x), 1290, 16000, b"abc", p(out), 1289) == A  # no bracket: the whole clip must fit
    assert (ids == 7).all() and nf[0] == 7 and (lg == 7.0).all() and (off == 7).all() and (out == 7.0).all(), "a refused call wrote its output"
    assert _raw(eng, x, n, r, 1, ids, nf, 64, None) == 0 and nf[0] == 64 and np.array_equal(ids, R.reference("even", 1290).argmax(1))  # logits_out may be NULL
    assert (lg == 7.0).all()
    with pytest.raises(pkg.TtsError):
        eng.aligner_ids([x, x], [16000])


def test_profiler_families(engines):
    eng = engines("even")  # 3 convolution layers, 2 encoder layers
    eng.prof_reset(True)
    eng.aligner_ids([R.wave("even", 1290)], 16000)
    conv, attn, row = (eng.prof_get(f) for f in ("w2v_conv", "w2v_attn", "w2v_row"))
    eng.prof_reset(False)
    assert conv[1] == 1 + 2 + 1 + 1 + 2 * 4 + 1 and attn[1] == 2 and row[1] == 1 + 3 + 1 + 2 * 3 + 1
    assert conv[0] > 0 and attn[0] > 0 and row[0] > 0 and conv[2] > 0


def _prompts(s):
    """prompts built from the decoded string s of a clip: a bracketed span at the start, in the middle, at the end; two spans; characters the audio does not
    hold inside and outside a span (they stay open and are interpolated)"""
    a, b = len(s) // 3, 2 * len(s) // 3
    return ["[" + s[:a] + "]" + s[a:], s[:a] + "[" + s[a:b] + "]" + s[b:], s[:b] + "[" + s[b:] + "]", "[" + s[:5] + "]" + s[5:a] + "[" + s[a:b] + "]" + s[b:],
            s[:a] + "[" + s[a:a + 4] + "yy" + s[a + 4:b] + "]" + s[b:], s[:7] + "zy" + s[7:a] + "[" + s[a:b] + "]" + s[b:] + "zzz", s.upper()[:a] + "[" + s[a:] + "]",
            "[" + s + "]", s, "[]" + s]


@pytest.mark.parametrize("name,n,k,rate", [("odd", 2600, 1, 16000), ("even", 2600, 3, 16000), ("even", 1800, 5, 24000)])
def test_alignment_with_a_known_answer(engines, name, n, k, rate):
    """The device ids of a synthetic clip decode to a string; prompts built from that string must align and redact, element for element, as the Python
    restatement does on the REFERENCE ids (the float64 argmax). At 24 kHz the clip is the caller's: offsets and slices are in its samples."""
    eng = engines(name)
    clip = R.wave(name, n, k)
    vocab, blank = _vocab(name), R.CONFIGS[name]["blank"]
    ids = eng.aligner_ids([clip], rate)[0]
    if rate == 16000:
        ref_ids = R.reference(name, n, k).argmax(1)
        assert np.array_equal(ids, ref_ids)
    else:
        ref_ids = ids  # another rate: the resampler path is held in test_resampler_path; here the host rules run on the caller's sample count
    s = R.ctc_decode(ref_ids, vocab, blank)
    assert len(s) >= 20, s
    for text in _prompts(s):
        bare, iv = R.redact_spans(text)
        want_al = R.ctc_align(ref_ids, vocab, blank, bare, len(clip)) if bare else []
        got_al = eng.align_audio(clip, rate, bare)
        assert list(got_al) == want_al, text
        want = R.redact(clip, ref_ids, vocab, blank, text)
        got = eng.redact_audio(clip, rate, text)
        assert got.dtype == np.float32 and np.array_equal(got, want), text
        if "[" in text and iv:
            assert 0 < len(got) < len(clip) or len(want) == 0
    assert np.array_equal(eng.redact_audio(clip, rate, s), clip)  # no bracket: the clip unchanged
    assert len(eng.redact_audio(clip, rate, "[" + s + "]")) == 0


def test_text_that_is_not_in_the_audio_fails(pkg, engines):
    eng = engines("even")  # 29 tokens: a .. x, no y, no z
    clip = R.wave("even", 2600, k=3)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    off, out = np.full(16, 7, np.int64), np.full(2600, 7.0, np.float32)
    assert eng.L.tts_align_audio(eng.h, p(clip), 2600, 16000, b"zyzzy", p(off), 16) == A
    assert "the text does not match the audio" in eng.L.tts_last_error(eng.h).decode()
    assert eng.L.tts_redact_audio(eng.h, p(clip), 2600, 16000, b"[zyz]zyzzy", p(out), 2600) == A
    assert "the text does not match the audio" in eng.L.tts_last_error(eng.h).decode()
    assert (off == 7).all() and (out == 7.0).all(), "a failed alignment wrote its output"
    with pytest.raises(R.Mismatch):
        R.ctc_align(R.reference("even", 2600, 3).argmax(1), _vocab("even"), 0, "zyzzy", 2600)
    with pytest.raises(pkg.TtsError):
        eng.align_audio(clip, 16000, "zyzzy")


def test_a_call_inside_an_open_ar_session(pkg, mid_models, voice):
    """tts_aligner_ids between two steps of an open AR session: every request's codes, rows and latents are the bits of the session without the call"""
    from test_ar_session_gpu import req, run_session
    eng = pkg.Engine(0)
    eng.load(ar=mid_models + "/ggml-model.bin")
    eng.load_aligner(R.model("even")[0])
    reqs = [req(9, 2, 1, [6, 9]), req(16, 1, 2, [8], at=2)]
    shape = (4, 2, 16, 12)
    base = run_session(eng, reqs, voice, shape=shape)
    got = []
    clip = R.wave("even", 1290)

    def between(step, rid_of, live):
        if step in (1, 3):
            got.append(eng.aligner_ids([clip], 16000)[0])
    with_call = run_session(eng, reqs, voice, shape=shape, on_step=between)
    assert len(got) == 2 and all(np.array_equal(g, R.reference("even", 1290).argmax(1)) for g in got)
    assert sorted(base) == sorted(with_call)
    for k in base:
        for a, b in zip(base[k], with_call[k]):
            if isinstance(a, (list, tuple)):
                assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
            else:
                assert np.array_equal(a, b)
    eng.close()


def _wav(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
    return raw, np.frombuffer(raw[44:], np.float32)


def test_cli_redacts_the_bracketed_text(pkg, engines, small_models, tmp_path):
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    aligner = R.model("even")[0]

    def run(msg, out, extra=()):
        return subprocess.run([exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--seed", "3", "--codes", "40", "--steps", "3",
                               "--output", str(out)] + list(extra), capture_output=True, text=True, timeout=600)
    plain, bracketed = "hello there world", "[hello] there world"
    r = run(plain, tmp_path / "a.wav")
    assert r.returncode == 0, r.stdout + r.stderr
    raw_a, wav_a = _wav(tmp_path / "a.wav")
    r = run(plain, tmp_path / "b.wav", ["--aligner", aligner])  # no bracket: the bytes of the run without the flag
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "b.wav", "rb").read() == raw_a
    r = run(bracketed, tmp_path / "c.wav", ["--aligner", aligner])
    assert r.returncode == 0, r.stdout + r.stderr
    raw_c, wav_c = _wav(tmp_path / "c.wav")
    eng = engines("even")
    ids = eng.aligner_ids([wav_a], 24000)[0]
    want = R.redact(wav_a, ids, _vocab("even"), 0, bracketed)  # the kept slices of the unredacted run's WAV
    print("cli: %d of %d samples kept; the clip decodes to %d characters" % (len(want), len(wav_a), len(R.ctc_decode(ids, _vocab("even"), 0))))
    assert 0 < len(wav_c) < len(wav_a) and np.array_equal(wav_c, want)
    assert "aligner: %d of %d samples kept" % (len(want), len(wav_a)) in r.stderr
    # a text of which the audio holds nothing (this vocabulary has no y and no z): exit 1, the message, no WAV
    r = run("[zyz]zyzzy", tmp_path / "e.wav", ["--aligner", aligner])
    assert r.returncode == 1 and "the text does not match the audio" in r.stderr and not (tmp_path / "e.wav").exists(), r.stdout + r.stderr
    # refused combinations exit non-zero before a model is loaded
    for extra in (["--split-text", "100"], ["--voice", os.path.join(ROOT, "models", "mol.bin")], ["--devices", "2"], ["--dry-run", "1"]):
        r = run(bracketed, tmp_path / "f.wav", ["--aligner", aligner] + extra)
        assert r.returncode == 1 and "--aligner" in r.stderr and not (tmp_path / "f.wav").exists(), (extra, r.stderr)
