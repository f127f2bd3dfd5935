"""tts_voice_from_audio / tts_audio_mel at engine level (marked gpu): the latents are, bit for bit, what the existing entry points give for the front-end's
mels; the mels lie inside the kernel bounds of tests/afe_cases.py against the float64 chain resample -> window -> mel; a 22 050 Hz input skips the first resampler;
either side works alone; refusals leave the context usable; a call between two steps of an open AR session changes nothing in it; the CLI's --voice-clips /
--save-voice round trip."""
import faulthandler
import os
import shutil
import subprocess

import numpy as np
import pytest

import afe_cases as V
from conftest import ROOT

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_LIMIT = -1, -5, -6


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def enc_files(pkg):
    """the 2-block synthetic encoders (the files tests/test_voice_encoder.py generates under the same names and seeds)"""
    from tortoise_cpp_amd import synth_weights as sw
    root = os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth")
    out = {}
    for key, sub, name, write, seed in (("venc", "venc", "ggml-conditioning-model-small.bin", sw.write_voice_encoder, 52),
                                        ("dcond", "dcond", "ggml-diffusion-conditioning-model-small.bin", sw.write_diffusion_conditioning_encoder, 72)):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        p = os.path.join(root, sub, name)
        if not os.path.exists(p + ".done"):
            write(p, blocks=2, seed=seed)
            open(p + ".done", "w").write("ok")
        out[key] = p
    return out


@pytest.fixture(scope="module")
def eng(pkg, enc_files):
    e = pkg.Engine(0)
    e.load_voice_encoder(enc_files["venc"])
    e.load_diffusion_conditioning_encoder(enc_files["dcond"])
    yield e
    e.close()


def clip(rate, secs, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(int(rate * secs)) / rate
    return (0.3 * np.sin(2 * np.pi * (150 + 35 * seed) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.03 * rs.randn(len(t))).astype(np.float32)


CLIPS = [(16000, 0.9, 1), (44100, 0.4, 2), (22050, 1.0, 3)]  # under full_clips


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def status(pkg, fn, *a, **k):
    with pytest.raises(pkg.TtsError) as e:
        fn(*a, **k)
    return int(str(e.value).rsplit("status ", 1)[1].rstrip(")"))


def test_latents_equal_the_encoders_on_the_front_ends_mels(eng):
    norms = V.mel_norms()
    clips = [clip(*c) for c in CLIPS]
    rates = [c[0] for c in CLIPS]
    kw = dict(mel_norms=norms, full_clips=True)
    v, d = eng.voice_from_audio(clips, rates, **kw)
    m80 = [eng.audio_mel(x, r, 80, **kw) for x, r in zip(clips, rates)]
    m100 = [eng.audio_mel(x, r, 100, **kw) for x, r in zip(clips, rates)]
    assert (_bits(v) == _bits(eng.voice_latent(m80))).all() and (_bits(d) == _bits(eng.diffusion_conditioning_latent(m100))).all()
    assert np.isfinite(v).all() and np.isfinite(d).all() and np.abs(v).max() > 0
    # a three-clip voice is the mean the entry points give; one clip alone is another voice; two calls agree
    v1, d1 = eng.voice_from_audio(clips[:1], rates[:1], **kw)
    assert (_bits(v1) == _bits(eng.voice_latent(m80[:1]))).all() and not (v1 == v).all() and not (d1 == d).all()
    v2, d2 = eng.voice_from_audio(clips, rates, **kw)
    assert (_bits(v2) == _bits(v)).all() and (_bits(d2) == _bits(d)).all()
    # either side alone, bit-equal
    va, none = eng.voice_from_audio(clips, rates, want=(True, False), **kw)
    none2, da = eng.voice_from_audio(clips, rates, want=(False, True), **kw)
    assert none is None and none2 is None and (_bits(va) == _bits(v)).all() and (_bits(da) == _bits(d)).all()


@pytest.mark.parametrize("rate,secs,seed", CLIPS)
def test_audio_mel_inside_the_kernel_bounds_of_the_float64_chain(eng, rate, secs, seed):
    """resample -> window -> mel in float64 (tests/afe_cases.py: chain64, mel_reference); the bound is the mel kernel's, with the resamplers' own bounds carried
    into it as a bound on the mel kernel's input signal"""
    x = clip(rate, secs, seed)
    norms = V.mel_norms()
    a22, e22, a24, e24 = V.chain64(x, rate)
    for bands, sig, err in ((80, a22, e22), (100, a24, e24)):
        got = eng.audio_mel(x, rate, bands, mel_norms=norms, full_clips=True)
        ref, bound = V.mel_reference(sig, 0, len(sig), bands, norms if bands == 80 else None, x_err=err)
        assert got.shape == ref.shape
        bad, r = V.judge(got, ref, bound)
        print("%d Hz -> %d bands: worst |err| / bound %.4f" % (rate, bands, r))
        assert bad == 0, (rate, bands, bad, r)


def test_upstream_windows_and_crop(eng):
    norms = V.mel_norms()
    x = clip(22050, 6.5, 4)  # longer than 132 300 samples: cropped; the 24 kHz side keeps its first 102 400
    m80 = eng.audio_mel(x, 22050, 80, mel_norms=norms)
    m100 = eng.audio_mel(x, 22050, 100)
    assert m80.shape == (80, 517) and m100.shape == (100, 401)
    ref, bound = V.mel_reference(x, 0, V.WIN80, 80, norms)
    assert V.judge(m80, ref, bound)[0] == 0  # a 22 050 Hz input skips the first resampler: the samples are the kernel's input as they are
    # crop_offset: the window from there; clamped so that it ends inside the clip
    last = len(x) - V.WIN80
    at = eng.audio_mel(x, 22050, 80, mel_norms=norms, crop_offset=1000)
    assert (_bits(at) == _bits(eng.audio_mel(x[1000:], 22050, 80, mel_norms=norms))).all()
    assert (_bits(eng.audio_mel(x, 22050, 80, mel_norms=norms, crop_offset=10 ** 9)) == _bits(eng.audio_mel(x[last:], 22050, 80, mel_norms=norms))).all()
    # a short clip is zero-padded to the window: silence behind it is the floor, exactly
    s = eng.audio_mel(x[:30000], 22050, 80)
    assert s.shape == (80, 517) and (_bits(s[:, 125:]) == _bits(V.LOG_FLOOR)).all()
    v, d = eng.voice_from_audio([x, x[:30000]], 22050, mel_norms=norms)
    m100s = eng.audio_mel(x[:30000], 22050, 100)
    assert (_bits(v) == _bits(eng.voice_latent([m80, eng.audio_mel(x[:30000], 22050, 80, mel_norms=norms)]))).all()
    assert (_bits(d) == _bits(eng.diffusion_conditioning_latent([m100, m100s]))).all()


def test_input_at_22050_equals_feeding_the_samples_directly(eng):
    """no resampler runs for the AR side: the mel kernel's own bound holds against the float64 mel of the samples as given"""
    x = clip(22050, 0.7, 5)
    got = eng.audio_mel(x, 22050, 80, full_clips=True)
    ref, bound = V.mel_reference(x, 0, len(x), 80)
    assert got.shape == ref.shape and V.judge(got, ref, bound)[0] == 0


def test_one_side_needs_only_its_encoder(pkg, enc_files):
    x, kw = [clip(16000, 0.5, 6)], dict(full_clips=True)
    e = pkg.Engine(0)
    try:
        assert status(pkg, e.voice_from_audio, x, 16000, **kw) == ERR_STATE  # nothing loaded
        e.load_diffusion_conditioning_encoder(enc_files["dcond"])
        assert status(pkg, e.voice_from_audio, x, 16000, **kw) == ERR_STATE  # the AR side's encoder is missing
        none, d = e.voice_from_audio(x, 16000, want=(False, True), **kw)
        assert none is None and np.isfinite(d).all()
    finally:
        e.close()
    e = pkg.Engine(0)
    try:
        e.load_voice_encoder(enc_files["venc"])
        assert status(pkg, e.voice_from_audio, x, 16000, want=(False, True), **kw) == ERR_STATE
        v, none = e.voice_from_audio(x, 16000, want=(True, False), **kw)
        assert none is None and np.isfinite(v).all()
        assert e.audio_mel(x[0], 16000, 100, **kw).shape[0] == 100  # the mel needs no encoder
    finally:
        e.close()


def test_refusals_leave_the_context_usable(eng, pkg):
    kw = dict(full_clips=True)
    good = [clip(16000, 0.5, 7)]
    want = eng.voice_from_audio(good, 16000, **kw)

    def still_fine():
        got = eng.voice_from_audio(good, 16000, **kw)
        assert (_bits(got[0]) == _bits(want[0])).all() and (_bits(got[1]) == _bits(want[1])).all()

    assert status(pkg, eng.voice_from_audio, [], [], **kw) == ERR_ARG  # n_clips 0
    still_fine()
    for rate in (0, -22050):
        assert status(pkg, eng.voice_from_audio, good, rate, **kw) == ERR_ARG
    still_fine()
    assert status(pkg, eng.voice_from_audio, [clip(22050, 512 / 22050.0, 8)], 22050, **kw) == ERR_ARG  # 512 samples at 22 050 Hz under full_clips
    assert status(pkg, eng.voice_from_audio, [clip(44100, 1000 / 44100.0, 8)], 44100, **kw) == ERR_ARG  # 1000 samples -> 500 after resampling
    still_fine()
    bad = good[0].copy()
    bad[len(bad) // 2] = np.nan
    assert status(pkg, eng.voice_from_audio, [good[0], bad], 16000, **kw) == ERR_ARG
    assert status(pkg, eng.audio_mel, bad, 16000, 80, **kw) == ERR_ARG
    still_fine()
    assert status(pkg, eng.voice_from_audio, good, 22051, **kw) == ERR_LIMIT  # a 22050 x 22065 tap table
    assert status(pkg, eng.audio_mel, good[0], 16000, 64, **kw) == ERR_ARG
    assert status(pkg, eng.audio_mel, good[0], 16000, 80, crop_offset=-1) == ERR_ARG
    o, keep = eng._audio_opts(None, 0, True, struct_size=8)
    a = good[0]
    n, r = np.array([len(a)], np.int64), np.array([16000], np.int32)
    out = np.empty(1024, np.float32)
    assert eng.L.tts_voice_from_audio(eng.h, a.ctypes.data, n.ctypes.data, r.ctypes.data, 1, pkg.C.addressof(o), out.ctypes.data, None) == ERR_ARG
    assert eng.L.tts_voice_from_audio(eng.h, a.ctypes.data, n.ctypes.data, r.ctypes.data, 1, None, None, None) == ERR_ARG  # both outputs NULL
    still_fine()


def test_legal_inside_an_open_ar_session(pkg, small_models, enc_files, voice):
    """One request is decoding; voice_from_audio runs between two session steps; a second request is admitted under the returned voice. The first request's codes are
    those of the run without the call, the second's those of tts_autoregressive alone with that voice."""
    from test_ar_session_gpu import alone, prompt, req
    e = pkg.Engine(0)
    try:
        e.load(ar=os.path.join(small_models, "ggml-model.bin"))
        e.load_voice_encoder(enc_files["venc"])
        e.load_diffusion_conditioning_encoder(enc_files["dcond"])
        x = [clip(16000, 0.6, 9)]
        new_voice, _ = e.voice_from_audio(x, 16000, full_clips=True)
        r1, r2 = req(12, 2, 21, [14, 14]), req(9, 1, 22, [10])
        want1 = alone(e, r1, voice, want_latents=False, max_steps=20)
        want2 = alone(e, r2, new_voice, want_latents=False, max_steps=20)

        def session(call):
            e.ar_session_open(4, 2, 16, 20, mask_stop=True, retire=True)
            a = e.ar_session_admit(r1["tokens"], voice, 2, r1["seed"], r1["stop_at"])
            for _ in range(3):
                e.ar_session_step()
            v = e.voice_from_audio(x, 16000, full_clips=True)[0] if call else new_voice
            e.ar_session_step()
            b = e.ar_session_admit(r2["tokens"], v, 1, r2["seed"], r2["stop_at"])
            out, steps = {}, 0
            while len(out) < 2:
                assert steps < 60
                e.ar_session_step()
                steps += 1
                for rid in e.ar_session_finished():
                    out[rid] = e.ar_session_collect(rid, want_latents=False)
            e.ar_session_close()
            return out[a], out[b], v

        with_call, without = session(True), session(False)
        assert (_bits(with_call[2]) == _bits(new_voice)).all()
        for k, want in ((0, want1), (1, want2)):
            assert (with_call[k][0] == without[k][0]).all() and (with_call[k][0] == want[0]).all(), k
            assert (with_call[k][1] == want[1]).all()
    finally:
        e.close()


def test_cli_voice_clips_round_trip(pkg, eng, enc_files, small_models, tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    x, rate = clip(16000, 0.8, 10), 16000
    wav = str(tmp_path / "x.wav")
    assert pkg.write_wav(wav, x, rate) == 0
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    base = [exe, "--models", str(d), "--message", "this is a test message.", "--seed", "0", "--codes", "12", "--steps", "3"]
    p = str(tmp_path / "p")
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    r = subprocess.run(base + ["--voice-clips", wav, "--conditioning-model", enc_files["venc"], "--diffusion-conditioning-model", enc_files["dcond"],
                               "--save-voice", p, "--output", str(a)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    y, got_rate = pkg.read_wav(wav)
    assert got_rate == rate and (y == x).all()
    v, dl = eng.voice_from_audio([y], rate)  # the CLI's call: upstream's windows, no norms
    assert open(p + ".bin", "rb").read() == v.tobytes() and open(p + ".diffusion.bin", "rb").read() == dl.tobytes()
    r = subprocess.run(base + ["--voice", p + ".bin", "--diffusion-latent", p + ".diffusion.bin", "--output", str(b)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert a.read_bytes() == b.read_bytes() and len(a.read_bytes()) > 1000
    # usage errors, before a model is loaded
    for extra, text in ((["--voice-clips", wav], "--conditioning-model"),
                        (["--voice-clips", wav, "--conditioning-model", enc_files["venc"]], "--diffusion-conditioning-model"),
                        (["--save-voice", p], "--voice-clips"),
                        (["--voice-clips", wav, "--conditioning-model", enc_files["venc"], "--diffusion-conditioning-model", enc_files["dcond"], "--dry-run", "1"], "--dry-run")):
        r = subprocess.run(base + extra + ["--output", str(tmp_path / "bad.wav")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and text in r.stderr, (extra, r.stderr)
