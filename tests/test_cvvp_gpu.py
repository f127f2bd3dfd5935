"""CVVP re-ranking at engine level (marked gpu): tts_load_cvvp / tts_cvvp_voice / tts_cvvp_voice_audio / tts_cvvp_score against the float64 reference
tests/cvvp_ref.py: NumpyCVVP (pinned on the CPU against an independent torch.nn.functional restatement and against TorchCLVP's layers: tests/test_cvvp_cpu.py).

Gate on every score: the project's 1e-3 absolute, the gate tests/test_clvp.py applies to the same arithmetic class (fp16-operand GEMMs, f32 accumulation, against
float64). A latent has no gate of its own in the issue; it is held to the same one through the only thing it is for: the scores it gives with the REFERENCE's
latents of the other side stay within 1e-3. The measured distances are printed (DESIGN.md "What pins CVVP" records them)."""
import faulthandler
import os
import shutil
import subprocess

import numpy as np
import pytest

import cvvp_ref as CR
from conftest import ROOT

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_FORMAT, ERR_STATE, ERR_LIMIT = -1, -3, -5, -6
GATE = 1e-3


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def status(pkg, fn, *a, **k):
    with pytest.raises(pkg.TtsError) as e:
        fn(*a, **k)
    return int(str(e.value).rsplit("status ", 1)[1].rstrip(")")), str(e.value)


@pytest.fixture(scope="module")
def files(pkg):
    return {"small": CR.synth_file(2), "full": CR.synth_file(8)}


@pytest.fixture(scope="module")
def eng(pkg, files):
    e = pkg.Engine(0)
    e.load_cvvp(files["small"])
    yield e
    e.close()


@pytest.fixture(scope="module")
def small_case(files):
    """the depth-2 inputs and the reference's latents, computed once and left unchanged"""
    mels, codes = CR.case_inputs()
    ref = CR.NumpyCVVP(files["small"])
    return {"mels": mels, "codes": codes, "ref": ref, "v": ref.voice(mels), "z": ref.speech(codes)}


def _check(ref, v_ref, z_ref, v_got, s_got_of, codes, what):
    """v_got: the engine's voice latents; s_got_of(latents) -> the engine's scores. Every clip alone and all clips together."""
    temp = float(np.exp(ref.w["temperature"].reshape(())[()]))
    lat_l2 = np.linalg.norm(v_got.astype(np.float64) - v_ref, axis=1).max()
    lat_score = np.abs((v_got.astype(np.float64) - v_ref) @ z_ref.T * temp).max()  # the engine's voice latents scored against the reference's speech latents
    worst, ranked = 0.0, 0
    for k in list(range(len(v_ref))) + [None]:
        sel = slice(None) if k is None else slice(k, k + 1)
        want = ref.score(v_ref[sel], codes, z_ref)
        got = s_got_of(v_got[sel])
        worst = max(worst, float(np.abs(got - want).max()))
        order = np.argsort(-want)
        if len(want) > 1 and want[order[0]] - want[order[1]] > 2 * GATE:  # twice the gate: the engine's arg-max is the reference's
            ranked += 1
            assert int(np.argmax(got)) == int(order[0]), (what, k, got, want)
    print("CVVP %s: max abs score error %.2e (gate %.0e); voice latents: L2 distance %.2e, their effect on a score %.2e; ranking checked in %d cases"
          % (what, worst, GATE, lat_l2, lat_score, ranked))
    assert worst < GATE and lat_score < GATE
    return ranked


def test_engine_vs_reference_small(eng, small_case):
    """clips of 4, 5, 7, 8, 130 and 517 frames (odd and even lengths on both strided convolutions, R = 1: one row of GroupNorm) x code lengths 1, 7, 13, 57, 200, 301
    (below, at and across the 128-row GEMM tile and the 256-row attention chunk), depth 2"""
    c = small_case
    v = eng.cvvp_voice(c["mels"])
    assert v.shape == (6, 512) and eng.cvvp_latent_dim == 512
    assert np.allclose(np.linalg.norm(v.astype(np.float64), axis=1), 1.0, atol=1e-6)
    ranked = _check(c["ref"], c["v"], c["z"], v, lambda lat: eng.cvvp_score(lat, c["codes"]), c["codes"], "depth 2")
    assert ranked >= 1  # tests/test_cvvp_cpu.py: test_gpu_cases_have_a_ranking_gap
    # two calls give equal bits
    assert (_bits(eng.cvvp_voice(c["mels"])) == _bits(v)).all()
    s = eng.cvvp_score(v, c["codes"])
    assert (_bits(eng.cvvp_score(v, c["codes"])) == _bits(s)).all()


def test_engine_vs_reference_upstream_size(pkg, files):
    """depth 8 + 8 at dim 512, upstream's size: three candidates of 60 / 187 / 200 codes against one 517-frame clip"""
    mels, codes = CR.case_inputs(frames=(517,), lens=CR.FULL_LENS, seed=CR.INPUT_SEED + 1)
    ref = CR.NumpyCVVP(files["full"])
    v_ref, z_ref = ref.voice(mels), ref.speech(codes)
    e = pkg.Engine(0)
    try:
        e.load_cvvp(files["full"])
        v = e.cvvp_voice(mels)
        _check(ref, v_ref, z_ref, v, lambda lat: e.cvvp_score(lat, codes), codes, "depth 8")
        assert (_bits(e.cvvp_score(v, codes)) == _bits(e.cvvp_score(v, codes))).all()
    finally:
        e.close()


def test_alone_and_in_a_batch(eng, small_case):
    """a candidate's score does not depend on who shares the batch, a clip's latent not on the other clips of the call (1e-6, as tests/test_clvp.py asks)"""
    c = small_case
    v = eng.cvvp_voice(c["mels"])
    s = eng.cvvp_score(v[4:5], c["codes"])
    for i in (0, 3, 5):
        solo = eng.cvvp_score(v[4:5], [c["codes"][i]])
        print("candidate %d alone vs in the batch: |diff| %.1e, bits equal: %s" % (i, abs(float(solo[0]) - float(s[i])), bool(_bits(solo)[0] == _bits(s)[i])))
        assert abs(float(solo[0]) - float(s[i])) < 1e-6
    for k in (0, 2, 5):
        one = eng.cvvp_voice([c["mels"][k]])
        print("clip %d alone vs among others: max |diff| %.1e, bits equal: %s" % (k, np.abs(one[0] - v[k]).max(), bool((_bits(one[0]) == _bits(v[k])).all())))
        assert np.abs(one[0] - v[k]).max() < 1e-6
    # two clips: the mean of the two one-clip calls
    two = eng.cvvp_score(v[[1, 5]], c["codes"])
    mean = (eng.cvvp_score(v[1:2], c["codes"]).astype(np.float64) + eng.cvvp_score(v[5:6], c["codes"])) / 2
    assert np.abs(two - mean).max() < 1e-6


def _clip(rate, secs, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(int(rate * secs)) / rate
    return (0.3 * np.sin(2 * np.pi * (150 + 35 * seed) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.03 * rs.randn(len(t))).astype(np.float32)


def test_voice_audio_equals_voice_of_the_front_ends_mel(eng):
    """the mel goes from the front-end's kernel straight into the stem's input buffer: bit for bit what tts_audio_mel hands back and tts_cvvp_voice takes"""
    import afe_cases as V
    norms = V.mel_norms()
    short, long_ = _clip(16000, 0.5, 1), _clip(44100, 7.0, 2)  # zero-padded to the window; longer than it: cropped from crop_offset
    for clips, rates, kw in (([short], [16000], {}), ([long_], [44100], dict(crop_offset=9000, mel_norms=norms)), ([short, long_], [16000, 44100], dict(crop_offset=9000, mel_norms=norms))):
        mels = [eng.audio_mel(x, r, 80, **kw) for x, r in zip(clips, rates)]
        assert all(m.shape == (80, 517) for m in mels)
        got = eng.cvvp_voice_audio(clips, rates, **kw)
        assert got.shape == (len(clips), 512) and (_bits(got) == _bits(eng.cvvp_voice(mels))).all()
    assert not (eng.cvvp_voice_audio([long_], 44100, crop_offset=9000) == eng.cvvp_voice_audio([long_], 44100)).all()  # the offset is used


def test_errors(pkg, eng, files, small_case, small_models):
    c = small_case
    mels, codes = c["mels"][:2], c["codes"][:3]
    v0 = eng.cvvp_voice(mels)
    s0 = eng.cvvp_score(v0, codes)

    def still_fine():
        v = eng.cvvp_voice(mels)
        assert (_bits(v) == _bits(v0)).all() and (_bits(eng.cvvp_score(v, codes)) == _bits(s0)).all()

    e = pkg.Engine(0)
    try:
        assert e.L.tts_cvvp_latent_dim(e.h) < 0
        for fn, args in ((e.cvvp_score, (v0, codes)),):
            st, msg = status(pkg, fn, *args)
            assert st == ERR_STATE and "tts_load_cvvp not called" in msg
        lat = np.empty((1, 512), np.float32)
        fr = np.array([mels[1].shape[1]], np.int32)
        assert e.L.tts_cvvp_voice(e.h, mels[1].ctypes.data, fr.ctypes.data, 1, lat.ctypes.data) == ERR_STATE
        n, r = np.array([8000], np.int64), np.array([16000], np.int32)
        a = _clip(16000, 0.5, 3)
        assert e.L.tts_cvvp_voice_audio(e.h, a.ctypes.data, n.ctypes.data, r.ctypes.data, 1, None, lat.ctypes.data) == ERR_STATE
        from tortoise_cpp_amd import synth_weights as sw
        clvp = os.path.join(os.path.dirname(files["small"]), "ggml-clvp-model-for-cvvp-test.bin")
        if not os.path.exists(clvp + ".done"):
            sw.write_clvp(clvp, depth=1, seed=5)
            open(clvp + ".done", "w").write("ok")
        for p in (clvp, os.path.join(small_models, "ggml-vocoder-model.bin")):
            st, msg = status(pkg, e.load_cvvp, p)
            assert st == ERR_FORMAT and "not a CVVP model file" in msg
    finally:
        e.close()

    L, h = eng.L, eng.h
    out, sc = np.empty((2, 512), np.float32), np.empty(3, np.float32)
    mel = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in mels]))
    frames = np.array([m.shape[1] for m in mels], np.int32)
    cl = np.array([len(x) for x in codes], np.int32)
    cd = np.zeros((3, int(cl.max())), np.int32)
    for i, x in enumerate(codes):
        cd[i, :len(x)] = x
    P = lambda a: a.ctypes.data
    # null pointers
    assert L.tts_cvvp_voice(h, None, P(frames), 2, P(out)) == ERR_ARG and L.tts_cvvp_voice(h, P(mel), None, 2, P(out)) == ERR_ARG
    assert L.tts_cvvp_voice(h, P(mel), P(frames), 2, None) == ERR_ARG
    assert L.tts_cvvp_score(h, None, 2, P(cd), P(cl), 3, cd.shape[1], P(sc)) == ERR_ARG and L.tts_cvvp_score(h, P(v0), 2, None, P(cl), 3, cd.shape[1], P(sc)) == ERR_ARG
    assert L.tts_cvvp_score(h, P(v0), 2, P(cd), None, 3, cd.shape[1], P(sc)) == ERR_ARG and L.tts_cvvp_score(h, P(v0), 2, P(cd), P(cl), 3, cd.shape[1], None) == ERR_ARG
    # n_clips < 1, frames < 1
    assert L.tts_cvvp_voice(h, P(mel), P(frames), 0, P(out)) == ERR_ARG and L.tts_cvvp_score(h, P(v0), 0, P(cd), P(cl), 3, cd.shape[1], P(sc)) == ERR_ARG
    assert L.tts_cvvp_voice(h, P(mel), P(np.array([4, 0], np.int32)), 2, P(out)) == ERR_ARG
    still_fine()
    # codes and lengths
    st, msg = status(pkg, eng.cvvp_score, v0, [np.array([5, 8192], np.int32)])
    assert st == ERR_ARG and "out of range" in msg
    st, msg = status(pkg, eng.cvvp_score, v0, [np.array([-1], np.int32)])
    assert st == ERR_ARG and "out of range" in msg
    for bad_len in (0, cd.shape[1] + 1):
        assert L.tts_cvvp_score(h, P(v0), 2, P(cd), P(np.array([cl[0], bad_len, cl[2]], np.int32)), 3, cd.shape[1], P(sc)) == ERR_ARG
    # non-finite values
    bad = [mels[0], mels[1].copy()]
    bad[1][3, 2] = np.inf
    st, msg = status(pkg, eng.cvvp_voice, bad)
    assert st == ERR_ARG and "non-finite" in msg
    vb = v0.copy()
    vb[1, 7] = np.nan
    st, msg = status(pkg, eng.cvvp_score, vb, codes)
    assert st == ERR_ARG and "non-finite" in msg
    still_fine()
    # whole clips are out of scope; the frame limit
    st, msg = status(pkg, eng.cvvp_voice_audio, [_clip(16000, 0.5, 3)], 16000, full_clips=True)
    assert st == ERR_ARG and "full_clips" in msg
    st, msg = status(pkg, eng.cvvp_voice, [np.zeros((80, 16385), np.float32)])
    assert st == ERR_LIMIT and "16384" in msg
    nan_clip = _clip(16000, 0.5, 3)
    nan_clip[100] = np.nan
    assert status(pkg, eng.cvvp_voice_audio, [nan_clip], 16000)[0] == ERR_ARG
    still_fine()


def test_rerank_blend(pkg, eng, small_case):
    """Engine.rerank = clvp * (1 - a) + cvvp * a of the two score calls; the side whose weight is 0 needs no model"""
    from tortoise_cpp_amd import synth_weights as sw
    c = small_case
    clvp = os.path.join(os.path.dirname(CR.synth_file(2)), "ggml-clvp-model-depth2.bin")
    if not os.path.exists(clvp + ".done"):
        sw.write_clvp(clvp, depth=2, seed=101)
        open(clvp + ".done", "w").write("ok")
    text = np.random.RandomState(2).randint(0, 256, 30).astype(np.int32)
    codes = c["codes"][1:5]
    e = pkg.Engine(0)
    try:
        e.load_clvp(clvp)
        s_clvp = e.clvp_score(text, codes)
        assert (_bits(e.rerank(text, codes)) == _bits(s_clvp)).all()  # amount 0: no CVVP file loaded, no voice latents
        assert (_bits(e.rerank(text, codes, None, 0.0)) == _bits(s_clvp)).all()
        assert status(pkg, e.rerank, text, codes, np.zeros((1, 512), np.float32), 0.5)[0] == ERR_STATE
        e.load_cvvp(CR.synth_file(2))
        v = e.cvvp_voice(c["mels"][4:])
        s_cvvp = e.cvvp_score(v, codes)
        assert (_bits(e.rerank(text, codes, v, 1.0)) == _bits(s_cvvp)).all()
        half = e.rerank(text, codes, v, 0.5)
        assert (_bits(half) == _bits(s_clvp * np.float32(0.5) + s_cvvp * np.float32(0.5))).all()
        assert np.abs(half - (s_clvp.astype(np.float64) + s_cvvp) / 2).max() < 1e-7
    finally:
        e.close()
    v = eng.cvvp_voice(c["mels"][4:])
    assert (_bits(eng.rerank(None, codes, v, 1.0)) == _bits(eng.cvvp_score(v, codes))).all()  # amount 1: no CLVP file loaded


def test_legal_inside_an_open_ar_session(pkg, files, small_models, small_case, voice):
    """a request is decoding; every CVVP call runs between two session steps; the request's codes are those of the run without the calls"""
    from test_ar_session_gpu import alone, req
    c = small_case
    e = pkg.Engine(0)
    try:
        e.load(ar=os.path.join(small_models, "ggml-model.bin"))
        e.load_cvvp(files["small"])
        x = _clip(16000, 0.5, 4)
        v_before = e.cvvp_voice(c["mels"][:3])
        a_before = e.cvvp_voice_audio([x], 16000)
        s_before = e.cvvp_score(v_before, c["codes"][:4])
        r1 = req(12, 2, 21, [14, 14])
        want = alone(e, r1, voice, want_latents=False, max_steps=20)

        def session(call):
            e.ar_session_open(4, 2, 16, 20, mask_stop=True, retire=True)
            a = e.ar_session_admit(r1["tokens"], voice, 2, r1["seed"], r1["stop_at"])
            for _ in range(3):
                e.ar_session_step()
            got = None
            if call:
                got = (e.cvvp_voice(c["mels"][:3]), e.cvvp_voice_audio([x], 16000), e.cvvp_score(v_before, c["codes"][:4]))
                e.load_cvvp(files["small"])  # the load too
            out, steps = {}, 0
            while len(out) < 1:
                assert steps < 60
                e.ar_session_step()
                steps += 1
                for rid in e.ar_session_finished():
                    out[rid] = e.ar_session_collect(rid, want_latents=False)
            e.ar_session_close()
            return out[a], got

        with_call, without = session(True), session(False)
        for got, before in zip(with_call[1], (v_before, a_before, s_before)):
            assert (_bits(got) == _bits(before)).all()
        assert (with_call[0][0] == without[0][0]).all() and (with_call[0][0] == want[0]).all() and (with_call[0][1] == want[1]).all()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the CLI: tortoise --cvvp FILE [--cvvp-amount x]
# ------------------------------------------------------------------------------------------------------------------------------
MSG = "this is a test message."


@pytest.fixture(scope="module")
def cli_files(pkg, files, small_models, tmp_path_factory):
    """the small models, the 2-block conditioning encoders (the files tests/test_voice_encoder.py generates under the same names and seeds), a depth-2 CLVP file
    and two clips as float32 WAV files"""
    from tortoise_cpp_amd import synth_weights as sw
    root = os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth")
    out = {"cvvp": files["small"], "exe": os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")}
    for key, sub, name, write, kw in (("venc", "venc", "ggml-conditioning-model-small.bin", sw.write_voice_encoder, dict(blocks=2, seed=52)),
                                      ("dcond", "dcond", "ggml-diffusion-conditioning-model-small.bin", sw.write_diffusion_conditioning_encoder, dict(blocks=2, seed=72)),
                                      ("clvp", "cvvp", "ggml-clvp-model-depth2.bin", sw.write_clvp, dict(depth=2, seed=101))):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        p = os.path.join(root, sub, name)
        if not os.path.exists(p + ".done"):
            write(p, **kw)
            open(p + ".done", "w").write("ok")
        out[key] = p
    tmp = tmp_path_factory.mktemp("cvvp_cli")
    d = tmp / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    out["models"] = str(d)
    out["clips"] = [(_clip(16000, 0.8, 10), 16000), (_clip(22050, 0.6, 11), 22050)]
    out["wavs"] = []
    for k, (x, rate) in enumerate(out["clips"]):
        out["wavs"].append(str(tmp / ("clip%d.wav" % k)))
        assert pkg.write_wav(out["wavs"][-1], x, rate) == 0
    out["encoders"] = ["--conditioning-model", out["venc"], "--diffusion-conditioning-model", out["dcond"]]
    out["base"] = [out["exe"], "--models", out["models"], "--seed", "0", "--codes", "12", "--steps", "3", "--candidates", "4"] + out["encoders"]
    return out


def _scores(stdout, label):
    lines = [l for l in stdout.splitlines() if l.startswith(label)]
    assert len(lines) == 1, (label, stdout)
    return np.array([float(t) for t in lines[0][len(label):].split()])


def _run(cmd, timeout=300):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)


def test_cli_scores_and_blended_argmax(pkg, cli_files, tmp_path):
    """--clvp F --cvvp G --voice-clips a.wav: the printed scores are the engine's, the kept candidate is the blended arg-max; --cvvp-amount 0 is the run without --cvvp"""
    f = cli_files
    one = f["base"] + ["--message", MSG, "--voice-clips", f["wavs"][0], "--clvp", f["clvp"]]
    r = _run(one + ["--cvvp", f["cvvp"], "--output", str(tmp_path / "a.wav")])
    assert r.returncode == 0, r.stdout + r.stderr
    clvp_cli, cvvp_cli = _scores(r.stdout, "clvp scores:"), _scores(r.stdout, "cvvp scores:")
    kept = [l for l in r.stdout.splitlines() if l.startswith("rerank: candidate ")]
    assert len(kept) == 1 and "cvvp amount 0.5" in kept[0], r.stdout
    e = pkg.Engine(0)
    try:
        x, rate = f["clips"][0]
        e.load_voice_encoder(f["venc"])
        e.load_cvvp(f["cvvp"])
        e.load_clvp(f["clvp"])
        voice, _ = e.voice_from_audio([x], rate, want=(True, False))
        lat = e.cvvp_voice_audio([x], rate)
        e.tokenizer_load(os.path.join(f["models"], "tokenizer.json"))
        tokens = e.tokenize(MSG)
        e.load(ar=os.path.join(f["models"], "ggml-model.bin"))
        e.seed(0)
        codes, rows, _, _ = e.autoregressive(tokens, voice, 4, 12, mask_stop=True, retire=True, want_latents=False)
        cl = [codes[c, 1:1 + rows[c]] for c in range(4)]
        s_clvp, s_cvvp = e.clvp_score(tokens, cl), e.cvvp_score(lat, cl)
        blend = e.rerank(tokens, cl, lat, 0.5)
    finally:
        e.close()
    assert clvp_cli.shape == (4,) and cvvp_cli.shape == (4,)
    assert np.abs(clvp_cli - s_clvp).max() < 6e-6 and np.abs(cvvp_cli - s_cvvp).max() < 6e-6  # printed with five decimals
    assert int(kept[0].split()[2]) == int(np.argmax(blend))
    # --cvvp-amount 0: CVVP is neither loaded nor evaluated (the file need not exist) and the WAV is the one the command writes without --cvvp
    r0 = _run(one + ["--output", str(tmp_path / "b.wav")])
    r1 = _run(one + ["--cvvp", str(tmp_path / "no-such-file.bin"), "--cvvp-amount", "0", "--output", str(tmp_path / "c.wav")])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert "cvvp scores" not in r1.stdout and r0.stdout == r1.stdout
    assert (tmp_path / "b.wav").read_bytes() == (tmp_path / "c.wav").read_bytes() and len((tmp_path / "b.wav").read_bytes()) > 1000


def test_cli_every_chunk_against_its_own_voice(pkg, cli_files, tmp_path):
    """several voices, --cvvp alone (amount 1): chunk c's printed scores are the engine's against the clips of chunk c's voice"""
    f = cli_files
    msg = "0|the first speaker says this.\n1|and the second one answers."
    r = _run(f["base"] + ["--message", msg, "--voice-clips", f["wavs"][0], "--voice-clips", f["wavs"][0] + "," + f["wavs"][1], "--cvvp", f["cvvp"],
                          "--output", str(tmp_path / "d.wav")])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clvp scores" not in r.stdout
    got = [_scores(r.stdout, "chunk %d cvvp scores:" % c) for c in range(2)]
    e = pkg.Engine(0)
    try:
        e.load_voice_encoder(f["venc"])
        e.load_cvvp(f["cvvp"])
        sets = [[f["clips"][0]], [f["clips"][0], f["clips"][1]]]
        voices = np.stack([e.voice_from_audio([x for x, _ in s], [r_ for _, r_ in s], want=(True, False))[0] for s in sets])
        lats = [e.cvvp_voice_audio([x for x, _ in s], [r_ for _, r_ in s]) for s in sets]
        assert lats[1].shape == (2, 512)
        e.tokenizer_load(os.path.join(f["models"], "tokenizer.json"))
        turns = e.split_turns(msg, 2)
        assert [v for _, v in turns] == [0, 1]
        e.load(ar=os.path.join(f["models"], "ggml-model.bin"))
        e.seed(0)
        codes, rows, _, _ = e.autoregressive_multi([e.tokenize(t) for t, _ in turns], n_cand=4, max_steps=12, mask_stop=True, retire=True, want_latents=False,
                                                   voices=voices, voice_of_prompt=[0, 1])
        for c in range(2):
            want = e.cvvp_score(lats[c], [codes[c][k, 1:1 + rows[c][k]] for k in range(4)])
            assert np.abs(got[c] - want).max() < 6e-6, (c, got[c], want)
            assert ("chunk %d: voice %d" % (c, c)) in r.stdout and ("candidate %d kept" % int(np.argmax(want))) in [l for l in r.stdout.splitlines() if l.startswith("chunk %d: voice" % c)][0]
    finally:
        e.close()


def test_cli_usage_errors(cli_files, tmp_path):
    """exit 1 before any model is loaded: the models directory does not exist, and neither do the files named"""
    f = cli_files
    clips = ["--voice-clips", f["wavs"][0], "--conditioning-model", "c.bin", "--diffusion-conditioning-model", "d.bin"]
    for extra, text in ((["--cvvp", "g.bin", "--voice", "latent.bin"], "holds no audio"),
                        (["--cvvp", "g.bin"], "holds no audio"),  # the default voice is a latent file
                        (["--cvvp", "g.bin", "--voice", "latent.bin", "--diffusion-latent", "l.bin"] + clips, "holds no audio"),
                        (["--cvvp", "g.bin", "--devices", "2"] + clips, "--devices > 1"),
                        (["--cvvp", "g.bin", "--decoder", "hifigan", "--stream"] + clips[:4], "--cvvp"),
                        (["--cvvp", "g.bin", "--cvvp-amount", "1.5"] + clips, "0 .. 1"),
                        (["--cvvp", "g.bin", "--cvvp-amount", "-0.1", "--clvp", "f.bin"] + clips, "0 .. 1"),
                        (["--cvvp", "g.bin", "--cvvp-amount", "0.5"] + clips, "needs --clvp"),
                        (["--cvvp-amount", "0.5"] + clips, "belongs to --cvvp")):
        r = _run([f["exe"], "--models", str(tmp_path / "nowhere"), "--message", MSG, "--output", str(tmp_path / "bad.wav")] + extra, timeout=60)
        assert r.returncode == 1 and text in r.stderr and "model_load" not in r.stderr and "Unable" not in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "bad.wav").exists()
