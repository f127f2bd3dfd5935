"""GPU: the DVAE encoder through the C ABI (tts_load_dvae / tts_dvae_codes / tts_dvae_codes_audio / tts_ar_latents_for_codes, csrc/dvae.h) against the float64
restatement tests/dvae_ref.py on synthetic weights (mid-size: hidden 64 / 128, 256 tokens; one full-size clip of about 2 s), its bit-level properties, the audio
entry, its error statuses, an open AR session beside it, and the re-voicing call against the manual sequence. Unpinned against upstream (no source or weights
offline); pinned between independent implementations: see tests/test_dvae_cpu.py.

Gate: 1e-3 absolute on z (dvae_ref.GATE), the project's gate for f32 stages. The codes must equal float64's on every row whose float64 gap exceeds
2 (2 |dz|_2 max_j |E_j|_2 + bound), dz the measured difference of that row; at most 2 % of the rows may fall under that margin. The measured figures are in
profiles/dvae.txt."""
import ctypes as C
import os

import numpy as np
import pytest

import dvae_ref as R

pytestmark = pytest.mark.gpu
ROOT = R.ROOT
ARG, HIP, STATE, LIMIT = -1, -4, -5, -6


@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(name):
        if name not in made:
            e = pkg.Engine(0)
            e.load_dvae(R.model(name)[0])
            made[name] = e
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _check(name, frames, codes, z, seed=0):
    ref = R.reference(name, frames, seed)
    E = R.model(name)[1]["dvae.codebook.embed"]
    assert z.shape == ref["z"].shape and codes.shape == (ref["z"].shape[0],)
    err = float(np.abs(z - ref["z"]).max())
    fails, out = R.judge_end_to_end(codes, z, ref["z"], ref["s"], ref["bound"], E)
    print("dvae %s T = %d: %d codes, z max abs distance from float64 %.2e (gate %.0e, z up to %.1f), %d codes differ from float64's, %.4f of the rows under the margin"
          % (name, frames, len(codes), err, R.GATE, np.abs(ref["z"]).max(), int((codes != ref["codes"]).sum()), out))
    assert np.isfinite(z).all() and err <= R.GATE
    assert not fails, fails[:3]
    assert out <= R.MAX_UNDECIDED


@pytest.mark.parametrize("frames", R.MID_FRAMES)
def test_engine_vs_float64(engines, frames):
    eng = engines("mid")
    codes, z = eng.dvae_codes([R.mel(frames)], z=True)
    _check("mid", frames, codes[0], z[0])
    assert np.array_equal(eng.dvae_codes([R.mel(frames)])[0], codes[0])  # without z: the same codes
    assert eng.dvae_tokens == 256 and eng.L.tts_dvae_dim(eng.h) == 64


def test_full_size_clip_vs_float64(engines):
    eng = engines("full")
    codes, z = eng.dvae_codes([R.mel(R.FULL_FRAMES)], z=True)
    _check("full", R.FULL_FRAMES, codes[0], z[0])
    assert eng.dvae_tokens == 8192 and len(codes[0]) == eng.dvae_rows(R.FULL_FRAMES) == 44


def test_ragged_batch_alone_twice_and_reversed(engines):
    eng = engines("mid")
    mels = [R.mel(f, 1 + i) for i, f in enumerate(R.RAGGED)]
    ca, za = eng.dvae_codes(mels, z=True)
    cb, zb = eng.dvae_codes(mels, z=True)
    cr, zr = eng.dvae_codes(mels[::-1], z=True)
    for i, m in enumerate(mels):
        assert np.array_equal(za[i], zb[i]) and np.array_equal(ca[i], cb[i]), "two calls differ"
        assert np.array_equal(za[i], zr[len(mels) - 1 - i]) and np.array_equal(ca[i], cr[len(mels) - 1 - i]), "the order of the clips matters"
        c1, z1 = eng.dvae_codes([m], z=True)
        assert np.array_equal(z1[0], za[i]) and np.array_equal(c1[0], ca[i]), "clip %d differs from itself alone" % i
        _check("mid", R.RAGGED[i], ca[i], za[i], 1 + i)


def _clip(n, seed, rate=22050):
    r = np.random.default_rng(seed)
    i = np.arange(n)
    return (0.2 * r.standard_normal(n) + 0.3 * np.sin(i * 2 * np.pi * 220.0 / rate) + 0.1 * np.sin(i * 2 * np.pi * 1300.0 / rate)).astype(np.float32)


def test_audio_entry_is_the_mel_entry_bit_for_bit(engines):
    eng = engines("mid")
    norms = (1.0 + 0.1 * np.arange(80)).astype(np.float32)
    clips, rates = [_clip(9000, 1), _clip(5000, 2, 16000), _clip(2049, 3)], [22050, 16000, 22050]
    mels = [eng.audio_mel(c, r, 80, norms, full_clips=True) for c, r in zip(clips, rates)]
    want_c, want_z = eng.dvae_codes(mels, z=True)
    got_c, got_z = eng.dvae_codes_audio(clips, rates, norms, z=True)
    for i in range(3):
        assert np.array_equal(got_c[i], want_c[i]) and np.array_equal(got_z[i], want_z[i]), "clip %d" % i
    one_c, one_z = eng.dvae_codes_audio([clips[1]], 16000, norms, z=True)
    assert np.array_equal(one_c[0], want_c[1]) and np.array_equal(one_z[0], want_z[1])
    # without norms the mel differs, hence z
    assert not np.array_equal(eng.dvae_codes_audio([clips[0]], 22050, None, z=True)[1][0], want_z[0])


def test_statuses(pkg, engines):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    m, fr = np.zeros(80 * 10, np.float32), np.array([10], np.int32)
    codes, nc, z = np.full(8, 7, np.int32), np.full(1, 7, np.int32), np.full(8 * 64, 7, np.float32)
    bare = pkg.Engine(0)
    assert bare.L.tts_dvae_codes(bare.h, p(m), p(fr), 1, p(codes), p(nc), 8, None) == STATE and "tts_load_dvae not called" in bare.L.tts_last_error(bare.h).decode()
    x, n, r = np.zeros(3000, np.float32), np.array([3000], np.int64), np.array([22050], np.int32)
    assert bare.L.tts_dvae_codes_audio(bare.h, p(x), p(n), p(r), 1, None, p(codes), p(nc), 8, None) == STATE
    assert bare.dvae_tokens == 0
    bare.close()
    eng = engines("mid")
    L, h = eng.L, eng.h
    call = lambda mel=m, frames=fr, k=1, co=codes, n_=nc, stride=8, zz=None: L.tts_dvae_codes(h, p(mel), p(frames), k, p(co), p(n_), stride, p(zz))  # noqa: E731
    assert call(mel=None) == ARG and call(frames=None) == ARG and call(co=None) == ARG and call(n_=None) == ARG and call(k=0) == ARG and call(stride=0) == ARG
    assert call(frames=np.array([0], np.int32)) == ARG
    assert call(stride=2) == ARG and "code_stride" in L.tts_last_error(h).decode()  # 10 frames make 3 codes
    bad = m.copy()
    bad[17] = np.nan
    assert call(mel=bad) == ARG and "non-finite" in L.tts_last_error(h).decode()
    assert call(frames=np.array([16385], np.int32)) == LIMIT
    assert call(frames=np.full(257, 1, np.int32), k=257) == LIMIT
    assert L.tts_dvae_codes_audio(h, p(np.zeros(400, np.float32)), p(np.array([400], np.int64)), p(r), 1, None, p(codes), p(nc), 8, None) == ARG  # reflect padding
    xb = x.copy()
    xb[5] = np.inf
    assert L.tts_dvae_codes_audio(h, p(xb), p(n), p(r), 1, None, p(codes), p(nc), 8, None) == ARG
    assert (codes == 7).all() and nc[0] == 7 and (z == 7).all(), "a refused call wrote its output"
    assert call(zz=z) == 0 and nc[0] == 3 and (codes[3:] == 7).all() and (z[3 * 64:] == 7).all() and not (z[:3 * 64] == 7).any()  # the rest is left alone


def test_a_call_inside_an_open_ar_session(pkg, mid_models, voice):
    """tts_dvae_codes between two steps of an open AR session: every request's codes, rows and latents are the bits of the session without the call"""
    from test_ar_session_gpu import req, run_session
    eng = pkg.Engine(0)
    eng.load(ar=mid_models + "/ggml-model.bin")
    eng.load_dvae(R.model("mid")[0])
    reqs = [req(9, 2, 1, [6, 9]), req(16, 1, 2, [8], at=2)]
    shape = (4, 2, 16, 12)
    base = run_session(eng, reqs, voice, shape=shape)
    got = []

    def between(step, rid_of, live):
        if step in (1, 3):
            got.append(eng.dvae_codes([R.mel(65)])[0])
    with_call = run_session(eng, reqs, voice, shape=shape, on_step=between)
    alone = eng.dvae_codes([R.mel(65)])[0]
    assert len(got) == 2 and all(np.array_equal(g, alone) for g in got)
    assert sorted(base) == sorted(with_call)
    for k in base:
        for a, b in zip(base[k], with_call[k]):
            if isinstance(a, (list, tuple)):
                assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
            else:
                assert np.array_equal(a, b)
    eng.close()


def test_ar_latents_for_codes_is_the_manual_sequence(pkg, mid_models, voice, tmp_path):
    eng = pkg.Engine(0)
    eng.load(ar=mid_models + "/ggml-model.bin")
    eng.load_dvae(R.model("full")[0])
    toks = np.array([255, 147, 2, 54, 2, 14, 2, 136, 63, 2, 80, 32, 150, 112, 9, 0], np.int32)
    codes = eng.dvae_codes([R.mel(R.FULL_FRAMES)])[0]  # a "recording's" codes: 44 of them, below 8192
    assert len(codes) == 44 and codes.min() >= 0 and codes.max() < 8192
    eng.seed(5)
    eng.rng_save_state(str(tmp_path / "before"))
    got = eng.ar_latents_for_codes(toks, voice, codes)
    eng.rng_save_state(str(tmp_path / "after"))
    assert open(tmp_path / "before", "rb").read() == open(tmp_path / "after", "rb").read(), "the generator was touched"
    eng.ar_begin(toks, voice, 1, 1)
    eng.ar_prefill()
    c502 = pkg.host_pad_codes(codes)
    lat = eng.ar_latents(c502)[0]
    rows = pkg.host_trimmed_rows(c502)
    assert got.shape == (rows, 1024) and np.array_equal(got, lat[:rows]) and np.isfinite(got).all()
    assert np.array_equal(eng.ar_latents_for_codes(toks, voice, codes), got)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    v = np.ascontiguousarray(voice, np.float32)
    rws, out = np.full(1, 7, np.int32), np.full(500 * 1024, 7, np.float32)
    call = lambda cd, n: eng.L.tts_ar_latents_for_codes(eng.h, p(toks), len(toks), p(v), p(cd), n, p(rws), p(out))  # noqa: E731
    assert call(np.zeros(501, np.int32), 501) == LIMIT
    assert call(np.array([8192], np.int32), 1) == ARG and call(np.array([-1], np.int32), 1) == ARG and call(codes, 0) == ARG
    assert rws[0] == 7 and (out == 7).all(), "a refused call wrote its output"
    eng.ar_session_open(2, 1, 16, 4)
    assert call(codes, len(codes)) == STATE
    eng.ar_session_close()
    eng.close()


# ---- the CLI ----
def _models(small_models, tmp_path):
    import shutil
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    R.sw.write_hifigan(str(d / "ggml-hifigan-model.bin"))
    return d


def _write_wav(pkg, path, x, rate):
    assert pkg.lib().tts_write_wav(str(path).encode(), np.ascontiguousarray(x, np.float32), len(x), rate) == 0
    return str(path)


def test_cli_codes_from_equals_the_abi(pkg, engines, tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    clips, rates = [_clip(9000, 1), _clip(5000, 2, 16000)], [22050, 16000]
    paths = [_write_wav(pkg, tmp_path / ("c%d.wav" % i), c, r) for i, (c, r) in enumerate(zip(clips, rates))]
    norms = (1.0 + 0.1 * np.arange(80)).astype(np.float32)
    norms.tofile(str(tmp_path / "norms.bin"))
    want = engines("mid").dvae_codes_audio(clips, rates, norms)
    base = [exe, "--dvae", R.model("mid")[0], "--codes-from", ",".join(paths), "--mel-norms", str(tmp_path / "norms.bin")]
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("codes: ")]
    assert len(lines) == 2
    for l, p, w in zip(lines, paths, want):
        assert l.split()[1] == p and [int(v) for v in l.split()[2:]] == list(w)
    r = subprocess.run(base + ["--codes-out", str(tmp_path / "codes.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "codes:" not in r.stdout, r.stdout + r.stderr
    got = [[int(v) for v in l.split()] for l in open(tmp_path / "codes.txt").read().splitlines()]
    assert got == [list(w) for w in want]


@pytest.mark.parametrize("decoder", ["diffusion", "hifigan"])
def test_cli_revoice_writes_the_abi_composition(pkg, small_models, voice, tmp_path, decoder):
    import subprocess
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    d = _models(small_models, tmp_path)
    clip = _clip(int(1.5 * 22050), 4)
    src = _write_wav(pkg, tmp_path / "in.wav", clip, 22050)
    msg = "hello there world"
    cmd = [exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--seed", "3", "--dvae", R.model("full")[0], "--revoice", src,
           "--output", str(tmp_path / "o.wav"), "--decoder", decoder] + (["--steps", "3"] if decoder == "diffusion" else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(tmp_path / "o.wav", "rb").read()
    assert raw[:4] == b"RIFF"
    got = np.frombuffer(raw[44:], np.float32)
    eng = pkg.Engine(0)
    eng.load(ar=str(d / "ggml-model.bin"))
    eng.tokenizer_load(str(d / "tokenizer.json"))
    eng.load_dvae(R.model("full")[0])
    eng.seed(3)
    codes = eng.dvae_codes_audio([clip], 22050)[0]
    lat = eng.ar_latents_for_codes(eng.tokenize(msg), voice, codes)
    assert "revoice: %d codes, %d latent rows" % (len(codes), len(lat)) in r.stdout
    if decoder == "hifigan":
        eng.load_hifigan(str(d / "ggml-hifigan-model.bin"))
        want = eng.hifigan_decode([lat], voice)[0]
    else:
        eng.load(diffusion=str(d / "ggml-diffusion-model.bin"), vocoder=str(d / "ggml-vocoder-model.bin"))
        want = eng.vocoder([eng.diffusion([lat], n_steps=3)[0]])[0]
    eng.close()
    assert len(got) == len(want) and np.array_equal(got, want)
    assert not np.array_equal(clip[:100], got[:100])
