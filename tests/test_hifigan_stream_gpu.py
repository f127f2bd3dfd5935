"""GPU: the streaming forms of the HiFi-GAN decoder. tts_hifigan_chunk: the chunks of any partition are the bits of tts_hifigan_decode, whatever the batch and
the tile variant; tts_hifigan_stream: tts_autoregressive's codes, rows, steps and RNG state, audio through a callback whose concatenation is the decode of the
latents it returns; every status; the CLI. The arithmetic behind the window and the prefix property is pinned in float64 by tests/test_hifigan_stream_cpu.py.

Stream latents against tts_autoregressive's latents: every latent pass of the stream runs on the multi-row kernels (at least 32 rows) and the comparison is
exact, at 39 rows (one GEMM row block, one attention block) and at 209 rows (passes of 40 .. 210 rows: two row blocks, several attention blocks). An utterance
that keeps fewer than 31 rows ends on the exact-f32 GEMV pass, whose order differs: it is held to rel_err < 1e-4, the gate
tests/test_ar_gpu.py::test_latents uses against the oracle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_hifigan_cpu import hifigan_model, inputs  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = 24
MSG = "this is a test message."
FLAGS = 3  # TTS_AR_MASK_STOP | TTS_AR_RETIRE


@pytest.fixture(scope="module")
def eng(pkg, hifigan_model):
    e = pkg.Engine(0)
    e.load_hifigan(hifigan_model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def whole(eng):
    """tts_hifigan_decode of the L-row input, once per length"""
    memo = {}

    def run(L):
        if L not in memo:
            lat, v = inputs(L)
            memo[L] = eng.hifigan_decode([lat], v)[0]
        return memo[L]
    return run


def partitions(T):
    out = [[(0, T)]]
    if T == 87:
        out += [[(t, 1) for t in range(T)], [(0, 24), (24, 1), (25, 38), (63, 24)]]
    if T > 50:
        out += [[(0, 30), (30, 20), (50, T - 50)]]  # [30, 50): both edges cut
    return out


def chunked(eng, L, parts):
    lat, v = inputs(L)
    return np.concatenate([eng.hifigan_chunk([lat], v, [f0], [n])[0] for f0, n in parts])


@pytest.mark.parametrize("L", [20, 1, 3, 60])
def test_partitions(eng, whole, L):
    T = eng.frames(L)
    for parts in partitions(T):
        got = chunked(eng, L, parts)
        assert got.tobytes() == whole(L).tobytes(), "L = %d, %d chunks starting %s" % (L, len(parts), parts[:4])


def test_ragged_batch_of_windows(eng):
    cases = [inputs(17), inputs(1, seed=6), inputs(20, seed=7)]
    lats = [c[0] for c in cases]
    voices = np.stack([cases[0][1], cases[1][1]])
    voice_of, f0, nf = [0, 1, 0], [40, 0, 3], [30, 4, 61]
    full = eng.hifigan_decode(lats, voices, voice_of)
    got = eng.hifigan_chunk(lats, voices, f0, nf, voice_of)
    for c in range(3):
        alone = eng.hifigan_chunk([lats[c]], voices[voice_of[c]], [f0[c]], [nf[c]])[0]
        assert got[c].tobytes() == alone.tobytes(), "candidate %d differs from its own single-candidate chunk" % c
        assert got[c].tobytes() == full[c][256 * f0[c]:256 * (f0[c] + nf[c])].tobytes(), "candidate %d differs from the whole decode" % c


def test_small_m_variant_on_and_off(pkg, eng, whole):
    try:
        for L in (20, 1, 3, 60):
            T = eng.frames(L)
            for parts in partitions(T):
                if len(parts) > 8:
                    parts = parts[::9]  # a sample of the single-frame chunks
                res = []
                for rows in (0, 1 << 24, 2048):  # never (the default), always (where the channels allow), up to stage 0 of a streaming window
                    eng.set_option("hfg_small_m", rows)
                    res.append(b"".join(eng.hifigan_chunk([inputs(L)[0]], inputs(L)[1], [f0], [n])[0].tobytes() for f0, n in parts))
                want = b"".join(whole(L)[256 * f0:256 * (f0 + n)].tobytes() for f0, n in parts)
                assert res[0] == want and res[1] == want and res[2] == want, (L, parts[:4])
    finally:
        eng.set_option("hfg_small_m", 0)
    with pytest.raises(pkg.TtsError, match="hfg_small_m"):
        eng.set_option("hfg_small_m", -1)


def test_no_hidden_state(eng):
    lat, v = inputs(20)
    a = eng.hifigan_decode([lat], v)[0]
    c1 = eng.hifigan_chunk([lat], v, [30], [20])[0]
    c2 = eng.hifigan_chunk([lat], v, [30], [20])[0]
    b = eng.hifigan_decode([lat], v)[0]
    assert a.tobytes() == b.tobytes() and c1.tobytes() == c2.tobytes()


def test_prefix_property_on_the_device(eng, whole):
    lat, v = inputs(60)
    n = eng.frames(33) - HALO
    assert n > 0
    got = eng.hifigan_chunk([lat[:33]], v, [0], [n])[0]
    assert got.tobytes() == whole(60)[:256 * n].tobytes()
    # ... and the first frame past it is not final yet
    more = eng.hifigan_chunk([lat[:33]], v, [0], [eng.frames(33)])[0]
    assert more.tobytes() != whole(60)[:256 * eng.frames(33)].tobytes()


# ---- the stream driver ----
@pytest.fixture(scope="module")
def ar(pkg, small_models, hifigan_model):
    e = pkg.Engine(0)
    e.load(ar=small_models + "/ggml-model.bin")
    e.load_hifigan(hifigan_model)
    e.tokenizer_load(os.path.join(ROOT, "models", "tokenizer.json"))
    yield e
    e.close()


def rng_state(e, tmp_path):
    p = str(tmp_path / "rng.txt")
    e.rng_save_state(p)
    return open(p).read()


@pytest.fixture(scope="module")
def plain(ar, voice, tmp_path_factory):
    """tts_autoregressive with one candidate, the stream tests' reference: (codes, rows, latents, steps, RNG state afterwards)"""
    ar.set_stop_schedule([30])
    ar.seed(11)
    codes, rows, lats, steps = ar.autoregressive(ar.tokenize(MSG), voice, 1, 40, mask_stop=True, retire=True)
    return codes[0], int(rows[0]), lats[0], steps, rng_state(ar, tmp_path_factory.mktemp("rng"))


@pytest.mark.parametrize("stride", [1, 8, 64])
def test_stream_driver(ar, voice, plain, tmp_path, stride):
    ar.set_stop_schedule([30])
    ar.seed(11)
    codes, rows, lat, chunks, steps = ar.hifigan_stream(ar.tokenize(MSG), voice, 40, FLAGS, stride)
    recaptures = ar.hifigan_stream_recaptures()
    assert codes.tobytes() == plain[0].tobytes() and rows == plain[1] and steps == plain[3]
    assert rng_state(ar, tmp_path) == plain[4]
    audio = np.concatenate([c[0] for c in chunks])
    assert audio.tobytes() == ar.hifigan_decode([lat], voice)[0].tobytes()
    assert [c[1] for c in chunks] == [False] * (len(chunks) - 1) + [True]
    assert all(len(c[0]) % 256 == 0 and len(c[0]) > 0 for c in chunks)
    print("stride %d: %d callbacks of %s frames, %d rows" % (stride, len(chunks), [len(c[0]) // 256 for c in chunks], rows))
    if stride == 8:
        assert len(chunks) > 1
    if stride == 64:
        assert len(chunks) == 1
    assert recaptures == 0, "the decode step was re-captured inside the loop"
    # stream latents against tts_autoregressive's (39 rows: every pass on the multi-row kernels)
    rel = np.abs(lat - plain[2]).max() / np.abs(plain[2]).max()
    print("stride %d: stream latents vs tts_autoregressive: rel_err %.2e, identical %s" % (stride, rel, lat.tobytes() == plain[2].tobytes()))
    assert lat.tobytes() == plain[2].tobytes()


def test_stream_latents_of_a_short_utterance(ar, voice):
    """20 rows at the end: the last pass is the exact-f32 GEMV path, the prefix pass the multi-row one — close, not identical"""
    ar.set_stop_schedule(None)
    ar.seed(5)
    _, rows, lats, _ = ar.autoregressive(ar.tokenize(MSG), voice, 1, 12, mask_stop=True)
    ar.seed(5)
    _, srows, lat, chunks, _ = ar.hifigan_stream(ar.tokenize(MSG), voice, 12, 1, 6)
    assert srows == int(rows[0]) and len(chunks) >= 1
    rel = np.abs(lat - lats[0]).max() / np.abs(lats[0]).max()
    print("short utterance (%d rows, %d callbacks): rel_err %.2e" % (srows, len(chunks), rel))
    assert rel < 1e-4
    assert np.concatenate([c[0] for c in chunks]).tobytes() == ar.hifigan_decode([lat], voice)[0].tobytes()


def test_stream_latents_of_a_long_utterance(ar, voice):
    """200 codes, 209 rows: the prefix passes grow from 40 to 201 rows and the last one has 210, so the passes cross the 128-row GEMM block and run several
    attention blocks, where the 39-row cases stay inside one of each. A row is computed from itself and the keys before it whatever the pass length: exact."""
    ar.set_stop_schedule(None)
    ar.seed(9)
    codes, rows, lats, steps = ar.autoregressive(ar.tokenize(MSG), voice, 1, 200, mask_stop=True)
    ar.seed(9)
    scodes, srows, lat, chunks, ssteps = ar.hifigan_stream(ar.tokenize(MSG), voice, 200, 1, 32)
    assert scodes.tobytes() == codes[0].tobytes() and srows == int(rows[0]) and ssteps == steps
    assert ar.hifigan_stream_recaptures() == 0
    rel = np.abs(lat - lats[0]).max() / np.abs(lats[0]).max()
    print("long utterance (%d rows, callbacks of %s frames): rel_err %.2e" % (srows, [len(c[0]) // 256 for c in chunks], rel))
    assert srows > 200 and len(chunks) > 3
    assert lat.tobytes() == lats[0].tobytes()
    assert np.concatenate([c[0] for c in chunks]).tobytes() == ar.hifigan_decode([lat], voice)[0].tobytes()


def test_callback_raises(ar, voice, plain):
    """an exception inside on_chunk cancels the call and comes out of hifigan_stream; the context works afterwards"""
    ar.set_stop_schedule([30])
    ar.seed(11)

    def boom(a, last):
        raise KeyError("from the callback")
    with pytest.raises(KeyError, match="from the callback"):
        ar.hifigan_stream(ar.tokenize(MSG), voice, 40, FLAGS, 8, on_chunk=boom)
    ar.seed(11)
    codes = ar.hifigan_stream(ar.tokenize(MSG), voice, 40, FLAGS, 8)[0]
    assert codes.tobytes() == plain[0].tobytes()


def test_callback_cancels(ar, voice, plain, pkg):
    ar.set_stop_schedule([30])
    ar.seed(11)
    seen = []
    with pytest.raises(pkg.TtsError, match=r"cancelled by the callback \(status -5\)"):
        ar.hifigan_stream(ar.tokenize(MSG), voice, 40, FLAGS, 8, on_chunk=lambda a, last: seen.append(len(a)) or True)
    assert len(seen) == 1
    ar.seed(11)
    codes, rows, lats, steps = ar.autoregressive(ar.tokenize(MSG), voice, 1, 40, mask_stop=True, retire=True)
    assert codes[0].tobytes() == plain[0].tobytes() and lats[0].tobytes() == plain[2].tobytes() and steps == plain[3]


def test_statuses(pkg, ar, eng, voice, small_models):
    A, S = -1, -5
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lat, v = inputs(3)  # T = 13
    rows, out = np.array([3], np.int32), np.empty(256 * 13, np.float32)
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731

    def chunk(e, lat=lat, rows=rows, n=1, v=v, nv=1, idx=None, f0=i32(0), nf=i32(13), out=out):
        return e.L.tts_hifigan_chunk(e.h, p(lat), p(rows), n, p(v), nv, p(idx), p(f0), p(nf), p(out)), e.L.tts_last_error(e.h).decode()
    base = eng.hifigan_chunk([lat], v, [0], [13])[0]
    for kw, msg in ((dict(f0=None), "bad argument"), (dict(nf=None), "bad argument"), (dict(lat=None), "bad argument"), (dict(out=None), "bad argument"),
                    (dict(f0=i32(-1)), "asks for 13 frames from frame -1"), (dict(nf=i32(0)), "asks for 0 frames from frame 0"),
                    (dict(f0=i32(1)), "asks for frames [1, 14) of 13"), (dict(f0=i32(2 ** 31 - 1), nf=i32(2 ** 31 - 1)), "of 13"),
                    (dict(rows=i32(0)), "0 latent rows"), (dict(nv=0), "0 voices"), (dict(idx=i32(1)), "names voice 1 of 1")):
        rc, err = chunk(eng, **kw)
        assert rc == A and "tts_hifigan_chunk" in err and msg in err, (kw, rc, err)
    assert eng.hifigan_chunk([lat], v, [0], [13])[0].tobytes() == base.tobytes()  # a refused call changed nothing
    fresh = pkg.Engine(0)
    rc, err = chunk(fresh)
    assert rc == S and "tts_load_hifigan not called" in err
    # the stream: stride, callback, call order
    tok = np.ascontiguousarray(ar.tokenize(MSG), np.int32)
    codes, r1, st = np.empty(502, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    cb = pkg.AUDIO_CB(lambda u, s, n, last: 0)

    def stream(e, stride=8, cb=cb, max_steps=8, codes=codes):
        rc = e.L.tts_hifigan_stream(e.h, p(tok), len(tok), p(voice), max_steps, 1, stride, None if cb is None else C.cast(cb, C.c_void_p), None, p(codes), p(r1),
                                    None, p(st))
        return rc, e.L.tts_last_error(e.h).decode()
    for kw in (dict(stride=0), dict(cb=None)):
        rc, err = stream(ar, **kw)
        assert rc == A and "tts_hifigan_stream: bad argument" in err, (kw, rc, err)
    rc, err = stream(ar, codes=None)
    assert rc == A and "null output" in err
    rc, err = stream(ar, max_steps=501)
    assert rc == -6 and "500 codes" in err
    rc, err = stream(fresh)
    assert rc == S and "AR model not loaded" in err
    fresh.load(ar=small_models + "/ggml-model.bin")
    rc, err = stream(fresh)
    assert rc == S and "tts_load_hifigan not called" in err
    fresh.close()
    rc, err = stream(ar)
    assert rc == 0, err  # and the context still works


def test_cli_stream(small_models, hifigan_model, tmp_path):
    d = tmp_path / "models"
    d.mkdir()
    os.symlink(os.path.join(small_models, "ggml-model.bin"), d / "ggml-model.bin")
    os.symlink(hifigan_model, d / "ggml-hifigan-model.bin")
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    base = [exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", MSG, "--seed", "3", "--codes", "40", "--decoder", "hifigan"]
    r = subprocess.run(base + ["--output", str(tmp_path / "a.wav")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(base + ["--output", str(tmp_path / "b.wav"), "--timing", "1", "--stream-stride", "8", "--stream"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[timing] first audio" in r.stderr and "stride 8" in r.stderr
    a, b = (tmp_path / "a.wav").read_bytes(), (tmp_path / "b.wav").read_bytes()
    assert len(a) == 44 + 4 * 256 * 208 and a == b  # 48 rows, 208 frames
    r = subprocess.run(base[:base.index("--message")] + ["--message", "--stream", "--seed", "3", "--codes", "40", "--decoder", "hifigan", "--timing", "1", "--output",
                                                        str(tmp_path / "c.wav")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "first audio" not in r.stderr, r.stdout + r.stderr  # a value that reads "--stream" is a value
    nowhere = str(tmp_path / "nowhere")  # no model there: a refusal must come before any load
    for extra, what in ((["--decoder", "diffusion"], "--decoder diffusion"), (["--clvp", "x.bin"], "--clvp"), (["--split-text", "50"], "--split-text"),
                        (["--voice", "second.bin"], "several --voice"), (["--devices", "2"], "--devices > 1"), (["--candidates", "2"], "--candidates > 1"),
                        (["--stream-stride", "0"], "--stream-stride 0")):
        r = subprocess.run([exe, "--models", nowhere, "--voice", "first.bin", "--message", MSG, "--decoder", "hifigan", "--stream"] + extra, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 1 and what in r.stderr and "model" not in r.stderr.replace("--models", ""), (extra, r.stderr)
