"""CPU tests: the product's host logic (C ABI on a host-only context) against the real reference code's answers
(stored under tests/golden/, and live from oracle/_ref/libref.so where the reference checkout was available at build
time) and against the committed golden vectors. No device compute happens here."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, MODELS


@pytest.fixture(scope="module")
def host(pkg):
    L = pkg.lib()
    h = L.tts_create(-1)
    assert h
    eng = pkg.Engine.__new__(pkg.Engine)
    eng.L, eng.h = L, h
    yield eng
    eng.close()


def test_library_exports_every_header_symbol(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    missing = [s for s in pkg.header_symbols() if not hasattr(L, s)]
    assert not missing, missing
    assert len(pkg.header_symbols()) >= 25


def test_host_only_context_refuses_compute(pkg, host):
    with pytest.raises(pkg.TtsError, match="no HIP device"):
        host.load(ar="/nonexistent")


def test_rng_matches_reference_fixtures(host, oracle):
    g = json.load(open(os.path.join(GOLDEN, "host_golden.json")))
    host.seed(245645656)
    got = [host.rng_uniform() for _ in range(8)]
    assert got == [np.float32(x) for x in g["uniform_seed_245645656"]]
    host.rng_load_state(os.path.join(GOLDEN, "reference_assets", "test_autoregressive_seed.bin"))
    assert [host.rng_uniform() for _ in range(8)] == got  # the fixture state == mt19937(245645656)
    host.rng_load_state(os.path.join(GOLDEN, "reference_assets", "test_diffusion_seed.bin"))
    n = host.rng_normal(len(g["normal_diffusion_seed"]))
    assert (n == np.array(g["normal_diffusion_seed"], np.float32)).all()
    # oracle restatement in lock-step with the product (libstdc++) over a long mixed stream
    r = oracle.Rng(99)
    host.seed(99)
    assert [host.rng_uniform() for _ in range(5)] == [r.uniform() for _ in range(5)]
    assert (host.rng_normal(10001) == r.normal(10001)).all()
    assert host.rng_uniform() == r.uniform()


def test_tokenizer_golden(host):
    g = json.load(open(os.path.join(GOLDEN, "host_golden.json")))
    host.tokenizer_load(os.path.join(MODELS, "tokenizer.json"))
    for msg, ids in g["tokenizer"].items():
        assert list(host.tokenize(msg)) == ids, msg


def _fuzz_golden():
    """The reference's own answers to the seeded fuzz inputs below (tests/golden/make_fuzz_golden.py, from oracle/_ref/libref.so)."""
    return np.load(os.path.join(GOLDEN, "reference_fuzz_golden.npz"))


def test_tokenizer_fuzz_vs_reference(host, oracle):
    """300 random messages: the product's and the oracle's tokenizer against the reference's (stored answers; and live, where libref.so was built)."""
    R = oracle.ref()
    g = _fuzz_golden()
    stored = np.split(g["tok_ids"], np.cumsum(g["tok_len"])[:-1])
    host.tokenizer_load(os.path.join(MODELS, "tokenizer.json"))
    if R is not None:
        R.ref_tokenizer_init(os.path.join(MODELS, "tokenizer.json").encode())
    tk = oracle.Tokenizer(os.path.join(MODELS, "tokenizer.json"))
    rs = np.random.RandomState(0)
    alphabet = list("abcdefghijklmnopqrstuvwxyz     .,!?'-\"[]0123456789ABCXYZ;:()\t\n") + ["[SPACE]", "[STOP]", "'s", "'re", "é", "ß"]
    devnull = os.open(os.devnull, os.O_WRONLY)
    saved = os.dup(2)
    os.dup2(devnull, 2)  # both sides print "unknown token" to stderr
    try:
        for i in range(300):
            msg = "".join(rs.choice(alphabet) for _ in range(rs.randint(0, 60)))
            want = list(stored[i])
            if R is not None:
                out = np.empty(2048, np.int32)
                n = R.ref_tokenize(msg.encode("utf-8"), out, 2048)
                assert list(out[:n]) == want, repr(msg)
            assert list(host.tokenize(msg)) == want, repr(msg)
            assert list(tk.encode(msg)) == want, repr(msg)
    finally:
        os.dup2(saved, 2)
        os.close(devnull)


def test_sampler_golden(host, oracle):
    g = np.load(os.path.join(GOLDEN, "sampler_golden.npz"))
    for k in range(len(g["seeds"])):
        logits, ids, seed, want = g["logits_%d" % k], g["ids_%d" % k], int(g["seeds"][k]), g["samples_%d" % k]
        host.seed(seed)
        assert (host.sample(logits, ids) == want).all(), k
        r = oracle.Rng(seed)
        assert (oracle.sample(logits, ids, r) == want).all(), k
        assert host.rng_uniform() == r.uniform()


def test_sampler_fuzz_vs_reference(host, oracle):
    """150 random logit batches: the product's sampler against the reference's (stored answers; and live, where libref.so was built)."""
    R = oracle.ref()
    g = _fuzz_golden()
    at = 0
    rs = np.random.RandomState(1)
    for trial in range(150):
        B = 16 if trial % 10 == 9 else rs.randint(1, 6)  # B >= 4 runs on the sampler thread pool
        scale = rs.choice([0.3, 1.0, 3.0, 8.0])
        logits = (rs.randn(B, 8194) * scale).astype(np.float32)
        if trial % 5 == 0:  # ties at the top-k boundary and among survivors
            logits = np.round(logits * 2) / 2
        k = rs.choice([1, 18])
        ids = rs.randint(0, 8194, (B, k)).astype(np.int32)
        if k == 18:
            ids[:, :-1] = 1
            ids[:, -1] = 8192
        seed = int(rs.randint(1 << 30))
        want, want_u = g["samp_ids"][at:at + B], g["samp_next_uniform"][trial]
        at += B
        if R is not None:
            R.ref_seed(seed)
            live = np.empty(B, np.int32)
            R.ref_process_logits_and_sample(logits.reshape(-1), ids.reshape(-1), ids.size, B, live, None)
            assert (live == want).all() and R.ref_uniform() == want_u, trial
        host.seed(seed)
        got = host.sample(logits, ids)
        assert (got == want).all(), (trial, got, want)
        assert host.rng_uniform() == want_u
    assert at == len(g["samp_ids"])


def test_sampler_from_prefiltered_list_equals_full_row(pkg, host):
    """Option device_topk (tts_ar_step_sample): the decode step hands the host only each candidate's 64..128 largest logits. Whatever the list decides
    must be what the full row decides; where it cannot know (ties among the survivors, the cut within 4 ulps of the list's smallest entry) it must say
    so (-1 -> the engine fetches the row) instead of guessing."""
    rs = np.random.RandomState(7)
    undecided = decided = 0
    for trial in range(400):
        scale = rs.choice([0.3, 1.0, 3.0, 8.0])
        row = (rs.randn(8194) * scale).astype(np.float32)
        kind = trial % 8
        if kind == 1:  # coarse values: ties everywhere, also across the threshold
            row = np.round(row * 4) / 4
        elif kind == 2:  # the logits around the top-k cut are consecutive floats: the 4-ulp window of sample_one reaches below the list
            order = np.argsort(-row)
            v = row[order[40]]
            for r in range(41, 75):
                v = np.nextafter(v, np.float32(-np.inf))
                row[order[r]] = v
        elif kind == 3:  # mostly negative rows (penalty = x * 2), zeros of both signs
            row = -np.abs(row)
            row[rs.randint(0, 8194, 40)] = 0.0
            row[rs.randint(0, 8194, 40)] = -0.0
        order = np.argsort(-row)
        pick = rs.randint(5)
        ids = [[order[0]], [order[rs.randint(50)]], [order[49], order[50]], [rs.randint(8194)], list(order[rs.randint(0, 60, 4)])][pick]
        if trial % 50 == 49:
            ids = list(order[:6])  # more than four distinct penalty ids: only the literal path knows
        u = 0.0 if trial % 37 == 0 else float(rs.rand())
        keep = int(rs.choice([54, 64, 64, 100, 128]))
        want = pkg.host_sample_row(row, ids, u)
        got = pkg.host_sample_prefiltered(row, ids, u, keep)
        assert got in (want, -1), (trial, kind, keep, got, want)
        if kind in (0, 4, 5, 6, 7) and len(set(ids)) <= 4 and keep >= 64:
            assert got == want, (trial, kind, keep)  # continuous random logits, the device's list sizes: the list always decides
            # (keep = 54 with four penalised top logits puts the 50th survivor AT the list's end: undecidable by design)
        undecided += got == -1
        decided += got == want
        # the pure function is the sampler tts_sample runs: same id from the ctx RNG's second uniform
        if trial % 10 == 0:
            host.seed(trial)
            ref = host.sample(row[None], np.asarray(ids, np.int32)[None])[0]
            host.seed(trial)
            host.rng_uniform()
            assert pkg.host_sample_row(row, ids, host.rng_uniform()) == ref
    assert decided > 200 and undecided > 50, (decided, undecided)  # both branches were exercised
    assert pkg.host_sample_prefiltered(np.zeros(8194, np.float32), [0], 0.5, 64) == -1  # 8194-way tie: no list


def test_schedule_scalars_golden_and_oracle(pkg, oracle):
    """The diffusion driver's schedule arithmetic (host_logic.cpp: DiffSchedule) against the committed golden vectors of
    the reference's own code (80 steps) and against the oracle for other step counts (SURVEY 8d config 5 uses 200)."""
    g = np.load(os.path.join(GOLDEN, "schedule_golden.npz"))
    tm, s = pkg.host_schedule(80)
    assert (tm == g["timestep_map"]).all()
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    assert (s["min_log"] == f32(g["post_logvar"])).all()
    assert (s["coef1"] == f32(g["coef1"])).all() and (s["coef2"] == f32(g["coef2"])).all()
    assert (s["sqrt_recip"] == f32(g["sqrt_recip"])).all() and (s["sqrt_recipm1"] == f32(g["sqrt_recipm1"])).all()
    assert np.abs(s["max_log"] - f32(np.log(g["betas"]))).max() <= 1e-6  # log in double on both sides, one float ulp at most
    t = np.arange(80, dtype=np.float32)
    assert (s["cfk"] == np.float32(2.0) * (np.float32(1) - t / np.float32(80))).all()
    for n in (2, 6, 200):
        tm, s = pkg.host_schedule(n)
        tmo = oracle.default_timestep_map(n)
        assert (tm == tmo).all() and tm[0] == 0 and tm[-1] == 3999
        o = oracle.schedule(tmo)
        assert (s["min_log"] == f32(o["post_logvar"])).all(), n
        assert (s["coef1"] == f32(o["coef1"])).all() and (s["coef2"] == f32(o["coef2"])).all(), n
        assert (s["sqrt_recip"] == f32(o["sqrt_recip"])).all() and (s["sqrt_recipm1"] == f32(o["sqrt_recipm1"])).all(), n
        assert np.abs(s["max_log"] - f32(np.log(o["betas"]))).max() <= 1e-6, n


def test_timestep_embedding_and_buckets_golden(pkg, oracle):
    g = np.load(os.path.join(GOLDEN, "schedule_golden.npz"))
    for t in (0, 51, 2025, 3999):
        assert (pkg.host_timestep_embedding(t) == g["temb_%d" % t]).all(), t
    hg = json.load(open(os.path.join(GOLDEN, "host_golden.json")))
    for n, tab in hg["buckets"].items():
        assert (pkg.host_rel_buckets(int(n)) == np.array(tab)).all(), n
    assert (pkg.host_rel_buckets(130) == oracle.buckets(130)).all()  # distances past the saturation point (>= 50)


def test_padding_and_trim_vs_oracle(pkg, oracle):
    """apply_padding / trim_latents of the product against the oracle's restatement (itself pinned to the reference's
    code by tests/test_oracle_golden.py), on sequences with stop-typo tokens (8139), real stops and long runs of 83."""
    rs = np.random.RandomState(3)
    cases = [np.array([], np.int32), np.array([8139], np.int32), np.array([5, 6, 83, 83, 7], np.int32),
             np.full(500, 83, np.int32), np.full(500, 7, np.int32)]
    for _ in range(40):
        n = int(rs.randint(0, 501))
        c = rs.choice([83, 83, 83, 45, 248, 8139, 8193, 17, 4000], n).astype(np.int32)
        if n and rs.rand() < 0.5:
            c[-int(rs.randint(1, min(n, 12) + 1)):] = 8139
        cases.append(c)
    for c in cases:
        got, want = pkg.host_pad_codes(c), oracle.apply_padding(c)
        assert (got == want).all(), c[:20]
        assert pkg.host_trimmed_rows(got) == oracle.trimmed_rows(want)
    with pytest.raises(pkg.TtsError):
        pkg.host_pad_codes(np.zeros(501, np.int32))


def test_wav_writer_header(pkg, tmp_path):
    """RIFF/WAVE, fmt chunk 16 bytes, format tag 3 (IEEE float), mono, 24 kHz, 32 bit, raw f32 data (main.cpp:4821-4868)."""
    import struct
    x = np.linspace(-1, 1, 1000).astype(np.float32)
    p = str(tmp_path / "a.wav")
    assert pkg.write_wav(p, x) == 0
    b = open(p, "rb").read()
    assert len(b) == 44 + 4000
    assert b[:4] == b"RIFF" and struct.unpack("<i", b[4:8])[0] == 36 + 4000 and b[8:16] == b"WAVEfmt "
    fmt_size, tag, ch, rate, brate, align, bits = struct.unpack("<ihhiihh", b[16:36])
    assert (fmt_size, tag, ch, rate, brate, align, bits) == (16, 3, 1, 24000, 96000, 4, 32)
    assert b[36:40] == b"data" and struct.unpack("<i", b[40:44])[0] == 4000
    assert (np.frombuffer(b[44:], np.float32) == x).all()


def test_rng_state_round_trip(pkg, tmp_path):
    """a host program that keeps its own std::mt19937 hands the state to the library before a stage call
    (tts_rng_load_state) and takes it back afterwards (tts_rng_save_state). The saved text is libstdc++'s `fout << generator`; a second
    context that loads it continues the very same stream (uniforms and normals)."""
    L = pkg.lib()
    a = pkg.Engine.__new__(pkg.Engine); a.L = L; a.h = L.tts_create(-1)
    b = pkg.Engine.__new__(pkg.Engine); b.L = L; b.h = L.tts_create(-1)
    a.seed(245645656)
    for _ in range(37):
        a.rng_uniform()
    a.rng_normal(10)  # an even count: no cached second value is left inside the normal distribution
    p = str(tmp_path / "rng.txt")
    a.rng_save_state(p)
    b.rng_load_state(p)
    assert [a.rng_uniform() for _ in range(5)] == [b.rng_uniform() for _ in range(5)]
    assert (a.rng_normal(8) == b.rng_normal(8)).all()
    # the text is what the reference's fixtures hold: the fixture loads, saves back identically
    fx = os.path.join(GOLDEN, "reference_assets", "test_autoregressive_seed.bin")
    b.rng_load_state(fx)
    b.rng_save_state(p)
    assert open(p).read().split() == open(fx).read().split()
    a.close(); b.close()


def test_header_is_plain_c_and_links(pkg, tmp_path):
    """The drop-in boundary is a C ABI: include/tortoise_mi355x.h must compile as C99 with no C++ or torch types, and a plain C program linked
    against the shared library must reach the host-side entries (no device: tts_create(-1))."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(r'''
#include <stdio.h>
#include <stdint.h>
#include "tortoise_mi355x.h"
int main(void) {
  tts_ctx *ctx = tts_create(-1);
  if (!ctx) return 2;
  int32_t codes[502];
  for (int i = 0; i < 502; i++) codes[i] = 83;
  printf("%d %d %d %d\n", tts_diffusion_frames(200), tts_vocoder_samples(870), tts_host_rel_bucket(0, 5), tts_host_trimmed_rows(codes));
  int rc = tts_load_ar(ctx, "/nonexistent");
  printf("%d %s\n", rc, tts_last_error(ctx));
  tts_destroy(ctx);
  return 0;
}
''')
    exe = tmp_path / "abi"
    inc = os.path.join(os.path.dirname(os.path.dirname(pkg.LIB_PATH)), "include")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(exe), "-L", libdir,
                    "-ltortoise_mi355x", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    a = out[0].split()
    assert int(a[0]) == 870 and int(a[1]) == 880 * 256 - 6
    assert int(a[3]) == pkg.host_trimmed_rows(np.full(502, 83, np.int32)) if hasattr(pkg, "host_trimmed_rows") else True
    assert out[1].startswith("-") and "no HIP device" in out[1]


def test_bulk_normal_draws_equal_single_draws(pkg, host, oracle):
    """Round 6: counts of 4096 and more take a two-phase form of libstdc++'s normal_distribution (host_logic.cpp: rng_normal_fill — the generator calls and the accept test on
    the calling thread, log / sqrt / divide of the accepted pairs on a few threads). Every float must equal the one a single operator() call returns, and generator and
    distribution must be left in the state single draws leave them in: odd and even counts in sequence (the cached second value crosses calls and crosses the two forms),
    uniforms in between, against a context with option rng_fast_normal = 0 — and against the reference's compiled sample_normal_noise (oracle/_ref)."""
    L = pkg.lib()
    slow = pkg.Engine.__new__(pkg.Engine); slow.L = L; slow.h = L.tts_create(-1)
    slow.set_option("rng_fast_normal", 0)
    counts = (5000, 4097, 3, 100001, 1, 8192, 65537, 7, 87000, 87001, 4096, 2)
    for seed in (0, 1, 245645656):
        host.seed(seed); slow.seed(seed)
        for n in counts:
            x, y = host.rng_normal(n), slow.rng_normal(n)
            assert (x.view(np.uint32) == y.view(np.uint32)).all(), (seed, n)
            assert host.rng_uniform() == slow.rng_uniform(), (seed, n)
    slow.close()
    R = oracle.ref()  # the reference's answers are stored (tests/golden/make_fuzz_golden.py); compared live as well where libref.so was built
    g = _fuzz_golden()
    host.seed(77)
    if R is not None:
        R.ref_seed(77)
    at = 0
    for n in (87000, 4097, 5, 20000):
        want = g["normal_seed77"][at:at + n]
        at += n
        if R is not None:
            live = np.empty(n, np.float32)
            R.ref_normal_fill(live, n)
            assert (live.view(np.uint32) == want.view(np.uint32)).all(), n
        assert (host.rng_normal(n).view(np.uint32) == want.view(np.uint32)).all(), n
    assert host.rng_uniform() == g["normal_seed77_next_uniform"][0]
    if R is not None:
        assert R.ref_uniform() == g["normal_seed77_next_uniform"][0]
