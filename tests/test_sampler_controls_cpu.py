"""CPU: the autoregressive sampler's controls (options "ar_temperature", "ar_top_k", "ar_top_p", "ar_repetition_penalty", "ar_penalty_scope"; probes
tts_host_sample_row_ex / tts_host_sample_prefiltered_ex; CLI flags --temperature / --top-k / --top-p / --repetition-penalty / --penalty-scope). No device:
tts_create(-1), the host probes and `tortoise --dry-run 1`.

What the fast paths are held to is the literal formulation (mode 1 of the probe: the reference's process_logits_and_sample with its literals made parameters), and
the literal formulation itself to `ref_sample` below, an independent float64 restatement. tests/test_sampler_controls_gpu.py imports the helpers."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 8194
f32 = np.float32
DEFAULTS = dict(temperature=0.8, top_k=50, top_p=0.8, penalty=2.0)
OPTION_OF = dict(temperature="ar_temperature", top_k="ar_top_k", top_p="ar_top_p", penalty="ar_repetition_penalty")


@pytest.fixture(scope="module")
def host(pkg):
    L = pkg.lib()
    h = L.tts_create(-1)
    assert h
    eng = pkg.Engine.__new__(pkg.Engine)
    eng.L, eng.h = L, h
    yield eng
    eng.close()


def ref_sample(row, ids, u, temperature, top_k, top_p, penalty, margin=1e-5):
    """float64 restatement of process_logits_and_sample (main.cpp:4753-4806) with the four literals as parameters (each narrowed to float first, as the engine
    holds them). Returns (id, near): near = the decision lies within `margin` of a boundary — the uniform against a cumulative-probability edge, a cumulative sum
    against 1 - top_p, or the k-th against the (k+1)-th tempered value relative to their magnitude — where float32 and float64 may legitimately part."""
    t, p, pen = float(f32(temperature)), float(f32(top_p)), float(f32(penalty))
    l = np.asarray(row, f32).astype(np.float64)
    ids = np.unique(np.asarray(ids, np.int64))
    g = l[ids]
    l[ids] = np.where(g < 0, g * pen, g / pen)
    l = l / t
    srt = np.sort(l)
    kth = srt[V - top_k]
    near = False
    if top_k < V:
        nxt = srt[V - top_k - 1]
        near |= abs(kth - nxt) <= margin * max(abs(kth), abs(nxt))
    keep = np.nonzero(l >= kth)[0]
    order = keep[np.argsort(l[keep], kind="stable")]  # ascending; everything else is exp(lowest) = 0 in front of it
    e = np.exp(l[order])
    cum = np.cumsum(e / e.sum())
    cut = 0.2 if f32(top_p) == f32(0.8) else 1.0 - p  # the reference's literal
    near |= bool((np.abs(cum[:-1] - cut) <= margin).any())
    masked = order[:-1][cum[:-1] <= cut]
    alive = np.setdiff1d(keep, masked)  # index order
    e = np.exp(l[alive])
    cum = np.cumsum(e / e.sum())
    near |= bool((np.abs(cum - u) <= margin).any())
    hit = np.nonzero(cum >= u)[0]
    return (int(alive[hit[0]]) if len(hit) else V - 1), near


def rows_of(rs, kind):
    row = (rs.randn(V) * rs.choice([0.5, 1.0, 2.0])).astype(f32)
    if kind == "peaky":  # a handful of logits far above the rest
        row[rs.randint(0, V, 6)] += f32(8)
    elif kind == "coarse":  # ties everywhere, also across the k-th place
        row = (np.round(row * 4) / 4).astype(f32)
    elif kind == "negative":
        row = -np.abs(row)
    return row


def test_defaults_are_the_parent_sampler(pkg, host):
    """(0.8, 50, 0.8, 2.0) through the explicit probe, both modes, is tts_host_sample_row; the five options set to their defaults leave tts_sample's ids and the RNG
    position alone; and 1 - 0.8f compares against a float sum exactly as the reference's literal 0.2 does."""
    rs = np.random.RandomState(101)
    for trial in range(60):
        row = rows_of(rs, ["gauss", "peaky", "coarse", "negative"][trial % 4])
        order = np.argsort(-row)
        ids = [np.array([1] * 17 + [8192]), order[rs.randint(0, 60, 1)], rs.randint(0, V, 3), order[:6]][trial % 4 if trial % 8 < 4 else rs.randint(4)]
        u = 0.0 if trial == 7 else float(rs.rand())
        want = pkg.host_sample_row(row, ids, u)
        for mode in (0, 1):
            assert pkg.host_sample_row_ex(row, ids, u, mode=mode, **DEFAULTS) == want, (trial, mode)
    logits = (rs.randn(5, V) * 2).astype(f32)
    ids = rs.randint(0, V, (5, 3)).astype(np.int32)
    host.seed(5)
    want, want_u = host.sample(logits, ids), host.rng_uniform()
    for k, v in DEFAULTS.items():
        host.set_option(OPTION_OF[k], v)
    host.set_option("ar_penalty_scope", 0)
    host.seed(5)
    assert (host.sample(logits, ids) == want).all() and host.rng_uniform() == want_u
    # the comparison: a float cumulative sum widened to double against 1.0 - (double)0.8f, for every float within 64 ulps of 0.2
    x = f32(0.2)
    for _ in range(64):
        x = np.nextafter(x, f32(0))
    cut = 1.0 - float(f32(0.8))
    for _ in range(129):
        assert (float(x) <= cut) == (float(x) <= 0.2), float(x)
        x = np.nextafter(x, f32(1))


GRID = [(t, k, p, pen, h) for t in (0.05, 0.5, 0.8, 1.0, 1.7, 4.0) for k in (1, 2, 49, 50, 51, 100, 101, 8194) for p in (0.05, 0.8, 1.0)
        for pen in (1.0, 1.3, 2.0, 10) for h in (0, 1, 4, 5, 60, 500)]


def test_fast_scan_equals_literal_over_the_grid(pkg):
    """Mode 0 (heap scan over overrides or a penalised copy, exact cut in the tempered domain, literal fallback) returns what mode 1 (the literal formulation)
    returns, for every grid point; the rows cycle through Gaussian, negative, coarse and near-tie rows (groups of logits 1-3 ulps apart around the k-th place)."""
    rs = np.random.RandomState(202)
    base = []
    for kind in ("gauss", "gauss", "negative", "coarse", "gauss", "negative"):
        row = rows_of(rs, kind)
        base.append((row, np.argsort(-row, kind="stable")))
    for n, (t, k, p, pen, h) in enumerate(GRID):
        row, order = base[n % len(base)]
        if n % 6 in (1, 5) and 4 <= k and k + 4 < V:  # near ties around the k-th place, on positive and on negative rows
            row = row.copy()
            v = row[order[k - 4]]
            for r in range(k - 3, k + 4):
                for _ in range(1 + (r + n) % 3):
                    v = np.nextafter(v, f32(-np.inf))
                row[order[r]] = v
        hist = np.concatenate([order[rs.randint(0, 70, h // 2)], rs.randint(0, V, h - h // 2)]).astype(np.int32)
        u = 0.0 if n % 97 == 0 else float(rs.rand())
        a = pkg.host_sample_row_ex(row, hist, u, t, k, p, pen, 0)
        b = pkg.host_sample_row_ex(row, hist, u, t, k, p, pen, 1)
        assert 0 <= b < V and a == b, (n, t, k, p, pen, h, a, b)


def test_literal_formulation_against_float64_restatement(pkg):
    """Mode 1 against ref_sample on random continuous rows with at most 50 survivors. A case is left out only within 1e-5 of a boundary (see ref_sample): each of
    the <= 50 + 49 + 1 windows is 2e-5 wide on a unit range or less, so random cases leave out a fraction of a per cent; the cap is 1 %."""
    rs = np.random.RandomState(303)
    n_cases, left_out = 1500, 0
    for n in range(n_cases):
        row = (rs.randn(V) * rs.choice([0.5, 1.0, 2.0])).astype(f32)
        t, k = float(rs.choice([0.3, 0.5, 0.8, 1.0, 1.7, 4.0])), int(rs.choice([1, 2, 5, 20, 49, 50]))
        p, pen = float(rs.choice([0.05, 0.5, 0.8, 0.8, 0.95, 1.0])), float(rs.choice([1.0, 1.3, 2.0, 10.0]))
        order = np.argsort(-row)
        h = int(rs.choice([0, 1, 4, 5, 60, 500]))
        hist = np.concatenate([order[rs.randint(0, 70, h // 2)], rs.randint(0, V, h - h // 2)]).astype(np.int32)
        u = float(f32(rs.rand()))
        want, near = ref_sample(row, hist, u, t, k, p, pen)
        if near:
            left_out += 1
            continue
        assert pkg.host_sample_row_ex(row, hist, u, t, k, p, pen, 1) == want, (n, t, k, p, pen, h)
    print("left out near a boundary: %d of %d" % (left_out, n_cases))
    assert left_out <= n_cases // 100, left_out


def test_list_path_returns_the_full_row_id_or_refuses(pkg):
    """tts_host_sample_prefiltered_ex: the list decides what the full row decides, or says -1. Raw lists (penalty scope 0: at most four distinct ids are looked up)
    and penalised lists (scope 1), keep from top_k to the list capacity. A penalised list of at least top_k + 14 entries (the device's keep window) always decides
    on continuous rows, whatever the history's size; a raw list refuses a 500-id history."""
    rs = np.random.RandomState(404)
    decided = refused = 0
    for n in range(600):
        kind = ["gauss", "gauss", "negative", "coarse", "peaky", "gauss"][n % 6]
        row = rows_of(rs, kind)
        t, k = float(rs.choice([0.05, 0.5, 0.8, 1.0, 1.7, 4.0])), int(rs.choice([1, 2, 20, 50, 80, 100]))
        p, pen = float(rs.choice([0.05, 0.8, 1.0])), float(rs.choice([1.0, 1.3, 2.0, 10.0]))
        order = np.argsort(-row)
        h = int(rs.choice([1, 2, 4, 5, 60, 500]))
        hist = np.concatenate([order[rs.randint(0, 70, h // 2)], rs.randint(0, V, h - h // 2)]).astype(np.int32)
        u = float(rs.rand())
        keep = int(rs.choice([k, min(128, k + 1), min(128, k + 14), 128]))
        want = pkg.host_sample_row_ex(row, hist, u, t, k, p, pen, 0)
        for ap in (0, 1):
            got = pkg.host_sample_prefiltered_ex(row, hist, u, t, k, p, pen, keep, ap)
            assert got in (want, -1), (n, ap, kind, t, k, p, pen, h, keep, got, want)
            decided += got == want
            refused += got == -1
            if ap == 1 and kind != "coarse" and keep >= k + 14 and t >= 0.5:  # (t = 0.05: exp overflows on some rows, the tail refuses and the literal decides)
                assert got == want, (n, kind, t, k, p, pen, h, keep)
            if ap == 0 and len(set(hist.tolist())) > 4:
                assert got == -1
    assert decided > 300 and refused > 100, (decided, refused)
    # the issue's pair: a 500-id history on a continuous row, top-k 50, the device's window
    row = (rs.randn(V) * 2).astype(f32)
    order = np.argsort(-row)
    hist = np.concatenate([order[:40], rs.randint(0, V, 460)]).astype(np.int32)
    want = pkg.host_sample_row_ex(row, hist, 0.37, mode=1, **DEFAULTS)
    assert pkg.host_sample_prefiltered_ex(row, hist, 0.37, keep=64, already_penalised=True, **DEFAULTS) == want
    assert pkg.host_sample_prefiltered_ex(row, hist, 0.37, keep=64, already_penalised=False, **DEFAULTS) == -1


def test_options_refuse_bad_values_and_keep_the_previous(pkg, host):
    rs = np.random.RandomState(505)
    logits = (rs.randn(3, V) * 2).astype(f32)
    ids = rs.randint(0, V, (3, 2)).astype(np.int32)
    good = {"ar_temperature": 1.3, "ar_top_k": 7, "ar_top_p": 0.6, "ar_repetition_penalty": 1.5, "ar_penalty_scope": 1}
    bad = {"ar_temperature": [0, -1, float("nan"), float("inf"), 1e-60, 1e60], "ar_top_k": [0, -3, 8195, 2.5, float("nan")],
           "ar_top_p": [0, -0.1, 1.0000001, float("nan"), 1e-60], "ar_repetition_penalty": [0.999, 0, -2, float("nan"), float("inf"), 1e60],
           "ar_penalty_scope": [-1, 2, 0.5, float("nan")]}
    try:
        for k, v in good.items():
            host.set_option(k, v)
        host.seed(9)
        want, want_u = host.sample(logits, ids), host.rng_uniform()
        row_wise = [pkg.host_sample_row_ex(logits[b], ids[b], 0.5, 1.3, 7, 0.6, 1.5, 0) for b in range(3)]
        assert all(0 <= r < V for r in row_wise)
        for k, vals in bad.items():
            for v in vals:
                assert host.L.tts_set_option(host.h, k.encode(), float(v)) == -1, (k, v)  # TTS_ERR_ARG
                assert k.encode() in host.L.tts_last_error(host.h)
        host.seed(9)
        assert (host.sample(logits, ids) == want).all() and host.rng_uniform() == want_u  # nothing moved
        # and the options are read: the defaults sample something else from these rows
        for k, v in DEFAULTS.items():
            host.set_option(OPTION_OF[k], v)
        host.seed(9)
        other = host.sample(logits, ids)
        assert host.rng_uniform() == want_u  # two uniforms per candidate whatever the controls
        host.seed(9)
        u = [(host.rng_uniform(), host.rng_uniform())[1] for _ in range(3)]
        assert [pkg.host_sample_row_ex(logits[b], ids[b], u[b], 1.3, 7, 0.6, 1.5, 1) for b in range(3)] == list(want)
        assert [pkg.host_sample_row_ex(logits[b], ids[b], u[b], mode=1, **DEFAULTS) for b in range(3)] == list(other)
    finally:
        for k, v in DEFAULTS.items():
            host.set_option(OPTION_OF[k], v)
        host.set_option("ar_penalty_scope", 0)


def test_cli_usage_errors_before_any_model_loads(tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    models = os.path.join(ROOT, "models")
    base = [exe, "--dry-run", "1", "--models", models, "--voice", os.path.join(models, "mol.bin"), "--seed", "11", "--codes", "5", "--candidates", "2",
            "--output", str(tmp_path / "o.wav")]
    run = lambda extra: subprocess.run(base + extra + ["--timing", "1"], capture_output=True, text=True, timeout=120)
    for extra in (["--temperature", "0"], ["--temperature", "nan"], ["--top-k", "0"], ["--top-k", "8195"], ["--top-k", "2.5"], ["--top-p", "0"], ["--top-p", "1.5"],
                  ["--repetition-penalty", "0.5"], ["--penalty-scope", "all"], ["--devices", "2", "--top-p", "7"]):
        r = run(extra)
        assert r.returncode == 1 and extra[-2] in r.stderr and "[timing]" not in r.stderr, (extra, r.stderr)
    r = run(["--temperature", "1.25", "--top-k", "80", "--top-p", "0.9", "--repetition-penalty", "1.5", "--penalty-scope", "history", "--devices", "2"])
    assert r.returncode == 0, r.stdout + r.stderr
    echoed = [l for l in r.stderr.splitlines() if l.startswith("[timing] ar sampler")]
    assert echoed == ["[timing] ar sampler temperature 1.25, top-k 80, top-p 0.9, repetition-penalty 1.5, penalty-scope history"] * 2, r.stderr
    r = run([])
    assert r.returncode == 0 and "[timing] ar sampler temperature 0.8, top-k 50, top-p 0.8, repetition-penalty 2, penalty-scope last\n" in r.stderr, r.stderr
