"""CPU side of tests/test_gn_kernels_gpu.py: the harness library builds for gfx950, loads and exports its surface; it refuses every invalid case before any HIP
call; the float64 reference is checked against torch and naive loops; a correct float32 implementation of every reduction form passes the acceptance rule on
every case of the matrix (the bound is not too tight); and every mutation of the reference leaves the acceptance interval of some element by at least 10 x its
tolerance on a case built to expose it (the bound is sharp). Which case catches which mutation is printed (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import gn_cases as G
from gn_cases import APPLY, AUTO, FUSED, GATHER_F16, GATHER_F32, REG512, REG1024, STATS, STATS_APPLY_F32, TO_F16, CH


def test_harness_library_builds_and_exports_its_surface():
    L = G.harness()  # builds it once if missing; raises otherwise
    for sym in ("tts_gn_test_run", "tts_gn_test_validate", "tts_gn_test_margin", "tts_gn_test_class"):
        assert hasattr(L, sym), sym
    assert L.tts_gn_test_margin() == 4096
    src_t = max(os.path.getmtime(G.SRC), os.path.getmtime(os.path.join(G.PKG, "csrc", "diffusion.hip")))
    assert os.path.getmtime(G.LIB) >= src_t or os.environ.get("TTS_GN_TEST_LIB"), "libtts_gn_test.so is older than its sources: run make"


def test_dispatch_thresholds_come_from_the_product():
    L = G.harness()
    assert [L.tts_gn_test_class(t) for t, _ in G.AUTO_LENGTHS] == [c for _, c in G.AUTO_LENGTHS] == [0, 1, 1, 2]
    assert L.tts_gn_test_class(1) == 0
    # the largest length of each explicit class of the matrix is the capacity NJ * NT / 8 of that class, and the class gn_class names for it
    for kind in (REG512, REG1024):
        cl = G.CLASS[kind]
        cap = cl["NJ"] * cl["NT"] // 8
        assert max(G.LENGTHS[kind]) == cap and L.tts_gn_test_class(cap) == kind and L.tts_gn_test_class(cap + 1) == kind + 1


def test_harness_is_not_part_of_the_product():
    mk = open(os.path.join(G.PKG, "Makefile")).read()
    assert "HIP_SRCS = $(wildcard csrc/*.hip)" in mk and not os.path.exists(os.path.join(G.PKG, "csrc", "diff_gn_harness.hip"))
    link = [l for l in mk.splitlines() if "-o $@ $(OBJS)" in l]
    assert len(link) == 1 and "testlib" not in link[0] and "gn_test" not in link[0]
    src = open(G.SRC).read()
    assert '#include "../csrc/diffusion.hip"' in src and "asm" not in src and "__global__" not in src  # the product's kernels, none of its own


# ---------------------------------------------------------------------------------------------------------------- validation (no HIP call is reached)

def _valid_case(kind):
    """A small valid case of every kind, as keyword arguments of G.struct()."""
    f32, i32 = np.float32, np.int32
    rows = 32
    kw = dict(kind=kind, ns=2, rows_total=rows, x_rows=rows, row0=0, x=np.zeros((rows, CH), f32), start=np.array([8, 16], i32), len=np.array([5, 7], i32),
              eps=1e-6, out=G.Guarded((rows, CH), np.uint16))
    if kind in (GATHER_F16, GATHER_F32):
        return dict(kind=kind, rows_total=rows, x_rows=8, x=np.zeros((8, CH), f32), src_row=np.array([-1, 7] * 16, i32),
                    out=G.Guarded((rows, CH), np.uint16 if kind == GATHER_F16 else f32))
    if kind == STATS:
        kw["out"] = G.Guarded((2, 32, 2), f32)
        return kw
    if kind == TO_F16:
        return kw
    kw.update(g=np.ones(CH, f32), b=np.zeros(CH, f32))
    if kind == STATS_APPLY_F32:
        kw.update(ss=np.zeros((3, 2 * CH), f32), n_steps=3, seq_voice=np.array([2, 0], i32), out=G.Guarded((rows, CH), f32))
        return kw
    kw.update(ss=np.zeros(2 * 2112 + 2 * CH, f32), n_steps=3, ss_step_stride=2112, seq_step=np.array([2, 0], i32), do_silu=1, lut=2,
              pf0=np.zeros(1280, np.uint8), pf0_bytes=1280, pf0_lines=10, pf1=np.zeros(128, np.uint8), pf1_bytes=128, pf1_lines=1)
    if kind == APPLY:
        kw["st"] = np.zeros((8, 2, 32, 4), np.int64)
    return kw


ALL_KINDS = [REG512, REG1024, FUSED, AUTO, STATS, STATS_APPLY_F32, APPLY, TO_F16, GATHER_F16, GATHER_F32]


def _rc(kw, run=True):
    kw = dict(kw)
    cs = G.struct(kw.pop("kind"), **kw)
    L = G.harness()
    rc = L.tts_gn_test_validate(C.byref(cs))
    if rc != 0 and run:  # an invalid case is refused by the run entry too, before any HIP call (this machine has no GPU: a HIP call would return another code)
        assert L.tts_gn_test_run(C.byref(cs)) == G.HIP_INVALID_VALUE
    return rc


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_valid_cases_validate(kind):
    assert _rc(_valid_case(kind), run=False) == 0


def test_null_case_is_refused():
    L = G.harness()
    assert L.tts_gn_test_validate(None) == G.HIP_INVALID_VALUE and L.tts_gn_test_run(None) == G.HIP_INVALID_VALUE


i32 = np.int32
INVALID = [
    ("unknown kind", REG512, dict(kind=10)), ("kind < 0", REG512, dict(kind=-1)),
    ("start not a multiple of 8", REG512, dict(start=np.array([8, 17], i32))), ("start not a multiple of 8 stats", STATS, dict(start=np.array([4, 16], i32))),
    ("starts out of order", REG1024, dict(start=np.array([16, 8], i32))), ("start < 0", FUSED, dict(start=np.array([-8, 16], i32))),
    ("no guard row between sequences", REG512, dict(len=np.array([8, 7], i32))), ("sequences overlap", APPLY, dict(len=np.array([9, 7], i32))),
    ("no guard row behind the last sequence", REG512, dict(len=np.array([5, 16], i32))), ("last sequence past the rows", TO_F16, dict(len=np.array([5, 17], i32))),
    ("len 0", REG512, dict(len=np.array([0, 7], i32))), ("len < 0", STATS, dict(len=np.array([5, -1], i32))),
    ("len overflow", FUSED, dict(len=np.array([5, 2 ** 31 - 1], i32))),
    ("rows not a multiple of 8", REG512, dict(rows_total=28, x_rows=28)), ("rows not a multiple of 4 apply", APPLY, dict(rows_total=30, x_rows=30)),
    ("rows 0", STATS, dict(rows_total=0, x_rows=0)), ("rows > 8192", TO_F16, dict(rows_total=8200, x_rows=8200)),
    ("apply rows > 2048", APPLY, dict(rows_total=2052, x_rows=2052)),
    ("ns 0", REG512, dict(ns=0)), ("ns 65", REG512, dict(ns=65)),
    ("len above the class capacity 512", REG512, dict(rows_total=1024, x_rows=1024, start=np.array([8, 32], i32), len=np.array([5, 897], i32))),
    ("len above the class capacity 1024", REG1024, dict(rows_total=4096, x_rows=4096, start=np.array([8, 32], i32), len=np.array([5, 2305], i32))),
    ("part past the buffers", REG512, dict(row0=8)), ("part offset not a multiple of 8", REG1024, dict(row0=4, x_rows=40)),
    ("part offset < 0", FUSED, dict(row0=-8)), ("part on a kernel gn_fused does not launch", APPLY, dict(row0=8, x_rows=40)),
    ("x_rows > 8192", AUTO, dict(x_rows=8200)),
    ("seq_step out of the table", REG512, dict(seq_step=np.array([3, 0], i32))), ("seq_step < 0", APPLY, dict(seq_step=np.array([0, -1], i32))),
    ("seq_step without ss", FUSED, dict(ss=None)), ("table of 0 rows", REG512, dict(n_steps=0)), ("table of 65 rows", REG512, dict(n_steps=65)),
    ("stride < 0", REG1024, dict(ss_step_stride=-1)), ("table without seq_step", REG512, dict(seq_step=None)),
    ("seq_voice out of the table", STATS_APPLY_F32, dict(seq_voice=np.array([0, 3], i32))), ("seq_voice < 0", STATS_APPLY_F32, dict(seq_voice=np.array([-1, 0], i32))),
    ("no voice table", STATS_APPLY_F32, dict(ss=None)), ("voice table of 0 rows", STATS_APPLY_F32, dict(n_steps=0)),
    ("touch lines past the buffer", REG512, dict(pf0_lines=11)), ("touch lines past the second buffer", APPLY, dict(pf1_lines=2)),
    ("touch lines < 0", REG1024, dict(pf0_lines=-1)), ("touch lines without a buffer", REG512, dict(pf1=None)), ("touch bytes < 0", REG512, dict(pf0_bytes=-128, pf0_lines=0)),
    ("touch lines overflow", REG512, dict(pf0_lines=2 ** 31 - 1)),
    ("lut 3", REG512, dict(lut=3)), ("lut < 0", APPLY, dict(lut=-1)), ("do_silu 2", FUSED, dict(do_silu=2)),
    ("no x", REG512, dict(x=None)), ("no x stats", STATS, dict(x=None)), ("no out", FUSED, dict(out=None)), ("no out gather", GATHER_F32, dict(out=None)),
    ("no g", REG1024, dict(g=None)), ("no b", STATS_APPLY_F32, dict(b=None)), ("no start", TO_F16, dict(start=None)), ("no len", STATS, dict(len=None)),
    ("no statistics", APPLY, dict(st=None)), ("no src_row", GATHER_F16, dict(src_row=None)),
    ("src_row past the source", GATHER_F16, dict(src_row=np.array([-1, 8] * 16, i32))), ("src_row < -1", GATHER_F32, dict(src_row=np.array([-2, 7] * 16, i32))),
    ("gather source of 0 rows", GATHER_F32, dict(x_rows=0)),
]


@pytest.mark.parametrize("name,kind,change", INVALID, ids=[i[0].replace(" ", "_") for i in INVALID])
def test_invalid_cases_are_refused_before_any_launch(name, kind, change):
    kw = _valid_case(kind)
    kw.update(change)
    assert _rc(kw) == G.HIP_INVALID_VALUE


# ---------------------------------------------------------------------------------------------------------------- reference

def test_reference_against_torch_float64():
    import torch
    for kind, lens, cfg in ((REG512, [5, 1, 9], G.CONFIGS[0]), (FUSED, [33], G.CONFIGS[5])):
        c = G.Case(kind, lens, cfg)
        ref = G.reference(c)
        for s in range(c.lay.ns):
            xs = torch.from_numpy(c.x[c.lay.seq_rows(s)].astype(np.float64))  # [T][1024] -> [1][1024][T]
            t = torch.nn.functional.group_norm(xs.t()[None], 32, torch.from_numpy(c.g.astype(np.float64)), torch.from_numpy(c.b.astype(np.float64)), eps=float(np.float32(c.eps)))
            want = t[0].t().numpy()
            assert np.abs(ref["z"][c.lay.seq_rows(s)] - want).max() <= 1e-11 * np.abs(want).max()
        assert (ref["z"][~c.lay.row_mask()] == 0).all()


def test_reference_against_naive_loops():
    c = G.triple(REG512, G.CONFIGS[1])  # scale / shift rows (2, 0, 1), 2112 floats apart, SiLU
    ref = G.reference(c)
    x = c.x.astype(np.float64)
    for s, row in ((0, 2), (1, 0), (2, 1)):
        T, r0 = int(c.lay.len[s]), int(c.lay.start[s])
        for grp in (0, 1, 2, 3, 17, 31):
            vals = [x[r0 + t, grp * 32 + i] for t in range(T) for i in range(32)]
            mean = sum(vals) / len(vals)
            var = sum((v - mean) ** 2 for v in vals) / len(vals)
            for t in (0, T // 2, T - 1):
                for i in (0, 13, 31):
                    ch = grp * 32 + i
                    u = (x[r0 + t, ch] - mean) / np.sqrt(var + float(np.float32(1e-5))) * float(c.g[ch]) + float(c.b[ch])
                    u = u * (float(c.ss[row * 2112 + ch]) + 1.0) + float(c.ss[row * 2112 + CH + ch])
                    want = u / (1.0 + np.exp(-u))
                    assert abs(ref["z"][r0 + t, ch] - want) <= 1e-12 * max(1.0, abs(want))


def test_silu_interval_logic():
    assert abs(G.X_MIN + 1.2784645) < 1e-6
    xs = np.linspace(-3, 1, 4001)
    assert abs(xs[np.argmin(G.silu(xs))] - G.X_MIN) <= 1e-3 and G.silu(G.X_MIN) <= G.silu(xs).min()
    lo, hi = G.silu_image(np.array([-2.0, -1.0, -5.0, 0.5]), np.array([-1.0, 0.0, -4.0, 0.75]))
    assert lo[0] == G.silu(G.X_MIN) and hi[0] == max(G.silu(-2.0), G.silu(-1.0))  # the minimum is inside: neither end point is the lower end
    assert (lo[1], hi[1]) == (G.silu(-1.0), G.silu(0.0)) and (lo[2], hi[2]) == (G.silu(-4.0), G.silu(-5.0)) and (lo[3], hi[3]) == (G.silu(0.5), G.silu(0.75))
    for a, b in ((-2.0, -1.0), (-1.3, -1.2), (-30.0, 30.0)):  # the image contains every value of the interval
        l, h = G.silu_image(np.array([a]), np.array([b]))
        v = G.silu(np.linspace(a, b, 1001))
        assert l[0] <= v.min() and v.max() <= h[0]
    assert G.silu(-800.0) == 0 and G.silu(800.0) == 800.0 and np.isfinite(G.silu_rel(np.array([-800.0, 800.0]))).all()
    assert (G.rn16(np.array([65520.0, 2049.0, 2051.0, 1e-8])) == np.array([np.inf, 2048.0, 2052.0, 0.0])).all()  # ties to even
    assert (G.ulp16(np.array([1.0, 1.5, 2.0 ** -14, 1e-7, 0.0])) == np.array([2.0 ** -10, 2.0 ** -10, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24])).all()


def test_fx_split_restatement_is_exact():
    p = np.array([0.0, 1.0, -1.0, 3.14159274, 1e-3, -123456.789, 2.0 ** 30, 5e-9], np.float32)
    hi, lo = G.fx_split(p)
    # The split itself loses nothing: hi 2^-8 + lo 2^-52 is p. (gemm_f16.h's fx_value reads lo in units of 2^-60, so the remainder, at most 2^-9 per partial sum,
    # reaches gn_apply_kernel divided by 256; stripes() decodes the integers as fx_value does, because the kernel takes its statistics as given.)
    assert (hi.astype(np.float64) / 256.0 + lo.astype(np.float64) / 2.0 ** 52 == p.astype(np.float64)).all()
    assert (np.abs(lo) <= 2.0 ** 43).all()
    c = G.single(APPLY, 9, G.CONFIGS[0])
    st, mean, var = G.stripes(c)
    m, v = G.reference(c)["mean"], G.reference(c)["var"]
    assert np.abs(mean - m).max() <= 1e-4 and (np.abs(var - v) <= 1e-4 * (1.0 + v + m * m)).all()  # f32 parts of the exact sums, less 255/256 of each remainder
    assert (st[3] == 0).all() and len({int(np.abs(st[k, :, :, 0]).sum()) for k in range(8)}) == 8  # unevenly spread, one stripe untouched


# ---------------------------------------------------------------------------------------------------------------- the bound is not too tight

def _given(c):
    if c.kind != APPLY:
        return None, None
    st, mean, var = G.stripes(c)
    return st, (mean, var)


def _check_restatement(c):
    _, given = _given(c)
    ref = G.reference(c, given=given)
    z, mean, rstd = G.f32_restatement(c, given)
    if c.kind == STATS:
        zz, lo, hi = G.stats_interval(c, ref)
        ok = G.accept32(np.stack([mean, rstd], axis=2), lo, hi)
    elif c.kind == STATS_APPLY_F32:
        lo, hi = G.interval(c, ref)
        ok = G.accept32(z, lo, hi)
    else:
        lo, hi = G.interval(c, ref)
        assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()
        ok = G.accept16(z.astype(np.float16).view(np.uint16), lo, hi)
    assert ok.all(), (c.name(), int((~ok).sum()), np.argwhere(~ok)[:4].tolist())


MATRIX = [(k, T) for k in (REG512, REG1024, FUSED, STATS, APPLY) for T in G.LENGTHS[k]] + [(STATS_APPLY_F32, T) for T in G.LENGTHS[STATS]]


@pytest.mark.parametrize("kind,T", MATRIX, ids=["%s-T%d" % (G.KIND_NAMES[k].replace(" ", ""), T) for k, T in MATRIX])
def test_f32_restatement_passes_every_case(kind, T):
    for cfg in G.configs(kind, T):
        _check_restatement(G.single(kind, T, cfg))


@pytest.mark.parametrize("kind", [REG512, REG1024, FUSED, STATS, STATS_APPLY_F32, APPLY])
def test_f32_restatement_passes_the_three_sequence_layouts(kind):
    for cfg in G.configs(kind):
        _check_restatement(G.triple(kind, cfg))


def test_outlier_pivot_bound_is_finite_and_recorded():
    """The one-pass kernels with the pivot on the outlier at the longest length of the matrix: the bound's relative variance error stays below 1 while a
    two-pass kernel's is 1e-6, and the f32 one-pass restatement's observed error is inside it."""
    c = G.single(FUSED, 2305, G.CONFIGS[0])
    ref = G.reference(c)
    xs = c.x.astype(np.float64)[c.lay.seq_rows(0)]
    grp = [f for f, _, _ in c.plans[0]].index("outlier-pivot")
    _, _, rho = G.stat_bounds(FUSED, xs, ref["mean"][0], ref["var"][0], 1e-6, 2305)
    _, _, rho2 = G.stat_bounds(REG1024, xs[:2304], *G.group_stats(xs[:2304]), 1e-6, 2304)
    _, _, rstd = G.f32_restatement(c)
    seen = abs((1.0 / float(rstd[0, grp]) ** 2 - 1e-6) / ref["var"][0, grp] - 1.0)
    print("outlier-pivot T=2305: bound on the relative variance error %.3g (two-pass at 2304: %.3g), f32 one-pass restatement %.3g" % (rho[grp], rho2[grp], seen))
    assert 0.1 < rho[grp] < 0.9 and rho2[grp] < 1e-5 and seen <= rho[grp]
    assert rho[[i for i in range(32) if i != grp]].max() < 1e-3  # every other placement has an ordinary pivot


# ---------------------------------------------------------------------------------------------------------------- the bound is sharp

def _moved(c, mut, ref=None, iv=None, given=None):
    """max over elements of |mutated reference - reference| / (half-width + one fp16 ulp), and the group of the element"""
    ref = ref or G.reference(c, given=given)
    m = G.reference(c, mut=mut, given=given)
    if c.kind == STATS:
        z, lo, hi = iv or G.stats_interval(c, ref)
        r = G.excess(np.stack([m["mean"], m["r"]], axis=2), z, lo, hi, False)
        i = np.unravel_index(np.argmax(r), r.shape)
        return float(r[i]), int(i[1])
    lo, hi = iv or G.interval(c, ref)
    r = G.excess(m["z"], ref["z"], lo, hi, c.kind != STATS_APPLY_F32)
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), int(i[1]) // 32


STRUCT_MATRIX = [(k, T) for k in (REG512, REG1024, FUSED, STATS) for T in G.LENGTHS[k]]


@pytest.mark.parametrize("kind,T", STRUCT_MATRIX, ids=["%s-T%d" % (G.KIND_NAMES[k], T) for k, T in STRUCT_MATRIX])
def test_spike_placements_catch_every_structural_mutation_at_every_length(kind, T):
    c = G.single(kind, T, G.configs(kind)[0])
    ref = G.reference(c)
    iv = G.stats_interval(c, ref) if kind == STATS else G.interval(c, ref)
    for mut in G.STRUCTURAL:
        if G.mutation_rows(mut, kind, T) is None or (mut == "drop_last" and T == 1):  # a sequence of one row without its row has no statistics at all
            continue
        r, grp = _moved(c, mut, ref, iv)
        print("%-24s T=%-5d %-16s moves group %2d (%s) by %.3g x its tolerance" % (G.KIND_NAMES[kind], T, mut, grp, c.plans[0][grp][0], r))
        assert r >= 10.0, (mut, r)


def _targets(kind):
    """mutation -> the cases of the matrix built to expose it"""
    cf = G.configs(kind)
    small = [T for T in G.LENGTHS[STATS if kind == STATS_APPLY_F32 else kind] if T <= 129]
    plain = [G.single(kind, T, cf[0]) for T in small]
    t = {"n_plus": plain[:2], "n_minus": [G.single(kind, 2, cf[0])] if kind == REG512 else [G.single(kind, small[1], cf[0])], "unbiased": plain[:1],
         "eps_outside": plain[:3], "eps_wrong": [G.single(kind, T, cfg) for T in small[:2] for cfg in cf[:2]], "group_plus": plain[-1:], "group_minus": plain[-1:]}
    if kind == APPLY:  # the statistics are an input: only the kernel's own use of them can be wrong
        t = {k: v for k, v in t.items() if k in ("eps_outside", "eps_wrong", "group_plus", "group_minus")}
    if kind == STATS:
        return t
    tri = G.triple(kind, cf[1] if kind != STATS_APPLY_F32 else cf[0])
    t.update({"scale_no_plus1": [tri], "ss_swapped": [tri], "voice_other" if kind == STATS_APPLY_F32 else "seq_step_other": [tri]})
    if kind != STATS_APPLY_F32:
        t["silu_missing"] = [tri, G.triple(kind, cf[2])]
        t["silu_wrong_mode"] = [G.triple(kind, cf[4]), G.triple(kind, cf[2])]
    return t


@pytest.mark.parametrize("kind", [REG512, REG1024, FUSED, STATS, STATS_APPLY_F32, APPLY])
def test_every_other_mutation_is_caught(kind):
    tg = _targets(kind)
    want = set(G.MUTATIONS) - set(G.STRUCTURAL)
    if kind == STATS:
        want -= {"scale_no_plus1", "ss_swapped", "seq_step_other", "voice_other", "silu_missing", "silu_wrong_mode"}
    elif kind == STATS_APPLY_F32:
        want -= {"seq_step_other", "silu_missing", "silu_wrong_mode"}
    else:
        want -= {"voice_other"}
    if kind == APPLY:
        want -= {"n_plus", "n_minus", "unbiased"}
    assert set(tg) == want  # no mutation of this kernel is left without a case
    for mut in sorted(tg):
        best = (0.0, None, None)
        for c in tg[mut]:
            _, given = _given(c)
            r, grp = _moved(c, mut, given=given)
            if r > best[0]:
                best = (r, c, grp)
        r, c, grp = best
        print("%-40s %-16s caught by %s, group %s: %.3g x its tolerance" % (G.KIND_NAMES[kind], mut, c.name() if c else None, grp, r))
        assert r >= (1.0 if mut == "silu_wrong_mode" else 10.0), (mut, r)  # silu_wrong_mode: see gn_cases.py, SHARPNESS
