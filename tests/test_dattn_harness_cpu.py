"""CPU side of tests/test_dattn_kernels_gpu.py: the harness library builds for gfx950, loads and exports its surface; it refuses every violation of the kernels'
memory contract before any HIP call; the float64 reference is checked against naive loops; the lengths of the matrix reach every (tile, wave) class; a NumPy
restatement of each kernel's arithmetic passes the bound on every case of the matrix (the bound is not too tight); and every mutation of the reference moves some
element of a case built to expose it by at least 10 x its bound (the bound is sharp). Which case catches which mutation is printed (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import dattn_cases as D
from dattn_cases import F16_Q128, F16_Q64, F32, CH, NH


def test_harness_library_builds_and_exports_its_surface():
    L = D.harness()  # builds it once if missing; raises otherwise
    for sym in ("tts_dattn_test_run", "tts_dattn_test_validate", "tts_dattn_test_margin"):
        assert hasattr(L, sym), sym
    assert L.tts_dattn_test_margin() == 4096
    src_t = max(os.path.getmtime(D.SRC), os.path.getmtime(os.path.join(D.PKG, "csrc", "diffusion.hip")))
    assert os.path.getmtime(D.LIB) >= src_t or os.environ.get("TTS_DATTN_TEST_LIB"), "libtts_dattn_test.so is older than its sources: run make"


def test_harness_is_not_part_of_the_product():
    mk = open(os.path.join(D.PKG, "Makefile")).read()
    assert "HIP_SRCS = $(wildcard csrc/*.hip)" in mk and not os.path.exists(os.path.join(D.PKG, "csrc", "diff_attn_harness.hip"))
    link = [l for l in mk.splitlines() if "-o $@ $(OBJS)" in l]
    assert len(link) == 1 and "testlib" not in link[0] and "dattn_test" not in link[0]
    src = open(D.SRC).read()
    assert '#include "../csrc/diffusion.hip"' in src and "asm" not in src and "__global__" not in src  # the product's kernels, none of its own
    rule = [l for l in mk.splitlines() if "testlib/diff_attn_harness.hip" in l and "$(HIPCC)" in l]
    assert len(rule) == 1 and "-mllvm -amdgpu-mfma-vgpr-form" in rule[0] and "$(PK)" in rule[0] and "csrc/host_logic.cpp" in rule[0]  # the flags of csrc/diffusion.o
    assert all("libtts_dattn_test.so" in l for l in mk.splitlines() if l.startswith("all:") or l.startswith("\trm -f"))


# ---------------------------------------------------------------------------------------------------------------- validation (no HIP call is reached)

def _valid_case(kind):
    """A small valid case, as keyword arguments of D.struct(): two sequences of 5 and 7 rows in a layout of 128."""
    rows = 128
    z16 = lambda *s: np.zeros(s, np.uint16)
    return dict(kind=kind, ns=2, rows=rows, ldvt=rows + 128, qk_rows=rows + 128, out_rows=rows + 2, start=np.array([8, 16], np.int32), len=np.array([5, 7], np.int32),
                qk=z16(rows + 128, 2048), vt=z16(CH, rows + 128), qk_lo=z16(rows + 128, 2048) if kind == F32 else None, vt_lo=z16(CH, rows + 128) if kind == F32 else None,
                bias_tab=np.zeros((NH, 128), np.float32), out=D.Guarded((rows + 2, CH), np.uint16), out_lo=D.Guarded((rows + 2, CH), np.uint16) if kind == F32 else None)


def _rc(kw, run=True, check=True):
    kw = dict(kw)
    cs = D.struct(kw.pop("kind"), _check=check, **kw)
    L = D.harness()
    rc = L.tts_dattn_test_validate(C.byref(cs))
    if rc != 0 and run:  # an invalid case is refused by the run entry too, before any HIP call (this machine has no GPU: a HIP call would return another code)
        assert L.tts_dattn_test_run(C.byref(cs)) == D.HIP_INVALID_VALUE
    return rc


@pytest.mark.parametrize("kind", D.KINDS)
def test_valid_cases_validate(kind):
    assert _rc(_valid_case(kind), run=False) == 0


@pytest.mark.parametrize("kind", D.KINDS)
def test_every_case_of_the_matrix_layouts_validates(kind):
    """the layouts the GPU tests launch, by the harness's own rule (host only)"""
    for lens in [[T] for T in D.LENGTHS] + [list(t) for t in D.TRIPLES] + [list(D.EIGHT)]:
        lay = D.Lay(lens)
        kw = _valid_case(kind)
        kw.update(ns=lay.ns, rows=lay.rows, ldvt=lay.rows + 128, qk_rows=lay.rows + 128, out_rows=lay.rows + 2, start=lay.start, len=lay.len)
        assert _rc(kw, run=False, check=False) == 0, lens


def test_null_case_is_refused():
    L = D.harness()
    assert L.tts_dattn_test_validate(None) == D.HIP_INVALID_VALUE and L.tts_dattn_test_run(None) == D.HIP_INVALID_VALUE


i32 = lambda *a: np.array(a, np.int32)
INVALID = [
    ("unknown kind", F16_Q128, dict(kind=3)), ("kind < 0", F16_Q128, dict(kind=-1)),
    ("ns 0", F16_Q128, dict(ns=0)), ("ns 9", F16_Q64, dict(ns=9)), ("ns < 0", F32, dict(ns=-1)),
    ("rows 0", F16_Q128, dict(rows=0, ldvt=128, qk_rows=128, out_rows=2)),
    ("rows not a multiple of 128", F16_Q128, dict(rows=120, ldvt=248, qk_rows=248, out_rows=122)),
    ("rows not a multiple of 128 f32", F32, dict(rows=136, ldvt=264, qk_rows=264, out_rows=138)),
    ("rows > 4096", F16_Q64, dict(rows=4224, ldvt=4352, qk_rows=4352, out_rows=4226)),
    ("ldvt too small", F16_Q128, dict(ldvt=248)), ("ldvt is the layout's rows", F32, dict(ldvt=128)), ("ldvt too large", F16_Q64, dict(ldvt=264)),
    ("qk without its 128 slack rows", F16_Q128, dict(qk_rows=128)), ("qk too small", F32, dict(qk_rows=248)),
    ("out without its two halo rows", F16_Q128, dict(out_rows=128)), ("out one row short", F32, dict(out_rows=129)),
    ("start not a multiple of 8", F16_Q128, dict(start=i32(8, 17))), ("first start not a multiple of 8", F32, dict(start=i32(9, 16))),
    ("first start < 8", F16_Q128, dict(start=i32(0, 16))), ("start < 0", F16_Q64, dict(start=i32(-8, 16))),
    ("starts out of order", F16_Q128, dict(start=i32(16, 8))),
    ("no guard row between sequences", F16_Q128, dict(len=i32(8, 7))), ("sequences overlap", F32, dict(len=i32(9, 7))),
    ("no guard row behind the last sequence", F16_Q128, dict(len=i32(5, 112))), ("last sequence past the rows", F16_Q64, dict(len=i32(5, 113))),
    ("len 0", F16_Q128, dict(len=i32(0, 7))), ("len < 0", F32, dict(len=i32(5, -1))), ("len overflow", F16_Q64, dict(len=i32(5, 2 ** 31 - 1))),
    ("start overflow", F16_Q128, dict(start=i32(8, 2 ** 31 - 8))),
    ("no qk", F16_Q128, dict(qk=None)), ("no vt", F16_Q64, dict(vt=None)), ("no bias table", F16_Q128, dict(bias_tab=None)), ("no out", F32, dict(out=None)),
    ("no start", F16_Q128, dict(start=None)), ("no len", F32, dict(len=None)),
    ("no qk_lo for the split kernel", F32, dict(qk_lo=None)), ("no vt_lo for the split kernel", F32, dict(vt_lo=None)),
    ("no out_lo for the split kernel", F32, dict(out_lo=None)),
]


@pytest.mark.parametrize("name,kind,change", INVALID, ids=[i[0].replace(" ", "_") for i in INVALID])
def test_invalid_cases_are_refused_before_any_launch(name, kind, change):
    kw = _valid_case(kind)
    kw.update(change)
    assert _rc(kw, check=False) == D.HIP_INVALID_VALUE


def test_images_put_every_operand_where_the_kernels_read_it():
    c = D.triple(D.TRIPLES[0], ("flat", "sharp"))
    lay = c.lay
    assert lay.rows % 128 == 0 and lay.start[0] == 8 and (lay.start % 8 == 0).all() and (lay.start[1:] >= lay.start[:-1] + lay.len[:-1] + 1).all()
    for poison in (False, True):
        im = c.images(poison)
        assert im["qk"].shape == (lay.rows + 128, 2048) and im["vt"].shape == (CH, lay.rows + 128)
        for s, sq in enumerate(c.seqs):
            r0 = int(lay.start[s])
            for h, t, d in ((0, 0, 0), (3, sq.T - 1, 63), (15, sq.T // 2, 17)):
                assert im["qk"][r0 + t, h * 128 + d] == D.bits(sq.qh[h, t, d]) and im["qk"][r0 + t, h * 128 + 64 + d] == D.bits(sq.kh[h, t, d])
                assert im["vt"][h * 64 + d, r0 + t] == D.bits(sq.vh[h, t, d]) and im["vt_lo"][h * 64 + d, r0 + t] == D.bits(sq.vl[h, t, d])
                assert im["qk_lo"][r0 + t, h * 128 + 64 + d] == D.bits(sq.kl[h, t, d])
            guard = im["qk"][r0 + sq.T].view(np.float16).astype(np.float64)
            assert (np.abs(guard) == D.POISON).all() if poison else (guard.reshape(NH, 2, 64)[:, 1] == sq.kh[:, sq.T]).all()
        out = ~lay.row_mask()
        vals = np.abs(im["qk"].view(np.float16).astype(np.float64))
        assert np.isfinite(vals).all() and (vals[lay.rows:] == (D.POISON if poison else 0.0)).all()  # the 128 slack rows
        if poison:
            assert (vals[:lay.rows][out] == D.POISON).all() and (np.abs(im["vt"].view(np.float16).astype(np.float64))[:, :lay.rows][:, out] == D.POISON).all()
        for a in im.values():  # no fp16 subnormal anywhere
            v = np.abs(a.view(np.float16).astype(np.float64))
            assert ((v == 0) | (v >= 2.0 ** -14)).all()


# ---------------------------------------------------------------------------------------------------------------- reference

def test_reference_against_naive_loops():
    for T, cfg, f32 in ((17, ("flat", "sharp"), False), (130, ("wide", "sharp"), True), (130, ("flat", "smooth"), False)):
        c = D.single(T, cfg)
        sq = c.seqs[0]
        ref = D.reference(sq, c.bias, f32)["out"]
        q, k, v = sq.operands(f32)
        for h, t in ((0, 0), (5, T - 1), (15, T // 2), (9, min(T - 1, 64))):
            sc = []
            for j in range(T):
                dot = sum(float(q[h, t, i]) * float(k[h, j, i]) for i in range(64))
                sc.append(dot / 8.0 + float(c.bias[h, (64 if j > t else 0) + min(abs(j - t), 63)]))
            mx = max(sc)
            w = [np.exp(x - mx) for x in sc]
            tot = sum(w)
            for d in (0, 31, 63):
                want = sum(w[j] * float(v[h, j, d]) for j in range(T)) / tot
                assert abs(ref[h, t, d] - want) <= 1e-12 * max(1.0, abs(want)), (T, h, t, d)


def test_lengths_reach_every_tile_class():
    """the kernel's a / b / last arithmetic, restated in D.tile_bounds: which lengths are the smallest with each class, and that the tail tile's far-below
    condition is never met by a wave that stores a query"""
    for kind in (F16_Q128, F16_Q64):
        cl = {T: D.tile_classes(T, kind) for T in range(1, 600)}
        first = lambda name: min(T for T in cl if name in cl[T])
        assert first("far-below") == 129 and first("far-above") == 192 and first("tail-far-above") == 129 and first("no-tail") == 64
        assert all(("tail-far-above" in cl[T]) == (T % 64 != 0) for T in range(129, 600))
        assert not any("tail-far-below" in c for c in cl.values())
        reached = set().union(*(cl[T] for T in D.LENGTHS))
        assert reached == {"far-below", "near", "far-above", "tail-near", "tail-far-above", "no-tail"}
        for T in (129, 190, 191):
            assert {"far-below", "tail-far-above", "tail-near"} <= cl[T] and "far-above" not in cl[T]
        assert cl[192] == {"far-below", "near", "far-above", "no-tail"} and cl[128] == {"near", "no-tail"} and cl[63] == {"tail-near"}
    assert D.tile_bounds(128, 32, 129)[:3] == (1, 2, 2) and D.tile_bounds(0, 32, 193)[:3] == (0, 2, 3) and D.tile_bounds(0, 16, 193)[:3] == (0, 2, 3)


def test_families_do_what_they_are_named_for():
    tab = D.bias_table("smooth")
    assert np.abs(tab).max() <= 1.0 and (np.diff(tab.reshape(NH, 2, 64), axis=2) < 0).all()
    sharp = D.bias_table("sharp")
    s3 = sharp.reshape(NH, 2, 64)
    assert np.abs(sharp).max() <= 4.0 and np.abs(np.diff(s3, axis=2)).min() >= 1.0 and np.abs(s3[:, 0] - s3[:, 1]).min() >= 1.0
    assert np.abs(s3[:, :, 62] - s3[:, :, 63]).min() >= 1.0 and np.abs(s3[0::2] - s3[1::2]).min() >= 1.0
    for T in (64, 193, 385):
        sq = D.single(T, ("wide", "sharp")).seqs[0]
        share = D.wide_condition(sq, sharp)
        print("wide T=%d: %.0f %% of the weights below 2^-14 of the running maximum" % (T, 100 * share))
        assert share >= 0.25
    T = 257
    nt = (T + 63) // 64
    for fam, rises in (("ramp-up", nt - 1), ("ramp-down", 0)):  # the running maximum after tile 0: rises at every tile / never
        r = D.reference(D.single(T, (fam, "smooth")).seqs[0], tab)
        s = np.full((NH, T, nt * 64), -np.inf)
        s[:, :, :T] = r["s"][:, :, :T]
        m = np.maximum.accumulate(s.reshape(NH, T, nt, 64).max(axis=3), axis=2)
        assert ((np.diff(m, axis=2) > 0).sum(axis=2) == rises).all(), fam
    r = D.reference(D.single(T, ("split", "smooth")).seqs[0], tab)
    top = r["p"].argmax(axis=2)  # [16, T]
    late = np.arange(T) % 32 >= 16
    assert (top[:, ~late] == 0).all() and (top[:, late] == T - 1).all()
    tags = [t for t, _ in D.placements(383)]
    assert tags == ["last", "beyond", "key0", "tile_first", "tile_prev_last", "d-64", "d-63", "d-62", "d+62", "d+63", "d+64"]
    pl = dict(D.placements(383))  # the last wave starts at query 352
    assert pl["d-63"] == 352 - 63 and pl["d+63"] == 31 + 63 and pl["beyond"] == 383 and pl["tile_first"] == 320 and pl["tile_prev_last"] == 319


# ---------------------------------------------------------------------------------------------------------------- the bound is not too tight

def configs(T):
    return [("flat", "sharp")] if T == 577 else D.CONFIGS  # one case of 577


def _check_restatement(c):
    worst = {}
    for sq in c.seqs:
        for name, got, ref, bd in (("f16", D.restate16(sq, c.bias), D.reference(sq, c.bias)["out"], D.bound16(sq, c.bias)),
                                   ("f32", D.restate32(sq, c.bias), D.reference(sq, c.bias, True)["out"], D.bound32(sq, c.bias))):
            assert np.isfinite(bd).all() and (bd > 0).all()
            r = np.where(got == ref, 0.0, np.abs(got - ref) / bd)
            assert (r <= 1.0).all(), (c.name(), name, float(r.max()), np.argwhere(r > 1)[:4].tolist())
            worst[name] = max(worst.get(name, 0.0), float(r.max()))
    return worst


@pytest.mark.parametrize("T", D.LENGTHS)
def test_numpy_restatements_pass_every_case(T):
    for cfg in configs(T):
        w = _check_restatement(D.single(T, cfg))
        print("%-28s restatement |err|/bound: fp16 %.3f split %.3f" % (D.single(T, cfg).name(), w["f16"], w["f32"]))


def test_numpy_restatements_pass_the_multi_sequence_layouts():
    for lens in D.TRIPLES:
        _check_restatement(D.triple(lens, ("flat", "sharp")))
    _check_restatement(D.Case(D.EIGHT, "wide", "sharp"))


# ---------------------------------------------------------------------------------------------------------------- the bound is sharp

PEAKED = [D.single(T, ("peaked", "sharp")) for T in (65, 193)]
BIAS = [D.single(T, ("flat", "sharp")) for T in (193, 257)]
TARGETS = {
    "drop_last": PEAKED, "admit_T": PEAKED, "drop_key0": PEAKED, "drop_first_of_last_tile": PEAKED, "v_halves_swapped": PEAKED,
    "sides_swapped": BIAS, "saturate_62": BIAS, "saturate_64": BIAS, "distance_plus_1": BIAS, "bias_of_head_xor_1": BIAS,
    "far_below_one_tile_late": BIAS, "far_above_one_tile_early": BIAS,
    "scale_sqrt63": [D.single(T, ("wide", "smooth")) for T in (65, 193)],
}


def test_every_mutation_has_a_target():
    assert set(TARGETS) == set(D.MUTATIONS)


@pytest.mark.parametrize("mut", D.MUTATIONS)
def test_every_mutation_of_the_reference_is_caught(mut):
    for f32, name in ((False, "fp16 kernels"), (True, "split-precision kernel")):
        best = (0.0, None, None)
        for c in TARGETS[mut]:
            sq = c.seqs[0]
            ref = D.reference(sq, c.bias, f32)["out"]
            m = D.reference(sq, c.bias, f32, mut=mut)["out"]
            r = np.abs(m - ref) / (D.bound32(sq, c.bias) if f32 else D.bound16(sq, c.bias))
            i = np.unravel_index(np.argmax(r), r.shape)
            if r[i] > best[0]:
                best = (float(r[i]), c, i)
        r, c, i = best
        print("%-26s %-24s caught by %s, head %d query %d channel %d: %.3g x its bound" % (mut, name, c.name() if c else None, i[0], i[1], i[2], r))
        assert r >= 10.0, (mut, name, r)


def test_saturation_mutations_touch_only_the_entries_they_name():
    """the targeted checks behind the table mutations: 62 / 64 differ from the correct index exactly at |d| = 63 / >= 64, and a far tile one off moves whole tiles"""
    T = 193
    ok = D.bias_index(T)
    t, j = np.arange(T)[:, None], np.arange(T + 1)[None, :]
    assert (ok == np.where(j > t, 64, 0) + np.minimum(np.abs(j - t), 63)).all()
    assert ((D.bias_index(T, "saturate_62") != ok) == (np.abs(j - t) >= 63)).all()
    assert ((D.bias_index(T, "saturate_64") != ok) == (np.abs(j - t) >= 64)).all()
    late, early = D.bias_index(T, "far_below_one_tile_late") != ok, D.bias_index(T, "far_above_one_tile_early") != ok
    assert late[128:160, 64:128].any() and not late[128:160, 128:].any() and early[0:32, 64:128].any() and not early[0:32, :64].any()
