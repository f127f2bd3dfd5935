"""CPU side of tests/test_voc_kernels_gpu.py: the harness library builds for gfx950, loads and exports its surface; it refuses every invalid case before any HIP
call; lvc_col is a bijection; the float64 references of tests/voc_cases.py are checked against naive loops written from the comments of vocoder.hip; the Philox
restatement against the Random123 known-answer vectors; a float32 restatement of every kernel, summing forward and backward, passes the acceptance rule on every
case of the matrix (the bound is not too tight); and every listed defect leaves the bound on some case (the bound is sharp). Which case catches which defect is
printed (pytest -s)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import voc_cases as V
from voc_cases import COND_F16, CONV, CONVT, DCONV, LVC_GATE, LVC_MFMA, MEL_ROWS, NOISE_ROWS, PHILOX, POST

f32, i32 = np.float32, np.int32


def test_harness_library_builds_and_exports_its_surface():
    L = V.harness()  # builds it once if missing; raises otherwise
    for sym in ("tts_voc_test_run", "tts_voc_test_validate", "tts_voc_test_margin", "tts_voc_test_lvc_col"):
        assert hasattr(L, sym), sym
    assert L.tts_voc_test_margin() == 4096
    src_t = max(os.path.getmtime(V.SRC), os.path.getmtime(os.path.join(V.PKG, "csrc", "vocoder.hip")))
    assert os.path.getmtime(V.LIB) >= src_t or os.environ.get("TTS_VOC_TEST_LIB"), "libtts_voc_test.so is older than its sources: run make"


def test_harness_is_not_part_of_the_product():
    mk = open(os.path.join(V.PKG, "Makefile")).read()
    assert "HIP_SRCS = $(wildcard csrc/*.hip)" in mk and not os.path.exists(os.path.join(V.PKG, "csrc", "voc_harness.hip"))
    link = [l for l in mk.splitlines() if "-o $@ $(OBJS)" in l]
    assert len(link) == 1 and "testlib" not in link[0] and "voc_test" not in link[0]
    rule = [l for l in mk.splitlines() if "testlib/voc_harness.hip csrc/host_logic.cpp -o $@" in l]
    assert len(rule) == 1 and "vgpr-form" not in rule[0]  # the flags of csrc/vocoder.o
    src = open(V.SRC).read()
    assert '#include "../csrc/vocoder.hip"' in src and "asm" not in src and "__global__" not in src  # the product's kernels, none of its own


def test_restated_launches_name_the_lines_of_voc_run_they_copy():
    """voc_run launches inline, so the harness restates grid and block; each restated launch cites vocoder.hip lines that launch the same kernel"""
    src = open(V.SRC).read().splitlines()
    voc = open(os.path.join(V.PKG, "csrc", "vocoder.hip")).read().splitlines()
    seen = []
    for i, line in enumerate(src):
        m = re.search(r"vocoder\.hip:(\d+)(?:-(\d+))?", line)
        if m:
            lo, hi = int(m.group(1)), int(m.group(2) or m.group(1))
            kernel = re.search(r"(\w+_kernel)<<<", " ".join(src[i:i + 4])).group(1)
            assert any(kernel + "<<<" in l for l in voc[lo - 1:hi]), (kernel, lo, hi)
            seen.append(kernel)
    assert sorted(seen) == sorted(V.KIND_NAMES)


def test_lvc_col_is_a_bijection_onto_one_layer():
    p = V.lvc_perm()
    assert p.shape == (6144,) and sorted(p.tolist()) == list(range(6144))
    L = V.harness()
    assert L.tts_voc_test_lvc_col(0, 0, 0) == 0 and p[(5 * 64 + 17) * 3 + 2] == L.tts_voc_test_lvc_col(2, 5, 17)


def test_layouts_are_those_voc_run_builds():
    rows = {n: V.layout(n).rows for n in "ABCD"}
    assert rows == dict(A=24, B=40, C=64, D=128)
    b = V.layout("B")
    assert b.start == [8, 24] and b.row_seq[22] == 0 and b.row_seq[23] == -1 and b.row_seq[24] == 1  # exactly one guard frame
    assert V.layout("C").start == [8, 24, 40]


# ---------------------------------------------------------------------------------------------------------------- validation (no HIP call is reached)

def _valid(kind):
    c = {CONV: lambda: V.make(CONV, "B", Cin=32, Cout=32, K=3, pre=1, post=1, hop=8, dil=3, resid=1), CONVT: lambda: V.make(CONVT, "B", hop=8, s=8),
         LVC_GATE: lambda: V.make(LVC_GATE, "B", hop=8, layer=1), LVC_MFMA: lambda: V.make(LVC_MFMA, "B", hop=64, layer=3),
         DCONV: lambda: V.make(DCONV, "B", hop=64, dil=27), POST: lambda: V.make(POST, "A")}.get(kind, lambda: V.make(kind, "B"))()
    shape, dt = V.out_shape(c)
    return V.to_struct(c, V.Guarded(shape, dt))


def _rc(cs):
    L = V.harness()
    rc = L.tts_voc_test_validate(C.byref(cs))
    if rc != 0:  # refused by the run entry too, before any HIP call (this machine has no GPU: a HIP call would return another code)
        assert L.tts_voc_test_run(C.byref(cs)) == V.HIP_INVALID_VALUE
    return rc


ALL_LAUNCH = [CONV, CONVT, LVC_GATE, LVC_MFMA, DCONV, POST, MEL_ROWS, NOISE_ROWS, COND_F16]


@pytest.mark.parametrize("kind", ALL_LAUNCH)
def test_valid_cases_validate(kind):
    assert V.harness().tts_voc_test_validate(C.byref(_valid(kind))) == 0


def test_valid_philox_validates_and_null_is_refused():
    L = V.harness()
    assert L.tts_voc_test_validate(C.byref(V.struct(PHILOX, out=V.Guarded((16,), f32), n=16, seed=1, stream=0))) == 0
    assert L.tts_voc_test_validate(None) == V.HIP_INVALID_VALUE and L.tts_voc_test_run(None) == V.HIP_INVALID_VALUE


def _arr(v):
    return np.array(v, i32)


# (what, kind, fields to overwrite; arrays are replaced through "start" / "len", None clears a pointer)
INVALID = [
    ("unknown kind", CONV, dict(kind=10)), ("kind < 0", CONV, dict(kind=-1)), ("no output", CONV, dict(out=None)), ("no input", DCONV, dict(x=None)),
    ("len < 11", CONV, dict(len=_arr([15, 10]))), ("len < 11 lvc", LVC_MFMA, dict(len=_arr([10, 11]))), ("len 0", POST, dict(len=_arr([0]))),
    ("start % 8 != 0", DCONV, dict(start=_arr([8, 25]))), ("start % 8 != 0 first", LVC_GATE, dict(start=_arr([9, 32]))),
    ("no guard row after a sequence", LVC_MFMA, dict(len=_arr([16, 11]))), ("sequences overlap", CONV, dict(len=_arr([17, 11]))),
    ("starts out of order", CONVT, dict(start=_arr([24, 8]))),
    ("first sequence before row 8", LVC_MFMA, dict(start=_arr([0, 24]))), ("first sequence before row 8 conv", CONV, dict(start=_arr([0, 24]))),
    ("negative start", DCONV, dict(start=_arr([-8, 24]))),
    ("live last row", LVC_MFMA, dict(len=_arr([15, 16]))), ("live last row dconv", DCONV, dict(len=_arr([15, 16]))), ("last sequence past the rows", CONV, dict(len=_arr([15, 17]))),
    ("rows % 8 != 0", CONV, dict(rows=41)), ("rows too small", CONV, dict(rows=0)), ("rows too large", CONV, dict(rows=264)),
    ("ns = 0", CONV, dict(ns=0)), ("ns too large", CONV, dict(ns=17)), ("no start", CONV, dict(start=None)), ("no len", MEL_ROWS, dict(len=None)),
    ("Cout = 16", CONV, dict(Cout=16)), ("Cout = 48", CONV, dict(Cout=48)), ("Cout = 128", CONV, dict(Cout=128)), ("Cout = 0", CONV, dict(Cout=0)),
    ("Cin = 0", CONV, dict(Cin=0)), ("Cin too large", CONV, dict(Cin=129)), ("K = 0", CONV, dict(K=0)), ("K = 8", CONV, dict(K=8)),
    ("conv hop not a power of two", CONV, dict(hop=6)), ("conv hop 0", CONV, dict(hop=0)), ("conv dil 0", CONV, dict(dil=0)), ("conv pad < 0", CONV, dict(pad=-1)),
    ("conv flag", CONV, dict(pre_leaky=2)), ("conv no weights", CONV, dict(w=None)), ("conv no bias", CONV, dict(bias=None)),
    ("dconv hop 128", DCONV, dict(hop=128)), ("dconv hop 8", DCONV, dict(hop=8)), ("dconv hop 512", DCONV, dict(hop=512)),
    ("dconv dil = hop", DCONV, dict(dil=64)), ("dconv dil > hop", DCONV, dict(dil=65)), ("dconv dil 0", DCONV, dict(dil=0)), ("dconv no weights", DCONV, dict(w=None)),
    ("lvc_mfma hop 32", LVC_MFMA, dict(hop=32)), ("lvc_mfma hop 96", LVC_MFMA, dict(hop=96)), ("lvc_mfma hop 8", LVC_MFMA, dict(hop=8)),
    ("lvc_mfma hop 0", LVC_MFMA, dict(hop=0)), ("lvc_mfma hop 512", LVC_MFMA, dict(hop=512)),
    ("lvc_mfma layer 4", LVC_MFMA, dict(layer=4)), ("lvc_mfma layer -1", LVC_MFMA, dict(layer=-1)), ("lvc_mfma no kernel", LVC_MFMA, dict(kern=None)),
    ("lvc_mfma no bias", LVC_MFMA, dict(kb=None)), ("lvc_mfma no x", LVC_MFMA, dict(xio=None)),
    ("lvc_gate hop 96", LVC_GATE, dict(hop=96)), ("lvc_gate hop 24", LVC_GATE, dict(hop=24)), ("lvc_gate layer 4", LVC_GATE, dict(layer=4)), ("lvc_gate no x", LVC_GATE, dict(xio=None)),
    ("convt hop 6", CONVT, dict(hop=6)), ("convt s 6", CONVT, dict(s=6)), ("convt s 0", CONVT, dict(s=0)), ("convt s 1", CONVT, dict(s=1)),
    ("convt hop * s too large", CONVT, dict(hop=64, s=8)), ("convt no weights", CONVT, dict(w=None)),
    ("post no weights", POST, dict(w=None)), ("post no bias", POST, dict(bias=None)),
]


@pytest.mark.parametrize("what,kind,over", INVALID, ids=[w for w, _, _ in INVALID])
def test_invalid_case_is_refused_before_any_hip_call(what, kind, over):
    cs = _valid(kind)
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            cs._keep.append(v)
            setattr(cs, k, v.ctypes.data_as(C.c_void_p))
        else:
            setattr(cs, k, v)
    assert _rc(cs) == V.HIP_INVALID_VALUE


@pytest.mark.parametrize("n", [0, -1, (1 << 22) + 1])
def test_invalid_philox_is_refused(n):
    assert _rc(V.struct(PHILOX, out=V.Guarded((16,), f32), n=n, seed=1, stream=0)) == V.HIP_INVALID_VALUE


# ---------------------------------------------------------------------------------------------------------------- references against naive loops

def _close(z, naive):
    assert z.shape == naive.shape
    assert np.abs(z - naive).max() <= 1e-12 * max(1.0, np.abs(naive).max())


def _h(v):
    return float(np.float16(v))


def _lk(v):
    return float(v) if v > 0 else float(f32(0.2) * f32(v))


@pytest.mark.parametrize("p", [dict(Cin=3, Cout=2, K=7, reflect=1), dict(Cin=5, Cout=2, K=5, post=1), dict(Cin=2, Cout=2, K=3, post=1, resid=1),
                               dict(Cin=2, Cout=3, K=3, pre=1, post=1, hop=4, dil=3), dict(Cin=2, Cout=3, K=3, pre=1, post=1, hop=2, dil=27)],
                         ids=["pre-reflect", "k5-post", "k3-resid", "hop4-dil3", "hop2-dil27"])
def test_conv_reference_against_naive_loops(p):
    """conv1d per sequence, zero padding (or reflection) at ITS ends: fp16(leaky(x)) x fp16 weights, + bias, leaky, + resid"""
    c = V.make(CONV, "B", "straddle", seed=3, **p)
    q, a, lay = c.p, c.a, c.lay
    hop, K, dil, pad = q["hop"], q["K"], q["dil"], q["pad"]
    out = np.zeros((lay.rows * hop, q["Cout"]))
    for s in range(lay.ns):
        n = lay.len[s] * hop
        xs = a["x"][lay.seq(s, hop)]
        for t in range(n):
            for co in range(q["Cout"]):
                acc = 0.0
                for k in range(K):
                    j = t + k * dil - pad
                    if q["reflect"]:
                        j = -j if j < 0 else j
                        j = 2 * (n - 1) - j if j >= n else j
                    if 0 <= j < n:
                        for ci in range(q["Cin"]):
                            v = xs[j, ci]
                            acc += _h(_lk(v) if q["pre"] else v) * float(a["w"][k, ci, co])
                v = acc + float(a["bias"][co])
                v = (v if v > 0 else V.L02 * v) if q["post"] else v
                out[lay.start[s] * hop + t, co] = v + (float(a["resid"][lay.start[s] * hop + t, co]) if q["resid"] else 0.0)
    _close(V.reference(c)["z"], out)


@pytest.mark.parametrize("hop,s", [(1, 8), (2, 4), (4, 2)])
def test_convt_reference_against_the_scatter_form(hop, s):
    """ConvTranspose1d(K = 2s, stride s) of leaky(x) written as a scatter, then s/2 samples cropped from either side, + bias"""
    c = V.make(CONVT, "B", "gauss", seed=4, hop=hop, s=s)
    lay, a = c.lay, c.a
    out = np.zeros((lay.rows * hop * s, 32))
    for q in range(lay.ns):
        n = lay.len[q] * hop
        xs = V.leaky32(a["x"][lay.seq(q, hop)]).astype(np.float64)
        full = np.zeros(((n - 1) * s + 2 * s, 32))
        for t in range(n):
            for k in range(2 * s):
                full[t * s + k] += xs[t] @ a["w"][k].astype(np.float64)
        out[lay.start[q] * hop * s:(lay.start[q] * hop + n) * s] = full[s // 2:s // 2 + n * s] + a["bias"].astype(np.float64)
    _close(V.reference(c)["z"], out)


def test_lvc_reference_against_naive_loops():
    """o[ch][pos] = b[ch] + sum_i sum_k ypad[i][pos + k - 1] W[i][ch][k] with the frame's own kernel; x += sigmoid(o[c]) tanh(o[32 + c])"""
    c = V.make(LVC_GATE, "B", "gauss", seed=5, hop=4, layer=2)
    lay, a, hop = c.lay, c.a, 4
    out = a["xio"].astype(np.float64)
    for s in range(lay.ns):
        sl = lay.seq(s, hop)
        n = sl.stop - sl.start
        ypad = np.zeros((n + 2, 32))
        ypad[1:n + 1] = a["x"][sl]
        for t in range(n):
            row = (sl.start + t) // hop
            W = a["W"][row].astype(np.float64)  # (i*64 + ch)*3 + tap
            o = np.zeros(64)
            for ch in range(64):
                acc = float(a["kbl"][row, ch])
                for i in range(32):
                    for k in range(3):
                        acc += ypad[t + k, i] * W[(i * 64 + ch) * 3 + k]
                o[ch] = acc
            out[sl.start + t] += 1.0 / (1.0 + np.exp(-o[:32])) * np.tanh(o[32:])
    _close(V.reference(c)["z"], out)


def test_dconv_and_post_references_against_naive_loops():
    c = V.make(DCONV, "A", "straddle", seed=6, hop=64, dil=27)
    lay, a = c.lay, c.a
    z = V.reference(c)["z"]
    n = lay.len[0] * 64
    xs = a["x"][lay.seq(0, 64)]
    rng = np.random.default_rng(0)
    for t in [0, 1, 26, 27, 28, n - 28, n - 27, n - 1] + list(rng.integers(0, n, 8)):
        for co in (0, 17, 31):
            acc = float(a["bias"][co])
            for k in range(3):
                j = t + (k - 1) * 27
                if 0 <= j < n:
                    acc += sum(_h(_lk(xs[j, ci])) * float(a["w"][k, ci, co]) for ci in range(32))
            assert abs(z[lay.start[0] * 64 + t, co] - (acc if acc > 0 else V.L02 * acc)) < 1e-12
    assert (z[~lay.live(64)] == 0).all()
    c = V.make(POST, "B", "gauss", seed=7)
    lay, a = c.lay, c.a
    z = V.reference(c)["z"]
    assert z.shape == (15 * 256 - 6 + 11 * 256 - 6,)
    for s, off in ((0, 0), (1, 15 * 256 - 6)):
        n = lay.len[s] * 256 - 6
        for j in (0, 1, 255, 256, n - 2, n - 1):  # n - 1 = the last valid sample len*256 - 7
            acc = float(a["bias"][0])
            for k in range(7):
                acc += sum(_h(_lk(a["x"][lay.start[s] * 256 + j + k, ci])) * float(a["w"][k, ci]) for ci in range(32))
            assert abs(z[off + j] - acc) < 1e-12


def test_row_references():
    c = V.make(MEL_ROWS, "B", "gauss", seed=8)
    r = V.reference(c)
    T = 5
    m = c.a["x"][:100 * T].reshape(100, T)
    assert abs(r["z"][8 + 3, 17] - ((float(m[17, 3]) + 1) / 2 * (2.3143386840820312 + 11.512925148010254) - 11.512925148010254)) < 1e-5
    assert (r["z"][8 + 5:8 + 15] == float(f32(-11.5129))).all() and (r["z"][23] == 0).all() and (r["bound"][8 + 5:8 + 15] == 0).all()
    assert r["bound"].max() < 1e-5  # a few f32 ulp of values of at most 13.8
    c = V.make(NOISE_ROWS, "B", "ramp", seed=8)
    z = V.reference(c)["z"]
    assert z[24 + 2, 9] == c.a["x"][64 * 15 + 9 * 11 + 2] and (z[23] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the rule accepts f32, rejects the defects

KINDS = [CONV, CONVT, LVC_GATE, LVC_MFMA, DCONV, POST, MEL_ROWS, NOISE_ROWS, COND_F16]


@pytest.mark.parametrize("kind", KINDS, ids=[V.KIND_NAMES[k] for k in KINDS])
def test_a_float32_restatement_is_accepted_on_every_case(kind):
    worst = 0.0
    for c in V.cases(kind):
        ref = V.reference(c)
        for order in (0, 1):
            out = V.restate32(c, order)
            bad, r = V.judge(out, ref)
            worst = max(worst, r)
            assert bad == 0 and V.guards_ok(c, out, ref), (c.name(), order, bad, r)
        if kind in (CONV, CONVT, LVC_GATE, POST):  # NaN on the guards of the input: kernels that check bounds never read them
            assert np.array_equal(V.restate32(V.poisoned(c), 0), V.restate32(c, 0)), c.name()
    print("%-24s f32 restatement, both orders: worst |err| / bound %.3f" % (V.KIND_NAMES[kind], worst))
    assert worst < 1.0


DEFECTS = {
    "tap_reversed": CONV, "dil_plus": CONV, "dil_minus": CONV, "reflect_edge": CONV, "neighbour": CONV, "leaky_after_round": CONV, "no_round": CONV,
    "no_bias": CONV, "no_post_leaky": CONV, "resid_before_leaky": CONV,
    "crop_plus": CONVT, "crop_minus": CONVT, "taps_swapped": CONVT,
    "halves_swapped": LVC_GATE, "ich_transposed": LVC_GATE, "window_shift": LVC_GATE, "neighbour_frame": LVC_GATE, "gate_1e-5": LVC_GATE,
    "post_no_leaky": POST, "post_6taps": POST,
}
_small = lambda k: [(l, f, p) for l, f, p in V.matrix(k) if l != "D" and (k == POST or p.get("hop", 1) <= 64)]


@pytest.mark.parametrize("mut", sorted(DEFECTS))
def test_every_defect_is_rejected_on_some_case(mut):
    kind, caught = DEFECTS[mut], []
    for l, f, p in _small(kind):
        c = V.make(kind, l, f, **p)
        ref = V.reference(c)
        bad, r = V.judge(V.reference(c, mut=mut)["z"], ref)
        if bad:
            caught.append((c.name(), bad, r))
    print("%-20s rejected on %d cases; first: %s" % (mut, len(caught), caught[:1]))
    assert caught


def test_the_same_defects_are_rejected_for_the_mfma_twins():
    """the MFMA kernels share the references of their VALU twins: the structural defects are caught on their cases too (not `neighbour`: with dil < hop and
    zero guard frames, reading across the end of a sequence IS voc_dconv_mfma_kernel's documented way to pad)"""
    for kind, muts in ((DCONV, ("tap_reversed", "dil_plus", "dil_minus", "leaky_after_round", "no_round", "no_bias", "no_post_leaky")),
                       (LVC_MFMA, ("halves_swapped", "ich_transposed", "window_shift", "neighbour_frame", "gate_1e-5"))):
        cs = [V.make(kind, l, f, **p) for l, f, p in V.matrix(kind) if p["hop"] == 64 and l != "D"]
        refs = [V.reference(c) for c in cs]
        for mut in muts:
            assert any(V.judge(V.reference(c, mut=mut)["z"], r)[0] for c, r in zip(cs, refs)), (V.KIND_NAMES[kind], mut)


def test_gate_bound_is_absolute_near_tanh_zero():
    """the corrected statement of gate_dev's accuracy: about 4u absolute at b -> 0 (so no relative accuracy there), relative where |tanh b| is near 1"""
    z = np.zeros(1)
    b0 = V.gate_bound(z, z + 1e-6, z, z, z)[0]
    assert 0.4 * 4 * V.U < b0 < 4 * V.U and b0 / (0.5 * 1e-6) > 0.1  # more than 10 % of the value itself
    assert V.gate_bound(z + 20, z + 20, z, z, z + 1)[0] < 8 * V.U
    g = V.GATE_GRID
    a, b = np.meshgrid(g, g)
    out = V.gate32(a, b)
    assert np.isfinite(out).all()
    assert (np.abs(out.astype(np.float64) - V.gate64(a.astype(np.float64), b.astype(np.float64))) <= V.gate_bound(a, b, 0, 0, 0)).all()


# ---------------------------------------------------------------------------------------------------------------- Philox

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_restatement_reproduces_the_known_answer_vectors():
    for ctr, key, want in KAT:
        assert V.philox4x32_10_int(ctr, key) == want
        got = V.philox4x32_10([np.array([c], np.uint32) for c in ctr], [np.array([k], np.uint32) for k in key])
        assert tuple(int(v[0]) for v in got) == want
    rng = np.random.default_rng(1)
    ctr, key = rng.integers(0, 2 ** 32, (4, 64), dtype=np.uint64), rng.integers(0, 2 ** 32, (2, 64), dtype=np.uint64)
    got = V.philox4x32_10(list(ctr), list(key))
    for j in range(64):
        assert tuple(int(v[j]) for v in got) == V.philox4x32_10_int([int(v) for v in ctr[:, j]], [int(v) for v in key[:, j]])


def test_philox_reference_bound_accepts_float32_box_muller_and_is_normal():
    for seed, stream in ((0x1234, 0), (0x9e3779b97f4a7c15, 5)):
        x, bound = V.philox_reference(4096, seed, stream)
        i = np.arange(4096, dtype=np.uint64)
        r = V.philox4x32_10([i >> np.uint64(1), 0x766f63, stream, 0x7716], [seed & 0xFFFFFFFF, seed >> 32])
        u1, u2 = (r[0].astype(f32) + f32(1)) * f32(2.0 ** -32), r[1].astype(f32) * f32(2.0 ** -32)
        rad, th = np.sqrt(f32(-2) * np.log(u1)), f32(6.283185307179586) * u2
        out = np.where(np.arange(4096) & 1, rad * np.sin(th), rad * np.cos(th))
        assert out.dtype == f32 and (np.abs(out - x) <= bound).all()
        assert (x[0::2] != x[1::2]).all() and bound.max() < 1e-5
        assert np.abs(V.philox_reference(4096, seed, stream + 1)[0] - x).max() > 1  # another stream, another sequence
    xs = np.stack([V.philox_reference(1024, 77, s)[0] for s in range(64)])
    assert (np.abs(xs.mean(axis=1)) < 5 / np.sqrt(1024)).all() and (np.abs(xs.var(axis=1, ddof=1) - 1) < 5 * np.sqrt(2.0 / 1023)).all()
    assert abs(xs.mean()) < 5 / 256.0 and abs(xs.var() - 1) < 5 * np.sqrt(2.0 / 65535)
