"""The fp16 GEMM kernel family of csrc/gemm_f16.h, called directly through launch_gemm_f16 (test-only harness: tortoise.cpp_amd/testlib/gemm_harness.hip) and
compared with a float64 NumPy reference written from the header's formula (tests/gemm_cases.py; checked against naive loops in test_gemm_harness_cpu.py).

(a) test_exact: integer (and fp16-subnormal) operands for which every f32 intermediate is exactly representable in any summation order — the condition is
    asserted on the reference side, see gemm_cases.exactness — so the reference rounded once to the output type must equal the kernel's output BIT FOR BIT, in
    every mode; canary margins, the sentinel in everything a mode must not write (leading-dimension padding) and its absence from everything it must write are
    asserted per case. A failure prints kernel, mode, th, ku and the first differing element with its XCD / tile / block / wave coordinates.
(b) test_real_valued: Gaussian and heavy-tailed fp16 operands at production shapes; products of fp16 values are exact in f32, so the error is f32 accumulation
    and output rounding: |got - ref64| <= (C_ACC * ktot + 3) * 2^-24 * (alpha * sum_k |a||w| + |bias| + |resid|) (+ half an fp16 ulp for fp16 outputs).
    C_ACC = 1 is what round-to-nearest summation in any order gives. Largest observed ratio |got - ref64| / (ktot * 2^-24 * sum) per kernel on an MI355X:
    see DESIGN.md ("What pins the GEMM kernels"); the test prints it.
(c) test_identity_*: the bit-identities the header claims in its comments, between harness runs on the operands of (b).
(d) test_refusals: argument sets launch_gemm_f16 must refuse without launching.
test_coverage (last) asserts that the exact cases reached every kernel x mode pair, launch form, tile height and per-wave block count the dispatcher has."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as G
from gemm_cases import (F16, F32, F32_MODES, F32_SCALED, F32_SCALED_STATS, F32_STATS, QKV, QKV_MODES, QKV_SPLIT, SCALED_MODES, STATS_MODES, Case, conv3,
                        dualb)

pytestmark = pytest.mark.gpu

C_ACC = 1  # accumulation constant of (b): round-to-nearest summation in any order
SEEN = {}  # case name -> (plan string, case): what the launcher selected for every exact case that ran


@pytest.fixture(scope="module")
def lib():
    return G.harness()  # raises when the library is missing and cannot be built: no skip


def run(lib, case, ops, **override):
    margin = lib.tts_gemm_test_margin()
    stripe = override.get("st_stripe_ll")
    outs = G.out_buffers(case, ops, margin, stripe_ll=stripe if stripe else None)
    if override.get("has_st") == 0:
        outs.pop("st", None)
    keep = []
    s = G.fill_struct(case, ops, outs=outs, keep=keep, **override)
    rc = lib.tts_gemm_test_run(C.byref(s))
    buf = C.create_string_buffer(160)
    lib.tts_gemm_test_last_kernel(buf, 160)
    return rc, outs, buf.value.decode()


def shapes(case, ops):
    M, N, pad, heads = case.M, case.N, case.pad, case.N // 192
    d = {}
    if case.mode in F32_MODES:
        d["outF"] = (np.float32, (M, N + pad), N)
    elif case.mode == F16:
        d["outH"] = (np.float16, (M, N + pad), N)
    else:
        d["outH"] = (np.float16, (M, heads * 128 + pad), heads * 128)
        d["outVt"] = (np.float16, (heads * 64, M + pad), M)
        if case.mode == QKV_SPLIT:
            d["outH2"], d["outVt2"] = d["outH"], d["outVt"]
    return d


def unpack(lib, case, ops, outs):
    """payload views; asserts the canary margins of every buffer"""
    margin = lib.tts_gemm_test_margin()
    got = {}
    for k, (dt, shape, _) in shapes(case, ops).items():
        got[k] = G.payload(outs[k], margin, dt, shape)
    for k, b in outs.items():
        assert (b[:margin] == G.SENTINEL).all() and (b[len(b) - margin:] == G.SENTINEL).all(), "%s: canary margin of %s overwritten" % (case.name, k)
    if "st" in outs:
        got["st"] = G.payload(outs["st"], margin, np.int64, (G.FX_STRIPES, -1))
    return got


def decode_stats(case, ops, st):
    """eight stripes summed (integers: exact), decoded with fx_value -> [sequence][group][sum, sum of squares]"""
    nseq = ops["nseq"]
    tot = st[:, :nseq * 32 * 4].sum(axis=0).reshape(nseq, 32, 4)[:, :case.N // 32]
    return np.stack([G.fx_value(tot[..., 0], tot[..., 1]), G.fx_value(tot[..., 2], tot[..., 3])], axis=-1), st[:, nseq * 32 * 4:]


def where(case, plan, name, r, c):
    """coordinates of output element (row r of the packed layout, GEMM column c) in the tile walk"""
    kern = plan.split()[0]
    th = int(plan.split("th=")[1].split()[0])
    nb, blk = case.M >> 4, r >> 4
    for x in range(8):
        b0, b1 = nb * x >> 3, nb * (x + 1) >> 3
        if b0 <= blk < b1:
            break
    t, bi = (blk - b0) // th, (blk - b0) % th
    wave = "wave %d" % ((c % 128) // 32) if kern == "wreg" else "wave (wm %d, wn %d)" % (bi & 1, (c % 128) // 64)
    return "%s: row %d col %d = XCD %d, row tile %d (%d blocks) block %d, column tile %d, %s, lane row %d" % (
        name, r, c, x, t, min(th, b1 - b0 - t * th), bi, c >> 7, wave, r & 15)


def gemm_col(case, name, j, i):
    """GEMM (row, column) of element [j][i] of an output array"""
    if name in ("outVt", "outVt2"):
        return i, (j // 64) * 192 + 128 + j % 64
    if case.mode in QKV_MODES:
        return j, (i // 128) * 192 + i % 128
    return j, i


def assert_bits(case, plan, name, got, ref, width, before=None):
    """`before`: what the leading-dimension padding held before the launch (an output that aliases the residual starts from the residual's padding), else the sentinel"""
    ut = np.uint32 if got.dtype == np.float32 else np.uint16
    g, r = got[:, :width].view(ut), np.ascontiguousarray(ref).view(ut)
    bad = np.argwhere(g != r)
    if len(bad):
        j, i = bad[0]
        rr, cc = gemm_col(case, name, int(j), int(i))
        raise AssertionError("%s [%s]: %d of %d elements of %s differ from the float64 reference; first: got %r (0x%x) want %r (0x%x) at %s; differing rows %s.. cols %s.." % (
            case.name, plan, len(bad), g.size, name, got[j, i], g[j, i], ref[j, i], r[j, i], where(case, plan, name, rr, cc),
            sorted(set(bad[:, 0].tolist()))[:12], sorted(set(bad[:, 1].tolist()))[:12]))
    padding = got[:, width:].view(np.uint8)
    untouched = np.uint8(G.SENTINEL) if before is None else np.ascontiguousarray(before[:, width:]).view(np.uint8)
    assert (padding == untouched).all(), "%s [%s]: %s written beyond its %d columns (leading-dimension padding)" % (case.name, plan, name, width)


def check_exact(lib, case):
    ops = G.operands(case)
    ref = G.reference(case, ops)
    worst = G.exactness(case, ops, ref)
    assert worst < 2.0 ** 24, (case.name, worst)  # the exactness CONDITION, on the reference
    rc, outs, plan = run(lib, case, ops)
    assert rc == 0, (case.name, plan, rc)
    SEEN[case.name] = (plan, case)
    got = unpack(lib, case, ops, outs)
    for k, (dt, shape, width) in shapes(case, ops).items():
        assert_bits(case, plan, k, got[k], ref[k], width, before=ops["resid"] if case.resid == "alias" else None)
    if "row_seq" in ops and case.mode in F32_MODES:
        guard = ops["row_seq"] < 0
        assert (got["outF"][guard][:, :case.N].view(np.uint32) == 0).all(), "%s: guard rows are not +0.0" % case.name
    if case.mode in STATS_MODES:
        st, tail = decode_stats(case, ops, got["st"])
        assert (tail == 0).all(), "%s: statistics written past the last sequence's records" % case.name
        bad = np.argwhere(st != ref["stats"])
        assert not len(bad), "%s [%s]: statistics differ at (sequence, group, sum|sumsq) %s: got %r want %r" % (
            case.name, plan, bad[:8].tolist(), st[tuple(bad[0])], ref["stats"][tuple(bad[0])])
    return plan


EXACT = G.exact_cases()


@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_exact(lib, case):
    check_exact(lib, case)


# ------------------------------------------------------------------------------------------------------------------------------------ (d) refusals

def _refusal_cases():
    sc = Case(tag="refuse", mode=F32_SCALED, M=128, N=128, kseg=64, resid="sep")
    stc = Case(tag="refuse", mode=F32_STATS, M=128, N=128, kseg=64)
    out = [("alpha=0", sc, dict(alpha=0.0)), ("alpha=3", sc, dict(alpha=3.0)), ("alpha=nan", sc, dict(alpha=float("nan"))),
           ("alpha=0 stats", Case(tag="refuse", mode=F32_SCALED_STATS, M=128, N=128, kseg=64), dict(alpha=0.0)),
           ("no st_out", stc, dict(has_st=0)), ("no chunk_seq", stc, dict(has_chunk_seq=0)), ("no stripe length", stc, dict(st_stripe_ll=0)),
           ("dual_b, plain mode", dualb(64, mode=F32), {}),
           ("dual_b, default weight layout", Case(tag="refuse", mode=F32_SCALED, nseg=2, kseg=64, dual_b=1), {}),
           ("dual_b, two activation buffers", dualb(64, a_sel=(0, 1, 0)), {}),
           ("dual_b, shifted rows", dualb(64, row_off=(0, 1, 0)), {}),
           ("dual_b, three segments", Case(tag="refuse", mode=F32_SCALED, nseg=3, kseg=64, dual_b=1, custom_w=1, ldw=192, w_off=(0, 64, 128)), {})]
    return out


@pytest.mark.parametrize("what,case,override", _refusal_cases(), ids=[r[0] for r in _refusal_cases()])
def test_refusals(lib, what, case, override):
    ops = G.operands(case)
    rc, outs, _ = run(lib, case, ops, **override)
    assert rc == G.HIP_INVALID_VALUE, (what, rc)
    margin = lib.tts_gemm_test_margin()
    assert (outs["outF"] == G.SENTINEL).all(), "%s: the refused launch wrote output" % what
    if "st" in outs:
        assert (G.payload(outs["st"], margin, np.int64, (-1,)) == 0).all(), what


def test_harness_refuses_malformed_cases(lib):
    """the harness validates before it launches: bad shapes and missing buffers never reach the GPU"""
    base = Case(tag="malformed", M=128, N=128, kseg=64, bias=False)
    ops = G.operands(base)
    for override in (dict(M=120), dict(N=192), dict(kseg=96), dict(lda=32), dict(ldo=64), dict(th=9), dict(ku=3), dict(has_bias=1), dict(nseg=4),
                     dict(row_off=(C.c_int * 3)(2, 0, 0)), dict(has_resid=1), dict(mode=7), dict(launches=0)):
        rc, outs, _ = run(lib, base, ops, **override)
        assert rc == G.HIP_INVALID_VALUE, override
        assert (outs["outF"] == 0).all(), override  # nothing came back: the host buffer is as the test made it


# ------------------------------------------------------------------------------------------------------------------------------------ (b), (c)

PROD_LENS = [300, 257, 411, 129, 350, 290]  # one utterance's worth of rows, ragged


def real_operands(case, seed, heavy=False):
    rs = np.random.RandomState(seed)
    M, N, K = case.M, case.N, case.kseg
    rows = None
    ops = {"nseq": 1}
    if isinstance(case.rows, (list, tuple)):
        rows, row_seq, chunk_seq, _ = G.layout(case.rows)
        ops.update(row_seq=row_seq, chunk_seq=chunk_seq, nseq=len(case.rows))
    elif case.mode in STATS_MODES:
        ops.update(row_seq=np.zeros(M, np.int32), chunk_seq=np.zeros(M // 8, np.int32))

    def draw(shape, scale):
        if heavy:  # a few channels and a few single values far outside the bulk, as trained weights and activations have
            v = rs.standard_t(3, size=shape) * scale
            v[..., rs.rand(shape[-1]) < 0.02] *= 12.0
            return np.clip(v, -6e4, 6e4)
        return rs.randn(*shape) * scale
    for b in range(1 + max(case.a_sel[:case.nseg])):
        A = draw((M + 2, K), 1.0)
        if rows is not None:
            A[1:M + 1][ops["row_seq"] < 0] = 0
            A[0] = 0
            A[M + 1] = 0
        ops["A%d" % b] = A.astype(np.float16)
    if case.dual_b:  # hi | lo halves of one f32 weight
        w = draw((N, K), 1.0 / np.sqrt(K)).astype(np.float32)
        hi = w.astype(np.float16)
        lo = (w - hi.astype(np.float32)).astype(np.float16)
        ops["W"] = np.concatenate([hi, lo], axis=1)
    else:
        ops["W"] = draw((N, case.w_cols), 1.0 / np.sqrt(case.ktot)).astype(np.float16)
    if case.bias:
        ops["bias"] = rs.randn(N).astype(np.float32)
    if case.resid:
        ops["resid"] = rs.randn(M, N).astype(np.float32)
    return ops


def ulp16(v):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def _qkv_ref_layout(case, x):
    heads = case.N // 192
    xh = x.reshape(case.M, heads, 192)
    return xh[:, :, :128].reshape(case.M, heads * 128), xh[:, :, 128:].transpose(1, 2, 0).reshape(heads * 64, case.M)


def check_real(lib, case, ops, label):
    ref = G.reference(case, ops)
    alpha = case.alpha if case.mode in SCALED_MODES else 1.0
    S = alpha * G.abs_product_sum(case, ops)
    if case.bias:
        S = S + np.abs(ops["bias"].astype(np.float64))[None, :]
    if case.resid:
        S = S + np.abs(ops["resid"].astype(np.float64))
    u = 2.0 ** -24
    unit = case.ktot * u * S          # the scale the measured ratio is reported in
    e32 = (C_ACC * case.ktot + 3) * u * S
    if "row_seq" in ops:
        e32[ops["row_seq"] < 0] = 0
    rc, outs, plan = run(lib, case, ops)
    assert rc == 0, (label, plan, rc)
    got = unpack(lib, case, ops, outs)
    x = ref["x"]

    def judge(name, g, r, bound, scale):
        err = np.abs(g.astype(np.float64) - r)
        ratio = float((err / np.maximum(scale, 1e-300)).max())
        print("%s [%s] %s: max |got - ref64| = %.3e, max ratio to ktot * 2^-24 * sum|a||w| = %.4f" % (label, plan, name, err.max(), ratio))
        bad = np.argwhere(err > bound)
        assert not len(bad), "%s [%s] %s: %d elements outside the bound, first %s: err %.3e bound %.3e" % (
            label, plan, name, len(bad), bad[0].tolist(), err[tuple(bad[0])], bound[tuple(bad[0])])
        return ratio
    if case.mode in F32_MODES:
        ratio = judge("outF", got["outF"][:, :case.N], x, e32, unit)
        if "row_seq" in ops:
            assert (got["outF"][ops["row_seq"] < 0].view(np.uint32) == 0).all()
    elif case.mode == F16:
        ratio = judge("outH", got["outH"][:, :case.N], x, e32 + 0.5 * ulp16(np.abs(x) + e32), unit)
    else:
        (xq, xv), (eq, ev), (uq, uv) = _qkv_ref_layout(case, x), _qkv_ref_layout(case, e32), _qkv_ref_layout(case, unit)
        ratio = 0.0
        for name, xr, er, ur in (("outH", xq, eq, uq), ("outVt", xv, ev, uv)):
            g = got[name][:, :xr.shape[1]]
            h16 = 0.5 * ulp16(np.abs(xr) + er)
            if case.mode == QKV:
                ratio = max(ratio, judge(name, g, xr, er + h16, ur))
            else:  # hi as the plain fp16 output; hi + lo = x up to the f32 error and half an fp16 ulp of the remainder (|lo| <= half an ulp of hi)
                judge(name + " (hi)", g, xr, er + h16, ur)
                both = g.astype(np.float64) + got[name + "2"][:, :xr.shape[1]].astype(np.float64)
                ratio = max(ratio, judge(name + " (hi + lo)", both, xr, er + 0.5 * ulp16(h16 + er), ur))
    if case.mode in STATS_MODES:
        # the records against float64 sums of the values the kernel itself stored: a chunk's partial is an f32 sum of 8 x 32 values (and of their squares, each
        # rounded once) in a fixed tree, exact from there on
        stored = got["outF"][:, :case.N].astype(np.float64)
        st, _ = decode_stats(case, ops, got["st"])
        want, mag = np.zeros_like(st), np.zeros_like(st)
        for ch, s in enumerate(ops["chunk_seq"]):
            if s >= 0:
                blk = stored[8 * ch:8 * ch + 8].reshape(8, case.N // 32, 32)
                want[s, :, 0] += blk.sum(axis=(0, 2)); want[s, :, 1] += (blk * blk).sum(axis=(0, 2))
                mag[s, :, 0] += np.abs(blk).sum(axis=(0, 2)); mag[s, :, 1] += (blk * blk).sum(axis=(0, 2))
        assert (np.abs(st - want) <= 257 * u * mag).all(), (label, float((np.abs(st - want) / np.maximum(mag, 1e-300)).max() / u))
    return ratio, got, plan


def _prod(M=None):
    rows = PROD_LENS if M is None else None
    kw = dict(rows=rows) if M is None else dict(M=M)
    out = []
    for mode in range(7):
        out.append(("vh", Case(tag="vh", mode=mode, N=3072 if mode in QKV_MODES else 1024, kseg=1024, resid="sep" if mode in F32_MODES else None, **kw)))
    out.append(("vh concat", Case(tag="concat", N=1024, nseg=2, a_sel=(0, 1, 0), kseg=1024, resid="alias", **kw)))
    for mode in (F32, F32_STATS, F16):
        out.append(("conv3", conv3(mode=mode, N=1024, kseg=1024, resid="sep" if mode != F16 else None, **kw)))
    for mode in (F32_SCALED, F32_SCALED_STATS):
        out.append(("dualb", dualb(1024, mode=mode, N=1024, resid="sep", **kw)))
    for mode in (F32, QKV, QKV_SPLIT):
        out.append(("wreg", Case(tag="wreg", mode=mode, wreg=1, th=8, N=3072 if mode in QKV_MODES else 1024, kseg=1024, **kw)))
    return out


REAL = [(k, c, False) for k, c in _prod()] + [
    ("vh", Case(tag="vh", mode=F16, N=1024, kseg=1024, rows=PROD_LENS), True),
    ("conv3", conv3(N=1024, kseg=1024, rows=PROD_LENS, resid="sep"), True),
    ("wreg", Case(tag="wreg", mode=QKV, wreg=1, th=8, N=3072, kseg=1024, rows=PROD_LENS), True),
    # the benchmark's layout: 32 sequences of T = 870 -> 28 032 packed rows, tile heights and kernels as the launcher chooses them
    ("wreg", Case(tag="wreg", wreg=1, N=1024, kseg=1024, rows=[870] * 32, resid="alias"), False),
    ("wreg", Case(tag="wreg", mode=QKV, wreg=1, N=3072, kseg=1024, rows=[870] * 32), False),
    ("conv3", conv3(N=1024, kseg=1024, rows=[870] * 32, resid="sep"), False),
    ("vh concat", Case(tag="concat", N=1024, nseg=2, a_sel=(0, 1, 0), kseg=1024, rows=[870] * 32), False),
    ("dualb", dualb(1024, N=1024, rows=[870] * 32, resid="sep"), False)]


@pytest.mark.parametrize("kernel,case,heavy", REAL, ids=[c.name + ("-heavy" if h else "") for _, c, h in REAL])
def test_real_valued(lib, kernel, case, heavy):
    if case.M > 20000:
        assert case.M == 28032
    ops = real_operands(case, 1234 + case.mode, heavy)
    _, _, plan = check_real(lib, case, ops, case.name + ("-heavy" if heavy else ""))
    assert plan.split()[0] == kernel.split()[0], plan


def _bits(lib, case, ops):
    rc, outs, plan = run(lib, case, ops)
    assert rc == 0, (case.name, plan, rc)
    return unpack(lib, case, ops, outs), plan


def _same(a, b, what, keys=None):
    for k in (keys or a.keys()):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        n = int((x.view(np.uint8) != y.view(np.uint8)).sum())
        assert n == 0, "%s: %s differs in %d bytes" % (what, k, n)


def _variant(case, **kw):
    d = {k: getattr(case, k) for k in Case.DEFAULTS}
    d.update(kw)
    return Case(**d)


IDENT = {"vh F32": Case(tag="vh", N=1024, kseg=1024, rows=PROD_LENS, resid="sep"),
         "vh F32_STATS": Case(tag="vh", mode=F32_STATS, N=1024, kseg=1024, rows=PROD_LENS, resid="sep"),
         "vh F32_SCALED_STATS": Case(tag="vh", mode=F32_SCALED_STATS, N=1024, kseg=1024, rows=PROD_LENS, resid="alias"),
         "vh QKV": Case(tag="vh", mode=QKV, N=3072, kseg=1024, rows=PROD_LENS),
         "vh QKV_SPLIT": Case(tag="vh", mode=QKV_SPLIT, N=3072, kseg=1024, rows=PROD_LENS),
         "conv3 F32_STATS": conv3(mode=F32_STATS, N=1024, kseg=1024, rows=PROD_LENS, resid="sep"),
         "dualb F32_SCALED_STATS": dualb(1024, mode=F32_SCALED_STATS, N=1024, rows=PROD_LENS, resid="sep")}


@pytest.mark.parametrize("which", ["vh F32_STATS", "vh QKV", "conv3 F32_STATS", "dualb F32_SCALED_STATS"])
def test_identity_tile_heights(lib, which):
    """'bit-identical to every other tiling'; the statistics are the same for every th ('the unit whose value does not depend on the tiling')"""
    base = _variant(IDENT[which], ku=1)
    ops = real_operands(base, 77)
    first, _ = _bits(lib, _variant(base, th=1), ops)
    for th in range(2, 9):
        got, plan = _bits(lib, _variant(base, th=th), ops)
        _same(first, got, "%s th 1 vs %s" % (which, plan))


@pytest.mark.parametrize("which", ["vh F32", "vh F32_SCALED_STATS", "vh QKV_SPLIT"])
def test_identity_k_tiles_per_barrier(lib, which):
    """KU = 2 / 4: 'same products in the same order: bit-identical to KU = 1'"""
    base = _variant(IDENT[which], th=4)
    ops = real_operands(base, 78)
    first, _ = _bits(lib, _variant(base, ku=1), ops)
    for ku in (2, 4):
        got, plan = _bits(lib, _variant(base, ku=ku), ops)
        assert "ku=%d" % ku in plan, plan
        _same(first, got, "%s ku 1 vs %s" % (which, plan))
    auto, plan = _bits(lib, _variant(base, th=0, ku=0), ops)  # the small-problem rule's own choice
    _same(first, auto, "%s ku 1 vs auto (%s)" % (which, plan))


def test_identity_dualb_k_tiles(lib):
    base = _variant(IDENT["dualb F32_SCALED_STATS"], th=4)
    ops = real_operands(base, 79)
    a, pa = _bits(lib, _variant(base, ku=1), ops)
    b, pb = _bits(lib, _variant(base, ku=2), ops)
    assert "dualb" in pa and "ku=1" in pa and "ku=2" in pb, (pa, pb)
    _same(a, b, "dual-B KU 1 vs 2")


@pytest.mark.parametrize("mode", [F32, QKV, QKV_SPLIT])
def test_identity_wreg_equals_vh(lib, mode):
    """gemm_f16_wreg_kernel: 'Bit-identical to gemm_f16_vh_kernel'"""
    base = Case(tag="vh", mode=mode, N=3072 if mode in QKV_MODES else 1024, kseg=1024, rows=PROD_LENS, th=8, ku=1, resid="sep" if mode == F32 else None)
    ops = real_operands(base, 80)
    a, pa = _bits(lib, base, ops)
    b, pb = _bits(lib, _variant(base, wreg=1), ops)
    assert pa.startswith("vh") and pb.startswith("wreg"), (pa, pb)
    _same(a, b, "wreg vs vh, mode %d" % mode)


@pytest.mark.parametrize("which,plain", [("vh F32_STATS", F32), ("vh F32_SCALED_STATS", F32_SCALED), ("conv3 F32_STATS", F32), ("dualb F32_SCALED_STATS", F32_SCALED)])
def test_identity_stats_modes_store_the_plain_output(lib, which, plain):
    base = IDENT[which]
    ops = real_operands(base, 81)
    a, pa = _bits(lib, base, ops)
    b, pb = _bits(lib, _variant(base, mode=plain), ops)
    assert pa.split()[0] == pb.split()[0], (pa, pb)
    _same(a, b, "%s vs its plain mode" % which, keys=["outF"])


# ------------------------------------------------------------------------------------------------------------------------------------ coverage

def _wave_blocks(M, th):
    """per-wave block counts (the MI bodies) and tile lengths a launch of M rows at height th contains"""
    nb, mi, lens = M >> 4, set(), set()
    for x in range(8):
        b0, b1 = nb * x >> 3, nb * (x + 1) >> 3
        for t0 in range(b0, b1, th):
            n = min(th, b1 - t0)
            lens.add(n)
            mi.update(((n + 1) >> 1, n >> 1))
    return mi, lens


def test_coverage(lib):
    """Runs last: what the launcher selected over the exact cases of this session (for a case deselected from this session: what it would select, the plan is host-only)."""
    seen = dict(SEEN)
    for case in EXACT:
        if case.name not in seen:
            s = G.fill_struct(case, G.operands(case))
            buf = C.create_string_buffer(160)
            assert lib.tts_gemm_test_plan(C.byref(s), buf, 160) == 0, case.name
            seen[case.name] = (buf.value.decode(), case)
    pairs, forms, heights, bodies, tails = set(), set(), {}, {}, {}
    for plan, case in seen.values():
        kern = plan.split()[0]
        th, ku = int(plan.split("th=")[1].split()[0]), int(plan.split("ku=")[1].split()[0])
        pairs.add((kern, case.mode))
        forms.add((kern, ku))
        heights.setdefault(kern, set()).add(th)
        mi, lens = _wave_blocks(case.M, th)
        if kern != "wreg":
            bodies.setdefault(kern, set()).update(mi)
        tails.setdefault(kern, set()).update(lens)
    want = {("vh", m) for m in range(7)} | {("conv3", m) for m in (F32, F16, F32_STATS)} | {("dualb", m) for m in (F32_SCALED, F32_SCALED_STATS)} | \
           {("wreg", m) for m in (F32, QKV, QKV_SPLIT)}
    assert pairs == want, (sorted(want - pairs), sorted(pairs - want))
    assert forms == {("vh", 1), ("vh", 2), ("vh", 4), ("dualb", 1), ("dualb", 2), ("conv3", 1), ("wreg", 1)}, sorted(forms)
    for kern in ("vh", "conv3", "dualb"):
        assert heights[kern] == set(range(1, 9)), (kern, heights[kern])
        assert bodies[kern] == {0, 1, 2, 3, 4}, (kern, bodies[kern])
        assert tails[kern] >= {1, 2, 3, 5, 7, 8}, (kern, tails[kern])
    assert heights["wreg"] == {8} and tails["wreg"] == set(range(1, 9)), (heights["wreg"], tails["wreg"])
    # each gemm_auto_th / KU-rule boundary of the four N has an exact case on both sides
    names = {(c.M, c.N) for _, c in seen.values() if c.tag == "boundary"}
    for N in G.BOUNDARY_N:
        bs = G.boundaries(N)
        assert len(bs) >= 2, (N, bs)
        for M in bs:
            assert lib.tts_gemm_test_auto_th(M, N) == G._auto_th(M, N)
            assert {(M - 32, N), (M - 16, N), (M, N), (M + 16, N)} <= names, (N, M)
