"""CPU side of tests/test_gemm_kernels_gpu.py: the harness library builds for gfx950 and exports its surface; the float64 NumPy reference the GPU tests compare
against is itself checked against naive loops (a wrong reference cannot pass a wrong kernel); gemm_wfrag_index is a bijection; and the exactness condition of
the exact tests holds for EVERY case of the matrix, so the GPU run cannot meet a case that had to be left out."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import gemm_cases as G
from gemm_cases import F16, F32, F32_MODES, F32_SCALED, F32_SCALED_STATS, F32_STATS, QKV, QKV_MODES, QKV_SPLIT, SCALED_MODES, STATS_MODES, Case, conv3, dualb

EXACT = G.exact_cases()


def test_harness_library_builds_and_exports_its_surface():
    L = G.harness()  # builds it once if missing; raises otherwise
    for sym in ("tts_gemm_test_run", "tts_gemm_test_auto_th", "tts_gemm_test_last_kernel", "tts_gemm_test_plan", "tts_gemm_test_margin"):
        assert hasattr(L, sym), sym
    assert L.tts_gemm_test_margin() >= 2048
    assert os.path.getmtime(G.LIB) >= os.path.getmtime(G.SRC) or os.environ.get("TTS_LIB_PATH"), "libtts_gemm_test.so is older than its source: run make"


def test_harness_is_not_part_of_the_product():
    mk = open(os.path.join(G.PKG, "Makefile")).read()
    assert "HIP_SRCS = $(wildcard csrc/*.hip)" in mk and not os.path.exists(os.path.join(G.PKG, "csrc", "gemm_harness.hip"))
    src = open(G.SRC).read()
    assert "tortoise_mi355x.h" not in src and "asm" not in src  # no product ABI, no inline assembly of its own


def test_auto_th_and_plan_match_their_restatement():
    L = G.harness()
    for N in G.BOUNDARY_N:
        for M in range(16, G.BOUNDARY_M_MAX + 1, 16):
            assert L.tts_gemm_test_auto_th(M, N) == G._auto_th(M, N), (M, N)
        bs = G.boundaries(N)
        assert len(bs) >= 2 and all(16 < b <= G.BOUNDARY_M_MAX - 16 for b in bs), (N, bs)
    # the plan of every boundary case: height and KU as the restated rules say
    for case in G.boundary_cases():
        s = G.fill_struct(case, G.operands(case))
        buf = C.create_string_buffer(160)
        assert L.tts_gemm_test_plan(C.byref(s), buf, 160) == 0, case.name
        small = G._small_rule(case.M, case.N)
        th = 4 if small else G._auto_th(case.M, case.N)
        kern = "wreg" if case.wreg and th == 8 else "vh"
        assert buf.value.decode().startswith("%s mode=0 th=%d ku=%d " % (kern, th, 4 if small else 1)), (case.name, buf.value)


def test_every_exact_case_is_valid_and_exact():
    """the exactness condition, evaluated on the CPU for the whole matrix; the harness accepts every case (nothing launched: plan only)"""
    L = G.harness()
    assert len({c.name for c in EXACT}) == len(EXACT)
    narrowed = 0
    for case in EXACT:
        ops = G.operands(case)
        worst = G.exactness(case, ops)
        assert worst < 2.0 ** 24, (case.name, worst)
        narrowed += ops["ra"] < 4
        for k in ("A0", "A1", "W"):
            if k in ops:
                assert ops[k].dtype == np.float16 and np.isfinite(ops[k]).all()
        if case.sub:
            a = np.abs(ops["A0"].astype(np.float64))
            assert a.max() < 2.0 ** -14 and (a > 0).any(), "operand A of a subnormal case is not subnormal"
        s = G.fill_struct(case, ops)
        buf = C.create_string_buffer(160)
        assert L.tts_gemm_test_plan(C.byref(s), buf, 160) == 0, case.name
    assert narrowed < len(EXACT) // 4  # most cases run at the full range


def test_ragged_layout_puts_guards_at_every_block_position():
    rows, rs, cs, start = G.layout(G.RAGGED)
    assert rows % 128 == 0 and start[0] == 8 and all(s % 8 == 0 for s in start)
    assert {int(r) & 15 for r in np.flatnonzero(rs < 0)} == set(range(16))
    for s, (b, n) in enumerate(zip(start, G.RAGGED)):
        assert rs[b - 1] < 0 and rs[b + n] < 0 and (rs[b:b + n] == s).all()
    for ch in range(rows // 8):
        owners = {int(v) for v in rs[8 * ch:8 * ch + 8] if v >= 0}
        assert owners == ({int(cs[ch])} if cs[ch] >= 0 else set()), ch
    assert G.layout([870] * 32)[0] == 28032


def test_wfrag_index_is_a_bijection():
    for N, K in {(c.N, c.kseg) for c in EXACT if c.wreg} | {(1024, 1024), (3072, 1024)}:
        n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
        idx = G.wfrag_index(n, k, K).ravel()
        assert idx.min() == 0 and idx.max() == N * K - 1 and len(np.unique(idx)) == N * K, (N, K)
    # the layout the header describes: Wf[n / 16][k / 32][lane = ((k % 32) / 8) * 16 + n % 16][k % 8]
    for n, k, K in ((0, 0, 64), (17, 45, 128), (127, 63, 64), (35, 200, 256)):
        want = (((n // 16) * (K // 32) + k // 32) * 64 + ((k % 32) // 8) * 16 + n % 16) * 8 + k % 8
        assert G.wfrag_index(n, k, K) == want


def _naive(case, ops):
    """the header's formula in plain loops, float64, and the epilogue element by element"""
    M, N, ks = case.M, case.N, case.kseg
    W = ops["W"].astype(np.float64)
    x = np.zeros((M, N))
    for m in range(M):
        guard = "row_seq" in ops and ops["row_seq"][m] < 0
        for n in range(N):
            acc = 0.0
            for s in range(case.nseg):
                A = ops["A%d" % case.a_sel[s]].astype(np.float64)
                for k in range(ks):
                    acc += A[m + case.row_off[s] + 1][k] * W[n][case.offs[s] + k]
            v = acc * (case.alpha if case.mode in SCALED_MODES else 1.0)
            v += float(ops["bias"][n]) if case.bias else 0.0
            v += float(ops["resid"][m][n]) if case.resid else 0.0
            x[m][n] = 0.0 if guard else v
    out = {"x": x}
    if case.mode in F32_MODES:
        out["outF"] = x.astype(np.float32)
    elif case.mode == F16:
        out["outH"] = x.astype(np.float16)
    else:
        heads = N // 192
        out["outH"], out["outVt"] = np.zeros((M, heads * 128), np.float16), np.zeros((heads * 64, M), np.float16)
        out["outH2"], out["outVt2"] = np.zeros_like(out["outH"]), np.zeros_like(out["outVt"])
        for m in range(M):
            for n in range(N):
                h, w = n // 192, n % 192
                hi = np.float16(x[m][n])
                lo = np.float16(x[m][n] - float(hi))
                if w < 128:
                    out["outH"][m][h * 128 + w], out["outH2"][m][h * 128 + w] = hi, lo
                else:
                    out["outVt"][h * 64 + w - 128][m], out["outVt2"][h * 64 + w - 128][m] = hi, lo
    if case.mode in STATS_MODES:
        st = np.zeros((ops["nseq"], N // 32, 2))
        stored = out["outF"].astype(np.float64)
        for m in range(M):
            s = ops["chunk_seq"][m // 8]
            if s >= 0:
                for n in range(N):
                    st[s][n // 32][0] += stored[m][n]
                    st[s][n // 32][1] += stored[m][n] ** 2
        out["stats"] = st * case.launches
    return out


TINY = [Case(M=16, N=128, kseg=64, resid="sep"),
        Case(mode=F16, M=16, N=128, nseg=2, a_sel=(0, 1, 0), kseg=64, rows=[5]),
        Case(mode=QKV, M=16, N=384, kseg=64, rows=[3]),
        Case(mode=QKV_SPLIT, M=16, N=384, kseg=64, sub=True),
        Case(mode=F32_SCALED, M=16, N=128, kseg=64, resid="alias", alpha=0.25),
        Case(mode=F32_STATS, M=128, N=128, kseg=64, rows=[5, 14, 9], launches=2),
        conv3(mode=F32_STATS, N=128, kseg=64, rows=[5, 14, 9], resid="sep"),
        conv3(M=32, N=128, kseg=64),
        dualb(64, mode=F32_SCALED_STATS, M=32, N=128, resid="sep", alpha=2.0),
        Case(M=32, N=128, nseg=3, kseg=64, custom_w=1, ldw=320, w_off=(192, 0, 96), row_off=(-1, 0, 1), a_sel=(0, 1, 0))]


@pytest.mark.parametrize("case", TINY, ids=[c.name for c in TINY])
def test_reference_against_naive_loops(case):
    ops = G.operands(case)
    ref, naive = G.reference(case, ops), _naive(case, ops)
    keys = [k for k in ("outF", "outH", "outVt", "outH2", "outVt2", "stats") if k in ref]
    assert keys and (case.mode != QKV_SPLIT or "outVt2" in keys) and (case.mode not in STATS_MODES or "stats" in keys)
    for k in keys:
        a, b = np.ascontiguousarray(ref[k]), np.ascontiguousarray(naive[k])
        assert a.dtype == b.dtype and a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all(), (case.name, k)
    assert np.abs(ref["x"]).max() > 0
    if case.mode == QKV_SPLIT:  # the low halves carry information: hi + lo restores what hi alone lost
        assert (ref["outH2"] != 0).any() or case.sub


def test_conv3_reference_reads_only_zero_guards_at_sequence_ends():
    """per-sequence k = 3 convolution with zero padding == the row-shifted GEMM over the packed layout, on the first and last row of every sequence (whose
    neighbours in the packing are other sequences' guard rows, while the sequence's own neighbours are non-zero)"""
    case = conv3(N=128, kseg=64, rows=G.RAGGED, bias=False)
    ops = G.operands(case)
    ref = G.reference(case, ops)["x"]
    _, rs, _, start = G.layout(G.RAGGED)
    A, W = ops["A0"].astype(np.float64)[1:-1], ops["W"].astype(np.float64)
    for b, n in zip(start, G.RAGGED):
        xs = np.zeros((n + 2, 64))
        xs[1:-1] = A[b:b + n]
        assert n < 2 or np.abs(xs[1:-1]).sum() > 0
        y = sum(xs[tap:tap + n] @ W[:, tap * 64:(tap + 1) * 64].T for tap in range(3))
        assert (y == ref[b:b + n]).all()


def test_real_valued_bound_is_the_references_own():
    """the bound of test_real_valued holds for a plain f32 accumulation in K order (and in reverse) of the same operands: c = 1 is not a fit to the kernel"""
    rs = np.random.RandomState(5)
    a, w = rs.randn(8, 1024).astype(np.float16), (rs.randn(16, 1024) / 32).astype(np.float16)
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    S = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    for order in (slice(None), slice(None, None, -1)):
        acc = np.zeros((8, 16), np.float32)
        for k in np.arange(1024)[order]:
            acc = acc + a[:, k].astype(np.float32)[:, None] * w[:, k].astype(np.float32)[None, :]
        assert (np.abs(acc - ref) <= 1024 * 2.0 ** -24 * S).all()
