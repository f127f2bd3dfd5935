"""gemm_epilogue_wreg_qkv_lds (csrc/gemm_f16.h): the fp16 QKV tile of gemm_f16_wreg_kernel parked in LDS and stored in whole cache lines (GemmArgs::wreg bit 1;
the harness passes a case's `wreg` through, so wreg = 1 is the epilogue that stores straight from the registers and wreg = 3 the one through LDS).

Both epilogues run on the same operands and outH / outVt must be BYTE-EQUAL over the whole allocation: the harness pre-fills every output with a sentinel and
copies margin | payload | margin back, so a store too many (leading-dimension padding, rows past a short tile, the canary margins) or too few shows up as a
difference. ldvt = rows + 128 as the engine allocates vt16 (pad = 128 widens lda and ldh by as much).

Shapes. The kernel takes 128-row tiles (th = 8) and K >= 128; at K = 64 both values of wreg must plan to the LDS-staged kernel, which the K = 64 cases assert.
The XCD split hands a tile nblk = 1 .. 8 sixteen-row blocks: M = 128 gives one block per XCD, 896 seven, 1200 tiles of 8 and of 1 / 2 blocks, 688 of 5 / 6 (the
8-block body) and 432 of 3 / 4 (the 4-block body). N = 384 holds the three kinds of column tile (q | k, v | q, k | v), N = 3072 the engine's sixteen heads.
One exact case pins the new epilogue itself to the float64 reference (tests/gemm_cases.py), zero mismatches."""
import numpy as np
import pytest

import gemm_cases as G
import test_gemm_kernels_gpu as T
from gemm_cases import QKV, Case

pytestmark = pytest.mark.gpu

PAD = 128
# one sequence of 1 .. 129 rows (layout(): first row 8, a guard row behind, rows rounded up to 128), two sequences meeting inside a tile, a last sequence ending at 870 of 896
ROWS = [[1], [7], [8], [102], [128], [129], [60, 50], [400, 454]]
PLAIN_M = [128, 432, 688, 1200]  # no row_seq


def _operands(case, seed):
    rs = np.random.RandomState(seed)
    M, K = case.M, case.kseg
    ops = {"nseq": 1}
    A = rs.randn(M + 2, K + case.pad)
    if isinstance(case.rows, (list, tuple)):
        _, row_seq, _, _ = G.layout(case.rows)
        ops.update(row_seq=row_seq, nseq=len(case.rows))
        A[1:M + 1][row_seq < 0] = 0
        A[0] = 0
        A[M + 1] = 0
    ops["A0"] = A.astype(np.float16)
    ops["W"] = (rs.randn(case.N, K) / np.sqrt(K)).astype(np.float16)
    if case.bias:
        ops["bias"] = rs.randn(case.N).astype(np.float32)
    return ops


def _cases():
    c = []
    for N in (384, 3072):
        for K in (64, 1024):
            for bias in (True, False):
                for rows in ROWS:
                    c.append(Case(tag="qkv", mode=QKV, wreg=1, th=8, N=N, kseg=K, rows=rows, bias=bias, pad=PAD))
                for M in PLAIN_M:
                    c.append(Case(tag="qkv", mode=QKV, wreg=1, th=8, M=M, N=N, kseg=K, bias=bias, pad=PAD))
    c.append(Case(tag="qkv", mode=QKV, wreg=1, th=8, N=384, kseg=128, rows=[60, 50], pad=PAD))  # two K tiles: the shortest ring walk
    c.append(Case(tag="qkv", mode=QKV, wreg=1, N=3072, kseg=1024, rows=[870] * 4 + [300], pad=PAD, bias=False))  # the launcher's own height (8) and column chunks
    return c


CASES = _cases()
IDS = [c.name + ("-" + "+".join(str(n) for n in c.rows) if isinstance(c.rows, list) and len(c.rows) < 3 else "") for c in CASES]


def test_layouts_are_the_ones_meant():
    assert G.layout([400, 454])[0] == 896 and G.layout([400, 454])[3][1] + 454 == 870
    assert G.layout([60, 50])[0] == 128 and [G.layout([n])[0] for n in (102, 128, 129)] == [128, 256, 256]


@pytest.fixture(scope="module")
def lib():
    return G.harness()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_byte_equal_to_the_direct_stores(lib, case):
    ops = _operands(case, 7 + case.M + case.N + case.kseg)
    rc, old, plan_old = T.run(lib, case, ops)
    assert rc == 0, (case.name, plan_old, rc)
    new_case = T._variant(case, wreg=3)
    rc, new, plan_new = T.run(lib, new_case, ops)
    assert rc == 0, (case.name, plan_new, rc)
    if case.kseg >= 128:
        assert plan_old.split()[0] == "wreg" and "qkv_lds" not in plan_old and "th=8" in plan_old, plan_old
        assert plan_new == plan_old + " qkv_lds", (plan_old, plan_new)
    else:
        assert plan_old.split()[0] == "vh" and plan_new == plan_old, (plan_old, plan_new)
    T.unpack(lib, case, ops, old)  # canary margins
    T.unpack(lib, new_case, ops, new)
    for k in ("outH", "outVt"):
        n = int((old[k] != new[k]).sum())
        assert n == 0, "%s [%s]: %s differs in %d of %d bytes (margins and padding included)" % (case.name, plan_new, k, n, old[k].size)
    got = T.unpack(lib, new_case, ops, new)
    assert (got["outH"][:, :case.N // 192 * 128].view(np.uint16) != 0xCBCB).any() and (got["outVt"][:, :case.M].view(np.uint16) != 0xCBCB).any()  # the launches wrote


def test_misaligned_leading_dimension_keeps_the_direct_stores(lib):
    """16-byte stores need rows of outH / outVt that start at multiples of 8 halves: with ldvt = M + 4 the plan must not name the epilogue through LDS"""
    case = Case(tag="qkv", mode=QKV, wreg=3, th=8, M=432, N=384, kseg=128, pad=8)
    ops = _operands(case, 3)
    rc, outs, plan = T.run(lib, case, ops, ldvt=case.M + 4)  # the host buffers keep the size of ldvt = M + 8: compared as raw bytes
    assert rc == 0 and plan.split()[0] == "wreg" and "qkv_lds" not in plan, (rc, plan)
    rc, ref, plan = T.run(lib, T._variant(case, wreg=1), ops, ldvt=case.M + 4)
    assert rc == 0 and plan.split()[0] == "wreg", (rc, plan)
    for k in ("outH", "outVt"):
        assert (outs[k] == ref[k]).all(), k


EXACT = [Case(tag="qkv", mode=QKV, wreg=3, th=8, N=384, kseg=128, rows=G.RAGGED, pad=PAD),
         Case(tag="qkv", mode=QKV, wreg=3, th=8, M=1200, N=768, kseg=256, pad=8, bias=False)]


@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_exact(lib, case):
    """small-integer operands against the float64 product rounded once to fp16 (test_gemm_kernels_gpu.check_exact): zero mismatches"""
    try:
        plan = T.check_exact(lib, case)
    finally:
        T.SEEN.pop(case.name, None)  # test_gemm_kernels_gpu.test_coverage counts its own cases
    assert plan.split()[0] == "wreg" and plan.endswith(" qkv_lds"), plan
