"""gemm_f16_conv3_wreg_kernel (csrc/gemm_f16.h): the k = 3 convolution with its weight streamed into registers from the per-tap fragment-major images, through the
harness entry point that builds those images (tts_gemm_test_run_images). Reference, exactness ladder, bit comparison and the real-valued bound are the ones of
tests/gemm_cases.py and tests/test_gemm_kernels_gpu.py (its check_exact / check_real run here with the image-building entry point in place of tts_gemm_test_run).

Every case asserts the canary margins and sentinels (unpack / assert_bits), that the plan names the new kernel, and that the same case plans to the LDS-staged
kernel with wreg = 0, with th < 8 and in the STATS and F16 modes."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as G
import test_gemm_kernels_gpu as T
from gemm_cases import F16, F32, F32_STATS, RAGGED, UNEVEN_M, conv3

pytestmark = pytest.mark.gpu

BENCH_ROWS = [870] * 32  # the benchmark's layout: 28 032 packed rows


@pytest.fixture(scope="module")
def lib():
    L = G.harness()
    L.tts_gemm_test_run_images.argtypes = [C.POINTER(G.CaseStruct)]
    L.tts_gemm_test_plan_images.argtypes = [C.POINTER(G.CaseStruct), C.c_char_p, C.c_int]
    L.tts_gemm_test_run_images.restype = L.tts_gemm_test_plan_images.restype = C.c_int
    return L


def run_images(lib, case, ops, **override):
    """test_gemm_kernels_gpu.run on the entry point that also builds the k = 3 images"""
    margin = lib.tts_gemm_test_margin()
    outs = G.out_buffers(case, ops, margin)
    keep = []
    s = G.fill_struct(case, ops, outs=outs, keep=keep, **override)
    rc = lib.tts_gemm_test_run_images(C.byref(s))
    buf = C.create_string_buffer(160)
    lib.tts_gemm_test_last_kernel(buf, 160)
    return rc, outs, buf.value.decode()


@pytest.fixture()
def images(monkeypatch):
    monkeypatch.setattr(T, "run", run_images)


def plan_images(lib, case, ops, **override):
    buf = C.create_string_buffer(160)
    rc = lib.tts_gemm_test_plan_images(C.byref(G.fill_struct(case, ops, keep=[], **override)), buf, 160)
    assert rc == 0, (case.name, override, rc)
    return buf.value.decode()


def assert_plans(lib, case, ops, plan):
    assert plan.split()[0] == "conv3w" and "th=8" in plan, (case.name, plan)
    assert plan_images(lib, case, ops) == plan
    for kw in (dict(wreg=0), dict(th=4), dict(th=7), dict(mode=F32_STATS, rows=case.rows if case.rows is not None else "valid"), dict(mode=F16, resid=None)):
        other = T._variant(case, **kw)
        o2 = dict(ops)  # a plan reads shapes and flags, not values: the same operands, plus the arrays a STATS case names
        if other.mode == F32_STATS:
            o2.setdefault("row_seq", np.zeros(case.M, np.int32))
            o2["chunk_seq"] = G.layout(case.rows)[2] if isinstance(case.rows, (list, tuple)) else np.zeros(case.M // 8, np.int32)
        # a statistics record is indexed seq * 32 + column / 32, so the harness takes a STATS case wider than 1024 columns only without records
        # (test_gemm_kernels_gpu's "no st_out" / "no chunk_seq" cases); the plan does not depend on them
        no_records = dict(has_st=0, has_chunk_seq=0, st_stripe_ll=0) if other.mode == F32_STATS and other.N > 1024 else {}
        p = plan_images(lib, other, o2, **no_records)
        assert p.split()[0] == "conv3", (case.name, kw, p)
    buf = C.create_string_buffer(160)  # the entry point without images keeps the case on the LDS-staged kernel
    assert lib.tts_gemm_test_plan(C.byref(G.fill_struct(case, ops, keep=[])), buf, 160) == 0 and buf.value.decode().split()[0] == "conv3", buf.value


def _exact_cases():
    c = []
    resids = (None, "sep", "alias")
    for i, M in enumerate(UNEVEN_M):  # last tiles of 1 .. 8 blocks: both bodies, every clamp of the slab
        c.append(conv3(wreg=1, th=8, M=M, N=128, kseg=128, resid=resids[i % 3], bias=i % 2 == 0))
        c.append(conv3(wreg=1, th=8, M=M, N=256, kseg=256, resid=resids[(i + 1) % 3], bias=i % 2 == 1, rows="valid"))
    i = 0
    for N in (128, 1024, 1152):
        for kseg in (128, 256, 1024):
            for M in (432, 1200):
                c.append(conv3(wreg=1, th=8, M=M, N=N, kseg=kseg, resid=resids[i % 3], bias=i % 2 == 0))
                i += 1
    for resid in resids:
        for bias in (True, False):
            c.append(conv3(wreg=1, th=8, N=256, kseg=128, rows=RAGGED, resid=resid, bias=bias))
    c.append(conv3(wreg=1, th=8, N=128, kseg=64, rows=RAGGED, resid="sep"))    # one chunk
    c.append(conv3(wreg=1, th=8, N=128, kseg=192, rows=RAGGED, resid="alias"))  # an odd number of chunks
    for resid in resids:  # leading dimensions wider than the payload
        c.append(conv3(wreg=1, th=8, M=688, N=1024, kseg=256, resid=resid, pad=8))
        c.append(conv3(wreg=1, th=8, N=128, kseg=128, rows=RAGGED, resid=resid, pad=24, bias=False))
    c.append(conv3(wreg=1, th=8, N=128, kseg=128, rows=BENCH_ROWS, resid="sep"))  # one column tile: the launcher's own choice here is 32-row tiles
    c.append(conv3(wreg=1, N=1024, kseg=256, rows=BENCH_ROWS, resid="alias"))  # the height the launcher chooses
    c.append(conv3(wreg=1, N=1152, kseg=128, rows=BENCH_ROWS, bias=False))      # cn = 3
    return c


EXACT = _exact_cases()


@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_exact(lib, images, case):
    if case.M > 20000:
        assert case.M == 28032
    try:
        plan = T.check_exact(lib, case)
    finally:
        T.SEEN.pop(case.name, None)  # test_gemm_kernels_gpu.test_coverage counts its own cases
    assert_plans(lib, case, G.operands(case), plan)


IDENT = [("M1792 resid", conv3(N=1024, kseg=1024, rows=T.PROD_LENS, th=8, resid="sep")),
         ("M1792", conv3(N=1024, kseg=1024, rows=T.PROD_LENS, th=8)),
         ("M28032 resid alias", conv3(N=1024, kseg=1024, rows=BENCH_ROWS, resid="alias")),
         ("M28032", conv3(N=1024, kseg=1024, rows=BENCH_ROWS, bias=False))]


@pytest.mark.parametrize("what,base", IDENT, ids=[w for w, _ in IDENT])
def test_identity_with_the_lds_staged_kernel(lib, what, base):
    """'bit-identical to gemm_f16_conv3_vh_kernel', on Gaussian operands"""
    assert base.M == (1792 if "1792" in what else 28032)
    ops = T.real_operands(base, 90)
    rc, outs, pa = T.run(lib, base, ops)
    assert rc == 0 and pa.split()[0] == "conv3", (pa, rc)
    a = T.unpack(lib, base, ops, outs)
    case = T._variant(base, wreg=1)
    rc, outs, pb = run_images(lib, case, ops)
    assert rc == 0 and pb.split()[0] == "conv3w", (pb, rc)
    b = T.unpack(lib, case, ops, outs)
    T._same(a, b, "conv3w vs conv3, %s" % what)


REAL = [(conv3(wreg=1, th=8, N=1024, kseg=1024, rows=T.PROD_LENS, resid="sep"), False),
        (conv3(wreg=1, th=8, N=1024, kseg=1024, rows=T.PROD_LENS, resid="sep"), True),
        (conv3(wreg=1, N=1024, kseg=1024, rows=BENCH_ROWS, resid="sep"), False)]


@pytest.mark.parametrize("case,heavy", REAL, ids=[c.name + ("-heavy" if h else "") for c, h in REAL])
def test_real_valued(lib, images, case, heavy):
    """the bound of test_gemm_kernels_gpu.test_real_valued (C_ACC = 1)"""
    assert T.C_ACC == 1
    ops = T.real_operands(case, 1234 + case.mode, heavy)
    _, _, plan = T.check_real(lib, case, ops, case.name + ("-heavy" if heavy else ""))
    assert plan.split()[0] == "conv3w", plan
