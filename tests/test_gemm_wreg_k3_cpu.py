"""Host side of the register-streamed k = 3 convolution (csrc/gemm_f16.h): where gemm_wfrag3_index puts every weight element, against naive loops over the layout the
kernel reads, and the rules by which gemm_plan selects gemm_f16_conv3_wreg_kernel (through the harness's plan entry points; no GPU)."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as G
from gemm_cases import F16, F32, F32_SCALED, F32_STATS, QKV, Case, conv3, dualb


@pytest.fixture(scope="module")
def lib():
    L = G.harness()
    L.tts_gemm_test_plan_images.argtypes = [C.POINTER(G.CaseStruct), C.c_char_p, C.c_int]
    L.tts_gemm_test_plan_images.restype = C.c_int
    L.tts_gemm_test_wfrag3_index.argtypes = [C.c_int] * 5
    L.tts_gemm_test_wfrag3_index.restype = C.c_longlong
    return L


@pytest.mark.parametrize("N,K", [(128, 64), (256, 192), (1024, 1024)])
def test_image_index(lib, N, K):
    """Per tap one image [n / 16][k / 32][lane][8]: wave w of column tile n0 reads, for chunk kc, K step ks and column block j, the 1 KB at
    tap * N * K + (((n0 / 16 + 2 w + j) * (K / 32) + 2 kc + ks) * 64 + lane) * 8, and lane (fr, fq) must find W[n0 + 32 w + 16 j + fr][tap * K + 64 kc + 32 ks + 8 fq ..]."""
    step = 1 if N * K <= 256 * 192 else 37  # the large shape: a stride co-prime to every dimension, plus the corners
    seen = np.zeros(3 * N * K, np.int32) if step == 1 else None
    pts = [(n, tap, k) for tap in range(3) for n in range(N) for k in range(K)][::step]
    if step > 1:
        pts += [(N - 1, 2, K - 1), (0, 0, 0), (N - 1, 0, 0), (0, 2, K - 1)]
    for n, tap, k in pts:
        got = lib.tts_gemm_test_wfrag3_index(n, tap, k, N, K)
        n0, w, j, fr = n // 128 * 128, n % 128 // 32, n % 32 // 16, n % 16
        kc, ks, fq, e = k // 64, k % 64 // 32, k % 32 // 8, k % 8
        want = tap * N * K + (((n0 // 16 + 2 * w + j) * (K // 32) + 2 * kc + ks) * 64 + fq * 16 + fr) * 8 + e
        assert got == want, (n, tap, k, got, want)
        if tap == 0:
            assert got == G.wfrag_index(n, k, K)  # tap 0 (and a k = 1 weight) is the one-segment image
        if seen is not None:
            seen[got] += 1
    if seen is not None:
        assert (seen == 1).all()  # every (n, tap, k) lands once, and nothing else does


def _plan(lib, case, images=True):
    ops = G.operands(case)
    buf = C.create_string_buffer(160)
    f = lib.tts_gemm_test_plan_images if images else lib.tts_gemm_test_plan
    assert f(C.byref(G.fill_struct(case, ops, keep=[])), buf, 160) == 0
    return buf.value.decode()


def test_plan_selection(lib):
    take = conv3(wreg=1, th=8, M=432, N=128, kseg=128)
    assert _plan(lib, take) == "conv3w mode=0 th=8 ku=1 cn=1"
    assert _plan(lib, conv3(wreg=1, th=8, M=432, N=128, kseg=64, resid="sep")).startswith("conv3w ")
    assert _plan(lib, conv3(wreg=1, M=28032, N=1024, kseg=1024, resid="alias")) == "conv3w mode=0 th=8 ku=1 cn=8"   # the launcher's own height at the benchmark's size
    assert _plan(lib, conv3(wreg=1, M=28032, N=1152, kseg=1024)).startswith("conv3w mode=0 th=8 ku=1 cn=3")
    # no image (the entry point every existing case uses), option off, shorter tiles, small grids, other modes: the LDS-staged kernel
    assert _plan(lib, take, images=False).startswith("conv3 ")
    assert _plan(lib, conv3(wreg=0, th=8, M=432, N=128, kseg=128)).startswith("conv3 ")
    for th in range(1, 8):
        assert _plan(lib, conv3(wreg=1, th=th, M=944, N=128, kseg=128)).startswith("conv3 mode=0 th=%d " % th)
    assert _plan(lib, conv3(wreg=1, M=1792, N=1024, kseg=1024)).startswith("conv3 mode=0 th=4 ")
    assert _plan(lib, conv3(wreg=1, th=8, mode=F32_STATS, M=432, N=128, kseg=128)).startswith("conv3 ")
    assert _plan(lib, conv3(wreg=1, th=8, mode=F16, M=432, N=128, kseg=128)).startswith("conv3 ")
    # three segments that are not the k = 3 convolution, and the other classes, plan as before
    assert _plan(lib, Case(tag="custom3", wreg=1, th=8, M=432, N=128, nseg=3, kseg=64, custom_w=1, ldw=320, w_off=(192, 0, 96), row_off=(-1, 0, 1), a_sel=(0, 1, 0))).startswith("vh ")
    assert _plan(lib, Case(tag="wreg", wreg=1, th=8, M=432, N=128, kseg=128)).startswith("wreg ")
    assert _plan(lib, Case(tag="wreg", mode=QKV, wreg=1, th=8, M=432, N=384, kseg=128)).startswith("wreg ")
    assert _plan(lib, dualb(128, wreg=1, th=8, M=432, N=128)).startswith("dualb ")
    assert _plan(lib, Case(tag="concat", wreg=1, th=8, M=432, N=128, nseg=2, a_sel=(0, 1, 0), kseg=128)).startswith("vh ")
