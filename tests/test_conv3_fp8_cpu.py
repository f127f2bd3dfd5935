"""Option "conv3_fp8" on a host-only context, the predicate that admits the fp8 convolution, and a float32 numpy restatement of gemm_f8_conv3_kernel's arithmetic
against the bound tests/test_gemm_f8_kernels_gpu.py holds the kernel to."""
import numpy as np
import pytest

import conv3_fp8_cases as F


def test_option_values(pkg):
    e = pkg.Engine(-1)
    for v in (0, 1, 0):
        e.set_option("conv3_fp8", v)
    for bad in (2, -1, 0.5, float("nan")):
        assert e.L.tts_set_option(e.h, b"conv3_fp8", float(bad)) == -1 and b"conv3_fp8" in e.L.tts_last_error(e.h)
        with pytest.raises(pkg.TtsError, match="conv3_fp8"):
            e.set_option("conv3_fp8", bad)
    e.close()


@pytest.mark.parametrize("args,want", [((1, 1, 0, 0, 28032, 1024, 1024), 1), ((0, 1, 0, 0, 28032, 1024, 1024), 0), ((1, 0, 0, 0, 28032, 1024, 1024), 0),
                                       ((1, 1, 1, 0, 28032, 1024, 1024), 0), ((1, 1, 0, 1, 28032, 1024, 1024), 0), ((1, 1, 0, 0, 1792, 1024, 1024), 0),
                                       ((1, 1, 0, 0, 28032, 1024, 1088), 0)])
def test_takes(args, want):
    """off, no images, latency-mode statistics, debug checksums, a layout of short tiles, a K that is no multiple of 128: the fp16 path"""
    assert F.harness().tts_f8_test_takes(*args) == want


@pytest.mark.parametrize("K", [128, 1024])
def test_float32_restatement_inside_the_bound(K):
    """the kernel's arithmetic in float32 (one tap and one 128-channel chunk at a time, then scale, bias, residual) on the Gaussian inputs"""
    rs = np.random.RandomState(K)
    N = 128
    _, _, M, rows_total, row_seq = F.layout([5, 130])
    live = row_seq >= 0
    a = np.clip(rs.randn(M + 2, K) * 100.0, -448, 448)
    a[1:M + 1][~live] = 0
    a[0] = a[M + 1] = 0
    A, W = F.decode(F.encode(a)), F.decode(F.encode(np.clip(rs.randn(N, 3, K) * 100.0, -448, 448)))
    inv_a = np.where(live, 2.0 ** -(6.0 + np.maximum(row_seq, 0)), 0).astype(np.float32)
    inv_w = (2.0 ** -(8.0 + np.arange(N) % 3)).astype(np.float32)
    bias, resid = rs.randn(N).astype(np.float32), rs.randn(M, N).astype(np.float32)
    acc = np.zeros((M, N), np.float32)
    for k0 in range(0, K, 128):
        for t in range(3):
            acc = acc + (A[t:t + M, k0:k0 + 128].astype(np.float32) @ W[:, t, k0:k0 + 128].astype(np.float32).T)
    got = (acc * (inv_a[:, None] * inv_w[None, :]) + bias[None, :]) + resid
    want = F.conv_ref(A, W, inv_a, inv_w, bias, resid.astype(np.float64), None)
    bound = F.conv_bound(A, W, inv_a, inv_w, bias, resid.astype(np.float64))
    assert (np.abs(got.astype(np.float64) - want)[live] <= bound[live]).all()
