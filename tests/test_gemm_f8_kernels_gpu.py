"""csrc/gemm_f8.h through its harness (testlib/gemm_f8_harness.hip): gemm_f8_conv3_kernel, the activation quantiser and the weight packer, each against a plain
float64 / torch.float8_e4m3fn reference. One launch per harness call; every convolution case checks the canary margins and the rows past rows_total."""
import numpy as np
import pytest

import conv3_fp8_cases as F

pytestmark = pytest.mark.gpu

# one sequence of 1 / 127 / 128 / 129 rows; 5 + 130 rows: two sequences with different scales that meet, guard rows between them, inside the first 128-row tile
LAYOUTS = [[1], [127], [128], [129], [5, 130]]
SHAPES = [(128, 128, False), (256, 256, True), (384, 128, True), (128, 256, False)]  # K, N, resid


def operands(lens, K, N, resid, seed, exact):
    rs = np.random.RandomState(seed)
    start, ln, M, rows_total, row_seq = F.layout(lens)
    live = row_seq >= 0
    if exact:  # small integers: exact in e4m3, every partial sum below 2^24; power-of-two scales; bias and residual on a coarse grid
        a = rs.randint(-8, 9, (M, K)).astype(np.float64)
        W = rs.randint(-4, 5, (N, 3, K)).astype(np.float64)
        inv_a = np.where(live, 2.0 ** -(3 + 2 * np.maximum(row_seq, 0)), 0).astype(np.float32)
        inv_w = (2.0 ** -(np.arange(N) % 4)).astype(np.float32)
        bias = (rs.randint(-64, 65, N) / 4.0).astype(np.float32)
        res = rs.randint(-64, 65, (M, N)) / 8.0 if resid else None
    else:
        a = np.clip(rs.randn(M, K) * 100.0, -448, 448)  # torch's e4m3fn has no saturation
        W = np.clip(rs.randn(N, 3, K) * 100.0, -448, 448)
        inv_a = np.where(live, 2.0 ** -(6 + np.maximum(row_seq, 0)), 0).astype(np.float32)
        inv_w = (2.0 ** -(8 + np.arange(N) % 3)).astype(np.float32)
        bias = rs.randn(N).astype(np.float32)
        res = rs.randn(M, N).astype(np.float32).astype(np.float64) if resid else None
    a[~live] = 0
    A8 = np.zeros((M + 2, K), np.uint8)
    A8[1:M + 1] = F.encode(a)
    return A8, F.encode(W), inv_a, inv_w, bias, res, row_seq, rows_total


CASES = [(lens, K, N, r) for lens in LAYOUTS for K, N, r in SHAPES]
GAUSS = CASES + [(lens, 1024, 128, True) for lens in ([129], [5, 130])]
ids = lambda cs: ["%s-K%d-N%d%s" % ("+".join(map(str, l)), K, N, "-resid" if r else "") for l, K, N, r in cs]


@pytest.mark.parametrize("lens,K,N,resid", CASES, ids=ids(CASES))
def test_exact(lens, K, N, resid):
    A8, W8, inv_a, inv_w, bias, res, row_seq, rows_total = operands(lens, K, N, resid, 7 * K + N + len(lens), True)
    got = F.run_conv(A8, W8, inv_a, inv_w, bias, res, row_seq, rows_total, alias=resid and K == 256)
    want = F.conv_ref(F.decode(A8), F.decode(W8), inv_a, inv_w, bias, res, row_seq).astype(np.float32)
    assert (got[:rows_total].view(np.uint32) == want[:rows_total].view(np.uint32)).all()


@pytest.mark.parametrize("where", ["first", "last"])
def test_planted(where):
    """a single non-zero at the first (last) row and channel of the second sequence: a tap that read across a guard row or off the slab end would show it elsewhere"""
    K, N = 256, 128
    _, W8, inv_a, inv_w, bias, _, row_seq, rows_total = operands([5, 130], K, N, False, 3, True)
    start = F.layout([5, 130])[0]
    r, c = (start[1], 0) if where == "first" else (start[1] + 129, K - 1)
    a = np.zeros((len(row_seq) + 2, K))
    a[r + 1, c] = 6.0
    A8 = F.encode(a)
    got = F.run_conv(A8, W8, inv_a, inv_w, bias, None, row_seq, rows_total)
    want = F.conv_ref(a, F.decode(W8), inv_a, inv_w, bias, None, row_seq).astype(np.float32)
    assert (got[:rows_total].view(np.uint32) == want[:rows_total].view(np.uint32)).all()
    touched = np.nonzero((want != bias[None, :] * (row_seq >= 0)[:, None]).any(1))[0]
    assert set(touched) <= {r - 1, r, r + 1} and r in touched


@pytest.mark.parametrize("lens,K,N,resid", GAUSS, ids=ids(GAUSS))
def test_gaussian(lens, K, N, resid):
    """against float64 on the kernel's own fp8 bytes: operand rounding is not in the distance"""
    A8, W8, inv_a, inv_w, bias, res, row_seq, rows_total = operands(lens, K, N, resid, K + 3 * N + len(lens), False)
    got = F.run_conv(A8, W8, inv_a, inv_w, bias, res, row_seq, rows_total)
    again = F.run_conv(A8, W8, inv_a, inv_w, bias, res, row_seq, rows_total)
    A, W = F.decode(A8), F.decode(W8)
    want = F.conv_ref(A, W, inv_a, inv_w, bias, res, row_seq)
    bound = F.conv_bound(A, W, inv_a, inv_w, bias, res)
    live = row_seq[:rows_total] >= 0
    err = np.abs(got[:rows_total].astype(np.float64) - want[:rows_total])[live]
    print("worst error over bound %.3f" % (err / bound[:rows_total][live]).max())
    assert (err <= bound[:rows_total][live]).all()
    assert (got[:rows_total][~live] == 0).all()
    assert (got[:rows_total].view(np.uint32) == again[:rows_total].view(np.uint32)).all()


def quantise(x16, lens):
    L = F.harness()
    start, ln, M, _, row_seq = F.layout(lens)
    A = np.zeros((M, x16[0].shape[1]), np.float16)
    for s, (a, n) in enumerate(zip(start, lens)):
        A[a:a + n] = x16[s]
    A8, inv_a = np.zeros((M, A.shape[1]), np.uint8), np.zeros(M, np.float32)
    assert L.tts_f8_test_quant(A, M, A.shape[1], len(lens), start, ln, A8, inv_a) == 0
    return A, A8, inv_a, start, row_seq


def test_quantiser():
    rs = np.random.RandomState(5)
    lens, Cn = [1, 8, 129, 896], 1024
    xs = [(rs.randn(n, Cn) * 3).astype(np.float16) for n in lens]
    xs[1][:] = 0          # an all-zero sequence
    xs[2][77, 513] = 3e4  # one outlier
    A, A8, inv_a, start, row_seq = quantise(xs, lens)
    for s, (a, n) in enumerate(zip(start, lens)):
        amax = float(np.abs(xs[s].astype(np.float32)).max())
        sc = 1.0 / float(inv_a[a])
        assert (inv_a[a:a + n] == inv_a[a]).all() and np.log2(sc) == np.round(np.log2(sc))
        assert sc == 1.0 if amax == 0 else 224 <= amax * sc < 448, (s, amax, sc)
        assert (A8[a:a + n] == F.encode(xs[s].astype(np.float32) * np.float32(sc))).all(), s
    assert (A8[row_seq < 0] == 0).all() and (inv_a[row_seq < 0] == 0).all()
    _, alone8, alone_inv, st1, _ = quantise([xs[2]], [lens[2]])  # a sequence alone = the sequence in the batch
    assert (alone8[st1[0]:st1[0] + 129] == A8[start[2]:start[2] + 129]).all() and alone_inv[st1[0]] == inv_a[start[2]]


def test_packer():
    L = F.harness()
    N, K = 32, 256
    idx = F.index_map(N, K)
    assert (np.sort(idx.ravel()) == np.arange(3 * N * K)).all()  # the map is a permutation of the image
    rs = np.random.RandomState(9)
    for exact in (True, False):
        W = rs.randint(-13, 14, (N, 3, K)).astype(np.float32) if exact else (rs.randn(N, 3, K) * np.exp(rs.randn(N, 1, 1))).astype(np.float32)
        if exact:
            W[:, 0, 0] = 14  # every row's maximum: scale 16, every integer times 16 is an e4m3 value
        else:
            W[5] = 0
        img, inv_w = np.zeros(3 * N * K, np.uint8), np.zeros(N, np.float32)
        assert L.tts_f8_test_pack(W, N, K, img, inv_w) == 0
        back = F.decode(img)[idx] * inv_w.astype(np.float64)[:, None, None]
        amax = np.abs(W).reshape(N, -1).max(1)
        sc = 1.0 / inv_w.astype(np.float64)
        assert ((amax == 0) & (sc == 1) | (224 <= amax * sc) & (amax * sc < 448)).all()
        if exact:
            assert (back == W).all()
        else:  # e4m3's half ulp: 2^-4 relative, 2^-10 absolute below the smallest normal, in units of 1 / scale
            assert (np.abs(back - W) <= np.maximum(np.abs(W) * 2.0 ** -4, 2.0 ** -10 * inv_w[:, None, None])).all()
