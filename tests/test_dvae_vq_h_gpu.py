"""GPU: dvae_vq_h_kernel<SPLIT> (csrc/dvae_vq_h.h, option dvae_precision 1 and 2), one launch at a time through libtts_dvae_test.so (tts_dvae_test_run_vq_h: the
loader's packer, then dvae_launch_vq_h) against float64 distances and argmin in NumPy on the float32 operands. bound() is the operand-derived bound of
DESIGN.md "What pins the DVAE on the fp16 MFMA" on one distance, nothing fitted: (2 r + (4 m D + 2) u) M_j + 2 u |E_j|^2 + 2^-24 sum_k (|E_kj| + |z_k| / s_j),
h = 2^-11, u = 2^-24, M_j = sum_k |z_k E_kj|, s_j the packer's power of two, r = 3 h^2, m = 3 (mode 2) | r = 2 h + h^2, m = 1 (mode 1). The code rule is
dvae_ref.judge's with this bound; at least 90 % of a Gaussian case's rows are decided, asserted on the reference alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import dvae_ref as R

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
H = 2.0 ** -11
ROWS, DIMS, TOKENS = (1, 63, 64, 65, 130), (64, 96), 2 * R.VQ_SLAB  # dim is a multiple of 32, hence of the K step of 16: 96 = six K steps, an odd count of 32s
MIN_DECIDED = 0.90

def scale(E):
    """the packer's power of two of every code: its largest |E_kj| s_j lies in [2^12, 2^13) (an all-zero code: 1)"""
    m = np.abs(E).max(0).astype(f64)
    return np.where(m > 0, 2.0 ** (12 - np.floor(np.log2(np.where(m > 0, m, 1.0)))), 1.0)

def bound(z, E, mode):
    z, E = np.abs(z.astype(f64)), np.abs(E.astype(f64))
    M, e2, D, m = z @ E, (E * E).sum(0)[None, :], E.shape[0], 3 if mode == 2 else 1
    r = 3 * H * H if mode == 2 else 2 * H + H * H
    return (2 * r + (4 * m * D + 2) * R.U) * M + 2 * R.U * e2 + 2.0 ** -24 * (E.sum(0)[None, :] + z.sum(1)[:, None] / scale(E)[None, :])

@functools.lru_cache(maxsize=None)
def inputs(family, rows, dim, tokens=TOKENS):
    S, rng = R.VQ_SLAB, np.random.default_rng(7000 + 13 * rows + dim)
    pl = np.full(rows, -1, np.int32)  # -1, or the code a planted winner or tie must return
    if family == "exact":  # small integers times powers of two: every hi is exact, every lo zero, every sum exact; many exact ties
        z, E = rng.integers(-4, 5, (rows, dim)).astype(f32) * f32(0.5), rng.integers(-4, 5, (dim, tokens)).astype(f32) * f32(0.25)
    else:
        z, E = rng.standard_normal((rows, dim)).astype(f32), rng.standard_normal((dim, tokens)).astype(f32)
    if family == "planted":
        edge = sorted({0, min(R.VQ_TILE - 1, rows - 1), rows - 1} | ({R.VQ_TILE} if rows > R.VQ_TILE else set()))  # the first and the last row of a tile
        ties = {3: (37, 45), 5: (70, 101), 6: (130, S + 9)} if rows >= 8 else {}  # one 32-code tile; two waves; two slabs
        for r, (lo, hi) in ties.items():
            E[:, lo] = E[:, hi] = z[r]
            pl[r] = lo
        for i, r in enumerate(edge):  # the winner in the first and the last column of either slab
            pl[r] = (0, S - 1, S, 2 * S - 1)[(i + rows) % 4]
            E[:, pl[r]] = z[r]
    for a in (z, E, pl):
        a.setflags(write=False)
    return z, E, pl

def run(z, E, mode):
    L, c = R.harness(), R.Case(R.VQ, z, E)
    L.tts_dvae_test_run_vq_h.argtypes, L.tts_dvae_test_run_vq_h.restype = [C.POINTER(R.CaseStruct), C.c_int], C.c_int
    g, g2 = R.Guarded((c.rows,), np.int32), R.Guarded((c.rows,), f32)
    assert L.tts_dvae_test_run_vq_h(C.byref(c.struct(g.raw, g2.raw)), mode) == 0 and g.canaries_intact() and g2.canaries_intact()
    return g.payload.copy(), g2.payload.copy()

def check(family, z, E, pl, mode, codes, best):
    s, b = R.vq64(z, E)[0], bound(z, E, mode)
    assert codes.min() >= 0 and codes.max() < E.shape[1] and np.isfinite(best).all()
    i = np.arange(len(codes))
    ratio = float((np.abs(best.astype(f64) - s[i, codes]) / b[i, codes]).max())
    fails, und = R.judge(codes, s, b, pl)
    print("dvae_vq_h %s mode %d rows %d dim %d: worst distance error / bound %.4f, undecided %.4f" % (family, mode, len(codes), E.shape[0], ratio, und))
    assert ratio <= 1.0 and not fails and (family != "gauss" or 1.0 - und >= MIN_DECIDED), fails[:3]
    if family == "exact":  # bit for bit float64's distances and codes
        assert np.array_equal(best, s.min(1).astype(f32)) and np.array_equal(codes, s.argmin(1))

@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("family", ["gauss", "exact", "planted"])
def test_vs_float64(family, rows, dim, mode):
    z, E, pl = inputs(family, rows, dim)
    assert R.harness().tts_dvae_test_vq_h_spw(rows, TOKENS) == 1
    check(family, z, E, pl, mode, *run(z, E, mode))

@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
def test_several_slabs_per_workgroup(mode):
    """2048 rows x 8192 codes: the launcher gives a workgroup two slabs (the only other path of the kernel); the last code planted as a winner"""
    z, E, _ = inputs("gauss", 2048, 64, 8192)
    E = E.copy()
    E[:, 8191] = z[2047]
    assert R.harness().tts_dvae_test_vq_h_spw(2048, 8192) == 2
    codes, best = run(z, E, mode)
    check("gauss", z, E, None, mode, codes, best)  # the rule holds row 2047 to float64's code, the planted 8191

@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
def test_rows_alone_in_a_batch_and_twice(mode):
    z, E, _ = inputs("gauss", 130, 64)
    a, b = run(z, E, mode), run(z, E, mode)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), "two runs differ"
    c = run(z[37:102], E, mode)  # 65 rows at another place of another tile
    assert np.array_equal(c[0], a[0][37:102]) and c[1].tobytes() == a[1][37:102].tobytes(), "rows alone differ from the rows in the batch"
