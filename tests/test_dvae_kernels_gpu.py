"""GPU: the DVAE encoder's new kernels (csrc/dvae.h: dvae_stem_kernel, cls_down_kernel + dvae_relu_kernel as the second strided layer, dvae_vq_kernel +
dvae_vq_reduce_kernel) one launch at a time through the test-only harness, against float64 under the derived bounds and the code rule of tests/dvae_ref.py.
Every output buffer carries canaries in front and behind and every input buffer NaNs (a convolution that read outside its clip's frames or rows, or a quantiser that
read outside z, would put a NaN into an output no bound admits; a NaN codebook column can never win, so the quantiser's guard there is the float64 argmin itself); the harness validates a case completely before any HIP call (tests/test_dvae_cpu.py)."""
import numpy as np
import pytest

import dvae_ref as R

pytestmark = pytest.mark.gpu


def _conv(c):
    rc, g, _ = c.run()
    assert rc == 0, "HIP status %d" % rc
    assert g.canaries_intact(), "a write outside the output buffer"
    y = g.payload
    assert np.isfinite(y).all(), "a row of the output was not written"
    worst = 0.0
    for got, (want, bound) in zip(c.clips_out(y), c.reference()):
        assert got.shape == want.shape
        worst = max(worst, float((np.abs(got.astype(np.float64) - want) / bound).max()))
        assert (got >= 0).all()  # the ReLU is in the stored tensor
    print("%s: at most %.3f of the bound" % (c.name(), worst))
    assert worst <= 1.0
    return y.copy()


@pytest.mark.parametrize("i", range(len(R.stem_cases())), ids=[c.name() for c in R.stem_cases()])
def test_stem_against_float64(i):
    _conv(R.stem_cases()[i])


@pytest.mark.parametrize("i", range(len(R.down_cases())), ids=[c.name() for c in R.down_cases()])
def test_strided_layer_with_relu_against_float64(i):
    _conv(R.down_cases()[i])


def test_a_clip_alone_gives_the_bits_of_the_clip_in_a_batch():
    for cases in (R.stem_cases(), R.down_cases()):
        rag = [c for c in cases if len(c.n) == 2][0]
        both = rag.clips_out(_conv(rag))
        for s in range(2):
            alone = R.Case(rag.kind, [rag.x[s]], rag.wt, rag.b, rag.stride, label="alone%d" % s)
            assert np.array_equal(_conv(alone), both[s])


def _vq(c, pl):
    rc, g, g2 = c.run()
    assert rc == 0, "HIP status %d" % rc
    assert g.canaries_intact() and g2.canaries_intact(), "a write outside the output buffers"
    codes, best = g.payload.copy(), g2.payload.copy()
    s, bound = R.vq64(c.x[0], c.w)
    fails, und = R.judge(codes, s, bound, pl)
    print("%s: %d rows, %d with an exact tie, undecided share %.4f" % (c.name(), c.rows, int((pl >= 0).sum()), und))
    assert not fails, fails[:3]
    assert und <= R.MAX_UNDECIDED
    # the minimum itself: the chosen code's distance under its bound
    assert (np.abs(best.astype(np.float64) - s[np.arange(c.rows), codes]) <= bound[np.arange(c.rows), codes]).all()
    return codes, best


@pytest.mark.parametrize("i", range(len(R.vq_cases())), ids=[c.name() for c, _ in R.vq_cases()])
def test_vq_code_rule_planted_winners_and_exact_ties(i):
    c, pl = R.vq_cases()[i]
    codes, _ = _vq(c, pl)
    assert codes[0] == 0  # planted: the first column
    if c.rows > 1:
        assert codes[-1] == c.cout - 1  # the last column
    if c.rows > 2 and c.cout > R.VQ_SLAB:
        assert codes[c.rows // 2] == R.VQ_SLAB - 1  # the last column of the first slab
    if c.rows >= 8:
        assert list(codes[[3, 5]]) == [37, 70] and (c.cout <= R.VQ_SLAB or codes[6] == 130)  # the lower index of every duplicated pair


def test_vq_full_size_two_runs_and_every_position_of_a_batch():
    c, pl = R.vq_full_case()
    codes, best = _vq(c, pl)
    assert codes[7] == 300 and codes[64] == 8191
    again = c.run()
    assert np.array_equal(again[1].payload, codes) and np.array_equal(again[2].payload, best), "two runs differ"
    # a row alone against the same row at every position of a batch: the small shape, one row tile + 1
    sc, _ = [x for x in R.vq_cases() if x[0].label == "N%d-R%d" % (R.VQ_SLAB + 64, R.VQ_TILE + 1)][0]
    row = sc.x[0][11]
    rc, g, g2 = R.Case(R.VQ, row[None, :], sc.w, label="alone").run()
    assert rc == 0
    z = np.ascontiguousarray(np.repeat(row[None, :], R.VQ_TILE + 1, 0))
    z[1::2] = sc.x[0][1::2]  # other rows between the copies
    rc, b, b2 = R.Case(R.VQ, z, sc.w, label="batch").run()
    assert rc == 0
    assert (b.payload[0::2] == g.payload[0]).all() and (b2.payload[0::2].view(np.uint32) == g2.payload.view(np.uint32)[0]).all(), "a row's code depends on its position"
