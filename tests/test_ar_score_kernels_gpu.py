"""GPU: the AR scoring kernel pair (csrc/ar_score.h: ar_score_kernel + ar_score_reduce_kernel) one launch at a time through the test-only harness
(tests/ar_score_cases.py), against float64 under the operand-derived bounds of tests/ar_score_ref.py: lse, the target's and the stop token's logit and
log-prob, and the argmax rule (planted exact ties resolve to the lower index at every level; elsewhere the float64 argmax on rows whose margin exceeds twice
the row's bound). Every output buffer carries canaries and starts as a sentinel, every input buffer's margins hold NaNs, the pad columns of W and b hold 1e30.
The harness validates a case completely before any HIP call (tests/test_ar_score_cpu.py).

Measured on an MI355X (profiles/ar_score.txt): the worst ratio to the bound over all cases is 0.071 (lse, reduced shape), 0.056 (logp); 0.002 on the full head."""
import numpy as np
import pytest

import ar_score_cases as A
import ar_score_ref as R

pytestmark = pytest.mark.gpu

_memo = {}


def _run(c):
    """the kernel's arrays of one case (one launch per case and session), canaries and sentinels checked"""
    if c.label not in _memo:
        rc, g = c.run()
        assert rc == 0, "HIP status %d" % rc
        for k, v in g.items():
            assert v.canaries_intact(), "a write outside the %s buffer" % k
            assert not (v.payload.view(np.uint32) == 0xCBCBCBCB).any(), "a row of %s was not written" % k
        _memo[c.label] = {k: v.payload.copy() for k, v in g.items()}
    return _memo[c.label]


def _check(c, ref):
    got = _run(c)
    for k in ("lse", "logp", "stop_logp", "tgt_logit", "stop_logit"):
        assert np.isfinite(got[k]).all(), k
    ratios = ref.ratios(got)
    print("%s: worst ratio to the bound %s" % (c.label, ", ".join("%s %.3f" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0, ratios
    fails = ref.argmax_failures(got["greedy"], c.planted)
    assert not fails, fails[:3]
    return got


@pytest.mark.parametrize("rows", A.FULL_ROWS)
def test_full_head_against_float64(rows):
    full = A.full_case()
    _check(full.first(rows), full.reference().rows(rows))


def test_reduced_shape_two_slabs_and_a_wave_without_a_tile():
    c = A.small_case()
    _check(c, c.reference())


def test_tail_slab_tie_resolves_to_the_lower_index():
    c = A.tail_tie_case()
    got = _check(c, c.reference())
    assert got["greedy"][1] == 8192


@pytest.mark.parametrize("shape", (A.SMALL, A.FULL), ids=("reduced", "full"))
def test_plus_80_minus_80_row_and_all_equal_row(shape):
    c = A.extreme_case(shape)
    got = _check(c, c.reference())
    N = shape["N"]
    assert list(got["greedy"]) == [5, 0, N - 1]
    assert got["lse"][0] == np.float32(80.0) and got["lse"][2] == np.float32(80.0)  # exp(-160) vanishes against 1: no overflow, no NaN
    assert abs(float(got["lse"][1]) - (-80.0 + np.log(N))) <= c.reference().b_lse[1]
    assert got["tgt_logit"][0] == np.float32(80.0) and got["stop_logit"][2] == np.float32(80.0) and got["stop_logit"][0] == np.float32(-80.0)


def test_pad_columns_have_no_effect():
    """the same rows with zeros in the pad columns instead of 1e30: every bit equal"""
    c = A.full_case().first(65)
    W, b = c.W.copy(), c.b.copy()
    W[:, c.N:] = 0.0
    b[c.N:] = 0.0
    z = A.Case("full-R65-zero-pad", c.hn, W, b, c.tgt, c.N, c.planted)
    got, want = _run(z), _run(c)
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


def test_a_row_alone_gives_the_bits_of_the_row_among_130_and_two_runs_agree():
    full = A.full_case()
    all_, alone = _run(full.first(130)), _run(full.first(1))
    for k in all_:
        assert all_[k].view(np.uint32)[0] == alone[k].view(np.uint32)[0], k
    # a row of the ragged last tile, alone and at its place
    one = A.Case("full-row129", full.hn[129:130], full.W, full.b, full.tgt[129:130], full.N)
    got = _run(one)
    for k in all_:
        assert all_[k].view(np.uint32)[129] == got[k].view(np.uint32)[0], k
    rc, g = full.first(130).run()
    assert rc == 0
    for k in all_:
        assert np.array_equal(g[k].payload.view(np.uint32), all_[k].view(np.uint32)), "two runs differ in %s" % k
    # and every prefix of the batch holds the same bits as the whole
    for n in (63, 64, 65):
        part = _run(full.first(n))
        for k in all_:
            assert np.array_equal(part[k].view(np.uint32), all_[k].view(np.uint32)[:n]), (n, k)
