"""GPU: the classifier's kernels (csrc/classifier.h), one launch at a time through the test-only harness (tortoise.cpp_amd/testlib/cls_harness.hip), against the
float64 references of tests/cls_cases.py under the bounds derived there from the operands. On every case: a ragged batch (most with gaps between the clips);
the rows of no clip keep the sentinel and the canaries around the buffer are intact; NaN in the input rows of no clip changes no bit; a clip alone equals the clip
in the batch; two runs are bit-equal. The GroupNorm statistics are read back and held to their double-precision bound."""
import numpy as np
import pytest

import cls_cases as K

pytestmark = pytest.mark.gpu
CASES = K.all_cases()


def _check(c):
    g, stat = K.run(c, want_stat=True)
    out = g.payload
    assert g.canaries_intact(), "a write outside the output buffer"
    worst = 0.0
    for s, (ref, bound) in enumerate(K.reference(c)):
        ok, r = K.judge(K.clip_output(c, out, s), ref, bound)
        worst = max(worst, r)
        assert ok, "%s clip %d: %.3f of the bound" % (c.name(), s, r)
    if c.kind != K.HEAD:  # every row of no clip still holds the sentinel
        dead = ~c.live(out=c.kind == K.DOWN)
        assert (out[dead].view(np.uint8) == K.SENTINEL).all(), "a row outside the clips was written"
    g2, _ = K.run(c)
    assert np.array_equal(g2.raw, g.raw), "two runs differ"
    gp, _ = K.run(K.poisoned(c))
    assert np.array_equal(gp.raw, g.raw), "NaN in the rows of no clip changed the output"
    for s in range(c.ns):
        a = K.alone(c, s)
        ga, _ = K.run(a)
        assert np.array_equal(K.clip_output(a, ga.payload, 0), K.clip_output(c, out, s)), "clip %d alone differs from the clip in the batch" % s
    return worst, stat


@pytest.mark.parametrize("c", CASES, ids=[c.name() for c in CASES])
def test_kernel_against_float64(c):
    worst, stat = _check(c)
    print("%s: worst |device - float64| / bound = %.3f" % (c.name(), worst))
    if c.kind == K.GN:
        G = K.groups(c.C)
        for s in range(c.ns):
            x = c.a["in_"][c.clip(s)].astype(np.float64).reshape(c.n[s], G, -1)
            mean = x.mean(axis=(0, 2))
            var = (x ** 2).mean(axis=(0, 2)) - mean ** 2
            N = x.shape[0] * x.shape[2]
            e_mean = (N + 2) * K.D * np.abs(x).mean(axis=(0, 2)) + K.FMIN
            e_var = (N + 2) * K.D * (x ** 2).mean(axis=(0, 2)) + 2 * np.abs(mean) * e_mean + K.D * mean ** 2
            r = 1 / np.sqrt(var + K.EPS)
            assert (np.abs(stat[s, :, 0] - mean) <= e_mean).all()
            assert (np.abs(stat[s, :, 1] - r) <= r * (e_var / (2 * (var + K.EPS)) + 2 * K.D) + K.FMIN).all()
