"""GPU: the aligner's five new kernels (csrc/aligner.h: clip statistics, stem, row LayerNorm / GELU, grouped positional convolution, CTC head), one launch at a
time through the test-only harness (tortoise.cpp_amd/testlib/w2v_harness.hip), against the float64 references of tests/w2v_cases.py under the bounds derived
there from the operands. On every case: a ragged batch with gaps between the clips; the rows of no clip keep the sentinel and the canaries around every buffer
are intact; NaN in the input rows of no clip changes no bit; a clip alone equals the clip in the batch; two runs are bit-equal. The head's ids are the float64
argmax wherever the margin allows one answer, and on the exact family (ties included) logits and ids equal float64 and numpy's lowest-index argmax bit for bit."""
import numpy as np
import pytest

import w2v_cases as K

pytestmark = pytest.mark.gpu
CASES = K.all_cases()


def _ids(c, g2, s):
    return g2.payload[c.clip(s)]


@pytest.mark.parametrize("c", CASES, ids=[c.name() for c in CASES])
def test_kernel_against_float64(c):
    g, g2 = K.run(c)
    out = g.payload
    assert g.canaries_intact() and (g2 is None or g2.canaries_intact()), "a write outside the output buffer"
    worst = 0.0
    for s, (ref, bound) in enumerate(K.reference(c)):
        got = K.clip_output(c, out, s)
        ok, r = K.judge(got, ref, bound)
        worst = max(worst, r)
        assert ok, "%s clip %d: %.3f of the bound" % (c.name(), s, r)
        if c.kind == K.HEAD:
            ids = _ids(c, g2, s)
            assert K.ids_accept(c, ids, ref, bound), "%s clip %d: an id outside the rule" % (c.name(), s)
            assert np.array_equal(ids, np.argmax(got, axis=1)), "the id is not the lowest index of the device's own largest logit"
            if c.fam == "exact":
                assert np.array_equal(got.astype(np.float64), ref) and np.array_equal(ids, K.ref_ids(ref))
    print("%s: worst |device - float64| / bound = %.3f" % (c.name(), worst))
    if c.kind != K.STATS:  # every row of no clip still holds the sentinel
        dead = ~c.live(out=c.kind == K.STEM)
        assert (out[dead].view(np.uint8) == K.SENTINEL).all(), "a row outside the clips was written"
        if c.kind == K.HEAD:
            assert (g2.payload[dead].view(np.uint8) == K.SENTINEL).all(), "an id outside the clips was written"
    h, h2 = K.run(c)
    assert np.array_equal(h.raw, g.raw) and (g2 is None or np.array_equal(h2.raw, g2.raw)), "two runs differ"
    p, p2 = K.run(K.poisoned(c))
    assert np.array_equal(p.raw, g.raw) and (g2 is None or np.array_equal(p2.raw, g2.raw)), "NaN in the rows of no clip changed the output"
    for s in range(c.ns):
        a = K.alone(c, s)
        ga, ga2 = K.run(a)
        assert np.array_equal(K.clip_output(a, ga.payload, 0), K.clip_output(c, out, s)), "clip %d alone differs from the clip in the batch" % s
        if c.kind == K.HEAD:
            assert np.array_equal(_ids(a, ga2, 0), _ids(c, g2, s))


def test_head_without_logits_leaves_them_alone():
    c = K.make(K.HEAD, [9, 2], 128, 29, mode=0)
    g, g2 = K.run(c)
    assert (g.payload.view(np.uint8) == K.SENTINEL).all() and g.canaries_intact()
    w = K.make(K.HEAD, [9, 2], 128, 29, mode=1)
    w.a = c.a
    gw, gw2 = K.run(w)
    assert np.array_equal(gw2.raw, g2.raw)
