"""GPU: the BigVGAN vocoder's three kernels (csrc/bigvgan.h), one launch at a time through the test-only harness (testlib/bvg_harness.hip), against the float64
references of tests/bvg_cases.py under the bound derived there from the operands (nothing fitted; tests/test_bvg_harness_cpu.py shows a float32 restatement
inside it and every seeded defect outside). bvg_act_kernel: C = 32, 64, 96; candidates of 1, 2, 5, 6, 10, 11, 12 rows (below 11 rows both clamps reach into one
window), one length on either side of the 64-row run of a thread and of the 512-row tile of a workgroup, a ragged three-candidate batch with and without gaps,
arguments alpha u in the hundreds. bvg_mel_kernel: T = 1, 7, 8, 9, bit for bit. bvg_post_kernel: 32 and 64 channels, candidates of 1 and 3 frames.
Properties on every case: the rows of no candidate keep the sentinel, the canaries are intact, NaN in the input rows of no candidate changes no bit, a
candidate alone equals its rows in the batch bit for bit, two runs are bit-equal. The worst |err| / bound per kernel is printed (pytest -s)."""
import numpy as np
import pytest

import bvg_cases as V
from bvg_cases import ACT, MEL, POST

pytestmark = pytest.mark.gpu


def _run(c):
    rc, g = V.run(c)
    assert rc == 0, (c.name(), rc)
    assert g.canaries_intact(), c.name()
    return g.payload.copy()


@pytest.mark.parametrize("kind", [ACT, MEL, POST], ids=[V.KIND_NAMES[k] for k in (ACT, MEL, POST)])
def test_kernel_against_float64(kind):
    assert (V.harness().tts_bvg_test_run_rows(), V.harness().tts_bvg_test_block_rows()) == (V.RUN, V.BLOCK)
    worst = 0.0
    for c in V.cases(kind):
        ref = V.reference(c)
        out = _run(c)
        bad, r = V.judge(out, ref)
        worst = max(worst, r)
        assert bad == 0, (c.name(), bad, r)
        assert V.guards_ok(c, out, ref), c.name() + ": a row of no candidate was written"
        assert np.isfinite(out[ref["live"]]).all()
        assert np.array_equal(_run(c).view(np.uint32), out.view(np.uint32)), c.name() + ": two runs differ"
        p = V.poisoned(c)
        if p is not None:
            assert np.array_equal(_run(p).view(np.uint32), out.view(np.uint32)), c.name() + ": a row outside the candidates was read"
        if c.ns > 1:
            off = 0
            for s in range(c.ns):
                one = _run(V.alone(c, s))
                if kind == POST:
                    n = c.T[s] * 256
                    assert np.array_equal(one.view(np.uint32), out[off:off + n].view(np.uint32)), (c.name(), s)
                    off += n
                else:
                    assert np.array_equal(one[:c.T[s] * c.rate].view(np.uint32), out[c.rows(s)].view(np.uint32)), (c.name(), s)
    print("%-16s %d cases: worst |err| / bound %.3f" % (V.KIND_NAMES[kind], len(V.cases(kind)), worst))


def test_mel_pads_with_zero_channels():
    c = V.make(MEL, (7, 1, 9), seed=2)
    out = _run(c)
    assert (out[c.live(1)][:, 100:] == 0).all() and (np.abs(out[c.live(1)][:, :100]) > 0).any()


def test_constant_rows_pass_the_resampler():
    """each polyphase half of the filter sums to 1/2: a constant candidate leaves the activation as snake(constant) on every row, the ends included"""
    c = V.make(ACT, (3, 1), 32, 4, fam="const", seed=7)
    out = _run(c)
    for s in range(c.ns):
        v = c.a["in_"][c.rows(s)][0].astype(np.float64)
        want = v + np.sin(c.a["alpha"].astype(np.float64) * v) ** 2 * c.a["inv_beta"].astype(np.float64)
        assert np.abs(out[c.rows(s)] - want[None, :]).max() <= 2e-6 * max(1.0, np.abs(want).max())  # the taps are rounded to f32: their halves sum to 1/2 within 1e-7
