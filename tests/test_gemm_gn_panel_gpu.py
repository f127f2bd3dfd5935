"""gemm_f16_gn_panel_kernel (csrc/gemm_f16.h, GroupNorm half in csrc/diffusion.hip) against the pair of launches it replaces in a ResBlock: launch_gemm_f16 with an
f32 output (the register-streamed gemm_f16_wreg_kernel) followed by gn_reg_kernel<512, 14>, on the same device operands. The pair is pinned to float64 by
tests/test_gemm_kernels_gpu.py and tests/test_gn_kernels_gpu.py; the panel kernel claims the SAME BITS — every accumulator adds the same products in the same K order,
one f32 bias add, then gn_reg_kernel's own arithmetic body on the values — so the check is byte equality of the fp16 output over the whole buffer: sequence rows,
guard rows and padding rows (zeros in both), with both buffers pre-filled with a poison byte and a margin on either side that must come back untouched.

Where N < 1024 the pair normalises all 1 024 channels (of an H whose other columns are zero) and the panel kernel owns channels < N only: those are compared, and the
channels >= N of the panel kernel's buffer must still hold the poison.

Shapes: T = 1, 17, 112, 113 in one layout (sequences shorter than one wave's 112 rows, exactly one wave's, and one row more), T = 870 (the benchmark's), T = 896 (the
full panel); N = 64 (one panel, an odd count of workgroups for the XCD order), 128 and 1 024 (every panel of the product's shape); K = 128 (the last-but-one and last
K steps alone: no steady-state step) and K = 1 024."""
import numpy as np
import pytest

import gnp_cases as G

pytestmark = pytest.mark.gpu

SHAPES = [
    ("short", [1, 17, 112, 113], 64, 128),
    ("short", [1, 17, 112, 113], 128, 1024),
    ("t870", [870], 128, 1024),
    ("t870", [870], 64, 128),
    ("t896", [896], 64, 1024),
    ("t896", [896], 128, 128),
    ("bench", [870, 896, 113], 1024, 1024),
]
VARIANTS = [
    ("gauss-bias-ss-silu0", dict(bias=True, ss="one", do_silu=1, lut=0)),
    ("gauss-nobias-noss-nosilu", dict(bias=False, ss="none", do_silu=0, lut=0)),
    ("gauss-bias-table-silu2", dict(bias=True, ss="table", do_silu=1, lut=2)),
    ("gauss-bias-noss-silu1", dict(bias=True, ss="none", do_silu=1, lut=1)),
    ("outlier-bias-ss-silu0", dict(outlier=True, bias=True, ss="one", do_silu=1, lut=0)),
    ("outlier-nobias-table-silu2", dict(outlier=True, bias=False, ss="table", do_silu=1, lut=2)),
]


@pytest.mark.parametrize("vname,var", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("sname,lens,N,K", SHAPES, ids=["%s-N%d-K%d" % (s[0], s[2], s[3]) for s in SHAPES])
def test_identity_with_the_pair(sname, lens, N, K, vname, var):
    case = G.Case(lens, N, K, seed=1 + len(vname) + N + K + len(lens), **var)
    rc, pair, fused, margins = G.run(case)
    assert rc == 0, rc
    for m in margins:
        assert (m == G.SENTINEL).all(), "a margin was written"
    poison = G.SENTINEL * 257
    # the pair's sequence rows hold finite values that are not all equal (the reference is alive)
    for s, L in enumerate(lens):
        rows = pair[case.start[s]:case.start[s] + L, :N].view(np.float16)
        assert np.isfinite(rows).all()
        assert len(np.unique(rows)) > 8
    inside = np.zeros(case.rows, bool)
    for s, L in enumerate(lens):
        inside[case.start[s]:case.start[s] + L] = True
    assert (pair[~inside, :N] == 0).all(), "the pair's guard / padding rows are zeros"
    diff = int((pair[:, :N] != fused[:, :N]).sum())
    print("%s N=%d K=%d %s: %d of %d fp16 values differ" % (sname, N, K, vname, diff, case.rows * N))
    assert diff == 0, (diff, np.argwhere(pair[:, :N] != fused[:, :N])[:8].tolist())
    assert (fused[:, N:] == poison).all(), "the panel kernel wrote a channel it does not own"
