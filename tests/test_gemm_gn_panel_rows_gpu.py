"""gemm_f16_gn_panel_kernel with wave-private staging (csrc/gemm_f16.h): wave w moves the 14 DMA pieces of rows 112 w .. 112 w + 111 and reads only those rows, so no
barrier orders the activation tile (the one barrier of a K step belongs to the weight tile, which the eight waves stage for each other). The claim is the one tests/test_gemm_gn_panel_gpu.py checks — the bits of launch_gemm_f16 + gn_reg_kernel<512, 14> — and the assertions are
that file's: byte equality over the whole buffer, guard and padding rows zero, margins untouched, channels >= N still poison. The shapes are the ones where a wave
that owns its rows can go wrong and that file does not reach:

  lengths on every wave boundary   a sequence ending one row before, exactly at, and one row after the last row a wave owns (112 w - 1, 112 w, 112 w + 1 for
                                   w = 1 .. 8; 896 is the full panel), so that the waves behind the boundary stage nothing but clamped copies of the last row and
                                   the wave on it stages one, none, or 111 of them;
  K = 192                          three K tiles: exactly one steady-state step (read, re-issue the wave's own DMA into the rows just read, multiply) between the
                                   first and the last; K = 1 024 is the product's.

Each layout runs at N = 64, K = 192 and at N = 128, K = 1 024, with two of that file's variants."""
import numpy as np
import pytest

import gnp_cases as G

pytestmark = pytest.mark.gpu

LAYOUTS = [
    ("w1w2", [111, 112, 113, 223, 224, 225]),
    ("w3w4", [335, 336, 337, 447, 448, 449]),
    ("w5w6", [559, 560, 561, 671, 672, 673]),
    ("w7w8", [783, 784, 785, 895, 896]),
]
SIZES = [(64, 192), (128, 1024)]
VARIANTS = [
    ("gauss-bias-ss-silu0", dict(bias=True, ss="one", do_silu=1, lut=0)),
    ("outlier-nobias-table-silu2", dict(outlier=True, bias=False, ss="table", do_silu=1, lut=2)),
]


@pytest.mark.parametrize("vname,var", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("N,K", SIZES, ids=["N%d-K%d" % s for s in SIZES])
@pytest.mark.parametrize("lname,lens", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_identity_on_wave_boundaries(lname, lens, N, K, vname, var):
    assert max(lens) <= G.PANEL_ROWS
    case = G.Case(lens, N, K, seed=7 + len(vname) + N + K + lens[0], **var)
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
    assert (fused[~inside, :N] == 0).all(), "the panel kernel's guard / padding rows are zeros"
    diff = int((pair[:, :N] != fused[:, :N]).sum())
    print("%s N=%d K=%d %s: %d of %d fp16 values differ" % (lname, N, K, vname, diff, case.rows * N))
    assert diff == 0, (diff, np.argwhere(pair[:, :N] != fused[:, :N])[:8].tolist())
    assert (fused[:, N:] == poison).all(), "the panel kernel wrote a channel it does not own"
