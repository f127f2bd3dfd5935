"""Host side of the fused in_layers GEMM + GroupNorm (csrc/gemm_f16.h: gemm_gn_panel_takes, gemm_gn_panel_grid) through the harness library's entry points, and
the harness's own validation; no GPU.

The rule (res_block, diffusion.hip): the option is on, latency_mode statistics are not in play, no debug sums are requested, the fragment-major weight image exists,
the longest sequence fits a 896-row panel, the layout is one gemm_auto_th gives 128-row tiles (the benchmark class), N is a multiple of 64 and K of the K tile (64)."""
import ctypes as C

import numpy as np
import pytest

import gnp_cases as G

BENCH_ROWS = 28032  # 32 sequences of T = 870, packed


@pytest.fixture(scope="module")
def lib():
    return G.harness()


def takes(lib, option=1, stats=0, debug=0, wf=1, max_len=870, rows=BENCH_ROWS, N=1024, K=1024):
    return lib.tts_gnp_test_takes(option, stats, debug, wf, max_len, rows, N, K)


def test_benchmark_layout_is_admitted(lib):
    assert G.pack([870] * 32)[1] == BENCH_ROWS
    assert takes(lib) == 1


def test_panel_height(lib):
    assert takes(lib, max_len=896) == 1
    assert takes(lib, max_len=897) == 0
    assert takes(lib, max_len=1) == 1
    assert takes(lib, max_len=0) == 0
    assert G.PANEL_ROWS == 896 and lib.tts_gnp_test_lds() == 896 * 128  # one K tile of [896][64] halves = one f32 panel [896][32]


def test_what_keeps_the_pair(lib):
    assert takes(lib, option=0) == 0
    assert takes(lib, stats=1) == 0   # latency_mode
    assert takes(lib, wf=0) == 0      # no fragment-major image
    assert takes(lib, debug=1) == 0   # debug sums need H
    # small layouts: one utterance (1 792 rows: 64-row tiles) and the ragged 8-sequence batch (3 296 rows: 32-row tiles)
    assert takes(lib, rows=1792) == 0
    assert takes(lib, rows=G.pack([31, 174, 535, 896] * 2)[1]) == 0
    assert takes(lib, rows=8192) == 1 and takes(lib, rows=7936) == 0  # where gemm_auto_th first gives 128-row tiles at N = 1 024
    # shapes
    assert takes(lib, N=1056) == 0 and takes(lib, K=1056) == 0 and takes(lib, K=32) == 0 and takes(lib, K=0) == 0
    assert takes(lib, N=1152, K=960, rows=BENCH_ROWS) == 1 and takes(lib, K=64) == 1


def test_grid_is_whole_xcd_rounds(lib):
    assert lib.tts_gnp_test_grid(32, 1024) == 512  # 32 sequences x 16 panels: two rounds of 256 CUs
    assert lib.tts_gnp_test_grid(4, 64) == 8       # 4 items: padded to one workgroup per XCD
    assert lib.tts_gnp_test_grid(3, 192) == 16


def test_block_order_covers_every_item_once():
    """The kernel's map from workgroup to (sequence, panel): XCD b % 8 takes the items [n x / 8, n (x + 1) / 8), a padded workgroup takes none."""
    for ns, N in ((32, 1024), (4, 64), (3, 192), (1, 64), (7, 320)):
        n_items, grid = ns * (N // 64), 8 * ((ns * (N // 64) + 7) // 8)
        seen = np.zeros(n_items, int)
        for b in range(grid):
            x, idx = b & 7, b >> 3
            i0, i1 = n_items * x >> 3, n_items * (x + 1) >> 3
            if idx < i1 - i0:
                seen[i0 + idx] += 1
        assert (seen == 1).all(), (ns, N)
    # 32 x 16: an XCD holds whole sequences, as gn_reg_kernel's order does
    assert all(((512 * x >> 3) % 16) == 0 for x in range(9))


def test_harness_validation(lib):
    m = lib.tts_gnp_test_margin()

    def check(case):
        bufs = [np.zeros(case.rows * G.CH * 2 + 2 * m, np.uint8) for _ in range(2)]
        return lib.tts_gnp_test_validate(C.byref(case.struct(bufs[0], bufs[1])))

    assert check(G.Case([1, 17, 112, 113], 64, 128)) == 0
    assert check(G.Case([896], 128, 1024, ss="table")) == 0
    assert check(G.Case([897], 128, 1024)) != 0          # longer than a panel
    assert check(G.Case([17], 96, 128)) != 0             # N not a multiple of 64
    assert check(G.Case([17], 64, 160)) != 0             # K not a multiple of 64
    bad = G.Case([17, 40], 64, 128)
    bad.start = bad.start.copy(); bad.start[1] = bad.start[0] + 17  # no guard row between the sequences
    assert check(bad) != 0
    bad = G.Case([17, 40], 64, 128, ss="table")
    bad.seq_step = bad.seq_step.copy(); bad.seq_step[0] = 3  # a timestep outside the table
    assert check(bad) != 0
