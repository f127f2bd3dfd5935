"""Option gemm_gn_fuse: a ResBlock's k = 1 in_layers GEMM and the GroupNorm in front of its k = 3 convolution run as ONE launch (gemm_f16.h:
gemm_f16_gn_panel_kernel) where the layout is admitted (gemm_gn_panel_takes: longest sequence <= 896 frames, a layout of the benchmark class). The mel must be
BYTE-EQUAL to option 0 (the two launches), and the profiler's launch counts must say which path ran: with the option on, an admitted layout launches one GroupNorm
(family diff_gn_fused) less per ResBlock evaluated without a precomputed in_layers output, and a layout that is not admitted launches exactly as many as with 0.

The issue's ragged batch (L = 7, 40, 123, 206) and its over-long batch (L = 207) are repeated three times / carried by six candidates so that their packed layouts
have the > 8 192 rows at which the engine's GEMMs take 128-row tiles: the rule admits no smaller layout, whatever its sequence lengths."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_STEPS = 3


@pytest.fixture()
def fuse_engine(engine):
    yield engine
    engine.prof_reset(False)
    engine.set_option("gemm_gn_fuse", DEFAULT)
    engine.set_option("attn_f32", 0)
    engine.set_option("share_uncond", 1)


DEFAULT = 1  # the option's default (common.h)


def _run(engine, lens, seed, expect_fused):
    rs = np.random.RandomState(seed)
    lats = [rs.randn(L, 1024).astype(np.float32) for L in lens]
    noise = [rs.randn(N_STEPS + 1, 100 * engine.frames(L)).astype(np.float32) for L in lens]
    mels, gn_launches = {}, {}
    for opt in (0, 1):
        engine.set_option("gemm_gn_fuse", opt)
        engine.prof_reset(True)
        mels[opt] = engine.diffusion(lats, n_steps=N_STEPS, noise=noise)
        gn_launches[opt] = engine.prof_get("diff_gn_fused")[1]
        engine.prof_reset(False)
    rows, seqs = engine.diffusion_last_layout()
    print("layout %d rows, %d sequences: diff_gn_fused launches %d with the pair, %d with gemm_gn_fuse" % (rows, seqs, gn_launches[0], gn_launches[1]))
    assert rows > 8192
    assert gn_launches[0] > 0
    if expect_fused:
        assert gn_launches[1] < gn_launches[0], gn_launches
    else:
        assert gn_launches[1] == gn_launches[0], gn_launches
    for c, (a, b) in enumerate(zip(mels[0], mels[1])):
        assert np.isfinite(b).all(), c
        diff = int((a.view(np.uint32) != b.view(np.uint32)).sum())
        print("candidate %d: %d of %d mel values differ between gemm_gn_fuse 0 and 1" % (c, diff, a.size))
        assert diff == 0, (c, diff)


def test_benchmark_layout(fuse_engine, mid_models):
    engine = fuse_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    assert engine.frames(200) == 870
    _run(engine, [200] * 16, 51, True)


def test_ragged_layout_with_a_full_panel(fuse_engine, mid_models):
    engine = fuse_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    assert engine.frames(206) == 896
    _run(engine, [7, 40, 123, 206] * 3, 52, True)


def test_one_sequence_too_long_falls_back_for_the_whole_layout(fuse_engine, mid_models):
    engine = fuse_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    assert engine.frames(207) == 901
    _run(engine, [207, 200, 200, 150, 206, 123], 53, False)


def test_benchmark_layout_reference_precision_attention(fuse_engine, mid_models):
    engine = fuse_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    engine.set_option("attn_f32", 1)  # the GroupNorm's SiLU in its exact mode (silu_dev mode 2)
    _run(engine, [200] * 16, 54, True)


def test_benchmark_layout_without_shared_unconditioned_branch(fuse_engine, mid_models):
    engine = fuse_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    engine.set_option("share_uncond", 0)
    _run(engine, [200] * 16, 55, True)
