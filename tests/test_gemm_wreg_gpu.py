"""Option gemm_wreg: the k = 1 in_layers convolution and the QKV projection of the diffusion stage stream their weight operand from a fragment-major image
straight into registers (gemm_f16.h: gemm_f16_wreg_kernel) instead of staging it in LDS. Every accumulator adds the same products in the same K order through the
same MFMA instruction and operand order as the LDS-staged kernels, so the mel must be BYTE-EQUAL with the option 0 (the LDS-staged kernels) and 1 (every class that
has a register-streamed kernel) — in the default arithmetic and with attn_f32 = 1 (the split-precision QKV epilogue)."""
import numpy as np
import pytest

from conftest import ATTN_MODES

pytestmark = pytest.mark.gpu


@pytest.fixture()
def wreg_engine(engine):
    yield engine
    engine.set_option("gemm_wreg", 1)
    engine.set_option("attn_f32", 0)


def _problem(engine, lens, n_steps, seed):
    rs = np.random.RandomState(seed)
    lats = [rs.randn(L, 1024).astype(np.float32) for L in lens]
    noise = [rs.randn(n_steps + 1, 100 * engine.frames(L)).astype(np.float32) for L in lens]
    return lats, noise


def _ab(engine, lats, noise, n_steps, what):
    for mode, name in ATTN_MODES:
        engine.set_option("attn_f32", mode)
        engine.set_option("gemm_wreg", 0)
        base = engine.diffusion(lats, n_steps=n_steps, noise=noise)
        engine.set_option("gemm_wreg", 1)
        got = engine.diffusion(lats, n_steps=n_steps, noise=noise)
        for c, (a, b) in enumerate(zip(base, got)):
            assert np.isfinite(b).all(), (what, name, c)
            diff = int((a.view(np.uint32) != b.view(np.uint32)).sum())
            print("%s [%s] candidate %d: %d of %d mel values differ between gemm_wreg 0 and 1" % (what, name, c, diff, a.size))
            assert diff == 0, (what, name, c, diff)


def test_forward_benchmark_layout_full_depth(wreg_engine, full_models):
    """The benchmark's layout (16 candidates of 200 latents, both guidance branches: 32 sequences of T = 870) through the full-depth network: two sampling steps, the shortest schedule the
    engine takes."""
    engine = wreg_engine
    engine.load(diffusion=full_models + "/ggml-diffusion-model.bin")
    lats, noise = _problem(engine, [200] * 16, 2, 31)
    assert engine.frames(200) == 870
    _ab(engine, lats, noise, 2, "full depth, 32 x 870")


def test_short_sampling_loop(wreg_engine, mid_models):
    """Six sampling steps at the benchmark's layout: differences would compound from step to step."""
    engine = wreg_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    lats, noise = _problem(engine, [200] * 16, 6, 32)
    _ab(engine, lats, noise, 6, "6 steps, 32 x 870")


def test_ragged_layout(wreg_engine, mid_models):
    """Sequence lengths that are no multiples of 128 (or of anything): 128-row tiles straddle sequences and their guard rows, and the last tile of an XCD's
    row range is short. Large enough (> 8 192 packed rows) that both classes take the 128-row tiles the register-streamed kernel serves."""
    engine = wreg_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    lens = [37, 113, 200, 61, 150, 89, 175, 23, 131, 199, 77, 166]
    assert 2 * sum(engine.frames(L) for L in lens) > 8192
    lats, noise = _problem(engine, lens, 3, 33)
    _ab(engine, lats, noise, 3, "ragged, 24 sequences")
