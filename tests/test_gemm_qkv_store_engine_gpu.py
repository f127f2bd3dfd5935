"""Option gemm_wreg, bit 3: the register-streamed QKV projection of the diffusion stage parks its fp16 tile in LDS and stores whole cache lines
(gemm_f16.h: gemm_epilogue_wreg_qkv_lds). The option's value 7 is every register-streamed class with the QKV tile stored straight from the registers, 15 (what 1
selects, the default) adds the stores through LDS: the same fp16 values at the same addresses, so the mel must be BYTE-EQUAL.

The profiler's family diff_gemm_qkv counts the QKV projections: both runs must launch the same, non-zero number (the option changes no launch), and the layout
must be one whose GEMMs take the 128-row tiles the register-streamed kernel serves (> 8 192 packed rows), or neither value would reach the kernel; WHICH epilogue
a set of arguments selects is the plan string of tests/test_gemm_qkv_store_gpu.py. Candidates of two different lengths, four steps; the first test repeats the
pair until the layout is that large, the second is the bare pair, whose QKV projection stays on the LDS-staged kernel under either value."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_STEPS = 4


@pytest.fixture()
def wreg_engine(engine):
    yield engine
    engine.prof_reset(False)
    engine.set_option("gemm_wreg", 1)


def _ab(engine, lens, seed):
    rs = np.random.RandomState(seed)
    lats = [rs.randn(L, 1024).astype(np.float32) for L in lens]
    noise = [rs.randn(N_STEPS + 1, 100 * engine.frames(L)).astype(np.float32) for L in lens]
    mels, launches = {}, {}
    for opt in (7, 15, 1):
        engine.set_option("gemm_wreg", opt)
        engine.prof_reset(True)
        mels[opt] = engine.diffusion(lats, n_steps=N_STEPS, noise=noise)
        launches[opt] = engine.prof_get("diff_gemm_qkv")[1]
        engine.prof_reset(False)
    rows, seqs = engine.diffusion_last_layout()
    print("layout %d rows, %d sequences: diff_gemm_qkv launches %s" % (rows, seqs, launches))
    assert launches[7] > 0 and launches[15] == launches[7] and launches[1] == launches[7], launches
    for opt in (15, 1):
        for c, (a, b) in enumerate(zip(mels[7], mels[opt])):
            assert np.isfinite(b).all(), (opt, c)
            diff = int((a.view(np.uint32) != b.view(np.uint32)).sum())
            print("candidate %d: %d of %d mel values differ between gemm_wreg 7 and %d" % (c, diff, a.size, opt))
            assert diff == 0, (opt, c, diff)
    return rows


def test_two_lengths_on_128_row_tiles(wreg_engine, mid_models):
    engine = wreg_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    assert engine.frames(200) == 870 and engine.frames(123) != 870
    assert _ab(engine, [200, 123] * 6, 61) > 8192


def test_two_candidates(wreg_engine, mid_models):
    engine = wreg_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    _ab(engine, [200, 123], 62)
