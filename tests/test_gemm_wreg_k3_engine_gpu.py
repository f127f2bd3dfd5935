"""Option gemm_wreg, one class at a time: value 4 streams only the weights of the k = 3 out_layers convolutions of the diffusion stage through registers
(gemm_f16.h: gemm_f16_conv3_wreg_kernel); the mel must be BYTE-EQUAL to option 0 (the LDS-staged kernels) and to 1 (every class that has such a kernel).
tests/test_gemm_wreg_gpu.py compares 0 with 1 at full depth, on the ragged layout and with attn_f32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def wreg_engine(engine):
    yield engine
    engine.set_option("gemm_wreg", 1)


def test_k3_class_alone_benchmark_layout(wreg_engine, mid_models):
    engine = wreg_engine
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    rs = np.random.RandomState(41)
    lens, n_steps = [200] * 16, 3
    assert engine.frames(200) == 870
    lats = [rs.randn(L, 1024).astype(np.float32) for L in lens]
    noise = [rs.randn(n_steps + 1, 100 * engine.frames(L)).astype(np.float32) for L in lens]
    mels = {}
    for opt in (0, 4, 1):
        engine.set_option("gemm_wreg", opt)
        mels[opt] = engine.diffusion(lats, n_steps=n_steps, noise=noise)
    for opt in (4, 1):
        for c, (a, b) in enumerate(zip(mels[0], mels[opt])):
            assert np.isfinite(b).all(), (opt, c)
            diff = int((a.view(np.uint32) != b.view(np.uint32)).sum())
            print("candidate %d: %d of %d mel values differ between gemm_wreg 0 and %d" % (c, diff, a.size, opt))
            assert diff == 0, (opt, c, diff)
