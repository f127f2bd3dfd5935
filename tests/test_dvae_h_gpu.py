"""GPU: option dvae_precision (1 fp16, 2 fp16 hi + lo pairs: cls_down_h_kernel, hfg_conv_h_kernel, dvae_vq_h_kernel) through the C ABI on the mid-size model,
mels and float64 reference of tests/dvae_ref.py (the configuration of tests/test_dvae_gpu.py), clips of 1, 65 and 257 code rows. z: mode 2 under the f32 path's
gate (1e-3), mode 1 printed, not gated. Codes: the decided share under the KERNEL's operand bound (test_dvae_vq_h_gpu.bound at float64's z) is asserted >= 90 % on
the reference alone; the codes stand under dvae_ref.judge_end_to_end with that bound and the stage's MEASURED z distance in place of an operand bound."""
import numpy as np
import pytest

import dvae_ref as R
import test_dvae_vq_h_gpu as K

pytestmark = pytest.mark.gpu
FRAMES = (1, 257, 1025)  # 1, 65 and 257 code rows behind two stride-2 layers

@pytest.fixture(scope="module")
def engines(pkg):
    made = {}
    for loaded_at in (0, 2):
        made[loaded_at] = e = pkg.Engine(0)
        e.set_option("dvae_precision", loaded_at)
        e.load_dvae(R.model("mid")[0])
        e.set_option("dvae_precision", 0)
    yield made.get
    for e in made.values():
        e.close()

def codes_z(eng, mode, mels):
    eng.set_option("dvae_precision", mode)
    try:
        return eng.dvae_codes(mels, z=True)
    finally:
        eng.set_option("dvae_precision", 0)

@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("frames", FRAMES)
def test_engine_vs_float64(engines, frames, mode):
    ref, E = R.reference("mid", frames), R.model("mid")[1]["dvae.codebook.embed"]
    b = K.bound(ref["z"], E, mode)
    assert 1.0 - R.judge(ref["codes"], ref["s"], b)[1] >= K.MIN_DECIDED  # the reference alone
    codes, z = codes_z(engines(2), mode, [R.mel(frames)])
    assert z[0].shape == ref["z"].shape and np.isfinite(z[0]).all()
    err = float(np.abs(z[0] - ref["z"]).max())
    fails, out = R.judge_end_to_end(codes[0], z[0], ref["z"], ref["s"], b, E)
    print("dvae mid T = %d dvae_precision %d: z max abs distance from float64 %.2e (gate %.0e), %d of %d codes differ from float64's, %.4f of the rows under the margin"
          % (frames, mode, err, R.GATE, int((codes[0] != ref["codes"]).sum()), len(codes[0]), out))
    assert (mode == 1 or err <= R.GATE) and not fails, fails[:3]

def test_batch_is_each_clip_alone_mode_0_is_the_default_and_planes_are_needed(pkg, engines):
    eng, mels = engines(2), [R.mel(f, 1 + i) for i, f in enumerate(R.RAGGED)]
    cb, zb = codes_z(eng, 2, mels)
    for i, m in enumerate(mels):
        c1, z1 = codes_z(eng, 2, [m])
        assert np.array_equal(c1[0], cb[i]) and z1[0].tobytes() == zb[i].tobytes(), "mode 2: clip %d differs from itself alone" % i
    never = engines(0)
    for a, b in zip(eng.dvae_codes(mels, z=True), never.dvae_codes(mels, z=True)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "mode 0 on a model loaded at 2 is not the default"
    for mode in (1, 2):  # loaded at 0: no planes
        with pytest.raises(pkg.TtsError, match=r"no fp16 planes.*\(status -5\)"):
            codes_z(never, mode, mels)
