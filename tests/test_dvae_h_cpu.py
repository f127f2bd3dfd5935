"""CPU: option dvae_precision on a host-only context, the CLI's --dvae-precision usage error, and the bound of tests/test_dvae_vq_h_gpu.py on that test's own
inputs: a float32 NumPy restatement of dvae_vq_h_kernel's arithmetic (the packer's scale, fp16 hi / lo planes, per K step of 16 the products eh zl, el zh, eh zh
into the f32 accumulator) stays inside it on every distance; one seeded defect, the eh zl product dropped, does not."""
import os
import subprocess

import numpy as np
import pytest

import dvae_ref as R
import test_dvae_vq_h_gpu as K

f32, f64, f16 = np.float32, np.float64, np.float16

def test_option_values(pkg):
    e = pkg.Engine(-1)
    for v in (0, 1, 2, 0):
        e.set_option("dvae_precision", v)
    for bad in (3, -1, 0.5, float("nan")):
        assert e.L.tts_set_option(e.h, b"dvae_precision", float(bad)) == -1 and b"dvae_precision" in e.L.tts_last_error(e.h)
        with pytest.raises(pkg.TtsError, match="dvae_precision"):
            e.set_option("dvae_precision", bad)
    e.close()

def test_cli_refuses_another_name_before_any_model_is_loaded():
    exe = os.path.join(R.ROOT, "tortoise.cpp_amd", "tortoise")
    r = subprocess.run([exe, "--models", "/nonexistent", "--dvae-precision", "bogus"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--dvae-precision bogus: f32, f16 or split" in r.stderr

def twin(z, E, mode, drop=False):
    """every distance as the kernel computes it, in float32 (an MFMA: its 16 products summed, then added to the accumulator and rounded)"""
    s = K.scale(E).astype(f32)
    pair = lambda x: (x.astype(f16), (x - x.astype(f16).astype(f32)).astype(f16))  # noqa: E731
    (zh, zl), (eh, el) = pair(np.clip(z, -65504, 65504)), pair(E * s[None, :])
    acc = np.zeros((z.shape[0], E.shape[1]), f32)
    for k in range(0, E.shape[0], 16):
        for a, b in ([(zl, eh)] * (not drop) + [(zh, el), (zh, eh)] if mode == 2 else [(zh, eh)]):
            acc = (acc.astype(f64) + a[:, k:k + 16].astype(f64) @ b[k:k + 16].astype(f64)).astype(f32)
    return (R.code_norms(E).astype(f64)[None, :] - 2.0 * acc.astype(f64) / s[None, :]).astype(f32)

@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("dim", K.DIMS)
@pytest.mark.parametrize("rows", K.ROWS)
def test_restatement_inside_the_bound_and_the_defect_outside(rows, dim, mode):
    z, E, _ = K.inputs("gauss", rows, dim)
    s, b = R.vq64(z, E)[0], K.bound(z, E, mode)
    d = twin(z, E, mode)
    fails, und = R.judge(d.argmin(1), s, b)
    assert (np.abs(d - s) <= b).all() and not fails and 1.0 - und >= K.MIN_DECIDED
    if mode == 2:
        assert (np.abs(twin(z, E, 2, drop=True) - s) > b).any()
