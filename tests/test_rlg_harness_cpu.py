"""Without a GPU: the random-voice kernel harness (testlib/rlg_harness.hip) refuses every invalid case before any HIP call and exports the kernel's constants;
the float64 layer reference of tests/rlg_cases.py equals a torch.nn.functional restatement; a NumPy float32 restatement in rlg_layer_kernel's own order stays
inside the derived bounds at every dim and batch size of the GPU matrix and is bit-equal on the exact family; six seeded defects of one layer fall at least ten
bounds outside; the Philox restatement equals tests/voc_cases.py's under the vocoder's counter words and differs under this stage's."""
import ctypes as C

import numpy as np
import pytest

import rlg_cases as K
import voc_cases as VC


def test_constants_the_kernel_exports():
    L = K.harness()
    assert L.tts_rlg_test_tile() == 8 and L.tts_rlg_test_min_dim() == 256 and L.tts_rlg_test_max_dim() == 2048
    assert L.tts_rlg_test_tag() == 0x7717 and L.tts_rlg_test_tag() not in (K.DIFFUSION_TAG, K.VOCODER_TAG)
    assert K.batch_sizes() == (1, 2, 7, 8, 9, 17)
    assert min(K.DIMS) == L.tts_rlg_test_min_dim() and max(K.DIMS) == L.tts_rlg_test_max_dim()


def test_every_invalid_case_is_refused_before_any_device_call():
    cases, keep = K.invalid_cases()
    assert len(cases) >= 20
    L = K.harness()
    for name, c in cases:
        assert L.tts_rlg_test_validate(C.byref(c)) == K.HIP_INVALID_VALUE, name
        assert L.tts_rlg_test_run(C.byref(c)) == K.HIP_INVALID_VALUE, name  # run() validates first: no HIP call was made (this machine has no device)
    assert L.tts_rlg_test_validate(None) == K.HIP_INVALID_VALUE
    w, b, x = K.layer_operands(256, 2, 1)
    out = K.Guarded((2, 256))
    assert L.tts_rlg_test_validate(C.byref(K.layer_struct(w, b, x, 1, out))) == 0
    for dim in K.DIMS:
        assert L.tts_rlg_test_validate(C.byref(K.layer_struct(w, b, x, 0, out, dim=dim, n=17))) == 0, dim


@pytest.mark.parametrize("act", [0, 1])
def test_layer_reference_equals_torch_functional(act):
    import torch
    import torch.nn.functional as F
    w, b, x = K.layer_operands(256, 5, 3)
    ref, bound = K.layer_reference(w, b, x, act)
    t = F.linear(torch.as_tensor(x.astype(np.float64)), torch.as_tensor(w.astype(np.float64)), torch.as_tensor(b.astype(np.float64)))
    if act:
        t = F.leaky_relu(t, 0.2) * np.sqrt(2.0)
    assert np.abs(ref - t.numpy()).max() < 1e-13
    assert (bound > 0).all() and bound.max() < 1e-4


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dim", K.DIMS)
def test_float32_in_the_kernels_order_stays_inside_the_bound(dim, act):
    worst = 0.0
    for n in (K.batch_sizes() if dim == 256 else (2,)):
        w, b, x = K.layer_operands(dim, n, 10 * dim + n)
        ref, bound = K.layer_reference(w, b, x, act)
        got = K.layer_kernel_order32(w, b, x, act)
        ratio = float((np.abs(got - ref) / bound).max())
        worst = max(worst, ratio)
    print("dim %d act %d: worst error / bound %.3f" % (dim, act, worst))
    assert worst <= 1.0
    assert worst > 1e-3  # the bound is of the error's order, not a blanket


@pytest.mark.parametrize("dim", K.DIMS)
def test_exact_family_is_bit_equal_in_the_kernels_order(dim):
    w, b, x = K.layer_operands(dim, 3, 7, "exact")
    ref = (x.astype(np.int64) @ w.astype(np.int64).T + b.astype(np.int64)).astype(np.float32)
    assert np.abs(ref).max() < 2 ** 24
    got = K.layer_kernel_order32(w, b, x, 0)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
    ref64, _ = K.layer_reference(w, b, x, 0)
    assert (ref64 == ref).all()


def test_seeded_defects_of_one_layer_fall_ten_bounds_outside():
    w, b, x = K.layer_operands(256, 3, 11)
    ref, bound = K.layer_reference(w, b, x, 1)
    v = x.astype(np.float64) @ w.astype(np.float64).T + b
    g = np.sqrt(2.0)
    defects = {"slope 0.1": np.where(v > 0, v, 0.1 * v) * g, "no gain": np.where(v > 0, v, 0.2 * v), "no bias": np.where(v - b > 0, v - b, 0.2 * (v - b)) * g,
               "transposed weight": (lambda t: np.where(t > 0, t, 0.2 * t) * g)(x.astype(np.float64) @ w.astype(np.float64) + b),
               "no activation": v, "neighbour's bias": (lambda t: np.where(t > 0, t, 0.2 * t) * g)(v - b + np.roll(b, 1))}
    for name, y in defects.items():
        assert (np.abs(y - ref) / bound).max() >= 10, name
    ref0, bound0 = K.layer_reference(w, b, x, 0)
    assert (np.abs(ref - ref0) / bound0).max() >= 10  # an activation where none belongs


def test_philox_restatement():
    x, bound = K.noise_reference(512, 0x123456789ABCDEF, 3, tag=K.VOCODER_TAG, c1=0x766f63)
    vx, vb = VC.philox_reference(512, 0x123456789ABCDEF, 3)
    assert (x == vx).all() and (bound == vb).all()  # the same restatement under the vocoder's counter words
    a, _ = K.noise_reference(1024, 7, 0)
    assert np.isfinite(a).all() and abs(a.mean()) < 0.15 and 0.85 < a.std() < 1.15
    for other in (K.noise_reference(1024, 7, 1)[0], K.noise_reference(1024, 8, 0)[0], K.noise_reference(1024, 7, 0, tag=K.DIFFUSION_TAG)[0],
                  K.noise_reference(1024, 7, 0, tag=K.DIFFUSION_TAG, c1=0xFFFFFFFF)[0], VC.philox_reference(1024, 7, 0)[0]):
        assert (a != other).mean() > 0.99
