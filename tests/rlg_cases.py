"""Shared by tests/test_rlg_kernels_gpu.py, tests/test_rlg_harness_cpu.py, tests/test_random_voice_cpu.py and tests/test_random_voice_gpu.py: the ctypes view of
the test-only harness library (tortoise.cpp_amd/testlib/rlg_harness.hip -> libtts_rlg_test.so), float64 references of the two kernels of csrc/random_voice.h,
the case matrix, the acceptance bounds, a float32 restatement in the kernel's own order, and the layer-by-layer judgement of a whole RandomLatentConverter.

BOUNDS, first order and term by term from rlg_layer_kernel's operation order, nothing fitted; u = 2^-24, D = the channel count, operands as the kernel reads them
(w, bias, x: f32 values, taken as exact).
  the dot product   lane l accumulates the D / 64 elements 4 l + 256 i + {0 .. 3} with one fmaf each (ONE rounding per term: the product is not rounded), then the
                    64 lane sums meet in a 6-level xor butterfly (one rounding per level). A term passes through at most m = D / 64 + 6 roundings, each of
                    relative size u of a partial sum that is at most S = sum_k |w[o][k] x[b][k]|:            gamma_m S = m u S
  the bias add      one rounding of a value of at most S + |bias|:                                             u (S + |bias|)
                    E_pre = (D / 64 + 7) u S + u |bias|
  the activation    v > 0 ? v : v * 0.2f, then * sqrt2f. leaky_relu is 1-Lipschitz, so E_pre passes unamplified and the gain multiplies it by sqrt(2). The
                    two products: each rounds once (u), and each constant is the f32 rounding of the reference's double (0.2, sqrt(2): relative u each). The
                    slope product exists for v < 0 only:    E = sqrt(2) E_pre + (2 + 2 [v < 0]) u |y|
A result below the smallest normal f32 may be flushed: + 2^-126.

THE WHOLE MODEL (layerwise_ratio): chaining the layer bounds through |w'| would multiply the error by the absolute row sums, about 0.8 sqrt(D) sqrt(2) per layer,
10^6 .. 10^8 over five layers: a true bound and a useless one. Instead every layer of an implementation is judged on ITS OWN input: layer l's output against the
float64 layer applied to the implementation's output of layer l - 1 (z for the first), under the layer bound above plus the load-time fold, which stands 2 u
relative beside the float64 reference's exact w scale and b lr_mul (w' = fl(w fl(scale)), b' = fl(b fl(lr_mul)): the constant's rounding and the product's):
    E_pre,l = (D / 64 + 7 + 2 f) u S + (1 + 2 f) u |b'|,   f = 1 for the EqualLinear layers, 0 for the last
The input of a layer is exact by construction (both sides read the same values).

NOISE: rlg_noise_kernel is diffusion.hip's philox_normal with counter {i >> 1, 0, side, TAG}; noise_reference restates tests/voc_cases.py's philox_reference with
those counter words and keeps its bound (logf 2 ulp, sqrtf 1 ulp, sincosf 2 ulp).

EXACT FAMILY: w in {-2 .. 2}, x in {-3 .. 3}, bias in {-8 .. 8}, act 0: every product, partial sum and the result are integers below 2^24 in magnitude, so any
order of f32 additions is exact and the kernel's result must equal the integer reference bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import voc_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_RLG_TEST_LIB") or os.path.join(PKG, "libtts_rlg_test.so")

LAYER, NOISE = 0, 1
SENTINEL = 0xCB
HIP_INVALID_VALUE = 1
U = 2.0 ** -24
FMIN = 2.0 ** -126
SLOPE32, GAIN32 = np.float32(0.2), np.float32(np.sqrt(2.0))
DIFFUSION_TAG, VOCODER_TAG = 0x7715, 0x7716
DIMS = (256, 1024, 2048)  # 256: the smallest the kernel accepts (a row is 64 lanes x float4); below it every case is refused


class CaseStruct(C.Structure):
    _fields_ = [("op", C.c_int), ("dim", C.c_int), ("n", C.c_int), ("act", C.c_int), ("side", C.c_int), ("poison", C.c_int),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("x", C.c_void_p), ("seeds", C.c_void_p), ("out", C.c_void_p)]


class HipError(RuntimeError):
    pass


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_rlg_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_rlg_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_rlg_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_rlg_test_validate.argtypes = [C.POINTER(CaseStruct)]
        for f in (L.tts_rlg_test_run, L.tts_rlg_test_validate, L.tts_rlg_test_margin, L.tts_rlg_test_tile, L.tts_rlg_test_min_dim, L.tts_rlg_test_max_dim):
            f.restype = C.c_int
        L.tts_rlg_test_tag.restype = C.c_uint
        _lib = L
    return _lib


def tile():
    return harness().tts_rlg_test_tile()


class Guarded:
    """margin | payload | margin, as the harness copies the output buffer back"""

    def __init__(self, shape):
        self.margin = harness().tts_rlg_test_margin()
        self.shape = shape
        self.raw = np.zeros(int(np.prod(shape)) * 4 + 2 * self.margin, np.uint8)

    @property
    def data(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(np.float32).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


def _p(a):
    return None if a is None else a.ctypes.data


def layer_struct(w, bias, x, act, out, poison=0, dim=None, n=None):
    return CaseStruct(op=LAYER, dim=w.shape[1] if dim is None else dim, n=x.shape[0] if n is None else n, act=act, side=0, poison=poison, w=_p(w), bias=_p(bias), x=_p(x),
                      seeds=None, out=_p(out.raw) if out is not None else None)


def run_layer(w, bias, x, act, poison=0):
    """one launch of rlg_layer_kernel -> Guarded [n, D]"""
    w, bias, x = (np.ascontiguousarray(a, np.float32) for a in (w, bias, x))
    out = Guarded(x.shape)
    rc = harness().tts_rlg_test_run(C.byref(layer_struct(w, bias, x, act, out, poison)))
    if rc != 0:
        raise HipError("rlg_layer_kernel: HIP error %d" % rc)
    return out


def run_noise(seeds, side, dim):
    s = np.ascontiguousarray(seeds, np.uint64)
    out = Guarded((len(s), dim))
    rc = harness().tts_rlg_test_run(C.byref(CaseStruct(op=NOISE, dim=dim, n=len(s), act=0, side=side, poison=0, w=None, bias=None, x=None, seeds=_p(s), out=_p(out.raw))))
    if rc != 0:
        raise HipError("rlg_noise_kernel: HIP error %d" % rc)
    return out


# ---------------------------------------------------------------------------------------------------------------- references and bounds

def layer_reference(w, bias, x, act, mut=None):
    """float64 on the f32 operands -> (y [n, D], bound [n, D])"""
    w64, b64, x64 = (np.asarray(a, np.float64) for a in (w, bias, x))
    D = w64.shape[1]
    v = x64 @ w64.T + b64
    S = np.abs(x64) @ np.abs(w64).T
    e_pre = (D // 64 + 7) * U * S + U * np.abs(b64)
    if not act:
        return v, e_pre + FMIN
    y = np.where(v > 0, v, v * 0.2) * np.sqrt(2.0)
    return y, np.sqrt(2.0) * e_pre + (2 + 2 * (v < 0)) * U * np.abs(y) + FMIN


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two f32 is exact in float64; the sum rounds to float64, then to float32 (a double rounding that differs from the
    fused result only on a tie the first rounding creates: inside u either way)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def layer_kernel_order32(w, bias, x, act):
    """float32 in rlg_layer_kernel's own order: per lane fmaf over elements 4 l + 256 i + j (i, then j ascending), the xor butterfly 32 .. 1, bias, activation"""
    w, bias, x = (np.ascontiguousarray(a, np.float32) for a in (w, bias, x))
    n, D = x.shape
    ns = D // 256
    wl = w.reshape(D, ns, 64, 4)   # [o][i][lane][j]
    xl = x.reshape(n, ns, 64, 4)
    out = np.empty((n, D), np.float32)
    lanes = np.arange(64)
    for b in range(n):
        acc = np.zeros((D, 64), np.float32)
        for i in range(ns):
            for j in range(4):
                acc = _fma32(wl[:, i, :, j], np.broadcast_to(xl[b, i, :, j], (D, 64)), acc)
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, lanes ^ o]).astype(np.float32)
        v = (acc[:, 0] + bias).astype(np.float32)
        if act:
            v = (np.where(v > 0, v, (v * SLOPE32).astype(np.float32)) * GAIN32).astype(np.float32)
        out[b] = v
    return out


def fold32(tensors):
    """[(w', b')] per layer as the loader folds them: float32 products with the float32 roundings of scale and lr_mul; the last layer unchanged"""
    L = 0
    while "layers.%d.weight" % L in tensors:
        L += 1
    out = []
    for l in range(L):
        w, b = np.asarray(tensors["layers.%d.weight" % l], np.float32), np.asarray(tensors["layers.%d.bias" % l], np.float32)
        if l < L - 1:
            w, b = w * np.float32(0.1 / np.sqrt(float(w.shape[1]))), b * np.float32(0.1)
        out.append((w, b))
    return out


def model_kernel_order32(tensors, z):
    """the whole model as the device runs it: the fold, then layer_kernel_order32 per layer -> the per-layer outputs"""
    x = np.ascontiguousarray(z, np.float32)
    layers = fold32(tensors)
    outs = []
    for l, (w, b) in enumerate(layers):
        x = layer_kernel_order32(w, b, x, l < len(layers) - 1)
        outs.append(x)
    return outs


def layerwise_ratio(tensors, z, outs):
    """outs: the per-layer outputs [L][n, D] of an implementation run on z. Every layer on its own input (module docstring) -> the worst |error| / bound per layer"""
    L = len(fold32(tensors))
    assert len(outs) == L
    worst = []
    for l in range(L):
        last = l == L - 1
        x = np.asarray(z if l == 0 else outs[l - 1], np.float64)
        D = x.shape[1]
        w = np.asarray(tensors["layers.%d.weight" % l], np.float64) * (1.0 if last else 0.1 / np.sqrt(float(D)))
        b = np.asarray(tensors["layers.%d.bias" % l], np.float64) * (1.0 if last else 0.1)
        f = 0 if last else 1
        v = x @ w.T + b
        S = np.abs(x) @ np.abs(w).T
        e_pre = (D // 64 + 7 + 2 * f) * U * S + (1 + 2 * f) * U * np.abs(b)
        if last:
            y, E = v, e_pre + FMIN
        else:
            y = np.where(v > 0, v, v * 0.2) * np.sqrt(2.0)
            E = np.sqrt(2.0) * e_pre + (2 + 2 * (v < 0)) * U * np.abs(y) + FMIN
        worst.append(float((np.abs(np.asarray(outs[l], np.float64) - y) / E).max()))
    return worst


def noise_reference(n, seed, side, tag=None, c1=0):
    """rlg_noise_kernel: -> (float64 reference [n], bound [n]); tests/voc_cases.py's philox_reference with this stage's counter words {i >> 1, c1, side, tag}"""
    tag = harness().tts_rlg_test_tag() if tag is None else tag
    seed = int(seed)
    i = np.arange(n, dtype=np.uint64)
    r = VC.philox4x32_10([i >> np.uint64(1), c1, side, tag], [seed & 0xFFFFFFFF, seed >> 32])
    f = np.float32
    u1 = (r[0].astype(f) + f(1)) * f(2.0 ** -32)
    u2 = r[1].astype(f) * f(2.0 ** -32)
    with np.errstate(divide="ignore"):
        rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    theta = 2.0 * np.pi * u2.astype(np.float64)
    x = np.where(np.arange(n) & 1, rad * np.sin(theta), rad * np.cos(theta))
    return x, rad * (2 * U * theta + 4 * U) + 5 * U * np.abs(x)


# ---------------------------------------------------------------------------------------------------------------- the case matrix

def batch_sizes():
    t = tile()
    return (1, 2, t - 1, t, t + 1, 2 * t + 1)


def layer_operands(D, n, seed, family="gauss"):
    """(w, bias, x) f32. gauss: the folded operands' scale (w ~ N(0, 1 / sqrt(D)), bias ~ 0.2 N, x ~ N(0, 1)); exact: the small-integer family"""
    r = np.random.default_rng(seed)
    if family == "exact":
        return (r.integers(-2, 3, (D, D)).astype(np.float32), r.integers(-8, 9, D).astype(np.float32), r.integers(-3, 4, (n, D)).astype(np.float32))
    w = (r.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    return w, (0.2 * r.standard_normal(D)).astype(np.float32), r.standard_normal((n, D)).astype(np.float32)


def invalid_cases():
    """(name, CaseStruct) the harness must refuse; the arrays are kept alive by the returned list"""
    D = 256
    w, b, x = layer_operands(D, 2, 1)
    seeds = np.array([1, 2], np.uint64)
    out = Guarded((2, D))
    keep = (w, b, x, seeds, out)
    good = dict(op=LAYER, dim=D, n=2, act=1, side=0, poison=0, w=_p(w), bias=_p(b), x=_p(x), seeds=None, out=_p(out.raw))
    gn = dict(good, op=NOISE, w=None, bias=None, x=None, seeds=_p(seeds))
    cases = [("op", dict(good, op=2)), ("op negative", dict(good, op=-1)), ("dim 0", dict(good, dim=0)), ("dim below the smallest", dict(good, dim=128)),
             ("dim 255", dict(good, dim=255)), ("dim not a multiple of 256", dict(good, dim=384)), ("dim above the largest", dict(good, dim=2304)),
             ("dim negative", dict(good, dim=-256)), ("n 0", dict(good, n=0)), ("n negative", dict(good, n=-1)), ("n above the cap", dict(good, n=65)),
             ("act 2", dict(good, act=2)), ("poison 2", dict(good, poison=2)), ("no w", dict(good, w=None)), ("no bias", dict(good, bias=None)),
             ("no x", dict(good, x=None)), ("no out", dict(good, out=None)), ("noise: no seeds", dict(gn, seeds=None)), ("noise: side 2", dict(gn, side=2)),
             ("noise: side negative", dict(gn, side=-1)), ("noise: dim 64", dict(gn, dim=64)), ("noise: no out", dict(gn, out=None))]
    return [(name, CaseStruct(**c)) for name, c in cases], keep
