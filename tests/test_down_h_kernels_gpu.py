"""cls_down_h_kernel (csrc/cls_down_h.h, option addon_conv_precision 1 and 2) and the weight packer, one launch at a time through libtts_down_h_test.so and
cls_launch_down_h, against float64 ON THE VALUES THE KERNEL MULTIPLIES: the clamp to +-65504, hi = rn_f16(v), lo = rn_f16(v - hi) and the pack (one power-of-two
scale s per output channel, the column's largest |w| s in [2^12, 2^13)) are restated bit for bit in NumPy; the products the mode forms (hi hi; in mode 2 lo hi,
hi lo, hi hi) are summed in float64. Bound, the rule of tests/test_hfg_h_kernels_gpu.py with nothing fitted: (2 n m + c) u mag, u = 2^-24, n = taps cin, m = 1 | 3,
c = 2 (the scale multiply, the bias add), mag = sum |terms| / s + |bias|. A clip of n rows has (n - 1) // stride + 1 output rows in every geometry
(cls_cases.Case): without padding the last rows read behind the clip's end, as zero."""
import ctypes as C
import os

import numpy as np
import pytest

import cls_cases as V

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
_lib = None

class CaseStruct(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("ns", "rows", "rows_out", "cin", "cout", "taps", "stride", "pad", "split")] + [
        (k, C.c_void_p) for k in ("n", "start", "n_out", "start_out", "in_", "w", "bias", "out")]

def harness():  # a missing library is an error, never a skip
    global _lib
    if _lib is None:
        _lib = C.CDLL(os.path.join(V.PKG, "libtts_down_h_test.so"))
        _lib.tts_down_h_test_run.argtypes = [C.POINTER(CaseStruct)]
        assert _lib.tts_down_h_test_margin() == V.harness().tts_cls_test_margin()  # cls_cases.Guarded's margin
    return _lib

R = 64  # the kernel's row tile (asserted against the harness in launch)
GEOMS = [(5, 4, 2), (3, 2, 0), (2, 2, 0), (2, 4, 0)]  # (taps, stride, pad): the classifier's, the aligner's two, taps < stride
ROWS = [([1], 8), ([R - 1], 8), ([R], 8), ([R + 1], 8), ([2 * R + 3], 8), ([40, 70], 0), ([5, 2 * R + 3], 8)]  # (output rows of the clips, gap: 0 = touching clips)
CH = [(32, 64), (96, 128), (96, 64), (32, 128)]  # cin 32: one chunk; 96: 64 + a tail of 32 in mode 1, three chunks in mode 2; cout 128: two column workgroups
CASES = [(g, r, CH[(i + j) % 4], "gauss") for i, g in enumerate(GEOMS) for j, r in enumerate(ROWS)] + [
    (g, ROWS[-1], CH[1], fam) for g in GEOMS for fam in ("small", "clamp", "exact")]

def make(geom, rows, ch, fam):
    (taps, stride, pad), (n_out, gap), (cin, cout) = geom, rows, ch
    c = V.make(V.DOWN, [o * stride - 1 for o in n_out], cin, cout, taps=taps, stride=stride, gap=gap)
    assert c.n_out == n_out
    x, live = c.a["in_"], c.live()
    if fam == "small":  # 2^-10: every low half is an fp16 subnormal
        x *= f32(2.0 ** -10)
    if fam == "clamp":  # 1e5 and -1e5 on live rows: the operand is +-65504
        x[c.start[0], 3], x[c.start[0] + 1, 17] = 1.0e5, -1.0e5
    if fam == "exact":
        rs = np.random.RandomState(5)
        x[:] = rs.randint(-4, 5, x.shape)
        c.a["w"], c.a["bias"] = rs.randint(-3, 4, c.a["w"].shape).astype(f32), rs.randint(-8, 9, cout).astype(f32)
    x[~live] = V.JUNK
    return c

def pair(v):  # hi = rn_f16(v), lo = rn_f16(v - hi) of an f32 array (v - hi is exact in f32), as float64
    v = np.asarray(v, f32)
    hi = v.astype(f16)
    return hi.astype(f64), (v - hi.astype(f32)).astype(f16).astype(f64)

def reference(c, s, pad, mode):  # (float64 output, bound) of clip s
    x, w, b = c.a["in_"][c.clip(s)], c.a["w"], c.a["bias"].astype(f64)
    n, F, K, n_out = len(x), c.stride, c.taps, c.n_out[s]
    m = np.abs(w).max(axis=(0, 1))
    e = np.where(m > 0, np.frexp(m)[1] - 1, harness().tts_down_h_test_scale_exp())
    sc = np.ldexp(f32(1), harness().tts_down_h_test_scale_exp() - e).astype(f32)
    xp = np.zeros((pad + n + F * n_out + K, x.shape[1]), f32)
    xp[pad:pad + n] = np.clip(x, f32(-65504), f32(65504))
    xh, xl = pair(xp)
    wh, wl = pair(w * sc[None, None, :])
    acc, mag = np.zeros((n_out, c.C2)), np.zeros((n_out, c.C2))
    for j in range(K):
        rows = slice(j, j + F * (n_out - 1) + 1, F)
        for x_, w_ in ([(xl, wh), (xh, wl), (xh, wh)] if mode == 2 else [(xh, wh)]):
            acc += x_[rows] @ w_[j]
            mag += np.abs(x_[rows]) @ np.abs(w_[j])
    mag = mag / sc + np.abs(b)
    return acc / sc + b, (2 * K * c.C * (3 if mode == 2 else 1) + 2) * V.U * mag

def launch(c, pad, mode):
    L = harness()
    assert L.tts_down_h_test_row_tile() == R
    out = V.Guarded((c.rows_out, c.C2))
    keep = [np.array(a, np.int32) for a in (c.n, c.start, c.n_out, c.start_out)] + [np.ascontiguousarray(c.a[k], f32) for k in ("in_", "w", "bias")]
    p = [a.ctypes.data_as(C.c_void_p) for a in keep]
    cs = CaseStruct(ns=c.ns, rows=c.rows, rows_out=c.rows_out, cin=c.C, cout=c.C2, taps=c.taps, stride=c.stride, pad=pad, split=mode - 1, n=p[0], start=p[1],
                    n_out=p[2], start_out=p[3], in_=p[4], w=p[5], bias=p[6], out=out.raw.ctypes.data_as(C.c_void_p))
    rc = L.tts_down_h_test_run(C.byref(cs))
    if rc:  # a failed HIP call (a fault included) ends the session: nothing more is started on a GPU that may have faulted
        pytest.exit("cls_down_h %s: status %d" % (c.name(), rc), returncode=3)
    assert out.canaries_intact()
    return np.ascontiguousarray(out.payload).view(np.uint32)

@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("case", CASES, ids=["k%d-s%d-p%d-n%s-g%d-c%d_%d-%s" % (g + ("_".join(map(str, r[0])), r[1]) + ch + (f,)) for g, r, ch, f in CASES])
def test_strided_convolution_against_float64(case, mode):
    c, pad, fam = make(*case), case[0][2], case[3]
    bits = launch(c, pad, mode)
    got, live = bits.view(f32), c.live(out=True)
    refs = [reference(c, s, pad, mode) for s in range(c.ns)]
    worst = max((np.abs(got[c.clip(s, out=True)].astype(f64) - ref) / bound).max() for s, (ref, bound) in enumerate(refs))
    print("%s mode %d: worst |err| / bound %.4f" % (case, mode, worst))
    assert np.isfinite(got[live]).all() and worst <= 1.0
    if fam == "exact":
        assert all(np.array_equal(got[c.clip(s, out=True)].astype(f64), ref) for s, (ref, _) in enumerate(refs)), "the exact family is not exact"
    assert (bits[~live] == V.SENTINEL * 0x01010101).all(), "a store left the live rows"
    assert np.array_equal(launch(c, pad, mode), bits), "two runs differ"
    assert np.array_equal(launch(V.poisoned(c), pad, mode), bits), "the launch read a row outside the clips"
    for s in range(c.ns if c.ns > 1 else 0):
        a = V.alone(c, s)
        assert np.array_equal(launch(a, pad, mode)[a.clip(0, out=True)], bits[c.clip(s, out=True)]), "clip %d differs from itself alone" % s
