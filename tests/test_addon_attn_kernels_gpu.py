"""addon_attn_h_kernel (csrc/addon_attn_h.h: the classifier's and the aligner's attention on the fp16 MFMA, option addon_attn_precision 1 and 2), one launch at a
time through the test-only harness libtts_attn_h_test.so and cls_launch_attn_h, the launcher classifier_run and aligner_run call, against float64 ON THE VALUES
THE KERNEL MULTIPLIES: the f32 multiply by DH^-1/4, the clamp to +-65504 and hi = rn_f16(v), lo = rn_f16(v - hi) of q, k and v are restated bit for bit in
NumPy; the products the mode forms (hi hi; in mode 2 also lo hi and hi lo) are summed in float64, the softmax and P V are float64.

Bound, nothing fitted: cls_cases.ref_attn's own bound on the same qkv (its U, EXP_REL and DIV; (DH + 4) roundings per score), plus, with A = sum |q k| / sqrt(DH),
w the float64 softmax and u = 2^-24:
  per score   DH (m - 1) u A  (m = 1 | 3 products per step)  +  in mode 2 the dropped lo lo products, 2^-22 A;  carried through the softmax as ref_attn carries e_s
  P           mode 1: its one fp16 rounding, 2^-11 w |v|;  mode 2: the residual of its pair and the dropped lo lo product, 2 x 2^-22 w |v|, and the two further
              accumulations per key, 2 n u w |v|;  both: a weight under 2^-28 meets fp16's subnormal quantum behind the 2^14 scale, 2^-39 sum_j |v_j|
  merge       the two key halves: two expf, two products, one fused multiply-add and the 2^-14 multiply (exact): (2 EXP_REL + 4 u) w |v|
The "small" family (q, k, v of 2^-10: every low half is an fp16 subnormal) leaves this bound at one key if the matrix pipe flushes them. Every case besides: two
runs agree, NaN outside the clips changes nothing, sentinel and canaries intact, each clip of a multi-clip case alone gives the bits it has in the batch."""
import ctypes as C
import os

import numpy as np
import pytest

import cls_cases as V

pytestmark = pytest.mark.gpu
LIB = os.path.join(V.PKG, "libtts_attn_h_test.so")
f16, f32, f64 = np.float16, np.float32, np.float64
_lib = None


class CaseStruct(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("ns", "rows", "E", "heads", "split")] + [(k, C.c_void_p) for k in ("n", "start", "qkv", "out")]


def harness():  # a missing library is an error, never a skip
    global _lib
    if _lib is None:
        _lib = C.CDLL(LIB)
        _lib.tts_attn_h_test_run.argtypes = [C.POINTER(CaseStruct)]
        assert _lib.tts_attn_h_test_margin() == V.harness().tts_cls_test_margin()  # cls_cases.Guarded's margin
    return _lib


Q = K = 64  # the kernel's query and key tiles (asserted against the harness in launch)
CASES = [(n, 8, "gauss") for n in ([1], [K - 1], [K], [K + 1], [215])] + [  # (rows of the clips, gap: 0 = touching clips, family); Q - 1, Q, Q + 1 are K - 1, K, K + 1
    ([40, 70], 0, "gauss"), ([5, 2 * K + 3], 8, "gauss"), ([215], 8, "peaked"), ([5, 2 * K + 3], 8, "peaked"),
    ([1], 8, "small"), ([K + 1], 8, "small"), ([40, 70], 0, "small"), ([Q - 1], 8, "clamp")]


def make(n, gap, fam, dh):
    c = V.make(V.ATTN, n, 2 * dh, heads=2, gap=gap, fam="peaked" if fam == "peaked" else "gauss")
    x, E = c.a["in_"], 2 * dh
    if fam == "small":
        x *= f32(2.0 ** -10)
    if fam == "clamp":  # one live v element each of 1e5 and -1e5: the operand is +-65504
        x[c.start[0], 2 * E + 3], x[c.start[0] + min(1, n[0] - 1), 2 * E + dh + 17] = 1.0e5, -1.0e5
    x[~c.live()] = V.JUNK
    return c


def pair(v):
    """hi = rn_f16(v), lo = rn_f16(v - hi) of an f32 array clamped to fp16's range (v - hi is exact in f32)"""
    v = np.clip(np.asarray(v, f32), f32(-65504), f32(65504))
    hi = v.astype(f16)
    return hi.astype(f64), (v - hi.astype(f32)).astype(f16).astype(f64)


def reference(c, s, mode):
    """(float64 output, bound) of clip s"""
    x = c.a["in_"][c.clip(s)]
    n, E, H, dh = len(x), c.C, c.heads, c.C // c.heads
    y, ext = np.zeros((n, E)), np.zeros((n, E))
    for h in range(H):
        q, k, v = (x[:, t * E + h * dh:t * E + (h + 1) * dh] for t in range(3))
        (qh, ql), (kh, kl), (vh, vl) = pair(q * f32(dh ** -0.25)), pair(k * f32(dh ** -0.25)), pair(v)
        sc = qh @ kh.T + ((ql @ kh.T + qh @ kl.T) if mode == 2 else 0.0)
        w = np.exp(sc - sc.max(axis=1, keepdims=True))
        w /= w.sum(axis=1, keepdims=True)
        y[:, h * dh:(h + 1) * dh] = w @ (vh + vl if mode == 2 else vh)
        A, av = (np.abs(q.astype(f64)) @ np.abs(k.astype(f64)).T) * dh ** -0.5, np.abs(v.astype(f64))
        e_s = (dh * 2 * V.U + 2.0 ** -22) * A if mode == 2 else 0.0 * A
        e_w = w * (e_s + (w * e_s).sum(axis=1, keepdims=True))
        p_rel = (2 * 2.0 ** -22 + 2 * n * V.U) if mode == 2 else 2.0 ** -11
        ext[:, h * dh:(h + 1) * dh] = e_w @ av + (p_rel + 2 * V.EXP_REL + 4 * V.U) * (w @ av) + 2.0 ** -39 * av.sum(axis=0)
    return y, V.ref_attn(c, s)[1] + ext


def launch(c, mode):
    L = harness()
    assert L.tts_attn_h_test_query_tile() == Q and L.tts_attn_h_test_key_tile() == K
    out = V.Guarded((c.rows, c.C))
    keep = [np.array(c.n, np.int32), np.array(c.start, np.int32), np.ascontiguousarray(c.a["in_"])]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cs = CaseStruct(ns=c.ns, rows=c.rows, E=c.C, heads=c.heads, split=mode - 1, n=p(keep[0]), start=p(keep[1]), qkv=p(keep[2]), out=p(out.raw))
    rc = L.tts_attn_h_test_run(C.byref(cs))
    if rc:  # a failed HIP call (a fault included) ends the session: nothing more is started on a GPU that may have faulted
        pytest.exit("addon_attn_h %s: status %d" % (c.name(), rc), returncode=3)
    assert out.canaries_intact()
    return np.ascontiguousarray(out.payload).view(np.uint32)


@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("case", CASES, ids=["n%s-g%d-%s" % ("_".join(map(str, c[0])), c[1], c[2]) for c in CASES])
def test_attention_against_float64(case, dh, mode):
    c = make(*case, dh)
    bits = launch(c, mode)
    got, live = bits.view(f32), c.live()
    refs = [reference(c, s, mode) for s in range(c.ns)]
    worst = max((np.abs(got[c.clip(s)].astype(f64) - ref) / bound).max() for s, (ref, bound) in enumerate(refs))
    print("%s dh %d mode %d: worst |err| / bound %.4f" % (case, dh, mode, worst))
    assert np.isfinite(got[live]).all() and worst <= 1.0
    assert (bits[~live] == V.SENTINEL * 0x01010101).all(), "a store left the live rows"
    assert np.array_equal(launch(c, mode), bits), "two runs differ"
    assert np.array_equal(launch(V.poisoned(c), mode), bits), "the launch read a row outside the clips"
    for s in range(c.ns if c.ns > 1 else 0):
        a = V.alone(c, s)
        assert np.array_equal(launch(a, mode)[a.clip(0)], bits[c.clip(s)]), "clip %d differs from itself alone" % s
