"""hfg_conv_h_kernel (csrc/hfg_conv_h.h: the HiFi-GAN convolutions on the fp16 MFMA, option hfg_precision 1 and 2) and its weight packer, one launch at a time
through the test-only harness libtts_hfg_h_test.so, against float64 ON THE VALUES THE KERNEL MULTIPLIES: the activation path (f32 leaky step, clamp to +-65504,
rn_f16, lo = rn_f16(v - hi)) and the pack (one power-of-two scale per output channel, hi = rn_f16(w s), lo = rn_f16(w s - hi)) are restated bit for bit in NumPy,
the products the kernel forms (hi hi in mode 1; lo hi, hi lo, hi hi in mode 2) are summed in float64, the epilogue is float64. Quantisation is in no kernel's error.
Bound, the rule of tests/hfg_cases.py with nothing fitted: (2n + c) u (sum |terms| + |bias| + |cbias| + |resid| + |out_prev|), u = 2^-24, n = the MFMA products
per element (taps cin, x 3 in mode 2), c = hfg_cases.conv_c + 1 for the scale multiply. The exact family (small integers, slope 0.5 or 1) must equal float64 bit
for bit. Every case besides: two runs give the same bits, NaN on every row outside the candidates changes nothing, no store leaves the live rows, canaries intact."""
import ctypes as C
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import hfg_cases as V
from hfg_cases import CONV

pytestmark = pytest.mark.gpu
LIB = os.path.join(V.PKG, "libtts_hfg_h_test.so")
f16, f32, f64 = np.float16, np.float32, np.float64
F16_MAX = f32(65504.0)
_lib = None


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def harness():
    """built once with make if it is missing; a missing library is an error, never a skip"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", V.PKG, "libtts_hfg_h_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        L = C.CDLL(LIB)
        L.tts_hfg_h_test_run.argtypes = [C.POINTER(V.CaseStruct), C.c_int]
        L.tts_hfg_h_test_run.restype = C.c_int
        assert L.tts_hfg_h_test_margin() == V.harness().tts_hfg_test_margin()  # hfg_cases.Guarded's margin
        _lib = L
    return _lib


def pair(v):
    """hi = rn_f16(v), lo = rn_f16(v - hi) of an f32 array (v - hi is exact in f32)"""
    v = np.asarray(v, f32)
    hi = v.astype(f16)
    return hi, (v - hi.astype(f32)).astype(f16)


def reference(c, split):
    p, a, lay = c.p, c.a, c.lay
    groups, shape, n = V._conv_groups(c)  # (output rows, leaky_relu'd f32 operand rows, W [cin][cout]) per tap
    m = np.abs(a["w"]).max(axis=(0, 2) if p["phases"] > 1 else (0, 1))  # a transposed convolution is held as [cin][cout][2u]
    e = np.where(m > 0, np.frexp(m)[1] - 1, harness().tts_hfg_h_test_scale_exp())
    s = np.ldexp(f32(1), harness().tts_hfg_h_test_scale_exp() - e).astype(f32)  # the column's largest |w| s lies in [2^12, 2^13)
    acc, asum = np.zeros(shape), np.zeros(shape)
    for idx, X, W in groups:
        xh, xl = pair(np.clip(X, -F16_MAX, F16_MAX))
        wh, wl = pair(W * s[None, :])
        for x_, w_ in ([(xl, wh), (xh, wl), (xh, wh)] if split else [(xh, wh)]):
            acc[idx] += x_.astype(f64) @ w_.astype(f64)
            asum[idx] += np.abs(x_.astype(f64)) @ np.abs(w_.astype(f64))
    acc, asum = acc / s.astype(f64), asum / s.astype(f64)
    live = lay.live(c.R_out)
    voice = np.zeros(shape[0], np.int64)
    for q in range(lay.ns):
        voice[lay.rows(q, c.R_out)] = lay.voice[q]
    bias = a["bias"].astype(f64)[None, :]
    cb = a["cbias"].astype(f64)[voice] if "cbias" in a else np.zeros(shape)
    prev = a["out0"].astype(f64) if "out0" in a else np.zeros(shape)
    resid = a["resid"].astype(f64) if p["resid"] == 1 else prev if p["resid"] == 2 else np.zeros(shape)
    v = acc + bias + cb + resid
    if p["acc"] == 1:
        v = prev + v
    elif p["acc"] == 2:
        v = (prev + v) / 3
    mag = asum + np.abs(bias) + np.abs(cb) + np.abs(resid) + (np.abs(prev) if p["acc"] else 0)
    lv = live[:, None]
    with np.errstate(invalid="ignore"):
        return dict(z=np.where(lv, v, 0.0), bound=np.where(lv, (2 * n * (3 if split else 1) + V.conv_c(p) + 1) * V.U * mag, 0.0), live=live,
                    exact=c.family == "exact", mag=np.where(lv, mag, 0.0))


def launch(c, split):
    out = V.Guarded(V.out_shape(c))
    rc = harness().tts_hfg_h_test_run(C.byref(V.to_struct(c, out)), split)
    if rc:  # a failed HIP call (a fault included) ends the session: nothing more is started on a GPU that may have faulted
        pytest.exit("%s: HIP error %d" % (c.name(), rc), returncode=3)
    assert out.canaries_intact(), c.name()
    return out.payload


G = "gauss"


def rows(W, rate):
    """one candidate of W * rate rows, three taps"""
    return V.Layout([V.whole(W)]), G, dict(cin=32, cout=32, taps=3, rate=rate)


CASES = [  # (layout, family, parameters): cin 32 | 96 = two chunks of 64 (three of 32 in mode 2), cout 32 | 64 = two column tiles of a workgroup | 96 = three workgroups
    ("A", G, dict(cin=32, cout=32, taps=1)),                                              # one product per chunk; 4 rows
    ("A", G, dict(cin=96, cout=64, taps=11, dil=5, resid=1)),                             # a candidate shorter than the tap reach
    ("B", G, dict(cin=32, cout=96, taps=3, rate=57, acc=1, resid=2)),                     # touching candidates, 513 and 228 rows; resid == out
    ("C", G, dict(cin=96, cout=32, taps=7, dil=3, rate=8, acc=2, cbias=1)),               # a short candidate in a long grid, two voices
    ("D", G, dict(cin=32, cout=64, taps=11, dil=5, rate=8, cbias=1, resid=1)),            # chunk windows
    ("C", G, dict(cin=96, cout=64, taps=2, phases=8, cbias=1)),
    ("B", G, dict(cin=32, cout=32, taps=2, phases=2, rate=57, slope=1.0)),
    rows(15, 17), rows(16, 16), rows(1, 257),                                             # tile - 1, tile, tile + 1 rows
    ("B", "exact", dict(cin=96, cout=64, taps=7, dil=3, rate=57, slope=0.5, acc=2, cbias=1)),
    ("B", "exact", dict(cin=32, cout=96, taps=3, rate=8, slope=1.0, acc=1, resid=2)),
    ("C", "exact", dict(cin=96, cout=32, taps=2, phases=8, slope=0.5, cbias=1)),
    ("A", "clamp", dict(cin=32, cout=32, taps=3, slope=1.0)),
]


@pytest.mark.parametrize("split", [0, 1], ids=["f16", "split"])
@pytest.mark.parametrize("l,fam,p", CASES, ids=["%s-%s-%s" % (l if isinstance(l, str) else "rows%d" % (l.W[0] * p["rate"]), f, "-".join("%s%s" % kv for kv in sorted(p.items())))
                                                for l, f, p in CASES])
def test_case_is_accepted(l, fam, p, split):
    c = V.make(CONV, l, G if fam == "clamp" else fam, seed=70, **p)
    if fam == "clamp":  # 1e5 and -1e5 on live rows: the operand is +-65504
        c.a["in_"][1, 3], c.a["in_"][2, 17] = 1.0e5, -1.0e5
    ref = reference(c, split)
    o = launch(c, split)
    bad, r = V.judge(o, ref)
    print("%-100s mode %d rejected %d worst |err|/bound %.4f" % (c.name(), split + 1, bad, r))
    assert bad == 0, (c.name(), bad, r)
    if ref["exact"]:
        assert V.exact_family_is_exact(c, ref) and V.exact_ok(o, ref), c.name()
    assert V.guards_ok(c, o), c.name()  # no store outside the live rows, every live element written
    bits = np.ascontiguousarray(o).view(np.uint32)
    assert np.array_equal(np.ascontiguousarray(launch(c, split)).view(np.uint32), bits), "two runs differ"
    assert np.array_equal(np.ascontiguousarray(launch(V.poisoned(c), split)).view(np.uint32), bits), "the launch read a row outside the candidates"
