"""w2v_linear_h_kernel (csrc/w2v_linear_h.h: the aligner's Linears on the fp16 MFMA, option aligner_precision 1 and 2), one launch at a time through the test-only
harness libtts_w2v_h_test.so and the launcher aligner_run calls, against float64 ON THE VALUES THE KERNEL MULTIPLIES, as tests/test_hfg_h_kernels_gpu.py does
it: the activation path (clamp to +-65504, rn_f16, lo = rn_f16(v - hi)) and the pack (one power-of-two scale s per column, hi = rn_f16(w s), lo = rn_f16(w s -
hi)) are restated bit for bit in NumPy, the products the kernel forms (hi hi in mode 1; lo hi, hi lo, hi hi in mode 2) are summed in float64, the epilogue is
float64 (GELU with erf). Bound, nothing fitted: e_v = (2 n m + c) u (sum |terms| / s + |bias| + |resid|), u = 2^-24, n = cin, m = 1 | 3, c = 2 (the scale
multiply, the bias add) + 1 with a residual. Under the GELU epilogue e_v goes through tests/w2v_cases.py's GELU rule (1.13 e_v + 0.5 |v| (ERF_ABS + 1.13 u |v|)
+ 3 u |y|, ERF_ABS = 8 u: the documented 4 ulp of the device erff). The exact family (small integers, weights a small integer times a power of two per column)
must equal float64 bit for bit in both modes, except under the GELU epilogue. An unwritten live element keeps the sentinel (-2.7e7) or out0 and leaves the bound.
Every case besides: two runs give the same bits, NaN on every row outside the clips changes nothing, no store leaves the live rows, canaries intact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import w2v_cases as V

pytestmark = pytest.mark.gpu
LIB = os.path.join(V.PKG, "libtts_w2v_h_test.so")
f16, f32, f64 = np.float16, np.float32, np.float64
BIAS, GELU, RESID, ALIAS = "bias", "gelu", "resid", "alias"  # alias: bias + residual with resid == out
_lib = None


class CaseStruct(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("ns", "rows", "cin", "cout", "epi", "alias", "split")] + \
               [(k, C.c_void_p) for k in ("n", "start", "in_", "w", "bias", "resid", "out0", "out")]


def harness():
    """built once with make if it is missing; a missing library is an error, never a skip"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", V.PKG, "libtts_w2v_h_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        _lib = C.CDLL(LIB)
        _lib.tts_w2v_h_test_run.argtypes = [C.POINTER(CaseStruct)]
        assert _lib.tts_w2v_h_test_margin() == V.harness().tts_w2v_test_margin()  # w2v_cases.Guarded's margin
    return _lib


TM = 64  # the kernel's row tile (asserted against the harness in launch)
CASES = [  # (rows of the clips, gap: 0 = touching clips, cin: 64 one staging chunk | 192 three (an odd count on the two-slot ring), cout, epilogue, family)
    ([1], 8, 64, 64, BIAS, "gauss"), ([TM - 1], 8, 64, 64, GELU, "gauss"), ([TM], 0, 192, 64, RESID, "gauss"), ([TM + 1], 8, 64, 192, ALIAS, "gauss"),
    ([40, 70], 0, 192, 192, GELU, "gauss"),   # two touching clips, the first ends mid-tile
    ([5, 130], 8, 192, 64, ALIAS, "gauss"),   # a short clip beside a long one: a ragged grid
    ([40, 70], 0, 192, 192, BIAS, "exact"), ([5, 130], 8, 64, 192, ALIAS, "exact"), ([TM + 1], 8, 192, 64, GELU, "exact"), ([TM + 1], 8, 64, 64, RESID, "exact"),
    ([TM - 1], 8, 64, 64, BIAS, "clamp"),
]


def make(n, gap, cin, cout, epi, fam):
    rs = np.random.RandomState(sum(n) + cin + 3 * cout + len(epi))
    start, rows = V._layout(n, gap)
    live = np.zeros(rows, bool)
    for s0, k in zip(start, n):
        live[s0:s0 + k] = True
    if fam == "exact":
        x, w = rs.randint(-2, 3, (rows, cin)).astype(f32), (rs.randint(-2, 3, (cin, cout)) * np.ldexp(1.0, rs.randint(-3, 4, cout))[None]).astype(f32)
        bias, resid = rs.randint(-2, 3, cout).astype(f32), rs.randint(-4, 5, (rows, cout)).astype(f32)
    else:
        x, w = rs.randn(rows, cin).astype(f32), (rs.randn(cin, cout) / np.sqrt(cin) * 2).astype(f32)
        bias, resid = rs.randn(cout).astype(f32), rs.randn(rows, cout).astype(f32)
    if fam == "clamp":  # 1e5 and -1e5 on live rows: the operand is +-65504
        x[start[0] + 1, 3], x[start[0] + 2, 17] = 1.0e5, -1.0e5
    x[~live] = V.JUNK
    return dict(n=n, start=start, rows=rows, live=live, cin=cin, cout=cout, epi=epi, fam=fam, x=x, w=w, bias=bias, resid=resid)


def pair(v):
    """hi = rn_f16(v), lo = rn_f16(v - hi) of an f32 array (v - hi is exact in f32)"""
    v = np.asarray(v, f32)
    hi = v.astype(f16)
    return hi, (v - hi.astype(f32)).astype(f16)


def reference(c, split):
    m, E = np.abs(c["w"]).max(axis=0), harness().tts_w2v_h_test_scale_exp()
    s = np.ldexp(f32(1), E - np.where(m > 0, np.frexp(m)[1] - 1, E)).astype(f32)  # the column's largest |w| s lies in [2^12, 2^13)
    (xh, xl), (wh, wl) = pair(np.clip(c["x"], -65504, 65504)), pair(c["w"] * s[None, :])
    fams = [(xl, wh), (xh, wl), (xh, wh)] if split else [(xh, wh)]
    acc = sum(a.astype(f64) @ b.astype(f64) for a, b in fams) / s.astype(f64)
    mag = sum(np.abs(a.astype(f64)) @ np.abs(b.astype(f64)) for a, b in fams) / s.astype(f64) + np.abs(c["bias"].astype(f64))
    v = acc + c["bias"].astype(f64)
    resid = c["resid"].astype(f64) if c["epi"] in (RESID, ALIAS) else 0.0
    e_v = (2 * c["cin"] * len(fams) + (3 if c["epi"] in (RESID, ALIAS) else 2)) * V.U * (mag + np.abs(resid))
    if c["epi"] == GELU:
        y = V.gelu64(v)
        return y, V._e_gelu(v, y, e_v) + V.FMIN
    return v + resid, e_v + V.FMIN


def launch(c, split, x=None):
    L = harness()
    assert L.tts_w2v_h_test_row_tile() == TM
    out = V.Guarded((c["rows"], c["cout"]))
    keep = [np.array(c["n"], np.int32), np.array(c["start"], np.int32), c["x"] if x is None else x]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cs = CaseStruct(ns=len(c["n"]), rows=c["rows"], cin=c["cin"], cout=c["cout"], epi={BIAS: 0, GELU: 1}.get(c["epi"], 2), alias=int(c["epi"] == ALIAS), split=split,
                    n=p(keep[0]), start=p(keep[1]), in_=p(keep[2]), w=p(c["w"]), bias=p(c["bias"]), resid=p(c["resid"]), out0=p(c["resid"]), out=p(out.raw))
    rc = L.tts_w2v_h_test_run(C.byref(cs))
    if rc:  # a failed HIP call (a fault included) ends the session: nothing more is started on a GPU that may have faulted
        pytest.exit("w2v_linear_h %s: status %d" % (c["n"], rc), returncode=3)
    assert out.canaries_intact()
    return np.ascontiguousarray(out.payload).view(np.uint32)


@pytest.mark.parametrize("split", [0, 1], ids=["f16", "split"])
@pytest.mark.parametrize("case", CASES, ids=["n%s-g%d-cin%d-cout%d-%s-%s" % ("_".join(map(str, c[0])), c[1], c[2], c[3], c[4], c[5]) for c in CASES])
def test_linear_against_float64(case, split):
    c = make(*case)
    ref, bound = reference(c, split)
    bits = launch(c, split)
    got, live = bits.view(f32), c["live"]
    r = np.abs(got[live].astype(f64) - ref[live]) / bound[live]
    print("%s mode %d: worst |err| / bound %.4f" % (case, split + 1, r.max()))
    assert np.isfinite(got[live]).all() and r.max() <= 1.0
    if c["fam"] == "exact" and c["epi"] != GELU:
        assert np.array_equal(ref[live].astype(f32).astype(f64), ref[live]) and np.array_equal(got[live].astype(f64), ref[live])
    untouched = c["resid"].view(np.uint32) if c["epi"] == ALIAS else np.full_like(bits, V.SENTINEL * 0x01010101)
    assert np.array_equal(bits[~live], untouched[~live]), "a store left the live rows"
    assert np.array_equal(launch(c, split), bits), "two runs differ"
    poisoned = c["x"].copy()
    poisoned[~live] = np.nan
    assert np.array_equal(launch(c, split, poisoned), bits), "the launch read a row outside the clips"
