"""Shared by tests/test_ar_dec_kernels_gpu.py and tests/test_ar_dec_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/ar_dec_harness.hip -> libtts_dec_test.so), the weight layouts of the AR decode step restated as NumPy index arrays, the float64
reference of the two decode GEMV kernels, the case matrix and the error bounds.

    dec_ln_gemv_kernel      out = epilogue(LN(h) . Wf + cf)      K = 1024, LayerNorm (eps 1e-5, biased variance) folded into Wf / cf; the head runs two LayerNorms
    dec_gemv_resid_kernel   h += X . W + bias                     K = 1024 or 4096, N = 1024

The reference shares no code with the harness or the kernels. LAYOUTS are restated from the prose in front of the *_at maps in ar.hip as reshapes and transposes
(unpack()), never through those maps. The kernel reference works from the values a slab HOLDS, decoded exactly ((hi + lo) / 64, hi / 64, e4m3 x scale, f32), so the
quantisation of a weight mode is no part of any kernel's error.

ERROR BOUND of dec_ln_gemv_kernel (ln_expected()). First order, per output element, in float64 from the case's inputs; u = 2^-24. Nothing is fitted.
  LayerNorm (ln_stage). A row's sum passes <= 23 additions (2 inside a float4, 16 along the lane, 2 across the lane quarters, 3 across the waves):
      |d mean| <= dm = 23 u mean|x|.  d_k = x_k - mean: u |d_k| + dm.  sum d^2: the common shift dm enters in second order (sum d = 0): 1024 dm^2; the products and
      the 23 additions: 24 u; the rounding of d: 2 u: d var <= 26 u var + dm^2.  sc = 1 / sqrtf(var + 1e-5f): the addition, the correctly rounded sqrt and
      division, the float constant: 3 u + (d var + u eps) / (2 (var + eps)) =: rho. A row whose variance is far below eps keeps rho ~ 3 u, a row with
      mean = 100 std pays sc dm = 2300 u per element.  xhat_k: |xhat_k| (rho + u) + sc (u |d_k| + dm).
      The head's first LayerNorm multiplies by g and adds b (u |xhat g| + u |y|); its error e_in enters the second one as
      sc (e_in_k + mean e_in) + |xhat_k| sum_j |d_j| (e_in_j + mean e_in) / (1024 (var + eps)).
  Product. e_x reaches the output as sum_k e_x_k |W_kn|.
      SPLIT 0: the fp32 MFMA is a k-ordered fma chain, 64 per accumulator: 64 u; the 2 additions of the four chains.
      SPLIT 1-3: x = xh + xl with xl = fp16(x - xh). Per element: 2^-11 |xl| |wh| (the rounding of xl), |xl| |wl| (the dropped product), and where an fp16
      operand may be a SUBNORMAL (|.| < 2^-14) the whole product it enters: the matrix pipe may flush it (xl: min(|xl|, 2^-14) |wh|; likewise xh, wh, wl).
      The 256 exact products of a wave and accumulator are summed in an order the hardware does not document: charged as 256 additions of which each commits
      at most u of its partial sum (what a correctly rounded addition commits; an internally wider sum commits less): 256 u; the 2 additions of the three
      accumulators; x 1/64 and the power-of-two column scale are exact. These multiply S = sum_k |xhat_k| |W_kn|; the 3 additions across the waves and the
      bias multiply S + |cf_n|.
  Epilogue. QKV: an fp16 value is accepted iff it is the rounding of some number inside [ref - B, ref + B]. GELU: |gelu'| B, the argument's 7 roundings, the
      hardware exp2 and rcp at E2 = 1e-6 relative each (the figure ar.hip's comment is charged with in tests/ar_attn_cases.py), 3 roundings of the products;
      under lut the input is one of the fp16 neighbours of ref +- B and the output an fp16 rounding of gelu(input) +- 8 u (tanhf, the products).

ERROR BOUND of dec_gemv_resid_kernel (resid_expected()): a thread's K / NT fmas, 6 butterfly additions, NW - 1 across the waves, on sum |x||w|; the bias
addition and the residual addition one u of their results. Exact cases (integers whose every partial sum is below 2^24) must be bit-equal to the reference
rounded once.

SHARPNESS. DEFECTS are wrong formulas applied to the REFERENCE; tests/test_ar_dec_harness_cpu.py checks that each moves some output element of a case built to
expose it by >= 10 x that element's bound."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_DEC_TEST_LIB") or os.path.join(PKG, "libtts_dec_test.so")
SRC = os.path.join(PKG, "testlib", "ar_dec_harness.hip")

D, FF, V, VPAD = 1024, 4096, 8194, 8256
QKV, GELU, LOGITS = range(3)
EPI_NAMES = ["QKV", "GELU", "LOGITS"]
STRIP, MFMA16, MFMA16H, COLS4, SPLITW = range(5)
LAYOUT_NAMES = ["strip-major", "mfma16", "mfma16h", "cols4", "split [N][2K]"]
F32, SPLIT, F16, E4M3 = range(4)
ENC_NAMES = ["f32", "hi|lo", "fp16", "e4m3"]
SENTINEL = 0xCB
SENT16 = 0xCBCB
SENT32 = np.frombuffer(bytes([SENTINEL] * 4), np.float32)[0]
HIP_INVALID_VALUE = 1
U = 2.0 ** -24
E2 = 1e-6
EPS = 1e-5
SUB16 = 2.0 ** -14
C_MFMA16 = 256 * U + 2 * U   # SPLIT 1-3, see the module docstring
C_MFMA32 = 64 * U + 2 * U    # SPLIT 0
C_TAIL = 4 * U               # across the waves + bias

# the product's launches: dec_ln_gemv_kernel<EPI, SPLIT, NTW, HT, RO> (22) and dec_gemv_resid_kernel<KG, NT, WH, NTW, HT> (8)
LN_INSTANCES = sorted({(e, s, int(s in (1, 3)), 0, 0) for e in range(3) for s in (0, 1)} |
                      {(e, s, int(s in (1, 3)), 1, 0) for e in range(3) for s in range(4)} | {(QKV, s, int(s in (1, 3)), 1, 1) for s in range(4)})
RESID_INSTANCES = sorted({(kg, 0, 0, 0) for kg in (1, 4)} | {(kg, wh, int(wh == 0), 1) for kg in (1, 4) for wh in range(3)})
# layout x encoding x packer the loader builds (0 host, 1 device)
PACK_PAIRS = sorted([(STRIP, F32, 0), (STRIP, F32, 1), (MFMA16, F32, 0), (MFMA16H, SPLIT, 0), (MFMA16H, SPLIT, 1), (MFMA16H, F16, 0), (MFMA16H, E4M3, 0),
                     (COLS4, F32, 0), (COLS4, F32, 1), (COLS4, F16, 0), (COLS4, E4M3, 0), (SPLITW, SPLIT, 1)])
REACHED = {"ln": set(), "resid": set(), "pack": set()}  # what the GPU tests launched (test_coverage)


class PackStruct(C.Structure):
    _fields_ = [("K", C.c_int), ("N", C.c_int), ("layout", C.c_int), ("enc", C.c_int), ("where", C.c_int), ("transpose", C.c_int), ("vrows", C.c_int),
                ("W", C.c_void_p), ("g", C.c_void_p), ("b", C.c_void_p), ("c", C.c_void_p), ("slab_bytes", C.c_size_t), ("slab", C.c_void_p),
                ("fold", C.c_void_p), ("bias", C.c_void_p), ("scales", C.c_void_p), ("absmax", C.c_void_p)]


class LnStruct(C.Structure):
    _fields_ = [("epi", C.c_int), ("split", C.c_int), ("ntw", C.c_int), ("ht", C.c_int), ("ro", C.c_int),
                ("rows", C.c_int), ("N", C.c_int), ("n_valid", C.c_int), ("ldo", C.c_int), ("prefill_B", C.c_int), ("n_past", C.c_int), ("max_pos", C.c_int),
                ("n_slots", C.c_int), ("lut", C.c_int),
                ("h", C.c_void_p), ("g1", C.c_void_p), ("b1", C.c_void_p), ("slab", C.c_void_p), ("slab_bytes", C.c_size_t),
                ("bias", C.c_void_p), ("wscale", C.c_void_p), ("row_off", C.c_void_p), ("out", C.c_void_p), ("kc", C.c_void_p), ("vc", C.c_void_p)]


class ResidStruct(C.Structure):
    _fields_ = [("kg", C.c_int), ("wh", C.c_int), ("ntw", C.c_int), ("ht", C.c_int), ("rows", C.c_int),
                ("X", C.c_void_p), ("slab", C.c_void_p), ("slab_bytes", C.c_size_t), ("bias", C.c_void_p), ("wscale", C.c_void_p), ("h_in", C.c_void_p),
                ("h_out", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_dec_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_dec_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        for name, st in (("pack", PackStruct), ("ln_gemv", LnStruct), ("resid", ResidStruct)):
            for f in (getattr(L, "tts_dec_test_" + name), getattr(L, "tts_dec_test_%s_validate" % name)):
                f.argtypes, f.restype = [C.POINTER(st)], C.c_int
        L.tts_dec_test_margin.restype = C.c_int
        L.tts_dec_test_h4_index.argtypes, L.tts_dec_test_h4_index.restype = [C.c_int, C.c_int], C.c_size_t
        L.tts_dec_test_fp8.argtypes, L.tts_dec_test_fp8.restype = [C.c_float], C.c_uint8
        _lib = L
    return _lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, Guarded):
        a = a.raw
    return a.ctypes.data_as(C.c_void_p)


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation (or a host result) into."""

    def __init__(self, shape, dtype):
        self.margin = harness().tts_dec_test_margin()
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * self.dtype.itemsize, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def fill_struct(cs, **kw):
    keep = []
    for k, v in kw.items():
        if isinstance(v, (np.ndarray, Guarded)):
            keep.append(v)
            v = _ptr(v)
        setattr(cs, k, v)
    cs._keep = keep
    return cs


# ------------------------------------------------------------------------------------------------------------------------------------------ encodings

def e4m3_values():
    """The value of every e4m3 code (OCP: 1-4-3, bias 7, no infinities, 0x7f / 0xff NaN)."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e.astype(np.float64) - 7))
    v = np.where((c & 0x7f) == 0x7f, np.nan, v)
    return np.where(c >> 7, -v, v)


E4M3_TABLE = e4m3_values()


def e4m3_encode(x):
    """Round to nearest even, saturating, restated on the value table: the nearest of codes 0 .. 0x7e, a tie to the even code."""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    t = E4M3_TABLE[:0x7f]
    hi = np.clip(np.searchsorted(t, a, side="left"), 1, 0x7e)
    lo = hi - 1
    dl, dh = a - t[lo], t[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(a >= 448.0, 0x7e, code)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def fp8_scales(w):
    """One power of two per column: the smallest with max |w| / scale <= 448; 1 for a zero column."""
    amax = np.abs(np.asarray(w, np.float64)).max(axis=0)
    with np.errstate(divide="ignore"):
        e = np.ceil(np.log2(np.where(amax > 0, amax, 448.0) / 448.0))
    s = 2.0 ** e
    s = np.where(amax / s > 448.0, s * 2, s)               # (log2's rounding at an exact power of two)
    s = np.where((amax > 0) & (amax / (s / 2) <= 448.0), s / 2, s)
    return np.where(amax > 0, s, 1.0).astype(np.float32)


def split_hilo(w):
    v = np.float32(64.0) * np.asarray(w, np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


# ------------------------------------------------------------------------------------------------------------------------------------------ layouts
# Each function turns a slab (flat array of stored elements) into [K][N] order: a reshape and a transpose that touch every stored element once, so equality of
# the [K][N] views is equality of the slabs byte for byte.

def unpack(layout, enc, slab, K, N):
    """-> the stored elements in [K][N] order: f32; (hi, lo) fp16; fp16; or uint8 codes."""
    raw = np.ascontiguousarray(slab).view(np.uint8).reshape(-1)
    if layout == STRIP:  # 64-column strips [N / 64][K][64]
        return raw.view(np.float32).reshape(N // 64, K, 64).transpose(1, 0, 2).reshape(K, N)
    if layout == MFMA16:  # workgroup cb (16 columns): 4 waves x 16 groups x 64 lanes (q = lane / 16, m = lane % 16) x 4: k = 256 wv + 16 g + 4 q + j, n = 16 cb + m
        return raw.view(np.float32).reshape(N // 16, 4, 16, 4, 16, 4).transpose(1, 2, 3, 5, 0, 4).reshape(K, N)
    if layout == MFMA16H:  # element ((((cb 4 + wv) 8 + s) 64 + lane) 8 + e): k = 256 wv + 32 s + 8 q + e, n = 16 cb + m
        if enc == SPLIT:  # per lane and K step: 8 hi, then 8 lo
            a = raw.view(np.float16).reshape(N // 16, 4, 8, 4, 16, 2, 8).transpose(5, 1, 2, 3, 6, 0, 4).reshape(2, K, N)
            return a[0], a[1]
        if enc == F16:
            return raw.view(np.float16).reshape(N // 16, 4, 8, 4, 16, 8).transpose(1, 2, 3, 5, 0, 4).reshape(K, N)
        # e4m3: K steps 2 t and 2 t + 1 of a lane share 16 bytes: byte ((((cb 4 + wv) 4 + t) 64 + lane) 2 + (s & 1)) 8 + e
        return raw.reshape(N // 16, 4, 4, 4, 16, 2, 8).transpose(1, 2, 5, 3, 6, 0, 4).reshape(K, N)
    if layout == COLS4:  # workgroup cb (4 columns): KG x 4 (kk) x 256 threads x 4 columns: k = 1024 i + 4 t + kk
        dt = {F32: np.float32, F16: np.float16, E4M3: np.uint8}[enc]
        return raw.view(dt).reshape(N // 4, K // 1024, 4, 256, 4).transpose(1, 3, 2, 0, 4).reshape(K, N)
    if layout == SPLITW:  # [N][2 K]: hi (K) | lo (K) of 64 W^T
        a = raw.view(np.float16).reshape(N, 2, K).transpose(1, 2, 0)
        return a[0], a[1]
    raise ValueError(layout)


def encode(enc, w, scale64=True):
    """The stored elements of w [K][N] f32 under an encoding, in [K][N] order (what unpack() of a correct slab returns)."""
    w = np.asarray(w, np.float32)
    if enc == F32:
        return w
    if enc == SPLIT:
        return split_hilo(w)
    if enc == F16:
        return ((np.float32(64.0) * w) if scale64 else w).astype(np.float16)
    return e4m3_encode(w.astype(np.float64) / fp8_scales(w).astype(np.float64))


def decode(enc, stored, scales=None, scale64=True):
    """The float64 value of every stored element: what the kernel multiplies with."""
    if enc == F32:
        return stored.astype(np.float64)
    if enc == SPLIT:
        return (stored[0].astype(np.float64) + stored[1].astype(np.float64)) / 64.0
    if enc == F16:
        return stored.astype(np.float64) / (64.0 if scale64 else 1.0)
    return E4M3_TABLE[stored] * np.asarray(scales, np.float64)


def h4_index(r, k):
    """h4[r / 16][k / 4][r % 16][k % 4] as a flat index (arrays broadcast)."""
    r, k = np.asarray(r), np.asarray(k)
    return (((r // 16) * 256 + k // 4) * 16 + r % 16) * 4 + k % 4


def from_h4(buf, rows):
    """[rows][1024] from an h4 buffer of whole tiles, and the padding rows' elements."""
    tiles = (rows + 15) // 16
    a = np.asarray(buf).reshape(tiles, 256, 16, 4).transpose(0, 2, 1, 3).reshape(tiles * 16, D)
    return a[:rows], a[rows:]


def fold_ref(w, g, b, c):
    """-> float32(g w) and the bias float(double(c) + sum_k double(b_k) double(w_kn)), k ascending."""
    wf = (np.asarray(g, np.float32)[:, None] * np.asarray(w, np.float32)).astype(np.float32)
    acc = np.zeros(w.shape[1], np.float64)
    w64, b64 = np.asarray(w, np.float64), np.asarray(b, np.float64)
    for k in range(w.shape[0]):  # ascending k: the order is part of the statement
        acc += b64[k] * w64[k]
    return wf, (np.asarray(c, np.float64) + acc).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------------ harness calls

def slab_bytes(K, N, layout, enc):
    n = K * N
    if layout == SPLITW:
        return n * 4
    return n * {F32: 4, SPLIT: 4, F16: 2, E4M3: 1}[enc]


class Packed(object):
    pass


def pack(w, layout, enc, where=0, g=None, b=None, c=None, transpose_vrows=0, N=None, want_fold=True):
    """One pack call. w [K][N] f32 (transpose_vrows: [vrows][K], N the padded width). -> Packed: slab (uint8), stored ([K][N] view), fold, bias, scales, absmax."""
    w = _f32(w)
    if transpose_vrows:
        K = w.shape[1]
    else:
        K, N = w.shape
    p = Packed()
    p.K, p.N, p.layout, p.enc, p.where = K, N, layout, enc, where
    nb = slab_bytes(K, N, layout, enc)
    slab = Guarded((nb,), np.uint8)
    fold = Guarded((K, N), np.float32) if want_fold and (where == 0 or g is not None or transpose_vrows) else None
    bias = Guarded((N,), np.float32) if g is not None else None
    scales = Guarded((N,), np.float32) if where == 0 else None
    absmax = Guarded((1,), np.float32) if where == 1 else None
    cs = fill_struct(PackStruct(), K=K, N=N, layout=layout, enc=enc, where=where, transpose=int(bool(transpose_vrows)), vrows=transpose_vrows, W=w, g=_f32(g),
                     b=_f32(b), c=_f32(c), slab_bytes=nb, slab=slab, fold=fold, bias=bias, scales=scales, absmax=absmax)
    rc = harness().tts_dec_test_pack(C.byref(cs))
    assert rc == 0, "pack returned %d" % rc
    for name, gb in (("slab", slab), ("fold", fold), ("bias", bias), ("scales", scales), ("absmax", absmax)):
        assert gb is None or gb.canaries_intact(), "a packer wrote outside its %s buffer" % name
        setattr(p, name, None if gb is None else gb.payload)
    p.stored = unpack(layout, enc, p.slab, K, N)
    REACHED["pack"].add((layout, enc, where))
    return p


class LnOut(object):
    pass


def run_ln(epi, split, ht, ro, h, slab, bias, N, wscale=None, g1=None, b1=None, n_valid=None, ldo=None, prefill_B=0, n_past=0, max_pos=1, n_slots=1, lut=0,
           row_off=None, validate_only=False):
    rows = h.shape[0]
    n_valid = N if n_valid is None else n_valid
    ldo = (D if epi == QKV else N) if ldo is None else ldo
    out = Guarded((rows, FF if epi == GELU else ldo), np.float32)
    kc = Guarded((n_slots, max_pos, D), np.uint16) if epi == QKV else None
    vc = Guarded((n_slots, max_pos, D), np.uint16) if epi == QKV else None
    slab = np.ascontiguousarray(slab).view(np.uint8).reshape(-1)
    cs = fill_struct(LnStruct(), epi=epi, split=split, ntw=int(split in (1, 3)), ht=ht, ro=ro, rows=rows, N=N, n_valid=n_valid, ldo=ldo, prefill_B=prefill_B,
                     n_past=n_past, max_pos=max_pos, n_slots=n_slots, lut=lut, h=_f32(h), g1=_f32(g1), b1=_f32(b1), slab=slab, slab_bytes=slab.nbytes,
                     bias=_f32(bias), wscale=_f32(wscale), row_off=None if row_off is None else np.ascontiguousarray(row_off, np.int32), out=out, kc=kc, vc=vc)
    if validate_only:
        return cs
    rc = harness().tts_dec_test_ln_gemv(C.byref(cs))
    assert rc == 0, "harness returned %d" % rc
    o = LnOut()
    for name, gb in (("out", out), ("kc", kc), ("vc", vc)):
        assert gb is None or gb.canaries_intact(), "dec_ln_gemv_kernel wrote outside its %s buffer" % name
        setattr(o, name, None if gb is None else gb.payload)
    REACHED["ln"].add((epi, split, int(split in (1, 3)), ht, ro))
    return o


def run_resid(kg, wh, ht, X, slab, bias, h_in, wscale=None, validate_only=False, ntw=None):
    rows = h_in.shape[0]
    tiles = (rows + 15) // 16
    h_out = Guarded((tiles * 16 if ht else rows, D), np.float32)
    slab = np.ascontiguousarray(slab).view(np.uint8).reshape(-1)
    ntw = int(ht and wh == 0) if ntw is None else ntw
    cs = fill_struct(ResidStruct(), kg=kg, wh=wh, ntw=ntw, ht=ht, rows=rows, X=_f32(X), slab=slab, slab_bytes=slab.nbytes, bias=_f32(bias),
                     wscale=_f32(wscale), h_in=_f32(h_in), h_out=h_out)
    if validate_only:
        return cs
    rc = harness().tts_dec_test_resid(C.byref(cs))
    assert rc == 0, "harness returned %d" % rc
    assert h_out.canaries_intact(), "dec_gemv_resid_kernel wrote outside h"
    REACHED["resid"].add((kg, wh, ntw, ht))
    if not ht:
        return h_out.payload
    out, pad = from_h4(h_out.payload, rows)
    assert np.isnan(pad).all() and (pad.view(np.uint32) == np.float32(np.nan).view(np.uint32)).all(), "a padding row of the last tile was stored"
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------ inputs

FAMILIES = ["gauss", "mean100", "const", "outlier", "tiny", "huge"]
OUTLIER_AT = [0, 255, 256, 1023, 31, 32]  # the wave edges and a 32-wide K-step edge
ROW_COUNTS = [1, 15, 16, 17, 19, 32]
# (rows, rot): every row count, every family in slot 0 (rot 0 .. 5) and in slot 15 (rot 0 .. 5 at >= 16 rows)
ROW_CASES = list(zip(ROW_COUNTS, range(6))) + [(16, 0), (32, 1)]
CONST = 3.25  # short mantissa: a sum of 1024 copies is exact, so xhat = 0 exactly


def family_of(r, rot):
    return FAMILIES[(r % 16 + rot) % 6]


def make_rows(rows, rot, seed=0):
    """[rows][1024] f32: slot s of every tile carries family (s + rot) % 6, so over rot = 0 .. 5 every family sits in slots 0 and 15."""
    rs = np.random.RandomState(1000 + 17 * seed + rot)
    h = np.empty((rows, D), np.float32)
    for r in range(rows):
        f = family_of(r, rot)
        z = rs.randn(D) if r % 2 == 0 else rs.standard_t(3, D)  # every other row heavy-tailed
        if f == "gauss":
            x = z
        elif f == "mean100":
            x = 100.0 + rs.randn(D)
        elif f == "const":
            x = np.full(D, CONST)
        elif f == "outlier":  # xhat ~ -0.03 on 1023 channels, 32 on one
            x = np.full(D, 0.5)
            x[OUTLIER_AT[r % 6]] = 1000.5
        elif f == "tiny":
            x = 1e-4 * z  # variance << eps
        else:
            x = 1e4 * z
        h[r] = x.astype(np.float32)
    return h


@functools.lru_cache(maxsize=None)
def make_weights(N, seed=0, fp8_cols=False, kind="real"):
    """w [1024][N] f32 (sigma 0.02), LayerNorm gain g (up to 12) and offset b, bias c. Special columns, repeated in every 1024-column section and at the end:
    +0 a 30 sigma column, +1 one entry that puts max |g w| just under the range guard (937.5), +2 |w| ~ 1e-5 (subnormal lo parts), +3 all zero,
    +4 / +5 (fp8_cols) largest entry exactly 448 x 2^-12 and the next float above it."""
    rs = np.random.RandomState(7 + seed + N)
    if kind == "exact":  # e4m3 values times a power of two per column (neighbours differ), the column's largest entry 448 x 2^e: every encoding holds them exactly
        w = E4M3_TABLE[rs.randint(0, 0x7f, (D, N)) | (rs.randint(0, 2, (D, N)) << 7)]
        w[0] = 448.0
        w = (w * 2.0 ** (-8.0 - np.arange(N) % 3)).astype(np.float32)
        c = (0.1 * rs.randn(N)).astype(np.float32)
        w.setflags(write=False)
        return w, None, None, c
    w = (0.02 * rs.randn(D, N)).astype(np.float32)
    g = rs.uniform(0.5, 2.0, D).astype(np.float32)
    g[rs.choice(D, 8, replace=False)] = 12.0
    g[5] = 1.0  # the row of the entries whose folded value is set exactly
    b = (0.1 * rs.randn(D)).astype(np.float32)
    c = (0.1 * rs.randn(N)).astype(np.float32)
    for base in sorted(set(list(range(0, N - 16, 1024)) + [N - 16])):
        w[:, base] *= 30.0
        w[5, base + 1] = 937.0
        w[:, base + 2] = (1e-5 * rs.randn(D)).astype(np.float32)
        w[:, base + 3] = 0.0
        if fp8_cols:
            for j, top in ((4, np.float32(448.0 * 2.0 ** -12)), (5, np.nextafter(np.float32(448.0 * 2.0 ** -12), np.float32(1.0)))):
                w[:, base + j] = np.clip(w[:, base + j], -0.005, 0.005)  # x 12 stays below the top entry
                w[5, base + j] = top
    for a in (w, g, b, c):
        a.setflags(write=False)
    return w, g, b, c


SPLIT_ENC = {0: (MFMA16, F32), 1: (MFMA16H, SPLIT), 2: (MFMA16H, F16), 3: (MFMA16H, E4M3)}
WH_ENC = {0: F32, 1: F16, 2: E4M3}


class Slab(object):
    """A packed matrix with what the reference needs: wdec [K][N] float64 (the values the slab holds), hi / lo parts in units of 1 (not 64), scales."""


@functools.lru_cache(maxsize=10)
def ln_slab(N, split, seed=0, kind="real"):
    """The decode slab of make_weights(N) for SPLIT, built by the product's HOST packers (no GPU), and its exact decoding."""
    w, g, b, c = make_weights(N, seed, True, kind)
    layout, enc = SPLIT_ENC[split]
    p = pack(w, layout, enc, 0, g, b, c if g is not None else None, want_fold=False)
    return slab_of(p, c)


def slab_of(p, bias=None):
    s = Slab()
    s.p, s.N, s.enc = p, p.N, p.enc
    s.slab = p.slab
    s.bias = p.bias if p.bias is not None else np.asarray(bias, np.float32)
    s.scales = p.scales if p.enc == E4M3 else None
    cols4 = p.layout == COLS4
    s.wdec = decode(p.enc, p.stored, s.scales, scale64=not cols4)
    if p.enc == SPLIT:
        s.wh, s.wl = p.stored[0].astype(np.float64) / 64, p.stored[1].astype(np.float64) / 64
    else:
        s.wh, s.wl = s.wdec, None
    return s


# ------------------------------------------------------------------------------------------------------------------------------------------ reference: LayerNorm

def ln_stage(x, e_in=None, g=None, b=None, eps=EPS, unbiased=False):
    with np.errstate(divide="ignore", invalid="ignore"):  # (a mutated reference may divide by a zero variance)
        return _ln_stage(x, e_in, g, b, eps, unbiased)


def _ln_stage(x, e_in, g, b, eps, unbiased):
    """One LayerNorm of rows x [R][1024] float64 -> (y, e): the exact result and the first-order bound of the kernel's held value (module docstring)."""
    K = x.shape[1]
    mean = x.mean(axis=1, keepdims=True)
    d = x - mean
    var = (d * d).sum(axis=1, keepdims=True) / (K - 1 if unbiased else K)
    sc = 1.0 / np.sqrt(var + eps)
    xhat = d * sc
    dm = 23 * U * np.abs(x).mean(axis=1, keepdims=True)
    dvar = 26 * U * var + dm * dm
    rho = 3 * U + (dvar + U * eps) / (2 * (var + eps))
    e = np.abs(xhat) * (rho + U) + sc * (U * np.abs(d) + dm)
    if e_in is not None:
        dd = e_in + e_in.mean(axis=1, keepdims=True)
        e = e + sc * dd + np.abs(xhat) * (np.abs(d) * dd).sum(axis=1, keepdims=True) / (K * (var + eps))
    if g is None:
        return xhat, e
    y = xhat * g + b
    return y, e * np.abs(g) + U * np.abs(xhat * g) + U * np.abs(y)


def f16_interval_ok(v16, ref, B):
    """v16 (float16 array) is the fp16 rounding of some number inside [ref - B, ref + B]."""
    with np.errstate(over="ignore"):
        lo, hi = (ref - B).astype(np.float16), (ref + B).astype(np.float16)
    v = v16.astype(np.float64)
    return (v >= lo.astype(np.float64)) & (v <= hi.astype(np.float64))


S_GELU, A_GELU = 0.79788456080286535587989211986876, 0.044715
X0_GELU = -0.75179  # where tanh-GELU has its minimum


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(S_GELU * x * (1.0 + A_GELU * x * x)))


def gelu_erf(x):
    from math import erf
    return 0.5 * x * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))


def gelu_bound(x, B):
    """|gelu'(x)| B + the kernel's own evaluation error at lut = 0."""
    t = S_GELU * x * (1.0 + A_GELU * x * x)
    th = np.tanh(t)
    dg = 0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * S_GELU * (1.0 + 3 * A_GELU * x * x)
    with np.errstate(over="ignore"):
        E = np.exp(np.minimum(2 * t, 700.0))
    r = 1.0 / (1.0 + E)
    dth = 2 * E * r * r * (E2 + 7 * U * np.abs(2 * t)) + 2 * r * (E2 + U) + U
    return np.abs(dg) * B + 0.5 * np.abs(x) * (dth + U * (1.0 + th)) + 2 * U * np.abs(gelu_tanh(x))


class LnCase(object):
    """One launch of dec_ln_gemv_kernel: inputs and launch parameters (run_case() launches it, ln_expected() is its reference)."""

    def __init__(self, epi, split, ht, h, slab, ro=0, g1=None, b1=None, n_valid=None, ldo=None, prefill_B=0, n_past=0, max_pos=4, n_slots=None, lut=0, row_off=None,
                 tag=""):
        self.epi, self.split, self.ht, self.ro, self.h, self.slab, self.g1, self.b1 = epi, split, ht, ro, h, slab, g1, b1
        self.N = slab.N
        self.rows = h.shape[0]
        self.n_valid = self.N if n_valid is None else n_valid
        self.ldo = (D if epi == QKV else self.N) if ldo is None else ldo
        self.prefill_B, self.n_past, self.max_pos, self.lut, self.tag = prefill_B, n_past, max_pos, lut, tag
        self.n_slots = (self.rows if prefill_B == 0 else prefill_B) if n_slots is None else n_slots
        tiles = (self.rows + 15) // 16
        self.row_off = np.zeros(tiles * 16, np.int32) if row_off is None else np.asarray(row_off, np.int32)

    def run(self):
        return run_ln(self.epi, self.split, self.ht, self.ro, self.h, self.slab.slab, self.slab.bias, self.N, self.slab.scales, self.g1, self.b1, self.n_valid,
                      self.ldo, self.prefill_B, self.n_past, self.max_pos, self.n_slots, self.lut, self.row_off if self.ro else None)


DEFECTS_LN = ["eps_dropped", "eps_wrong", "unbiased_var", "one_ln_head", "lohi_dropped", "hilo_dropped", "fp8_neighbour_scale", "kv_late", "row_off_ignored",
              "kv_swapped", "q_unrounded", "erf_gelu", "wrong_lut", "drop_last_valid", "store_n_valid"]
DEFECTS_FOLD = ["gain_not_folded", "bW_missing"]
DEFECTS_RESID = ["last_kgroup_dropped", "cols_swapped", "cand_mirror", "bias_twice", "resid_dropped"]


class Expected(object):
    pass


def ln_expected(c, defect=None):
    """The float64 reference of a case and the bound of every element: ref / B [rows][N] before the epilogue, plus what the epilogue must store where."""
    s = c.slab
    x = c.h.astype(np.float64)
    eps = {"eps_dropped": 0.0, "eps_wrong": 1e-6}.get(defect, EPS)
    unb = defect == "unbiased_var"
    e = None
    if c.epi == LOGITS and defect != "one_ln_head":
        x, e = ln_stage(x, None, c.g1.astype(np.float64), c.b1.astype(np.float64), eps, unb)
    elif c.epi == LOGITS:  # the defect: ln_f's affine part applied to the raw rows
        x = x * c.g1.astype(np.float64) + c.b1.astype(np.float64)
    xhat, ex = ln_stage(x, e, None, None, eps, unb)
    W, bias = s.wdec, s.bias.astype(np.float64)
    aW = np.abs(W)
    S = np.abs(xhat) @ aW
    T = S + np.abs(bias)
    B = ex @ aW
    if c.split == 0:
        ref = xhat @ W + bias
        B = B + C_MFMA32 * S + C_TAIL * T
    else:
        x32 = xhat.astype(np.float32)
        xh = x32.astype(np.float16).astype(np.float64)
        xl = x32.astype(np.float64) - xh
        sc = np.ones(c.N) if s.scales is None else s.scales.astype(np.float64)
        if defect == "fp8_neighbour_scale":
            sc = np.roll(sc, 1)
        wh = s.wh if s.scales is None else E4M3_TABLE[s.p.stored]  # the fp16 operand of the matrix pipe, in units of 1 (x 64 inside the kernel)
        unit = 1.0 / 64 if s.scales is None else 1.0            # what one unit of an fp16 WEIGHT operand's subnormal threshold is worth
        awh = np.abs(wh)
        awl = np.zeros_like(awh) if s.wl is None else np.abs(s.wl)
        if defect in ("lohi_dropped", "hilo_dropped"):
            part = (xh @ s.wl) if defect == "lohi_dropped" else (xl @ s.wh)
            ref = xhat @ W + bias - part
        else:
            ref = (xhat @ wh) * sc + bias if s.scales is not None else xhat @ W + bias
        axl, axh = np.abs(xl), np.abs(xh)
        may_sub = (axl - ex) < SUB16
        e_xl = np.where(may_sub, np.minimum(axl + ex, SUB16), 2.0 ** -11 * (axl + ex))
        xh_sub = np.where(axh < SUB16 * 1.01, axh, 0.0)
        wh_sub = np.where(awh < SUB16 * unit, awh, 0.0)
        wl_sub = np.where(awl < SUB16 * unit, awl, 0.0)
        Bs = e_xl @ awh + axl @ awl + xh_sub @ (awh + awl) + (axh + axl) @ wh_sub + axh @ wl_sub
        B = B + Bs * sc + C_MFMA16 * S + C_TAIL * T
    r = Expected()
    r.c, r.defect, r.xhat, r.S, r.ref, r.B = c, defect, xhat, S, ref, B
    return r


def ln_render(r):
    """The buffers a kernel that computes r.ref exactly would leave: (out, kc, vc) with the sentinel everywhere else."""
    c, d = r.c, r.defect
    out = np.full((c.rows, FF if c.epi == GELU else c.ldo), SENT32, np.float32)
    if c.epi == GELU:
        lut = c.lut if d != "wrong_lut" else 1 - c.lut
        v = r.ref
        if lut:
            v = v.astype(np.float32).astype(np.float16).astype(np.float64)
        y = gelu_erf(v) if d == "erf_gelu" else gelu_tanh(v)
        out[:] = (y.astype(np.float16) if lut else y).astype(np.float32)
        return out, None, None
    if c.epi == LOGITS:
        nv = c.n_valid + (1 if d == "store_n_valid" else 0)
        out[:, :nv] = r.ref[:, :nv].astype(np.float32)
        if d == "drop_last_valid":
            out[:, c.n_valid - 1] = SENT32
        return out, None, None
    v16 = r.ref.astype(np.float16)
    out[:, :D] = r.ref[:, :D].astype(np.float32) if d == "q_unrounded" else v16[:, :D].astype(np.float32)
    kc = np.full((c.n_slots, c.max_pos, D), SENT16, np.uint16)
    vc = kc.copy()
    k16, v_16 = v16[:, D:2 * D].view(np.uint16), v16[:, 2 * D:].view(np.uint16)
    if d == "kv_swapped":
        k16, v_16 = v_16, k16
    for slot, pos, row in kv_targets(c, d):
        kc[slot, pos], vc[slot, pos] = k16[row], v_16[row]
    return out, kc, vc


def kv_targets(c, defect=None):
    """(slot, position, row) of every K/V store."""
    if c.prefill_B > 0:
        return [(s, r, r) for s in range(c.prefill_B) for r in range(c.rows)]
    t = []
    for r in range(c.rows):
        pos = c.n_past + (int(c.row_off[r]) if c.ro and defect != "row_off_ignored" else 0) + (1 if defect == "kv_late" else 0)
        t.append((r, pos % c.max_pos if defect else pos, r))
    return t


def ln_check(r, out, kc=None, vc=None):
    """The largest |error| / bound over the elements of a launch's buffers against the UNMUTATED expectation r; inf where a store is missing, misplaced or a value
    outside its rounding interval. -> (ratio, detail)."""
    c = r.c
    assert r.defect is None
    worst, what = 0.0, ""

    def fail(msg):
        return np.inf, msg

    if c.epi == GELU:
        if c.lut:
            lo16, hi16 = (r.ref - r.B).astype(np.float16), (r.ref + r.B).astype(np.float16)
            o16 = out.astype(np.float16)
            if not (o16.astype(np.float32) == out).all():
                return fail("ff holds a value that is no fp16 number")
            # the input is an fp16 number in [lo16, hi16]: gelu over that interval lies between its end values, and its minimum at x0 = -0.7518 if inside
            xl_, xh_ = lo16.astype(np.float64), hi16.astype(np.float64)
            ya, yb = gelu_tanh(xl_), gelu_tanh(xh_)
            y_lo = np.where((xl_ < X0_GELU) & (xh_ > X0_GELU), gelu_tanh(X0_GELU), np.minimum(ya, yb))
            y_hi = np.maximum(ya, yb)
            tol = 8 * U * (np.maximum(np.abs(ya), np.abs(yb)) + np.maximum(np.abs(xl_), np.abs(xh_)))
            with np.errstate(over="ignore"):
                ok = (o16.astype(np.float64) >= (y_lo - tol).astype(np.float16).astype(np.float64)) & (o16.astype(np.float64) <= (y_hi + tol).astype(np.float16).astype(np.float64))
            if not ok.all():
                i = np.argwhere(~ok)[0]
                return fail("ff[%d][%d] = %r is not gelu of an fp16 number within the bound of %r" % (i[0], i[1], out[i[0], i[1]], r.ref[i[0], i[1]]))
            return 0.0, "lut: every element inside its fp16 interval"
        with np.errstate(divide="ignore", invalid="ignore"):  # (0 / 0 on an all-zero column with a zero bias: exact, no figure)
            ratio = np.abs(out.astype(np.float64) - gelu_tanh(r.ref)) / gelu_bound(r.ref, r.B)
        return float(np.nanmax(np.where(np.isfinite(out), ratio, np.inf))), "gelu"
    if c.epi == LOGITS:
        if not (out[:, c.n_valid:].view(np.uint32) == SENT32.view(np.uint32)).all():
            return fail("a column >= n_valid was stored")
        o = out[:, :c.n_valid]
        if (o.view(np.uint32) == SENT32.view(np.uint32)).any() or not np.isfinite(o).all():
            return fail("a column < n_valid was not stored")
        ratio = np.abs(o.astype(np.float64) - r.ref[:, :c.n_valid]) / r.B[:, :c.n_valid]
        return float(ratio.max()), "logits"
    # QKV
    if not (out[:, D:].view(np.uint32) == SENT32.view(np.uint32)).all():
        return fail("q was written past column 1023")
    q = out[:, :D]
    if not np.isfinite(q).all() or not (q.astype(np.float16).astype(np.float32) == q).all():
        return fail("q holds a value that is no fp16 number")
    if not f16_interval_ok(q.astype(np.float16), r.ref[:, :D], r.B[:, :D]).all():
        return fail("a q element is outside its rounding interval")
    seen = np.zeros(kc.shape[:2], bool)
    for slot, pos, row in kv_targets(c):
        seen[slot, pos] = True
        for name, cache, sec in (("K", kc, 1), ("V", vc, 2)):
            if not f16_interval_ok(cache[slot, pos].view(np.float16), r.ref[row, sec * D:(sec + 1) * D], r.B[row, sec * D:(sec + 1) * D]).all():
                return fail("%s of row %d at slot %d position %d is outside its rounding interval" % (name, row, slot, pos))
    for name, cache in (("K", kc), ("V", vc)):
        if not (cache[~seen] == SENT16).all():
            return fail("a %s cache row that is no target was written" % name)
    # (the fp16 rounding hides the pre-rounding value: the figure reported is the distance of the stored value in units of bound + half an fp16 ulp)
    full = np.concatenate([q.astype(np.float64)] + [np.stack([cache[s_, p_].view(np.float16).astype(np.float64) for s_, p_, _ in kv_targets(c)[:c.rows]])
                                                    for cache in (kc, vc)], axis=1)
    half_ulp = np.maximum(np.abs(r.ref), 2.0 ** -14) * 2.0 ** -11
    return float((np.abs(full - r.ref) / (r.B + half_ulp)).max()), "qkv"


def ln_defect_ratio(c, defect):
    """How far the buffers of the mutated reference lie from the expectation, in bounds."""
    return ln_check(ln_expected(c), *ln_render(ln_expected(c, defect)))[0]


def split_units(r, out, cols=None):
    """The error in the unit of the "2^-22 relative" statement: per row, max over the columns of |out - ref| / (2^-22 sum_k |xhat_k||w_kn|) (head cases)."""
    cols = np.arange(r.c.n_valid) if cols is None else cols
    S = r.S[:, cols]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(out[:, cols].astype(np.float64) - r.ref[:, cols]) / (2.0 ** -22 * S)
    return np.nanmax(np.where(S > 0, q, 0.0), axis=1)


@functools.lru_cache(maxsize=None)
def identity_slab(split):
    """W = I (N = 1024), bias 0: the head's output is then the operand the product stage was handed. SPLIT 0: xhat as the kernel's LayerNorm left it (x 1 and + 0
    are exact); SPLIT 1: xh + xl with xl = fp16(xhat - xh) as it reached the matrix pipe (64 xh + 64 xl fits 24 bits), so a flushed subnormal xl shows as xl = 0."""
    return custom_slab(np.eye(D, dtype=np.float32), np.zeros(D, np.float32), split)


def split_only_expected(c, y):
    """The split product ALONE: reference and bound of a SPLIT 1-3 head launch given y [rows][1024], the operand values xh + xl the kernel multiplied (an
    identity_slab(1) launch on the same rows). No LayerNorm term and no rounding of xl: the dropped lo . lo product, the subnormal operands the pipe may
    flush, and the accumulation."""
    s = c.slab
    y = y.astype(np.float64)
    xh = y.astype(np.float16).astype(np.float64)
    xl = y - xh
    sc = np.ones(c.N) if s.scales is None else s.scales.astype(np.float64)
    wh = s.wh if s.scales is None else E4M3_TABLE[s.p.stored]
    unit = 1.0 / 64 if s.scales is None else 1.0
    awh = np.abs(wh)
    awl = np.zeros_like(awh) if s.wl is None else np.abs(s.wl)
    axl, axh = np.abs(xl), np.abs(xh)
    bias = s.bias.astype(np.float64)
    r = Expected()
    r.c, r.defect, r.xhat = c, None, y
    r.S = np.abs(y) @ np.abs(s.wdec)
    r.ref = (y @ wh) * sc + bias if s.scales is not None else y @ s.wdec + bias
    sub = lambda a, lim: np.where(a < lim, a, 0.0)
    Bs = axl @ awl + sub(axl, SUB16) @ awh + sub(axh, SUB16) @ (awh + awl) + (axh + axl) @ sub(awh, SUB16 * unit) + axh @ sub(awl, SUB16 * unit)
    r.B = Bs * sc + C_MFMA16 * r.S + C_TAIL * (r.S + np.abs(bias))
    return r


def head_affine(seed=3):
    """ln_f's gain and offset of the head cases: not the identity."""
    rs = np.random.RandomState(seed)
    return rs.uniform(0.5, 2.0, D).astype(np.float32), (0.1 * rs.randn(D)).astype(np.float32)


def custom_slab(w, c, split, g=None, b=None):
    """A slab of a matrix of the test's own through the host packer."""
    layout, enc = SPLIT_ENC[split]
    return slab_of(pack(w, layout, enc, 0, g, b, c if g is not None else None, want_fold=False), c)


def ln_case(epi, split, ht, rows, rot=0, N=64, kind="real", **kw):
    """A case of the matrix: make_rows(rows, rot) on the slab of make_weights(N) (QKV: 3072, GELU: 4096, LOGITS: N)."""
    N = {QKV: 3 * D, GELU: FF}.get(epi, N)
    if epi == LOGITS:
        kw.setdefault("g1", head_affine()[0])
        kw.setdefault("b1", head_affine()[1])
    return LnCase(epi, split, ht, make_rows(rows, rot), ln_slab(N, split, 0, kind), tag="%s split %d ht %d rows %d rot %d" % (EPI_NAMES[epi], split, ht, rows, rot), **kw)


# ---- an f32 restatement of the kernel's arithmetic (NumPy float32, its own summation order): what the bound must admit. flush: fp16 subnormal operands become 0.

def _ln32(x, g=None, b=None):
    f = np.float32
    mean = x.sum(axis=1, keepdims=True, dtype=f) * f(1.0 / D)
    d = x - mean
    var = (d * d).sum(axis=1, keepdims=True, dtype=f) * f(1.0 / D)
    y = d * (f(1.0) / np.sqrt(var + f(1e-5)))
    return y if g is None else y * g + b


def _flush16(a):
    return np.where(np.abs(a.astype(np.float32)) < np.float32(SUB16), np.float16(0), a)


def emulate_ln(c, flush=False):
    """-> (out, kc, vc) as a kernel of plain float32 / fp16 arithmetic would leave them."""
    f = np.float32
    s = c.slab
    x = c.h.astype(f)
    if c.epi == LOGITS:
        x = _ln32(x, c.g1, c.b1)
    x = _ln32(x)
    if c.split == 0:
        v = x @ s.wdec.astype(f) + s.bias
    else:
        xh = x.astype(np.float16)
        xl = (x - xh.astype(f)).astype(np.float16)
        wh = (s.p.stored[0] if c.split == 1 else s.p.stored if c.split == 2 else E4M3_TABLE[s.p.stored].astype(np.float16))
        wl = s.p.stored[1] if c.split == 1 else None
        if flush:
            xh, xl, wh = _flush16(xh), _flush16(xl), _flush16(wh)
            wl = None if wl is None else _flush16(wl)
        a0, a2 = xh.astype(f) @ wh.astype(f), xl.astype(f) @ wh.astype(f)
        if c.split == 3:
            v = (a2 + a0) * s.scales + s.bias
        else:
            a1 = xh.astype(f) @ wl.astype(f) if wl is not None else f(0)
            v = ((a1 + a2) + a0) * f(1.0 / 64) + s.bias
    r = Expected()
    r.c, r.defect, r.ref = c, None, v.astype(np.float64)
    if c.epi == GELU and not c.lut:  # the float32 formula of the source, with this library's exp2
        u_ = f(S_GELU) * v * (f(1) + f(A_GELU) * v * v)
        with np.errstate(over="ignore"):
            th = f(1) - f(2) / (f(1) + np.exp2(u_ * f(2.88539008177793)))
        return (f(0.5) * v * (f(1) + th)).astype(f), None, None
    return ln_render(r)


def emulate_resid(c):
    f = np.float32
    s = c.slab
    t = c.X.astype(f) @ s.wdec.astype(f) if s.scales is None else (c.X.astype(f) @ E4M3_TABLE[s.p.stored].astype(f)) * s.scales
    return c.h_in + (t + s.bias)


# ------------------------------------------------------------------------------------------------------------------------------------------ reference: projection

class ResidCase(object):
    def __init__(self, kg, wh, ht, X, slab, h_in, tag="", exact=False):
        self.kg, self.wh, self.ht, self.X, self.slab, self.h_in, self.tag, self.exact = kg, wh, ht, X, slab, h_in, tag, exact
        self.rows = h_in.shape[0]

    def run(self):
        return run_resid(self.kg, self.wh, self.ht, self.X, self.slab.slab, self.slab.bias, self.h_in, self.slab.scales)


def resid_expected(c, defect=None):
    s = c.slab
    X, W = c.X.astype(np.float64), s.wdec
    bias, h = s.bias.astype(np.float64), c.h_in.astype(np.float64)
    K = 1024 * c.kg
    NT = 256 if c.kg == 1 else 512
    if defect == "last_kgroup_dropped":  # the last K group of NT * 4 values
        X = X.copy()
        X[:, K - NT * 4:] = 0
    if defect == "cols_swapped":
        W = W.copy()
        W[:, [1, 2]] = W[:, [2, 1]]
    if defect == "cand_mirror":
        idx = np.arange(c.rows)
        m = (idx // 16) * 16 + 15 - idx % 16
        X = X[np.where(m < c.rows, m, idx)]
    t = X @ W
    r = Expected()
    r.c = c
    r.ref = (0 if defect == "resid_dropped" else h) + t + bias * (2 if defect == "bias_twice" else 1)
    S = np.abs(c.X.astype(np.float64)) @ np.abs(s.wdec)
    r.S = S
    r.B = U * ((K // NT + 6 + NT // 64 - 1) * S + (S + np.abs(bias)) + np.abs(r.ref))
    r.exact_ok = S + np.abs(bias) + np.abs(h) < 2.0 ** 24  # every partial sum is an integer (or a multiple of the case's unit) below 2^24
    return r


def resid_ratio(r, out):
    if not np.isfinite(out).all():
        return np.inf
    return float((np.abs(out.astype(np.float64) - r.ref) / r.B).max())


@functools.lru_cache(maxsize=None)
def resid_weights(kg, wh, kind="real", seed=0):
    """A cols4 slab of a [1024 kg][1024] matrix through the host packer. kind: real (sigma 0.02 with the special columns) or int (integers up to
    8 times power-of-two column scales that differ between neighbours: f32, fp16 and e4m3 hold them exactly)."""
    K = 1024 * kg
    rs = np.random.RandomState(31 + 7 * kg + seed)
    if kind == "real":
        w = (0.02 * rs.randn(K, D)).astype(np.float32)
        w[:, 0] *= 30.0
        w[:, 2] = (1e-5 * rs.randn(K)).astype(np.float32)
        w[:, 3] = 0.0
        w[:, 4:6] = np.clip(w[:, 4:6], -0.1, 0.1)
        w[5, 4] = np.float32(448.0 * 2.0 ** -12)
        w[5, 5] = np.nextafter(np.float32(448.0 * 2.0 ** -12), np.float32(1.0))
        bias = (0.1 * rs.randn(D)).astype(np.float32)
    else:
        w = rs.randint(-8, 9, (K, D)).astype(np.float32)  # integers up to 8: e4m3 and fp16 hold them
        w[0, :] = 8.0                                     # every column's largest entry: the fp8 scale is 2^e with 8 / 2^e <= 448
        bias = rs.randint(-16, 17, D).astype(np.float32)
        w = w * (2.0 ** ((np.arange(D) % 3) - 1)).astype(np.float32)  # power-of-two column scales that differ between neighbouring columns
    p = pack(w, COLS4, WH_ENC[wh], 0)
    s = slab_of(p, bias)
    s.w = w
    return s


def find_association_probe():
    """(t, b, h) f32 with h + (t + b) != (h + t) + b != (h + b) + t in float32 (searched, seeded): the association the source states is the only one that fits."""
    rs = np.random.RandomState(5)
    f = np.float32
    while True:
        t, b, h = f(rs.randint(1, 1 << 12)), f(rs.randint(1, 1 << 24) * 2.0 ** -24), f(rs.randint(1, 1 << 24) * 2.0 ** -12)
        a0, a1, a2 = f(h + f(t + b)), f(f(h + t) + b), f(f(h + b) + t)
        if a0 != a1 and a0 != a2:
            return t, b, h, a0
