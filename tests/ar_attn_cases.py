"""Shared by tests/test_ar_attn_kernels_gpu.py and tests/test_ar_attn_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/ar_attn_harness.hip -> libtts_ar_test.so), the float64 NumPy reference of the AR stage's attention, the case matrix and the error bound.

    out[r][h][d] = sum_{j < nk_r} softmax_j(q[r][h] . K[j][h] / 8) * V[j][h][d]            16 heads of 64, nk_r = the keys row r may see

The reference shares no code with the harness or the kernels; test_ar_attn_harness_cpu.py checks it against naive loops.

INPUTS. q is f32 holding fp16-representable values (the QKV epilogue rounds it; two kernels convert it to fp16), K and V are fp16. No input is an fp16
subnormal (the generator zeroes them), so no flush-to-zero mode of a dot or FMA instruction matters, and every q x K product is exact in f32. Families:
  flat    q, K ~ N(0, 1): score standard deviation about 1 (0.5 under LUT, see below).
  peaked  q = 8 g_r e_h + noise, K_j = t_j e_h + noise with e_h a +-1/8 pattern (|e_h|^2 = 1) and 1 <= g_r <= 1.125, so score(r, j) ~ g_r t_j: one dominant key at
          t = +30, every other key in [-30, -22.5]. The dominant key sits, in turn, on the last visible key of the last row, one key BEYOND it (visible to no
          row: a mask one key too long shows), key 0, the first key of the last chunk / group / decode sub-chunk and the key in front of it (= the last key of
          the unit before), and on a key of each of the four waves' shares.
  ramp    the same construction without noise and t_j linear from -30 (key 0) to +30 (the key beyond the last row's last): scores strictly increasing with the
          key index, so every group of the online softmax forces a rescale; `down` is the mirror image.
  poison  peaked-last, peaked-beyond and ramp-up with every cache row no row of the case may see (rows kernels: >= n_past + S; decode: >= nk of the candidate)
          filled with fp16 NaN in K and V. The K and V columns of the qkv buffer, which no attention kernel reads, are NaN in EVERY case.

ERROR BOUND (bound()). First order, per output element, evaluated in float64 from the case's inputs; u = 2^-24, E2 = 1e-6 (the relative error ar.hip's
comment states for the hardware exp2; the library expf of the two exact kernels is charged the same). p_j is the exact weight, B_d = sum_j p_j |V_jd|.
A key's weight reaches the output as a product of exponentials whose arguments telescope to s_j - M (M the row's maximum), so a common error of M cancels
between numerator and denominator and key j's weight carries the relative error

    eps_j = 64 u A_j                     the f32 dot of 64 exact products in any order (<= 64 roundings on any term), A_j = sum_i |q_i K_ji| / 8; x 0.125 is exact
          + c_arg u |s_j - M|            the scaled exponent argument: exp2 kernels (s - m) * L2E = subtraction, the rounded constant, the product: c_arg = 3,
                                         summed over the telescoping factors; expf kernels: the subtraction only, c_arg = 1
          + n_j E2                       one exponential per factor: the key's own, one per LATER rescale of its wave's state (rows kernels: later groups of
                                         the same wave up to the row's last visible key; decode: later 288-key chunks), one in the merge; expf kernels: n_j = 1
          + LUT only: 2^-11 (|s_j - M| + 1) + 2^-25     f16_round(expf(f16_round(s - mx))): the argument's rounding (absolute 2^-11 |s - mx|, or 2^-25 below
                                         2^-14) and the result's (relative 2^-11), valid while |s - mx| <= 8 keeps every weight >= e^-8 > 2^-14, a NORMAL fp16
                                         number. lut_condition() asserts that; peaked and ramp therefore run at +-3 instead of +-30 under LUT, flat at 0.5.

    bound_d = sum_j p_j eps_j |V_jd| + |o_d| sum_j p_j eps_j          numerator and denominator weights
            + u (c_num B_d + (c_den + 4) |o_d|)                       f32 accumulation, the merge and the division

c_num / c_den count the roundings on the longest chain of one term (every FMA, every rescale multiplication, every cross-lane add, the merge's FMAs):
  rows kernels       a wave walks ceil(G / 4) groups, G = ceil(nk / 8): 8 FMAs + 1 rescale each, then the 4-FMA merge and the product with 1 / tot: 9 ceil(G / 4) + 5
  decode fast        a lane takes <= ceil(nk / 32) keys and one rescale per chunk, 3 cross-lane adds, the 4-FMA merge, the division: ceil(nk/32) + ceil(nk/288) + 8
  attention_kernel   numerator: sc * inv, then nk sequential FMAs: nk + 1; denominator: ceil(nk / 64) lane terms + 6 shuffles
  attn_decode_kernel numerator: sc * inv, ceil(nk / 16) FMAs per key group, 16 adds: ceil(nk / 16) + 17; denominator: ceil(nk / 256) + 6 + 3
and the "+ 4" covers 1 / tot (or o / tot) and the final product. Nothing is fitted to a measurement.

SHARPNESS. MUTATIONS are wrong masks applied to the REFERENCE (a dropped last key, one key too many, a dropped key 0, a dropped first key of the last chunk,
group or sub-chunk, a dropped wave share). Every variant names the mutations it is built to expose (`targets`); test_ar_attn_harness_cpu.py checks that each
targeted mutation moves some output element by >= 10 x its bound, and that the peaked family of every shape targets every mutation whose key exists."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_AR_TEST_LIB") or os.path.join(PKG, "libtts_ar_test.so")
SRC = os.path.join(PKG, "testlib", "ar_attn_harness.hip")

ATTENTION, ROWS, RAGGED, DECODE_FAST, DECODE, EPILOGUE = range(6)
KERNEL_NAMES = ["attention_kernel", "attention_rows_kernel", "attention_rows_ragged_kernel", "attn_decode_fast_kernel", "attn_decode_kernel", "epilogue"]
D, NH, HD = 1024, 16, 64
SENTINEL = 0xCB
HIP_INVALID_VALUE = 1
U = 2.0 ** -24
E2 = 1e-6
F16_NAN = 0x7E00


class CaseStruct(C.Structure):
    _fields_ = [("kernel", C.c_int), ("lut", C.c_int), ("ro", C.c_int),
                ("n_cand", C.c_int), ("S", C.c_int), ("n_past", C.c_int), ("max_pos", C.c_int),
                ("n_items", C.c_int), ("n_rows", C.c_int), ("pscale", C.c_float),
                ("q", C.c_void_p), ("kc", C.c_void_p), ("vc", C.c_void_p),
                ("items", C.c_void_p), ("row_off", C.c_void_p), ("row_dst", C.c_void_p),
                ("part", C.c_void_p), ("bias", C.c_void_p),
                ("out", C.c_void_p), ("out2", C.c_void_p),
                ("kout", C.c_void_p), ("vout", C.c_void_p), ("kout2", C.c_void_p), ("vout2", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_ar_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_ar_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_ar_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_ar_test_validate.argtypes = [C.POINTER(CaseStruct)]
        for f in (L.tts_ar_test_run, L.tts_ar_test_validate, L.tts_ar_test_margin):
            f.restype = C.c_int
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape, dtype):
        self.margin = harness().tts_ar_test_margin()
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * self.dtype.itemsize, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


def struct(kernel, q=None, kc=None, vc=None, n_cand=1, S=1, n_past=0, max_pos=1, lut=0, ro=0, items=None, row_off=None, n_rows=0, out=None, **kw):
    """A CaseStruct over the given arrays (kept alive on the struct). Array SIZES are checked here, everything else by the harness."""
    cs = CaseStruct()
    cs.kernel, cs.lut, cs.ro, cs.n_cand, cs.S, cs.n_past, cs.max_pos, cs.n_rows = kernel, lut, ro, n_cand, S, n_past, max_pos, n_rows
    cs.n_items = 0 if items is None else len(items)
    keep = [q, kc, vc, items, row_off, out]
    for name, a, dt in (("q", q, np.float32), ("kc", kc, np.uint16), ("vc", vc, np.uint16), ("items", items, np.int32), ("row_off", row_off, np.int32)):
        if a is not None:
            assert a.dtype == dt and a.flags.c_contiguous, name
            setattr(cs, name, _ptr(a))
    if out is not None:
        cs.out = _ptr(out.raw) if isinstance(out, Guarded) else out
    for k, v in kw.items():
        setattr(cs, k, v)
    cs._keep = keep
    return cs


def run_attention(kernel, q, kc, vc, S=1, n_past=0, lut=0, row_off=None, items=None):
    """One launch. q: [n_cand * S, 3072] (ATTENTION, ROWS), [n_rows, 3072] (RAGGED) or [n_cand, 1024] (decode) f32; kc / vc [n_cand, max_pos, 1024] uint16.
    -> out [rows, 1024] f32. Asserts success, intact canaries and that every payload element was written."""
    n_cand, max_pos = kc.shape[0], kc.shape[1]
    assert kc.shape == vc.shape == (n_cand, max_pos, D)
    decode = kernel in (DECODE_FAST, DECODE)
    rows = q.shape[0]
    assert q.shape == (rows, D if decode else 3 * D)
    if kernel in (ATTENTION, ROWS):
        assert rows == n_cand * S
    if decode:
        assert rows == n_cand and (row_off is None or row_off.shape == (n_cand,))
    if items is not None:
        assert items.ndim == 2 and items.shape[1] == 4
    out = Guarded((rows, D), np.float32)
    cs = struct(kernel, q=q, kc=kc, vc=vc, n_cand=n_cand, S=S, n_past=n_past, max_pos=max_pos, lut=lut, ro=int(row_off is not None),
                items=items, row_off=row_off, n_rows=rows if kernel == RAGGED else 0, out=out)
    rc = harness().tts_ar_test_run(C.byref(cs))
    assert rc == 0, "harness returned HIP error %d" % rc
    assert out.canaries_intact(), "a kernel wrote outside its output buffer"
    return out


# ---------------------------------------------------------------------------------------------------------------- reference

def reference(q, K, V, mask, s=None):
    """q [R, 16, 64], K / V [P, 16, 64], mask [R, P] bool -> dict(out [R, 16, 64], p [R, 16, P], s [R, 16, P], M) in float64. A row without keys, or one
    whose mask admits a poisoned (NaN) cache row, gives NaN. s: the scores of an earlier call on the same q and K."""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    kbad = ~(np.isfinite(K).all(axis=2) & np.isfinite(V).all(axis=2))  # [P, 16]
    if s is None:
        s = np.einsum("rhd,phd->rhp", q, np.where(np.isfinite(K), K, 0.0)) / 8.0
    m3 = np.broadcast_to(mask[:, None, :], s.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        sm = np.where(m3, s, -np.inf)
        M = sm.max(axis=2, keepdims=True)
        w = np.where(m3, np.exp(sm - np.where(np.isfinite(M), M, 0.0)), 0.0)
        p = w / w.sum(axis=2, keepdims=True)
        out = np.einsum("rhp,phd->rhd", p, np.where(np.isfinite(V), V, 0.0))
    bad = (m3 & kbad.T[None]).any(axis=2)
    out = np.where(bad[:, :, None], np.nan, out)
    return dict(out=out, p=p, s=s, M=M)


def causal_mask(nk, P):
    return np.arange(P)[None, :] < np.asarray(nk)[:, None]


KINDS = {ATTENTION: "attention", ROWS: "rows", RAGGED: "rows", DECODE_FAST: "dfast", DECODE: "decode"}


def bound(kind, q, K, V, nk, lut=0, ref=None):
    """The module docstring's bound for kernel class `kind` ('rows', 'dfast', 'attention', 'decode'): [R, 16, 64] float64. nk [R]: keys per row."""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    nk = np.asarray(nk)
    P = K.shape[0]
    mask = causal_mask(nk, P)
    r = ref or reference(q, K, V, mask)
    Kz, Vz = np.where(np.isfinite(K), K, 0.0), np.abs(np.where(np.isfinite(V), V, 0.0))
    A = np.einsum("rhd,phd->rhp", np.abs(q), np.abs(Kz)) / 8.0
    with np.errstate(invalid="ignore"):
        gap = np.where(mask[:, None, :], np.abs(np.where(np.isfinite(r["s"]), r["s"], 0.0) - r["M"]), 0.0)
    j = np.arange(P)[None, :]
    last = (nk - 1)[:, None]
    if kind == "rows":
        n_exp = 2 + np.maximum(last // 8 - j // 8, 0) // 4
        c_arg = 3
        G = (nk + 7) // 8
        c_num = c_den = 9 * ((G + 3) // 4) + 5
    elif kind == "dfast":
        n_exp = 2 + np.maximum(last // 288 - j // 288, 0)
        c_arg = 3
        c_num = c_den = (nk + 31) // 32 + (nk + 287) // 288 + 8
    elif kind == "attention":
        n_exp, c_arg = np.ones_like(j), 1
        c_num, c_den = nk + 1, (nk + 63) // 64 + 6
    elif kind == "decode":
        n_exp, c_arg = np.ones_like(j), 1
        c_num, c_den = (nk + 15) // 16 + 17, (nk + 255) // 256 + 9
    else:
        raise ValueError(kind)
    eps = 64 * U * A + c_arg * U * gap + (n_exp * E2)[:, None, :]
    if lut:
        assert kind in ("attention", "decode")
        eps = eps + 2.0 ** -11 * (gap + 1.0) + 2.0 ** -25
    pe = r["p"] * eps
    o = np.abs(r["out"])
    B = np.einsum("rhp,phd->rhd", r["p"], Vz)
    return (np.einsum("rhp,phd->rhd", pe, Vz) + o * pe.sum(axis=2)[:, :, None]
            + U * (np.asarray(c_num)[:, None, None] * B + (np.asarray(c_den) + 4)[:, None, None] * o))


def lut_condition(ref, mask):
    """|s - mx| <= 8 over every visible key: the condition of the LUT terms of the bound."""
    with np.errstate(invalid="ignore"):
        gap = np.where(mask[:, None, :], np.abs(np.where(np.isfinite(ref["s"]), ref["s"], 0.0) - ref["M"]), 0.0)
    return bool(gap.max() <= 8.0)


# ---------------------------------------------------------------------------------------------------------------- structure and mutations

class Structure(object):
    """Where a kernel class cuts the key axis. units: sizes whose multiples start a chunk / group / sub-chunk; wave(j): the wave that owns key j."""

    def __init__(self, name, units, wave):
        self.name, self.units, self.wave = name, units, wave


# rows kernels: 128-key LDS chunks, groups of 8 keys dealt to the 4 waves (chunks hold 16 groups, so group g of the sequence belongs to wave g % 4)
ROWS_STRUCT = Structure("rows", (("chunk", 128), ("group", 8)), lambda j: (j // 8) % 4)
# decode: 288-key chunks cut into 32-key rounds r = 0 .. NR - 1 (288 = 9 x 32: rounds start at multiples of 32), key group kg = (j - j0) % 32, wave = kg // 8;
# attn_decode_kernel's score phase strides by 256
DECODE_STRUCT = Structure("decode", (("chunk", 288), ("round", 32), ("stride", 256)), lambda j: (j % 32) // 8)


def mutation_names(st):
    return ["drop_last", "admit_one", "drop_key0"] + ["drop_first_of_last_" + n for n, _ in st.units] + ["drop_wave%d" % w for w in range(4)]


def mutate(name, st, nk, P):
    """The wrong mask of mutation `name` for rows of nk keys over P cache rows, or None where no row has the key it would touch."""
    nk = np.asarray(nk)
    mask = causal_mask(nk, P)
    R = np.arange(len(nk))
    m = mask.copy()
    if name == "drop_last":
        m[R, nk - 1] = False
    elif name == "admit_one":
        ok = nk < P
        m[R[ok], nk[ok]] = True
    elif name == "drop_key0":
        m[:, 0] = False
    elif name.startswith("drop_first_of_last_"):
        u = dict(st.units)[name[len("drop_first_of_last_"):]]
        m[R, (nk - 1) // u * u] = False
    elif name.startswith("drop_wave"):
        m &= (st.wave(np.arange(P)) != int(name[-1]))[None, :]
    else:
        raise ValueError(name)
    return None if (m == mask).all() else m


def placements(st, nk_last, P):
    """Dominant-key positions of the peaked family for a case whose last row sees nk_last keys of P cache rows: [(tag, key, targets)], duplicates merged."""
    pl = [("last", nk_last - 1, ["drop_last"]), ("key0", 0, ["drop_key0"])]
    if nk_last < P:
        pl.append(("beyond", nk_last, ["admit_one"]))
    for n, u in st.units:
        f = (nk_last - 1) // u * u
        pl.append((n + "_first", f, ["drop_first_of_last_" + n]))
        if f > 0:
            pl.append((n + "_prev_last", f - 1, []))
    for w in range(4):
        own = [j for j in range(nk_last - 1, max(nk_last - 33, -1), -1) if st.wave(j) == w]
        if own:
            pl.append(("wave%d" % w, own[0], ["drop_wave%d" % w]))
    merged = {}
    for tag, key, tg in pl:
        if key in merged:
            merged[key] = (merged[key][0] + "+" + tag, key, merged[key][2] + tg)
        else:
            merged[key] = (tag, key, list(tg))
    out = []
    for tag, key, tg in merged.values():
        if key == nk_last - 1 and "drop_last" not in tg:
            tg.append("drop_last")
        if key == 0 and "drop_key0" not in tg:
            tg.append("drop_key0")
        out.append((tag, key, tg))
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs

def f16(x):
    """Round to fp16 without subnormals -> (float32 values, uint16 bits)."""
    h = np.asarray(x, np.float32).astype(np.float16)
    h = np.where(np.abs(h.astype(np.float32)) < 2.0 ** -14, np.float16(0), h)
    return h.astype(np.float32), h.view(np.uint16)


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def gen(seed, family, R, P, nk_last, jstar=None, down=False, lut=0):
    """One sequence: q [R, 16, 64] f32 (fp16 values), K, V [P, 16, 64] f32 (fp16 values)."""
    rng = np.random.RandomState(seed)
    if family == "flat":
        q = rng.randn(R, NH, HD) * (0.5 if lut else 1.0)
        k = rng.randn(P, NH, HD)
    else:
        smax = 3.0 if lut else 30.0
        e = rng.choice([-0.125, 0.125], (NH, HD))
        g = 1.0 + rng.randint(0, 5, (R, NH)) / 32.0
        j = np.arange(P, dtype=np.float64)
        if family == "peaked":
            t = -smax * rng.uniform(0.75, 1.0, (P, NH))
            t[jstar, :] = smax
            nq, nkk = 0.125 * rng.randn(R, NH, HD), 0.125 * rng.randn(P, NH, HD)
        elif family == "ramp":
            if lut:  # a shallow rise to -2, then the last 32 keys climb to +3: non-decreasing, |s - mx| <= 8
                up = np.maximum(-smax + j / P, smax - (nk_last - 1 - j) * (2 * smax - 1) / 32.0)
            else:
                up = -smax + 2 * smax * j / max(nk_last, 1)  # the key beyond the last row's last continues the ramp at +smax
            t = up if not down else np.where(j < nk_last, up[np.clip(nk_last - 1 - j.astype(int), 0, P - 1)], -smax)
            t = np.repeat(t[:, None], NH, axis=1)
            nq, nkk = 0.0, 0.0
        else:
            raise ValueError(family)
        q = 8.0 * e[None] * g[:, :, None] + nq
        k = t[:, :, None] * e[None] + nkk
    v = rng.randn(P, NH, HD)
    return f16(q)[0], f16(k)[0], f16(v)[0]


class Variant(object):
    """One candidate of a launch: a sequence of R rows over P cache rows. nk [R]; poison_from: first cache row filled with NaN (None: no poison)."""

    def __init__(self, family, tag, targets, q, K, V, nk, poison_from=None, lut=0):
        self.family, self.tag, self.targets, self.nk, self.lut = family, tag, targets, np.asarray(nk), lut
        self.q, self.K, self.V = q, K.copy(), V.copy()
        self.poison_from = poison_from
        if poison_from is not None:
            self.K[poison_from:] = np.nan
            self.V[poison_from:] = np.nan
        self._ref, self._bounds = None, {}

    @property
    def P(self):
        return self.K.shape[0]

    def mask(self):
        return causal_mask(self.nk, self.P)

    def ref(self):
        if self._ref is None:
            self._ref = reference(self.q, self.K, self.V, self.mask())
        return self._ref

    def bound(self, kind):
        if kind not in self._bounds:
            self._bounds[kind] = bound(kind, self.q, self.K, self.V, self.nk, self.lut, self.ref())
        return self._bounds[kind]

    def bits(self, a):
        h = np.asarray(a, np.float32).astype(np.float16).view(np.uint16).copy()
        h[np.isnan(np.asarray(a, np.float32))] = F16_NAN
        return h


def variants(st, shape_key, R, P, nk, lut=0, see_to=None, want=None):
    """Every variant of one shape: flat, peaked at each placement, ramp up and down, three poisoned ones. nk [R]; see_to: the first cache row no row may see.
    want(family, tag, targets): build only the variants it accepts (the same ones, from the same seeds)."""
    nk = np.asarray(nk)
    nk_last = int(nk[-1])
    see_to = int(nk.max()) if see_to is None else see_to
    out = []

    def add(family, tag, targets, poison=False, **kw):
        if want is not None and not want(family, tag, targets):
            return
        q, K, V = gen(_seed(st.name, shape_key, family, tag, lut), family if family != "poison" else kw.pop("base"), R, P, nk_last, lut=lut, **kw)
        out.append(Variant(family, tag, targets, q, K, V, nk, see_to if poison else None, lut))

    add("flat", "flat", [])
    pls = placements(st, nk_last, P)
    for tag, key, tg in pls:
        if key == nk_last - 1 and R > 1 and "admit_one" not in tg:  # the last row's last key is the key beyond the row before it
            tg = tg + ["admit_one"]
        add("peaked", tag, tg, jstar=key)
    add("ramp", "up", ["drop_last"] + (["admit_one"] if nk_last < P else []))
    add("ramp", "down", ["drop_key0"], down=True)
    add("poison", "peaked-last", ["drop_last"], poison=True, base="peaked", jstar=nk_last - 1)
    if see_to < P:
        add("poison", "peaked-beyond", ["admit_one"] if nk_last < P else [], poison=True, base="peaked", jstar=min(nk_last, P - 1))
    add("poison", "ramp-up", ["drop_last"], poison=True, base="ramp")
    return out


ROWS_SHAPES = [(1, 0), (7, 0), (8, 0), (9, 0), (63, 0), (64, 0), (65, 0), (127, 0), (128, 0), (129, 0), (1, 127), (1, 128), (1, 1023),
               (40, 281), (130, 300), (64, 960)]
DECODE_COUNTS = [1, 2, 8, 31, 32, 33, 95, 96, 97, 159, 160, 161, 223, 224, 225, 287, 288, 289, 384, 385, 576, 577, 1023, 1024]


def rows_max_pos(S, n_past):
    return min(1024, n_past + S + 1)  # one cache row beyond the sequence where the cache has one


def rows_variants(S, n_past, lut=0, want=None):
    P = rows_max_pos(S, n_past)
    return variants(ROWS_STRUCT, (S, n_past), S, P, n_past + 1 + np.arange(S), lut, see_to=n_past + S, want=want)


def decode_max_pos(nk):
    return min(1024, nk + 1)


def decode_variants(nk, lut=0, want=None):
    return variants(DECODE_STRUCT, nk, 1, decode_max_pos(nk), [nk], lut, want=want)


def pack_rows(vs, S):
    """Variants of one rows shape as the candidates of one launch -> qkv [n * S, 3072] f32 (K and V columns NaN), kc, vc [n, P, 1024] uint16."""
    P = vs[0].P
    qkv = np.full((len(vs) * S, 3 * D), np.nan, np.float32)
    kc = np.zeros((len(vs), P, D), np.uint16)
    vc = np.zeros((len(vs), P, D), np.uint16)
    for c, v in enumerate(vs):
        qkv[c * S:(c + 1) * S, :D] = v.q.reshape(S, D)
        kc[c] = v.bits(v.K).reshape(P, D)
        vc[c] = v.bits(v.V).reshape(P, D)
    return qkv, kc, vc


def pack_decode(vs, max_pos=None):
    """Single-row variants as the candidates of one decode launch -> q [n, 1024], kc, vc [n, max_pos, 1024]; cache rows behind a variant's own are zero, or NaN
    where the variant is poisoned."""
    max_pos = max_pos or max(v.P for v in vs)
    q = np.zeros((len(vs), D), np.float32)
    kc = np.zeros((len(vs), max_pos, D), np.uint16)
    vc = np.zeros((len(vs), max_pos, D), np.uint16)
    for c, v in enumerate(vs):
        q[c] = v.q.reshape(D)
        kc[c, :v.P] = v.bits(v.K).reshape(v.P, D)
        vc[c, :v.P] = v.bits(v.V).reshape(v.P, D)
        if v.poison_from is not None:
            kc[c, v.P:] = F16_NAN
            vc[c, v.P:] = F16_NAN
    return q, kc, vc


def ratio(out, v, kind):
    """max |out - reference| / bound over a variant's elements (inf where the output is not finite)."""
    o = np.asarray(out, np.float64).reshape(v.ref()["out"].shape)
    if not np.isfinite(o).all():
        return float("inf")
    err, b = np.abs(o - v.ref()["out"]), v.bound(kind)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(err == 0, 0.0, err / b).max())  # a bound of 0 (every visible V element 0) asks for the exact 0
