"""Shared by tests/test_dattn_kernels_gpu.py and tests/test_dattn_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/diff_attn_harness.hip -> libtts_dattn_test.so), the float64 NumPy reference of the diffusion AttentionBlock core, the error bounds and
the case matrix. Per sequence of T rows, head h, query t:

    o[t] = sum_{j < T} softmax_j(q_t . k_j / 8 + bias[h][(j > t ? 64 : 0) + min(|j - t|, 63)]) v_j                 16 heads of 64

The reference shares no code with the harness or the kernels; test_dattn_harness_cpu.py checks it against naive loops. Operands are the values the kernel
multiplies: the fp16 values for the two fp16 kernels (F16_Q128 = diff_attn_kernel<2,2>, F16_Q64 = diff_attn_kernel<2,1>), hi + lo for the split-precision kernel
(F32 = diff_attn_f32_kernel), whose output is compared as out_hi + out_lo. The bias table [16][128] is an input of the case, not derived from T5 bucketing.

INPUTS. No value is an fp16 subnormal (hi and lo halves alike: the generator zeroes them). One case = one (family, bias table) on a layout; every head of a
sequence draws its own numbers. Families, with e_h a +-1/8 pattern (|e_h|^2 = 1), q_t = 8 g_t e_h + noise, k_j = c_j e_h + noise, 1 <= g_t <= 1.125, so that
score(t, j) ~ g_t c_j:
  flat       q, k ~ N(0, 1): score standard deviation 1; every key matters, so every wrong bias index shows under the `sharp` table.
  peaked     one dominant key (c = +30, every other key in [-30, -22.5]). Head h takes placement h mod n of: key T - 1; key T (visible to nobody: it is the
             guard row's content); key 0; the first key of the last 64-key tile and the key before it; the keys at distance -64, -63, -62 from the first query of
             a 32-query wave and +62, +63, +64 from the last query of one.
  ramp-up    c_j linear from -30 (key 0) to +30 (key T, the guard row): the running maximum rises at every tile, every tile rescales. ramp-down is the mirror
             image: the maximum is in tile 0 and the rescale branch is never taken after it.
  split      two orthogonal patterns: queries 0 .. 15 of every 32-query wave peak on key 0, queries 16 .. 31 on key T - 1, so in the last tile half the lanes of a
             wave have alpha == 1 and half do not (the `!__all(alpha == 1)` branch with mixed lanes).
  wide       flat with q and k doubled: score standard deviation 4; wide_condition() asserts that at least a quarter of the weights lie below 2^-14 of the
             running maximum (T >= 64), where the fp16 weight is a subnormal.
Bias tables: `smooth` (trained-like: |b| <= 1, monotone in distance on either side) and `sharp` (an independent magnitude uniform in [0.5, 4] per (head, side, distance), the sign
alternating with distance, side and head: neighbouring entries, the two sides, entries 62 / 63 and heads h / h ^ 1 all differ by at least 1, far more than any
bound).
Every case exists unpoisoned (the guard row behind a sequence holds key T of its family, every other row outside a sequence is zero) and poisoned (every row no
query or key of a sequence may see: guard rows, the 128 slack rows, the rows in front of the first sequence: +-60000 in Q, K and V^T). Finite, not NaN: a masked
key has weight 0 and the matrix pipe would turn 0 x Inf into NaN; "rows outside a sequence hold finite values" is the product's contract.

LENGTHS and the (tile, wave) classes they reach, from the a / b / last arithmetic of the kernel's tile loop (restated in tile_classes(); queries qw .. qw + QW - 1
of a wave, QW = 32 (16 with 64-query workgroups), 64-key tile kb): far below = kb < a, a = (qw - 126) / 64 + 1 for qw >= 126; far above = kb >= b,
b = (qw + QW + 125) / 64; the masked tail = tile `last` when T % 64 != 0, itself far above when 64 last - (qw + QW - 1) >= 63.
  1 .. 63          one masked tail tile, near (1, 15, 16, 17, 31, 32, 33, 63: the 16-query block and the 32-query wave)
  64               one full near tile, no tail (the 64-query workgroup edge); 65, 95, 96, 97, 127: a full near tile and a near tail
  128              two full near tiles, no tail (the 128-query workgroup edge)
  129 .. 191       a second query block: its wave 0 (qw = 128) has tile 0 FAR BELOW; the tail (tile 2) is FAR ABOVE for the waves qw <= 32 (qw <= 48 with QW = 16) and
                   near for the others (129, 190, 191)
  192              tile 2 is a full FAR ABOVE tile of the waves qw = 0, 32; no tail. 193, 255: the same with a tail that is far above for qw <= 96
  256, 257, 320, 383, 384, 385, 577     every class at once, in up to 5 query blocks and 10 tiles; 256, 320, 384 without a tail
The tail tile's second condition, `qw - (kmin + 63) >= 63` (far BELOW), needs qw >= 64 last + 126 >= T + 62: a wave without a stored query. It is never taken by a
stored query (test_dattn_harness_cpu.py asserts it over every length).

ERROR BOUND, fp16 kernels (bound16()). First order, per output element, evaluated in float64 from the case's inputs; u = 2^-24 and E2 = 1e-6 (the hardware exp2)
as in tests/ar_attn_cases.py. p_j the exact weight, L = sum_j e^(s_j - M), M the row's maximum, m_j the exact running maximum after key j's tile, A_j =
sum_i |q_i k_ji| / 8, nt = ceil(T / 64). A key's weight reaches the output as 2^(its argument - m_tile) times the later rescale factors; the arguments telescope
to s_j - M whatever the rounded maxima are, and numerator and denominator are BOTH sums of the same rounded weights (the row sum comes from the matrix pipe, ones
x P^T), so a weight error d_j moves o_d by d_j (v_jd - o_d) / L, bounded by d_j (|v_jd| + |o_d|) / L. The relative weight error:
    eps_j = 64 u A_j                         the f32 MFMA accumulation of 64 exact products, any order
          + u (2 |s_j| + 2 |b_j| + |M|)      the folded scaling: the table is pre-multiplied by L2E / SC = 8 (exact: SC = 0.125 L2E), v = S + 8 b is one rounding
                                             (u |s_j| after the scaling); a far tile instead rounds boff = 8 b SC, sub = boff - m and the FMA
          + 3 u |s_j - M|                    the rounded constant SC on the telescoped argument, the FMA's rounding, the subtractions m_old - m_new
          + (1 + nt - 1 - tile_j) E2         one exp2 for the weight and one per later rescale
          + 2^-11                            the fp16 rounding of the weight
    and the absolute term 2^-25 e^(m_j - M) / L: below 2^-14 of the RUNNING maximum the fp16 weight is a subnormal (spacing 2^-24), and the later rescales
    multiply that error by e^(m_j - M).
    bound_d = sum_j (p_j eps_j + 2^-25 e^(m_j - M) / L) (|v_jd| + |o_d|)
            + u (65 nt B_d + (65 nt + 4) |o_d|)       B_d = sum_j p_j |v_jd|; f32 accumulation over nt tiles: two MFMAs of 32 products and one rescale per tile
                                                      on the longest chain, the same for the row sum; 1 / l and the product
            + ulp16(|o_d| + the above) / 2            the final fp16 rounding of a value that close to o_d
Split-precision kernel (bound32()); out_hi + out_lo is compared. Its weights are NOT rounded in the denominator (lsum adds the unrounded p on the VALU) but split
into fp16 pairs in the numerator, so the split's error does not cancel:
    eps_j = (2^-22 + 192 u) A_j              the dropped lo x lo products; three times 64 exact products
          + u (|s_j| + 3 |s_j - M| + 6)      v = fma(S, 0.125, b); v - m, the rounded L2E, the FMA with the + 8 offset (8 ln 2 < 6), the alphas
          + (nt - tile_j) E2
    bound_d = sum_j p_j eps_j (|v_jd| + |o_d|)
            + sum_j (2^-21 p_j + 2^-33 e^(m_j - M) / L) |v_jd|        p = hi + lo: lo is rounded to 2^-22 p, or to 2^-25 absolute (at the scale 2^8 e^(s - m) the
                                                                      kernel gives p) where p - hi is a subnormal; the dropped v_lo x p_lo, 2^-22 of the term
            + u (193 nt B_d + (18 nt + 6) |o_d|)                       six MFMAs of 32 products and a rescale per tile; 16 adds, one add and a rescale per tile
                                                                      and the two cross-lane adds for l; 1 / l and the product
            + 2^-22 |o_d| + 2^-25                                      the hi / lo split of the output
Nothing is fitted to a measurement.

SHARPNESS. MUTATIONS are applied to the REFERENCE; test_dattn_harness_cpu.py checks that each moves some element of a case that targets it by >= 10 x its bound.
The saturated constant `one tile too late` below the diagonal (tile a treated as far) and `one tile too early` above it (tile b - 1) change values; the opposite
directions only send a far tile down the near path, which computes the same bias, so they are no mutation of the arithmetic."""
import ctypes as C
import functools
import os
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_DATTN_TEST_LIB") or os.path.join(PKG, "libtts_dattn_test.so")
SRC = os.path.join(PKG, "testlib", "diff_attn_harness.hip")

F16_Q128, F16_Q64, F32 = range(3)
KINDS = [F16_Q128, F16_Q64, F32]
KIND_NAMES = ["diff_attn_kernel<2,2>", "diff_attn_kernel<2,1>", "diff_attn_f32_kernel"]
CH, NH, HD = 1024, 16, 64
SENTINEL = 0xCB
HIP_INVALID_VALUE = 1
U = 2.0 ** -24
E2 = 1e-6
POISON = 60000.0

LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 190, 191, 192, 193, 255, 256, 257, 320, 383, 384, 385, 577]
FAMILIES = ["flat", "peaked", "ramp-up", "ramp-down", "split", "wide"]
TABLES = ["smooth", "sharp"]
CONFIGS = [(f, t) for f in FAMILIES for t in TABLES]
TRIPLES = [(65, 1, 129), (193, 1, 33), (257, 1, 127)]
EIGHT = (17, 64, 1, 129, 33, 192, 63, 130)


class CaseStruct(C.Structure):
    _fields_ = [("kind", C.c_int), ("ns", C.c_int), ("rows", C.c_int), ("ldvt", C.c_int), ("qk_rows", C.c_int), ("out_rows", C.c_int),
                ("start", C.c_void_p), ("len", C.c_void_p),
                ("qk", C.c_void_p), ("qk_lo", C.c_void_p), ("vt", C.c_void_p), ("vt_lo", C.c_void_p),
                ("bias_tab", C.c_void_p), ("out", C.c_void_p), ("out_lo", C.c_void_p), ("launch", C.c_void_p)]


try:  # the batched matrix products here are small: BLAS worker threads cost several times what they save (the numbers do not change)
    from threadpoolctl import threadpool_limits
except ImportError:
    threadpool_limits = None


def one_thread(f):
    @functools.wraps(f)
    def g(*a, **kw):
        if threadpool_limits is None:
            return f(*a, **kw)
        with threadpool_limits(limits=1, user_api="blas"):
            return f(*a, **kw)
    return g


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_dattn_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_dattn_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_dattn_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_dattn_test_validate.argtypes = [C.POINTER(CaseStruct)]
        for f in (L.tts_dattn_test_run, L.tts_dattn_test_validate, L.tts_dattn_test_margin):
            f.restype = C.c_int
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape, dtype):
        self.margin = harness().tts_dattn_test_margin()
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * self.dtype.itemsize, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


def struct(kind, _check=True, **kw):
    """A CaseStruct over the given arrays (kept alive on the struct). Array SIZES are checked here against the sizes the case names, everything else by the
    harness."""
    cs = CaseStruct()
    cs.kind = kind
    keep = []
    sizes = {"start": lambda: kw["ns"], "len": lambda: kw["ns"], "qk": lambda: kw["qk_rows"] * 2048, "qk_lo": lambda: kw["qk_rows"] * 2048,
             "vt": lambda: CH * kw["ldvt"], "vt_lo": lambda: CH * kw["ldvt"], "bias_tab": lambda: NH * 128}
    for k, v in kw.items():
        if k in ("out", "out_lo"):
            if v is not None:
                assert not _check or v.payload.size == kw["out_rows"] * CH, k
                setattr(cs, k, _ptr(v.raw))
            keep.append(v)
        elif k in sizes:
            if v is not None:
                want = np.float32 if k == "bias_tab" else np.int32 if k in ("start", "len") else np.uint16
                assert v.dtype == want and v.flags.c_contiguous, k
                n = sizes[k]() if _check else 0
                assert not _check or v.size == n, (k, v.size, n)  # (_check=False: a case the harness must refuse before it reads anything)
                setattr(cs, k, _ptr(v))
            keep.append(v)
        elif k == "launch":
            setattr(cs, k, _ptr(v))
            keep.append(v)
        else:
            setattr(cs, k, v)
    cs._keep = keep
    return cs


class HipError(RuntimeError):
    """a HIP call of the harness failed: nothing more is launched in this session (test_dattn_kernels_gpu.py ends it)"""


# ---------------------------------------------------------------------------------------------------------------- layout and tile classes

class Lay(object):
    """Layout::build: sequences from row 8 on, every start a multiple of 8, a guard row behind every sequence, rows padded to a multiple of 128."""

    def __init__(self, lens):
        self.ns = len(lens)
        self.len = np.array(lens, np.int32)
        self.start = np.zeros(self.ns, np.int32)
        r = 8
        for s, n in enumerate(lens):
            self.start[s] = r
            r = (r + n + 1 + 7) & ~7
        self.rows = (r + 127) & ~127

    def seq_rows(self, s):
        return slice(int(self.start[s]), int(self.start[s] + self.len[s]))

    def row_mask(self):
        m = np.zeros(self.rows, bool)
        for s in range(self.ns):
            m[self.seq_rows(s)] = True
        return m


def queries_per_wave(kind):
    return 16 if kind == F16_Q64 else 32


def tile_bounds(qw, QW, T):
    """The kernel's tile loop for the wave of queries qw .. qw + QW - 1: (a, b, last, nkb): tiles [0, a) far below, [a, b) near, [b, last) far above, `last` the
    masked tail when last < nkb."""
    nkb = (T + 63) // 64
    last = nkb - 1 if T % 64 else nkb
    a = min(max((qw - 126) // 64 + 1 if qw >= 126 else 0, 0), last)
    b = min((qw + QW + 62 + 63) // 64, last)
    return a, b, last, nkb


def tile_classes(T, kind=F16_Q128):
    """The set of (tile, wave) classes the stored queries of a sequence of T rows reach in the fp16 kernels."""
    QW = queries_per_wave(kind)
    got = set()
    for qw in range(0, T, QW):
        a, b, last, nkb = tile_bounds(qw, QW, T)
        if a > 0:
            got.add("far-below")
        if b > a:
            got.add("near")
        if last > b:
            got.add("far-above")
        if last < nkb:
            kmin = last * 64
            far_hi, far_lo = kmin - (qw + QW - 1) >= 63, qw - (kmin + 63) >= 63
            got.add("tail-far-above" if far_hi else "tail-far-below" if far_lo else "tail-near")
        else:
            got.add("no-tail")
    return got


# ---------------------------------------------------------------------------------------------------------------- inputs

def f16(x):
    """Round to fp16 without subnormals -> float64 values."""
    h = np.asarray(x, np.float64).astype(np.float16)
    h = np.where(np.abs(h.astype(np.float64)) < 2.0 ** -14, np.float16(0), h)
    return h.astype(np.float64)


def split(x):
    """x -> (hi, lo), fp16 values without subnormals, as float64"""
    hi = f16(x)
    return hi, f16(np.asarray(x, np.float64) - hi)


def bits(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def bias_table(name, seed=0):
    rng = np.random.RandomState(_seed("bias", name, seed))
    if name == "sharp":
        sign = np.where((np.arange(NH)[:, None, None] + np.arange(2)[None, :, None] + np.arange(64)[None, None, :]) % 2 == 0, 1.0, -1.0)
        return (sign * rng.uniform(0.5, 4.0, (NH, 2, 64))).reshape(NH, 128).astype(np.float32)
    c = rng.uniform(0.3, 1.0, (NH, 2, 1))
    return (-c * (np.arange(64) / 63.0)[None, None, :]).reshape(NH, 128).astype(np.float32)  # 0 on the diagonal, falling with distance on either side


def placements(T):
    """Dominant-key positions of the peaked family for a sequence of T rows: [(tag, key)] (keys 0 .. T; T is the guard row)."""
    f = (T - 1) // 64 * 64
    pl = [("last", T - 1), ("beyond", T), ("key0", 0), ("tile_first", f)]
    if f > 0:
        pl.append(("tile_prev_last", f - 1))
    for d in (-64, -63, -62):  # from the first query of the last wave that has such a key
        tq = (T - 1) // 32 * 32
        if tq + d >= 0:
            pl.append(("d%d" % d, tq + d))
    for d in (62, 63, 64):  # from the last query of wave 0
        if 31 + d < T:
            pl.append(("d+%d" % d, 31 + d))
    out, seen = [], set()
    for tag, key in pl:
        if key not in seen:
            seen.add(key)
            out.append((tag, key))
    return out


def gen(seed, family, T):
    """One sequence -> q, k, v [16, T + 1, 64] float64 before the fp16 split (row T: the guard row's content)"""
    rng = np.random.RandomState(seed)
    P = T + 1
    v = rng.randn(NH, P, HD)
    if family in ("flat", "wide"):
        sc = 2.0 if family == "wide" else 1.0
        return sc * rng.randn(NH, P, HD), sc * rng.randn(NH, P, HD), v
    smax = 30.0
    e = rng.choice([-0.125, 0.125], (NH, 1, HD))
    g = 1.0 + rng.randint(0, 5, (NH, P, 1)) / 32.0
    j = np.arange(P, dtype=np.float64)
    if family == "peaked":
        c = -smax * rng.uniform(0.75, 1.0, (NH, P))
        pl = placements(T)
        for h in range(NH):
            c[h, pl[h % len(pl)][1]] = smax
        q = 8.0 * e * g + 0.125 * rng.randn(NH, P, HD)
        k = c[:, :, None] * e + 0.125 * rng.randn(NH, P, HD)
    elif family in ("ramp-up", "ramp-down"):
        up = -smax + 2 * smax * j / T
        c = up if family == "ramp-up" else np.where(j < T, up[np.clip(T - 1 - j.astype(int), 0, T)], -smax)
        q = 8.0 * e * g + 0.01 * rng.randn(NH, P, HD)
        k = c[None, :, None] * e + 0.01 * rng.randn(NH, P, HD)
    elif family == "split":
        flip = np.where(np.arange(HD) % 2 == 0, 1.0, -1.0)[None, None, :]  # e2 = e with every other sign flipped: orthogonal to e
        e2 = e * flip
        late = (np.arange(P) % 32 >= 16)[None, :, None]
        q = 8.0 * g * np.where(late, e2, e) + 0.125 * rng.randn(NH, P, HD)
        c1 = -smax * rng.uniform(0.75, 1.0, (NH, P))
        c2 = -smax * rng.uniform(0.75, 1.0, (NH, P))
        c1[:, 0] = smax
        c2[:, T - 1] = smax
        k = c1[:, :, None] * e + c2[:, :, None] * e2 + 0.125 * rng.randn(NH, P, HD)
    else:
        raise ValueError(family)
    return q, k, v


class Seq(object):
    """One sequence's operands: qh, ql, kh, kl, vh, vl [16, T + 1, 64] float64 (fp16 values), row T = the guard row's content."""

    def __init__(self, family, T, tag):
        self.family, self.T = family, T
        q, k, v = gen(_seed(family, T, tag), family, T)
        (self.qh, self.ql), (self.kh, self.kl), (self.vh, self.vl) = split(q), split(k), split(v)
        self._ref = {}

    def operands(self, f32):
        if f32:
            return self.qh + self.ql, self.kh + self.kl, self.vh + self.vl
        return self.qh, self.kh, self.vh


class Case(object):
    """One launch: sequences of `lens` of one family under one bias table. Sequences of the same (family, length, index tag) are the same numbers in every layout."""

    def __init__(self, lens, family, table, tags=None):
        self.lens, self.family, self.table = list(lens), family, table
        self.lay = Lay(self.lens)
        tags = tags or list(range(len(lens)))
        self.seqs = [_seq(family, T, tag) for T, tag in zip(self.lens, tags)]
        self.bias = bias_table(table)

    def name(self):
        return "%s/%s T=%s" % (self.family, self.table, ",".join(map(str, self.lens)))

    def images(self, poison):
        """-> dict(qk, qk_lo [rows + 128][2048], vt, vt_lo [1024][rows + 128]) of fp16 bit patterns"""
        if getattr(self, "_im", None) is not None and self._im[0] == poison:
            return self._im[1]  # the last image is kept: a case is launched several times in a row
        R = self.lay.rows + 128
        qk = np.zeros((2, R, NH, 2, HD), np.float64)
        vt = np.zeros((2, NH, HD, R), np.float64)
        if poison:
            rng = np.random.RandomState(_seed("poison", self.name()))
            qk[:] = POISON * rng.choice([-1.0, 1.0], qk.shape)  # the low halves too
            vt[:] = POISON * rng.choice([-1.0, 1.0], vt.shape)
        for s, sq in enumerate(self.seqs):
            n = sq.T if poison else sq.T + 1  # unpoisoned: the guard row holds key T of the family
            r0 = int(self.lay.start[s])
            for i, (q, k, v) in enumerate(((sq.qh, sq.kh, sq.vh), (sq.ql, sq.kl, sq.vl))):
                qk[i, r0:r0 + n, :, 0] = q[:, :n].transpose(1, 0, 2)
                qk[i, r0:r0 + n, :, 1] = k[:, :n].transpose(1, 0, 2)
                vt[i, :, :, r0:r0 + n] = v[:, :n].transpose(0, 2, 1)
        qb, vb = bits(qk).reshape(2, R, 2048), bits(vt).reshape(2, CH, R)
        self._im = (poison, dict(qk=np.ascontiguousarray(qb[0]), qk_lo=np.ascontiguousarray(qb[1]), vt=np.ascontiguousarray(vb[0]), vt_lo=np.ascontiguousarray(vb[1])))
        return self._im[1]


_seqs = {}


def _seq(family, T, tag):
    key = (family, T, tag)
    if key not in _seqs:
        if len(_seqs) > 64:
            _seqs.clear()
        _seqs[key] = Seq(family, T, tag)
    return _seqs[key]


def single(T, cfg):
    return Case([T], cfg[0], cfg[1])


def triple(lens, cfg):
    return Case(lens, cfg[0], cfg[1])


def alone(c, s):
    """sequence s of case c in a single-sequence layout (the same numbers)"""
    o = Case.__new__(Case)
    o.lens, o.family, o.table = [c.lens[s]], c.family, c.table
    o.lay, o.seqs, o.bias, o._im = Lay(o.lens), [c.seqs[s]], c.bias, None
    return o


class Out(object):
    def __init__(self, hi, lo, launch):
        self.hi, self.lo, self.launch = hi, lo, launch

    def canaries_intact(self):
        return self.hi.canaries_intact() and (self.lo is None or self.lo.canaries_intact())

    def rows(self, which="hi"):
        """layout rows [rows][1024] uint16 (buffer rows 1 .. rows)"""
        g = self.hi if which == "hi" else self.lo
        return g.payload[1:-1]

    def value(self, f32):
        v = self.rows().view(np.float16).astype(np.float64)
        return v + self.lo.payload[1:-1].view(np.float16).astype(np.float64) if f32 else v


def run(c, kind, poison=False):
    """Launch case c once. -> Out (canaries asserted by the caller)"""
    lay = c.lay
    im = c.images(poison)
    hi = Guarded((lay.rows + 2, CH), np.uint16)
    lo = Guarded((lay.rows + 2, CH), np.uint16) if kind == F32 else None
    launch = np.zeros(4, np.int32)
    cs = struct(kind, ns=lay.ns, rows=lay.rows, ldvt=lay.rows + 128, qk_rows=lay.rows + 128, out_rows=lay.rows + 2, start=lay.start, len=lay.len,
                qk=im["qk"], vt=im["vt"], qk_lo=im["qk_lo"] if kind == F32 else None, vt_lo=im["vt_lo"] if kind == F32 else None,
                bias_tab=c.bias, out=hi, out_lo=lo, launch=launch)
    rc = harness().tts_dattn_test_run(C.byref(cs))
    if rc != 0:
        raise HipError("%s %s: HIP error %d" % (KIND_NAMES[kind], c.name(), rc))
    return Out(hi, lo, launch)


# ---------------------------------------------------------------------------------------------------------------- reference and mutations

MUTATIONS = ["drop_last", "admit_T", "drop_key0", "drop_first_of_last_tile", "sides_swapped", "saturate_62", "saturate_64", "distance_plus_1",
             "far_below_one_tile_late", "far_above_one_tile_early", "v_halves_swapped", "bias_of_head_xor_1", "scale_sqrt63"]


def bias_index(T, mut=None, QW=32):
    """idx [T, T + 1] into a head's 128 bias entries for query t, key j (correct, or as mutation `mut` would read it)"""
    t, j = np.arange(T)[:, None], np.arange(T + 1)[None, :]
    d = j - t + (1 if mut == "distance_plus_1" else 0)
    sat = 62 if mut == "saturate_62" else 64 if mut == "saturate_64" else 63
    side = (d > 0) != (mut == "sides_swapped")
    idx = (np.where(side, 64, 0) + np.minimum(np.abs(d), sat)) % 128
    if mut in ("far_below_one_tile_late", "far_above_one_tile_early"):
        for qw in range(0, T, QW):
            a, b, last, nkb = tile_bounds(qw, QW, T)
            rows = slice(qw, min(qw + QW, T))
            if mut == "far_below_one_tile_late":
                idx[rows, :min((a + 1) * 64, T + 1)] = 63
            else:
                idx[rows, max(b - 1, 0) * 64:] = 64 + 63
    return idx


@one_thread
def reference(sq, bias, f32=False, mut=None):
    """One sequence in float64 -> dict(out [16, T, 64], p, s [16, T, T + 1] (column T: the guard row's key, weight 0 unless a mutation admits it), M [16, T, 1])"""
    key = (id(bias), f32, mut)
    if mut is None and key in sq._ref and sq._ref[key][0] is bias:
        return sq._ref[key][1]
    T = sq.T
    q, k, v = sq.operands(f32)
    idx = bias_index(T, mut)
    b = np.asarray(bias, np.float64)
    if mut == "bias_of_head_xor_1":
        b = b[np.arange(NH) ^ 1]
    scale = 1.0 / np.sqrt(63.0) if mut == "scale_sqrt63" else 0.125
    s = np.matmul(q[:, :T], k.transpose(0, 2, 1)) * scale + b[:, idx]
    vis = np.ones((T, T + 1), bool)
    vis[:, T] = mut == "admit_T"
    if mut == "drop_last":
        vis[:, T - 1] = False
    elif mut == "drop_key0":
        vis[:, 0] = False
    elif mut == "drop_first_of_last_tile":
        vis[:, (T - 1) // 64 * 64] = False
    vv = v
    if mut == "v_halves_swapped":
        jj = np.arange(T + 1)
        sw = np.where((jj ^ 4) < T, jj ^ 4, jj)
        sw[T] = T
        vv = v[:, sw]
    with np.errstate(invalid="ignore", divide="ignore"):
        sm = np.where(vis[None], s, -np.inf)
        M = sm.max(axis=2, keepdims=True)
        w = np.exp(sm - np.where(np.isfinite(M), M, 0.0))
        L = w.sum(axis=2, keepdims=True)
        p = w / L
        out = np.matmul(p, vv)
    r = dict(out=out, p=p, s=s, M=M, L=L, w=w, b=b[:, idx])
    if mut is None:
        sq._ref[key] = (bias, r)
    return r


def running_gap(r, T):
    """e^(m_j - M) [16, T, T + 1]: m_j the running maximum over the tiles up to key j's, in the exact arithmetic"""
    nt = (T + 63) // 64
    s = np.full((NH, T, nt * 64), -np.inf)
    s[:, :, :T] = r["s"][:, :, :T]
    m = np.maximum.accumulate(s.reshape(NH, T, nt, 64).max(axis=3), axis=2)
    g = np.exp(m - r["M"])
    return np.concatenate([np.repeat(g, 64, axis=2)[:, :, :T], np.zeros((NH, T, 1))], axis=2)  # column T (the guard row's key): no weight


def ulp16(x):
    x = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(x > 0, x, 1.0)))
    return np.maximum(2.0 ** (np.where(x > 0, e, -30.0) - 10.0), 2.0 ** -24)


def rn16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _common(sq, bias, f32):
    T = sq.T
    r = reference(sq, bias, f32)
    q, k, v = sq.operands(f32)
    A = np.matmul(np.abs(q[:, :T]), np.abs(k).transpose(0, 2, 1)) / 8.0
    gap = np.abs(np.where(r["p"] > 0, r["s"] - r["M"], 0.0))  # only where the weight is not exactly 0 (column T)
    nt = (T + 63) // 64
    later = nt - 1 - np.minimum(np.arange(T + 1) // 64, nt - 1)
    g = running_gap(r, T)
    return T, r, np.abs(v), A, gap, nt, later, g


@one_thread
def bound16(sq, bias):
    """The module docstring's bound of the fp16 kernels for one sequence: [16, T, 64] float64"""
    T, r, va, A, gap, nt, later, g = _common(sq, bias, False)
    eps = 64 * U * A + U * (2 * np.abs(r["s"]) + 2 * np.abs(r["b"]) + np.abs(r["M"])) + 3 * U * gap + (1 + later)[None, None, :] * E2 + 2.0 ** -11
    e = r["p"] * eps + 2.0 ** -25 * g / r["L"]
    e[:, :, T] = 0.0
    o = np.abs(r["out"])
    B = np.matmul(r["p"], va)
    pre = np.matmul(e, va) + o * e.sum(axis=2, keepdims=True) + U * (65 * nt * B + (65 * nt + 4) * o)
    return pre + 0.5 * ulp16(o + pre)


@one_thread
def bound32(sq, bias):
    """The module docstring's bound of the split-precision kernel for one sequence: [16, T, 64] float64"""
    T, r, va, A, gap, nt, later, g = _common(sq, bias, True)
    eps = (2.0 ** -22 + 192 * U) * A + U * (np.abs(r["s"]) + 3 * gap + 6) + (1 + later)[None, None, :] * E2
    e = r["p"] * eps
    e[:, :, T] = 0.0
    e2 = 2.0 ** -21 * r["p"] + 2.0 ** -33 * g / r["L"]
    e2[:, :, T] = 0.0
    o = np.abs(r["out"])
    B = np.matmul(r["p"], va)
    return (np.matmul(e, va) + o * e.sum(axis=2, keepdims=True) + np.matmul(e2, va) + U * (193 * nt * B + (18 * nt + 6) * o)
            + 2.0 ** -22 * o + 2.0 ** -25)


def bound(sq, bias, kind):
    return bound32(sq, bias) if kind == F32 else bound16(sq, bias)


def wide_condition(sq, bias):
    """the share of (query, key) weights below 2^-14 of the running maximum at their tile"""
    r = reference(sq, bias)
    T = sq.T
    g = running_gap(r, T)[:, :, :T]
    with np.errstate(divide="ignore"):
        rel = r["w"][:, :, :T] / g  # e^(s - m_j)
    return float((rel < 2.0 ** -14).mean())


def ratios(c, value, kind):
    """value [rows][1024] float64 (the output, out_hi + out_lo for F32) -> per sequence (|err| / bound [16, T, 64], reference, output)"""
    res = []
    for s, sq in enumerate(c.seqs):
        o = value[c.lay.seq_rows(s)].reshape(sq.T, NH, HD).transpose(1, 0, 2)
        ref = reference(sq, c.bias, kind == F32)["out"]
        bd = bound(sq, c.bias, kind)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(o == ref, 0.0, np.abs(o - ref) / bd)
            r = np.where(np.isfinite(o), r, np.inf)
        res.append((r, ref, o))
    return res


# ---------------------------------------------------------------------------------------------------------------- NumPy restatements of the kernels' arithmetic

@one_thread
def restate16(sq, bias):
    """diff_attn_kernel's arithmetic in float32 NumPy: f32 scores, tile-wise running maximum, fp16 weights, row sums of the ROUNDED weights -> fp16 values
    [16, T, 64] as float64"""
    f = np.float32
    T = sq.T
    q, k, v = sq.qh[:, :T].astype(f), sq.kh.astype(f), sq.vh.astype(f)
    L2E = f(1.44269504088896)
    SC = f(0.125) * L2E
    tab = np.asarray(bias, f)[:, bias_index(T)] * (L2E / SC)
    o, l, m = np.zeros((NH, T, HD), f), np.zeros((NH, T, 1), f), np.full((NH, T, 1), -np.inf, f)
    with np.errstate(invalid="ignore", over="ignore"):
        for kb in range((T + 63) // 64):
            js = slice(kb * 64, min(kb * 64 + 64, T))
            val = np.matmul(q, k[:, js].transpose(0, 2, 1)) + tab[:, :, js]
            mnew = np.maximum(m, val.max(axis=2, keepdims=True) * SC)
            alpha = np.exp2(m - mnew)
            p = np.exp2(val * SC - mnew).astype(np.float16).astype(f)
            o = o * alpha + np.matmul(p, v[:, js])
            l = l * alpha + p.sum(axis=2, keepdims=True, dtype=f)
            m = mnew
        return (o * (f(1.0) / l)).astype(np.float16).astype(np.float64)


@one_thread
def restate32(sq, bias):
    """diff_attn_f32_kernel's arithmetic in float32 NumPy: three partial products per matrix product, unrounded row sums, split weights, a split output
    -> out_hi + out_lo [16, T, 64] as float64"""
    f = np.float32
    T = sq.T
    qh, ql, kh, kl, vh, vl = (a.astype(f) for a in (sq.qh[:, :T], sq.ql[:, :T], sq.kh, sq.kl, sq.vh, sq.vl))
    L2E = f(1.44269504088896)
    tab = np.asarray(bias, f)[:, bias_index(T)]
    o, l, m = np.zeros((NH, T, HD), f), np.zeros((NH, T, 1), f), np.full((NH, T, 1), -np.inf, f)
    tr = lambda a: a.transpose(0, 2, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for kb in range((T + 63) // 64):
            js = slice(kb * 64, min(kb * 64 + 64, T))
            S = np.matmul(qh, tr(kl[:, js])) + np.matmul(ql, tr(kh[:, js])) + np.matmul(qh, tr(kh[:, js]))
            val = S * f(0.125) + tab[:, :, js]
            mnew = np.maximum(m, val.max(axis=2, keepdims=True))
            alpha = np.exp2((m - mnew) * L2E)
            p = np.exp2((val - mnew) * L2E + f(8.0))
            ph = p.astype(np.float16).astype(f)
            pl = (p - ph).astype(np.float16).astype(f)
            o = o * alpha + (np.matmul(ph, vl[:, js]) + np.matmul(pl, vh[:, js]) + np.matmul(ph, vh[:, js]))
            l = l * alpha + p.sum(axis=2, keepdims=True, dtype=f)
            m = mnew
        val = o * (f(1.0) / l)
        hi = val.astype(np.float16).astype(f)
        lo = (val - hi).astype(np.float16).astype(f)
        return hi.astype(np.float64) + lo.astype(np.float64)
