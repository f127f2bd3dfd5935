"""Shared by tests/test_bvg_kernels_gpu.py and tests/test_bvg_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/bvg_harness.hip -> libtts_bvg_test.so), float64 NumPy references of the BigVGAN vocoder's three kernels (csrc/bigvgan.h), the case
matrix, the acceptance rule and its error bound, float32 restatements in another summation order, and the defects the rule must reject.

LAYOUT, as bigvgan_run builds it: candidate s owns the rows [start_s R, (start_s + T_s) R) of a buffer with R rows per frame, start = the running sum of
ceil8(T). The input rows that belong to no candidate hold 3.5 (NaN in the poisoned twin); the output starts as the sentinel byte everywhere.

REFERENCES are float64 on the values the kernel multiplies: the taps, alpha and 1 / (beta + 1e-9) are the float32 numbers the device holds, widened, so that the
bound covers arithmetic only. The activation, with cl(i, n) = min(max(i, 0), n - 1) and R the CANDIDATE's rows:
      u[m] = 2 sum_j x[cl(j, R)] f[m + 5 - 2 j],   s = u + sin^2(alpha u) ib,   y[t] = sum_k f[k] s[cl(2 t + k - 5, 2 R)].

ACCEPTANCE, first order and term by term, nothing fitted; U = 2^-24. A chain of n fused multiply-adds rounds n times, each time a partial sum of at most
A = sum |terms|: n U A.
      e_u   = 6 U A_u                                   A_u = 2 sum |x| |f|  (the final doubling is exact)
      e_arg = alpha e_u + U |alpha u|                   the product's rounding: the argument is unbounded, its ABSOLUTE error grows with it, and that is real
      e_sin = e_arg + SIN_ULP 2 U |sin|                 |sin'| <= 1
      e_sq  = 2 |sin| e_sin + e_sin^2 + U sin^2
      e_s   = e_u + ib e_sq + U (|u| + sin^2 ib)        one fused multiply-add
      e_y   = sum_k |f[k]| e_s[k] + 12 U sum_k |f[k] s[k]|
SIN_ULP = 2: device sinf, in ulp. Source: the HIP math API reference's table of maximum ulp errors of the single-precision device functions, which OCML
implements (the source of hfg_cases.py's TANH_ULP and of voc_cases.py's sincosf figure, 2 ulp; sinf is listed no higher).
bvg_post_kernel: the activation's e_y carried through the 7 x C products, plus a chain of n = 7 C fused multiply-adds started from the bias,
      bound = sum |w| e_y + n U (sum |a w| + |b|) + TANH_ULP 2 U |tanh| + 2^-126          (|tanh'| <= 1)
bvg_mel_kernel is ONE chain, fma(fl(fl(m + 1) 0.5), fl(MAX - MIN), MIN): restated exactly (rational arithmetic, one rounding per operation) and compared bit for bit.

DEFECTS are applied to the reference (reference(mut=...)); test_bvg_harness_cpu.py requires each to leave the bound of the unmutated reference on some case."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

f32, f64, i32 = np.float32, np.float64, np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
SRC = os.path.join(PKG, "testlib", "bvg_harness.hip")
LIB = os.environ.get("TTS_BVG_TEST_LIB", os.path.join(PKG, "libtts_bvg_test.so"))
ACT, MEL, POST = 0, 1, 2
KIND_NAMES = {ACT: "bvg_act_kernel", MEL: "bvg_mel_kernel", POST: "bvg_post_kernel"}
HIP_INVALID_VALUE = 1
SENTINEL = 0xCB
SEQ = 9
U = 2.0 ** -24
FMIN = 2.0 ** -126
SIN_ULP = 2.0   # device sinf, in ulp (module docstring)
TANH_ULP = 2.0  # device tanhf, in ulp (hfg_cases.py)
JUNK = f32(3.5)
MAXV, MINV = f32(2.3143386840820312), f32(-11.512925148010254)
# the literals of csrc/bigvgan.h's BVG_F, as the float32 numbers the device holds
TAPS = np.array([0.0020289664498962, 0.0093894639440679, -0.0255434640652947, -0.0576573754753650, 0.1285726090813288, 0.4432098000653667,
                 0.4432098000653667, 0.1285726090813288, -0.0576573754753650, -0.0255434640652947, 0.0093894639440679, 0.0020289664498962], f64).astype(f32)
RUN, BLOCK = 64, 512  # rows of one thread / one workgroup of bvg_act_kernel (checked against the library: tts_bvg_test_run_rows / _block_rows)


class CaseStruct(C.Structure):
    _fields_ = [("kind", C.c_int), ("ns", C.c_int), ("frames", C.c_int), ("C", C.c_int), ("rate", C.c_int),
                ("T", C.c_void_p), ("start", C.c_void_p), ("in_", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("alpha", C.c_void_p),
                ("inv_beta", C.c_void_p), ("out", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_bvg_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_bvg_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_bvg_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_bvg_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_bvg_test_table.argtypes = [C.POINTER(CaseStruct), C.c_void_p]
        L.tts_bvg_test_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
        L.tts_bvg_test_packed.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong]
        L.tts_bvg_test_packed.restype = C.c_longlong
        for f in (L.tts_bvg_test_run, L.tts_bvg_test_validate, L.tts_bvg_test_table, L.tts_bvg_test_parse, L.tts_bvg_test_margin, L.tts_bvg_test_run_rows,
                  L.tts_bvg_test_block_rows):
            f.restype = C.c_int
        _lib = L
    return _lib


def parse(path):
    """the loader's host half on a file: (status, [C0, stages, 6 strides, 7 padded channel counts], message)"""
    out, err = np.zeros(15, i32), C.create_string_buffer(512)
    rc = harness().tts_bvg_test_parse(path.encode(), out.ctypes.data_as(C.c_void_p), err, 512)
    return rc, out, err.value.decode()


def packed(path, which, i=0, j=0, n=0):
    L = harness()
    cnt = L.tts_bvg_test_packed(path.encode(), which, i, j, n, None, 0)
    assert cnt > 0, cnt
    out = np.zeros(cnt, f32)
    assert L.tts_bvg_test_packed(path.encode(), which, i, j, n, out.ctypes.data_as(C.c_void_p), cnt) == cnt
    return out


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape):
        self.margin = harness().tts_bvg_test_margin()
        self.shape = shape
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * 4, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(f32).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


class Case(object):
    def __init__(self, kind, T, C_=32, rate=1, start=None, frames=None, fam="gauss", seed=0):
        self.kind, self.T, self.C, self.fam, self.seed = kind, list(T), C_, fam, seed
        self.rate = 256 if kind == POST else 1 if kind == MEL else rate
        self.start, run = [], 0
        for s, t in enumerate(self.T):
            st = run if start is None else start[s]
            self.start.append(st)
            run = st + (t + 7) // 8 * 8
        self.frames = run if frames is None else frames
        self.before = [int(v) for v in np.cumsum([0] + self.T[:-1])]
        self.explicit_start = start is not None
        self.a = {}

    @property
    def ns(self):
        return len(self.T)

    def rows(self, s, R=None):
        R = self.rate if R is None else R
        return slice(self.start[s] * R, (self.start[s] + self.T[s]) * R)

    def live(self, R=None):
        R = self.rate if R is None else R
        m = np.zeros(self.frames * R, bool)
        for s in range(self.ns):
            m[self.rows(s, R)] = True
        return m

    def table(self):
        t = np.zeros((self.ns, SEQ), i32)
        for s in range(self.ns):
            t[s, 0], t[s, 1], t[s, 5], t[s, 8] = self.start[s], self.T[s], self.before[s], self.T[s]
        return t

    def name(self):
        return "%s T%s C%d R%d %s%s" % (KIND_NAMES[self.kind][4:-7], "-".join(map(str, self.T)), self.C, self.rate, self.fam, "" if not self.explicit_start else " start" + str(self.start))


def make(kind, T, C_=32, rate=1, start=None, frames=None, fam="gauss", seed=0):
    """fam: gauss = unit-scale rows, a, b ~ 0.3 N; big = rows x 20 and a ~ 1 + 0.3 N (|alpha u| reaches the hundreds: the accurate sine's range reduction);
    const = every row of a candidate equal (the up-sampler must pass it unchanged)"""
    c = Case(kind, T, C_, rate, start, frames, fam, seed)
    rs = np.random.RandomState(1000 * kind + 31 * seed + sum(c.T) + 7 * c.C + c.rate)
    if kind == MEL:
        c.a["in_"] = np.clip(rs.randn(100 * sum(c.T)) * 0.6, -1.5, 1.5).astype(f32)
        c.a["in_"][:3] = (-1.0, 1.0, f32(-1 + 2.0 ** -20))
        return c
    scale = 20.0 if fam == "big" else 1.5
    x = (rs.randn(c.frames * c.rate, c.C) * scale).astype(f32)
    if fam == "const":
        for s in range(c.ns):
            x[c.rows(s)] = x[c.rows(s)][0]
    x[~c.live()] = JUNK
    c.a["in_"] = x
    c.a["alpha"] = np.exp((1.0 if fam == "big" else 0.0) + 0.3 * rs.randn(c.C)).astype(f32)
    c.a["inv_beta"] = (1.0 / (np.exp(0.3 * rs.randn(c.C)) + 1e-9)).astype(f32)
    if kind == POST:
        c.a["w"] = (rs.randn(7, c.C) / np.sqrt(7 * c.C) * 0.5).astype(f32)
        c.a["bias"] = np.array([0.1], f32)
    return c


def poisoned(c):
    """the same case with NaN on every input row outside the candidates (None where there is none): a kernel that clamps to the candidate never reads them"""
    if c.kind == MEL or c.live().all():
        return None
    p = Case(c.kind, c.T, c.C, c.rate, c.start, c.frames, c.fam, c.seed)
    p.a = dict(c.a)
    p.a["in_"] = c.a["in_"].copy()
    p.a["in_"][~c.live()] = np.nan
    return p


def alone(c, s):
    """candidate s of the case as a batch of one (its rows, its parameters)"""
    p = Case(c.kind, [c.T[s]], c.C, c.rate, None, None, c.fam, c.seed)
    p.a = dict(c.a)
    if c.kind == MEL:
        p.a["in_"] = c.a["in_"][100 * c.before[s]:100 * (c.before[s] + c.T[s])].copy()
    else:
        x = np.full((p.frames * p.rate, c.C), JUNK, f32)
        x[p.rows(0)] = c.a["in_"][c.rows(s)]
        p.a["in_"] = x
    return p


def out_shape(c):
    return (c.frames * c.rate, c.C) if c.kind == ACT else (c.frames, 128) if c.kind == MEL else (sum(c.T) * 256,)


def to_struct(c, out):
    cs = CaseStruct()
    cs._keep = [out]
    cs.kind, cs.ns, cs.frames, cs.C, cs.rate = c.kind, c.ns, c.frames, c.C, c.rate
    arrs = dict(T=np.array(c.T, i32), start=np.array(c.start, i32) if c.explicit_start else None)
    for k in ("in_", "w", "bias", "alpha", "inv_beta"):
        arrs[k] = None if c.a.get(k) is None else np.ascontiguousarray(c.a[k], f32)
    for k, v in arrs.items():
        if v is not None:
            cs._keep.append(v)
            setattr(cs, k, v.ctypes.data_as(C.c_void_p))
    cs.out = out.raw.ctypes.data_as(C.c_void_p)
    return cs


def run(c):
    """-> (status, Guarded) of one launch through the harness; the output buffer starts as the sentinel"""
    g = Guarded(out_shape(c))
    rc = harness().tts_bvg_test_run(C.byref(to_struct(c, g)))
    return rc, g


# ------------------------------------------------------------------------------------------------------------------------------ references

MUTS_ACT = ("no_factor2", "clamp_buffer", "pad_6_5", "swap_ab", "sin_not_sq", "zero_boundary")


def act_ref(buf, r0, R, al, ib, mut=None):
    """(y, e_y) float64 [R][C] of the candidate at rows [r0, r0 + R) of buf; al, ib float64 [C]"""
    f = TAPS.astype(f64)

    def gather(a, idx, n, base, total):
        if mut == "clamp_buffer":
            return a[np.clip(base + idx, 0, total - 1)]
        g = a[base + np.clip(idx, 0, n - 1)]
        if mut == "zero_boundary":
            g = np.where(((idx < 0) | (idx >= n))[:, None], 0.0, g)
        return g
    if mut == "swap_ab":
        al, ib = 1.0 / ib, 1.0 / al
    x = buf.astype(f64)
    xp = gather(x, np.arange(-3, R + 4), R, r0, len(x))
    u, au = np.zeros((2 * R, x.shape[1])), np.zeros((2 * R, x.shape[1]))
    for i in range(6):
        u[0::2] += xp[5 - i:5 - i + R] * f[1 + 2 * i]
        u[1::2] += xp[6 - i:6 - i + R] * f[2 * i]
        au[0::2] += np.abs(xp[5 - i:5 - i + R] * f[1 + 2 * i])
        au[1::2] += np.abs(xp[6 - i:6 - i + R] * f[2 * i])
    if mut != "no_factor2":
        u, au = 2 * u, 2 * au
    e_u = 6 * U * au
    arg = al * u
    e_arg = al * e_u + U * np.abs(arg)
    sn = np.sin(arg)
    e_sin = e_arg + SIN_ULP * 2 * U * np.abs(sn) + FMIN
    sq = sn if mut == "sin_not_sq" else sn * sn
    e_sq = 2 * np.abs(sn) * e_sin + e_sin ** 2 + U * np.abs(sq)
    s = u + sq * ib
    e_s = e_u + ib * e_sq + U * (np.abs(u) + np.abs(sq) * ib) + FMIN
    off = 6 if mut == "pad_6_5" else 5
    idx = np.arange(-off, 2 * R + 11 - off)
    sp, ep = s[np.clip(idx, 0, 2 * R - 1)], e_s[np.clip(idx, 0, 2 * R - 1)]
    if mut == "zero_boundary":
        sp = np.where(((idx < 0) | (idx >= 2 * R))[:, None], 0.0, sp)
    y, e_y, ay = np.zeros((R, x.shape[1])), np.zeros((R, x.shape[1])), np.zeros((R, x.shape[1]))
    for k in range(12):
        y += f[k] * sp[k:k + 2 * R:2]
        ay += np.abs(f[k] * sp[k:k + 2 * R:2])
        e_y += abs(f[k]) * ep[k:k + 2 * R:2]
    return y, e_y + 12 * U * ay + FMIN


def _round32(fr):
    """the float32 nearest to a Fraction (one rounding)"""
    v = f32(float(fr))
    best = min((v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))), key=lambda q: abs(Fraction(float(q)) - fr))
    return f32(best)


def mel_exact(m):
    """fma(fl(fl(m + 1) 0.5), fl(MAX - MIN), MIN), one rounding per operation, in rational arithmetic"""
    span = Fraction(float(f32(MAXV - MINV)))
    out = np.zeros(len(m), f32)
    for i, v in enumerate(m):
        h = Fraction(float(f32(f32(v) + f32(1.0)))) / 2  # the halving is exact
        out[i] = _round32(h * span + Fraction(float(MINV)))
    return out


def reference(c, mut=None):
    """dict(z, bound, live): float64 reference, its elementwise bound (0 = equality), the elements a kernel writes"""
    if c.kind == MEL:
        z = np.zeros((c.frames, 128), f64)
        for s in range(c.ns):
            m = c.a["in_"][100 * c.before[s]:100 * (c.before[s] + c.T[s])]
            z[c.rows(s, 1), :100] = mel_exact(m).reshape(100, c.T[s]).T
        live = np.repeat(c.live(1)[:, None], 128, 1)
        return dict(z=z, bound=np.zeros_like(z), live=live)
    al, ib = c.a["alpha"].astype(f64), c.a["inv_beta"].astype(f64)
    if c.kind == ACT:
        z, b = np.zeros((c.frames * c.rate, c.C)), np.zeros((c.frames * c.rate, c.C))
        for s in range(c.ns):
            sl = c.rows(s)
            z[sl], b[sl] = act_ref(c.a["in_"], sl.start, sl.stop - sl.start, al, ib, mut)
        return dict(z=z, bound=b, live=np.repeat(c.live()[:, None], c.C, 1))
    w, bias, n = c.a["w"].astype(f64), float(c.a["bias"][0]), 7 * c.C
    zs, bs = [], []
    for s in range(c.ns):
        sl = c.rows(s)
        R = sl.stop - sl.start
        a, ea = act_ref(c.a["in_"], sl.start, R, al, ib, None if mut in ("post_6taps", "post_no_tanh") else mut)
        ap = np.concatenate([np.zeros((3, c.C)), a, np.zeros((3, c.C))])
        ep = np.concatenate([np.zeros((3, c.C)), ea, np.zeros((3, c.C))])
        pre, mag, err = np.full(R, bias), np.full(R, abs(bias)), np.zeros(R)
        for tap in range(6 if mut == "post_6taps" else 7):
            pre += ap[tap:tap + R] @ w[tap]
            mag += np.abs(ap[tap:tap + R]) @ np.abs(w[tap])
            err += ep[tap:tap + R] @ np.abs(w[tap])
        z = pre if mut == "post_no_tanh" else np.tanh(pre)
        zs.append(z)
        bs.append(err + n * U * mag + TANH_ULP * 2 * U * np.abs(z) + FMIN)
    z, b = np.concatenate(zs), np.concatenate(bs)
    return dict(z=z, bound=b, live=np.ones(len(z), bool))


def restate32(c):
    """a float32 restatement of the kernel in another order of summation (taps descending, separate multiplies and adds; bvg_mel_kernel has one chain and one
    order: mel_exact); the buffer a launch would leave"""
    out = np.frombuffer(bytes([SENTINEL]) * (4 * int(np.prod(out_shape(c)))), f32).reshape(out_shape(c)).copy()
    if c.kind == MEL:
        for s in range(c.ns):
            m = c.a["in_"][100 * c.before[s]:100 * (c.before[s] + c.T[s])].reshape(100, c.T[s]).T
            out[c.rows(s, 1), :100] = mel_exact(np.ascontiguousarray(m.T).reshape(-1)).reshape(100, c.T[s]).T  # the one chain, exactly
            out[c.rows(s, 1), 100:] = 0
        return out
    al, ib, f = c.a["alpha"], c.a["inv_beta"], TAPS

    def act32(x):
        R = len(x)
        xp = x[np.clip(np.arange(-3, R + 4), 0, R - 1)]
        u = np.zeros((2 * R, x.shape[1]), f32)
        for i in reversed(range(6)):
            u[0::2] += xp[5 - i:5 - i + R] * f[1 + 2 * i]
            u[1::2] += xp[6 - i:6 - i + R] * f[2 * i]
        u *= f32(2)
        sn = np.sin(al * u)
        s = u + sn * sn * ib
        sp = s[np.clip(np.arange(-5, 2 * R + 6), 0, 2 * R - 1)]
        y = np.zeros_like(x)
        for k in reversed(range(12)):
            y += f[k] * sp[k:k + 2 * R:2]
        return y
    if c.kind == ACT:
        for s in range(c.ns):
            out[c.rows(s)] = act32(c.a["in_"][c.rows(s)])
        return out
    off = 0
    for s in range(c.ns):
        a = act32(c.a["in_"][c.rows(s)])
        R = len(a)
        ap = np.concatenate([np.zeros((3, c.C), f32), a, np.zeros((3, c.C), f32)])
        pre = np.zeros(R, f32)
        for tap in reversed(range(7)):
            pre += ap[tap:tap + R] @ c.a["w"][tap]
        out[off:off + R] = np.tanh(pre + c.a["bias"][0])
        off += R
    return out


def judge(out, ref):
    """-> (number of rejected elements, largest |err| / bound over the elements with a non-zero bound). NaN is rejected; a zero bound asks for equality."""
    o = np.asarray(out).astype(f64)
    z, b, live = ref["z"], ref["bound"], ref["live"]
    o, z, b = o[live], z[live], b[live]
    with np.errstate(invalid="ignore"):
        err = np.abs(o - z)
        bad = ~(err <= b)
        r = np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)
    return int(bad.sum()), float(np.nanmax(r)) if r.size else 0.0


def guards_ok(c, out, ref):
    """every element no kernel writes still holds the sentinel"""
    o = np.asarray(out).view(np.uint8).reshape(-1, 4)
    return bool((o[~ref["live"].reshape(-1)] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------ the case matrix

SMALL_ROWS = (1, 2, 5, 6, 10, 11, 12)       # below 11 rows both clamps reach into one window
EDGE_ROWS = (RUN - 1, RUN, RUN + 1, BLOCK - 1, BLOCK, BLOCK + 1)
RAGGED = dict(T=(5, 1, 13), rate=8)          # rows 40, 8, 104


def cases(kind):
    out = []
    if kind == ACT:
        for rows in SMALL_ROWS + EDGE_ROWS:
            out.append(make(ACT, (1,), 32, rows, seed=rows))
        for C_ in (64, 96):
            for rows in (1, 5, 11, RUN + 1, BLOCK + 1):
                out.append(make(ACT, (1,), C_, rows, seed=rows))
        for C_ in (32, 64, 96):
            out.append(make(ACT, RAGGED["T"], C_, RAGGED["rate"], seed=3))
        out.append(make(ACT, RAGGED["T"], 64, RAGGED["rate"], start=(8, 24, 32), frames=48, seed=4))   # a gap in front of and between the candidates
        out.append(make(ACT, (2, 3), 32, 70, fam="big", seed=5))
        out.append(make(ACT, (1,), 64, 200, fam="big", seed=6))
        out.append(make(ACT, (3, 1), 32, 4, fam="const", seed=7))
    elif kind == MEL:
        for T in (1, 7, 8, 9):
            out.append(make(MEL, (T,), seed=T))
        out.append(make(MEL, (7, 1, 9), seed=2))
    else:
        out.append(make(POST, (1, 3), 32, seed=1))
        out.append(make(POST, (3,), 64, seed=2))
        out.append(make(POST, (1,), 32, fam="big", seed=3))
    return out
