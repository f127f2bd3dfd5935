"""Shared by tests/test_enc_harness_cpu.py and tests/test_enc_kernels_gpu.py: the binding of the test-only harness around the kernels of csrc/extras.hip and
csrc/cvvp.hip (tortoise.cpp_amd/testlib/enc_harness.hip -> libtts_enc_test.so), the case matrix, float64 references, derived error bounds, a NumPy float32
restatement of each kernel's operation order, and seeded defects of the references (`mut`).

References are float64 ON THE VALUES A KERNEL HOLDS (fp16 inputs as they are, f32 inputs as they are): quantisation of inputs is in no kernel's error.
Bounds are first order, term by term from the kernel's operation order, on the reference's own |terms| (DESIGN.md "What pins the CLVP / CVVP / voice-encoder
kernels" has the argument); u = 2^-24, gamma_m = m u / (1 - m u) for m f32 roundings in a chain (FMA contraction either way: a contracted product saves a rounding).
Nothing here is fitted to GPU output.

  embed, mel_rows, im2col3, im2col5   no arithmetic beyond one fp16 rounding: bit for bit.
  rmsnorm    relative: gamma_(K+9) / 2 (sum of squares: K = dim / 256 terms a thread, the square, the 8 adds of block_sum; halved by the root) + sqrtf + rsqrtf
             + their product + the division + the two products.
  LayerNorm  (rownorm, pool, groupnorm) two pass: dmean = gamma_m sum|x| / N + DIV |mean|; d = x - mean carries dmean + u |d|; the second sum carries
             sum 2 |d| dd + gamma_(m+1) sum d^2; var + eps: the division, the add, the f32 constant; rstd: dv / (2 v) + rsqrtf; the output: |w| rstd dd
             + |t| (e_rstd + 2u) + u |out|. pool adds gamma_n sum_r |val_r| / n and the division; groupnorm has m = ceil(T / SW) + 8, N = G T.
  rowmean    gamma_n sum |x| / n + DIV |ref|.
  geglu      s = 1 + erf(x), x = g / sqrt 2: ds = 16 ulp(erf) + 2u |x| erf'(x) + u s; y = u (0.5 g s): |u| (0.5 |g| ds + u |0.5 g s|) + u |y|.
  attention  see attn_reference().
  fp16 out   the f32 chain's bound b plus half an fp16 ulp taken at |ref| + b."""
import ctypes as C
import math
import os
import zlib

import numpy as np

from ar_attn_cases import E2 as _E2_AR  # the project's figure for an exponential: 1e-6 relative (ar_attn_cases.py, gn_cases.py, dattn_cases.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB_PATH = os.path.join(PKG, "libtts_enc_test.so")
SRC = os.path.join(PKG, "testlib", "enc_harness.hip")
EMBED, RMSNORM, ATTN, GEGLU, POOL, MEL_ROWS, GROUPNORM, IM2COL3, IM2COL5, ROWNORM, ROWMEAN = range(11)
ROT64, PLAIN64, BIAS128 = 0, 1, 2
OP_NAMES = ["clvp_embed_kernel", "clvp_rmsnorm_kernel", "clvp_attn_kernel", "clvp_geglu_kernel", "clvp_pool_kernel", "venc_mel_rows_kernel", "venc_groupnorm_kernel",
            "dcond_im2col_kernel", "cvvp_im2col5_kernel", "cvvp_rownorm_kernel", "cvvp_rowmean_kernel"]
ATTN_NAMES = ["clvp_attn_kernel<true,64,false>", "clvp_attn_kernel<false,64,false>", "clvp_attn_kernel<false,128,true>"]
F16_OUT = {RMSNORM, ATTN, GEGLU, MEL_ROWS, GROUPNORM, IM2COL3, IM2COL5, ROWNORM}
COPY_OPS = {EMBED, MEL_ROWS, IM2COL3, IM2COL5}
HIP_INVALID = 1
SENTINEL = 0xCB
MAX_SEQ, MAX_ROWS, MAX_COLS, MAX_VOCAB = 8, 1100, 3072, 512
U = 2.0 ** -24
ULP = 2.0 * U  # one f32 ulp, relative, at most
# ---- what a library function is charged, relative to its value (one table; the source of each figure) ----
EXPF = _E2_AR        # expf: the project's figure for the library exponential (ar_attn_cases.E2, "the library expf ... is charged the same")
EXP2F = 3 * ULP      # exp2f: OpenCL full profile, 3 ulp
COSF = 4 * ULP       # cosf, sinf: OpenCL full profile, 4 ulp
SINF = 4 * ULP
ERFF = 16 * ULP      # erff: OpenCL full profile, 16 ulp
RSQRTF = 2 * ULP     # rsqrtf: OpenCL full profile, 2 ulp
SQRTF = 2 * U        # sqrtf: gn_cases.py ("an IEEE division or square root 2u")
DIV = 2 * U          # division: gn_cases.py, the same line
SECOND = 1.0 + 2.0 ** -10  # the second-order terms a first-order bound leaves out: products of two of the charges above, each below 2^-10 of a first-order term


class HipError(RuntimeError):
    pass


class _Case(C.Structure):
    _fields_ = [("op", C.c_int), ("variant", C.c_int), ("nseq", C.c_int), ("rows", C.c_int), ("dim", C.c_int), ("kpad", C.c_int), ("vocab", C.c_int),
                ("out_rows", C.c_int), ("poison", C.c_int), ("in_count", C.c_longlong), ("start", C.c_void_p), ("len", C.c_void_p), ("out_start", C.c_void_p),
                ("out_len", C.c_void_p), ("tok", C.c_void_p), ("mel_off", C.c_void_p), ("in_", C.c_void_p), ("p0", C.c_void_p), ("p1", C.c_void_p), ("out", C.c_void_p)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        L.tts_enc_test_out_bytes.restype = C.c_longlong
        _lib = L
    return _lib


class Case:
    """op and, by op (enc_harness.hip: tts_enc_case): x (the input array), variant, dim, rows, start / len, out_start / out_len / out_rows / kpad, tok / vocab,
    mel_off, p0 / p1, poison"""

    def __init__(self, op, family="", **p):
        self.op, self.family, self.p = op, family, p

    def __getattr__(self, k):
        try:
            return self.__dict__["p"][k]
        except KeyError:
            raise AttributeError(k)

    def kernel(self):
        if self.op == ATTN:
            return ATTN_NAMES[self.p["variant"]]
        if self.op == GROUPNORM:
            return "venc_groupnorm_kernel<%d>" % self.p["dim"]
        if self.op == IM2COL3:
            return "dcond_im2col_kernel<%s>" % ("true" if self.p.get("variant") else "false")
        return OP_NAMES[self.op]

    def name(self):
        q = {k: (v if np.ndim(v) == 0 else list(np.asarray(v).ravel()[:8])) for k, v in self.p.items() if k not in ("x", "p0", "p1", "tok", "clips", "mel_off")}
        return "%s %s %s" % (self.kernel(), self.family, q)

    def struct(self, out_ptr=1, **override):
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data

        p, c = self.p, _Case()
        c.op = self.op
        for k in ("variant", "nseq", "rows", "dim", "kpad", "vocab", "out_rows", "poison"):
            setattr(c, k, int(p.get(k, 0)))
        x = p["x"]
        c.in_ = arr(x, x.dtype)
        c.in_count = x.size if "mel_off" in p else 0
        for k in ("start", "len", "out_start", "out_len", "tok"):
            if p.get(k) is not None:
                setattr(c, k, arr(p[k], np.int32))
        if p.get("mel_off") is not None:
            c.mel_off = arr(p["mel_off"], np.int64)
        for k in ("p0", "p1"):
            if p.get(k) is not None:
                setattr(c, k, arr(p[k], np.float32))
        c.out = out_ptr
        for k, v in override.items():
            setattr(c, k, v)
        return c, keep


class Out:
    def __init__(self, raw, margin, nbytes, f16):
        self.raw, self.margin = raw, margin
        self.payload = raw[margin:margin + nbytes].view(np.uint16 if f16 else np.uint32).copy()  # bits

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


def validate(case, **override):
    c, keep = case.struct(**override)
    return lib().tts_enc_test_validate(C.byref(c))


def run(case):
    """launches the case once; HipError for anything but success (a refused case included)"""
    L = lib()
    c, keep = case.struct()
    nbytes = L.tts_enc_test_out_bytes(C.byref(c))
    if nbytes < 0:
        raise HipError("%s: refused (%d)" % (case.name(), nbytes))
    margin = L.tts_enc_test_margin()
    raw = np.zeros(nbytes + 2 * margin, np.uint8)
    c.out = raw.ctypes.data
    rc = L.tts_enc_test_run(C.byref(c))
    if rc != 0:
        raise HipError("%s: HIP error %d" % (case.name(), rc))
    return Out(raw, margin, nbytes, case.op in F16_OUT)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def gamma(m):
    return m * U / (1.0 - m * U)


def ulp32(x):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 23)


def ulp16(x):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14))) - 10)


def rn16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def f16_out(ref, b):
    """the bound of an fp16 output whose f32 chain is within b of ref"""
    return b + 0.5 * ulp16(np.abs(ref) + b)


def values(bits, f16):
    """the float64 values of a payload's bits"""
    return bits.view(np.float16 if f16 else np.float32).astype(np.float64)


def judge(got, ref, bound):
    """(elements outside the bound, largest |err| / bound); a NaN is outside"""
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        bad = int((~(err <= bound)).sum())
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(r), np.inf, r)
    return bad, float(r.max()) if r.size else 0.0


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def _rng(*parts):
    return np.random.RandomState(_seed(*parts))


def layout(lens, first=0, tail=0):
    start, r = [], first
    for n in lens:
        start.append(r)
        r += n
    return np.array(start, np.int32), np.array(lens, np.int32), r + tail


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the block_sum tree of both files, float32: 256 lane values -> the workgroup's sum
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def block_sum32(v):
    v = np.asarray(v, np.float32).reshape(4, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    red = v[:, 0]
    return np.float32(np.float32(red[0] + red[1]) + np.float32(red[2] + red[3]))


def _lanes32(row_fn, count, stride=256):
    """per-thread strided f32 partial sums: thread t takes elements t, t + stride, ... of row_fn(indices) in order"""
    acc = np.zeros(stride, np.float32)
    for i0 in range(0, count, stride):
        idx = np.arange(i0, min(i0 + stride, count))
        acc[:len(idx)] = acc[:len(idx)] + row_fn(idx)
    return acc


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# rmsnorm
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
DIMS = [128, 512, 640, 768, 896, 1024]
ROW_KINDS = ["gauss", "offset", "outlier"]


def norm_rows(dim, seed, zero=False):
    """the rows of the issue: Gaussian, offset (mean 100 x std), one outlier of 1e4 (and, for rmsnorm, the all-zero row)"""
    rng = _rng("rows", dim, seed)
    x = rng.randn(4 if zero else 3, dim)
    x[1] += 100.0
    x[2, dim // 3] = 1e4
    if zero:
        x[3] = 0.0
    return x.astype(np.float32)


def rmsnorm_case(dim, seed=0):
    rng = _rng("rms", dim, seed)
    return Case(RMSNORM, "rows", x=norm_rows(dim, seed, zero=True), rows=4, dim=dim, p0=(1.0 + 0.2 * rng.randn(dim)).astype(np.float32))


def rmsnorm_reference(c, mut=None):
    x, g = c.x.astype(np.float64), c.p0.astype(np.float64)
    dim = c.dim
    if mut == "mean_subtracted":
        x = x - x.mean(1, keepdims=True)
    nrm = np.sqrt((x * x).sum(1)) * (1.0 if mut == "no_dim_scale" else dim ** -0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = x / (nrm if mut == "no_clamp" else np.maximum(nrm, 1e-8))[:, None] * g
    K = -(-dim // 256)
    e = 0.5 * gamma(K + 9) + SQRTF + RSQRTF + U + DIV + 2 * U
    return y, f16_out(y, np.abs(y) * e * SECOND)


def rmsnorm_emulate(c):
    f = np.float32
    out = np.zeros(c.x.shape, np.float16)
    for r, xr in enumerate(c.x):
        ss = block_sum32(_lanes32(lambda i: xr[i] * xr[i], c.dim))
        inv = f(1.0) / np.maximum(np.sqrt(ss) * f(1.0 / np.sqrt(f(c.dim))), f(1e-8))
        out[r] = (xr * inv * c.p0).astype(np.float16)
    return out.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm family: rownorm, pool, groupnorm
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _norm_block(blk, w, b, m, eps=1e-5, ddof=0):
    """two-pass normalisation of a [T][G] block with shared statistics; w, b [G]; m roundings in each sum -> (value, f32 bound)"""
    N = blk.size
    mean = blk.mean()
    dmean = gamma(m) * np.abs(blk).sum() / N + DIV * abs(mean)
    d = blk - mean
    dd = dmean + U * np.abs(d)
    sq = (d * d).sum()
    dsq = (2 * np.abs(d) * dd).sum() + gamma(m + 1) * sq
    v = sq / (N - ddof) + eps
    dv = dsq / N + (DIV + 2 * U) * v
    rstd = v ** -0.5
    e_r = dv / (2 * v) + RSQRTF
    t = d * rstd * w
    out = t + b
    return out, (np.abs(w) * rstd * dd + np.abs(t) * (e_r + 2 * U) + U * np.abs(out)) * SECOND


def rownorm_case(dim, seed=0):
    rng = _rng("rownorm", dim, seed)
    return Case(ROWNORM, "rows", x=norm_rows(dim, seed), rows=3, dim=dim, p0=(1.0 + 0.2 * rng.randn(dim)).astype(np.float32),
                p1=(0.1 * rng.randn(dim)).astype(np.float32))


def rownorm_reference(c):
    w, b = c.p0.astype(np.float64), c.p1.astype(np.float64)
    K = -(-c.dim // 256)
    res = [_norm_block(xr[None, :], w, b, K + 8) for xr in c.x.astype(np.float64)]
    y, bd = np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
    return y, f16_out(y, bd)


def _ln_row32(xr, w, b, dim):
    f = np.float32
    mean = block_sum32(_lanes32(lambda i: xr[i], dim)) / f(dim)
    sq = block_sum32(_lanes32(lambda i: (xr[i] - mean) * (xr[i] - mean), dim))
    rstd = f(1.0 / np.sqrt(np.float64(f(sq / f(dim) + f(1e-5)))))
    return (xr - mean) * rstd * w + b


def rownorm_emulate(c):
    return np.stack([_ln_row32(xr, c.p0, c.p1, c.dim) for xr in c.x]).astype(np.float16).astype(np.float64)


POOL_NS = [1, 2, 3, 301]


def pool_case(dim, lens, seed=0, kinds=True):
    rng = _rng("pool", dim, tuple(lens), seed)
    start, ln, rows = layout(lens, first=1, tail=1)
    x = rng.randn(rows, dim)
    if kinds:  # the three kinds of row, spread over the sequences
        x[start[0]] += 100.0
        x[start[-1] + ln[-1] - 1, dim // 3] = 1e4
    return Case(POOL, "rows", x=x.astype(np.float32), rows=rows, nseq=len(lens), start=start, len=ln, dim=dim,
                p0=(1.0 + 0.2 * rng.randn(dim)).astype(np.float32), p1=(0.1 * rng.randn(dim)).astype(np.float32))


def pool_reference(c, mut=None):
    w, b = c.p0.astype(np.float64), c.p1.astype(np.float64)
    x = c.x.astype(np.float64)
    K = -(-c.dim // 256)
    y, bd = np.zeros((c.nseq, c.dim)), np.zeros((c.nseq, c.dim))
    for s, (r0, n) in enumerate(zip(c.start, c.len)):
        if mut == "mean_first":
            y[s] = _norm_block(x[r0:r0 + n].mean(0)[None, :], w, b, K + 8)[0]
            continue
        res = [_norm_block(x[r][None, :], w, b, K + 8) for r in range(r0, r0 + n)]
        val, vb = np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
        div = max(c.len) if mut == "divisor_maxlen" else n
        y[s] = val.sum(0) / div
        bd[s] = ((vb.sum(0) + gamma(n) * np.abs(val).sum(0)) / n + DIV * np.abs(y[s])) * SECOND
    return y, bd


def pool_emulate(c):
    out = np.zeros((c.nseq, c.dim), np.float32)
    for s, (r0, n) in enumerate(zip(c.start, c.len)):
        acc = np.zeros(c.dim, np.float32)
        for r in range(r0, r0 + n):
            acc = acc + _ln_row32(c.x[r], c.p0, c.p1, c.dim)
        out[s] = acc / np.float32(n)
    return out.astype(np.float64)


GN_SW = {512: 16, 1024: 8, 2048: 4}


def gn_lengths(D):
    sw = GN_SW[D]
    return [1, sw - 1, sw, sw + 1, 130, 517]


def gn_case(D, lens, family="gauss", seed=0, first=0):
    rng = _rng("gn", D, tuple(lens), family, seed)
    start, ln, rows = layout(lens, first=first, tail=1)
    x = rng.randn(rows, D)
    if family == "offset":
        x += 100.0
    if family == "neighbour":  # every clip but the first holds 1e4: statistics that leak across clips show
        x[start[0] + ln[0]:] = 1e4
        x[:start[0]] = 1e4
    return Case(GROUPNORM, family, x=x.astype(np.float32), rows=rows, nseq=len(lens), start=start, len=ln, dim=D,
                p0=(1.0 + 0.2 * rng.randn(D)).astype(np.float32), p1=(0.1 * rng.randn(D)).astype(np.float32))


def gn_reference(c, mut=None):
    """-> (value [rows][D], bound, written mask)"""
    D, G, SW = c.dim, c.dim // 32, GN_SW[c.dim]
    if mut == "other_width":
        G = G * 2 if D < 2048 else G // 2
    x, w, b = c.x.astype(np.float64), c.p0.astype(np.float64), c.p1.astype(np.float64)
    y, bd, wr = np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape, bool)
    for r0, T in zip(c.start, c.len):
        m = -(-T // SW) + 8
        wr[r0:r0 + T] = True
        for g0 in range(0, D, G):
            blk, ww, bb = x[r0:r0 + T, g0:g0 + G], w[g0:g0 + G], b[g0:g0 + G]
            if mut == "per_row":
                for t in range(T):
                    y[r0 + t, g0:g0 + G] = _norm_block(blk[t:t + 1], ww, bb, m)[0]
            elif mut == "neighbour_row":  # the row behind the clip joins the statistics
                y[r0:r0 + T, g0:g0 + G] = _norm_block(x[r0:r0 + T + 1, g0:g0 + G], ww, bb, m)[0][:T]
            else:
                kw = dict(ddof=1) if mut == "unbiased" else dict(eps=1e-6) if mut == "eps_1e-6" else {}
                y[r0:r0 + T, g0:g0 + G], bd[r0:r0 + T, g0:g0 + G] = _norm_block(blk, ww, bb, m, **kw)
    return y, f16_out(y, bd), wr


def gn_emulate(c):
    f = np.float32
    D, G, SW = c.dim, c.dim // 32, GN_SW[c.dim]
    out = np.zeros(c.x.shape, np.float16)
    for r0, T in zip(c.start, c.len):
        for g0 in range(0, D, G):
            blk = c.x[r0:r0 + T, g0:g0 + G]  # thread t0 * G + j takes rows t0, t0 + SW, ...
            flat = blk.reshape(-1)  # element index = t * G + j: a sweep of SW rows is 256 consecutive elements, in thread order
            n = f(f(G) * f(T))
            mean = block_sum32(_lanes32(lambda i: flat[i], flat.size)) / n
            sq = block_sum32(_lanes32(lambda i: (flat[i] - mean) * (flat[i] - mean), flat.size))
            rstd = f(1.0 / np.sqrt(np.float64(f(sq / n + f(1e-5)))))
            out[r0:r0 + T, g0:g0 + G] = ((blk - mean) * rstd * c.p0[g0:g0 + G] + c.p1[g0:g0 + G]).astype(np.float16)
    return out.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# rowmean
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def rowmean_case(dim, lens, seed=0):
    rng = _rng("rowmean", dim, tuple(lens), seed)
    start, ln, rows = layout(lens, first=2, tail=1)
    x = rng.randn(rows, dim) + 3.0 * rng.randn(1, dim)
    return Case(ROWMEAN, "rows", x=x.astype(np.float32), rows=rows, nseq=len(lens), start=start, len=ln, dim=dim)


def rowmean_reference(c):
    x = c.x.astype(np.float64)
    y, bd = np.zeros((c.nseq, c.dim)), np.zeros((c.nseq, c.dim))
    for s, (r0, n) in enumerate(zip(c.start, c.len)):
        y[s] = x[r0:r0 + n].mean(0)
        bd[s] = (gamma(n) * np.abs(x[r0:r0 + n]).sum(0) / n + DIV * np.abs(y[s])) * SECOND
    return y, bd


def rowmean_emulate(c):
    out = np.zeros((c.nseq, c.dim), np.float32)
    for s, (r0, n) in enumerate(zip(c.start, c.len)):
        acc = np.zeros(c.dim, np.float32)
        for r in range(r0, r0 + n):
            acc = acc + c.x[r]
        out[s] = acc / np.float32(n)
    return out.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# geglu
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
FFS = [128, 384, 1536]
_erf = np.vectorize(math.erf, otypes=[np.float64])


def geglu_case(ff, seed=0):
    rng = _rng("geglu", ff, seed)
    rows = 4
    gate = np.tile(np.concatenate([np.linspace(-8, 8, 126), [0.0, -0.0]]), (rows, ff // 128)).astype(np.float32)  # a grid over [-8, 8] with +-0
    for r in range(rows):
        gate[r] = np.roll(gate[r], 37 * r)
    val = (rng.randn(rows, ff) * np.where(np.arange(ff) % 2, 1.0, -1.0) * (1 + np.arange(rows))[:, None]).astype(np.float32)  # u of both signs
    return Case(GEGLU, "grid", x=np.concatenate([val, gate], axis=1), rows=rows, dim=ff)


def geglu_reference(c, mut=None):
    x = c.x.astype(np.float64)
    ff = c.dim
    uu, g = (x[:, ff:], x[:, :ff]) if mut == "halves_swapped" else (x[:, :ff], x[:, ff:])
    if mut == "tanh":
        return uu * 0.5 * g * (1 + np.tanh(math.sqrt(2 / math.pi) * (g + 0.044715 * g ** 3))), None
    a = g * math.sqrt(0.5)
    E = _erf(a)
    s = 1.0 + E
    ds = ERFF / ULP * ulp32(E) + 2 * U * np.abs(a) * (2 / math.sqrt(math.pi)) * np.exp(-a * a) + U * np.abs(s)
    inner = 0.5 * g * s
    y = uu * inner
    return y, f16_out(y, (np.abs(uu) * (0.5 * np.abs(g) * ds + U * np.abs(inner)) + U * np.abs(y)) * SECOND)


def geglu_emulate(c):
    f = np.float32
    ff = c.dim
    uu, g = c.x[:, :ff], c.x[:, ff:]
    E = _erf((g * f(0.70710678118654752)).astype(np.float64)).astype(f)  # a correctly rounded erff
    return (uu * (f(0.5) * g * (f(1.0) + E))).astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the copy kernels: embed, mel_rows, im2col3, im2col5 (bit for bit)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
TINS = [1, 2, 3, 4, 5, 7, 8, 130]


def coded(shape, salt=0):
    """f32 values that stay distinguishable after the fp16 rounding: element i is the fp16 number with the bit pattern 0x0400 + (7919 i + salt) mod 29000 (a normal
    number; every element distinct up to 29000 of them, repeats 29000 apart beyond), its sign by the parity of i, moved 0, 0.3 or 0.7 fp16 ulp up so that the
    rounding itself is exercised"""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    h = (0x0400 + (7919 * i + salt) % 29000).astype(np.uint16).view(np.float16).astype(np.float64)
    v = (h + np.array([0.0, 0.3, 0.7])[i % 3] * ulp16(h)) * np.where(i % 2, -1.0, 1.0)
    return v.astype(np.float32).reshape(shape)


def embed_case(dim, seed=0):
    rng = _rng("embed", dim, seed)
    vocab, rows = 37, 21
    tok = rng.randint(0, vocab, rows)
    tok[:3] = [0, vocab - 1, vocab - 1]
    return Case(EMBED, "coded", x=coded((vocab, dim), seed), rows=rows, dim=dim, vocab=vocab, tok=tok.astype(np.int32))


def embed_reference(c):
    return c.x[c.tok].view(np.uint32).reshape(-1), np.ones(c.rows * c.dim, bool)


def _mel_clips(lens, bands, salt):
    clips = [coded((bands, T), salt + 1000 * s) for s, T in enumerate(lens)]
    off = np.cumsum([0] + [m.size for m in clips[:-1]]).astype(np.int64)
    return clips, off, np.concatenate([m.reshape(-1) for m in clips])


def mel_rows_case(lens, seed=0):
    clips, off, flat = _mel_clips(lens, 80, seed)
    start, ln, rows = layout(lens, first=1, tail=2)
    return Case(MEL_ROWS, "coded", x=flat, mel_off=off, rows=rows, nseq=len(lens), start=start, len=ln, dim=80, clips=clips)


def mel_rows_reference(c, mut=None):
    out = np.full((c.rows, 128), SENTINEL * 0x0101, np.uint16)
    wr = np.zeros((c.rows, 128), bool)
    for m, r0, T in zip(c.clips, c.start, c.len):
        src = m.reshape(-1)[:T * 80].reshape(T, 80) if mut == "transposed" else m.T  # mel[c * T + t] against mel[t * 80 + c]
        out[r0:r0 + T, :80] = src.astype(np.float16).view(np.uint16)
        out[r0:r0 + T, 80:] = 0
        wr[r0:r0 + T] = True
    return out.reshape(-1), wr.reshape(-1)


def im2col_case(taps, lens, cin, kpad, cm, seed=0):
    out_lens = [(T - 1) // 2 + 1 for T in lens]
    ostart, olen, orows = layout(out_lens, first=1, tail=1)
    p = dict(nseq=len(lens), out_start=ostart, out_len=olen, out_rows=orows, dim=cin, kpad=kpad, len=np.array(lens, np.int32), taps=taps)
    if cm:
        clips, off, flat = _mel_clips(lens, cin, seed)
        p.update(x=flat, mel_off=off, rows=1, variant=1 if taps == 3 else 0)
    else:
        start, ln, rows = layout(lens, first=2, tail=1)
        x = coded((rows, cin), seed)
        clips = [x[r0:r0 + T].T for r0, T in zip(start, ln)]  # [cin][T] views
        p.update(x=x, start=start, rows=rows, variant=0)
    return Case(IM2COL3 if taps == 3 else IM2COL5, "coded", clips=clips, **p)


def im2col_reference(c, mut=None):
    taps, cin, kpad = c.taps, c.dim, c.kpad
    pad = taps // 2 + (1 if mut == "pad_off_by_one" else 0)
    out = np.full((c.out_rows, kpad), SENTINEL * 0x0101, np.uint16)
    wr = np.zeros((c.out_rows, kpad), bool)
    for m, r0, To, Tin in zip(c.clips, c.out_start, c.out_len, c.len):
        if mut == "tin_for_tout":
            To = min(Tin, c.out_rows - r0)
        for t in range(To):
            row = np.zeros(kpad, np.float32)
            for tap in range(taps):
                ti = 2 * t + tap - pad
                if 0 <= ti < Tin:
                    if mut == "channel_major_k":
                        row[tap:taps * cin:taps] = m[:, ti]  # k = c * taps + tap
                    else:
                        row[tap * cin:(tap + 1) * cin] = m[:, ti]
            out[r0 + t] = row.astype(np.float16).view(np.uint16)
            wr[r0 + t] = True
    return out.reshape(-1), wr.reshape(-1)


def copy_cases():
    cs = [embed_case(d, d) for d in (128, 768, 1024)]
    ragged = (7, 1, 130)
    for T in TINS:
        cs.append(mel_rows_case([T], T))
        cs.append(im2col_case(3, [T], 100, 320, True, T))      # the first conditioning convolution: 320 > 3 * 100
        cs.append(im2col_case(3, [T], 256, 768, False, T))     # CVVP's second stem convolution: kpad = 3 cin
        cs.append(im2col_case(5, [T], 80, 448, True, T))       # CVVP's first stem convolution: k0pad = 448
    cs.append(im2col_case(3, [5, 8], 1024, 3072, False, 3))    # the second conditioning convolution: 3072 = 3 * 1024
    cs += [mel_rows_case(ragged, 77), im2col_case(3, ragged, 100, 320, True, 77), im2col_case(3, ragged, 256, 768, False, 77), im2col_case(5, ragged, 80, 448, True, 77)]
    return cs


def copy_reference(c, mut=None):
    if c.op == EMBED:
        return embed_reference(c)
    if c.op == MEL_ROWS:
        return mel_rows_reference(c, mut)
    return im2col_reference(c, mut)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def attn_dh(variant):
    return 128 if variant == BIAS128 else 64


def attn_kc(variant):
    return 8192 // attn_dh(variant)


def attn_lengths(variant):
    kc = attn_kc(variant)
    return sorted({1, 2, kc - 1, kc, kc + 1, 2 * kc - 1, 2 * kc, 2 * kc + 1, 255, 256, 257, 3 * kc + 1, 517})


RAGGED = (257, 1, 130)
EIGHT = (17, 64, 1, 129, 33, 192, 63, 130)
PRODUCT_HEADS = [(ROT64, 768), (ROT64, 512), (PLAIN64, 512), (PLAIN64, 1024), (BIAS128, 2048)]  # CLVP 12 x 64, CVVP 8 x 64 (layers, AttentionBlock), voice encoder, conditioning
DOM_DIM = 40  # the dominant key's direction: a head dim the rotary embedding leaves alone


def bias_table(name, heads, seed=0):
    """`smooth` and `sharp` as dattn_cases.bias_table: sharp has an independent magnitude in [0.5, 4] per (head, side, distance) with alternating signs, so that
    neighbouring entries, the two sides, entries 62 / 63 and neighbouring heads differ by at least 1"""
    rng = _rng("bias", name, heads, seed)
    if name == "sharp":
        sign = np.where((np.arange(heads)[:, None, None] + np.arange(2)[None, :, None] + np.arange(64)[None, None, :]) % 2 == 0, 1.0, -1.0)
        return (sign * rng.uniform(0.5, 4.0, (heads, 2, 64))).reshape(heads, 128).astype(np.float32)
    c = rng.uniform(0.3, 1.0, (heads, 2, 1))
    return (-c * (np.arange(64) / 63.0)[None, None, :]).reshape(heads, 128).astype(np.float32)


def _family(rng, family, n, DH):
    """q, k, v [n][DH] of one (sequence, head)"""
    scale = DH ** -0.5
    q, k, v = rng.randn(n, DH), rng.randn(n, DH), rng.randn(n, DH)
    if family.startswith("ramp"):  # the score moves by 0.5 a key: up (a new maximum, a rescale, at every key) or down (none after key 0)
        q, k = 0.3 * q, 0.3 * k
        q[:, DOM_DIM] = 4.0
        j = np.arange(n) if family == "ramp_up" else -np.arange(n)
        k[:, DOM_DIM] = 0.5 * j / (4.0 * scale)
    elif family.startswith("dom"):  # one key 12 above the others for every query
        pos = int(family[3:])
        q, k = 0.5 * q, 0.5 * k
        q[:, DOM_DIM] = 4.0
        k[:, DOM_DIM] = 0.0
        k[pos % n, DOM_DIM] = 12.0 / (4.0 * scale)
    return q, k, v


def attn_case(variant, lens, family="flat", table="smooth", heads=3, first=0, tail=1, seed=0, poison=False):
    DH = attn_dh(variant)
    inner = heads * DH
    start, ln, rows = layout(lens, first=first, tail=tail)
    rng = _rng("attn", variant, tuple(lens), family, heads, seed)
    qkv = rng.randn(rows, 3 * inner)  # rows outside the sequences: finite noise (or NaN: poison)
    for s, (r0, n) in enumerate(zip(start, ln)):
        for h in range(heads):
            q, k, v = _family(_rng("seq", variant, int(n), family, h, seed + 31 * s), family, int(n), DH)
            for i, t in enumerate((q, k, v)):
                qkv[r0:r0 + n, i * inner + h * DH:i * inner + (h + 1) * DH] = t
    qkv = qkv.astype(np.float16)
    if poison:
        live = np.zeros(rows, bool)
        for r0, n in zip(start, ln):
            live[r0:r0 + n] = True
        qkv[~live] = np.nan
    p = dict(x=qkv, variant=variant, rows=rows, nseq=len(lens), start=start, len=ln, dim=inner, heads=heads, poison=int(poison), table=table, seed=seed)
    if variant == BIAS128:
        p["p0"] = bias_table(table, heads, seed)
    return Case(ATTN, "%s/%s" % (family, table) if variant == BIAS128 else family, **p)


def attn_alone(c, s):
    """sequence s of c at row 0 of a case of its own"""
    r0, n = int(c.start[s]), int(c.len[s])
    p = dict(c.p)
    p.update(x=np.ascontiguousarray(c.x[r0:r0 + n]), rows=n, nseq=1, start=np.array([0], np.int32), len=np.array([n], np.int32), poison=0)
    return Case(ATTN, c.family, **p)


def attn_poisoned(c):
    p = dict(c.p)
    x = c.x.copy()
    live = np.zeros(c.rows, bool)
    for r0, n in zip(c.start, c.len):
        live[r0:r0 + n] = True
    x[~live] = np.nan
    p.update(x=x, poison=1)
    return Case(ATTN, c.family, **p)


C16 = 13.287712379549449 / 16.0  # log2(10000) / 16, the kernel's constant


def rot_ref(t, pos, pairs=16, half=16, freq_div=16.0, dims=(0,)):
    """rotary embedding in float64 on dims base .. base + 31 of t [n][DH] at positions pos [n]: pairs (d, d + half), angle pos 10000^(-d / 16) -> (value, bound of the
    f32 rotation). The angle's own error: pos freq times (the exponent -d C16, rounded constant and product: 2u d C16 ln 2 through 2^x; exp2f; the product)"""
    out, err = t.copy(), np.zeros(t.shape)
    d = np.arange(16)
    ang = pos[:, None] * 10000.0 ** (-d / freq_div)[None, :]
    dang = np.abs(ang) * (2 * U * d * C16 * math.log(2.0) + EXP2F + U)[None, :]
    c, s = np.cos(ang), np.sin(ang)
    for base in dims:
        ia = base + (d if half == 16 else 2 * d)
        ib = ia + half
        a, b = t[:, ia], t[:, ib]
        out[:, ia], out[:, ib] = a * c - b * s, b * c + a * s
        e = (np.abs(a) + np.abs(b)) * (dang + max(COSF, SINF) + 3 * U)  # |a| dcos + |b| dsin, dcos <= |sin| dang + 4 ulp; two products and the sum
        err[:, ia], err[:, ib] = e, e
    return out, err


def _staged16(r, dr):
    """what the kernel stores in LDS for a rotated value r whose f32 rotation is within dr: the float64 value rounded to fp16, and the charge where the f32
    rotation can round the other way: a whole fp16 step for every rounding boundary within dr of r"""
    h = rn16(r)
    below = ulp16(np.abs(h) * (1 - 2.0 ** -12))  # the spacing just below |h| (half the one above at a power of two)
    dist = 0.5 * below - np.abs(r - h)
    sp = ulp16(np.abs(r) + dr)
    return h, np.where((dr > 0) & (dist <= dr), sp * (1.0 + np.floor(dr / sp)), 0.0)


ATTN_MUTS = ["drop_last", "admit_n", "stale_chunk", "pairs_adjacent", "freq_32", "v_unrotated", "v_at_query", "global_rows", "z_restart", "rot_upper", "other_scale",
             "sides_swapped", "saturate_62", "saturate_64", "distance_plus_1", "next_head_table", "head_stride_64"]


def attn_reference(c, s, h, mut=None, stage=True):
    """float64 reference and bound of one (sequence, head): -> (o [n][DH], bound [n][DH]); with mut: the defective reference alone; stage=False leaves the
    rotated k and v unrounded (the form an independent float64 restatement can be compared with to 1e-12).

    q is rotated in float64 at its position within the sequence; k and v are rotated at the key's position and rounded to fp16 as the kernel stores them in LDS;
    s_j = q . k_j / sqrt(DH) + tab[h][(q < k) 64 + min(|k - q|, 63)]; softmax and the weighted sum in float64.
    Bound: ds_j = scale (gamma_DH sum |q k| + sum |k| dq + sum |q| dk) + 3u |s_j|   (the f32 dot; the rotation of q; the staged k; scale, its constant, the bias add)
           eps_j = ds_j + EXPF (n - j) + u (m - s_j)       one expf for the weight and one rescale per later key (the kernel rescales at EVERY key); the rounded arguments
           numerator and denominator are sums of the SAME weights w_j (1 + eps_j): do = sum_j w~_j eps_j |v_j - o|, w~ the normalised weights
           + sum_j w~_j dv_j                               the staged v
           + u sum_j w~_j ((3 (n - j) + 1) |v_j| + 2 (n - j) |o|)       the running sums: p v, and a product and an add per later key, in acc and in l
           + (DIV + u) |o|                                 1 / l and the product; then the fp16 rounding (f16_out)"""
    variant, inner, DH = c.variant, c.dim, attn_dh(c.variant)
    r0, n = int(c.start[s]), int(c.len[s])
    x = c.x.astype(np.float64)
    hs = 64 if mut == "head_stride_64" else DH
    nk = n + 1 if mut == "admit_n" else n - 1 if mut == "drop_last" else n
    q = x[r0:r0 + n, h * hs:h * hs + DH]
    k = x[r0:r0 + nk, inner + h * hs:inner + h * hs + DH]
    v = x[r0:r0 + nk, 2 * inner + h * hs:2 * inner + h * hs + DH]
    qi, kj = np.arange(n), np.arange(nk)
    kdist = kj  # the key index the bias distance is taken from
    if mut == "stale_chunk":  # the last chunk read to its full KC: LDS rows kn .. KC - 1 still hold the previous chunk's keys
        KC = attn_kc(variant)
        k0 = (n - 1) // KC * KC
        if k0 > 0:
            slots = np.arange(n - k0, KC)
            k, v = np.concatenate([k, k[k0 - KC + slots]]), np.concatenate([v, v[k0 - KC + slots]])
            kj, kdist = np.concatenate([kj, k0 - KC + slots]), np.concatenate([kj, k0 + slots])  # rotated at their own position, seen at the slot's
    qpos = qi % 256 if mut == "z_restart" else qi
    dq = np.zeros(q.shape)
    dk, dv = np.zeros(k.shape), np.zeros(v.shape)
    if variant == ROT64:
        off = r0 if mut == "global_rows" else 0
        kw = dict(half=1) if mut == "pairs_adjacent" else dict(freq_div=32.0) if mut == "freq_32" else dict(dims=(0, 32)) if mut == "rot_upper" else {}
        q, dq = rot_ref(q, (qpos + off).astype(np.float64), **kw)
        kr, dkr = rot_ref(k, (kj + off).astype(np.float64), **kw)
        k, dk = _staged16(kr, dkr) if stage else (kr, dkr)
        if mut != "v_unrotated" and mut != "v_at_query":
            vr, dvr = rot_ref(v, (kj + off).astype(np.float64), **kw)
            v, dv = _staged16(vr, dvr) if stage else (vr, dvr)
    scale = (128 if DH == 64 else 64) ** -0.5 if mut == "other_scale" else DH ** -0.5
    S = q @ k.T * scale
    if variant == BIAS128:
        tab = np.concatenate([c.p0.astype(np.float64).reshape(-1), np.zeros(256)])
        dist = kdist[None, :] - qpos[:, None] + (1 if mut == "distance_plus_1" else 0)
        side = (dist < 0) if mut == "sides_swapped" else (dist > 0)
        sat = 62 if mut == "saturate_62" else 64 if mut == "saturate_64" else 63
        hh = h + 1 if mut == "next_head_table" else h
        S = S + tab[hh * 128 + side * 64 + np.minimum(np.abs(dist), sat)]
    m = S.max(1, keepdims=True)
    W = np.exp(S - m)
    Wn = W / W.sum(1, keepdims=True)
    o = Wn @ v
    if mut == "v_at_query":  # the rotation is linear: rotating every v at the query's position rotates the weighted sum
        o = rot_ref(o, qpos.astype(np.float64))[0]
    if mut is not None:
        return o, None
    dS = scale * (gamma(DH) * (np.abs(q) @ np.abs(k).T) + dq @ np.abs(k).T + np.abs(q) @ dk.T) + 3 * U * np.abs(S)
    later = (n - kj).astype(np.float64)[None, :]
    WE = Wn * (dS + EXPF * later + U * (m - S))
    t1 = np.zeros(o.shape)
    for d in range(DH):
        t1[:, d] = (WE * np.abs(v[None, :, d] - o[:, d:d + 1])).sum(1)
    b = t1 + Wn @ dv + U * ((Wn * (3 * later + 1)) @ np.abs(v)) + U * 2 * (Wn * later).sum(1, keepdims=True) * np.abs(o) + (DIV + U) * np.abs(o)
    return o, f16_out(o, b * SECOND)


def attn_reference_all(c):
    """-> (value [rows][inner], bound, written mask) over the whole output"""
    DH = attn_dh(c.variant)
    y, bd, wr = np.zeros((c.rows, c.dim)), np.zeros((c.rows, c.dim)), np.zeros((c.rows, c.dim), bool)
    for s, (r0, n) in enumerate(zip(c.start, c.len)):
        wr[r0:r0 + n] = True
        for h in range(c.dim // DH):
            y[r0:r0 + n, h * DH:(h + 1) * DH], bd[r0:r0 + n, h * DH:(h + 1) * DH] = attn_reference(c, s, h)
    return y, bd, wr


def _rot32(t, pos):
    f = np.float32
    d = np.arange(16, dtype=f)
    ang = pos.astype(f)[:, None] * np.exp2(-d * f(f(13.287712379549449) / f(16.0)))[None, :].astype(f)
    c, sn = np.cos(ang), np.sin(ang)
    a, b = t[:, :16].copy(), t[:, 16:32].copy()
    t[:, :16], t[:, 16:32] = a * c - b * sn, b * c + a * sn


def attn_emulate(c):
    """the kernel's operation order in float32: f32 rotation, fp16 staging of k and v in chunks of KC keys, a sequential f32 dot, per-key online softmax with a
    running maximum and a rescale of l and acc at every key, 1 / l, the fp16 rounding"""
    f = np.float32
    variant, inner, DH, KC = c.variant, c.dim, attn_dh(c.variant), attn_kc(c.variant)
    scale = f(0.125) if DH == 64 else f(0.08838834764831845)
    out = np.zeros((c.rows, inner), np.float64)
    x = c.x.astype(f)
    for r0, n in zip(c.start, c.len):
        pos = np.arange(n)
        for h in range(inner // DH):
            q = x[r0:r0 + n, h * DH:(h + 1) * DH].copy()
            k = x[r0:r0 + n, inner + h * DH:inner + (h + 1) * DH].copy()
            v = x[r0:r0 + n, 2 * inner + h * DH:2 * inner + (h + 1) * DH].copy()
            if variant == ROT64:
                _rot32(q, pos); _rot32(k, pos); _rot32(v, pos)
            k, v = k.astype(np.float16).astype(f), v.astype(np.float16).astype(f)
            m, l, acc = np.full(n, -np.inf, f), np.zeros(n, f), np.zeros((n, DH), f)
            for k0 in range(0, n, KC):
                kk = k[k0:k0 + KC]
                sc = np.add.accumulate(q[:, None, :] * kk[None, :, :], axis=2, dtype=f)[:, :, -1] * scale  # the f32 dot, dims ascending
                if variant == BIAS128:
                    dist = (k0 + np.arange(len(kk)))[None, :] - pos[:, None]
                    sc = sc + c.p0[h][(dist > 0) * 64 + np.minimum(np.abs(dist), 63)]
                for j in range(len(kk)):
                    mn = np.maximum(m, sc[:, j])
                    with np.errstate(invalid="ignore"):
                        a, p = np.exp(m - mn), np.exp(sc[:, j] - mn)
                    l = l * a + p
                    acc = acc * a[:, None] + p[:, None] * v[k0 + j][None, :]
                    m = mn
            out[r0:r0 + n, h * DH:(h + 1) * DH] = (acc * (f(1.0) / l)[:, None]).astype(np.float16)
    return out


def attn_cases(variant):
    """the matrix of one instantiation: every length flat (both tables under BIAS); ramps and dominant keys at the chunk and z-block edges; the layouts"""
    kc = attn_kc(variant)
    tables = ["smooth", "sharp"] if variant == BIAS128 else ["smooth"]
    cs = []
    for i, n in enumerate(attn_lengths(variant)):
        for t in tables:
            cs.append(attn_case(variant, [n], "flat", t, seed=i))
    for n in (kc + 1, 2 * kc + 1, 517):
        cs += [attn_case(variant, [n], "ramp_up", tables[-1]), attn_case(variant, [n], "ramp_down", tables[-1])]
    for pos in (0, 516, 512, kc - 1, 100):  # key 0, key n - 1, the first key of the last chunk, the last key of the first chunk, and one that every distance
        cs.append(attn_case(variant, [517], "dom%d" % pos, tables[-1]))  # -64 .. +64 is measured from (queries 36 .. 164)
    cs.append(attn_case(variant, [3 * kc + 1], "dom%d" % (3 * kc), tables[-1]))  # a last chunk of one key
    cs.append(attn_case(variant, [130], "flat", tables[-1], first=3, tail=2))  # positions are not global rows
    cs.append(attn_case(variant, RAGGED, "flat", tables[-1], first=1))  # z = 2, two sequences return early in z = 1
    cs.append(attn_case(variant, EIGHT, "flat", tables[-1], first=2))
    return cs


def attn_product_cases():
    return [attn_case(v, [130], "flat", "sharp", heads=inner // attn_dh(v), first=1) for v, inner in PRODUCT_HEADS]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# one entry for every op
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def reference(c):
    """-> (value, bound, written mask), flat over the payload; the copy kernels: (bits, None, written mask)"""
    if c.op in COPY_OPS:
        bits, wr = copy_reference(c)
        return bits, None, wr
    if c.op == ATTN:
        y, b, wr = attn_reference_all(c)
    elif c.op == GROUPNORM:
        y, b, wr = gn_reference(c)
    else:
        y, b = {RMSNORM: rmsnorm_reference, ROWNORM: rownorm_reference, POOL: pool_reference, ROWMEAN: rowmean_reference, GEGLU: geglu_reference}[c.op](c)
        wr = np.ones(y.shape, bool)
    return y.reshape(-1), b.reshape(-1), wr.reshape(-1)


def emulate(c):
    fn = {RMSNORM: rmsnorm_emulate, ROWNORM: rownorm_emulate, POOL: pool_emulate, ROWMEAN: rowmean_emulate, GEGLU: geglu_emulate, GROUPNORM: gn_emulate, ATTN: attn_emulate}
    return fn[c.op](c).reshape(-1)


def norm_cases():
    """rmsnorm, rownorm, pool, rowmean, geglu, groupnorm"""
    cs = []
    for d in DIMS:
        cs += [rmsnorm_case(d), rownorm_case(d)]
    for d in DIMS:
        cs.append(pool_case(d, [3, 1, 2]))
    cs.append(pool_case(768, [301, 2]))
    cs += [rowmean_case(512, [1, 2, 301]), rowmean_case(640, [301, 1, 2])]
    cs += [geglu_case(ff) for ff in FFS]
    for D in (512, 1024, 2048):
        for T in gn_lengths(D):
            cs.append(gn_case(D, [T], "gauss", seed=T))
        cs.append(gn_case(D, [GN_SW[D] + 1, 33], "offset", first=1))
        cs.append(gn_case(D, [GN_SW[D] + 1, 1, 9], "gauss", first=1))
        cs.append(gn_case(D, [9, 5], "neighbour", first=2))
    return cs


def alone(c, s):
    """sequence s of a groupnorm / attention case as a case of its own"""
    if c.op == ATTN:
        return attn_alone(c, s)
    r0, n = int(c.start[s]), int(c.len[s])
    p = dict(c.p)
    p.update(x=np.ascontiguousarray(c.x[r0:r0 + n]), rows=n, nseq=1, start=np.array([0], np.int32), len=np.array([n], np.int32))
    return Case(c.op, c.family, **p)
