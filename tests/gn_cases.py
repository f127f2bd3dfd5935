"""Shared by tests/test_gn_kernels_gpu.py and tests/test_gn_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/diff_gn_harness.hip -> libtts_gn_test.so), the float64 NumPy reference of the diffusion stage's GroupNorm(32), the case matrix, the
acceptance rule and its error bound.

    mean, var (biased) per (sequence, group of 32 channels) over the T x 32 elements;  v = (x - mean) / sqrt(var + eps)
    u = (v g + b) (scale + 1) + shift   [scale | shift = one row of 2048 of `ss`, optional]     z = silu(u) in the case's mode, optional

The reference shares no code with the harness or the kernels; test_gn_harness_cpu.py checks it against torch.nn.functional.group_norm in float64 and naive loops.

INPUTS. x is f32 [rows][1024] in the packed layout of the diffusion stage (sequence starts on multiples of 8, at least one guard row behind every sequence). The 32
groups of a sequence are reduced by 32 independent workgroups, so ONE launch carries the input families side by side, one per group (group_plan()):
  flat     N(0, 1) with the group's own offset (within +-4) and scale (0.25 .. 4): a neighbour group's statistics are wrong by many standard deviations.
  offset   mean = 100 std: the conditioning the pivot comment of gn_stats_kernel speaks of.
  tiny     std = 2e-3, var = 4e-6 between the two gn_eps values the engine exposes (1e-6, 1e-5; configurations below use both): eps and its place matter.
  spike    flat plus ONE element of 64 std sqrt(32 T) / 8 (it alone carries 64 / 65 of the variance) on, in turn: row 0, row T - 1, row T (the guard row, visible
           to nothing), rows SWEEP - 1 and SWEEP of the class, the first row of the last register slot (NJ - 1) SWEEP (pivot kernels: rows 255 / 256, the edge of
           the `unroll 8` sweep), each once on channel 0 and once on channel 31 of its group (channel 0 of the NEXT group is then the spike of a neighbour).
  outlier-pivot  the spike on element [0][0] of the group: for the pivot kernels the worst case of the (pivot - mean)^2 / var term below, for gn_reg another spike.
  poison   (a case flag) every guard row of x is NaN: guard rows of the output must still be +0 and sequence rows unchanged.
g, b = 1 +- 0.05 and +- 0.1, ss scale / shift +- 0.5. `hot` configurations multiply g by 6 so that |u| reaches about 20 under SiLU, where exp2 is furthest from 1.

ACCEPTANCE. No tolerance is fitted. For every element a bound on the error of the f32 value the kernel rounds gives an interval [lo, hi] of f32 values a correct
kernel can hold; fp16 outputs are accepted exactly when rn16(lo) <= out <= rn16(hi) (rounding is monotone), f32 outputs and statistics when lo <= out <= hi.
SiLU is not monotone (minimum at X_MIN = -1.27846...), so the IMAGE of the pre-activation interval is taken (silu_image()), not its end points.
lut = 1 is rn16(silu(rn16(u))): the pre-activation interval is rounded to fp16 first, the image taken over the rounded interval, then the output rounding.

ERROR BOUND, term by term; u = 2^-24, E2 = 1e-6 (no ISA accuracy statement for v_exp_f32 / v_rcp_f32 is available to this suite: each is charged the 1e-6 relative
ar_attn_cases.py already uses; the library expf of the two exact modes is charged the same and an IEEE division or square root 2u). Per (sequence, group), with
mean|.| the average over the T x 32 elements and d = x - mean:
  the sum      k_sum = roundings on the longest chain of one term.
               gn_reg<NT, NJ>: (a+b)+(c+d) 2, NJ serial adds, 6 shuffle steps, NW = NT / 64 partials:       k_sum = 2 + NJ + 6 + NW
                               dmean = k_sum u mean|x| + u |mean|                                              (the division by n)
               pivot kernels (gn_fused_kernel<0>, gn_stats_kernel), p = the group's first element: a thread adds its rows t, t + 32, .. serially, so
                               row t meets w_t = (rows of its thread's chain) - t // 32 <= ceil(T / 32) serial adds (counted per row: with the pivot on an
                               outlier every |x - p| is large and the flat count ceil(T / 32) for all rows would double the bound), and
                               x - p 1, (a+b)+(c+d) 2, 6 shuffles, 4 partials as (a+b)+(c+d) 2:                k_t = w_t + 11
                               dmd = u mean(k_t |x - p|) + u |p - mean|,  dmean = dmd + u |mean|               (mean = p + md)
  the squares  gn_reg, two-pass on the registers: x - mean' 1 (twice under the square), the square 1, the same tree, / n 1:  k_sq = 2 + 1 + 2 + NJ + 6 + NW + 1
                               rho_var = k_sq u + 2 dmean mean|d| / var + dmean^2 / var                          (the propagated error of the mean)
               pivot kernels, E[(x-p)^2] - md^2 with E[(x-p)^2] = var + (p - mean)^2: x - p twice, the square, the tree, / n:   k_t = w_t + 14
                               rho_var = (u mean(k_t (x - p)^2) + 2 |p - mean| dmd + u (p - mean)^2) / var + u
               This is the cancellation the one-pass form pays: with the pivot on an outlier (p - mean)^2 / var is about 32 T and rho_var reaches about 0.6 at
               T = 2305 where the two-pass form stays at 1e-6. A property of gn_fused_kernel<0> and gn_stats_kernel that is recorded here, not a defect.
               gn_apply_kernel: statistics given, f64 from exact integer sums: dmean = u |mean| (the cast), rho_var = 2^-50 (1 + mean^2 / var).
  rstd         rho_pe = rho_var var / (var + eps) + u   (eps damps the variance error), rho_r = (1 - rho_pe)^(-1/2) - 1 + 4u   (exact in rho_pe; sqrt and division)
  the chain    one rounding per product or sum (an FMA contraction only removes roundings):
               Dd = dmean + u |d|;  Dv = Dd rstd + |v| (rho_r + u);  D1 = Dv |g| + u |v g|;  D2 = D1 + u |v g + b|
               with ss:  D3 = D2 |scale + 1| + 2u |u3| (the +1 and the product);  D4 = D3 + u |u4|
  SiLU         relative (1 - s)(E2 + 2u |x|) + E2 + 2u of silu(x), s = sigmoid(x): the argument x * -log2(e) (constant and product), exp2, 1 + e, rcp, the product;
               evaluated at both ends of the interval and at X_MIN where it is inside.
Nothing in the bound is fitted to what a GPU printed.

SHARPNESS. MUTATIONS are defects applied to the REFERENCE (reference(mut=...)). test_gn_harness_cpu.py checks that every one of them leaves the acceptance interval
of some element by >= 10 x (half-width + one fp16 ulp of the value) on a case of the matrix, and that the spike placements catch each structural mutation (dropped
last row, admitted row T, dropped row SWEEP, dropped last register slot) at EVERY length of the matrix at which the row exists. Two recorded limits:
  * for the pivot kernels the outlier-pivot group's bound is too loose to catch a dropped row (rho_var up to about 0.6); those mutations are caught by the other spike
    placements of the same case, whose pivot is an ordinary element.
  * `silu_wrong_mode` (fp16-table emulation where the hardware form was asked, or the reverse) differs from the right mode by the rounding of the argument to fp16
    only: at most about |u| / 2 fp16 ulps of the output while the output is a normal fp16 number (|u| < 12.5), so 10 x is out of reach by arithmetic. It is
    required to leave the acceptance interval (ratio > 1); `silu_missing` carries the 10 x requirement of that line of the issue."""
import ctypes as C
import math
import os
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_GN_TEST_LIB") or os.path.join(PKG, "libtts_gn_test.so")
SRC = os.path.join(PKG, "testlib", "diff_gn_harness.hip")

REG512, REG1024, FUSED, AUTO, STATS, STATS_APPLY_F32, APPLY, TO_F16, GATHER_F16, GATHER_F32 = range(10)
KIND_NAMES = ["gn_reg_kernel<512,14>", "gn_reg_kernel<1024,18>", "gn_fused_kernel<0>", "gn_fused() dispatch", "gn_stats_kernel",
              "gn_stats_kernel + gn_apply_f32_kernel", "gn_apply_kernel", "to_f16_kernel", "gather_f16_kernel", "gather_f32_kernel"]
CH = 1024
SENTINEL = 0xCB
HIP_INVALID_VALUE = 1
U = 2.0 ** -24
E2 = 1e-6
FX_STRIPES = 8

# where a kernel class cuts the row axis. form: how it reduces
CLASS = {
    REG512: dict(form="two", NT=512, NJ=14, SWEEP=64, edges=(63, 64, 13 * 64)),
    REG1024: dict(form="two", NT=1024, NJ=18, SWEEP=128, edges=(127, 128, 17 * 128)),
    FUSED: dict(form="pivot", SWEEP=32, edges=(31, 32, 255, 256)),
    STATS: dict(form="pivot", SWEEP=32, edges=(31, 32, 255, 256)),
    STATS_APPLY_F32: dict(form="pivot", SWEEP=32, edges=(31, 32, 255, 256)),
    APPLY: dict(form="given", SWEEP=4, edges=(3, 4, 7, 8)),
}
LENGTHS = {
    REG512: [1, 2, 63, 64, 65, 127, 128, 129, 895, 896],
    REG1024: [1, 127, 128, 129, 255, 257, 897, 2303, 2304],
    FUSED: [1, 31, 32, 33, 255, 256, 257, 2305],
    STATS: [1, 31, 32, 33, 127, 128, 129, 500],
    APPLY: [1, 3, 4, 5, 7, 8, 9, 435],
}
AUTO_LENGTHS = [(896, 0), (897, 1), (2304, 1), (2305, 2)]
TRIPLES = {REG512: (65, 1, 128), REG1024: (129, 1, 257), FUSED: (33, 1, 257), STATS: (33, 1, 129), APPLY: (9, 1, 5)}


class CaseStruct(C.Structure):
    _fields_ = [("kind", C.c_int), ("ns", C.c_int), ("rows_total", C.c_int), ("row0", C.c_int), ("x_rows", C.c_int),
                ("do_silu", C.c_int), ("lut", C.c_int), ("n_steps", C.c_int), ("ss_step_stride", C.c_int),
                ("pf0_lines", C.c_int), ("pf1_lines", C.c_int), ("eps", C.c_float),
                ("pf0_bytes", C.c_longlong), ("pf1_bytes", C.c_longlong),
                ("start", C.c_void_p), ("len", C.c_void_p), ("seq_step", C.c_void_p), ("seq_voice", C.c_void_p), ("src_row", C.c_void_p),
                ("x", C.c_void_p), ("g", C.c_void_p), ("b", C.c_void_p), ("ss", C.c_void_p),
                ("st", C.c_void_p), ("pf0", C.c_void_p), ("pf1", C.c_void_p), ("out", C.c_void_p), ("picked", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_gn_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_gn_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_gn_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_gn_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_gn_test_class.argtypes = [C.c_int]
        for f in (L.tts_gn_test_run, L.tts_gn_test_validate, L.tts_gn_test_margin, L.tts_gn_test_class):
            f.restype = C.c_int
        _lib = L
    return _lib


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape, dtype):
        self.margin = harness().tts_gn_test_margin()
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * self.dtype.itemsize, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


_DTYPES = dict(start=np.int32, len=np.int32, seq_step=np.int32, seq_voice=np.int32, src_row=np.int32, x=np.float32, g=np.float32, b=np.float32, ss=np.float32,
               st=np.int64, pf0=np.uint8, pf1=np.uint8)


def struct(kind, out=None, **kw):
    """A CaseStruct over the given arrays (kept alive on the struct). Array dtypes are checked here, everything else by the harness."""
    cs = CaseStruct()
    cs.kind = kind
    keep = [out]
    for k, v in kw.items():
        if k in _DTYPES:
            if v is not None:
                assert v.dtype == _DTYPES[k] and v.flags.c_contiguous, k
                keep.append(v)
                setattr(cs, k, v.ctypes.data_as(C.c_void_p))
        else:
            setattr(cs, k, v)
    if out is not None:
        cs.out = out.raw.ctypes.data_as(C.c_void_p) if isinstance(out, Guarded) else out
    cs._keep = keep
    return cs


# ---------------------------------------------------------------------------------------------------------------- layout

class Lay(object):
    """The packed row layout by the rule of the diffusion stage: the first sequence on row 8, every next one on the next multiple of 8 that leaves a guard row."""

    def __init__(self, lens, pad=8, first=8):
        self.len = np.asarray(lens, np.int32)
        self.ns = len(lens)
        st, r = [], first
        for n in lens:
            st.append(r)
            r = (r + int(n) + 1 + 7) & ~7
        self.start = np.asarray(st, np.int32)
        self.rows = (r + pad - 1) // pad * pad

    def seq_rows(self, s):
        return slice(int(self.start[s]), int(self.start[s] + self.len[s]))

    def row_mask(self):
        m = np.zeros(self.rows, bool)
        for s in range(self.ns):
            m[self.seq_rows(s)] = True
        return m


# ---------------------------------------------------------------------------------------------------------------- reference

def _newton_silu_min():
    x = -1.28
    for _ in range(60):  # s(x) (1 + x (1 - s(x))) = 0
        s = 1.0 / (1.0 + math.exp(-x))
        f = 1.0 + x * (1.0 - s)
        x -= f / ((1.0 - s) - x * s * (1.0 - s))
    return x


X_MIN = _newton_silu_min()


def silu(x):
    x = np.asarray(x, np.float64)
    return x * np.exp(-np.logaddexp(0.0, -x))


def rn16(x):
    """round to nearest even fp16, as float64 (overflow -> inf)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def ulp16(x):
    """spacing of fp16 at |x| (subnormal spacing 2^-24 below 2^-14)"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def silu_image(a, b):
    """[min, max] of silu over [a, b] elementwise"""
    fa, fb = silu(a), silu(b)
    lo, hi = np.minimum(fa, fb), np.maximum(fa, fb)
    return np.where((a <= X_MIN) & (X_MIN <= b), silu(X_MIN), lo), hi


def silu_apply(u, lut):
    return silu(u) if lut != 1 else rn16(silu(rn16(u)))


MUTATIONS = ["drop_last", "admit_T", "drop_sweep_row", "drop_last_slot", "n_plus", "n_minus", "unbiased", "eps_outside", "eps_wrong", "group_plus", "group_minus",
             "scale_no_plus1", "ss_swapped", "seq_step_other", "voice_other", "silu_missing", "silu_wrong_mode"]
STRUCTURAL = ["drop_last", "admit_T", "drop_sweep_row", "drop_last_slot"]


def mutation_rows(mut, kind, T):
    """The rows a structural mutation removes from (or the one row T it adds to) the sums of a sequence of T rows; None where that row does not exist."""
    cl = CLASS[kind]
    if mut == "drop_last":
        return [T - 1]
    if mut == "admit_T":
        return [T]
    if mut == "drop_sweep_row":
        return [cl["SWEEP"]] if T > cl["SWEEP"] else None
    if mut == "drop_last_slot":
        if cl["form"] != "two":
            return None
        first = (cl["NJ"] - 1) * cl["SWEEP"]
        return list(range(first, T)) if T > first else None
    raise ValueError(mut)


def group_stats(xs, n=None):
    """xs [R][1024] float64 -> mean [32], biased variance [32] over the R x 32 elements of each group (n: the divisor, R * 32 unless a mutation says otherwise)"""
    R = xs.shape[0]
    n = float(n or R * 32)
    x3 = xs.reshape(R, 32, 32)
    mean = x3.sum(axis=(0, 2)) / n
    var = ((x3 - mean[None, :, None]) ** 2).sum(axis=(0, 2)) / n
    return mean, var


def reference(case, mut=None, given=None):
    """The float64 GroupNorm of a Case -> dict(z [rows][1024] (guard rows 0), u (before the activation), mean, var [ns][32], r [ns][32]).
    given: (mean, var) [ns][32] to use instead of the data's (gn_apply_kernel: the statistics are an input). mut: one of MUTATIONS."""
    c = case
    x = c.x.astype(np.float64)
    lay = c.lay
    z = np.zeros((lay.rows, CH))
    uu = np.zeros((lay.rows, CH))
    means, vars_, rs = np.zeros((lay.ns, 32)), np.zeros((lay.ns, 32)), np.zeros((lay.ns, 32))
    eps = float(np.float32(c.eps))
    if mut == "eps_wrong":
        eps = float(np.float32(1e-5 if c.eps < 5e-6 else 1e-6))
    for s in range(lay.ns):
        T, r0 = int(lay.len[s]), int(lay.start[s])
        xs = x[r0:r0 + T]
        if given is not None:
            mean, var = given[0][s], given[1][s]
        elif mut in STRUCTURAL:
            rows = mutation_rows(mut, c.kind, T)
            if rows is None:
                mean, var = group_stats(xs)
            elif mut == "admit_T":
                mean, var = group_stats(x[r0:r0 + T + 1], n=T * 32)
            else:
                keep = np.ones(T, bool)
                keep[rows] = False
                mean, var = group_stats(xs[keep], n=T * 32)
        elif mut == "n_plus":
            mean, var = group_stats(xs, n=(T + 1) * 32)
        elif mut == "n_minus" and T > 1:
            mean, var = group_stats(xs, n=(T - 1) * 32)
        else:
            mean, var = group_stats(xs)
        if mut == "unbiased":
            var = var * (T * 32.0) / (T * 32.0 - 1.0)
        if mut == "group_plus":
            mean, var = np.roll(mean, -1), np.roll(var, -1)
        if mut == "group_minus":
            mean, var = np.roll(mean, 1), np.roll(var, 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = 1.0 / (np.sqrt(var) + eps) if mut == "eps_outside" else 1.0 / np.sqrt(var + eps)
        means[s], vars_[s], rs[s] = mean, var, r
        v = (xs - np.repeat(mean, 32)[None]) * np.repeat(r, 32)[None]
        u = v * c.g.astype(np.float64)[None] + c.b.astype(np.float64)[None]
        row = c.ss_row(s, other=(mut in ("seq_step_other", "voice_other")))
        if row is not None:
            sc, sh = row[:CH].astype(np.float64), row[CH:].astype(np.float64)
            if mut == "ss_swapped":
                sc, sh = sh, sc
            u = u * (sc + (0.0 if mut == "scale_no_plus1" else 1.0))[None] + sh[None]
        uu[r0:r0 + T] = u
        silu_on, lut = c.do_silu, c.lut
        if mut == "silu_missing":
            silu_on = 0
        if mut == "silu_wrong_mode":
            lut = 0 if lut == 1 else 1
        z[r0:r0 + T] = silu_apply(u, lut) if silu_on else u
    return dict(z=z, u=uu, mean=means, var=vars_, r=rs)


def stat_bounds(kind, xs, mean, var, eps, T):
    """-> dmean [32] (absolute), rho_r [32] (relative error of rstd) of the module docstring, for one sequence xs [T][1024] float64"""
    cl = CLASS[kind]
    x3 = xs.reshape(T, 32, 32)
    m3 = mean[None, :, None]
    ad = np.abs(x3 - m3).mean(axis=(0, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        if cl["form"] == "two":
            NJ, NW = cl["NJ"], cl["NT"] // 64
            ax = np.abs(x3).mean(axis=(0, 2))
            dm = (2 + NJ + 6 + NW) * U * ax + U * np.abs(mean)
            rho_var = (2 + 1 + 2 + NJ + 6 + NW + 1) * U + 2 * dm * ad / var + dm * dm / var
        elif cl["form"] == "pivot":
            t = np.arange(T)
            w = ((T - t % 32 + 31) // 32 - t // 32).astype(np.float64)  # serial adds behind row t in its thread's chain
            p = x3[0, :, 0]
            dp = np.abs(p - mean)
            a3 = np.abs(x3 - p[None, :, None])
            n = T * 32.0
            dmd = U * ((w + 11)[:, None] * a3.sum(axis=2)).sum(axis=0) / n + U * dp
            dm = dmd + U * np.abs(mean)
            rho_var = (U * ((w + 14)[:, None] * (a3 * a3).sum(axis=2)).sum(axis=0) / n + 2 * dp * dmd + U * dp * dp) / var + U
        else:
            dm = U * np.abs(mean)
            rho_var = 2.0 ** -50 * (1 + mean * mean / var)
        rho_pe = np.where(var > 0, rho_var * var / (var + eps), 0.0) + U
        rho_r = np.where(rho_pe < 1, (1 - np.minimum(rho_pe, 0.999)) ** -0.5 - 1, np.inf) + 4 * U
    return dm, rho_r, rho_var


def silu_rel(x):
    x = np.asarray(x, np.float64)
    s = np.exp(-np.logaddexp(0.0, -x))
    return np.abs(silu(x)) * ((1 - s) * (E2 + 2 * U * np.abs(x)) + E2 + 2 * U)


def interval(case, ref=None, given=None):
    """-> (lo, hi) [rows][1024] float64: the f32 values a correct kernel of case.kind can hold in front of its output rounding; guard rows [0, 0]"""
    c = case
    ref = ref or reference(c, given=given)
    lay = c.lay
    x = c.x.astype(np.float64)
    lo, hi = np.zeros((lay.rows, CH)), np.zeros((lay.rows, CH))
    eps = float(np.float32(c.eps))
    g, b = c.g.astype(np.float64), c.b.astype(np.float64)
    for s in range(lay.ns):
        T, r0 = int(lay.len[s]), int(lay.start[s])
        xs = x[r0:r0 + T]
        mean, var, r = ref["mean"][s], ref["var"][s], ref["r"][s]
        dm, rho_r, _ = stat_bounds(c.kind, xs, mean, var, eps, T)
        e = lambda a: np.repeat(a, 32)[None]
        d = xs - e(mean)
        v = d * e(r)
        Dd = e(dm) + U * np.abs(d)
        Dv = Dd * e(r) + np.abs(v) * (e(rho_r) + U)
        u1 = v * g[None]
        D = Dv * np.abs(g)[None] + U * np.abs(u1)
        u2 = u1 + b[None]
        D = D + U * np.abs(u2)
        row = c.ss_row(s)
        if row is not None:
            sc, sh = row[:CH].astype(np.float64) + 1.0, row[CH:].astype(np.float64)
            u3 = u2 * sc[None]
            D = D * np.abs(sc)[None] + 2 * U * np.abs(u3)
            u4 = u3 + sh[None]
            D = D + U * np.abs(u4)
        else:
            u4 = u2
        a, bb = u4 - D, u4 + D
        if c.do_silu:
            if c.lut == 1:
                a, bb = rn16(a), rn16(bb)
            l, h = silu_image(a, bb)
            comp = np.maximum(silu_rel(a), silu_rel(bb))
            comp = np.where((a <= X_MIN) & (X_MIN <= bb), np.maximum(comp, silu_rel(X_MIN)), comp)
            a, bb = l - comp, h + comp
        lo[r0:r0 + T], hi[r0:r0 + T] = a, bb
    return lo, hi


def accept16(out_bits, lo, hi):
    """fp16 outputs (uint16 bits): exactly the values in [rn16(lo), rn16(hi)] -> bool per element"""
    o = np.asarray(out_bits, np.uint16).view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (rn16(lo) <= o) & (o <= rn16(hi))


def accept32(out, lo, hi):
    o = np.asarray(out, np.float64)
    with np.errstate(invalid="ignore"):
        return (lo <= o) & (o <= hi)


def excess(val, z, lo, hi, fp16):
    """How far a value lies from the reference in units of the element's tolerance: |val - z| / (half-width of [lo, hi] (+ one fp16 ulp of z)). nan -> inf."""
    val = np.asarray(val, np.float64)
    tol = 0.5 * (hi - lo) + (ulp16(z) if fp16 else 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(val == z, 0.0, np.abs(val - z) / tol)
    return np.where(np.isnan(r), np.inf, r)


# ---------------------------------------------------------------------------------------------------------------- inputs

def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def group_plan(kind, T):
    """The input family of each of the 32 groups of a sequence of T rows: [(family, spike row or None, spike channel)]"""
    cl = CLASS[kind]
    plan = [("flat", None, 0), ("offset", None, 0), ("tiny", None, 0)]
    rows = []
    for r in (0, T - 1, T) + tuple(cl["edges"]):
        if r <= T and r not in rows:  # row T is the guard row
            rows.append(r)
    for r in rows:
        for ch in (0, 31):
            fam = "outlier-pivot" if (r, ch) == (0, 0) else "guard-spike" if r == T else "spike"
            plan.append((fam, r, ch))
    assert len(plan) <= 31
    return plan + [("flat", None, 0)] * (32 - len(plan))


class Case(object):
    """One launch: a layout, x, the affine vectors, an optional scale / shift table with per-sequence rows, the activation."""

    def __init__(self, kind, lens, cfg, seed=0, pad=8, first=8, seq_rows=None, n_table=1, stride=2 * CH):
        self.kind, self.cfg = kind, cfg
        self.lay = Lay(lens, pad, first)
        self.eps, self.do_silu, self.lut, self.poison = cfg["eps"], cfg["silu"], cfg["lut"], cfg["poison"]
        rng = np.random.RandomState(_seed(kind, tuple(lens), seed))
        lay = self.lay
        x = np.zeros((lay.rows, CH))
        self.plans = []
        for s in range(lay.ns):
            T, r0 = int(lay.len[s]), int(lay.start[s])
            plan = group_plan(kind, T)
            self.plans.append(plan)
            for gi, (fam, row, ch) in enumerate(plan):
                std = 2e-3 if fam == "tiny" else 2.0 ** rng.uniform(-2, 2)
                off = 100.0 * std * rng.choice([-1, 1]) if fam == "offset" else rng.uniform(-4, 4) * (std if fam == "tiny" else 1.0)
                x[r0:r0 + T, gi * 32:(gi + 1) * 32] = off + std * rng.randn(T, 32)
                if row is not None:
                    x[r0 + row, gi * 32 + ch] = rng.choice([-1, 1]) * 64.0 * std * math.sqrt(32.0 * T) / 8.0
        self.x = x.astype(np.float32)
        if self.poison:
            self.x[~lay.row_mask()] = np.nan
        self.g = ((1.0 + 0.05 * rng.randn(CH)) * rng.choice([-1, 1], CH) * (6.0 if cfg.get("hot") else 1.0)).astype(np.float32)
        self.b = (0.1 * rng.randn(CH)).astype(np.float32)
        self.n_table, self.stride, self.seq_rows = n_table, stride, None
        self.ss = None
        if cfg["ss"]:
            tab = np.full(((n_table - 1) * stride + 2 * CH,), np.nan, np.float32)  # the floats between two rows of a wider stride are never read
            for k in range(n_table):
                tab[k * stride:k * stride + 2 * CH] = rng.uniform(-0.5, 0.5, 2 * CH)
            self.ss = tab
            self.seq_rows = None if seq_rows is None else np.asarray(seq_rows, np.int32)

    def ss_row(self, s, other=False):
        """the 2048 scale | shift floats sequence s reads (other: those of the next sequence's row, the seq_step_other / voice_other mutations)"""
        if self.ss is None:
            return None
        k = 0 if self.seq_rows is None else int(self.seq_rows[(s + 1) % self.lay.ns if other else s])
        return self.ss[k * self.stride:k * self.stride + 2 * CH]

    def name(self):
        return "%s T=%s %s" % (KIND_NAMES[self.kind], ",".join(str(int(n)) for n in self.lay.len), cfg_name(self.cfg))


def cfg_name(cfg):
    return "%s%s eps=%g%s%s" % ("ss " if cfg["ss"] else "", ("silu lut=%d" % cfg["lut"]) if cfg["silu"] else "linear", cfg["eps"], " hot" if cfg.get("hot") else "",
                               " poison" if cfg["poison"] else "")


def _cfg(ss, silu_, lut, eps, hot=0, poison=0):
    return dict(ss=ss, silu=silu_, lut=lut, eps=eps, hot=hot, poison=poison)


# every kernel that normalises to fp16 runs every length under each of these
CONFIGS = [_cfg(0, 0, 0, 1e-6), _cfg(1, 1, 0, 1e-5), _cfg(1, 1, 1, 1e-6, poison=1), _cfg(0, 1, 2, 1e-5, poison=1), _cfg(1, 1, 0, 1e-6, hot=1), _cfg(0, 0, 0, 1e-5, poison=1)]
# gn_stats_kernel alone has neither affine part nor activation; with gn_apply_f32_kernel the voice table plays the part of ss
STATS_CONFIGS = [_cfg(0, 0, 0, 1e-6), _cfg(0, 0, 0, 1e-5, poison=1)]
F32_CONFIGS = [_cfg(1, 0, 0, 1e-6), _cfg(1, 0, 0, 1e-5, poison=1)]


def configs(kind, T=1):
    """The configurations a length runs under: all of them up to 300 rows, the first three (both eps values, both table modes, poison) beyond"""
    cf = STATS_CONFIGS if kind == STATS else F32_CONFIGS if kind == STATS_APPLY_F32 else CONFIGS
    return cf if T <= 300 else cf[:3]


def stats_interval(case, ref):
    """gn_stats_kernel's own output float2 [ns][32] = (mean, rstd) -> (z, lo, hi) [ns][32][2]"""
    x = case.x.astype(np.float64)
    z = np.stack([ref["mean"], ref["r"]], axis=2)
    w = np.zeros_like(z)
    for s in range(case.lay.ns):
        dm, rho_r, _ = stat_bounds(case.kind, x[case.lay.seq_rows(s)], ref["mean"][s], ref["var"][s], float(np.float32(case.eps)), int(case.lay.len[s]))
        w[s, :, 0], w[s, :, 1] = dm, ref["r"][s] * rho_r
    return z, z - w, z + w


def single(kind, T, cfg):
    return Case(kind, [T], cfg)


def triple(kind, cfg):
    """(T, 1, T') with seq_step = (2, 0, 1) and rows 2112 floats apart where the configuration has a scale / shift table"""
    base = STATS if kind == STATS_APPLY_F32 else kind
    if kind == STATS_APPLY_F32:
        return Case(kind, TRIPLES[base], cfg, seq_rows=(2, 0, 1), n_table=3)
    return Case(kind, TRIPLES[base], cfg, seq_rows=(2, 0, 1), n_table=3, stride=2 * CH + 64)


# ---------------------------------------------------------------------------------------------------------------- fixed-point statistics (gn_apply_kernel)

def fx_split(p):
    """gemm_f16.h's fx_split restated: f32 -> (hi in units of 2^-8, lo in units of 2^-60) int64"""
    p = np.asarray(p, np.float32)
    h = np.rint(p * np.float32(256.0)).astype(np.float32)
    rem = (p - h * np.float32(1.0 / 256.0)).astype(np.float32)
    return h.astype(np.int64), np.rint(rem * np.float32(4503599627370496.0)).astype(np.float32).astype(np.int64)


def stripes(case, seed=1):
    """Fixed-point statistics of a case's x as the GEMM epilogues leave them, the sums spread unevenly over the 8 stripes -> (st int64 [8][ns][32][4], mean, var
    [ns][32]: what those integers say, in float64 — gn_apply_kernel takes them as given)."""
    lay = case.lay
    rng = np.random.RandomState(_seed("stripes", case.kind, tuple(lay.len), seed))
    st = np.zeros((FX_STRIPES, lay.ns, 32, 4), np.int64)
    x = case.x.astype(np.float64)
    for s in range(lay.ns):
        x3 = x[lay.seq_rows(s)].reshape(-1, 32, 32)
        for q, tot in enumerate((x3.sum(axis=(0, 2)), (x3 * x3).sum(axis=(0, 2)))):
            w = rng.uniform(-1, 1, (FX_STRIPES - 1, 32)) * np.array([4, 1, 0.25, 0, 1e-3, 2, 1], np.float64)[:, None]  # one stripe untouched, one nearly so
            parts = (w * tot[None]).astype(np.float32)
            last = (tot - parts.astype(np.float64).sum(axis=0)).astype(np.float32)
            for k, p in enumerate(list(parts) + [last]):
                st[k, s, :, 2 * q], st[k, s, :, 2 * q + 1] = fx_split(p)
    tot = st.sum(axis=0)
    n = (lay.len.astype(np.float64) * 32.0)[:, None]
    val = lambda hi, lo: hi.astype(np.float64) / 256.0 + lo.astype(np.float64) / 2.0 ** 60
    mean = val(tot[..., 0], tot[..., 1]) / n
    var = np.maximum(val(tot[..., 2], tot[..., 3]) / n - mean * mean, 0.0)
    return np.ascontiguousarray(st), mean, var


# ---------------------------------------------------------------------------------------------------------------- f32 restatements (the bound is not too tight)

def f32_restatement(case, given=None):
    """A correct float32 implementation of case.kind's reduction form and affine chain with NumPy's own summation order -> (z f32 [rows][1024] in front of the
    output rounding (lut = 1: after it), mean, rstd f32 [ns][32])."""
    c, f = case, np.float32
    lay = c.lay
    form = CLASS[c.kind]["form"]
    z = np.zeros((lay.rows, CH), f)
    means, rstds = np.zeros((lay.ns, 32), f), np.zeros((lay.ns, 32), f)
    eps = f(c.eps)
    for s in range(lay.ns):
        T = int(lay.len[s])
        xs = c.x[lay.seq_rows(s)]
        x3 = xs.reshape(T, 32, 32)
        n = f(T * 32)
        if form == "two":
            mean = x3.sum(axis=(0, 2), dtype=f) / n
            d3 = x3 - mean[None, :, None]
            rstd = f(1) / np.sqrt((d3 * d3).sum(axis=(0, 2), dtype=f) / n + eps)
        elif form == "pivot":
            p = x3[0, :, 0]
            d3 = x3 - p[None, :, None]
            md = d3.sum(axis=(0, 2), dtype=f) / n
            var = np.maximum((d3 * d3).sum(axis=(0, 2), dtype=f) / n - md * md, f(0))
            mean, rstd = p + md, f(1) / np.sqrt(var + eps)
        else:
            mean = given[0][s].astype(f)
            rstd = (1.0 / np.sqrt(given[1][s] + float(eps))).astype(f)
        means[s], rstds[s] = mean, rstd
        u = (xs - np.repeat(mean, 32)[None]) * np.repeat(rstd, 32)[None]
        u = u * c.g[None]
        u = u + c.b[None]
        row = c.ss_row(s)
        if row is not None:
            u = u * (row[:CH] + f(1))[None]
            u = u + row[CH:][None]
        if c.do_silu:
            if c.lut == 1:
                with np.errstate(over="ignore"):
                    u = u.astype(np.float16).astype(f)
                    u = (u / (f(1) + np.exp(-u))).astype(np.float16).astype(f)
            else:
                with np.errstate(over="ignore"):
                    u = u / (f(1) + np.exp(-u))
        assert u.dtype == f
        z[lay.seq_rows(s)] = u
    return z, means, rstds


# ---------------------------------------------------------------------------------------------------------------- running

def run(case, kind=None, out_rows=None, x=None, lay=None, row0=0, x_rows=None, touch=None, st=None, ss=None, seq_rows="case", picked=None):
    """One launch of `case` (kind: another kernel for the same case, e.g. AUTO) -> Guarded output. Asserts success and intact canaries.
    lay / row0 / x_rows: launch a part (relative starts) of the buffers x. touch: (pf0, lines0, pf1, lines1). ss / seq_rows: override the table."""
    c = case
    kind = c.kind if kind is None else kind
    lay = lay or c.lay
    x = c.x if x is None else x
    x_rows = x.shape[0] if x_rows is None else x_rows
    if kind == STATS:
        out = Guarded((lay.ns, 32, 2), np.float32)
    elif kind == STATS_APPLY_F32:
        out = Guarded((lay.rows, CH), np.float32)
    else:
        out = Guarded((x_rows if kind <= AUTO else lay.rows, CH), np.uint16)
    kw = dict(ns=lay.ns, rows_total=lay.rows, row0=row0, x_rows=x_rows, start=lay.start, len=lay.len, x=x, eps=c.eps)
    if kind not in (STATS, TO_F16):
        kw.update(g=c.g, b=c.b, do_silu=c.do_silu, lut=c.lut)
        sr = c.seq_rows if isinstance(seq_rows, str) else seq_rows
        tab = c.ss if ss is None else ss
        if tab is not None:
            kw.update(ss=tab, n_steps=c.n_table if ss is None else 1, ss_step_stride=c.stride)
            if sr is not None:
                kw["seq_voice" if kind == STATS_APPLY_F32 else "seq_step"] = np.ascontiguousarray(sr, np.int32)
    if touch:
        kw.update(pf0=touch[0], pf0_lines=touch[1], pf0_bytes=0 if touch[0] is None else touch[0].nbytes,
                  pf1=touch[2], pf1_lines=touch[3], pf1_bytes=0 if touch[2] is None else touch[2].nbytes)
    if st is not None:
        kw["st"] = st
    pk = C.c_int(-1)
    cs = struct(kind, out=out, picked=C.cast(C.pointer(pk), C.c_void_p), **kw)
    rc = harness().tts_gn_test_run(C.byref(cs))
    assert rc == 0, "harness returned HIP error %d" % rc
    assert out.canaries_intact(), "a kernel wrote outside its output buffer"
    if picked is not None:
        picked.append(pk.value)
    return out
