"""Shared by tests/test_gemm_kernels_gpu.py and tests/test_gemm_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/gemm_harness.hip -> libtts_gemm_test.so), the float64 NumPy reference of launch_gemm_f16 written from the formula in
csrc/gemm_f16.h, and the case matrix of the exact tests.

    C[m][n] = sum_seg sum_k A_seg[m + row_off_seg][k] * W[n][w_off_seg + k]          then the mode's epilogue

The reference shares no code with the harness or the kernels; test_gemm_harness_cpu.py checks it against naive loops.

EXACT CASES. Operands are fp16-exact integers (one variant: integers x 2^-24, fp16 subnormals), bias and residual integers, alpha a power of two. Then every f32
value a kernel can form — any partial sum of products in any order, the accumulator that starts from resid / alpha, alpha * acc, + bias, + resid, and for the
STATS modes the per-chunk sums and sums of squares — is a multiple of one power of two q with magnitude below 2^24 q, hence exactly representable, and the
float64 reference rounded ONCE to the output type must equal the kernel's output bit for bit. `exactness()` evaluates that condition on the reference side
(an upper bound of every partial sum over q); `operands()` narrows the value range of a case until it holds and never drops a case."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.path.join(PKG, "libtts_gemm_test.so")
SRC = os.path.join(PKG, "testlib", "gemm_harness.hip")

F32, F16, QKV, QKV_SPLIT, F32_SCALED, F32_STATS, F32_SCALED_STATS = range(7)
MODE_NAMES = ["F32", "F16", "QKV", "QKV_SPLIT", "F32_SCALED", "F32_STATS", "F32_SCALED_STATS"]
F32_MODES = (F32, F32_SCALED, F32_STATS, F32_SCALED_STATS)
SCALED_MODES = (F32_SCALED, F32_SCALED_STATS)
STATS_MODES = (F32_STATS, F32_SCALED_STATS)
QKV_MODES = (QKV, QKV_SPLIT)
FX_STRIPES = 8
SENTINEL = 0xCB
HIP_INVALID_VALUE = 1


class CaseStruct(C.Structure):
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("nseg", C.c_int), ("kseg", C.c_int),
                ("row_off", C.c_int * 3), ("a_sel", C.c_int * 3),
                ("mode", C.c_int), ("th", C.c_int), ("ku", C.c_int), ("wreg", C.c_int), ("dual_b", C.c_int), ("custom_w", C.c_int), ("ldw", C.c_int),
                ("w_off", C.c_int * 3), ("alpha", C.c_float),
                ("has_bias", C.c_int), ("has_resid", C.c_int), ("resid_aliases_out", C.c_int), ("has_row_seq", C.c_int), ("has_chunk_seq", C.c_int),
                ("has_st", C.c_int),
                ("lda", C.c_int), ("ldo", C.c_int), ("ldh", C.c_int), ("ldvt", C.c_int), ("nseq", C.c_int), ("st_stripe_ll", C.c_int), ("launches", C.c_int),
                ("A0", C.c_void_p), ("A1", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("resid", C.c_void_p),
                ("row_seq", C.c_void_p), ("chunk_seq", C.c_void_p),
                ("outF", C.c_void_p), ("outH", C.c_void_p), ("outH2", C.c_void_p), ("outVt", C.c_void_p), ("outVt2", C.c_void_p), ("st", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_gemm_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_gemm_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_gemm_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_gemm_test_plan.argtypes = [C.POINTER(CaseStruct), C.c_char_p, C.c_int]
        L.tts_gemm_test_last_kernel.argtypes = [C.c_char_p, C.c_int]
        L.tts_gemm_test_auto_th.argtypes = [C.c_int, C.c_int]
        for f in (L.tts_gemm_test_run, L.tts_gemm_test_plan, L.tts_gemm_test_last_kernel, L.tts_gemm_test_auto_th, L.tts_gemm_test_margin):
            f.restype = C.c_int
        _lib = L
    return _lib


# ---------------------------------------------------------------------------------------------------------------- cases

def layout(lens):
    """The diffusion stage's packing of ragged sequences along M (diffusion.hip, Layout::build): first sequence at row 8, at least one guard row behind each,
    starts at multiples of 8, rows rounded up to 128. -> rows, row_seq [rows] (-1: guard), chunk_seq [rows / 8] (-1: guard rows only), starts"""
    r, start = 8, []
    for n in lens:
        start.append(r)
        r = (r + n + 1 + 7) & ~7
    rows = (r + 127) & ~127
    rs = np.full(rows, -1, np.int32)
    cs = np.full(rows // 8, -1, np.int32)
    for s, (b, n) in enumerate(zip(start, lens)):
        rs[b:b + n] = s
        cs[b >> 3:((b + n - 1) >> 3) + 1] = s
    return rows, rs, cs, start


RAGGED = [5, 14, 31, 8, 64, 1, 23, 42, 11, 3, 17, 26, 47, 12, 9, 36, 2, 21, 58, 7, 29, 13, 4, 19, 35, 10, 6, 27, 45, 15, 22, 33]  # 896 packed rows
RAGGED_SMALL = [5, 14, 31, 8, 1, 23, 11]  # 128 packed rows


class Case(object):
    """One launch. rows: None (no row_seq), 'valid' (all rows >= 0), or a list of sequence lengths (packed by layout(); M follows from it).
    resid: None, 'sep', 'alias'. a_sel: activation buffer of each segment. sub: operand A in fp16 subnormals (integers x 2^-24)."""
    DEFAULTS = dict(M=128, N=128, nseg=1, kseg=64, row_off=(0, 0, 0), a_sel=(0, 0, 0), mode=F32, th=0, ku=0, wreg=0, dual_b=0, custom_w=0, ldw=0,
                    w_off=(0, 0, 0), alpha=0.5, bias=True, resid=None, rows=None, sub=False, pad=0, launches=1, tag="")

    def __init__(self, **kw):
        d = dict(self.DEFAULTS)
        bad = set(kw) - set(d)
        assert not bad, bad
        d.update(kw)
        self.__dict__.update(d)
        if isinstance(self.rows, (list, tuple)):
            self.M = layout(self.rows)[0]
        if self.mode in STATS_MODES and self.rows is None:
            self.rows = "valid"

    @property
    def ktot(self):
        return self.nseg * self.kseg

    @property
    def w_cols(self):
        return self.ldw if self.custom_w else self.nseg * self.kseg

    @property
    def offs(self):
        return list(self.w_off[:self.nseg]) if self.custom_w else [s * self.kseg for s in range(self.nseg)]

    @property
    def name(self):
        p = [self.tag or "case", MODE_NAMES[self.mode], "M%d" % self.M, "N%d" % self.N, "K%dx%d" % (self.nseg, self.kseg), "th%d" % self.th, "ku%d" % self.ku]
        for flag in ("wreg", "dual_b", "custom_w", "sub"):
            if getattr(self, flag):
                p.append(flag)
        if not self.bias:
            p.append("nobias")
        if self.resid:
            p.append("resid_" + self.resid)
        if self.rows is not None:
            p.append("rows_" + (self.rows if isinstance(self.rows, str) else "ragged%d" % len(self.rows)))
        if self.launches > 1:
            p.append("x%d" % self.launches)
        return "-".join(p)


def conv3(**kw):
    return Case(nseg=3, row_off=(-1, 0, 1), tag="conv3", **kw)


def dualb(kseg, **kw):
    """hi | lo halves of one weight side by side in one [N][2 kseg] matrix, one activation operand"""
    kw.setdefault("mode", F32_SCALED)
    return Case(nseg=2, kseg=kseg, dual_b=1, custom_w=1, ldw=2 * kseg, w_off=(0, kseg, 0), tag="dualb", **kw)


# M with uneven per-XCD block ranges (nb * x >> 3): range lengths {1,2} {3,4} {5,6} {7,8} {9,10} -> with th = 8 the last tile of a range has 1 .. 8 blocks,
# i.e. wave rows of 0 .. 4 blocks (every MI body); M = 16 is one block on one XCD.
UNEVEN_M = [16, 144, 432, 688, 944, 1200]


def static_cases():
    c = []
    # generic kernel, one segment: every mode, every uneven M, th = 8 (all MI bodies) and auto
    for mode in range(7):
        n = 384 if mode in QKV_MODES else 128
        for M in UNEVEN_M:
            c.append(Case(tag="vh", mode=mode, M=M, N=n, kseg=128, th=8, rows="valid" if mode in STATS_MODES else None))
        c.append(Case(tag="vh", mode=mode, M=432, N=n, kseg=192, th=0, resid="sep" if mode in F32_MODES else None))
    # every explicit tile height (ranges of 7 and 8 blocks: last tiles of every length), three kernels
    for th in range(1, 9):
        c.append(Case(tag="vh", M=944, N=256, kseg=128, th=th, resid="alias"))
        c.append(Case(tag="vh", mode=F32_STATS, M=944, N=128, kseg=64, th=th, rows=RAGGED))
        c.append(conv3(M=944, N=128, kseg=64, th=th, resid="sep"))
        c.append(dualb(128, M=944, N=128, th=th, resid="sep"))
        c.append(Case(tag="vh", mode=QKV, M=688, N=384, kseg=64, th=th))
    # K tiles per barrier pair, with the kseg values that make the launcher fall back to one
    for ku in (0, 1, 2, 4):
        for kseg in (64, 128, 192, 256, 1024):
            c.append(Case(tag="vh", M=432, N=128, kseg=kseg, th=3, ku=ku))
        c.append(Case(tag="vh", mode=F16, M=144, N=256, nseg=2, a_sel=(0, 1, 0), kseg=256, ku=ku))
        c.append(Case(tag="vh", mode=F32_SCALED_STATS, M=256, N=256, kseg=512, ku=ku, resid="sep", rows=RAGGED_SMALL, alpha=2.0))
        c.append(dualb(192, M=432, N=128, ku=ku, th=4))
        c.append(dualb(256, M=432, N=256, ku=ku, th=5, mode=F32_SCALED_STATS, rows="valid", alpha=0.25))
    # segment structures: channel concat of two buffers; three custom segments (shifted rows, permuted weight columns, a gap in ldw) that are NOT the k = 3 kernel
    for mode in (F32, F16, F32_SCALED, F32_STATS):
        c.append(Case(tag="concat", mode=mode, M=688, N=256, nseg=2, a_sel=(0, 1, 0), kseg=128, th=8, resid="sep" if mode != F16 else None))
        c.append(Case(tag="custom3", mode=mode, M=432, N=128, nseg=3, kseg=64, custom_w=1, ldw=320, w_off=(192, 0, 96), row_off=(-1, 0, 1), a_sel=(0, 1, 0)))
    c.append(Case(tag="concat", M=1152, N=1152, nseg=2, a_sel=(0, 1, 0), kseg=1024, resid="alias"))  # NT = 9: cn = 3, the real 2 x 1024 total
    c.append(Case(tag="custom3", M=256, N=1024, nseg=3, kseg=1024, custom_w=1, ldw=3072, w_off=(2048, 0, 1024), rows=RAGGED_SMALL))
    # k = 3 convolution
    for mode in (F32, F32_STATS, F16):
        for M in UNEVEN_M:
            c.append(conv3(mode=mode, M=M, N=128, kseg=64, th=8))
        for resid in ((None, "sep", "alias") if mode != F16 else (None,)):
            c.append(conv3(mode=mode, N=256, kseg=128, rows=RAGGED, resid=resid))
            c.append(conv3(mode=mode, N=128, kseg=192, rows=RAGGED, resid=resid, bias=False, th=7))
    c.append(conv3(M=256, N=1024, kseg=1024, rows=RAGGED_SMALL, resid="sep"))  # the real 3 x 1024
    c.append(conv3(mode=F32_STATS, M=256, N=1024, kseg=1024, rows=RAGGED_SMALL))
    c.append(conv3(M=432, N=1152, kseg=256, th=8))
    # split-precision weight (dual-B)
    for mode in (F32_SCALED, F32_SCALED_STATS):
        for M in UNEVEN_M:
            c.append(dualb(64, mode=mode, M=M, N=128, th=8, rows="valid" if mode in STATS_MODES else None))
        for resid in (None, "sep", "alias"):
            c.append(dualb(256, mode=mode, N=1024, rows=RAGGED, resid=resid, alpha=4.0))  # auto: th = 4, ku = 2 (small-problem rule)
        c.append(dualb(1024, mode=mode, N=256, rows=RAGGED_SMALL, bias=False, alpha=0.125))
    # weight through registers: 128-row tiles, >= 2 K tiles; kseg = 64 must stay with the LDS-staged kernel
    for mode in (F32, QKV, QKV_SPLIT):
        n = 384 if mode in QKV_MODES else 128
        for M in UNEVEN_M:
            c.append(Case(tag="wreg", mode=mode, wreg=1, M=M, N=n, kseg=128, th=8))
        c.append(Case(tag="wreg", mode=mode, wreg=1, M=432, N=n, kseg=64, th=8))
        c.append(Case(tag="wreg", mode=mode, wreg=1, N=n, kseg=192, th=8, rows=RAGGED, bias=False))
        c.append(Case(tag="wreg", mode=mode, wreg=1, M=2560, N=3072, kseg=128))  # auto height 8 at the QKV width
        c.append(Case(tag="wreg", mode=mode, wreg=1, N=1152, kseg=2048, th=8, rows=RAGGED_SMALL))  # cn = 3
        c.append(Case(tag="wreg", mode=mode, wreg=1, M=688, N=768 if mode in QKV_MODES else 1024, kseg=1024, th=8, pad=8))
    for resid in ("sep", "alias"):
        c.append(Case(tag="wreg", wreg=1, M=1200, N=256, kseg=256, th=8, resid=resid))
    # residual x bias x row_seq on the generic kernel; leading dimensions wider than the payload
    for resid in (None, "sep", "alias"):
        for bias in (True, False):
            for rows in (None, "valid", RAGGED):
                c.append(Case(tag="vh", M=896, N=256, kseg=128, resid=resid, bias=bias, rows=rows, pad=24))
    for mode in (F16, QKV, QKV_SPLIT, F32_SCALED, F32_STATS, F32_SCALED_STATS):
        c.append(Case(tag="vh", mode=mode, N=384 if mode in QKV_MODES else 256, kseg=128, rows=RAGGED, pad=8, resid="alias" if mode in F32_MODES else None))
    c.append(Case(tag="vh", mode=QKV, M=432, N=3072, kseg=128, th=8))       # column tiles start inside q, k and v spans; cn = 8
    c.append(Case(tag="vh", mode=QKV_SPLIT, M=144, N=3072, kseg=1024))
    c.append(Case(tag="vh", mode=QKV, M=144, N=1152, kseg=2048, th=3))      # cn = 3
    # the STATS epilogue accumulates: a second launch doubles the records
    c.append(Case(tag="vh", mode=F32_STATS, N=1024, kseg=256, rows=RAGGED, launches=2))
    c.append(conv3(mode=F32_STATS, N=256, kseg=64, rows=RAGGED, launches=2))
    c.append(dualb(128, mode=F32_SCALED_STATS, N=256, rows=RAGGED, launches=2))
    # fp16 subnormal operands
    for mode in (F32, F16, QKV_SPLIT, F32_SCALED):
        c.append(Case(tag="vh", mode=mode, M=432, N=384, kseg=128, th=8, sub=True))
    c.append(conv3(M=432, N=128, kseg=128, sub=True))
    c.append(conv3(mode=F16, M=144, N=128, kseg=64, sub=True))
    c.append(dualb(128, M=432, N=128, sub=True))
    c.append(Case(tag="wreg", wreg=1, M=432, N=128, kseg=128, th=8, sub=True))
    c.append(Case(tag="wreg", mode=QKV, wreg=1, M=432, N=384, kseg=128, th=8, sub=True))
    return c


BOUNDARY_N = (128, 256, 1024, 3072)
BOUNDARY_M_MAX = 70000


def _auto_th(M, N):
    """gemm_auto_th restated (test_gemm_harness_cpu.py compares it with the library's over the whole sweep)"""
    maxb, NT, th = ((M >> 4) + 7) // 8 + 1, N >> 7, 2
    while th < 8 and 8 * ((maxb + th - 1) // th) * NT > 1024:
        th *= 2
    return th


def _small_rule(M, N):
    """the launcher's small-problem rule (th = 4, KU = 4) for th = 0, ku = 0, kseg % 256 == 0"""
    maxb, NT = ((M >> 4) + 7) // 8 + 1, N >> 7
    return NT <= 8 and 8 * ((maxb + 3) // 4) * NT <= 256


def boundaries(N):
    """every M (multiple of 16) at which the chosen height or the KU = 4 rule differs from M - 16"""
    out, prev = [], None
    for M in range(16, BOUNDARY_M_MAX + 1, 16):
        cur = (_auto_th(M, N), _small_rule(M, N))
        if prev is not None and cur != prev:
            out.append(M)
        prev = cur
    return out


def boundary_cases():
    """an exact case at each boundary, at the last M before it, and one block to either side of the pair; kseg = 256 keeps the KU = 4 rule live"""
    c = []
    for N in BOUNDARY_N:
        ms = sorted({M + d for M in boundaries(N) for d in (-32, -16, 0, 16)})
        for M in ms:
            c.append(Case(tag="boundary", M=M, N=N, kseg=256, wreg=1 if N == 3072 else 0, bias=(M // 16) % 2 == 0))
    return c


def exact_cases():
    return static_cases() + boundary_cases()


# ---------------------------------------------------------------------------------------------------------------- operands

def _seed(case):
    import zlib
    return zlib.crc32(case.name.encode()) & 0x7FFFFFFF


def _int_operands(case, r, density, blim, rlim):
    rs = np.random.RandomState(_seed(case))
    M, N = case.M, case.N

    def ints(shape, lim, dens=1.0):
        v = rs.randint(-lim, lim + 1, size=shape).astype(np.float64)
        if dens < 1.0:
            v *= rs.rand(*shape) < dens
        return v
    ops = {}
    rows, row_seq, chunk_seq, nseq = None, None, None, 1
    if isinstance(case.rows, (list, tuple)):
        rows, row_seq, chunk_seq, _ = layout(case.rows)
        nseq = len(case.rows)
    elif case.rows == "valid":
        row_seq = np.zeros(M, np.int32)
        chunk_seq = np.zeros(M // 8, np.int32)
    a_scale = 2.0 ** -24 if case.sub else 1.0
    for b in range(1 + max(case.a_sel[:case.nseg])):
        A = ints((M + 2, case.kseg + case.pad), r, density) * a_scale  # rows -1 .. M; the rows outside 0 .. M - 1 are non-zero unless the layout says guard
        if rows is not None:
            A[1:M + 1][row_seq < 0] = 0  # the product keeps guard rows (and the halo rows) of every GEMM operand zero
            A[0] = 0
            A[M + 1] = 0
        ops["A%d" % b] = A.astype(np.float16)
        assert (ops["A%d" % b].astype(np.float64) == A).all()
    W = ints((N, case.w_cols), r, density)
    ops["W"] = W.astype(np.float16)
    out_scale = a_scale
    if case.bias:
        ops["bias"] = (ints((N,), blim) * out_scale).astype(np.float32)
    if case.resid:
        ops["resid"] = (ints((M, N + case.pad), rlim) * out_scale).astype(np.float32)
    if row_seq is not None:
        ops["row_seq"] = row_seq
    if case.mode in STATS_MODES:
        ops["chunk_seq"] = chunk_seq
    ops["nseq"] = nseq
    ops["ra"], ops["rw"], ops["rb"], ops["rr"], ops["unit"] = r, r, blim, rlim, out_scale
    return ops


def exactness(case, ops, ref=None):
    """Largest magnitude any f32 intermediate of the case can reach, in units of the power of two q all of them are multiples of. < 2^24 <=> all exact.
    Upper bounds only: sum_k |a||w| <= ktot * max|a| * max|w|; the STATS partial sums are bounded by the per-chunk totals of |x| and x^2 of the reference."""
    u = ops["unit"]
    alpha = case.alpha if case.mode in SCALED_MODES else 1.0
    s = case.ktot * ops["ra"] * ops["rw"]                     # |any partial sum of products| / u
    b = ops["rb"] if case.bias else 0
    r = ops["rr"] if case.resid else 0
    q_acc = min(1.0, 1.0 / alpha)                              # the accumulator may start from resid / alpha
    worst = (s + r / alpha) / q_acc
    q_out = min(1.0, alpha)
    worst = max(worst, (alpha * s + r + b) / q_out)
    if case.mode in STATS_MODES:
        if ref is None:
            ref = reference(case, ops)
        x = np.abs(ref["x"]) / u / q_out
        M, N = x.shape
        xc = x.reshape(M // 8, 8, N // 32, 32)
        worst = max(worst, xc.sum(axis=(1, 3)).max(), (xc * xc).sum(axis=(1, 3)).max())
    return worst


def operands(case):
    """integer operands of the widest range in the ladder for which the exactness condition holds"""
    for ladder in ((4, 1.0, 64, 1024), (3, 1.0, 64, 256), (2, 1.0, 32, 64), (1, 1.0, 16, 32), (1, 0.5, 8, 16), (1, 0.25, 4, 8), (1, 0.1, 2, 4), (1, 0.03, 1, 2)):
        ops = _int_operands(case, *ladder)
        if exactness(case, ops) < 2.0 ** 24:
            return ops
    raise AssertionError("no operand range makes %s exact" % case.name)


# ---------------------------------------------------------------------------------------------------------------- reference

def round_f16(x):
    return np.asarray(x, np.float64).astype(np.float16)


def reference(case, ops):
    """float64. 'x': the values the mode stores, before the rounding to the output type; then the outputs as the epilogue lays them out."""
    M, N, ks = case.M, case.N, case.kseg
    W = ops["W"].astype(np.float64)
    acc = np.zeros((M, N))
    for s in range(case.nseg):
        A = ops["A%d" % case.a_sel[s]].astype(np.float64)
        rows = A[1 + case.row_off[s]:1 + case.row_off[s] + M, :ks]   # buffer row 0 is row -1 of the layout
        acc += np.einsum("mk,nk->mn", rows, W[:, case.offs[s]:case.offs[s] + ks], optimize=True)
    x = acc * case.alpha if case.mode in SCALED_MODES else acc
    if case.bias:
        x = x + ops["bias"].astype(np.float64)[None, :]
    if case.resid:
        x = x + ops["resid"].astype(np.float64)[:, :N]
    guard = ops["row_seq"] < 0 if "row_seq" in ops else np.zeros(M, bool)
    x = np.where(guard[:, None], 0.0, x)
    out = {"x": x, "acc": acc}
    if case.mode in F32_MODES:
        out["outF"] = x.astype(np.float32)
    elif case.mode == F16:
        out["outH"] = round_f16(x)
    else:
        heads = N // 192
        xh = x.reshape(M, heads, 192)
        qk, v = xh[:, :, :128].reshape(M, heads * 128), xh[:, :, 128:].transpose(1, 2, 0).reshape(heads * 64, M)
        out["outH"], out["outVt"] = round_f16(qk), round_f16(v)
        if case.mode == QKV_SPLIT:
            out["outH2"] = round_f16(qk - out["outH"].astype(np.float64))
            out["outVt2"] = round_f16(v - out["outVt"].astype(np.float64))
    if case.mode in STATS_MODES:
        stored = out["outF"].astype(np.float64)
        st = np.zeros((ops["nseq"], N // 32, 2))
        for ch, s in enumerate(ops["chunk_seq"]):
            if s >= 0:
                blk = stored[8 * ch:8 * ch + 8].reshape(8, N // 32, 32)
                st[s, :, 0] += blk.sum(axis=(0, 2))
                st[s, :, 1] += (blk * blk).sum(axis=(0, 2))
        out["stats"] = st * case.launches
    return out


def abs_product_sum(case, ops):
    """sum_seg sum_k |a||w| per output element: the scale of the accumulation error bound"""
    M, ks = case.M, case.kseg
    W = np.abs(ops["W"].astype(np.float64))
    acc = np.zeros((M, case.N))
    for s in range(case.nseg):
        A = np.abs(ops["A%d" % case.a_sel[s]].astype(np.float64))
        acc += A[1 + case.row_off[s]:1 + case.row_off[s] + M, :ks] @ W[:, case.offs[s]:case.offs[s] + ks].T
    return acc


def wfrag_index(n, k, K):
    """gemm_wfrag_index restated: Wf[n / 16][k / 32][lane = ((k % 32) / 8) * 16 + n % 16][k % 8]"""
    return ((((n >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k >> 3) & 3) * 16 + (n & 15)) << 3) + (k & 7)


def fx_value(hi, lo):
    """the header's fx_value: hi in units of 2^-8, lo in units of 2^-60"""
    return hi.astype(np.float64) / 256.0 + lo.astype(np.float64) / 2.0 ** 60


# ---------------------------------------------------------------------------------------------------------------- running

def fill_struct(case, ops, outs=None, keep=None, **override):
    """the C struct of a case; `keep` collects the arrays the struct points to"""
    keep = keep if keep is not None else []
    s = CaseStruct()
    M, N = case.M, case.N
    s.M, s.N, s.nseg, s.kseg = M, N, case.nseg, case.kseg
    s.row_off, s.a_sel = (C.c_int * 3)(*case.row_off), (C.c_int * 3)(*case.a_sel)
    s.mode, s.th, s.ku, s.wreg, s.dual_b, s.custom_w, s.ldw = case.mode, case.th, case.ku, case.wreg, case.dual_b, case.custom_w, case.ldw
    s.w_off = (C.c_int * 3)(*case.w_off)
    s.alpha = case.alpha
    s.lda = case.kseg + case.pad
    s.ldo = s.ldh = N + case.pad
    if case.mode in QKV_MODES:
        s.ldh = N // 192 * 128 + case.pad
    s.ldvt = M + case.pad
    s.launches = case.launches
    s.nseq = ops["nseq"]

    def ptr(a):
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data
    s.A0 = ptr(ops["A0"])
    if "A1" in ops:
        s.A1 = ptr(ops["A1"])
    s.W = ptr(ops["W"])
    if case.bias:
        s.has_bias, s.bias = 1, ptr(ops["bias"])
    if case.resid:
        s.has_resid, s.resid, s.resid_aliases_out = 1, ptr(ops["resid"]), int(case.resid == "alias")
    if "row_seq" in ops:
        s.has_row_seq, s.row_seq = 1, ptr(ops["row_seq"])
    if case.mode in STATS_MODES:
        s.has_chunk_seq, s.chunk_seq = 1, ptr(ops["chunk_seq"])
        s.has_st, s.st_stripe_ll = 1, ops["nseq"] * 32 * 4 + 8
    for k, v in override.items():
        setattr(s, k, v)
    if outs is not None:
        for k, a in outs.items():
            setattr(s, k, a.ctypes.data)
    return s


def out_buffers(case, ops, margin, stripe_ll=None):
    """host buffers margin | payload | margin, as raw bytes, zero-filled (the harness overwrites all of it)"""
    M, N, pad = case.M, case.N, case.pad
    heads = N // 192
    sizes = {}
    if case.mode in F32_MODES:
        sizes["outF"] = M * (N + pad) * 4
    elif case.mode == F16:
        sizes["outH"] = M * (N + pad) * 2
    else:
        sizes["outH"] = M * (heads * 128 + pad) * 2
        sizes["outVt"] = heads * 64 * (M + pad) * 2
        if case.mode == QKV_SPLIT:
            sizes["outH2"], sizes["outVt2"] = sizes["outH"], sizes["outVt"]
    if case.mode in STATS_MODES:
        sizes["st"] = FX_STRIPES * (ops["nseq"] * 32 * 4 + 8 if stripe_ll is None else stripe_ll) * 8
    return {k: np.zeros(v + 2 * margin, np.uint8) for k, v in sizes.items()}


def payload(buf, margin, dtype, shape):
    return buf[margin:len(buf) - margin].view(dtype).reshape(shape)
