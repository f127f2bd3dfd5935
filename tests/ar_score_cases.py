"""The case matrix of the AR scoring kernels and the binding of their test-only harness (tortoise.cpp_amd/testlib/ar_score_harness.hip -> libtts_score_test.so).
Used by tests/test_ar_score_kernels_gpu.py (launches) and tests/test_ar_score_cpu.py (validation, float32 restatement, seeded defects; no GPU).

Shapes: the full head (N = 8194 valid of NPAD = 8256 columns, K = 1024: 33 slabs, the last with 2 valid columns) at 130 rows, of which the launches take the first
1, 63, 64, 65 and all 130 (three row tiles, the last ragged); one reduced shape (N = 290 of NPAD = 320, K = 64: two slabs, the second with two tiles, so two of its
waves have none). A row's reference does not depend on the rows beside it: the float64 side is computed once at 130 rows and sliced."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import ar_score_ref as R

f32, f64, i32 = np.float32, np.float64, np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_SCORE_TEST_LIB", os.path.join(PKG, "libtts_score_test.so"))
HIP_INVALID_VALUE = 1
SENTINEL = 0xCB
FULL = dict(N=8194, NPAD=8256, K=1024)
SMALL = dict(N=290, NPAD=320, K=64)
FULL_ROWS = (1, 63, 64, 65, 130)
PAD_VALUE = 1e30  # what the pad columns of W and b hold in every case: they must have no effect


class CaseStruct(C.Structure):
    _fields_ = [("R", C.c_int), ("K", C.c_int), ("N", C.c_int), ("NPAD", C.c_int), ("hn", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p), ("tgt", C.c_void_p),
                ("lse", C.c_void_p), ("logp", C.c_void_p), ("stop_logp", C.c_void_p), ("greedy", C.c_void_p), ("tgt_logit", C.c_void_p), ("stop_logit", C.c_void_p)]


OUTS = (("lse", f32), ("logp", f32), ("stop_logp", f32), ("greedy", i32), ("tgt_logit", f32), ("stop_logit", f32))
_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_score_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_score_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_score_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_score_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_score_test_lds.argtypes = [C.c_int]
        for f in (L.tts_score_test_run, L.tts_score_test_validate, L.tts_score_test_margin, L.tts_score_test_tile, L.tts_score_test_slab, L.tts_score_test_lds):
            f.restype = C.c_int
        _lib = L
    return _lib


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, n, dtype):
        self.margin = harness().tts_score_test_margin()
        self.dtype = dtype
        self.raw = np.zeros(2 * self.margin + n * 4, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


class Case(object):
    """hn [R][K], W [K][NPAD] (row-major; the harness lays it out as the loader does), b [NPAD], tgt [R]; planted [R]: the lower index of a planted exact tie, or -1."""

    def __init__(self, label, hn, W, b, tgt, N, planted=None):
        self.label, self.N = label, N
        self.hn, self.W, self.b, self.tgt = (np.ascontiguousarray(hn, f32), np.ascontiguousarray(W, f32), np.ascontiguousarray(b, f32), np.ascontiguousarray(tgt, i32))
        self.R, self.K, self.NPAD = self.hn.shape[0], self.W.shape[0], self.W.shape[1]
        self.planted = np.full(self.R, -1, i32) if planted is None else np.asarray(planted, i32)

    def first(self, n):
        return Case("%s-R%d" % (self.label, n), self.hn[:n], self.W, self.b, self.tgt[:n], self.N, self.planted[:n])

    def struct(self, outs, **override):
        s = CaseStruct(self.R, self.K, self.N, self.NPAD, _p(self.hn), _p(self.W), _p(self.b), _p(self.tgt), *[_p(o) for o in outs])
        for k, v in override.items():
            if not k.startswith("_"):  # (a "_keep" entry only keeps an overriding array alive)
                setattr(s, k, v)
        return s

    def validate(self, **override):
        dummy = np.zeros(8, np.uint8)
        return harness().tts_score_test_validate(C.byref(self.struct([dummy] * 6, **override)))

    def run(self):
        """(status, {name: Guarded})"""
        g = {k: Guarded(self.R, dt) for k, dt in OUTS}
        rc = harness().tts_score_test_run(C.byref(self.struct([g[k].raw for k, _ in OUTS])))
        return rc, g

    @functools.lru_cache(maxsize=None)
    def reference(self):
        return R.Ref(self.hn, self.W, self.b, self.tgt, self.N)


def _weights(shape, seed):
    """W [K][NPAD] ~ N(0, 0.02^2), b ~ N(0, 0.1^2), the pad columns of both PAD_VALUE"""
    N, NPAD, K = shape["N"], shape["NPAD"], shape["K"]
    g = np.random.default_rng(seed)
    W = (g.standard_normal((K, NPAD)) * 0.02).astype(f32)
    b = (g.standard_normal(NPAD) * 0.1).astype(f32)
    W[:, N:] = PAD_VALUE
    b[N:] = PAD_VALUE
    return W, b


def _random_case(label, shape, rows, seed, ties, targets):
    """Random rows; ties {row: (lo, hi)}: columns lo < hi hold bit-equal logits on that row, its maximum. Tie i owns channel i: every other row is zero there, the tie
    row is zero everywhere else (so both columns run the same chain on it: one product, 10 x 1, and one bias, 0), and W[i][lo] = W[i][hi] = 10. On every other
    row lo and hi stay two ordinary random columns."""
    N = shape["N"]
    g = np.random.default_rng(seed + 1)
    W, b = _weights(shape, seed)
    hn = g.standard_normal((rows, shape["K"])).astype(f32)  # LayerNorm output: unit scale
    tgt = g.integers(0, N, rows).astype(i32)
    planted = np.full(rows, -1, i32)
    hn[:, :len(ties)] = 0.0
    for ch, (row, (lo, hi)) in enumerate(ties.items()):
        hn[row] = 0.0
        hn[row, ch] = 1.0
        W[ch, lo] = W[ch, hi] = 10.0
        b[lo] = b[hi] = 0.0
        planted[row] = lo
    for row, t in targets.items():
        tgt[row] = t
    return Case(label, hn, W, b, tgt, N, planted)


@functools.lru_cache(maxsize=None)
def full_case():
    """130 rows of the full head. Planted exact ties (each must resolve to the lower index): neighbouring lanes (100, 101), neighbouring waves (31, 32), a
    wave's own two tiles (5, 133), the slab edge (255, 256), far slabs (700, 8000), the last full slab against the tail slab (8191, 8193 on row 128 of the ragged
    row tile) . Targets on column 0, the slab edge 255 / 256, 8191, and the tail slab's 8192 / 8193."""
    ties = {2: (100, 101), 3: (31, 32), 4: (5, 133), 66: (255, 256), 67: (700, 8000), 128: (8191, 8193)}
    targets = {0: 0, 1: 255, 5: 256, 6: 8191, 7: 8192, 8: 8193, 62: 8193, 63: 0, 64: 255, 65: 8192, 128: 8193, 129: 8191}
    return _random_case("full", FULL, 130, 9101, ties, targets)


@functools.lru_cache(maxsize=None)
def tail_tie_case():
    """the tail slab's own two columns tied (8192, 8193), on 2 rows of the full head (its columns cannot hold a second tie in full_case)"""
    return _random_case("tail-tie", FULL, 2, 9103, {1: (8192, 8193)}, {0: 8193, 1: 8192})


@functools.lru_cache(maxsize=None)
def small_case():
    """70 rows of the reduced shape: two row tiles, two slabs; ties across lanes, waves, a wave's two tiles, the slab edge, inside the tail tile and across the
    slabs; targets on 0, 255, 256, 288, 289"""
    ties = {2: (10, 11), 3: (63, 64), 4: (7, 135), 65: (255, 256), 66: (288, 289), 67: (3, 287)}
    return _random_case("small", SMALL, 70, 9102, ties, {0: 0, 1: 255, 5: 256, 6: 288, 7: 289, 64: 289, 69: 0})


def extreme_case(shape):
    """row 0: one logit at +80 (column 5), every other at -80: no overflow, lse = 80 + log(1 + (N - 1) e^-160) = 80; row 1: every logit equal (-80): lse = -80 + log N
    and argmax 0; row 2: the +80 on the stop column"""
    N, NPAD, K = shape["N"], shape["NPAD"], shape["K"]
    W = np.zeros((K, NPAD), f32)
    b = np.full(NPAD, -80.0, f32)
    W[:, N:] = PAD_VALUE
    b[N:] = PAD_VALUE
    hn = np.zeros((3, K), f32)
    hn[0, 0] = 1.0
    hn[2, 1] = 1.0
    W[0, 5] = 160.0
    W[1, N - 1] = 160.0
    c = Case("extreme-N%d" % N, hn, W, b, np.array([5, 0, N - 1], i32), N, planted=[5, 0, N - 1])
    return c


def invalid_overrides():
    """(name, field overrides of small_case().struct) the harness must refuse before any HIP call"""
    bad_t = small_case().tgt.copy()
    bad_t[3] = SMALL["N"]  # a pad column as a target: no lane would store it
    neg_t = small_case().tgt.copy()
    neg_t[0] = -1
    return [("R0", dict(R=0)), ("R-huge", dict(R=1 << 20)), ("K-not-32", dict(K=48)), ("K-576", dict(K=576)), ("K-huge", dict(K=8192)), ("K0", dict(K=0)), ("N0", dict(N=0)),
            ("N>NPAD", dict(N=321)), ("NPAD-not-64", dict(NPAD=304)), ("NPAD-far", dict(NPAD=640)), ("null-hn", dict(hn=None)), ("null-w", dict(w=None)), ("null-b", dict(b=None)),
            ("null-tgt", dict(tgt=None)), ("null-lse", dict(lse=None)), ("null-greedy", dict(greedy=None)), ("tgt-pad", dict(tgt=_p(bad_t), _keep=bad_t)),
            ("tgt-negative", dict(tgt=_p(neg_t), _keep=neg_t))]
