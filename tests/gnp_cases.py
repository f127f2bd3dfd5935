"""Shared by tests/test_gemm_gn_panel_gpu.py and tests/test_gemm_gn_panel_cpu.py: the ctypes view of the test-only harness library around
gemm_f16_gn_panel_kernel (tortoise.cpp_amd/testlib/gemm_gn_panel_harness.hip -> libtts_gnp_test.so), the engine's packing rule and the case builder."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_GNP_TEST_LIB") or os.path.join(PKG, "libtts_gnp_test.so")
CH = 1024
SENTINEL = 0xCB
PANEL_ROWS = 896


class CaseStruct(C.Structure):
    _fields_ = [("ns", C.c_int), ("rows", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("do_silu", C.c_int), ("lut", C.c_int), ("n_steps", C.c_int), ("ss_step_stride", C.c_int),
                ("eps", C.c_float),
                ("start", C.c_void_p), ("len", C.c_void_p), ("seq_step", C.c_void_p),
                ("A", C.c_void_p), ("W", C.c_void_p),
                ("bias", C.c_void_p), ("g", C.c_void_p), ("b", C.c_void_p), ("ss", C.c_void_p),
                ("out_pair", C.c_void_p), ("out_fused", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_gnp_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_gnp_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_gnp_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_gnp_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_gnp_test_takes.argtypes = [C.c_int] * 8
        L.tts_gnp_test_grid.argtypes = [C.c_int] * 2
        for f in (L.tts_gnp_test_run, L.tts_gnp_test_validate, L.tts_gnp_test_margin, L.tts_gnp_test_takes, L.tts_gnp_test_grid, L.tts_gnp_test_lds):
            f.restype = C.c_int
        _lib = L
    return _lib


def pack(lens):
    """Layout::build: sequences start on multiples of 8 from row 8, one guard row behind each, rows padded to 128."""
    r, start = 8, []
    for L in lens:
        start.append(r)
        r = (r + L + 1 + 7) & ~7
    return np.array(start, np.int32), (r + 127) & ~127


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Case:
    """Operands of one case (NumPy arrays kept alive here) and its C view."""

    def __init__(self, lens, N, K, seed=0, outlier=False, bias=True, ss="none", do_silu=1, lut=0):
        rs = np.random.RandomState(seed)
        self.lens, self.N, self.K = list(lens), N, K
        self.start, self.rows = pack(lens)
        self.len = np.array(lens, np.int32)
        nw = (N + 127) // 128 * 128
        a = rs.randn(self.rows, K).astype(np.float32)  # guard and padding rows carry values too: nothing may read them into a statistic
        if outlier:  # one row of one sequence 50 times larger: the two-pass variance and the fp16 rounding of its neighbours must not care who computes them
            s = len(lens) - 1
            a[self.start[s] + lens[s] // 2] *= 50.0
        self.A = a.astype(np.float16)
        self.W = (rs.randn(nw, K) / np.sqrt(K)).astype(np.float16)
        self.bias = (0.5 * rs.randn(nw)).astype(np.float32) if bias else None
        self.g = (1.0 + 0.2 * rs.randn(CH)).astype(np.float32)
        self.b = (0.2 * rs.randn(CH)).astype(np.float32)
        self.ss, self.seq_step, self.n_steps, self.stride = None, None, 0, 0
        if ss == "one":
            self.n_steps, self.stride = 1, 0
            self.ss = (0.3 * rs.randn(2 * CH)).astype(np.float32)
        elif ss == "table":  # a timestep per sequence, rows of the table 2 048 + 64 floats apart
            self.n_steps, self.stride = 3, 2 * CH + 64
            self.ss = (0.3 * rs.randn((self.n_steps - 1) * self.stride + 2 * CH)).astype(np.float32)
            self.seq_step = np.array([(2 * s + 1) % self.n_steps for s in range(len(lens))], np.int32)
        self.do_silu, self.lut = do_silu, lut

    def struct(self, out_pair, out_fused):
        c = CaseStruct()
        c.ns, c.rows, c.N, c.K = len(self.lens), self.rows, self.N, self.K
        c.do_silu, c.lut, c.n_steps, c.ss_step_stride, c.eps = self.do_silu, self.lut, self.n_steps, self.stride, 1e-5
        c.start, c.len, c.seq_step = _ptr(self.start), _ptr(self.len), _ptr(self.seq_step)
        c.A, c.W, c.bias, c.g, c.b, c.ss = _ptr(self.A), _ptr(self.W), _ptr(self.bias), _ptr(self.g), _ptr(self.b), _ptr(self.ss)
        c.out_pair, c.out_fused = _ptr(out_pair), _ptr(out_fused)
        return c


def run(case):
    """(rc, pair, fused, margins): the two fp16 outputs as uint16 [rows][1024] and the four margin slices as bytes."""
    L = harness()
    m = L.tts_gnp_test_margin()
    n = case.rows * CH * 2
    bufs = [np.zeros(n + 2 * m, np.uint8) for _ in range(2)]
    rc = L.tts_gnp_test_run(C.byref(case.struct(bufs[0], bufs[1])))
    outs = [b[m:m + n].view(np.uint16).reshape(case.rows, CH) for b in bufs]
    margins = [b[:m] for b in bufs] + [b[m + n:] for b in bufs]
    return rc, outs[0], outs[1], margins
