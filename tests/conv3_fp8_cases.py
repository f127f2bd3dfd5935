"""Shared by the conv3_fp8 tests: the harness library around csrc/gemm_f8.h, the packed row layout, the float64 convolution and the kernel's bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tortoise.cpp_amd")
LIB = os.path.join(PKG, "libtts_gemm_f8_test.so")
U, SENTINEL = 2.0 ** -24, 0xCB
_u8p, _f32p, _i32p = (np.ctypeslib.ndpointer(t, flags="C_CONTIGUOUS") for t in (np.uint8, np.float32, np.int32))


class ConvCase(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("M", "rows_total", "N", "K", "resid_aliases_out")] + \
               [(n, C.c_void_p) for n in ("A8", "Wimg", "inv_a", "inv_w", "bias", "resid", "row_seq", "out")]


_lib, _maps = None, {}


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_gemm_f8_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        L = C.CDLL(LIB)
        L.tts_f8_test_wfrag_index.restype, L.tts_f8_test_wfrag_index.argtypes = C.c_longlong, [C.c_int] * 5
        L.tts_f8_test_pack.argtypes = [_f32p, C.c_int, C.c_int, _u8p, _f32p]
        L.tts_f8_test_quant.argtypes = [np.ctypeslib.ndpointer(np.float16, flags="C_CONTIGUOUS"), C.c_int, C.c_int, C.c_int, _i32p, _i32p, _u8p, _f32p]
        L.tts_f8_test_conv3.argtypes = [C.POINTER(ConvCase)]
        L.tts_f8_test_takes.argtypes = [C.c_int] * 7
        _lib = L
    return _lib


def layout(lens):
    """diffusion.hip's Layout: starts at multiples of 8 from row 8, a guard row behind every sequence; M = the rows padded to 128, rows_total = the last guard row + 1"""
    start, r = [], 8
    for n in lens:
        start.append(r)
        r = (r + n + 1 + 7) & ~7
    row_seq = np.full((r + 127) & ~127, -1, np.int32)
    for s, (a, n) in enumerate(zip(start, lens)):
        row_seq[a:a + n] = s
    return np.array(start, np.int32), np.array(lens, np.int32), len(row_seq), start[-1] + lens[-1] + 1, row_seq


def decode(b):
    return torch.from_numpy(np.ascontiguousarray(b)).view(torch.float8_e4m3fn).to(torch.float64).numpy()


def encode(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def index_map(N, K):
    """gemm_f8_wfrag_index for every (n, tap, k), from the harness: the one statement of the order"""
    if (N, K) not in _maps:
        f = harness().tts_f8_test_wfrag_index
        _maps[N, K] = np.array([f(n, t, k, N, K) for n in range(N) for t in range(3) for k in range(K)], np.int64).reshape(N, 3, K)
    return _maps[N, K]


def conv_acc(A, W):
    """A [M + 2][K] (rows -1 .. M), W [N][3][K], float64 -> sum over taps and channels [M][N]"""
    return sum(A[t:t + A.shape[0] - 2] @ W[:, t, :].T for t in range(3))


def conv_ref(A, W, inv_a, inv_w, bias, resid, row_seq):
    out = conv_acc(A, W) * np.outer(inv_a.astype(np.float64), inv_w.astype(np.float64)) + bias.astype(np.float64)[None, :]
    out = out if resid is None else out + resid
    if row_seq is not None:
        out[row_seq < 0] = 0
    return out


def conv_bound(A, W, inv_a, inv_w, bias, resid):
    """(2 * 3K + 4) u * sum |a||w| * inv_a * inv_w + 2u (|bias| + |resid|): 3K products and 3K additions of the accumulator in any order, the scaling (exact) and
    the two roundings of the epilogue, counted as the fp16 kernels' tests count theirs"""
    b = (6 * A.shape[1] + 4) * U * conv_acc(np.abs(A), np.abs(W)) * np.outer(inv_a.astype(np.float64), inv_w.astype(np.float64))
    return b + 2 * U * (np.abs(bias.astype(np.float64))[None, :] + (0 if resid is None else np.abs(resid)))


def run_conv(A8, W8, inv_a, inv_w, bias, resid, row_seq, rows_total, alias=False):
    """one launch; returns the [M][N] output after checking the canary margins and that rows >= rows_total still hold the sentinel"""
    L = harness()
    M, K, N = A8.shape[0] - 2, A8.shape[1], W8.shape[0]
    margin = L.tts_f8_test_margin()
    img = np.zeros(3 * N * K, np.uint8)
    img[index_map(N, K)] = W8
    out = np.zeros(2 * margin + M * N * 4, np.uint8)
    arrs = [np.ascontiguousarray(A8), img] + [None if x is None else np.ascontiguousarray(x, t) for x, t in
                                              ((inv_a, np.float32), (inv_w, np.float32), (bias, np.float32), (resid, np.float32), (row_seq, np.int32))] + [out]
    c = ConvCase(M, rows_total, N, K, int(alias), *[None if a is None else a.ctypes.data for a in arrs])
    assert L.tts_f8_test_conv3(C.byref(c)) == 0
    assert (out[:margin] == SENTINEL).all() and (out[-margin:] == SENTINEL).all(), "canary margin written"
    body = out[margin:-margin].reshape(M, N * 4)
    assert alias or (body[rows_total:] == SENTINEL).all(), "a row past rows_total was written"
    return body.view(np.float32)
