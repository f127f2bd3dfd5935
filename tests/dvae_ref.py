"""Shared by the DVAE tests (tests/test_dvae_cpu.py, tests/test_dvae_kernels_gpu.py, tests/test_dvae_gpu.py): two independent float64 restatements of the
encoder and quantiser of upstream tortoise-tts' DiscreteVAE.get_codebook_indices (one on torch.nn.functional, one in naive loops), a float32 twin in the kernels'
operation order with its seeded defects, the derived error bounds, the code rule, the synthetic models and inputs, and the ctypes view of the test-only harness
(tortoise.cpp_amd/testlib/dvae_harness.hip -> libtts_dvae_test.so). Upstream's source and weights are not available offline: the model is restated from memory,
unpinned against upstream.

  h = ReLU(Conv1d(80 -> C0, k 3, stride 2, pad 1)(mel));  h = ReLU(Conv1d(C0 -> H, k 3, stride 2, pad 1)(h))
  blocks x:  h = h + Conv1(ReLU(Conv3(ReLU(Conv3(h)))))          (pad 1; no activation on the block's input)
  z = Conv1d(H -> dim, k 1)(h);  code[t] = argmin_j |z[t] - E[:, j]|^2 = argmin_j (|E_j|^2 - 2 z[t] . E_j), the lowest index on a tie

BOUNDS, first order, nothing fitted; U = 2^-24, gamma_n = n U / (1 - n U). A chain of n fused multiply-adds from 0 rounds n times, each a partial sum of at most
sum |terms| (the f32-input MFMA is such a chain); the bias add and a residual add round once more each:
  convolution   gamma_{n + 2} (|b| + sum |w x| + |resid|), n = taps x input channels, evaluated in float64 on the float32 values the layer reads; ReLU is exact
  quantiser     s_j = fl(|E_j|^2 - 2 fl(z . E_j)): gamma_{dim + 2} (|E_j|^2 + 2 sum_k |z_k E_kj|)   (|E_j|^2 is the double sum rounded once)
THE CODE RULE. A row is DECIDED when the float64 gap between its best and its second-best code exceeds the sum of the two codes' bounds; there the code must be the
float64 argmin. On an undecided row it must be a code whose float64 distance is within (its bound + the best code's bound) of the minimum. At most 2 % of the rows
of a test may be undecided (MAX_UNDECIDED; rows with a PLANTED exact tie are undecided on purpose and are counted apart: there the lower index must win).
END TO END (through every layer) the kernel's z differs from float64's by dz; a code's distance moves by at most 2 |dz|_2 |E_j|_2, so the codes must agree on rows
whose float64 gap exceeds 2 (2 |dz|_2 max_j |E_j|_2 + the largest bound of the row); z itself is held to the project's 1e-3 gate for f32 stages."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import torch
import torch.nn.functional as F

import tortoise_cpp_amd_loader

tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

f32, f64, i32 = np.float32, np.float64, np.int32
U = 2.0 ** -24
GATE = 1e-3
MAX_UNDECIDED = 0.02
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_DVAE_TEST_LIB", os.path.join(PKG, "libtts_dvae_test.so"))
_DIR = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "dvae")
# mid: the ABI tests' model (hidden 64 / 128, 256 tokens); full: upstream's sizes
CONFIGS = {"mid": dict(channels=80, hidden=64, layers=2, blocks=3, dim=64, tokens=256, k=3, stride=2), "full": dict(sw.DVAE_UPSTREAM)}
SEEDS = {"mid": 1281, "full": 1282}
MID_FRAMES = (1, 2, 3, 4, 63, 64, 65, 130)  # both parities at both clip ends under stride 2 twice; around a stem tile x 4; two row tiles behind the stem
FULL_FRAMES = 173                            # about 2 s at 22 050 Hz / hop 256: 44 codes
RAGGED = (65, 3, 130, 1)


def gamma(n):
    return n * U / (1.0 - n * U)


@functools.lru_cache(maxsize=None)
def model(name):
    """(path of the model file, {name: float32 tensor}) of a configuration; written once per machine"""
    os.makedirs(_DIR, exist_ok=True)
    path = os.path.join(_DIR, "ggml-dvae-%s.bin" % name)
    if not os.path.exists(path + ".done"):
        sw.write_dvae(path + ".tmp", SEEDS[name], **CONFIGS[name])
        os.replace(path + ".tmp", path)
        open(path + ".done", "w").write("ok")
    return path, sw.read_ggml(path)


def mel(frames, seed=0, channels=80):
    """a test mel [channels][frames]: of the order of a normalised log-mel, smooth in time with noise on top"""
    r = np.random.default_rng(9000 + 31 * frames + seed)
    t = np.arange(frames)[None, :]
    b = np.arange(channels)[:, None]
    return (0.6 * np.sin(0.11 * t + 0.3 * b + seed) + 0.5 * r.standard_normal((channels, frames)) - 0.2).astype(f32)


def layout(t):
    """(strided layers, ResBlocks, stride) read from the names, as the loader reads them"""
    L = 0
    while "dvae.encoder.%d.0.weight" % L in t:
        L += 1
    nb = 0
    while "dvae.encoder.%d.net.0.weight" % (L + nb) in t:
        nb += 1
    return L, nb, int(t["dvae.config"][0]) if "dvae.config" in t else 2


def rows(frames, stride=2, layers=2):
    for _ in range(layers):
        frames = (frames - 1) // stride + 1
    return frames


# ---- float64, restatement 1: torch.nn.functional ----
def forward(t, m, dtype=torch.float64):
    """{"h": [the tensor behind every strided layer and every ResBlock, time-major], "z": [rows, dim], "s": [rows, tokens], "codes": [rows]}"""
    L, nb, stride = layout(t)
    w = lambda n: torch.from_numpy(np.ascontiguousarray(t[n])).to(dtype)  # noqa: E731
    h = torch.from_numpy(np.ascontiguousarray(m)).to(dtype)[None]
    hs = []
    for i in range(L):
        p = "dvae.encoder.%d.0." % i
        k = t[p + "weight"].shape[2]
        h = F.relu(F.conv1d(h, w(p + "weight"), w(p + "bias"), stride=stride, padding=(k - 1) // 2))
        hs.append(h[0].T.numpy().copy())
    for j in range(nb):
        p = "dvae.encoder.%d.net." % (L + j)
        y = h
        for q in (0, 2, 4):
            k = t[p + "%d.weight" % q].shape[2]
            y = F.conv1d(y if q == 0 else F.relu(y), w(p + "%d.weight" % q), w(p + "%d.bias" % q), padding=(k - 1) // 2)
        h = h + y
        hs.append(h[0].T.numpy().copy())
    p = "dvae.encoder.%d." % (L + nb)
    z = F.conv1d(h, w(p + "weight"), w(p + "bias"))[0].T
    E = w("dvae.codebook.embed")
    s = (E * E).sum(0)[None, :] - 2.0 * (z @ E)
    return {"h": hs, "z": z.numpy().copy(), "s": s.numpy().copy(), "codes": s.argmin(1).numpy().astype(i32)}


# ---- float64, restatement 2: naive loops, the distance itself (not the expanded form) ----
def _conv_loops(x, w, b, stride, relu_in):
    cout, cin, k = w.shape
    pad, T = (k - 1) // 2, x.shape[0]
    To = (T + 2 * pad - k) // stride + 1
    y = np.zeros((To, cout), f64)
    for to in range(To):
        for co in range(cout):
            acc = float(b[co])
            for j in range(k):
                ti = to * stride - pad + j
                if 0 <= ti < T:
                    row = np.maximum(x[ti], 0.0) if relu_in else x[ti]
                    acc += float(np.dot(w[co, :, j], row))
            y[to, co] = acc
    return y


def forward_loops(t, m):
    L, nb, stride = layout(t)
    g = lambda n: t[n].astype(f64)  # noqa: E731
    h = m.astype(f64).T
    for i in range(L):
        p = "dvae.encoder.%d.0." % i
        h = np.maximum(_conv_loops(h, g(p + "weight"), g(p + "bias"), stride, False), 0.0)
    for j in range(nb):
        p = "dvae.encoder.%d.net." % (L + j)
        y = _conv_loops(h, g(p + "0.weight"), g(p + "0.bias"), 1, False)
        y = _conv_loops(y, g(p + "2.weight"), g(p + "2.bias"), 1, True)
        h = h + _conv_loops(y, g(p + "4.weight"), g(p + "4.bias"), 1, True)
    p = "dvae.encoder.%d." % (L + nb)
    z = _conv_loops(h, g(p + "weight"), g(p + "bias"), 1, False)
    E = g("dvae.codebook.embed")
    d = np.zeros((z.shape[0], E.shape[1]), f64)
    for r in range(z.shape[0]):
        for j in range(E.shape[1]):
            d[r, j] = float(((z[r] - E[:, j]) ** 2).sum())
    return {"z": z, "d": d, "codes": d.argmin(1).astype(i32)}


# ---- one convolution: float64 with its bound, and the float32 twin in the kernels' order ----
def _gather(x, k, stride, pad):
    """[rows_out][k][cin]: the input rows under every tap, zero outside the clip"""
    T, cin = x.shape
    To = (T + 2 * pad - k) // stride + 1
    xp = np.zeros((T + 2 * pad + stride, cin), x.dtype)
    xp[pad:pad + T] = x
    idx = np.arange(To)[:, None] * stride + np.arange(k)[None, :]
    return xp[idx]


def conv64(x, w, b, stride=1, relu_in=False, relu_out=False, resid=None, pad=None):
    """(float64 output [rows_out][cout], its bound) of a layer on the float32 values x [rows][cin] (time-major), w [cout][cin][k], b"""
    cout, cin, k = w.shape
    x = x.astype(f64)
    if relu_in:
        x = np.maximum(x, 0.0)
    g = _gather(x, k, stride, (k - 1) // 2 if pad is None else pad).reshape(-1, k * cin)
    wm = w.astype(f64).transpose(2, 1, 0).reshape(k * cin, cout)
    y = g @ wm + b.astype(f64)[None, :]
    a = np.abs(g) @ np.abs(wm) + np.abs(b.astype(f64))[None, :]
    if resid is not None:
        y = y + resid.astype(f64)
        a = a + np.abs(resid.astype(f64))
    if relu_out:
        y = np.maximum(y, 0.0)
    return y, gamma(k * cin + 2) * a


def _chain(g, wm):
    """acc = fma(g[:, i], wm[i], acc) for i ascending, in float32 (a float64 multiply-add of float32 values rounded to float32: fmaf up to a rare double rounding)"""
    acc = np.zeros((g.shape[0], wm.shape[1]), f32)
    for i in range(g.shape[1]):
        acc = (acc.astype(f64) + g[:, i:i + 1].astype(f64) * wm[i:i + 1].astype(f64)).astype(f32)
    return acc


def conv32(x, w, b, stride=1, relu_in=False, relu_out=False, resid=None, stem=False, pad=None):
    """the float32 twin: the stem sums taps outer, bands ascending (dvae_stem_kernel); the others 32-channel chunks outer, then taps, then the chunk's channels
    ascending (cls_down_kernel, hfg_conv_kernel); the bias is added last, then the residual"""
    cout, cin, k = w.shape
    x = x.astype(f32)
    if relu_in:
        x = np.where(x < 0, f32(0), x)
    g = _gather(x, k, stride, (k - 1) // 2 if pad is None else pad)  # [To][k][cin]
    wt = w.astype(f32).transpose(2, 1, 0)                            # [k][cin][cout]
    if stem:
        order = [(j, c) for j in range(k) for c in range(cin)]
    else:
        order = [(j, c) for c0 in range(0, cin, 32) for j in range(k) for c in range(c0, min(c0 + 32, cin))]
    jj, cc = np.array([o[0] for o in order]), np.array([o[1] for o in order])
    y = _chain(g[:, jj, cc], wt[jj, cc]) + b.astype(f32)[None, :]
    if resid is not None:
        y = y + resid.astype(f32)
    if relu_out:
        y = np.maximum(y, f32(0))
    return y.astype(f32)


DEFECTS = ("pad", "relu_in", "no_skip", "drop_last", "tie_high", "no_e2", "slab_merge")


def twin(t, m, defect=None, slab=256):
    """The encoder and quantiser in float32, layer by layer in the kernels' order. Returns a list of (name, output of the twin, float64 output of the CORRECT
    layer on the twin's own input, bound) and the codes. A seeded defect changes the twin only: the correct layer's float64 and bound judge it."""
    L, nb, stride = layout(t)
    out = []
    x = np.ascontiguousarray(m.T)
    if defect == "drop_last":
        bad = x.copy()
        bad[-1] = 0
    for i in range(L):
        p = "dvae.encoder.%d.0." % i
        w, b = t[p + "weight"], t[p + "bias"]
        y = conv32(bad if (defect == "drop_last" and i == 0) else x, w, b, stride, relu_out=True, stem=i == 0, pad=0 if (defect == "pad" and i == 0) else None)
        want, bound = conv64(x, w, b, stride, relu_out=True)
        if y.shape != want.shape:  # a wrong padding may change the row count: judged as a miss on every element
            y = np.full(want.shape, np.inf, f32)
        out.append(("down%d" % i, y, want, bound))
        x = y if np.isfinite(y).all() else want.astype(f32)
    for j in range(nb):
        p = "dvae.encoder.%d.net." % (L + j)
        ws = [(t[p + "%d.weight" % q], t[p + "%d.bias" % q]) for q in (0, 2, 4)]
        a = conv32(x, *ws[0], relu_in=defect == "relu_in")
        out.append(("res%d.0" % j, a) + conv64(x, *ws[0]))
        c = conv32(a, *ws[1], relu_in=True)
        out.append(("res%d.2" % j, c) + conv64(a, *ws[1], relu_in=True))
        y = conv32(c, *ws[2], relu_in=True, resid=None if defect == "no_skip" else x)
        out.append(("res%d.4" % j, y) + conv64(c, *ws[2], relu_in=True, resid=x))
        x = y
    p = "dvae.encoder.%d." % (L + nb)
    z = conv32(x, t[p + "weight"], t[p + "bias"])
    out.append(("z", z) + conv64(x, t[p + "weight"], t[p + "bias"]))
    return out, vq32(z, t["dvae.codebook.embed"], defect, slab)


# ---- the quantiser ----
def code_norms(E):
    """|E_j|^2 as the loader makes it: double, channels ascending, rounded once"""
    acc = np.zeros(E.shape[1], f64)
    for k in range(E.shape[0]):
        acc += E[k].astype(f64) ** 2
    return acc.astype(f32)


def vq64(z, E):
    """(float64 distances s [rows][tokens] of the float32 values, bound [rows][tokens])"""
    z, E = z.astype(f64), E.astype(f64)
    e2 = (E * E).sum(0)
    s = e2[None, :] - 2.0 * (z @ E)
    return s, gamma(E.shape[0] + 2) * (e2[None, :] + 2.0 * (np.abs(z) @ np.abs(E)))


def vq32(z, E, defect=None, slab=256):
    """the kernel's arithmetic: s = fmaf(-2, chain(z . E_j), |E_j|^2); the minimum per slab, then over the slabs, the lowest index on a tie"""
    dot = _chain(z.astype(f32), E.astype(f32))
    e2 = np.zeros(E.shape[1], f32) if defect == "no_e2" else code_norms(E)
    s = (e2[None, :].astype(f64) - 2.0 * dot.astype(f64)).astype(f32)
    N = E.shape[1]
    best_v = np.full(z.shape[0], np.inf, f32)
    best_i = np.zeros(z.shape[0], i32)
    for c0 in range(0, N, slab):
        blk = s[:, c0:c0 + slab]
        if defect == "tie_high":
            li = blk.shape[1] - 1 - blk[:, ::-1].argmin(1)
        else:
            li = blk.argmin(1)
        v = blk[np.arange(len(li)), li]
        gi = li if defect == "slab_merge" else li + c0  # the defect: a slab's own index, its offset forgotten
        take = v < best_v
        best_v = np.where(take, v, best_v)
        best_i = np.where(take, gi, best_i).astype(i32)
    return best_i


def judge(codes, s, bound, planted=None):
    """The code rule on one batch of rows: returns (list of failures, undecided share among the rows without a planted tie)."""
    fails, und, counted = [], 0, 0
    for r in range(s.shape[0]):
        o = np.argsort(s[r], kind="stable")
        j0, j1 = int(o[0]), int(o[1])
        decided = s[r, j1] - s[r, j0] > bound[r, j0] + bound[r, j1]
        c = int(codes[r])
        if planted is not None and planted[r] >= 0:
            if c != planted[r]:
                fails.append("row %d: code %d, the planted tie's lower index is %d" % (r, c, planted[r]))
            continue
        counted += 1
        if decided:
            if c != j0:
                fails.append("row %d (decided, gap %.3e): code %d, float64 argmin %d" % (r, s[r, j1] - s[r, j0], c, j0))
        else:
            und += 1
            if not (0 <= c < s.shape[1]) or s[r, c] - s[r, j0] > bound[r, c] + bound[r, j0]:
                fails.append("row %d (undecided): code %d is not within the bound of the minimum (code %d)" % (r, c, j0))
    return fails, und / max(counted, 1)


def judge_end_to_end(codes, z, z64, s64, bound64, E):
    """through every layer: (failures, share of rows the margin leaves out). z: the kernel's, z64 / s64 / bound64: float64's own."""
    emax = float(np.sqrt((E.astype(f64) ** 2).sum(0)).max())
    fails, out = [], 0
    for r in range(s64.shape[0]):
        o = np.argsort(s64[r], kind="stable")
        j0, j1 = int(o[0]), int(o[1])
        dz = float(np.sqrt(((z[r].astype(f64) - z64[r]) ** 2).sum()))
        if s64[r, j1] - s64[r, j0] > 2.0 * (2.0 * dz * emax + bound64[r].max()):
            if int(codes[r]) != j0:
                fails.append("row %d: code %d, float64 argmin %d (gap %.3e)" % (r, int(codes[r]), j0, s64[r, j1] - s64[r, j0]))
        else:
            out += 1
    return fails, out / s64.shape[0]


@functools.lru_cache(maxsize=None)
def reference(name, frames, seed=0):
    """float64 of mel(frames, seed) on model(name): computed once, shared, never written to"""
    r = forward(model(name)[1], mel(frames, seed))
    r["bound"] = vq64(r["z"], model(name)[1]["dvae.codebook.embed"])[1]  # float64's own z: the bound at the reference
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---- the kernel harness ----
STEM, DOWN, VQ = 0, 1, 2
HIP_INVALID_VALUE = 1
SENTINEL = 0xCB
STEM_TILE, DOWN_TILE, VQ_TILE, VQ_SLAB = 16, 64, 64, 256


class CaseStruct(C.Structure):
    _fields_ = [("kind", C.c_int), ("ns", C.c_int), ("rows", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("taps", C.c_int), ("stride", C.c_int),
                ("rows_out", C.c_int), ("n", C.c_void_p), ("in_", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("out2", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_dvae_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_dvae_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_dvae_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_dvae_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_dvae_test_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
        L.tts_dvae_test_packed.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong]
        L.tts_dvae_test_packed.restype = C.c_longlong
        L.tts_dvae_test_code_norms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        for f in (L.tts_dvae_test_run, L.tts_dvae_test_validate, L.tts_dvae_test_parse, L.tts_dvae_test_margin, L.tts_dvae_test_stem_tile, L.tts_dvae_test_down_tile,
                  L.tts_dvae_test_vq_tile, L.tts_dvae_test_vq_slab, L.tts_dvae_test_code_norms):
            f.restype = C.c_int
        _lib = L
    return _lib


def parse(path):
    """the loader's host half on a file: (status, [strided layers, ResBlocks, mel channels, hidden, dim, tokens, stride], message)"""
    out, err = np.zeros(7, i32), C.create_string_buffer(512)
    rc = harness().tts_dvae_test_parse(path.encode(), out.ctypes.data_as(C.c_void_p), err, 512)
    return rc, out, err.value.decode()


def packed(path, which, i=0):
    L = harness()
    cnt = L.tts_dvae_test_packed(path.encode(), which, i, None, 0)
    assert cnt > 0, cnt
    out = np.zeros(cnt, f32)
    assert L.tts_dvae_test_packed(path.encode(), which, i, out.ctypes.data_as(C.c_void_p), cnt) == cnt
    return out


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape, dtype=f32):
        self.margin = harness().tts_dvae_test_margin()
        self.shape, self.dtype = shape, dtype
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * np.dtype(dtype).itemsize, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


class Case(object):
    """One harness case. STEM: x = list of mels [cin][n]; DOWN: x = list of [n][cin]; VQ: x = z [rows][dim], w = E [dim][tokens]."""

    def __init__(self, kind, x, w, b=None, stride=2, label=""):
        self.kind, self.stride, self.label = kind, stride, label
        if kind == VQ:
            self.x = [np.ascontiguousarray(x, f32)]
            self.n = np.array([self.x[0].shape[0]], i32)
            self.w = np.ascontiguousarray(w, f32)  # [dim][tokens]
            self.b = None
            self.cin, self.cout, self.taps = self.w.shape[0], self.w.shape[1], 1
            self.rows = self.rows_out = int(self.n[0])
            self.inbuf = self.x[0]
        else:
            self.x = [np.ascontiguousarray(a, f32) for a in x]
            self.wt = np.ascontiguousarray(w, f32)  # PyTorch's [cout][cin][k]
            self.w = np.ascontiguousarray(self.wt.transpose(2, 1, 0))  # [k][cin][cout]
            self.b = np.ascontiguousarray(b, f32)
            self.cout, self.cin, self.taps = self.wt.shape
            self.n = np.array([a.shape[1] if kind == STEM else a.shape[0] for a in self.x], i32)
            self.rows = int(self.n.sum())
            self.n_out = np.array([(int(v) - 1) // stride + 1 for v in self.n], i32)
            self.rows_out = int(self.n_out.sum())
            self.inbuf = np.ascontiguousarray(np.concatenate([a.reshape(-1) for a in self.x]))

    def name(self):
        return "%s-%s" % ({STEM: "stem", DOWN: "down", VQ: "vq"}[self.kind], self.label)

    def struct(self, out=None, out2=None, **override):
        s = CaseStruct(self.kind, len(self.n), self.rows, self.cin, self.cout, self.taps, self.stride, self.rows_out, _p(self.n), _p(self.inbuf), _p(self.w),
                       _p(self.b), _p(out), _p(out2))
        for k, v in override.items():
            setattr(s, k, v)
        return s

    def validate(self, **override):
        dummy = np.zeros(8, np.uint8)
        s = self.struct(dummy, dummy)
        for k, v in override.items():
            setattr(s, k, v)
        return harness().tts_dvae_test_validate(C.byref(s))

    def run(self):
        """(status, Guarded out, Guarded out2 or None)"""
        if self.kind == VQ:
            g, g2 = Guarded((self.rows,), i32), Guarded((self.rows,), f32)
        else:
            g, g2 = Guarded((self.rows_out, self.cout), f32), None
        rc = harness().tts_dvae_test_run(C.byref(self.struct(g.raw, None if g2 is None else g2.raw)))
        return rc, g, g2

    def clips_out(self, y):
        o, res = 0, []
        for v in self.n_out:
            res.append(y[o:o + v])
            o += v
        return res

    def reference(self):
        """per clip: (float64 output, bound)"""
        return [conv64(a.T if self.kind == STEM else a, self.wt, self.b, self.stride, relu_out=True) for a in self.x]


def _rw(shape, seed, std):
    return (np.random.default_rng(seed).standard_normal(shape) * std).astype(f32)


@functools.lru_cache(maxsize=None)
def stem_cases():
    w, b = _rw((64, 80, 3), 11, np.sqrt(2.0 / 240)), _rw((64,), 12, 0.05)
    cs = [Case(STEM, [mel(n, 1)], w, b, label="T%d" % n) for n in (1, 2, 3, 4, 63, 64, 65)]
    cs.append(Case(STEM, [mel(35, 2), mel(4, 3)], w, b, label="ragged35+4"))
    w5, b5 = _rw((320, 7, 5), 13, 0.2), _rw((320,), 14, 0.05)  # other sizes: 7 bands, 5 taps, stride 3, two channel blocks of 256
    cs.append(Case(STEM, [mel(50, 4, 7)], w5, b5, stride=3, label="c7k5s3T50"))
    return cs


@functools.lru_cache(maxsize=None)
def down_cases():
    w, b = _rw((64, 64, 3), 21, np.sqrt(2.0 / 192)), _rw((64,), 22, 0.05)
    x = lambda n, s: np.abs(_rw((n, 64), 23 + s, 1.0)) * (np.random.default_rng(99 + s).random((n, 64)) < 0.6)  # noqa: E731  (behind a ReLU: half zeros)
    cs = [Case(DOWN, [x(n, n)], w, b, label="T%d" % n) for n in (1, 2, 3, 127, 128, 129)]
    cs.append(Case(DOWN, [x(130, 1), x(3, 2)], w, b, label="ragged130+3"))
    return cs


def _planted(z, E, row, col, dup=None):
    """make code `col` the clear winner of `row`: its column becomes the row itself (distance 0); dup: the same column again (an exact tie)"""
    E[:, col] = z[row]
    if dup is not None:
        E[:, dup] = z[row]


def _tie_rows(z, E, pairs):
    """int32 [rows]: -1, or for a row whose float64 minimum lies on a duplicated column (an exact tie in every arithmetic) the pair's lower index"""
    pl = np.full(z.shape[0], -1, i32)
    best = vq64(z, E)[0].argmin(1)
    for lo, hi in pairs:
        assert lo < hi and np.array_equal(E[:, lo], E[:, hi])
        pl[(best == lo) | (best == hi)] = lo
    return pl


@functools.lru_cache(maxsize=None)
def vq_cases():
    """(Case, planted: int32 [rows], -1 or the code that must win by the planted tie)"""
    cs = []
    T, S = VQ_TILE, VQ_SLAB
    for tokens in (128, 192, S + 64):
        for rows_ in (1, T - 1, T, T + 1, 2 * T + 1):
            z, E = _rw((rows_, 64), 3100 + rows_ + tokens, 1.0), _rw((64, tokens), 3200 + tokens, 1.0)
            # the winner in the first column, the last column, the last column of the first slab; an exact tie inside a 32-code tile and (two slabs) across slabs
            _planted(z, E, 0, 0)
            if rows_ > 1:
                _planted(z, E, rows_ - 1, tokens - 1)
            if rows_ > 2 and tokens > S:
                _planted(z, E, rows_ // 2, S - 1)
            pairs = []
            if rows_ >= 8:
                _planted(z, E, 3, 37, 45)  # the same tile, the same wave
                _planted(z, E, 5, 70, 101)  # two tiles: two waves of a workgroup
                pairs += [(37, 45), (70, 101)]
                if tokens > S:
                    _planted(z, E, 6, 130, S + 9)  # two slabs: two workgroups and the reduce
                    pairs.append((130, S + 9))
            pl = _tie_rows(z, E, pairs)  # rows 3, 5, 6 and whichever other row has a duplicated column nearest
            cs.append((Case(VQ, z, E, label="N%d-R%d" % (tokens, rows_)), pl))
    return cs


@functools.lru_cache(maxsize=None)
def vq_full_case():
    """dim 512 x 8192 tokens x (tile + 1) rows; one exact tie across far slabs"""
    rows_ = VQ_TILE + 1
    z, E = _rw((rows_, 512), 41, 1.0), _rw((512, 8192), 42, 1.0)
    _planted(z, E, 7, 300, 8000)
    _planted(z, E, 64, 8191)
    return Case(VQ, z, E, label="full"), _tie_rows(z, E, [(300, 8000)])
