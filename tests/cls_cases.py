"""Shared by tests/test_cls_kernels_gpu.py and tests/test_cls_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/cls_harness.hip -> libtts_cls_test.so), float64 NumPy references of the classifier's kernels (csrc/classifier.h), the case matrix, the
acceptance rule and its error bounds, float32 restatements in another summation order, and the defects the rule must reject.

LAYOUT, as classifier_run builds it: clip s owns the rows [start_s, start_s + n_s) of a buffer, start = the running sum of ceil8(n) (the cases add gaps). The
input rows that belong to no clip hold 3.5 (NaN in the poisoned twin); the output starts as the sentinel byte everywhere and keeps it outside the clips.

REFERENCES are float64 on the float32 values the kernel reads, so that a bound covers arithmetic only.

ACCEPTANCE, first order and term by term, nothing fitted; U = 2^-24, D = 2^-53. A chain of n fused multiply-adds rounds n times, each time a partial sum of at
most A = sum |terms|: n U A (the f32-input MFMA is such a chain, k ascending: one rounding per product, no wider accumulator).
  stem      3 U (|b| + sum_k |w_k x_k|)
  GroupNorm the statistics are double sums of exact products over N = rows x channels-per-group values:
              e_mean = (N + 2) D mean|x|,  e_var = (N + 2) D mean(x^2) + 2 |mean| e_mean + D mean^2,  r = 1 / sqrt(var + eps): e_r / r = e_var / (2 (var + eps)) + 2 D + U
            d = fl(x - mean): e_d = e_mean + U |d|;  p = fl(d r): e_p = r e_d + |d r| (e_r / r + U);  v = fma(p, gamma, beta): e_v = |gamma| e_p + U |v|
            y = v / (1 + expf(-v)): e_y = 1.1 e_v + |y| (EXP_REL E / (1 + E) + U + DIV), E = exp(-v)       (|SiLU'| <= 1.1; without SiLU e_y = e_v)
  down      (taps cin + 1) U (|b| + sum |x w|)
  attention s_j = sum_d fl(q c) fl(k c): e_s = (DH + 4) U sum |q k| c^2 (two operand roundings, c's own two, DH chain steps);
            w = softmax(s): e_w_j = w_j (e_s_j + sum_i w_i e_s_i);  the running-maximum form rounds the exponent's argument (U (max s - min s)), evaluates expf
            twice per key and rounds the product and the fused multiply-add of every step: rel = n (2 EXP_REL + 3 U) + U (max s - min s) + DIV
            e_out_d = sum_j e_w_j |v_jd| + rel sum_j w_j |v_jd|
  head      (E / 64 + 7) U (|b| + sum |w x|) per logit (64 strided chains, a 6-level tree, the bias);  p = e0 / (e0 + e1): e_p = p0 p1 (e_l0 + e_l1) + (2 EXP_REL + 3 U) p0
EXP_REL = 2 ulp = 4 U: device expf (the HIP math API reference's table of maximum ulp errors lists 1; charged double, as ar_attn_cases.py charges it). DIV = 2 U
(gn_cases.py: "an IEEE division or square root 2u").

DEFECTS are applied to the reference (reference(case, mut=...)); test_cls_harness_cpu.py requires each to leave the bound of the unmutated reference on some case."""
import ctypes as C
import os
import subprocess

import numpy as np

f32, f64, i32 = np.float32, np.float64, np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
SRC = os.path.join(PKG, "testlib", "cls_harness.hip")
LIB = os.environ.get("TTS_CLS_TEST_LIB", os.path.join(PKG, "libtts_cls_test.so"))
STEM, GN, DOWN, ATTN, HEAD = 0, 1, 2, 3, 4
KIND_NAMES = {STEM: "stem", GN: "gn_silu", DOWN: "down", ATTN: "attn", HEAD: "head"}
HIP_INVALID_VALUE = 1
SENTINEL = 0xCB
SEQ = 9
U, D = 2.0 ** -24, 2.0 ** -53
FMIN = 2.0 ** -126
EXP_REL, DIV = 4 * U, 2 * U
JUNK = f32(3.5)
GN_TILE, DOWN_TILE, STEM_TILE = 256, 64, 64  # checked against the library: tts_cls_test_gn_tile / _down_tile / _stem_tile
EPS = 1e-5


class CaseStruct(C.Structure):
    _fields_ = [("kind", C.c_int), ("ns", C.c_int), ("rows", C.c_int), ("C", C.c_int), ("C2", C.c_int), ("taps", C.c_int), ("stride", C.c_int), ("heads", C.c_int),
                ("rows_out", C.c_int), ("n", C.c_void_p), ("start", C.c_void_p), ("start_out", C.c_void_p), ("in_", C.c_void_p), ("w", C.c_void_p),
                ("bias", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("out", C.c_void_p), ("stat", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_cls_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_cls_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_cls_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_cls_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_cls_test_table.argtypes = [C.POINTER(CaseStruct), C.c_void_p, C.c_void_p]
        L.tts_cls_test_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
        L.tts_cls_test_packed.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong]
        L.tts_cls_test_packed.restype = C.c_longlong
        L.tts_cls_test_groups.argtypes = [C.c_int]
        for f in (L.tts_cls_test_run, L.tts_cls_test_validate, L.tts_cls_test_table, L.tts_cls_test_parse, L.tts_cls_test_margin, L.tts_cls_test_gn_tile,
                  L.tts_cls_test_down_tile, L.tts_cls_test_stem_tile, L.tts_cls_test_groups):
            f.restype = C.c_int
        _lib = L
    return _lib


def parse(path):
    """the loader's host half on a file: (status, [b0, depth, K, E, ResBlocks per level, attention blocks, F, H], message)"""
    out, err = np.zeros(8, i32), C.create_string_buffer(512)
    rc = harness().tts_cls_test_parse(path.encode(), out.ctypes.data_as(C.c_void_p), err, 512)
    return rc, out, err.value.decode()


def packed(path, which, i=0):
    L = harness()
    cnt = L.tts_cls_test_packed(path.encode(), which, i, None, 0)
    assert cnt > 0, cnt
    out = np.zeros(cnt, f32)
    assert L.tts_cls_test_packed(path.encode(), which, i, out.ctypes.data_as(C.c_void_p), cnt) == cnt
    return out


def groups(C_):
    g = 8 if C_ <= 16 else 16 if C_ <= 64 else 32
    while C_ % g:
        g //= 2
    return g


def ceil8(v):
    return (v + 7) // 8 * 8


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape):
        self.margin = harness().tts_cls_test_margin()
        self.shape = shape
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * 4, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(f32).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


def _layout(n, start, gap):
    out, run = [], gap
    for s, v in enumerate(n):
        st = run if start is None else start[s]
        out.append(st)
        run = st + ceil8(v) + gap
    return out, run


class Case(object):
    """gap: rows of no clip in front of, between and behind the clips (a multiple of 8; 0 = classifier_run's own packing, no explicit start table)"""

    def __init__(self, kind, n, C_=32, C2=0, taps=5, stride=4, heads=2, gap=8, fam="gauss", seed=0):
        self.kind, self.n, self.C, self.C2, self.taps, self.stride, self.heads, self.gap, self.fam, self.seed = kind, list(n), C_, C2, taps, stride, heads, gap, fam, seed
        self.start, self.rows = _layout(self.n, None, gap)
        self.n_out = [(v - 1) // stride + 1 for v in self.n]
        self.start_out, self.rows_out = _layout(self.n_out, None, gap)
        self.a = {}

    @property
    def ns(self):
        return len(self.n)

    def clip(self, s, out=False):
        st, n = (self.start_out[s], self.n_out[s]) if out else (self.start[s], self.n[s])
        return slice(st, st + n)

    def live(self, out=False):
        m = np.zeros(self.rows_out if out else self.rows, bool)
        for s in range(self.ns):
            m[self.clip(s, out)] = True
        return m

    def out_shape(self):
        return {STEM: (self.rows, self.C), GN: (self.rows, self.C), DOWN: (self.rows_out, self.C2), ATTN: (self.rows, self.C), HEAD: (self.ns, 3)}[self.kind]

    def table(self, out=False):
        t, tiles = np.zeros((self.ns, SEQ), i32), 0
        for s in range(self.ns):
            st, n = (self.start_out[s], self.n_out[s]) if out else (self.start[s], self.n[s])
            t[s, 0], t[s, 1], t[s, 3], t[s, 4] = st, n, tiles, st
            tiles += (n + GN_TILE - 1) // GN_TILE
        return t

    def name(self):
        return "%s n%s C%d%s %s" % (KIND_NAMES[self.kind], "-".join(map(str, self.n)), self.C, "->%d" % self.C2 if self.kind == DOWN else " h%d" % self.heads if self.kind == ATTN else "", self.fam)


def make(kind, n, C_=32, C2=0, taps=5, stride=4, heads=2, gap=8, fam="gauss", seed=0):
    """fam: gauss = unit-scale rows; offset (GN) = every group's mean is 100 x its deviation; peaked (ATTN) = scores spread over +-20"""
    c = Case(kind, n, C_, C2, taps, stride, heads, gap, fam, seed)
    rs = np.random.RandomState(1000 * kind + 31 * seed + sum(c.n) + 7 * c.C + c.C2 + heads)
    if kind == STEM:
        x = (rs.randn(c.rows) * 0.6).astype(f32)  # some of it outside [-1, 1]: the clamp
        x[~c.live()] = JUNK
        c.a.update(in_=x, w=(rs.randn(c.C, 3) * 0.6).astype(f32), bias=(rs.randn(c.C) * 0.1).astype(f32))
        return c
    width = 3 * c.C if kind == ATTN else c.C
    x = (rs.randn(c.rows, width) * (2.5 if fam == "peaked" else 1.0)).astype(f32)
    if fam == "offset":
        x = (x * f32(0.37) + f32(37.0)).astype(f32)
    x[~c.live()] = JUNK
    c.a["in_"] = x
    if kind == GN:
        c.a.update(gamma=(1 + 0.3 * rs.randn(c.C)).astype(f32), beta=(0.3 * rs.randn(c.C)).astype(f32))
    elif kind == DOWN:
        c.a.update(w=(rs.randn(taps, c.C, c.C2) / np.sqrt(taps * c.C)).astype(f32), bias=(rs.randn(c.C2) * 0.1).astype(f32))
    elif kind == HEAD:
        c.a.update(w=(rs.randn(2, c.C) / np.sqrt(c.C) * 3).astype(f32), bias=(rs.randn(2) * 0.3).astype(f32))
    return c


def struct(c, out_buf, stat_buf=None, **override):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    keep = dict(n=np.array(c.n, i32), start=np.array(c.start, i32) if c.gap else None, start_out=np.array(c.start_out, i32) if c.gap else None)
    f = dict(kind=c.kind, ns=c.ns, rows=c.rows, C=c.C, C2=c.C2, taps=c.taps, stride=c.stride, heads=c.heads, rows_out=c.rows_out, n=p(keep["n"]),
             start=p(keep["start"]), start_out=p(keep["start_out"]), in_=p(c.a.get("in_")), w=p(c.a.get("w")), bias=p(c.a.get("bias")), gamma=p(c.a.get("gamma")),
             beta=p(c.a.get("beta")), out=p(out_buf), stat=p(stat_buf))
    f.update(override)
    return CaseStruct(**f), keep


def validate(c, **override):
    g = Guarded(c.out_shape())
    s, keep = struct(c, g.raw, **override)
    return harness().tts_cls_test_validate(C.byref(s))


def run(c, want_stat=False):
    """one launch on the device: (Guarded output, stat [ns][G][2] or None)"""
    g = Guarded(c.out_shape())
    g.raw[:] = 0x11  # the harness overwrites all of it
    stat = np.zeros((c.ns, groups(c.C), 2), f64) if want_stat and c.kind == GN else None
    s, keep = struct(c, g.raw, stat)
    rc = harness().tts_cls_test_run(C.byref(s))
    assert rc == 0, "harness status %d on %s" % (rc, c.name())
    return g, stat


def alone(c, s):
    """clip s of a case as a case of its own (same operands, packed as classifier_run packs a single clip)"""
    a = Case(c.kind, [c.n[s]], c.C, c.C2, c.taps, c.stride, c.heads, 0, c.fam, c.seed)
    a.a = dict(c.a)
    x = c.a["in_"]
    blank = np.full((a.rows,) + x.shape[1:], JUNK, f32)
    blank[a.clip(0)] = x[c.clip(s)]
    a.a["in_"] = blank
    return a


def poisoned(c):
    a = Case(c.kind, c.n, c.C, c.C2, c.taps, c.stride, c.heads, c.gap, c.fam, c.seed)
    a.a = dict(c.a)
    x = c.a["in_"].copy()
    x[~c.live()] = np.nan
    a.a["in_"] = x
    return a


def judge(got, ref, bound):
    """(ok, worst |got - ref| / bound); a non-finite value or a shape mismatch is a failure"""
    if got.shape != ref.shape or not np.isfinite(got).all():
        return False, np.inf
    r = np.abs(got.astype(f64) - ref) / bound
    return bool((r <= 1.0).all()), float(r.max()) if r.size else 0.0


# ---- float64 references and their bounds: lists over the clips of (ref, bound), each shaped like the clip's rows of the output ----
def _silu(v):
    return v / (1 + np.exp(-v))


def ref_stem(c, s, mut=None):
    x = c.a["in_"][c.clip(s)].astype(f64)
    x = x if mut == "no_clamp" else np.clip(x, -1, 1)
    xp = np.concatenate([[0.0], x, [0.0]])
    w, b = c.a["w"].astype(f64), c.a["bias"].astype(f64)
    terms = np.stack([np.outer(xp[k:k + len(x)], w[:, k]) for k in range(3)])
    return b + terms.sum(0), 3 * U * (np.abs(b) + np.abs(terms).sum(0)) + FMIN


def ref_gn(c, s, mut=None, silu=True):
    x = c.a["in_"][c.clip(s)].astype(f64)
    n, C_ = x.shape
    G = 32 if mut == "groups32" else groups(C_)
    cg = C_ // G
    xg = x.reshape(n, G, cg)
    N = n * cg
    mean = xg.mean(axis=(0, 2), keepdims=True)
    var = (xg ** 2).mean(axis=(0, 2), keepdims=True) - mean ** 2
    if mut == "unbiased":
        var = var * N / max(N - 1, 1)
    r = 1 / (np.sqrt(var) + EPS) if mut == "eps_outside" else 1 / np.sqrt(var + EPS)
    g, b = c.a["gamma"].astype(f64), c.a["beta"].astype(f64)
    d = (xg - mean)
    if mut == "silu_first":
        return (_silu(d * r).reshape(n, C_) * g + b), None
    v = (d * r).reshape(n, C_) * g + b
    y = _silu(v) if silu else v
    e_mean = (N + 2) * D * np.abs(xg).mean(axis=(0, 2), keepdims=True)
    e_var = (N + 2) * D * (xg ** 2).mean(axis=(0, 2), keepdims=True) + 2 * np.abs(mean) * e_mean + D * mean ** 2
    e_r_rel = e_var / (2 * (var + EPS)) + 2 * D + U
    e_d = e_mean + U * np.abs(d)
    e_p = (r * e_d + np.abs(d * r) * (e_r_rel + U)).reshape(n, C_)
    e_v = np.abs(g) * e_p + U * np.abs(v)
    if not silu:
        return y, e_v + FMIN
    E = np.exp(-v)
    return y, 1.1 * e_v + np.abs(y) * (EXP_REL * E / (1 + E) + U + DIV) + FMIN


def ref_down(c, s, mut=None):
    x = c.a["in_"][c.clip(s)].astype(f64)
    w, b = c.a["w"].astype(f64), c.a["bias"].astype(f64)
    n, F, K = len(x), c.stride, c.taps
    pad = 1 if mut == "pad1" else (K - 1) // 2
    step = F + 1 if mut == "stride_off" else F
    n_out = c.n_out[s]
    xp = np.zeros((n + 2 * K + step * n_out + 8, x.shape[1]))
    xp[pad:pad + n] = x
    y, A = np.tile(b, (n_out, 1)), np.tile(np.abs(b), (n_out, 1))
    for j in range(K):
        rows = xp[j:j + step * (n_out - 1) + 1:step]
        y += rows @ w[j]
        A += np.abs(rows) @ np.abs(w[j])
    if mut == "len_div":  # n / F rows: the last row of every clip whose length is no multiple of F is never written
        y = y.copy()
        y[n // F:] = np.nan
    return y, (K * x.shape[1] + 1) * U * A + FMIN


def ref_attn(c, s, mut=None):
    qkv = c.a["in_"][c.clip(s)].astype(f64)
    n, E, H = len(qkv), c.C, c.heads
    dh = E // H
    c2 = dh ** -0.5
    y, bound = np.zeros((n, E)), np.zeros((n, E))
    for h in range(H):
        q, k, v = (qkv[:, t * E + h * dh:t * E + (h + 1) * dh] for t in range(3))
        sc = (q @ k.T) * (dh ** -0.25 if mut == "scale_once" else c2)
        e_s = (dh + 4) * U * (np.abs(q) @ np.abs(k).T) * c2
        w = np.exp(sc - sc.max(axis=1, keepdims=True))
        w /= w.sum(axis=1, keepdims=True)
        e_w = w * (e_s + (w * e_s).sum(axis=1, keepdims=True))
        rel = n * (2 * EXP_REL + 3 * U) + U * (sc.max(axis=1, keepdims=True) - sc.min(axis=1, keepdims=True)) + DIV
        y[:, h * dh:(h + 1) * dh] = w @ v
        bound[:, h * dh:(h + 1) * dh] = e_w @ np.abs(v) + rel * (w @ np.abs(v))
    return y, bound + FMIN


def ref_head(c, s, mut=None):
    x = c.a["in_"][c.clip(s)].astype(f64)
    row = x[-1] if mut == "last_position" else x[0]
    w, b = c.a["w"].astype(f64), c.a["bias"].astype(f64)
    l = w @ row + b
    e_l = (c.C / 64 + 7) * U * (np.abs(w) @ np.abs(row) + np.abs(b))
    e = np.exp(l - l.max())
    p = e / e.sum()
    return np.array([l[0], l[1], p[0]]), np.array([e_l[0], e_l[1], p[0] * p[1] * e_l.sum() + (2 * EXP_REL + 3 * U) * p[0]]) + FMIN


_REF = {STEM: ref_stem, GN: ref_gn, DOWN: ref_down, ATTN: ref_attn, HEAD: ref_head}


def reference(c, mut=None):
    return [_REF[c.kind](c, s, mut) for s in range(c.ns)]


def clip_output(c, payload, s):
    return payload[s] if c.kind == HEAD else payload[c.clip(s, out=c.kind == DOWN)]


# ---- float32 restatements, another summation order ----
def emulate(c, s):
    x = c.a["in_"][c.clip(s)]
    if c.kind == STEM:
        xc = np.concatenate([[f32(0)], np.clip(x, f32(-1), f32(1)), [f32(0)]]).astype(f32)
        w, n = c.a["w"], len(x)
        return (np.outer(xc[2:2 + n], w[:, 2]) + np.outer(xc[1:1 + n], w[:, 1]) + (np.outer(xc[:n], w[:, 0]) + c.a["bias"])).astype(f32)
    if c.kind == GN:  # the statistics in double, as the kernel keeps them (in numpy's pairwise order); everything behind them in float32
        n, C_ = x.shape
        G = groups(C_)
        xg = x.reshape(n, G, C_ // G).astype(f64)
        mean = xg.mean(axis=(0, 2), keepdims=True)
        var = ((xg - mean) ** 2).mean(axis=(0, 2), keepdims=True)  # the two-pass form: another route to the same number
        r = (1 / np.sqrt(var + EPS)).astype(f32)
        d = (xg - mean).astype(f32)
        v = ((d * r).reshape(n, C_) * c.a["gamma"] + c.a["beta"]).astype(f32)
        return (v / (f32(1) + np.exp(-v))).astype(f32)
    if c.kind == DOWN:
        n, F, K, pad = len(x), c.stride, c.taps, (c.taps - 1) // 2
        n_out = c.n_out[s]
        xp = np.zeros((n + 2 * K + F * n_out + 8, x.shape[1]), f32)
        xp[pad:pad + n] = x
        y = np.zeros((n_out, c.C2), f32)
        for j in reversed(range(K)):
            y += xp[j:j + F * (n_out - 1) + 1:F] @ c.a["w"][j]
        return (y + c.a["bias"]).astype(f32)
    if c.kind == ATTN:
        n, E, H = len(x), c.C, c.heads
        dh = E // H
        y = np.zeros((n, E), f32)
        for h in range(H):
            q, k, v = (x[:, t * E + h * dh:t * E + (h + 1) * dh] for t in range(3))
            sc = ((q * f32(dh ** -0.25)) @ (k * f32(dh ** -0.25)).T).astype(f32)
            w = np.exp(sc - sc.max(axis=1, keepdims=True)).astype(f32)
            y[:, h * dh:(h + 1) * dh] = (w @ v) / w.sum(axis=1, keepdims=True, dtype=f32)
        return y
    l = (c.a["w"] @ x[0] + c.a["bias"]).astype(f32)
    e = np.exp(l - l.max()).astype(f32)
    return np.array([l[0], l[1], e[0] / (e[0] + e[1])], f32)


# ---- the case matrix (tests/test_cls_kernels_gpu.py runs every one of these; the CPU test holds the restatement and the defects to them) ----
def stem_cases():
    return [make(STEM, n, 32) for n in ((1, 2, 3), (255, 256, 257))] + [make(STEM, (63, 64, 65), 32, gap=0)]


def gn_cases():
    t = GN_TILE
    out = [make(GN, n, C_) for C_ in (32, 64, 128) for n in ((1, 2, t - 1), (t, t + 1, 3 * t + 1))]
    return out + [make(GN, (3 * t + 1, t - 1), 32, fam="offset"), make(GN, (t + 1, 5), 128, fam="offset", gap=0), make(GN, (9, 300), 1024)]


def down_cases():
    t = DOWN_TILE * 4
    ns = ((1, 2, 3), (4, 5, 6), (7, 8, 9), (t - 4, t - 3, t + 1))  # the last: 63, 64 and 65 output rows
    return [make(DOWN, n, 32, 64) for n in ns] + [make(DOWN, n, 512, 1024) for n in ns] + [make(DOWN, (10, 33), 64, 128, stride=2, gap=0)]


def attn_cases():
    return [make(ATTN, n, 256, heads=2) for n in ((1, 2, 63), (64, 65, 215))] + [make(ATTN, (33, 215), 256, heads=2, fam="peaked"),
                                                                                 make(ATTN, (65, 7), 256, heads=4, gap=0)]


def head_cases():
    return [make(HEAD, (1, 9, 215), 512), make(HEAD, (4,), 256, gap=0)]


def all_cases():
    return stem_cases() + gn_cases() + down_cases() + attn_cases() + head_cases()


DEFECTS = {STEM: ["no_clamp"], GN: ["unbiased", "eps_outside", "silu_first", "groups32"], DOWN: ["pad1", "stride_off", "len_div"], ATTN: ["scale_once"],
           HEAD: ["last_position"]}
