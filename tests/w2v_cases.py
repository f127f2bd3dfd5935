"""Shared by tests/test_w2v_kernels_gpu.py and tests/test_w2v_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/w2v_harness.hip -> libtts_w2v_test.so), float64 NumPy references of the aligner's five new kernels (csrc/aligner.h), the case matrix,
the acceptance rule and its error bounds, float32 restatements in another summation order, and the defects the rule must reject.

LAYOUT, as aligner_run builds it: clip s owns the rows [start_s, start_s + n_s) of a buffer, start = the running sum of ceil8(n) (the cases add gaps). The input
rows that belong to no clip hold 3.5 (NaN in the poisoned twin); the output starts as the sentinel byte everywhere and keeps it outside the clips.

REFERENCES are float64 on the float32 values the kernel reads, so that a bound covers arithmetic only.

ACCEPTANCE, first order and term by term, nothing fitted; U = 2^-24, D = 2^-53. A chain of n fused multiply-adds rounds n times, each time a partial sum of at
most A = sum |terms|: n U A (the f32-input MFMA is such a chain: one rounding per product, no wider accumulator).
  stats     double sums of exact widenings and of products rounded once, over n samples: e_mean = (n + 2) D mean|x|;  var = (sum x^2 - sum x mean) / (n - 1):
            e_var = (n + 4) D (mean(x^2) + mean^2) n / (n - 1);  r = 1 / sqrt(var + eps): e_r = r (e_var / (2 (var + eps)) + 2 D)
  stem      xn = fl(fl(x - mean) fl(r)): three roundings, 3 U |xn|;  then taps fused multiply-adds: (taps + 3) U (|b| + sum_k |w_k xn_k|)
  LayerNorm mean = sum / C (C / 64 chained adds per lane, a 6-level tree, the division): e_mean = (C / 64 + 7) U mean|x|;  d = fl(x - mean): e_d = e_mean + U |d|
            var = sum d^2 / C: e_var = (C / 64 + 8) U var + 2 mean(|d| e_d);  r = 1 / sqrtf(var + eps): e_r / r = e_var / (2 (var + eps)) + 3 DIV
            p = fl(d r): e_p = r e_d + |d r| (e_r / r + U);  v = fma(p, gamma, beta): e_v = |gamma| e_p + U |v|
  GELU      y = 0.5 v (1 + erff(v / sqrt 2)): e_y = 1.13 e_v + 0.5 |v| (ERF_ABS + 1.13 U |v|) + 3 U |y|       (|GELU'| <= 1.13, the argument's rounding through
            erf' <= 2 / sqrt(pi), three multiplications and the addition)
  pos       v = bias + the chain over taps x channels-per-group products: e_v = (taps cg + 1) U (|b| + sum |x w|);  out = in + GELU(v): e = e_y(e_v) + U |out|
  head      (D + 1) U (|b| + sum |w x|) per logit. The id: the float64 argmax wherever the row's top-two margin exceeds twice the row's largest bound; elsewhere
            any id whose float64 logit is within that distance of the maximum. On the exact family (small integers: every logit exact in f32) the logits are
            bit-equal to float64 and the id is numpy's argmax: the lowest index on a tie.
ERF_ABS = 4 ulp of a value below 1 = 8 U: device erff (the HIP math API reference's table of maximum ulp errors lists 4). DIV = 2 U (gn_cases.py: "an IEEE
division or square root 2u").

DEFECTS are applied to the reference (reference(case, mut=...)); test_w2v_harness_cpu.py requires each to leave the bound of the unmutated reference on some case."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

f32, f64, i32 = np.float32, np.float64, np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
SRC = os.path.join(PKG, "testlib", "w2v_harness.hip")
LIB = os.environ.get("TTS_W2V_TEST_LIB", os.path.join(PKG, "libtts_w2v_test.so"))
STATS, STEM, LN, POS, HEAD = 0, 1, 2, 3, 4
KIND_NAMES = {STATS: "stats", STEM: "stem", LN: "ln", POS: "pos", HEAD: "head"}
HIP_INVALID_VALUE = 1
SENTINEL = 0xCB
SEQ = 9
U, D = 2.0 ** -24, 2.0 ** -53
FMIN = 2.0 ** -126
DIV, ERF_ABS = 2 * U, 8 * U
JUNK = f32(3.5)
ST_TILE, STEM_TILE, POS_TILE, HEAD_TILE = 4096, 64, 64, 8
EPS_CLIP, EPS_LN = 1e-7, 1e-5
_erf = np.vectorize(math.erf, otypes=[f64])


class CaseStruct(C.Structure):
    _fields_ = [("kind", C.c_int), ("ns", C.c_int), ("rows", C.c_int), ("C", C.c_int), ("C2", C.c_int), ("taps", C.c_int), ("stride", C.c_int), ("mode", C.c_int),
                ("rows_out", C.c_int), ("n", C.c_void_p), ("start", C.c_void_p), ("start_out", C.c_void_p), ("in_", C.c_void_p), ("w", C.c_void_p),
                ("bias", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("stat", C.c_void_p), ("out", C.c_void_p), ("out2", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_w2v_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_w2v_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_w2v_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_w2v_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_w2v_test_table.argtypes = [C.POINTER(CaseStruct), C.c_void_p, C.c_void_p]
        L.tts_w2v_test_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
        L.tts_w2v_test_packed.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong]
        L.tts_w2v_test_packed.restype = C.c_longlong
        for f in (L.tts_w2v_test_run, L.tts_w2v_test_validate, L.tts_w2v_test_table, L.tts_w2v_test_parse, L.tts_w2v_test_margin, L.tts_w2v_test_stat_tile,
                  L.tts_w2v_test_stem_tile, L.tts_w2v_test_pos_tile, L.tts_w2v_test_head_tile):
            f.restype = C.c_int
        _lib = L
    return _lib


def parse(path):
    """the loader's host half on a file: (status, [N, C, D, K, channels of a group, depth, feed-forward width, V, heads, blank], message)"""
    out, err = np.zeros(10, i32), C.create_string_buffer(512)
    rc = harness().tts_w2v_test_parse(path.encode(), out.ctypes.data_as(C.c_void_p), err, 512)
    return rc, out, err.value.decode()


def packed(path, which, i=0):
    L = harness()
    cnt = L.tts_w2v_test_packed(path.encode(), which, i, None, 0)
    assert cnt > 0, cnt
    out = np.zeros(cnt, f32)
    assert L.tts_w2v_test_packed(path.encode(), which, i, out.ctypes.data_as(C.c_void_p), cnt) == cnt
    return out


def ceil8(v):
    return (v + 7) // 8 * 8


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape, dtype=f32):
        self.margin = harness().tts_w2v_test_margin()
        self.shape, self.dtype = shape, dtype
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * np.dtype(dtype).itemsize, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


def _layout(n, gap):
    out, run = [], gap
    for v in n:
        out.append(run)
        run += ceil8(v) + gap
    return out, run


class Case(object):
    """gap: rows of no clip in front of, between and behind the clips (a multiple of 8; 0 = aligner_run's own packing, no explicit start table).
    C2: POS channels of a group, HEAD V. mode: LN 0 LayerNorm / 1 + GELU / 2 the GELU kernel alone; HEAD 1 = logits wanted."""

    def __init__(self, kind, n, C_=64, C2=0, taps=10, stride=5, mode=0, gap=8, fam="gauss", seed=0):
        self.kind, self.n, self.C, self.C2, self.taps, self.stride, self.mode, self.gap, self.fam, self.seed = kind, list(n), C_, C2, taps, stride, mode, gap, fam, seed
        self.start, self.rows = _layout(self.n, gap)
        self.n_out = [(v - taps) // stride + 1 for v in self.n] if kind == STEM else list(self.n)
        self.start_out, self.rows_out = _layout(self.n_out, gap)
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
        return {STATS: (self.ns, 2), STEM: (self.rows_out, self.C), LN: (self.rows, self.C), POS: (self.rows, self.C), HEAD: (self.rows, self.C2)}[self.kind]

    def table(self, out=False):
        t, tiles = np.zeros((self.ns, SEQ), i32), 0
        for s in range(self.ns):
            st, n = (self.start_out[s], self.n_out[s]) if out else (self.start[s], self.n[s])
            t[s, 0], t[s, 1], t[s, 3], t[s, 4] = st, n, tiles, st
            tiles += (n + ST_TILE - 1) // ST_TILE
        return t

    def name(self):
        extra = {STATS: "", STEM: " k%d s%d" % (self.taps, self.stride), LN: " m%d" % self.mode, POS: " g%d K%d" % (self.C2, self.taps), HEAD: " V%d" % self.C2}[self.kind]
        return "%s n%s C%d%s %s" % (KIND_NAMES[self.kind], "-".join(map(str, self.n)), self.C, extra, self.fam)


def make(kind, n, C_=64, C2=0, taps=10, stride=5, mode=0, gap=8, fam="gauss", seed=0):
    """fam: gauss = unit-scale values; offset (STATS, LN) = the mean is 30 x the deviation; exact (HEAD) = small integers, every logit exact in f32, many ties"""
    c = Case(kind, n, C_, C2, taps, stride, mode, gap, fam, seed)
    rs = np.random.RandomState(1000 * kind + 31 * seed + sum(c.n) + 7 * c.C + c.C2 + taps + mode)
    if kind in (STATS, STEM):
        x = (rs.randn(c.rows) * 0.2 + (6.0 if fam == "offset" else 0.05)).astype(f32)
        x[~c.live()] = JUNK
        c.a["in_"] = x
        if kind == STEM:
            stat = np.zeros((c.ns, 2), f64)
            for s in range(c.ns):
                v = x[c.clip(s)].astype(f64)
                stat[s] = [v.mean() * (1 + 1e-9), 1 / np.sqrt(v.var(ddof=1) + EPS_CLIP)]  # any double pair is a legal operand: the mean is not f32-representable
            c.a.update(stat=stat, w=(rs.randn(c.C, taps) / np.sqrt(taps)).astype(f32), bias=(rs.randn(c.C) * 0.1).astype(f32))
        return c
    if fam == "exact":
        x = rs.randint(-2, 3, (c.rows, c.C)).astype(f32)
    else:
        x = rs.randn(c.rows, c.C).astype(f32)
        if fam == "offset":
            x = (x * f32(0.37) + f32(11.0)).astype(f32)
    x[~c.live()] = JUNK
    c.a["in_"] = x
    if kind == LN:
        c.a.update(gamma=(1 + 0.3 * rs.randn(c.C)).astype(f32), beta=(0.3 * rs.randn(c.C)).astype(f32))
    elif kind == POS:
        G = c.C // c.C2
        c.a.update(w=(rs.randn(G, taps, c.C2, c.C2) / np.sqrt(taps * c.C2) * 2).astype(f32), bias=(rs.randn(c.C) * 0.1).astype(f32))
    elif kind == HEAD:
        if fam == "exact":
            c.a.update(w=rs.randint(-1, 2, (c.C, c.C2)).astype(f32), bias=rs.randint(-1, 2, c.C2).astype(f32))
        else:
            c.a.update(w=(rs.randn(c.C, c.C2) / np.sqrt(c.C) * 4).astype(f32), bias=rs.randn(c.C2).astype(f32))
    return c


def struct(c, out_buf, out2_buf=None, **override):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    keep = dict(n=np.array(c.n, i32), start=np.array(c.start, i32) if c.gap else None, start_out=np.array(c.start_out, i32) if c.gap else None)
    f = dict(kind=c.kind, ns=c.ns, rows=c.rows, C=c.C, C2=c.C2, taps=c.taps, stride=c.stride, mode=c.mode, rows_out=c.rows_out, n=p(keep["n"]),
             start=p(keep["start"]), start_out=p(keep["start_out"]), in_=p(c.a.get("in_")), w=p(c.a.get("w")), bias=p(c.a.get("bias")), gamma=p(c.a.get("gamma")),
             beta=p(c.a.get("beta")), stat=p(c.a.get("stat")), out=p(out_buf), out2=p(out2_buf))
    f.update(override)
    return CaseStruct(**f), keep


def _buffers(c):
    g = Guarded(c.out_shape(), f64 if c.kind == STATS else f32)
    g2 = Guarded((c.rows,), i32) if c.kind == HEAD else None
    return g, g2


def validate(c, **override):
    g, g2 = _buffers(c)
    s, keep = struct(c, g.raw, None if g2 is None else g2.raw, **override)
    return harness().tts_w2v_test_validate(C.byref(s))


def run(c):
    """one launch on the device: (Guarded output, Guarded ids or None)"""
    g, g2 = _buffers(c)
    g.raw[:] = 0x11  # the harness overwrites all of it
    if g2 is not None:
        g2.raw[:] = 0x11
    s, keep = struct(c, g.raw, None if g2 is None else g2.raw)
    rc = harness().tts_w2v_test_run(C.byref(s))
    assert rc == 0, "harness status %d on %s" % (rc, c.name())
    return g, g2


def alone(c, s):
    """clip s of a case as a case of its own (same operands, packed as aligner_run packs a single clip)"""
    a = Case(c.kind, [c.n[s]], c.C, c.C2, c.taps, c.stride, c.mode, 0, c.fam, c.seed)
    a.a = dict(c.a)
    x = c.a["in_"]
    blank = np.full((a.rows,) + x.shape[1:], JUNK, f32)
    blank[a.clip(0)] = x[c.clip(s)]
    a.a["in_"] = blank
    if "stat" in c.a:
        a.a["stat"] = c.a["stat"][s:s + 1].copy()
    return a


def poisoned(c):
    a = Case(c.kind, c.n, c.C, c.C2, c.taps, c.stride, c.mode, c.gap, c.fam, c.seed)
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
def gelu64(v, mut=None):
    if mut == "gelu_tanh":
        return 0.5 * v * (1 + np.tanh(np.sqrt(2 / np.pi) * (v + 0.044715 * v ** 3)))
    return 0.5 * v * (1 + _erf(v / np.sqrt(2.0)))


def _e_gelu(v, y, e_v):
    return 1.13 * e_v + 0.5 * np.abs(v) * (ERF_ABS + 1.13 * U * np.abs(v)) + 3 * U * np.abs(y)


def ref_stats(c, s, mut=None):
    x = c.a["in_"][c.clip(s)].astype(f64)
    n = len(x)
    mean = x.mean()
    var = ((x - mean) ** 2).sum() / (n if mut == "biased" else max(n - 1, 1)) if n > 1 else 0.0
    r = 1 / np.sqrt(var + EPS_CLIP)
    e_mean = (n + 2) * D * np.abs(x).mean() + FMIN
    e_var = (n + 4) * D * ((x ** 2).mean() + mean ** 2) * n / max(n - 1, 1)
    return np.array([mean, r]), np.array([e_mean, r * (e_var / (2 * (var + EPS_CLIP)) + 2 * D) + FMIN])


def ref_stem(c, s, mut=None):
    x = c.a["in_"][c.clip(s)].astype(f64)
    mean, r = c.a["stat"][s]
    xn = (x - mean) * f64(f32(r))
    w, b = c.a["w"].astype(f64), c.a["bias"].astype(f64)
    T, k, st = c.n_out[s], c.taps, c.stride
    ref, A = np.tile(b, (T, 1)), np.tile(np.abs(b), (T, 1))
    for j in range(k):
        col = xn[j:j + st * (T - 1) + 1:st][:, None]
        wj = w[:, k - 1 - j] if mut == "tap_order" else w[:, j]
        ref += col * wj[None]
        A += np.abs(col * wj[None])
    return ref, (k + 3) * U * A + FMIN


def _ln64(x, g, b):
    Cn = x.shape[1]
    mean = x.mean(axis=1, keepdims=True)
    d = x - mean
    var = (d ** 2).mean(axis=1, keepdims=True)
    r = 1 / np.sqrt(var + EPS_LN)
    v = d * r * g + b
    e_mean = (Cn / 64 + 7) * U * np.abs(x).mean(axis=1, keepdims=True)
    e_d = e_mean + U * np.abs(d)
    e_var = (Cn / 64 + 8) * U * var + 2 * (np.abs(d) * e_d).mean(axis=1, keepdims=True)
    e_r = e_var / (2 * (var + EPS_LN)) + 3 * DIV
    e_p = r * e_d + np.abs(d * r) * (e_r + U)
    return v, np.abs(g) * e_p + U * np.abs(v)


def ref_ln(c, s, mut=None):
    x = c.a["in_"][c.clip(s)].astype(f64)
    if c.mode == 2:
        y = gelu64(x, mut)
        return y, _e_gelu(x, gelu64(x), 0.0) + FMIN
    v, e_v = _ln64(x, c.a["gamma"].astype(f64), c.a["beta"].astype(f64))
    if c.mode == 0:
        return v, e_v + FMIN
    return gelu64(v, mut), _e_gelu(v, gelu64(v), e_v) + FMIN


def ref_pos(c, s, mut=None):
    x = c.a["in_"][c.clip(s)].astype(f64)
    w, b = c.a["w"].astype(f64), c.a["bias"].astype(f64)
    T, Dm, cg, K = x.shape[0], c.C, c.C2, c.taps
    pad = K // 2
    xp = np.zeros((T + 2 * pad + 1, Dm), f64)
    xp[pad:pad + T] = x
    shift = 1 if (mut == "keep_last_row" and K % 2 == 0) else 0  # rows 1 .. T of PyTorch's T + 1 outputs instead of 0 .. T - 1
    v, A = np.tile(b, (T, 1)), np.tile(np.abs(b), (T, 1))
    for g in range(Dm // cg):
        cols = slice(g * cg, (g + 1) * cg)
        src = slice(g * cg + 1, (g + 1) * cg + 1) if mut == "group_offset" else cols
        for j in range(K):
            rows = xp[j + shift:j + shift + T]
            xin = np.concatenate([rows, rows[:, :1]], axis=1)[:, src] if mut == "group_offset" else rows[:, cols]
            v[:, cols] += xin @ w[g, j]
            A[:, cols] += np.abs(xin) @ np.abs(w[g, j])
    e_v = (K * cg + 1) * U * A
    y = gelu64(v, mut)
    out = y if mut == "no_residual" else x + y
    return out, _e_gelu(v, gelu64(v), e_v) + U * np.abs(x + gelu64(v)) + FMIN


def ref_head(c, s, mut=None):
    x = c.a["in_"][c.clip(s)].astype(f64)
    w, b = c.a["w"].astype(f64), c.a["bias"].astype(f64)
    ref = x @ w + b
    return ref, (c.C + 1) * U * (np.abs(x) @ np.abs(w) + np.abs(b)) + FMIN


def ref_ids(logits, mut=None):
    if mut == "argmax_last":
        return logits.shape[1] - 1 - np.argmax(logits[:, ::-1], axis=1)
    return np.argmax(logits, axis=1)


def ids_ok(ids, ref, bound):
    """the float64 argmax where the row's margin exceeds twice its largest bound; elsewhere an id within that distance of the maximum"""
    if ids.shape != (ref.shape[0],) or (ids < 0).any() or (ids >= ref.shape[1]).any():
        return False
    slack = 2 * bound.max(axis=1)
    top = ref.max(axis=1)
    chosen = ref[np.arange(len(ids)), ids]
    srt = np.sort(ref, axis=1)
    sure = (srt[:, -1] - srt[:, -2] > slack) if ref.shape[1] > 1 else np.ones(len(ids), bool)
    return bool((chosen >= top - slack).all() and (ids[sure] == np.argmax(ref, axis=1)[sure]).all())


def ids_accept(c, ids, ref, bound):
    """the rule for a case: on the exact family every logit is exact, so the id is numpy's argmax (the lowest index on a tie) and nothing else"""
    return bool(np.array_equal(ids, ref_ids(ref))) if c.fam == "exact" else ids_ok(ids, ref, bound)


_REF = {STATS: ref_stats, STEM: ref_stem, LN: ref_ln, POS: ref_pos, HEAD: ref_head}


def reference(c, mut=None):
    return [_REF[c.kind](c, s, mut) for s in range(c.ns)]


def clip_output(c, payload, s):
    """clip s's rows of an output payload (STATS: its pair)"""
    return payload[s] if c.kind == STATS else payload[c.clip(s, out=c.kind == STEM)]


def emulate(c, s):
    """float32 restatement of the kernel on clip s in ANOTHER summation order (statistics: double, descending): a correct implementation the bound must admit"""
    x = c.a["in_"][c.clip(s)]
    if c.kind == STATS:
        v = x.astype(f64)[::-1]
        n = len(v)
        sm, sq = np.cumsum(v)[-1], np.cumsum(v * v)[-1]
        mean = sm / n
        var = max((sq - sm * mean) / (n - 1), 0.0) if n > 1 else 0.0
        return np.array([mean, 1 / np.sqrt(var + EPS_CLIP)])
    if c.kind == STEM:
        mean, r = c.a["stat"][s]
        xn = ((x.astype(f64) - mean).astype(f32) * f32(r)).astype(f32)
        T, k, st = c.n_out[s], c.taps, c.stride
        acc = np.zeros((T, c.C), f32)
        for j in reversed(range(k)):
            acc = (acc + xn[j:j + st * (T - 1) + 1:st][:, None] * c.a["w"][:, j][None]).astype(f32)
        return (acc + c.a["bias"]).astype(f32)
    g32 = lambda v: (f32(0.5) * v * (f32(1) + _erf(v.astype(f64) / np.sqrt(2.0)).astype(f32))).astype(f32)  # noqa: E731
    if c.kind == LN:
        if c.mode == 2:
            return g32(x)
        mean = x.mean(axis=1, keepdims=True, dtype=f32)
        d = (x - mean).astype(f32)
        var = (d * d).mean(axis=1, keepdims=True, dtype=f32)
        v = (d * (f32(1) / np.sqrt(var + f32(EPS_LN))).astype(f32) * c.a["gamma"] + c.a["beta"]).astype(f32)
        return g32(v) if c.mode == 1 else v
    if c.kind == POS:
        T, cg, K = x.shape[0], c.C2, c.taps
        xp = np.zeros((T + 2 * (K // 2), c.C), f32)
        xp[K // 2:K // 2 + T] = x
        v = np.zeros((T, c.C), f32)
        for g in range(c.C // cg):
            cols = slice(g * cg, (g + 1) * cg)
            for j in reversed(range(K)):  # taps descending, the channels by numpy's own blocking
                v[:, cols] = (v[:, cols] + xp[j:j + T, cols] @ c.a["w"][g, j]).astype(f32)
        return (x + g32((v + c.a["bias"]).astype(f32))).astype(f32)
    return (x[:, ::-1] @ c.a["w"][::-1] + c.a["bias"]).astype(f32)


# ---- the case matrix: tile edges (1 row, tile - 1, tile, tile + 1), two and three clips of different lengths, both K parities, V off a multiple of 32 ----
def stats_cases():
    return [make(STATS, n, fam=fam, seed=i) for i, (n, fam) in enumerate([([2], "gauss"), ([ST_TILE - 1], "gauss"), ([ST_TILE, ST_TILE + 1, 100], "gauss"),
                                                                           ([9000, 3], "offset"), ([2 * ST_TILE + 5], "offset")])]


def stem_cases():
    f = lambda F, k=10, s=5: k + s * (F - 1)  # noqa: E731  samples of F frames
    return ([make(STEM, n, 64, taps=10, stride=5, seed=i) for i, n in enumerate([[f(1)], [f(STEM_TILE - 1) + 4], [f(STEM_TILE), f(STEM_TILE + 1), f(2) + 3], [f(130), f(1)]])]
            + [make(STEM, [f(70, 3, 2), f(1, 3, 2) + 1], 128, taps=3, stride=2, seed=9), make(STEM, [f(65)], 64, taps=10, stride=5, fam="offset", seed=10)])


def ln_cases():
    out = []
    for i, (n, C_, mode, fam) in enumerate([([1], 64, 0, "gauss"), ([3, 4, 5], 64, 1, "gauss"), ([70, 9], 128, 0, "offset"), ([70, 9], 128, 1, "gauss"),
                                            ([5, 1], 1024, 1, "gauss"), ([6], 512, 0, "offset"), ([63, 64, 65], 256, 2, "gauss"), ([1], 64, 2, "gauss")]):
        out.append(make(LN, n, C_, mode=mode, fam=fam, seed=i))
    return out


def pos_cases():
    out = []
    for i, (n, Dm, cg, K) in enumerate([([1], 128, 64, 8), ([POS_TILE - 1], 128, 64, 8), ([POS_TILE, POS_TILE + 1, 3], 128, 64, 8), ([1], 128, 64, 7),
                                        ([POS_TILE + 1, POS_TILE], 128, 64, 7), ([70, 5], 64, 64, 128), ([65, 10], 256, 128, 3), ([130], 128, 64, 1)]):
        out.append(make(POS, n, Dm, cg, taps=K, seed=i))
    return out


def head_cases():
    out = []
    for i, (n, Dm, V, fam) in enumerate([([1], 128, 29, "gauss"), ([HEAD_TILE - 1, HEAD_TILE, HEAD_TILE + 1], 128, 33, "gauss"), ([70], 128, 29, "gauss"),
                                         ([9], 1024, 32, "gauss"), ([5, 2], 64, 1024, "gauss"), ([3], 64, 1, "gauss"), ([40, 7], 128, 33, "exact"),
                                         ([9], 64, 65, "exact")]):
        out.append(make(HEAD, n, Dm, V, mode=1, fam=fam, seed=i))
    return out


def all_cases():
    return stats_cases() + stem_cases() + ln_cases() + pos_cases() + head_cases()


DEFECTS = {STATS: ["biased"], STEM: ["tap_order"], LN: ["gelu_tanh"], POS: ["keep_last_row", "group_offset", "gelu_tanh", "no_residual"], HEAD: ["argmax_last"]}

# what the harness must refuse before any HIP call: (kind of the base case, the fields it changes)
INVALID = [(LN, dict(ns=0)), (LN, dict(ns=5)), (LN, dict(rows=7)), (LN, dict(rows=1 << 16)), (LN, dict(C=96)), (LN, dict(C=2048)), (LN, dict(C=32)), (LN, dict(mode=3)),
           (LN, dict(gamma=None)), (LN, dict(in_=None)), (LN, dict(out=None)), (LN, dict(n=None)), (LN, dict(kind=5)), (LN, dict(kind=-1)),
           (STEM, dict(taps=0)), (STEM, dict(taps=65)), (STEM, dict(stride=0)), (STEM, dict(stride=9)), (STEM, dict(stat=None)), (STEM, dict(w=None)), (STEM, dict(rows_out=4)),
           (POS, dict(C2=32)), (POS, dict(C2=96)), (POS, dict(taps=0)), (POS, dict(taps=200, C2=128, C=128)), (POS, dict(bias=None)),
           (HEAD, dict(C2=0)), (HEAD, dict(C2=1025)), (HEAD, dict(mode=2)), (HEAD, dict(out2=None)), (HEAD, dict(w=None))]
