"""Shared by tests/test_voc_kernels_gpu.py and tests/test_voc_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/voc_harness.hip -> libtts_voc_test.so), float64 NumPy references of the UnivNet vocoder's kernels (csrc/vocoder.hip), the case matrix,
the acceptance rule and its error bound, float32 restatements that sum in two orders, and the defects the rule must reject.

The references share no code with the harness or the kernels; test_voc_harness_cpu.py checks them against naive loops written from the comments of vocoder.hip.

LAYOUTS, as voc_run builds them (first start 8, next start (r + len + 1 + 7) & ~7): A (11,) 24 rows; B (15, 11) 40 rows with exactly ONE guard frame between the
sequences; C (12, 11, 20) 64 rows; D = B padded to 128 rows. An audio-rate tensor at `hop` samples per frame is [rows * hop][channels].

REFERENCES are float64 on the values the kernel multiplies. The fp16-operand convs (conv_direct, voc_dconv_mfma, conv_post) get the operand path bit-exactly:
leaky as v > 0 ? v : float32(0.2) * v in float32, then round-to-nearest fp16, weights already fp16-valued; their products are exact in f32, so only the
accumulation is in the kernel's error. convt and the two LVC kernels take f32 operands (convt: the float32 leaky of x). The LVC reference takes the predicted
kernel in the reference's order (i*64 + ch)*3 + tap; the runner permutes it with the lvc_col the harness exports from the product.

ACCEPTANCE, first order and term by term, nothing fitted; u = 2^-24. A sum of n terms in ANY order (the order inside an MFMA included) puts at most n roundings
on a term (for f32 operands: the product's and n - 1 additions'), each of relative size u of a partial sum that is at most sum |terms|:
      bound = (n + c) u (sum |terms| + |bias| + |resid|)
with c = the roundings after the sum:  conv_direct 3 (bias add, leaky multiply, residual add); voc_dconv_mfma 2 (bias add, leaky multiply); conv_post 1 (bias
add); convt 1 (the bias is the accumulator's first value: one more term); the LVC pre-activations 1 (bias add). leaky is 1-Lipschitz, so an error in front of it
is not amplified. voc_mel_rows: v = ((m + 1) / 2) d + MINV with d = fl(MAXV - MINV): the sum m + 1, the product and the final add round once each (a contracted
multiply-add removes one), |m + 1| / 2 * d and |MINV| bound the partial values: 4 u (|m + 1| / 2 * d + |MINV|). voc_noise_rows / voc_cond_f16: exact.

GATE, x += sigmoid(a) tanh(b) =: g(a, b), with Da, Db the bounds of the two pre-activations from the rule above:
  propagated   Da |dg/da| + Db |dg/db| <= Da / 4 + Db
  gate_dev     hardware exp2 and reciprocal: 1 ulp each (<= 2u relative); f32 products, sums: u.
     sg = rcp(1 + exp2(fl(a * -log2e))):  the scaled argument carries 2u relative (the f32 constant and the product), i.e. 2u |a| log2e absolute, and
          2^x turns an absolute error d of x into the relative error d ln2:  E = e^-a carries rE = 2u |a| + 2u (exp2);  1 + E: u;  rcp: 2u.
          d sg / sg = -dE / (1 + E) = -rE (1 - sg):        rel(sg) <= (1 - sg) rE + 3u
     th = 1 - 2 rcp(1 + exp2(fl(b * 2 log2e))):  F = e^2b carries rF = 4u |b| + 2u;  r = 1 / (1 + F) carries rF F / (1 + F) + 3u relative, F / (1 + F) = (1 + tanh b) / 2;
          2 r = 1 - tanh b exactly, and the subtraction rounds once:
                                                           abs(th) <= (1 - tanh b) (rF (1 + tanh b) / 2 + 3u) + u |tanh b|
          This is ABSOLUTE: at b -> 0 it tends to 4u = 2.4e-7 whatever b is, so the relative error of tanh near 0 is unbounded (b = 1e-6: up to 24 %). The
          comment in vocoder.hip that says "1e-7-level relative error" holds for sigmoid and for |tanh| near 1, not for tanh near 0.
     g = fl(sg th):                                        abs(g) <= |tanh b| sg rel(sg) + sg abs(th) + u |g|
     results below the smallest normal f32 may be flushed to zero: + 4 * 2^-126.
  the add      u |x + g|
  |a|, |b| = 88, 200 overflow exp2 to +inf or flush it to 0; rcp(inf) = 0 and 1 + 0 = 1 give sg in {0, 1}, th = -1, 1 there, which the bound above accepts
  (the true values differ from those by < 1e-38).

voc_philox_kernel: philox4x32_10() restates Philox4x32-10 (Salmon et al., SC'11) on NumPy uint32/uint64; pinned on the CPU against the Random123 known-answer
vectors and a pure-Python-int version. u1, u2 are restated in float32 bit for bit; Box-Muller in float64 with theta = 2 pi u2. Bound, with logf 2 ulp, sqrtf 1
ulp, sincosf 2 ulp (4u, 2u, 4u) and theta' = fl(fl(2 pi) u2) carrying 2u theta absolute:
      rad: 4u / 2 + 2u = 4u relative;  trig: 2u theta + 4u absolute;  x = fl(rad trig):   bound = rad (2u theta + 4u) + 5u |x|

INPUT FAMILIES: gauss; ramp (signed ramps); outlier (gauss plus one element of 3e4 per sequence: below the fp16 overflow at 65504, and so is 0.2 * 3e4; the same
value is used for the f32-operand kernels); straddle (gauss * 2^-6 with a quarter of the elements exactly +0 / -0 and signs mixed, so that the leaky branch and the
fp16 rounding of 0.2 v decide the operand); for the LVC kernels `gate`: predicted kernel = 0 and kb sweeping (a, b) over GATE_GRID x GATE_GRID, so that the output
is x + gate_dev(a, b) alone (`gate0`: the same with x = 0 on the live positions, so that the output is gate_dev(a, b) itself and its error can be reported). The
layers of kern / kb that the launch does not name are NaN.

DEFECTS are applied to the reference (reference(mut=...)); test_voc_harness_cpu.py requires each to leave the bound of the unmutated reference on some case."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_VOC_TEST_LIB") or os.path.join(PKG, "libtts_voc_test.so")
SRC = os.path.join(PKG, "testlib", "voc_harness.hip")

CONV, CONVT, LVC_GATE, LVC_MFMA, DCONV, POST, MEL_ROWS, NOISE_ROWS, COND_F16, PHILOX = range(10)
KIND_NAMES = ["conv_direct_kernel", "convt_kernel", "lvc_gate_kernel", "lvc_mfma_kernel", "voc_dconv_mfma_kernel", "conv_post_kernel", "voc_mel_rows_kernel",
              "voc_noise_rows_kernel", "voc_cond_f16_kernel", "voc_philox_kernel"]
SENTINEL = 0xCB
HIP_INVALID_VALUE = 1
U = 2.0 ** -24
FMIN = 2.0 ** -126
L02 = float(np.float32(0.2))
C_AFTER = {CONV: 3, DCONV: 2, POST: 1, CONVT: 1, LVC_GATE: 1, LVC_MFMA: 1}
OUTLIER = 3.0e4
GATE_GRID = np.array([s * m for m in (0.0, 1e-6, 1e-4, 1e-2, 1.0, 10.0, 20.0, 88.0, 200.0) for s in (1.0, -1.0)], np.float32)
MAXV, MINV = np.float32(2.3143386840820312), np.float32(-11.512925148010254)
PADV = np.float32(-11.5129)
LAYOUTS = {"A": ((11,), None), "B": ((15, 11), None), "C": ((12, 11, 20), None), "D": ((15, 11), 128)}


class CaseStruct(C.Structure):
    _fields_ = [("kind", C.c_int), ("ns", C.c_int), ("rows", C.c_int), ("hop", C.c_int), ("s", C.c_int), ("dil", C.c_int), ("layer", C.c_int),
                ("Cin", C.c_int), ("Cout", C.c_int), ("K", C.c_int), ("pad", C.c_int), ("pre_leaky", C.c_int), ("post_leaky", C.c_int), ("reflect", C.c_int),
                ("stream", C.c_uint), ("seed", C.c_ulonglong), ("n", C.c_longlong),
                ("start", C.c_void_p), ("len", C.c_void_p),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("resid", C.c_void_p), ("kern", C.c_void_p), ("kb", C.c_void_p), ("xio", C.c_void_p),
                ("out", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_voc_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_voc_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_voc_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_voc_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_voc_test_lvc_col.argtypes = [C.c_int, C.c_int, C.c_int]
        for f in (L.tts_voc_test_run, L.tts_voc_test_validate, L.tts_voc_test_margin, L.tts_voc_test_lvc_col):
            f.restype = C.c_int
        _lib = L
    return _lib


_perm = None


def lvc_perm():
    """perm[(i*64 + ch)*3 + tap] = lvc_col(tap, i, ch), read from the product through the harness (never restated here)"""
    global _perm
    if _perm is None:
        L = harness()
        _perm = np.array([L.tts_voc_test_lvc_col(tap, i, ch) for i in range(32) for ch in range(64) for tap in range(3)], np.int64)
    return _perm


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape, dtype):
        self.margin = harness().tts_voc_test_margin()
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * self.dtype.itemsize, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


_ARRAYS = dict(start=np.int32, len=np.int32, x=np.float32, w=np.float32, bias=np.float32, resid=np.float32, kern=np.float32, kb=np.float32, xio=np.float32)


def struct(kind, out=None, **kw):
    """A CaseStruct over the given arrays (kept alive on the struct). Array dtypes are checked here, everything else by the harness."""
    cs = CaseStruct()
    cs.kind = kind
    keep = [out]
    for k, v in kw.items():
        if k in _ARRAYS:
            if v is not None:
                assert v.dtype == _ARRAYS[k] and v.flags.c_contiguous, k
                keep.append(v)
                setattr(cs, k, v.ctypes.data_as(C.c_void_p))
        else:
            setattr(cs, k, v)
    if out is not None:
        cs.out = out.raw.ctypes.data_as(C.c_void_p) if isinstance(out, Guarded) else out
    cs._keep = keep
    return cs


# ---------------------------------------------------------------------------------------------------------------- layout

class Layout(object):
    def __init__(self, lens, pad=None):
        self.len = [int(l) for l in lens]
        self.start, r = [], 8
        for l in self.len:
            self.start.append(r)
            r = (r + l + 1 + 7) & ~7
        self.rows = r if pad is None else (r + pad - 1) // pad * pad
        self.ns = len(self.len)
        self.row_seq = np.full(self.rows, -1, np.int64)
        for s in range(self.ns):
            self.row_seq[self.start[s]:self.start[s] + self.len[s]] = s

    def live(self, hop=1):
        return np.repeat(self.row_seq >= 0, hop)

    def seq(self, s, hop=1):
        return slice(self.start[s] * hop, (self.start[s] + self.len[s]) * hop)


def layout(name):
    lens, pad = LAYOUTS[name]
    return Layout(lens, pad)


def rn16(v):
    return np.asarray(v, np.float32).astype(np.float16).astype(np.float32)


def leaky32(v):
    v = np.asarray(v, np.float32)
    return np.where(v > 0, v, np.float32(0.2) * v).astype(np.float32)


def leaky64(v):
    return np.where(v > 0, v, L02 * v)


def field(rng, lay, hop, ch, family):
    """[rows * hop][ch] f32 of the family, +0 on every guard position"""
    P = lay.rows * hop
    x = np.zeros((P, ch), np.float32)
    for s in range(lay.ns):
        sl = lay.seq(s, hop)
        n = sl.stop - sl.start
        g = rng.standard_normal((n, ch)).astype(np.float32)
        if family == "ramp":
            g = (((np.arange(n * ch) * 7) % 31 - 15) / 4.0).reshape(n, ch).astype(np.float32) * (1 if s % 2 == 0 else -1)
        elif family == "outlier":
            g[int(rng.integers(n)), int(rng.integers(ch))] = OUTLIER * (1 if s % 2 == 0 else -1)
        elif family == "straddle":
            g = g * np.float32(2.0 ** -6)
            z = rng.integers(0, 8, (n, ch))
            g[z == 0] = 0.0
            g[z == 1] = -0.0
        x[sl] = g
    return x


class Case(object):
    """One launch: kind, layout, parameters p, host arrays a (guards of the inputs +0), family"""

    def __init__(self, kind, lay, family, p, a, lname=""):
        self.kind, self.lay, self.family, self.p, self.a, self.lname = kind, lay, family, p, a, lname

    def name(self):
        return "%s %s %s %s" % (KIND_NAMES[self.kind], self.lname, self.family, " ".join("%s=%s" % kv for kv in sorted(self.p.items())))

    @property
    def hop_out(self):
        return self.p["hop"] * self.p.get("s", 1)


def make(kind, lname, family="gauss", seed=0, **p):
    lay = layout(lname) if isinstance(lname, str) else lname
    rng = np.random.default_rng([seed, kind, lay.rows] + [int(v) for _, v in sorted(p.items())])
    a = {}
    if kind == CONV:
        p = dict(dict(hop=1, dil=1, pre=0, post=0, reflect=0, resid=0), **p)
        p.setdefault("pad", p["dil"] * (p["K"] // 2))
        n = p["K"] * p["Cin"]
        a["x"] = field(rng, lay, p["hop"], p["Cin"], family)
        a["w"] = rn16(rng.standard_normal((p["K"], p["Cin"], p["Cout"])) / np.sqrt(n))
        a["bias"] = rng.standard_normal(p["Cout"]).astype(np.float32) * np.float32(0.5)
        if p["resid"]:
            a["resid"] = field(rng, lay, p["hop"], p["Cout"], "gauss")
    elif kind == CONVT:
        a["x"] = field(rng, lay, p["hop"], 32, family)
        a["w"] = (rng.standard_normal((2 * p["s"], 32, 32)) / 8.0).astype(np.float32)
        a["bias"] = rng.standard_normal(32).astype(np.float32) * np.float32(0.5)
    elif kind == DCONV:
        a["x"] = field(rng, lay, p["hop"], 32, family)
        a["w"] = rn16(rng.standard_normal((3, 32, 32)) / np.sqrt(96.0))
        a["bias"] = rng.standard_normal(32).astype(np.float32) * np.float32(0.5)
    elif kind == POST:
        p = dict(p, hop=256)
        a["x"] = field(rng, lay, 256, 32, family)
        a["w"] = rn16(rng.standard_normal((7, 32)) / 15.0)
        a["bias"] = rng.standard_normal(1).astype(np.float32)
    elif kind in (LVC_GATE, LVC_MFMA):
        hop, R = p["hop"], lay.rows
        a["x"] = field(rng, lay, hop, 32, "gauss" if family in ("gate", "gate0") else family)  # the dilated conv's output y
        a["xio"] = field(rng, lay, hop, 32, "gauss")
        a["xio"][~lay.live(hop)] = np.float32(7.25)  # guard positions of x: the LVC kernels must leave them as they are
        W = (rng.standard_normal((R, 6144)) / np.sqrt(96.0)).astype(np.float32)  # reference order (i*64 + ch)*3 + tap
        kb = rng.standard_normal((R, 64)).astype(np.float32)
        if family in ("gate", "gate0"):
            if family == "gate0":
                a["xio"][lay.live(hop)] = 0  # the output is gate_dev(a, b) itself, no final rounding: what the report's gate_dev lines measure
            W[:] = 0
            ng = len(GATE_GRID)
            idx = (np.cumsum(lay.row_seq >= 0)[:, None] * 32 + np.arange(32)[None, :]) % (ng * ng)
            kb[:, :32], kb[:, 32:] = GATE_GRID[idx // ng], GATE_GRID[idx % ng]
        if family == "outlier":
            W = W * np.float32(1e-3)  # keeps |a|, |b| around 30 under the 3e4 outlier instead of saturating both halves
        a["W"], a["kbl"] = W, kb
    elif kind == MEL_ROWS:
        a["x"] = np.concatenate([np.clip(field(rng, Layout((l - 10,)), 1, 100, family)[8:8 + l - 10].T / 3.0, -1, 1).ravel() for l in lay.len]).astype(np.float32)
    elif kind == NOISE_ROWS:
        a["x"] = np.concatenate([field(rng, Layout((l,)), 1, 64, family)[8:8 + l].T.ravel() for l in lay.len]).astype(np.float32)
    elif kind == COND_F16:
        a["x"] = field(rng, lay, 1, 64, family)
        a["x"][~lay.live()] = np.float32(3.5)  # the kernel writes zero guard rows whatever the input holds
    return Case(kind, lay, family, p, a, lname if isinstance(lname, str) else "")


def poisoned(c):
    """The same case with NaN on every guard position of its position-indexed inputs (kernels that check bounds themselves must not notice)"""
    a = dict(c.a)
    for k in ("x", "resid"):
        if k in a and c.kind in (CONV, CONVT, LVC_GATE, POST):
            v = a[k].copy()
            v[~c.lay.live(len(v) // c.lay.rows)] = np.nan
            a[k] = v
    return Case(c.kind, c.lay, c.family + " poison", c.p, a, c.lname)


def alone(c, s):
    """Candidate s of case c as a case of its own (layout (len[s],), start 8)"""
    lay = Layout((c.lay.len[s],))
    a = {}
    for k, v in c.a.items():
        if c.kind in (MEL_ROWS, NOISE_ROWS):
            per = [(100 * (l - 10)) if c.kind == MEL_ROWS else 64 * l for l in c.lay.len]
            o = int(np.sum(per[:s]))
            a[k] = v[o:o + per[s]].copy()
        elif k in ("w", "bias"):
            a[k] = v
        else:
            hop = len(v) // c.lay.rows
            n = np.zeros((lay.rows * hop,) + v.shape[1:], v.dtype)
            if k == "xio":
                n[:] = np.float32(7.25)
            if k == "x" and c.kind == COND_F16:
                n[:] = np.float32(3.5)
            n[lay.seq(0, hop)] = v[c.lay.seq(s, hop)]
            a[k] = n
    return Case(c.kind, lay, c.family, c.p, a, "alone")


def twin(c):
    """The same inputs for the other kernel of the same operation: lvc_mfma <-> lvc_gate, voc_dconv_mfma -> conv_direct (k3, pre- and post-leaky, pad = dil)"""
    if c.kind in (LVC_MFMA, LVC_GATE):
        return Case(LVC_GATE if c.kind == LVC_MFMA else LVC_MFMA, c.lay, c.family, c.p, c.a, c.lname)
    assert c.kind == DCONV
    p = dict(Cin=32, Cout=32, K=3, pre=1, post=1, hop=c.p["hop"], dil=c.p["dil"], pad=c.p["dil"], reflect=0, resid=0)
    return Case(CONV, c.lay, c.family, p, c.a, c.lname)


# ---------------------------------------------------------------------------------------------------------------- the sums

def _groups(c, mut=None):
    """The sum of a conv-like kernel as a list of (output index, X [n_out][Cin], W [Cin][Cout]); -> groups, output shape, terms per output"""
    lay, p, a, k = c.lay, c.p, c.a, c.kind
    out = []
    if k in (CONV, DCONV):
        hop, dil = p["hop"], p["dil"]
        K, pad, pre, reflect = (3, dil, 1, 0) if k == DCONV else (p["K"], p["pad"], p["pre"], p["reflect"])
        x, w = a["x"], a["w"]
        if mut == "tap_reversed":
            w = w[::-1]
        if mut in ("dil_plus", "dil_minus"):
            dil = dil + (1 if mut == "dil_plus" else -1)
        xl = leaky32(x) if pre else x
        xo = rn16(xl)
        if mut == "leaky_after_round":
            xo = leaky32(rn16(x)) if pre else xo
        if mut == "no_round":
            xo = xl
        for s in range(lay.ns):
            lo, n = lay.start[s] * hop, lay.len[s] * hop
            pos = np.arange(n)
            for t in range(K):
                q = pos + t * dil - pad
                if reflect:
                    if mut == "reflect_edge":
                        q = np.where(q < 0, -q - 1, q)
                        q = np.where(q >= n, 2 * n - 1 - q, q)
                    else:
                        q = np.abs(q)
                        q = np.where(q >= n, 2 * (n - 1) - q, q)
                ok = (q >= 0) & (q < n)
                if mut == "neighbour":
                    g = np.clip(lo + q, 0, len(xo) - 1)
                    out.append((lo + pos, xo[g], w[t]))
                else:
                    out.append((lo + pos[ok], xo[lo + q[ok]], w[t]))
        return out, (lay.rows * hop, w.shape[2]), K * w.shape[1]
    if k == POST:
        xo = rn16(a["x"] if mut == "post_no_leaky" else leaky32(a["x"]))
        w = a["w"]
        off = 0
        for s in range(lay.ns):
            n = lay.len[s] * 256 - 6
            for t in range(6 if mut == "post_6taps" else 7):
                out.append((off + np.arange(n), xo[lay.start[s] * 256 + t:lay.start[s] * 256 + t + n], w[t][:, None]))
            off += n
        return out, (off, 1), 7 * 32
    if k == CONVT:
        hop, s = p["hop"], p["s"]
        crop = s // 2 + (1 if mut == "crop_plus" else -1 if mut == "crop_minus" else 0)
        xl, w = leaky32(a["x"]), a["w"]
        for q in range(lay.ns):
            lo, n = lay.start[q] * hop, lay.len[q] * hop
            tl = np.arange(n * s)
            u = tl + crop
            t0, k0 = u // s, u % s
            for j in range(2):
                t, kk = t0 - j, k0 + (1 - j if mut == "taps_swapped" else j) * s
                ok = (t >= 0) & (t < n)
                for kv in range(2 * s):
                    m = ok & (kk == kv)
                    if m.any():
                        out.append((lo * s + tl[m], xl[lo + t[m]], w[kv]))
        return out, (lay.rows * hop * s, 32), 64
    # the location-variable convolution: 64 pre-activations per position
    hop = p["hop"]
    y = a["x"]
    for r in np.nonzero(lay.row_seq >= 0)[0]:
        rk = r + 1 if mut == "neighbour_frame" and lay.row_seq[r + 1] >= 0 else r
        Wr = a["W"][rk].reshape(64, 32, 3).transpose(1, 0, 2) if mut == "ich_transposed" else a["W"][rk].reshape(32, 64, 3)
        sl = lay.seq(int(lay.row_seq[r]), hop)
        pos = np.arange(r * hop, (r + 1) * hop)
        for t in range(3):
            q = pos + t - (0 if mut == "window_shift" else 1)
            ok = (q >= sl.start) & (q < sl.stop)
            out.append((pos[ok], y[q[ok]], Wr[:, :, t]))
    return out, (lay.rows * hop, 64), 96


def _sum64(groups, shape):
    acc, asum = np.zeros(shape), np.zeros(shape)
    for idx, X, W in groups:
        X, W = X.astype(np.float64), W.astype(np.float64)
        acc[idx] += X @ W
        asum[idx] += np.abs(X) @ np.abs(W)
    return acc, asum


def _sum32(groups, shape, order, start=None):
    """float32, one rounding for every product and every addition, forward (order 0) or backward (order 1) over the taps and the input channels"""
    acc = np.zeros(shape, np.float32) if start is None else start.copy()
    gs = groups if order == 0 else groups[::-1]
    with np.errstate(over="ignore", invalid="ignore"):
        for idx, X, W in gs:
            cur = acc[idx]
            cis = range(X.shape[1]) if order == 0 else range(X.shape[1] - 1, -1, -1)
            for ci in cis:
                cur = cur + X[:, ci, None] * W[ci][None, :]
            acc[idx] = cur
    return acc


def gate64(a, b):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-a)) * np.tanh(b)


def gate_bound(a, b, Da, Db, xg):
    """the bound of x + gate_dev(a, b) (module docstring), xg = the exact sum"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(over="ignore"):
        sg, th = 1.0 / (1.0 + np.exp(-a)), np.tanh(b)
    rel_sg = (1 - sg) * (2 * U * np.abs(a) + 2 * U) + 3 * U
    abs_th = (1 - th) * ((4 * U * np.abs(b) + 2 * U) * (1 + th) / 2 + 3 * U) + U * np.abs(th)
    dev = np.abs(th) * sg * rel_sg + sg * abs_th + U * np.abs(sg * th) + 4 * FMIN
    return Da / 4 + Db + dev + U * np.abs(xg)


def gate32(a, b, th_off=None):
    """gate_dev restated: exact exp2 and reciprocal, each rounded to f32"""
    f = np.float32
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        ea = np.exp2((a * f(-1.44269504088896)).astype(np.float64)).astype(f)
        sg = (1.0 / (f(1) + ea).astype(np.float64)).astype(f)
        eb = np.exp2((b * f(2.88539008177793)).astype(np.float64)).astype(f)
        th = f(1) - f(2) * (1.0 / (f(1) + eb).astype(np.float64)).astype(f)
    if th_off is not None:
        th = th + th_off
    return sg * th


# ---------------------------------------------------------------------------------------------------------------- reference, bound, restatement

def reference(c, mut=None):
    """-> dict(z float64 output, bound, live mask of output positions [P], exact = the output must equal z bit for bit)"""
    k, lay, p, a = c.kind, c.lay, c.p, c.a
    if k == MEL_ROWS:
        z, bound, off = np.zeros((lay.rows, 100)), np.zeros((lay.rows, 100)), 0
        d = float(np.float32(MAXV - MINV))
        for s in range(lay.ns):
            T = lay.len[s] - 10
            m = a["x"][off:off + 100 * T].reshape(100, T).T.astype(np.float64)
            z[lay.start[s]:lay.start[s] + T] = (m + 1) / 2 * d + float(MINV)
            bound[lay.start[s]:lay.start[s] + T] = 4 * U * (np.abs(m + 1) / 2 * d + abs(float(MINV)))
            z[lay.start[s] + T:lay.start[s] + T + 10] = float(PADV)
            off += 100 * T
        return dict(z=z, bound=bound, live=lay.live())
    if k == NOISE_ROWS:
        z, off = np.zeros((lay.rows, 64)), 0
        for s in range(lay.ns):
            z[lay.start[s]:lay.start[s] + lay.len[s]] = a["x"][off:off + 64 * lay.len[s]].reshape(64, lay.len[s]).T
            off += 64 * lay.len[s]
        return dict(z=z, bound=np.zeros_like(z), live=lay.live())
    if k == COND_F16:
        z = np.where(lay.live()[:, None], a["x"].astype(np.float16).astype(np.float64), 0.0)
        return dict(z=z, bound=np.zeros_like(z), live=lay.live())
    groups, shape, n = _groups(c, mut)
    acc, asum = _sum64(groups, shape)
    cc = C_AFTER[k]
    if k in (LVC_GATE, LVC_MFMA):
        hop, layer = p["hop"], p["layer"]
        live = lay.live(hop)
        kb = np.repeat(a["kbl"].astype(np.float64), hop, axis=0)
        pre = acc + kb
        D = (n + cc) * U * (asum + np.abs(kb))
        lo, hi = pre[:, :32], pre[:, 32:]
        if mut == "halves_swapped":
            lo, hi = hi, lo
        g = gate64(lo, hi)
        if mut == "gate_1e-5":
            g = g + 1e-5 * (np.abs(hi) < 1e-3) / (1.0 + np.exp(-lo))
        x0 = a["xio"].astype(np.float64)
        z = np.where(live[:, None], x0 + g, x0)
        bound = np.where(live[:, None], gate_bound(lo, hi, D[:, :32], D[:, 32:], z), 0.0)
        return dict(z=z, bound=bound, live=live)
    if k == POST:
        z = acc + float(a["bias"][0])
        return dict(z=z[:, 0], bound=((n + cc) * U * (asum + abs(float(a["bias"][0]))))[:, 0], live=np.ones(shape[0], bool))
    live = lay.live(c.hop_out)
    bias = a["bias"].astype(np.float64)[None, :] * (0 if mut == "no_bias" else 1)
    resid = a["resid"].astype(np.float64) if "resid" in a else 0.0
    v = acc + bias
    if mut == "resid_before_leaky":
        v = v + resid
    if (k == DCONV or (k == CONV and p["post"])) and mut != "no_post_leaky":
        v = leaky64(v)
    if mut != "resid_before_leaky":
        v = v + resid
    z = np.where(live[:, None], v, 0.0)
    bound = np.where(live[:, None], (n + cc) * U * (asum + np.abs(a["bias"].astype(np.float64))[None, :] + np.abs(resid)), 0.0)
    return dict(z=z, bound=bound, live=live)


def restate32(c, order):
    """A float32 restatement of the kernel of case c that sums forward (order 0) or backward (order 1); -> the output as the kernel's dtype"""
    k, lay, p, a = c.kind, c.lay, c.p, c.a
    f = np.float32
    if k == MEL_ROWS:
        out = np.zeros((lay.rows, 100), f)
        off = 0
        for s in range(lay.ns):
            T = lay.len[s] - 10
            mm = a["x"][off:off + 100 * T].reshape(100, T).T
            out[lay.start[s]:lay.start[s] + T] = ((mm + f(1)) / f(2)) * f(MAXV - MINV) + MINV if order == 0 else \
                (((mm + f(1)) / f(2)).astype(np.float64) * float(f(MAXV - MINV)) + float(MINV)).astype(f)  # order 1: the contracted multiply-add
            out[lay.start[s] + T:lay.start[s] + T + 10] = PADV
            off += 100 * T
        return out
    if k in (NOISE_ROWS, COND_F16):
        z = reference(c)["z"]
        return z.astype(np.float16) if k == COND_F16 else z.astype(f)
    groups, shape, n = _groups(c)
    if k == CONVT:
        start = np.zeros(shape, f) + a["bias"][None, :]  # the bias is the accumulator's first value
        return np.where(lay.live(c.hop_out)[:, None], _sum32(groups, shape, order, start), f(0))
    acc = _sum32(groups, shape, order)
    if k in (LVC_GATE, LVC_MFMA):
        hop = p["hop"]
        live = lay.live(hop)
        pre = acc + np.repeat(a["kbl"], hop, axis=0)
        return np.where(live[:, None], a["xio"] + gate32(pre[:, :32], pre[:, 32:]), a["xio"]).astype(f)
    if k == POST:
        return (acc + a["bias"][0])[:, 0]
    v = acc + a["bias"][None, :]
    if k == DCONV or p["post"]:
        v = leaky32(v)
    if "resid" in a:
        v = a["resid"] + v
    return np.where(lay.live(c.hop_out)[:, None], v, f(0)).astype(f)


def judge(out, ref):
    """-> (number of rejected elements, largest |err| / bound over the elements with a non-zero bound). NaN is rejected; a zero bound asks for equality."""
    o = np.asarray(out).astype(np.float64)
    z, b = ref["z"], ref["bound"]
    with np.errstate(invalid="ignore"):
        err = np.abs(o - z)
        bad = ~(err <= b)
        r = np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)
    return int(bad.sum()), float(np.nanmax(r)) if r.size else 0.0


def guards_ok(c, out, ref):
    """every guard position of a producer's output holds bit pattern +0 (not -0, not the sentinel); no live element still holds the sentinel.
    LVC kernels: guard positions of x keep their bits."""
    o = np.ascontiguousarray(out)
    bits = o.view(np.uint16 if o.dtype == np.float16 else np.uint32)
    live = ref["live"]
    sent = SENTINEL * (0x0101 if o.dtype == np.float16 else 0x01010101)
    if c.kind in (LVC_GATE, LVC_MFMA):
        return bool((bits[~live] == c.a["xio"].view(np.uint32)[~live]).all())
    if c.kind == POST:
        return bool((bits != sent).all())
    return bool((bits[~live] == 0).all() and (bits[live] != sent).all())


# ---------------------------------------------------------------------------------------------------------------- the runner

def out_shape(c):
    k, lay, p = c.kind, c.lay, c.p
    if k == CONV:
        return (lay.rows * p["hop"], p["Cout"]), np.float32
    if k == CONVT:
        return (lay.rows * p["hop"] * p["s"], 32), np.float32
    if k in (LVC_GATE, LVC_MFMA, DCONV):
        return (lay.rows * p["hop"], 32), np.float32
    if k == POST:
        return (sum(l * 256 - 6 for l in lay.len),), np.float32
    return (lay.rows, {MEL_ROWS: 100, NOISE_ROWS: 64, COND_F16: 64}[k]), (np.float16 if k == COND_F16 else np.float32)


def to_struct(c, out=None):
    k, lay, p, a = c.kind, c.lay, c.p, c.a
    kw = dict(ns=lay.ns, rows=lay.rows, start=np.array(lay.start, np.int32), len=np.array(lay.len, np.int32), x=a["x"], hop=p.get("hop", 1))
    if k == CONV:
        kw.update(w=a["w"], bias=a["bias"], resid=a.get("resid"), Cin=p["Cin"], Cout=p["Cout"], K=p["K"], dil=p["dil"], pad=p["pad"], pre_leaky=p["pre"],
                  post_leaky=p["post"], reflect=p["reflect"])
    elif k == CONVT:
        kw.update(w=a["w"], bias=a["bias"], s=p["s"])
    elif k == DCONV:
        kw.update(w=a["w"], bias=a["bias"], dil=p["dil"])
    elif k == POST:
        kw.update(w=a["w"], bias=a["bias"])
    elif k in (LVC_GATE, LVC_MFMA):
        layer, R = p["layer"], lay.rows
        kern = np.full((R, 4, 6144), np.nan, np.float32)  # layers the launch does not name: NaN
        kern[:, layer, lvc_perm()] = a["W"]
        kb = np.full((R, 4, 64), np.nan, np.float32)
        kb[:, layer] = a["kbl"]
        kw.update(kern=kern.reshape(R, 24576), kb=kb.reshape(R, 256), xio=a["xio"], layer=layer)
    return struct(k, out=out, **kw)


class HipError(RuntimeError):
    """a HIP call of the harness failed: nothing more is launched in this session (test_voc_kernels_gpu.py ends it)"""


def run(c):
    """Launch case c once. -> Guarded (canaries asserted by the caller)"""
    shape, dt = out_shape(c)
    out = Guarded(shape, dt)
    rc = harness().tts_voc_test_run(C.byref(to_struct(c, out)))
    if rc != 0:
        raise HipError("%s: HIP error %d" % (c.name(), rc))
    return out


def run_philox(n, seed, stream):
    out = Guarded((n,), np.float32)
    rc = harness().tts_voc_test_run(C.byref(struct(PHILOX, out=out, n=n, seed=seed, stream=stream)))
    if rc != 0:
        raise HipError("voc_philox_kernel: HIP error %d" % rc)
    return out


# ---------------------------------------------------------------------------------------------------------------- the case matrix

def conv_shapes():
    """every shape voc_run launches conv_direct_kernel with"""
    yield dict(Cin=64, Cout=32, K=7, reflect=1)                      # conv_pre
    yield dict(Cin=100, Cout=64, K=5, post=1)                        # kernel predictor input_conv
    yield dict(Cin=64, Cout=64, K=3, post=1)                         # residual_convs, first
    yield dict(Cin=64, Cout=64, K=3, post=1, resid=1)                # residual_convs, second
    for d in (1, 3, 9, 27):                                          # conv_blocks at hop 8 (dil 27 reaches past layout B's single guard frame)
        yield dict(Cin=32, Cout=32, K=3, pre=1, post=1, hop=8, dil=d)


def matrix(kind):
    """(layout name, family, parameters) of every case of a kernel"""
    if kind == CONV:
        return [(l, f, p) for p in conv_shapes() for l, f in (("A", "gauss"), ("B", "ramp"), ("B", "straddle"), ("C", "outlier"), ("D", "gauss"))]
    if kind == CONVT:
        return [(l, f, dict(hop=h, s=s)) for h, s in ((1, 8), (8, 8), (64, 4)) for l, f in (("A", "straddle"), ("B", "gauss"), ("C", "outlier"), ("D", "ramp"))]
    if kind == LVC_GATE:
        fams = (("A", "gate"), ("B", "gauss"), ("C", "outlier"), ("B", "ramp"), ("D", "straddle"))
        return [(l, f, dict(hop=h, layer=(i + j) % 4)) for i, h in enumerate((8, 64, 256)) for j, (l, f) in enumerate(fams)]
    if kind == LVC_MFMA:
        fams = (("A", "gate"), ("B", "gauss"), ("C", "outlier"), ("D", "straddle"))
        return [(l, f, dict(hop=h, layer=ly)) for h in (64, 256) for ly, (l, f) in enumerate(fams)] + \
               [("B", "ramp", dict(hop=64, layer=ly)) for ly in range(4)] + [("A", "gate", dict(hop=256, layer=3)), ("B", "gate", dict(hop=64, layer=2))]
    if kind == DCONV:
        fams = (("B", "gauss"), ("A", "straddle"), ("C", "outlier"), ("D", "ramp"))
        return [fams[(i + j) % 4] + (dict(hop=h, dil=d),) for i, h in enumerate((64, 256)) for j, d in enumerate((1, 3, 9, 27))] + \
               [("B", f, dict(hop=64, dil=27)) for f in ("straddle", "outlier", "ramp")]
    if kind == POST:
        return [("A", "gauss", {}), ("B", "straddle", {}), ("C", "outlier", {}), ("B", "ramp", {})]
    return [("A", "gauss", {}), ("B", "ramp", {}), ("C", "outlier", {}), ("D", "straddle", {})]


def cases(kind):
    return [make(kind, l, f, **p) for l, f, p in matrix(kind)]


# ---------------------------------------------------------------------------------------------------------------- Philox4x32-10

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays, key: 2 uint32 arrays (broadcast) -> 4 uint32 arrays. The round function of Salmon, Moraes, Dror, Shaw (SC'11), 10 rounds."""
    c = [np.asarray(v, np.uint64) for v in ctr]
    k = [np.asarray(v, np.uint64) for v in key]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return [v.astype(np.uint32) for v in c]


def philox4x32_10_int(ctr, key):
    """the same on Python ints, written on its own"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        a, b = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((b >> 32) ^ c1 ^ k0) & 0xFFFFFFFF, b & 0xFFFFFFFF, ((a >> 32) ^ c3 ^ k1) & 0xFFFFFFFF, a & 0xFFFFFFFF
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_reference(n, seed, stream):
    """voc_philox_kernel: -> (float64 reference [n], bound [n])"""
    i = np.arange(n, dtype=np.uint64)
    r = philox4x32_10([i >> np.uint64(1), 0x766f63, stream, 0x7716], [seed & 0xFFFFFFFF, seed >> 32])
    f = np.float32
    u1 = (r[0].astype(f) + f(1)) * f(2.0 ** -32)   # float32, as the kernel
    u2 = r[1].astype(f) * f(2.0 ** -32)
    with np.errstate(divide="ignore"):
        rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    theta = 2.0 * np.pi * u2.astype(np.float64)
    x = np.where(np.arange(n) & 1, rad * np.sin(theta), rad * np.cos(theta))
    return x, rad * (2 * U * theta + 4 * U) + 5 * U * np.abs(x)
