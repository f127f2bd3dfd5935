"""Shared by tests/test_hfg_kernels_gpu.py and tests/test_hfg_harness_cpu.py: the ctypes view of the test-only harness library
(tortoise.cpp_amd/testlib/hfg_harness.hip -> libtts_hfg_test.so), float64 NumPy references of the HiFi-GAN decoder's kernels (csrc/hifigan.hip), the case matrix,
the acceptance rule and its error bound, float32 restatements that sum in two orders, and the defects the rule must reject.

The references share no code with the harness or the kernels; test_hfg_harness_cpu.py checks them against torch.nn.functional in float64.

LAYOUTS, as hifigan_run builds them (start = the running sum of ceil8(W); activations are [frames * R][channels] at R rows per frame):
  A (4,) on 8 frames: shorter than every tap reach.   B (9, 4) on 16 + 8 frames: the candidates touch with only B's 7 padding rows between them.
  C (13, 1, 20) on 48 frames, two voices, voice_of (1, 0, 1): the grid is sized by the longest candidate, the short one's workgroups exit early.
  D chunk windows: (W 12, L 20, w0 30, keep0 5, keep_n 4) and (W 9, L 3, w0 2, keep0 3, keep_n 2), two voices.
  I whole utterances of L = 1, 2, 3 rows (T = 4, 8, 13 = tts_diffusion_frames(L)); J three windows of an L = 500 utterance (T = 2176): its first 12 frames, its
  last 12, and 9 in the middle. The input rows that belong to no candidate hold 3.5 (NaN in the poisoned twin), the rows of `out0` / `resid` there the sentinel.

REFERENCES are float64 on the values the kernel multiplies. Convolutions: the operand path is restated bit for bit, v < 0 ? float32(v) * float32(slope) : v in
float32; then the sum over channels and taps and the epilogue in float64. A transposed convolution is held in PyTorch's layout [cin][cout][2u] and evaluated by
the definition y[i u + k - u/2] += x[i] W[:, :, k]; repack_convt() turns that layout into the kernel's [phase][2][cin][cout] from the same definition.

ACCEPTANCE, first order and term by term, nothing fitted; u = 2^-24. A sum of n = taps x cin products in ANY order puts at most 2n roundings on a partial sum that
is at most sum |terms| (the product's own rounding counted for every term: whether v_mfma_f32_32x32x2_f32 rounds the product before the add is not documented;
if it is fused the achieved ratio is simply lower), and the epilogue adds c more:
      bound = (2n + c) u (sum |terms| + |bias| + |cbias| + |resid| + |out_prev|) + n 2^-126
c = 1 (acc + bias) + 1 with cbias (bias + cbias) + 1 with resid + 1 for acc_mode 1, 2 (+ out) + 1 for acc_mode 2 (/ 3). n 2^-126: a flush of subnormal products
or partial sums to zero (unmeasured for the f32 MFMA). hfg_cond_kernel: n = 1024, c = 1. hfg_post_kernel: n = 224, c = 1 on the pre-activation, carried through
|tanh'| <= 1, plus device tanhf: 2 ulp = 4u |tanh| (the HIP math API reference's table of maximum ulp errors of the single-precision device functions, which OCML
implements: the source of voc_cases.py's logf / sincosf figures) and one smallest normal.
hfg_interp_kernel: the output is continuous and piecewise linear in the source position, so a position error d moves it by at most d x the largest difference of
neighbouring samples. The level-2 position fl(fl((t + 0.5) fl(0.91875)) - 0.5) carries the constant's, the product's and the subtraction's rounding (a contracted
multiply-add removes one): d2 <= 3u (t + 0.5) 0.91875. The level-1 position (i + 0.5) 0.25 - 0.5 is exact in f32; it is given the same allowance 3u (i + 0.5) 0.25.
Each of the two lerps (1 - l) p + l q rounds 1 - l, both products and the sum: 4u max(|p|, |q|).
      bound = d2 D2 + max E1 + 4u max |y1|,  E1 = d1 D1 + 4u max |lat|      (D: largest neighbouring difference around the source index, per channel)
For L = 1 every difference is 0 and a frame must equal the row to within the 8u |row| of the value roundings alone.

EXACT FAMILY: integer activations in [-4, 4], weights in [-2, 2], bias / cbias / resid / out_prev small integers, slope 1 or 0.5: every product and every partial
sum is a multiple of 1/2 below 2^23 (asserted), so every order of summation gives the float64 sum and the output must equal it BIT FOR BIT (acc_mode 2 divides
by 3 last: one correctly rounded f32 division of an exact value).

DEFECTS are applied to the reference (reference(mut=...)); test_hfg_harness_cpu.py requires each to leave the bound of the unmutated reference on some case."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tortoise.cpp_amd")
LIB = os.environ.get("TTS_HFG_TEST_LIB") or os.path.join(PKG, "libtts_hfg_test.so")
SRC = os.path.join(PKG, "testlib", "hfg_harness.hip")

CONV, CONV_SMALL, INTERP, COND, POST = range(5)
KIND_NAMES = ["hfg_conv_kernel", "hfg_conv_small_kernel", "hfg_interp_kernel", "hfg_cond_kernel", "hfg_post_kernel"]
SENTINEL = 0xCB
SENT32 = np.uint32(0xCBCBCBCB)
HIP_INVALID_VALUE = 1
U = 2.0 ** -24
FMIN = 2.0 ** -126
TANH_ULP = 2.0   # device tanhf, in ulp (module docstring)
OUTLIER = 1.0e4
JUNK = np.float32(3.5)
LAT, C0 = 1024, 512
UP = (8, 8, 2, 2)
RES_K, RES_D = (3, 7, 11), (1, 3, 5)
S2 = 22050.0 / 24000.0
f32 = np.float32


class CaseStruct(C.Structure):
    _fields_ = [("kind", C.c_int), ("ns", C.c_int), ("frames", C.c_int), ("n_voices", C.c_int),
                ("cin", C.c_int), ("cout", C.c_int), ("taps", C.c_int), ("dil", C.c_int), ("phases", C.c_int), ("rate", C.c_int), ("acc_mode", C.c_int),
                ("alias", C.c_int), ("slope", C.c_float),
                ("cand", C.c_void_p), ("start", C.c_void_p),
                ("in_", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("cbias", C.c_void_p), ("resid", C.c_void_p), ("out0", C.c_void_p),
                ("out", C.c_void_p)]


_lib = None


def harness():
    """The harness library; built once with make if it is missing. A missing library is an error, never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", PKG, "libtts_hfg_test.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        if not os.path.exists(LIB):
            raise RuntimeError("libtts_hfg_test.so is not built and `make` did not produce it")
        L = C.CDLL(LIB)
        L.tts_hfg_test_run.argtypes = [C.POINTER(CaseStruct)]
        L.tts_hfg_test_validate.argtypes = [C.POINTER(CaseStruct)]
        L.tts_hfg_test_table.argtypes = [C.POINTER(CaseStruct), C.c_void_p]
        L.tts_hfg_test_frames.argtypes = [C.c_int]
        L.tts_hfg_test_lds_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.tts_hfg_test_lds_bytes.restype = C.c_longlong
        for f in (L.tts_hfg_test_run, L.tts_hfg_test_validate, L.tts_hfg_test_table, L.tts_hfg_test_margin, L.tts_hfg_test_seq_ints, L.tts_hfg_test_frames):
            f.restype = C.c_int
        _lib = L
    return _lib


class Guarded(object):
    """A host buffer margin | payload | margin the harness copies a device allocation into."""

    def __init__(self, shape, dtype=np.float32):
        self.margin = harness().tts_hfg_test_margin()
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.raw = np.zeros(2 * self.margin + int(np.prod(shape)) * self.dtype.itemsize, np.uint8)

    @property
    def payload(self):
        return self.raw[self.margin:len(self.raw) - self.margin].view(self.dtype).reshape(self.shape)

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == SENTINEL).all() and (self.raw[len(self.raw) - self.margin:] == SENTINEL).all())


_ARRAYS = dict(cand=np.int32, start=np.int32, in_=np.float32, w=np.float32, bias=np.float32, cbias=np.float32, resid=np.float32, out0=np.float32)


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

def ceil8(v):
    return (v + 7) // 8 * 8


class Layout(object):
    """cand: (W, voice, L, w0, keep0, keep_n) per candidate; the table is hifigan_run's: start = running sum of ceil8(W)"""

    def __init__(self, cand, n_voices=1, frames=None):
        self.cand = [tuple(int(v) for v in c) for c in cand]
        self.ns, self.n_voices = len(self.cand), n_voices
        self.W = [c[0] for c in self.cand]
        self.voice = [c[1] for c in self.cand]
        self.L = [c[2] for c in self.cand]
        self.w0 = [c[3] for c in self.cand]
        self.keep0 = [c[4] for c in self.cand]
        self.keep_n = [c[5] for c in self.cand]
        self.start, r = [], 0
        for w in self.W:
            self.start.append(r)
            r += ceil8(w)
        self.frames = r if frames is None else frames
        self.lat0 = [int(v) for v in np.cumsum([0] + self.L[:-1])]
        self.before = [int(v) for v in np.cumsum([0] + self.keep_n[:-1])]

    def live(self, R=1):
        m = np.zeros(self.frames * R, bool)
        for s in range(self.ns):
            m[self.rows(s, R)] = True
        return m

    def rows(self, s, R=1):
        return slice(self.start[s] * R, (self.start[s] + self.W[s]) * R)

    def table(self):
        return np.array([[self.start[s], self.W[s], self.voice[s], self.L[s], self.lat0[s], self.before[s], self.w0[s], self.keep0[s], self.keep_n[s]]
                         for s in range(self.ns)], np.int32)

    def one(self, s):
        """candidate s as a layout of its own (its voice index kept: the voice table is shared)"""
        return Layout([self.cand[s]], self.n_voices)


def frames_of(L):
    """T of an utterance of L latent rows (tts_diffusion_frames; the CPU test holds it to the harness's export)"""
    return L * 4 * 24000 // 22050


def whole(T, voice=0, L=None):
    """a whole window of T frames; L defaults to the shortest utterance that has them"""
    if L is None:
        L = next(l for l in range(1, 501) if frames_of(l) >= T)
    return (T, voice, L, 0, 0, T)


T500 = frames_of(500)  # 2176
LAYOUTS = {
    "A": lambda: Layout([whole(4)]),
    "B": lambda: Layout([whole(9), whole(4)]),
    "C": lambda: Layout([whole(13, 1), whole(1, 0), whole(20, 1)], 2),
    "D": lambda: Layout([(12, 0, 20, 30, 5, 4), (9, 1, 3, 2, 3, 2)], 2),
    "I": lambda: Layout([whole(4, 0, 1), whole(8, 0, 2), whole(13, 0, 3)]),
    "J": lambda: Layout([(12, 0, 500, 0, 0, 12), (12, 0, 500, T500 - 12, 0, 12), (9, 0, 500, 1000, 0, 9)]),
    "V3": lambda: Layout([whole(4)], 3),
}


def layout(name):
    return LAYOUTS[name]()


def leaky32(v, slope):
    """the kernels' operand path, bit for bit: v < 0 ? v * slope : v in float32"""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, v * f32(slope), v).astype(f32)


def field(rng, lay, R, ch, family, amp=4):
    """[frames * R][ch] f32 of the family on the candidates' rows, JUNK on every other row"""
    x = np.full((lay.frames * R, ch), JUNK, f32)
    for s in range(lay.ns):
        sl = lay.rows(s, R)
        n = sl.stop - sl.start
        g = rng.standard_normal((n, ch)).astype(f32)
        if family == "ramp":
            g = (((np.arange(n * ch) * 7) % 31 - 15) / 4.0).reshape(n, ch).astype(f32) * (1 if s % 2 == 0 else -1)
        elif family == "outlier":
            g[int(rng.integers(n)), int(rng.integers(ch))] = OUTLIER * (1 if s % 2 == 0 else -1)
        elif family == "straddle":
            g = g * f32(2.0 ** -6)
            z = rng.integers(0, 8, (n, ch))
            g[z == 0] = 0.0
            g[z == 1] = -0.0
        elif family == "exact":
            g = rng.integers(-amp, amp + 1, (n, ch)).astype(f32)
        x[sl] = g
    return x


def sentinel_outside(x, lay, R):
    x.view(np.uint32)[~lay.live(R)] = SENT32
    return x


class Case(object):
    """One launch: kind, layout, parameters p, host arrays a, family"""

    def __init__(self, kind, lay, family, p, a, lname=""):
        self.kind, self.lay, self.family, self.p, self.a, self.lname = kind, lay, family, p, a, lname

    def name(self):
        return "%s %s %s %s" % (KIND_NAMES[self.kind], self.lname, self.family, " ".join("%s=%s" % kv for kv in sorted(self.p.items())))

    @property
    def R_out(self):
        return self.p["rate"] * self.p["phases"] if self.kind in (CONV, CONV_SMALL) else 1


CONV_DEFAULTS = dict(taps=3, dil=1, phases=1, rate=1, slope=0.1, acc=0, cbias=0, resid=0)  # resid: 0 none, 1 its own tensor, 2 resid == out


def make(kind, lname, family="gauss", seed=0, **p):
    lay = layout(lname) if isinstance(lname, str) else lname
    rng = np.random.default_rng([seed, kind, lay.frames] + [int(round(float(v) * 1000)) for _, v in sorted(p.items())])
    a = {}
    ex = family == "exact"
    if kind in (CONV, CONV_SMALL):
        p = dict(CONV_DEFAULTS, **p)
        cin, cout, taps, u, R = p["cin"], p["cout"], p["taps"], p["phases"], p["rate"]
        if u > 1:
            assert taps == 2
        n = taps * cin
        a["in_"] = field(rng, lay, R, cin, family)
        shape = (cin, cout, 2 * u) if u > 1 else (taps, cin, cout)  # a transposed convolution in PyTorch's layout
        a["w"] = rng.integers(-2, 3, shape).astype(f32) if ex else (rng.standard_normal(shape) / np.sqrt(n)).astype(f32)
        a["bias"] = rng.integers(-8, 9, cout).astype(f32) if ex else rng.standard_normal(cout).astype(f32) * f32(0.5)
        if p["cbias"]:
            a["cbias"] = rng.integers(-8, 9, (lay.n_voices, cout)).astype(f32) if ex else rng.standard_normal((lay.n_voices, cout)).astype(f32) * f32(0.5)
        if p["resid"] == 1:
            a["resid"] = sentinel_outside(field(rng, lay, R * u, cout, "exact" if ex else "gauss", 64), lay, R * u)
        if p["acc"] or p["resid"] == 2:
            a["out0"] = sentinel_outside(field(rng, lay, R * u, cout, "exact" if ex else "gauss", 64), lay, R * u)
    elif kind == INTERP:
        a["in_"] = field(rng, _LatLayout(lay), 1, LAT, family)
    elif kind == COND:
        a["in_"] = (rng.integers(-4, 5, (lay.n_voices, LAT)) if ex else rng.standard_normal((lay.n_voices, LAT))).astype(f32)
        if family == "outlier":
            a["in_"][:, 17] = OUTLIER
        if family == "straddle":
            a["in_"] *= f32(2.0 ** -6)
            a["in_"][:, ::4] = 0.0
            a["in_"][:, 1::8] = -0.0
        a["w"] = (rng.integers(-2, 3, (C0, LAT)) if ex else rng.standard_normal((C0, LAT)) / 32.0).astype(f32)
        a["bias"] = (rng.integers(-8, 9, C0) if ex else rng.standard_normal(C0) * 0.5).astype(f32)
    elif kind == POST:
        a["in_"] = field(rng, lay, 256, 32, family)
        a["w"] = (rng.integers(-2, 3, (7, 32)) if ex else rng.standard_normal((7, 32)) / 15.0).astype(f32)
        a["bias"] = (rng.standard_normal(1) * 0.3).astype(f32)
        if family == "tanh":  # the pre-activation IS one input element (weight 1 on the centre tap of channel 0, zero bias): the output is device tanhf of it
            a["w"][:] = 0
            a["w"][3, 0] = 1
            a["bias"][:] = 0
            for s in range(lay.ns):
                sl = lay.rows(s, 256)
                n = sl.stop - sl.start
                a["in_"][sl, 0] = (np.exp(rng.uniform(np.log(1e-6), np.log(12.0), n)) * np.where(rng.integers(0, 2, n), 1, 100)).astype(f32)  # >= 0: no leaky
    return Case(kind, lay, family, p, a, lname if isinstance(lname, str) else "")


class _LatLayout(object):
    """the latents of a layout as rows: candidate s owns [lat0, lat0 + L), nothing between"""

    def __init__(self, lay):
        self.ns, self.frames = lay.ns, int(sum(lay.L))
        self._lat0, self._L = lay.lat0, lay.L

    def rows(self, s, R=1):
        return slice(self._lat0[s], self._lat0[s] + self._L[s])


def poisoned(c):
    """The same case with NaN on every row of `in` (and of `resid`) outside the candidates' rows: these kernels check bounds themselves"""
    if c.kind not in (CONV, CONV_SMALL, POST):
        return None
    a = dict(c.a)
    R = c.p["rate"] if c.kind != POST else 256
    v = a["in_"].copy()
    v[~c.lay.live(R)] = np.nan
    a["in_"] = v
    if "resid" in a:
        v = a["resid"].copy()
        v[~c.lay.live(c.R_out)] = np.nan
        a["resid"] = v
    return Case(c.kind, c.lay, c.family + " poison", c.p, a, c.lname)


def alone(c, s):
    """Candidate s of case c as a case of its own"""
    lay = c.lay.one(s)
    a = {}
    for k, v in c.a.items():
        if k in ("w", "bias", "cbias") or c.kind == COND:
            a[k] = v
        elif c.kind == INTERP:
            a[k] = v[c.lay.lat0[s]:c.lay.lat0[s] + c.lay.L[s]].copy()
        else:
            R = len(v) // c.lay.frames
            n = np.full((lay.frames * R,) + v.shape[1:], JUNK, v.dtype)
            if k in ("resid", "out0"):
                n.view(np.uint32)[:] = SENT32
            n[lay.rows(0, R)] = v[c.lay.rows(s, R)]
            a[k] = n
    return Case(c.kind, lay, c.family, c.p, a, "alone")


def seq_out(c, o, s):
    """candidate s's part of the output o of case c"""
    if c.kind == POST:
        return o[c.lay.before[s] * 256:(c.lay.before[s] + c.lay.keep_n[s]) * 256]
    if c.kind == COND:
        return o
    return o[c.lay.rows(s, c.R_out)]


def twin(c):
    """The same inputs for the other convolution kernel"""
    assert c.kind in (CONV, CONV_SMALL)
    return Case(CONV_SMALL if c.kind == CONV else CONV, c.lay, c.family, c.p, c.a, c.lname)


def repack_convt(wt, u):
    """PyTorch ConvTranspose1d weight [cin][cout][2u] (stride u, padding u / 2) -> the kernel's [phase][2][cin][cout].
    From the definition y[i u + k - pad] += x[i] W[:, :, k]: output row o = q u + p receives k with k = p + pad (mod u), i.e. k0 = (p + pad) % u from input row
    i = q + (p + pad) // u and k0 + u from the row before it. The kernel's tap 0 is the earlier row, tap 1 the later one."""
    cin, cout, ku = wt.shape
    assert ku == 2 * u
    pad = u // 2
    out = np.zeros((u, 2, cin, cout), wt.dtype)
    for p in range(u):
        k0 = (p + pad) % u
        out[p, 0] = wt[:, :, k0 + u]
        out[p, 1] = wt[:, :, k0]
    return np.ascontiguousarray(out)


def repack_conv(w):
    """PyTorch Conv1d weight [cout][cin][k] -> the kernel's [k][cin][cout]"""
    return np.ascontiguousarray(np.transpose(w, (2, 1, 0)))


# ---------------------------------------------------------------------------------------------------------------- the sums

def _conv_groups(c, mut=None):
    """The sum of a convolution as a list of (output rows, X [n][cin] f32 operand, W [cin][cout]); -> groups, output shape, terms per output"""
    lay, p, a = c.lay, c.p, c.a
    cin, cout, taps, dil, u, R = p["cin"], p["cout"], p["taps"], p["dil"], p["phases"], p["rate"]
    slope = p["slope"]
    if mut == "slope_swap":
        slope = 0.01 if abs(slope - 0.1) < 1e-6 else 0.1
    x = a["in_"]
    if mut == "resid_before_leaky" and "resid" in a and u == 1 and cin == cout:
        with np.errstate(invalid="ignore", over="ignore"):
            x = (x + a["resid"]).astype(f32)
    xa = x if mut == "leaky_after" else leaky32(x, slope)
    if mut == "chunks_swapped" and cin == 64:
        xa = np.concatenate([xa[:, 32:], xa[:, :32]], axis=1)
    w = a["w"]
    out = []
    for s in range(lay.ns):
        r0, n = lay.start[s] * R, lay.W[s] * R
        t = np.arange(n)

        def add(rows_out, src, Wm):
            if mut == "neighbour":
                ok = (r0 + src >= 0) & (r0 + src < len(xa))
            else:
                ok = (src >= 0) & (src < n)
            out.append((rows_out[ok], xa[r0 + src[ok]], Wm))
        if u == 1:
            d = dil + (1 if mut == "dil_plus" else -1 if mut == "dil_minus" else 0)
            lo = -(dil * (taps - 1) // 2) + (1 if mut == "lo_plus" else -1 if mut == "lo_minus" else 0)
            ws = w[::-1] if mut == "tap_reversed" else w
            for j in range(taps):
                add(r0 + t, t + lo + j * d, ws[j])
        else:
            pad = u // 2
            for ph in range(u):
                pw = (ph + 1) % u if mut == "phase_next" else ph
                k0 = (pw + pad) % u
                sp = (ph + pad + (1 if mut == "pad_plus" else -1 if mut == "pad_minus" else 0)) // u
                ks = (k0, k0 + u) if mut != "taps_swapped" else (k0 + u, k0)
                add((r0 + t) * u + ph, t + sp, w[:, :, ks[0]])
                add((r0 + t) * u + ph, t + sp - 1, w[:, :, ks[1]])
    return out, (lay.frames * R * u, cout), taps * cin


def _post_groups(c, mut=None):
    lay, a = c.lay, c.a
    slope = 0.1 if mut == "slope_swap" else 1.0 if mut == "post_no_leaky" else 0.01
    xa = leaky32(a["in_"], slope)
    out = []
    for s in range(lay.ns):
        r0, n = lay.start[s] * 256, lay.W[s] * 256
        k0 = 0 if mut == "keep0_ignored" else lay.keep0[s]
        j = np.arange(lay.keep_n[s] * 256)
        for tap in range(6 if mut == "post_6taps" else 7):
            src = k0 * 256 + j + tap - 3
            ok = (src >= 0) & (src < n)
            out.append((lay.before[s] * 256 + j[ok], xa[r0 + src[ok]], c.a["w"][tap][:, None]))
    return out, (int(sum(lay.keep_n)) * 256, 1), 224


def _sum64(groups, shape, leaky_after=None):
    acc, asum = np.zeros(shape), np.zeros(shape)
    for idx, X, W in groups:
        X, W = X.astype(np.float64), W.astype(np.float64)
        if leaky_after is not None:  # the defect: the slope applied to the product
            P = X[:, :, None] * W[None]
            acc[idx] += np.where(P < 0, leaky_after * P, P).sum(1)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                acc[idx] += X @ W
        with np.errstate(invalid="ignore", over="ignore"):
            asum[idx] += np.abs(X) @ np.abs(W)
    return acc, asum


def _sum32(groups, shape, order, start=None):
    """float32, one rounding for every product and every addition, forward (order 0) or backward (order 1) over the taps and the input channels"""
    acc = np.zeros(shape, f32) if start is None else start.copy()
    gs = groups if order == 0 else groups[::-1]
    with np.errstate(over="ignore", invalid="ignore"):
        for idx, X, W in gs:
            cur = acc[idx]
            cis = range(X.shape[1]) if order == 0 else range(X.shape[1] - 1, -1, -1)
            for ci in cis:
                cur = cur + X[:, ci, None] * W[ci][None, :]
            acc[idx] = cur
    return acc


def conv_c(p):
    return 1 + (1 if p["cbias"] else 0) + (1 if p["resid"] else 0) + (1 if p["acc"] else 0) + (1 if p["acc"] == 2 else 0)


# ---------------------------------------------------------------------------------------------------------------- interpolation

def _lerp_idx(n_out, off, scale_inv, n_in, mut=None):
    """source indices and weight of F.interpolate(linear, align_corners=False) for destination indices off .. off + n_out"""
    d = off + np.arange(n_out, dtype=np.float64)
    s = np.maximum((d + 0.5) * scale_inv - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = i0 + 1 if mut == "no_upper_clamp" else np.minimum(i0 + 1, n_in - 1)
    return s, i0, i1, s - i0


def interp_ref(lat, L, w0, W, mut=None, after=None):
    """frames [w0, w0 + W) of the two-step interpolation of lat [L][1024]; -> z [W][1024], bound [W][1024]. `after` = the row that follows the candidate's latents in
    the buffer (what a missing clamp reads)."""
    lat = lat.astype(np.float64)
    T = L * 4 * 24000 // 22050
    if mut == "w0_ignored":
        w0 = 0
    if mut == "one_step":
        s, i0, i1, l = _lerp_idx(W, w0, 22050.0 / (4 * 24000.0), L)
        return (1 - l)[:, None] * lat[i0] + l[:, None] * lat[i1], None
    if mut == "align_corners":
        y1 = np.stack([np.interp(np.arange(4 * L) * ((L - 1) / max(4 * L - 1, 1)), np.arange(L), lat[:, ch]) for ch in range(0, lat.shape[1])], 1) if L > 1 else np.repeat(lat, 4, 0)
        pos = (w0 + np.arange(W)) * ((4 * L - 1) / max(T - 1, 1))
        i0 = np.minimum(np.floor(pos).astype(np.int64), 4 * L - 1)
        i1 = np.minimum(i0 + 1, 4 * L - 1)
        l = pos - i0
        return (1 - l)[:, None] * y1[i0] + l[:, None] * y1[i1], None
    ext = np.concatenate([lat, (after if after is not None else np.full((1, lat.shape[1]), float(JUNK))).astype(np.float64)])
    s1, a0, a1, la = _lerp_idx(4 * L, 0, 0.25, L, mut)
    y1 = (1 - la)[:, None] * ext[a0] + la[:, None] * ext[a1]
    s2, i0, i1, l2 = _lerp_idx(W, w0, S2, 4 * L)
    z = (1 - l2)[:, None] * y1[i0] + l2[:, None] * y1[i1]
    if mut is not None:
        return z, None
    # the bound (module docstring)
    def around(v, i, lo, hi):  # largest |v[j + 1] - v[j]| for j in {i - 1, i, i + 1}, and largest |v[j]| for j in {i - 1 .. i + 2}, indices clipped
        n = len(v)
        D = np.zeros((len(i), v.shape[1]))
        M = np.zeros((len(i), v.shape[1]))
        for k in range(lo, hi + 1):
            j = np.clip(i + k, 0, n - 1)
            M = np.maximum(M, np.abs(v[j]))
            if k < hi:
                D = np.maximum(D, np.abs(v[np.clip(i + k + 1, 0, n - 1)] - v[j]))
        return D, M
    D1, M1 = around(lat, a0, -1, 2)
    E1 = (3 * U * (np.arange(4 * L) + 0.5) * 0.25)[:, None] * D1 + 4 * U * M1
    D2, M2 = around(y1, i0, -1, 2)
    E1m = np.zeros_like(D2)
    for k in range(-1, 3):
        E1m = np.maximum(E1m, E1[np.clip(i0 + k, 0, 4 * L - 1)])
    bound = (3 * U * (w0 + np.arange(W) + 0.5) * S2)[:, None] * D2 + E1m + 4 * U * M2
    return z, bound


def interp32(lat, L, w0, W, fma):
    """hfg_interp_kernel restated in float32; fma: the source position contracted to one multiply-add"""
    t = (w0 + np.arange(W)).astype(f32)
    if fma:
        src2 = np.maximum(((t.astype(np.float64) + 0.5) * float(f32(0.91875)) - 0.5).astype(f32), f32(0))
    else:
        src2 = np.maximum((t + f32(0.5)) * f32(0.91875) - f32(0.5), f32(0))
    i0 = np.minimum(src2.astype(np.int64), 4 * L - 1)
    i1 = np.minimum(i0 + 1, 4 * L - 1)
    l2 = (src2 - i0.astype(f32))[:, None]

    def level1(i):
        sa = np.maximum((i.astype(f32) + f32(0.5)) * f32(0.25) - f32(0.5), f32(0))
        a0 = np.minimum(sa.astype(np.int64), L - 1)
        a1 = np.minimum(a0 + 1, L - 1)
        la = (sa - a0.astype(f32))[:, None]
        return (f32(1) - la) * lat[a0] + la * lat[a1]
    with np.errstate(over="ignore", invalid="ignore"):
        return ((f32(1) - l2) * level1(i0) + l2 * level1(i1)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------- reference, bound, restatement

def reference(c, mut=None):
    """-> dict(z float64 output, bound, live mask of output rows, exact = the output must equal z bit for bit)"""
    k, lay, p, a = c.kind, c.lay, c.p, c.a
    if k == INTERP:
        z, bound = np.zeros((lay.frames, LAT)), np.zeros((lay.frames, LAT))
        for s in range(lay.ns):
            lat = a["in_"][lay.lat0[s]:lay.lat0[s] + lay.L[s]]
            after = a["in_"][lay.lat0[s] + lay.L[s]:lay.lat0[s] + lay.L[s] + 1]
            zs, bs = interp_ref(lat, lay.L[s], lay.w0[s], lay.W[s], mut, after if len(after) else None)
            z[lay.rows(s)] = zs
            if bs is not None:
                bound[lay.rows(s)] = bs
        return dict(z=z, bound=bound, live=lay.live(), exact=False)
    if k == COND:
        g, w = a["in_"].astype(np.float64), a["w"].astype(np.float64)
        if mut == "cond_transposed":
            w = a["w"].reshape(LAT, C0).T.astype(np.float64)
        z = g @ w.T + a["bias"].astype(np.float64)[None, :]
        asum = np.abs(g) @ np.abs(w.T) + np.abs(a["bias"].astype(np.float64))[None, :]
        return dict(z=z, bound=(2 * LAT + 1) * U * asum + LAT * FMIN, live=np.ones(lay.n_voices, bool), exact=c.family == "exact", asum=asum)
    if k == POST:
        groups, shape, n = _post_groups(c, mut)
        acc, asum = _sum64(groups, shape)
        b = float(a["bias"][0])
        pre = (acc + b)[:, 0]
        z = np.tanh(pre)
        bound = (2 * n + 1) * U * (asum[:, 0] + abs(b)) + n * FMIN + TANH_ULP * 2 * U * np.abs(z) + FMIN
        return dict(z=z, bound=bound, live=np.ones(shape[0], bool), exact=False, pre=pre)
    groups, shape, n = _conv_groups(c, mut)
    acc, asum = _sum64(groups, shape, p["slope"] if mut == "leaky_after" else None)
    live = lay.live(c.R_out)
    row_voice = np.zeros(shape[0], np.int64)
    for s in range(lay.ns):
        row_voice[lay.rows(s, c.R_out)] = lay.voice[s] if mut != "cbias_other" else (lay.voice[s] + 1) % lay.n_voices
    bias = a["bias"].astype(np.float64)[None, :]
    cb = a["cbias"].astype(np.float64)[row_voice] if "cbias" in a else np.zeros(shape)
    prev = a["out0"].astype(np.float64) if "out0" in a else np.zeros(shape)
    resid = a["resid"].astype(np.float64) if p["resid"] == 1 else prev if p["resid"] == 2 else np.zeros(shape)
    v = acc + bias + (0 if mut == "cbias_none" else cb)
    if mut not in ("resid_none", "resid_before_leaky"):
        v = v + resid
    if p["acc"] == 1:
        v = prev + v
    elif p["acc"] == 2:
        v = v / 3 if mut == "acc2_forget" else (prev + v) / (2 if mut == "acc2_div2" else 3)
    mag = asum + np.abs(bias) + np.abs(cb) + np.abs(resid) + (np.abs(prev) if p["acc"] else 0)
    lv = live[:, None]
    with np.errstate(invalid="ignore"):
        z = np.where(lv, v, 0.0)
        bound = np.where(lv, (2 * n + conv_c(p)) * U * mag + n * FMIN, 0.0)
    return dict(z=z, bound=bound, live=live, exact=c.family == "exact", mag=np.where(lv, mag, 0.0))


def restate32(c, order):
    """A float32 restatement of the kernel of case c that sums forward (order 0) or backward (order 1); -> the output the kernel would leave in the buffer"""
    k, lay, p, a = c.kind, c.lay, c.p, c.a
    if k == INTERP:
        out = np.full((lay.frames, LAT), 0, f32)
        out.view(np.uint32)[:] = SENT32
        for s in range(lay.ns):
            out[lay.rows(s)] = interp32(a["in_"][lay.lat0[s]:lay.lat0[s] + lay.L[s]], lay.L[s], lay.w0[s], lay.W[s], order)
        return out
    if k == COND:
        ch = range(LAT) if order == 0 else range(LAT - 1, -1, -1)
        acc = np.zeros((lay.n_voices, C0), f32)
        for ci in ch:
            acc = acc + a["in_"][:, ci, None] * a["w"][None, :, ci]
        return acc + a["bias"][None, :]
    if k == POST:
        groups, shape, n = _post_groups(c)
        acc = _sum32(groups, shape, order, np.zeros(shape, f32) + a["bias"][0])
        return np.tanh(acc[:, 0].astype(np.float64)).astype(f32)
    groups, shape, n = _conv_groups(c)
    acc = _sum32(groups, shape, order)
    live = lay.live(c.R_out)
    bv = np.zeros(shape, f32) + a["bias"][None, :]
    if "cbias" in a:
        rv = np.zeros(shape[0], np.int64)
        for s in range(lay.ns):
            rv[lay.rows(s, c.R_out)] = lay.voice[s]
        bv = bv + a["cbias"][rv]
    with np.errstate(over="ignore", invalid="ignore"):
        v = acc + bv
        prev = a.get("out0")
        if p["resid"]:
            v = v + (a["resid"] if p["resid"] == 1 else prev)
        if p["acc"] == 1:
            v = v + prev
        elif p["acc"] == 2:
            v = (prev + v) / f32(3)
    out = np.zeros(shape, f32)
    out.view(np.uint32)[:] = SENT32
    if prev is not None:
        out[:] = prev
    out[live] = v[live]
    return out


def judge(out, ref):
    """-> (number of rejected elements, largest |err| / bound over the elements with a non-zero bound). NaN is rejected; a zero bound asks for equality.
    Only the live rows are judged here (the others must keep the bits they had: guards_ok)."""
    o = np.asarray(out).astype(np.float64)
    z, b, live = ref["z"], ref["bound"], ref["live"]
    o, z, b = o[live], z[live], b[live]
    with np.errstate(invalid="ignore"):
        err = np.abs(o - z)
        bad = ~(err <= b)
        r = np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)
    return int(bad.sum()), float(np.nanmax(r)) if r.size else 0.0


def exact_ok(out, ref):
    """the exact family: every live element equals the float64 reference, rounded once to f32, bit for bit"""
    live = ref["live"]
    want = ref["z"][live].astype(f32)
    got = np.ascontiguousarray(np.asarray(out)[live])
    return bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))


def exact_family_is_exact(c, ref):
    """every product and every partial sum of the case is a multiple of 1/2 of magnitude below 2^23: representable in f32 whatever the order"""
    m = ref["mag"] if "mag" in ref else ref["asum"]
    ok = float(m.max()) * 2 < 2.0 ** 24
    for k in ("in_", "w", "bias", "cbias", "resid", "out0"):
        if k in c.a:
            v = c.a[k]
            if k in ("resid", "out0"):
                v = v[c.lay.live(c.R_out)]
            elif k == "in_" and c.kind != COND:
                v = v[c.lay.live(c.p["rate"])]
            ok = ok and bool((2 * v == np.round(2 * v)).all())
    return ok and (c.kind == COND or c.p["slope"] in (1.0, 0.5))


def guards_ok(c, out):
    """no store leaves the candidates' live rows: every other row of the output buffer keeps the bits it started with (the 0xCB pattern); every live element is
    written. POST and COND write their whole output."""
    o = np.ascontiguousarray(out)
    bits = o.view(np.uint32)
    if c.kind in (POST, COND):
        return bool((bits != SENT32).all())
    live = c.lay.live(c.R_out)
    return bool((bits[~live] == SENT32).all() and (bits[live] != SENT32).all())


# ---------------------------------------------------------------------------------------------------------------- the runner

def out_shape(c):
    k, lay, p = c.kind, c.lay, c.p
    if k in (CONV, CONV_SMALL):
        return (lay.frames * p["rate"] * p["phases"], p["cout"])
    if k == INTERP:
        return (lay.frames, LAT)
    if k == COND:
        return (lay.n_voices, C0)
    return (int(sum(lay.keep_n)) * 256,)


def to_struct(c, out=None):
    k, lay, p, a = c.kind, c.lay, c.p, c.a
    kw = dict(ns=lay.ns, frames=lay.frames, n_voices=lay.n_voices, cand=np.ascontiguousarray(np.array(lay.cand, np.int32)), in_=a["in_"],
              w=a.get("w"), bias=a.get("bias"))
    if k in (CONV, CONV_SMALL):
        w = repack_convt(a["w"], p["phases"]) if p["phases"] > 1 else a["w"]
        kw.update(w=w, cbias=a.get("cbias"), resid=a.get("resid"), out0=a.get("out0"), cin=p["cin"], cout=p["cout"], taps=p["taps"], dil=p["dil"],
                  phases=p["phases"], rate=p["rate"], slope=float(p["slope"]), acc_mode=p["acc"], alias=1 if p["resid"] == 2 else 0)
    return struct(k, out=out, **kw)


class HipError(RuntimeError):
    """a HIP call of the harness failed: nothing more is launched in this session (test_hfg_kernels_gpu.py ends it)"""


def run(c):
    """Launch case c once. -> Guarded (canaries asserted by the caller)"""
    out = Guarded(out_shape(c))
    rc = harness().tts_hfg_test_run(C.byref(to_struct(c, out)))
    if rc != 0:
        raise HipError("%s: HIP error %d" % (c.name(), rc))
    return out


# ---------------------------------------------------------------------------------------------------------------- the case matrix

def product_convs():
    """every distinct (cin, cout, taps, dil, phases, rate, slope, acc_mode, cbias, resid) hifigan_run issues, in its order, with the layout it is run on here"""
    seen, out = set(), []

    def add(**p):
        key = tuple(sorted(p.items()))
        if key not in seen:
            seen.add(key)
            out.append(p)
    add(cin=LAT, cout=C0, taps=7, dil=1, phases=1, rate=1, slope=1.0, acc=0, cbias=1, resid=0)
    ch, rate = C0, 1
    for i in range(4):
        add(cin=ch, cout=ch // 2, taps=2, dil=1, phases=UP[i], rate=rate, slope=0.1, acc=0, cbias=0, resid=0)
        ch //= 2
        rate *= UP[i]
        for j in range(3):
            for n in range(3):
                add(cin=ch, cout=ch, taps=RES_K[j], dil=RES_D[n], phases=1, rate=rate, slope=0.1, acc=0, cbias=0, resid=0)
                # conv2: resid = u (n = 0: its own buffer), = x = out (n = 1: the alias), n = 2 writes m with the mean's acc_mode j
                add(cin=ch, cout=ch, taps=RES_K[j], dil=1, phases=1, rate=rate, slope=0.1, acc=j if n == 2 else 0, cbias=0, resid=2 if n == 1 else 1)
    return out


FAMS = ("gauss", "ramp", "outlier", "straddle", "exact")
LR = (("A", 64), ("B", 57), ("C", 59), ("C", 1), ("A", 1))  # Tin % 256 = 0 | 1 (513), 228 | 255 (767), 59, 156 | Tin < 32 | Tin = 4
SYN = ((32, 32), (64, 64), (64, 128))
SYN_SMALL = ((64, 128), (32, 256))


def _syn(shapes):
    out = []
    for si, (cin, cout) in enumerate(shapes):
        for ti, (taps, dil) in enumerate([(t, d) for t in (3, 7, 11) for d in (1, 3, 5)]):
            i = 9 * si + ti
            l, rate = LR[i % 5]
            fam = FAMS[(2 * i + si) % 5]
            slope = (1.0, 0.5)[i % 2] if fam == "exact" else (0.1, 1.0, 0.01)[i % 3]
            out.append((l, fam, dict(cin=cin, cout=cout, taps=taps, dil=dil, rate=rate, slope=slope, acc=(i // 2) % 3, cbias=i % 2, resid=(i // 3) % 3)))
    return out


def _exact(shapes):
    out = []
    for cin, cout in shapes:
        for acc in (0, 1, 2):
            out.append(("B", "exact", dict(cin=cin, cout=cout, taps=7, dil=3, rate=57, slope=(0.5, 1.0, 0.5)[acc], acc=acc, cbias=1, resid=(1, 2, 0)[acc])))
        out.append(("C", "exact", dict(cin=cin, cout=cout, taps=2, phases=8, rate=1, slope=0.5, cbias=1)))
        out.append(("B", "exact", dict(cin=cin, cout=cout, taps=2, phases=2, rate=57, slope=1.0)))
    return out


def _transposed(shapes):
    out = []
    for si, (cin, cout) in enumerate(shapes):
        for ui, u in enumerate((8, 2)):
            for li, (l, rate) in enumerate((("A", 1), ("B", 57), ("C", 8), ("C", 1))):
                out.append((l, FAMS[(si + ui + li) % 4], dict(cin=cin, cout=cout, taps=2, phases=u, rate=rate, slope=0.1)))
    return out


def _reach(shapes):
    """dilation 5 with 11 taps on layout B at one row per frame: the window reaches +-25 rows, past B's padding rows into the neighbouring candidate"""
    return [("B", f, dict(cin=cin, cout=cout, taps=11, dil=5, rate=1, slope=0.1, resid=1)) for cin, cout in shapes for f in ("gauss", "outlier")]


def _product(small):
    out = []
    for i, p in enumerate(product_convs()):
        if small and p["cout"] % 128:
            continue
        l = "A" if p["rate"] * p["phases"] >= 64 else "B"
        out.append((l, FAMS[i % 4], p))
    return out


def matrix(kind):
    """(layout name, family, parameters) of every case of a kernel"""
    if kind == CONV:
        return _syn(SYN) + _exact(SYN) + _transposed(((64, 32), (64, 64), (128, 128))) + _reach(SYN) + _product(False)
    if kind == CONV_SMALL:
        return _syn(SYN_SMALL) + _exact(SYN_SMALL) + _transposed(((64, 128), (32, 256))) + _reach(SYN_SMALL) + _product(True)
    if kind == INTERP:
        return [("I", "gauss", {}), ("I", "ramp", {}), ("I", "outlier", {}), ("I", "straddle", {}), ("J", "gauss", {}), ("J", "ramp", {}), ("J", "outlier", {}),
                ("D", "gauss", {}), ("D", "straddle", {})]
    if kind == COND:
        return [("A", "gauss", {}), ("V3", "gauss", {}), ("V3", "outlier", {}), ("V3", "straddle", {}), ("V3", "exact", {}), ("A", "ramp", {})]
    return [("A", "gauss", {}), ("B", "straddle", {}), ("C", "outlier", {}), ("B", "ramp", {}), ("D", "gauss", {}), ("D", "ramp", {}), ("C", "gauss", {}),
            ("B", "tanh", {})]


def cases(kind):
    return [make(kind, l, f, **p) for l, f, p in matrix(kind)]
