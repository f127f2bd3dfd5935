"""Shared by tests/test_afe_harness_cpu.py, tests/test_afe_kernels_gpu.py and tests/test_voice_audio_gpu.py: the binding of the test-only harness around the audio
front-end's kernels (tortoise.cpp_amd/testlib/afe_harness.hip -> libtts_afe_test.so), the case matrix, float64 references, the derived error bounds, and a NumPy
float32 restatement of each kernel's operation order (with switches that seed one defect each).

References (float64, independent of the kernels' code):
  resampler   torchaudio.functional.resample's defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) written two ways: the polyphase tap table applied
              with stride o, and a direct evaluation of the continuous kernel h((m / o - j / n) base) per output sample j and input sample m.
  mel         torch.stft in float64 (centre, reflect, periodic Hann) and the vectorised filterbank restatement of tests/test_mel_frontend.py.

Bounds (derived; DESIGN.md "What pins the audio front-end" has the argument), u = 2^-24:
  resampler   |y - ref| <= gamma * sum_k |w_k x_k| + K 2^-126 (1 + max |x|), gamma = (K + 1) u / (1 - (K + 1) u): K fused multiply-adds in a fixed order, one
              rounding of each tap; the second term is the f32 format's underflow (taps at the window's zero are 1e-49 in double and 0 in float).
  mel         per bin |dX| <= delta = (10 eta + 2 u) sqrt(1024) |x_w|_2 with eta = u + gamma_4 (sqrt 2 + u) per radix-2 stage (Higham, Accuracy and Stability of
              Numerical Algorithms, theorem 24.2, with table twiddles of error u) and 2 u for the window table and the windowing product;
              power: ds = (2 |X| delta + delta^2) (1 + 2 u) + 2 u |X|^2, magnitude: ds = delta + 2.5 u |X|;
              band: dm = sum fb ds + gamma_(cnt + 1) sum fb (s + ds) (one rounding of each weight, cnt fused multiply-adds);
              log: |d| <= log(max(m + dm, 1e-5) / max(m - dm, 1e-5)) / norm + 3 u |ref| (logf within 1 ulp, one division, the f32 clamp constant)."""
import ctypes as C
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tortoise.cpp_amd", "libtts_afe_test.so")
RESAMPLE, MEL80, MEL100, NONFINITE = 0, 1, 2, 3
KIND_NAMES = {RESAMPLE: "afe_resample_kernel", MEL80: "afe_mel_kernel<80,2>", MEL100: "afe_mel_kernel<100,1>", NONFINITE: "afe_nonfinite_kernel"}
U = 2.0 ** -24
ERR_LIMIT = -6
HIP_INVALID = 1
LOG_FLOOR = np.float32(np.log(1e-5))
WIN80, WIN100 = 132300, 102400
MEL_PARAMS = {80: (22050.0, 8000.0, True, 2), 100: (24000.0, 12000.0, False, 1)}  # bands -> sample rate, f_max, HTK scale, power


class HipError(RuntimeError):
    pass


class _Case(C.Structure):
    _fields_ = [("kind", C.c_int), ("n_clips", C.c_int), ("orig_rate", C.c_int), ("new_rate", C.c_int), ("in_len", C.c_void_p), ("start", C.c_void_p),
                ("win", C.c_void_p), ("in_", C.c_void_p), ("norms", C.c_void_p), ("out", C.c_void_p)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        L.tts_afe_test_out_floats.restype = C.c_longlong
        _lib = L
    return _lib


def geometry(orig, new):
    """(status, o, n, width, taps) from the product's afe_resample_geometry"""
    g = (C.c_int * 4)()
    rc = lib().tts_afe_test_geometry(int(orig), int(new), g)
    return (rc,) + tuple(g)


class Case:
    """kind, clips (list of float32 arrays) and, by kind: orig / new (rates), start / win (per clip), norms"""

    def __init__(self, kind, clips, family="", **p):
        self.kind, self.clips, self.family, self.p = kind, [np.ascontiguousarray(c, np.float32) for c in clips], family, p

    def name(self):
        q = {k: v for k, v in self.p.items() if k != "norms"}
        return "%s %s lens %s %s%s" % (KIND_NAMES[self.kind], self.family, [len(c) for c in self.clips], q, " norms" if self.p.get("norms") is not None else "")

    def alone(self, s):
        q = dict(self.p)
        for k in ("start", "win"):
            if k in q:
                q[k] = [q[k][s]]
        return Case(self.kind, [self.clips[s]], self.family, **q)

    def struct(self, out_ptr=1, **override):
        keep = []

        def arr(v, dt):
            a = np.ascontiguousarray(v, dt)
            keep.append(a)
            return a.ctypes.data

        c = _Case()
        c.kind, c.n_clips = self.kind, len(self.clips)
        c.orig_rate, c.new_rate = int(self.p.get("orig", 0)), int(self.p.get("new", 0))
        c.in_len = arr([len(x) for x in self.clips], np.int64)
        c.in_ = arr(np.concatenate(self.clips) if self.clips else np.zeros(1, np.float32), np.float32)
        if "start" in self.p:
            c.start, c.win = arr(self.p["start"], np.int64), arr(self.p["win"], np.int64)
        if self.p.get("norms") is not None:
            c.norms = arr(self.p["norms"], np.float32)
        c.out = out_ptr
        for k, v in override.items():
            setattr(c, k, v)
        return c, keep


class Out:
    def __init__(self, raw, margin, floats):
        self.raw, self.margin = raw, margin
        self.payload = raw[margin:margin + 4 * floats].view(np.float32).copy()

    def canaries_intact(self):
        return bool((self.raw[:self.margin] == 0xCB).all() and (self.raw[len(self.raw) - self.margin:] == 0xCB).all())


def validate(case, **override):
    c, keep = case.struct(**override)
    return lib().tts_afe_test_validate(C.byref(c))


def run(case):
    """launches the case once; HipError for anything but success (a refused case included)"""
    L = lib()
    c, keep = case.struct()
    floats = L.tts_afe_test_out_floats(C.byref(c))
    if floats < 0:
        raise HipError("%s: refused (%d)" % (case.name(), floats))
    margin = L.tts_afe_test_margin()
    raw = np.zeros(4 * floats + 2 * margin, np.uint8)
    c.out = raw.ctypes.data
    rc = L.tts_afe_test_run(C.byref(c))
    if rc != 0:
        raise HipError("%s: HIP error %d" % (case.name(), rc))
    return Out(raw, margin, floats)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# resampler
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def res_geometry(orig, new, width_short=0):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    width = int(math.ceil(6.0 * o / base)) - width_short
    return o, n, width, 2 * width + o, base


def _h(t, scaled=1.0):
    """the continuous kernel: sinc(pi t) cos^2(pi t / 12) of the clamped t (float64)"""
    t = np.clip(t, -6.0, 6.0)
    a = t * np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(a == 0.0, 1.0, np.sin(a) / a)
    return s * np.cos(t * np.pi / 12.0) ** 2 * scaled


def res_table(orig, new, width_short=0, no_scale=False, phase_shift=0):
    o, n, width, taps, base = res_geometry(orig, new, width_short)
    k = np.arange(taps, dtype=np.float64) - width + phase_shift
    p = np.arange(n, dtype=np.float64)
    t = (-p[:, None] / n + k[None, :] / o) * base
    return _h(t, 1.0 if no_scale else base / o)


def res_len(orig, new, length, floor=False):
    o, n = res_geometry(orig, new)[:2]
    return (n * length) // o if floor else -((-n * length) // o)


def _res_windows(x, o, width, taps, blocks):
    xp = np.concatenate([np.zeros(width), np.asarray(x, np.float64), np.zeros(width + o + taps)])
    return np.lib.stride_tricks.as_strided(xp, (blocks, taps), (xp.strides[0] * o, xp.strides[0]))


def res_reference(x, orig, new):
    """spelling 1, the polyphase table: (y [ceil(n len / o)], A = sum |w x| per output), float64"""
    o, n, width, taps, _ = res_geometry(orig, new)
    tab = res_table(orig, new)
    out = res_len(orig, new, len(x))
    blocks = -(-out // n)
    X = _res_windows(x, o, width, taps, blocks)
    y = np.einsum("bk,pk->bp", X, tab).reshape(-1)[:out]
    A = np.einsum("bk,pk->bp", np.abs(X), np.abs(tab)).reshape(-1)[:out]
    return y, A


def res_direct(x, orig, new):
    """spelling 2: every output sample j from the continuous kernel at (m / o - j / n) base over the input samples m under its taps"""
    o, n, width, taps, base = res_geometry(orig, new)
    x = np.asarray(x, np.float64)
    out = res_len(orig, new, len(x))
    j = np.arange(out)
    m = (j // n)[:, None] * o - width + np.arange(taps)[None, :]
    t = (m / o - j[:, None] / n) * base
    xv = np.where((m >= 0) & (m < len(x)), x[np.clip(m, 0, len(x) - 1)], 0.0)
    return (_h(t, base / o) * xv).sum(axis=1)


def res_gamma(taps):
    return (taps + 1) * U / (1.0 - (taps + 1) * U)


def res_bound(A, taps, xmax):
    """gamma A, and the f32 format's floor: a tap below 2^-126 (the window's zero at |t| = 6 leaves taps of 1e-49) or a product below it may be flushed to zero"""
    return res_gamma(taps) * A + taps * 2.0 ** -126 * (1.0 + xmax)


def _fma32(a, b, c):
    """f32 fused multiply-add: the product of two floats is exact in double; one rounding of the double sum, then the narrowing (a double rounding in rare ties)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def res_emulate(x, orig, new, width_short=0, no_scale=False, phase_shift=0, floor=False):
    """the kernel's operation order in float32: taps ascending, one fused multiply-add each; the switches seed one defect each"""
    o, n, width, taps, _ = res_geometry(orig, new)
    tab = res_table(orig, new, 0, no_scale, phase_shift).astype(np.float32)
    out = res_len(orig, new, len(x), floor)
    blocks = max(1, -(-out // n))
    # width_short: the zero padding in front one sample short of the table's width. (A table built with width - 1 throughout is no defect: ceil(6 o / base) always
    # leaves the outermost tap at |t| >= 6, where the window is zero.)
    X = _res_windows(x, o, width - width_short, taps, blocks).astype(np.float32)
    acc = np.zeros((blocks, n), np.float32)
    for k in range(taps):
        acc = _fma32(np.broadcast_to(tab[None, :, k], acc.shape), np.broadcast_to(X[:, k:k + 1], acc.shape), acc)
    return acc.reshape(-1)[:out]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# mel
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def filterbank(n_mels, sr, f_max, htk, n_fft=1024):
    """tests/test_mel_frontend.py's vectorised restatement (librosa / torchaudio: triangles on the mel scale, Slaney area normalisation), float64 [n_mels][513]"""
    def h2m(f):
        f = np.asarray(f, np.float64)
        if htk:
            return 2595.0 * np.log10(1.0 + f / 700.0)
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-9) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3))

    def m2h(m):
        m = np.asarray(m, np.float64)
        if htk:
            return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
        return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)

    pts = m2h(np.linspace(h2m(0.0), h2m(f_max), n_mels + 2))
    freqs = np.linspace(0, sr / 2, n_fft // 2 + 1)
    d = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower, upper = -ramps[:-2] / d[:-1, None], ramps[2:] / d[1:, None]
    return np.maximum(0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]


_FB = {}


def fb_of(bands, swap_scale=False):
    key = (bands, swap_scale)
    if key not in _FB:
        sr, f_max, htk, _ = MEL_PARAMS[bands]
        _FB[key] = filterbank(bands, sr, f_max, htk != swap_scale)
    return _FB[key]


def virtual_signal(x, start, win):
    """the window the kernel reads: x[start : start + win], zeros behind"""
    v = np.zeros(win, np.float64)
    seg = np.asarray(x, np.float64)[start:start + win]
    v[:len(seg)] = seg
    return v


def _frames_of(v, frames):
    """[frames][1024]: the reflect-padded signal cut into hops"""
    vp = np.concatenate([v[1:513][::-1], v, v[-513:-1][::-1]])
    return np.lib.stride_tricks.as_strided(vp, (frames, 1024), (vp.strides[0] * 256, vp.strides[0]))


def mel_reference(x, start, win, bands, norms=None, x_err=None):
    """float64: (ref [bands][frames], bound [bands][frames]). x_err: a per-sample bound on how far the kernel's input signal may lie from x (the resampler's bound,
    when x is the float64 resampler's output): it moves a bin by at most sum_i win_i x_err_i and the frame's norm by at most |x_err_w|_2."""
    import torch
    _, _, _, power = MEL_PARAMS[bands]
    v = virtual_signal(x, start, win)
    w = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    S = torch.stft(torch.from_numpy(v), 1024, hop_length=256, win_length=1024, window=w, center=True, pad_mode="reflect", return_complex=True).numpy()
    mag = np.abs(S)  # [513][frames]
    frames = mag.shape[1]
    assert frames == win // 256 + 1
    # |x_w|_2 per frame: the windowed samples of the reflect-padded signal
    fr = _frames_of(v, frames) * w.numpy()[None, :]
    norm2 = np.sqrt((fr ** 2).sum(axis=1))  # [frames]
    moved = np.zeros(frames)
    if x_err is not None:
        fe = _frames_of(virtual_signal(x_err, start, win), frames) * w.numpy()[None, :]
        moved = fe.sum(axis=1)
        norm2 = norm2 + np.sqrt((fe ** 2).sum(axis=1))
    eta = U + (4 * U / (1 - 4 * U)) * (math.sqrt(2.0) + U)
    delta = ((10 * eta + 2 * U) * 32.0 * norm2 + moved)[None, :]
    if power == 2:
        s = mag ** 2
        ds = (2 * mag * delta + delta ** 2) * (1 + 2 * U) + 2 * U * s
    else:
        s = mag
        ds = delta + 2.5 * U * mag
    fb = fb_of(bands)
    cnt = (fb != 0).sum(axis=1).astype(np.float64) + 1
    g = (cnt * U / (1 - cnt * U))[:, None]
    m = fb @ s
    dm = fb @ ds + g * (fb @ (s + ds))
    nrm = np.ones(bands) if norms is None else np.asarray(norms, np.float64)
    ref = np.log(np.maximum(m, 1e-5)) / nrm[:, None]
    bound = np.log(np.maximum(m + dm, 1e-5) / np.maximum(m - dm, 1e-5)) / np.abs(nrm[:, None]) + 3 * U * np.abs(ref)
    return ref, bound


def _bitrev10():
    i = np.arange(1024)
    r = np.zeros(1024, np.int64)
    for b in range(10):
        r |= ((i >> b) & 1) << (9 - b)
    return r


def mel_emulate(x, start, win, bands, norms=None, reflect_off=0, symmetric_hann=False, power=None, swap_scale=False, clamp_after_log=False):
    """the kernel's operation order in float32 (tables rounded once from float64; bit-reversed load; ten radix-2 stages; spans ascending, one fused multiply-add per
    bin; the clamp's constant branch); the switches seed one defect each"""
    power = MEL_PARAMS[bands][3] if power is None else power
    x = np.asarray(x, np.float32)
    frames = win // 256 + 1
    i = np.arange(1024, dtype=np.float64)
    wn = (0.5 - 0.5 * np.cos(2 * np.pi * i / (1023.0 if symmetric_hann else 1024.0))).astype(np.float32)
    k = np.arange(512, dtype=np.float64)
    twr, twi = np.cos(-2 * np.pi * k / 1024).astype(np.float32), np.sin(-2 * np.pi * k / 1024).astype(np.float32)
    j = np.arange(frames)[:, None] * 256 + np.arange(1024)[None, :] - 512
    j = np.where(j < 0, -j - reflect_off, j)
    j = np.where(j >= win, 2 * (win - 1) - j + reflect_off, j)
    j = np.clip(j, 0, win - 1)
    avail = len(x) - start
    v = np.where(j < avail, x[np.clip(start + j, 0, len(x) - 1)], np.float32(0))
    re = np.zeros((frames, 1024), np.float32)
    re[:, _bitrev10()] = v * wn[None, :]
    im = np.zeros_like(re)
    ln = 2
    while ln <= 1024:
        half, step = ln // 2, 1024 // ln
        wr, wi = twr[::step][:half], twi[::step][:half]
        R, I = re.reshape(frames, 1024 // ln, 2, half), im.reshape(frames, 1024 // ln, 2, half)
        ur, ui, ar, ai = R[:, :, 0].copy(), I[:, :, 0].copy(), R[:, :, 1].copy(), I[:, :, 1].copy()
        WR, WI = np.broadcast_to(wr, ar.shape), np.broadcast_to(wi, ar.shape)
        vr = _fma32(ar, WR, -(ai * WI))
        vi = _fma32(ar, WI, ai * WR)
        R[:, :, 0], I[:, :, 0], R[:, :, 1], I[:, :, 1] = ur + vr, ui + vi, ur - vr, ui - vi
        ln *= 2
    re, im = re[:, :513], im[:, :513]
    p = _fma32(re, re, im * im)
    s = p if power == 2 else np.sqrt(p)
    fb = fb_of(bands, swap_scale)
    out = np.zeros((bands, frames), np.float32)
    for b in range(bands):
        nz = np.nonzero(fb[b])[0]
        m = np.zeros(frames, np.float32)
        if len(nz):
            for kk in range(nz[0], nz[-1] + 1):
                m = _fma32(np.full(frames, np.float32(fb[b, kk])), s[:, kk], m)
        with np.errstate(divide="ignore"):
            if clamp_after_log:
                lg = np.maximum(np.log(m), np.float32(1e-5))
            else:
                lg = np.where(m > np.float32(1e-5), np.log(np.maximum(m, np.float32(1e-30))), LOG_FLOOR).astype(np.float32)
        out[b] = lg / np.float32(norms[b]) if norms is not None else lg
    return out


def judge(got, ref, bound):
    """(elements outside their bound, worst |err| / bound): every element counts"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = int((~(err <= bound)).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return bad, float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
RATE_PAIRS = [(22050, 24000), (44100, 22050), (48000, 22050), (16000, 22050), (8000, 22050)]
LIMIT_PAIR = (22051, 22050)
BLOCK = 256  # outputs per workgroup of afe_resample_kernel (tts_afe_test_block)
FPW = 4      # frames per workgroup of afe_mel_kernel (tts_afe_test_fpw)


def res_lengths(orig, new):
    """1, o - 1, o, o + 1, 3 o + 1, and an input length whose output count lies a few samples past a multiple of the kernel's block"""
    o, n = res_geometry(orig, new)[:2]
    past = -(-(2 * BLOCK + 3) * o // n)
    return sorted({1, max(1, o - 1), o, o + 1, 3 * o + 1, past})


def res_input(family, length, seed):
    rs = np.random.RandomState(seed)
    x = np.zeros(length, np.float32)
    if family == "impulse_first":
        x[0] = 1
    elif family == "impulse_last":
        x[-1] = 1
    elif family == "dc":
        x[:] = 1
    elif family == "noise":
        x = rs.randn(length).astype(np.float32)
    elif family == "noise_1e-3":
        x = (1e-3 * rs.randn(length)).astype(np.float32)
    elif family == "noise_30":
        x = (30 * rs.randn(length)).astype(np.float32)
    else:
        raise ValueError(family)
    return x


RES_FAMILIES = ["impulse_first", "impulse_last", "dc", "noise", "noise_1e-3", "noise_30"]


def res_cases():
    out = []
    for pi, (a, b) in enumerate(RATE_PAIRS):
        for li, n in enumerate(res_lengths(a, b)):
            for fi, fam in enumerate(RES_FAMILIES):
                out.append(Case(RESAMPLE, [res_input(fam, n, 1000 * pi + 10 * li + fi)], fam, orig=a, new=b))
    return out


# mel lengths (the window; the clip is as long unless the window case says otherwise): the minimum reflect padding allows, 600, around a hop multiple, a frame count
# that is no multiple of FPW (256 * 5 -> 6 frames), and upstream's two windows
MEL_LENGTHS = [513, 600, 256 * 3 - 1, 256 * 3, 256 * 3 + 1, 256 * 5]
MEL_FAMILIES = ["zeros", "impulse", "tone", "noise", "tone_over_noise"]


def mel_input(family, length, seed, bands):
    rs = np.random.RandomState(seed)
    t = np.arange(length)
    if family == "zeros":
        return np.zeros(length, np.float32)
    if family == "impulse":
        x = np.zeros(length, np.float32)
        x[length // 2] = 1
        return x
    if family == "tone":  # the centre of bin 40
        return np.sin(2 * np.pi * 40 * t / 1024.0).astype(np.float32)
    if family == "noise":
        return (0.3 * rs.randn(length)).astype(np.float32)
    if family == "tone_over_noise":
        return (np.sin(2 * np.pi * 40 * t / 1024.0) + 1e-4 * rs.randn(length)).astype(np.float32)
    raise ValueError(family)


def mel_cases(bands, lengths=MEL_LENGTHS):
    kind = MEL80 if bands == 80 else MEL100
    out = []
    for li, n in enumerate(lengths):
        for fi, fam in enumerate(MEL_FAMILIES):
            out.append(Case(kind, [mel_input(fam, n, 77 * li + fi + bands, bands)], fam, start=[0], win=[n]))
    return out


def mel_norms(seed=5):
    return (1.0 + np.random.RandomState(seed).rand(80)).astype(np.float32)


def reference(case):
    """per clip: list of (ref, bound) in float64"""
    out = []
    for s, x in enumerate(case.clips):
        if case.kind == RESAMPLE:
            y, A = res_reference(x, case.p["orig"], case.p["new"])
            out.append((y, res_bound(A, res_geometry(case.p["orig"], case.p["new"])[3], float(np.abs(x).max()))))
        else:
            bands = 80 if case.kind == MEL80 else 100
            ref, b = mel_reference(x, case.p["start"][s], case.p["win"][s], bands, case.p.get("norms"))
            out.append((ref.reshape(-1), b.reshape(-1)))
    return out


def emulate(case, **defect):
    out = []
    for s, x in enumerate(case.clips):
        if case.kind == RESAMPLE:
            out.append(res_emulate(x, case.p["orig"], case.p["new"], **defect))
        else:
            bands = 80 if case.kind == MEL80 else 100
            out.append(mel_emulate(x, case.p["start"][s], case.p["win"][s], bands, case.p.get("norms"), **defect).reshape(-1))
    return out


def resample64(x, orig, new):
    """the float64 resampler as the front-end applies it: equal rates pass the samples through"""
    x = np.asarray(x, np.float64)
    return x if orig == new else res_reference(x, orig, new)[0]


def chain64(x, rate):
    """The front-end's chain in float64 with the resampler bounds it accumulates: (a22, e22, a24, e24). e22: the first resampler's bound per sample; e24: the
    second's own bound plus the first's carried through the second's taps (sum |w| e22)."""
    x = np.asarray(x, np.float64)
    if rate == 22050:
        a22, e22 = x, np.zeros(len(x))
    else:
        a22, A = res_reference(x, rate, 22050)
        e22 = res_bound(A, res_geometry(rate, 22050)[3], float(np.abs(x).max()))
    a24, A = res_reference(a22, 22050, 24000)
    e24 = res_bound(A, res_geometry(22050, 24000)[3], float(np.abs(a22).max())) + res_reference(e22, 22050, 24000)[1]
    return a22, e22, a24, e24
