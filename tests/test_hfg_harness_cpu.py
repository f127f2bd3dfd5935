"""CPU side of tests/test_hfg_kernels_gpu.py: the harness library builds for gfx950, loads and exports its surface; it refuses every invalid case before any HIP
call; it builds hifigan_run's candidate table; the float64 references of tests/hfg_cases.py are checked against torch.nn.functional in float64 (conv1d,
conv_transpose1d, interpolate, leaky_relu) and the transposed convolution against a scatter followed by the crop, to 1e-12; the Python repack of a ConvTranspose1d
weight is checked through the kernel's own phase formula; a float32 restatement of every kernel, summing forward and backward, passes the acceptance rule on every
case of the matrix (the bound is not too tight) and equals float64 bit for bit on the exact family; and every listed defect leaves the bound on some case (the
bound is sharp). Which case catches which defect is printed (pytest -s)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hfg_cases as V
from hfg_cases import COND, CONV, CONV_SMALL, INTERP, POST

f32, i32 = np.float32, np.int32
KINDS = [CONV, CONV_SMALL, INTERP, COND, POST]


def test_harness_library_builds_and_exports_its_surface():
    L = V.harness()  # builds it once if missing; raises otherwise
    for sym in ("tts_hfg_test_run", "tts_hfg_test_validate", "tts_hfg_test_table", "tts_hfg_test_margin", "tts_hfg_test_seq_ints", "tts_hfg_test_frames",
                "tts_hfg_test_lds_bytes"):
        assert hasattr(L, sym), sym
    assert L.tts_hfg_test_margin() == 4096 and L.tts_hfg_test_seq_ints() == 9
    src_t = max(os.path.getmtime(V.SRC), os.path.getmtime(os.path.join(V.PKG, "csrc", "hifigan.hip")))
    assert os.path.getmtime(V.LIB) >= src_t or os.environ.get("TTS_HFG_TEST_LIB"), "libtts_hfg_test.so is older than its sources: run make"


def test_harness_is_not_part_of_the_product():
    mk = open(os.path.join(V.PKG, "Makefile")).read()
    assert "HIP_SRCS = $(wildcard csrc/*.hip)" in mk and not os.path.exists(os.path.join(V.PKG, "csrc", "hfg_harness.hip"))
    link = [l for l in mk.splitlines() if "-o $@ $(OBJS)" in l]
    assert len(link) == 1 and "testlib" not in link[0] and "hfg_test" not in link[0]
    rule = [l for l in mk.splitlines() if "testlib/hfg_harness.hip csrc/host_logic.cpp -o $@" in l]
    assert len(rule) == 1 and "vgpr-form" not in rule[0]  # the flags of csrc/hifigan.o
    assert all("libtts_hfg_test.so" in l for l in mk.splitlines() if l.startswith("all:") or l.startswith("\trm -f"))
    src = open(V.SRC).read()
    assert '#include "../csrc/hifigan.hip"' in src and "asm" not in src and "__global__" not in src  # the product's kernels, none of its own


# expressions the harness restates: each stands, spelled the same, in hifigan.hip and in the harness
RESTATED = ["hfg_interp_kernel<<<dim3(maxW, B), 256, 0,", "hfg_cond_kernel<<<dim3(HFG_C0 / 4,", "hfg_post_kernel<<<dim3(maxKeep, B), 256, 0,",
            "a.lo = -dil * (taps - 1) / 2; a.phases = phases; a.pad_t = phases / 2; a.rate = rate;",
            "const dim3 grid((unsigned)(((size_t)maxW * rate + HFG_TS - 1) / HFG_TS), (unsigned)B, (unsigned)(cout / 128 * phases));",
            "hfg_conv_small_kernel<<<grid, 256, (size_t)(HFG_TS + (taps - 1) * dil) * 33 * 4,",
            "const int nt = cout >= 64 ? 2 : 1;",
            "const dim3 grid((unsigned)(((size_t)maxW * rate + HFG_TM - 1) / HFG_TM), (unsigned)B, (unsigned)(cout / (32 * nt) * phases));",
            "const size_t lds = (size_t)(HFG_TM + (taps - 1) * dil) * 33 * 4;",
            "if (nt == 2) hfg_conv_kernel<2><<<grid, 256, lds,", "else hfg_conv_kernel<1><<<grid, 256, lds,"]
# what ties a citation `hifigan.hip:N` to the lines it names: one of these stands in the cited lines AND within a few lines of the citation
TOKENS = ["hfg_interp_kernel<<<", "hfg_cond_kernel<<<", "hfg_post_kernel<<<", "hfg_conv_small_kernel<<<grid, 256,", "hfg_conv_kernel<2><<<grid, 256, lds,",
          "cout >= 64 ? 2 : 1", "a.lo = -dil * (taps - 1) / 2", "a.acc_mode = ", "a.seq = d_seq", "(int)lat_rows", "lat_rows +=", "* dil) * 33 * 4", "cout % 128"]


def test_restated_launches_name_the_lines_of_hifigan_run_they_copy():
    """hifigan_run launches inline, so the harness restates grids, blocks, LDS sizes and the derived fields; each restated expression stands, spelled the same, in
    the harness and in hifigan.hip, and every citation `hifigan.hip:N` of the harness points at lines that hold what the lines beside the citation restate"""
    src = open(V.SRC).read()
    hfg = open(os.path.join(V.PKG, "csrc", "hifigan.hip")).read()
    for expr in RESTATED:
        assert expr in hfg and expr in src, expr
    lines, hl = src.splitlines(), hfg.splitlines()
    used = set()
    for i, line in enumerate(lines):
        for m in re.finditer(r"hifigan\.hip:(\d+)(?:-(\d+))?", line):
            lo, hi = int(m.group(1)), int(m.group(2) or m.group(1))
            cited, near = "\n".join(hl[lo - 1:hi]), "\n".join(lines[i:i + 6])
            hit = [t for t in TOKENS if t in cited and t in near]
            assert hit, (i + 1, lo, hi)
            used.update(hit)
    assert used == set(TOKENS)
    # the table rule: start is the running sum of ceil8(W)
    assert "q[0] = (int)fpad; q[1] = W; q[2] = v; q[3] = rows[c]; q[4] = (int)lat_rows; q[5] = (int)frames; q[6] = w0; q[7] = keep0; q[8] = keep_n;" in hfg
    assert "fpad += (W + 7) / 8 * 8" in hfg and "fpad = start + ceil8(W)" in src


def test_layouts_and_table_are_those_hifigan_run_builds():
    L = V.harness()
    assert [V.layout(n).frames for n in "ABCD"] == [8, 24, 48, 32]
    b = V.layout("B")
    assert b.start == [0, 16] and b.W == [9, 4]  # rows 9 .. 15 are padding: the candidates touch with nothing else between them
    c = V.layout("C")
    assert c.start == [0, 16, 24] and c.voice == [1, 0, 1] and c.n_voices == 2
    for n in range(1, 501):
        assert L.tts_hfg_test_frames(n) == V.frames_of(n)
    i = V.layout("I")
    assert i.W == [L.tts_hfg_test_frames(l) for l in (1, 2, 3)] == [4, 8, 13]  # the harness's T is tts_diffusion_frames(L)
    j = V.layout("J")
    assert j.L == [500] * 3 and j.w0[1] + j.W[1] == L.tts_hfg_test_frames(500) == 2176
    for name in V.LAYOUTS:
        lay = V.layout(name)
        for kind in ((INTERP,) if name in "IJ" else (CONV, POST, INTERP) if name == "D" else (CONV, POST)):
            c = V.make(kind, name, "gauss", **(dict(cin=32, cout=32) if kind == CONV else {}))
            got = np.zeros((lay.ns, 9), i32)
            assert L.tts_hfg_test_table(C.byref(V.to_struct(c, V.Guarded(V.out_shape(c)))), got.ctypes.data_as(C.c_void_p)) == 0
            assert np.array_equal(got, lay.table()), (name, got, lay.table())
    d = V.layout("D")
    assert all(w0 > 0 and k0 > 0 and kn < W for W, _, _, w0, k0, kn in d.cand) and d.before == [0, 4]


# ---------------------------------------------------------------------------------------------------------------- validation (no HIP call is reached)

def _valid(kind):
    c = {CONV: lambda: V.make(CONV, "C", cin=64, cout=64, taps=7, dil=3, rate=8, acc=2, cbias=1, resid=1),
         CONV_SMALL: lambda: V.make(CONV_SMALL, "C", cin=64, cout=128, taps=2, phases=8, rate=1, cbias=1),
         INTERP: lambda: V.make(INTERP, "D"), COND: lambda: V.make(COND, "V3"), POST: lambda: V.make(POST, "D")}[kind]()
    return V.to_struct(c, V.Guarded(V.out_shape(c)))


def _rc(cs):
    L = V.harness()
    rc = L.tts_hfg_test_validate(C.byref(cs))
    if rc != 0:  # refused by the run entry too, before any HIP call (this machine has no GPU: a HIP call would return another code)
        assert L.tts_hfg_test_run(C.byref(cs)) == V.HIP_INVALID_VALUE
    return rc


@pytest.mark.parametrize("kind", KINDS)
def test_valid_cases_validate(kind):
    assert V.harness().tts_hfg_test_validate(C.byref(_valid(kind))) == 0


def test_every_case_of_the_matrix_validates():
    L = V.harness()
    for kind in KINDS:
        for c in V.cases(kind):
            assert L.tts_hfg_test_validate(C.byref(V.to_struct(c, V.Guarded(V.out_shape(c))))) == 0, c.name()
    assert L.tts_hfg_test_validate(None) == V.HIP_INVALID_VALUE and L.tts_hfg_test_run(None) == V.HIP_INVALID_VALUE


def _cand(rows):
    return np.ascontiguousarray(np.array(rows, i32))


C_OK = [(13, 1, 3, 0, 0, 13), (1, 0, 1, 0, 0, 1), (20, 1, 5, 0, 0, 20)]


def _c(s, **kw):
    """layout C's candidate list with fields of candidate s replaced"""
    names = ("W", "voice", "L", "w0", "keep0", "keep_n")
    rows = [list(r) for r in C_OK]
    for k, v in kw.items():
        rows[s][names.index(k)] = v
    return _cand(rows)


# (what, kind, fields to overwrite; arrays replace `cand` / `start`, None clears a pointer)
INVALID = [
    ("unknown kind", CONV, dict(kind=5)), ("kind < 0", CONV, dict(kind=-1)), ("no output", CONV, dict(out=None)), ("no input", CONV, dict(in_=None)),
    ("no input post", POST, dict(in_=None)), ("no latents", INTERP, dict(in_=None)), ("no voice", COND, dict(in_=None)),
    ("no weights", CONV, dict(w=None)), ("no bias", CONV_SMALL, dict(bias=None)), ("post no weights", POST, dict(w=None)), ("post no bias", POST, dict(bias=None)),
    ("cond no weights", COND, dict(w=None)), ("cond no bias", COND, dict(bias=None)), ("no candidates", CONV, dict(cand=None)), ("no candidates interp", INTERP, dict(cand=None)),
    ("acc_mode 2 without out", CONV, dict(out0=None)), ("acc_mode 1 without out", CONV, dict(out0=None, acc_mode=1)), ("resid == out without out", CONV, dict(out0=None, acc_mode=0, alias=1)),
    ("cin % 32", CONV, dict(cin=48)), ("cin 0", CONV, dict(cin=0)), ("cin % 32 small", CONV_SMALL, dict(cin=33)), ("cin too large", CONV, dict(cin=2048)),
    ("cout % 64 at nt 2", CONV, dict(cout=96)), ("cout 48", CONV, dict(cout=48)), ("cout 16", CONV, dict(cout=16)), ("cout 0", CONV, dict(cout=0)),
    ("cout too large", CONV, dict(cout=2048)), ("cout % 128 small", CONV_SMALL, dict(cout=64)), ("cout 192 small", CONV_SMALL, dict(cout=192)),
    ("taps 0", CONV, dict(taps=0)), ("dil 0", CONV, dict(dil=0)), ("taps 12", CONV, dict(taps=12)), ("dil 6", CONV, dict(dil=6)), ("taps < 0", CONV, dict(taps=-1)),
    ("LDS window", CONV, dict(taps=11, dil=25)), ("LDS window small", CONV_SMALL, dict(phases=1, taps=11, dil=47)),
    ("phases 3", CONV, dict(phases=3, taps=2)), ("phases 4", CONV, dict(phases=4, taps=2)), ("phases 0", CONV, dict(phases=0)), ("phases 16", CONV_SMALL, dict(phases=16)),
    ("phases 8 with 3 taps", CONV_SMALL, dict(taps=3)), ("phases 2 with 7 taps", CONV, dict(phases=2)),
    ("in == out", CONV, dict(alias=2)), ("alias < 0", CONV, dict(alias=-1)), ("acc_mode 3", CONV, dict(acc_mode=3)), ("acc_mode < 0", CONV, dict(acc_mode=-1)),
    ("rate 0", CONV, dict(rate=0)), ("rate 257", CONV, dict(rate=257)), ("rows above the cap", CONV, dict(rate=256, phases=2, taps=2)), ("slope NaN", CONV, dict(slope=float("nan"))),
    ("start % 8", CONV, dict(start=np.array([0, 20, 32], i32))), ("start % 8 post", POST, dict(start=np.array([0, 20], i32))),
    ("candidates overlap", CONV, dict(start=np.array([0, 8, 24], i32))), ("starts out of order", CONV, dict(start=np.array([24, 16, 0], i32))),
    ("negative start", CONV, dict(start=np.array([-8, 16, 24], i32))), ("last candidate past the buffer", CONV, dict(start=np.array([0, 16, 32], i32))),
    ("voice outside the table", CONV, dict(cand=_c(1, voice=2))), ("voice < 0", CONV_SMALL, dict(cand=_c(0, voice=-1))), ("voice outside the table post", POST, dict(n_voices=1)),
    ("keep0 + keep_n > W", CONV, dict(cand=_c(0, keep0=1))), ("keep_n > W post", POST, dict(cand=_cand([(12, 0, 20, 30, 5, 8), (9, 1, 3, 2, 3, 2)]))),
    ("keep_n 0", POST, dict(cand=_cand([(12, 0, 20, 30, 5, 0), (9, 1, 3, 2, 3, 2)]))), ("keep0 < 0", CONV, dict(cand=_c(2, keep0=-1, keep_n=5))),
    ("L 0", CONV, dict(cand=_c(1, L=0))), ("L 0 interp", INTERP, dict(cand=_cand([(12, 0, 0, 30, 5, 4), (9, 1, 3, 2, 3, 2)]))), ("L 501", CONV, dict(cand=_c(1, L=501))),
    ("w0 < 0", INTERP, dict(cand=_cand([(12, 0, 20, -1, 5, 4), (9, 1, 3, 2, 3, 2)]))), ("window past the utterance", INTERP, dict(cand=_cand([(12, 0, 20, 30, 5, 4), (9, 1, 3, 5, 3, 2)]))),
    ("W 0", CONV, dict(cand=_c(1, W=0, keep_n=0))), ("W past the buffer", CONV, dict(cand=_c(2, W=25, keep_n=25))),
    ("ns 0", CONV, dict(ns=0)), ("ns 4", CONV, dict(ns=4)), ("frames 56", CONV, dict(frames=56)), ("frames 56 post", POST, dict(frames=56)), ("frames % 8", CONV, dict(frames=50)),
    ("frames 0", INTERP, dict(frames=0)), ("frames too few", CONV, dict(frames=40)), ("voices 0", COND, dict(n_voices=0)), ("voices 4", COND, dict(n_voices=4)),
    ("voices 4 conv", CONV, dict(n_voices=4)),
]


@pytest.mark.parametrize("what,kind,over", INVALID, ids=[w for w, _, _ in INVALID])
def test_invalid_case_is_refused_before_any_hip_call(what, kind, over):
    cs = _valid(kind)
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            cs._keep.append(v)
            setattr(cs, k, v.ctypes.data_as(C.c_void_p))
        else:
            setattr(cs, k, v)
    assert _rc(cs) == V.HIP_INVALID_VALUE


def test_the_lds_refusal_is_the_64_kb_window():
    L = V.harness()
    assert L.tts_hfg_test_lds_bytes(CONV, 11, 5) == (256 + 50) * 33 * 4 and L.tts_hfg_test_lds_bytes(CONV_SMALL, 11, 5) == (32 + 50) * 33 * 4
    assert L.tts_hfg_test_lds_bytes(CONV, 11, 24) == 65472 <= 65536 < L.tts_hfg_test_lds_bytes(CONV, 11, 25)  # (what refuses 11 x 24 is the cap on the dilation)


# ---------------------------------------------------------------------------------------------------------------- references against torch in float64

def _close(z, want):
    assert z.shape == want.shape
    assert np.abs(z - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def test_the_operand_path_is_torch_leaky_relu():
    """slopes 1 and 0.5 are exact in any precision (float64 leaky_relu, 1e-12); 0.1 and 0.01 round in f32, where the restated path is torch's float32 leaky_relu bit for bit"""
    x = V.make(CONV, "C", "straddle", cin=32, cout=32, rate=8).a["in_"]
    for slope in (1.0, 0.5):
        _close(V.leaky32(x, slope).astype(np.float64), F.leaky_relu(_t(x), slope).numpy())
    for slope in (0.1, 0.01):
        want = F.leaky_relu(torch.from_numpy(x), float(f32(slope))).numpy()
        assert np.array_equal(V.leaky32(x, slope).view(np.uint32), want.view(np.uint32))


CONV_TORCH = [dict(cin=32, cout=32, taps=3, dil=1, rate=1), dict(cin=64, cout=64, taps=7, dil=3, rate=8, acc=1, resid=1, cbias=1),
              dict(cin=64, cout=128, taps=11, dil=5, rate=1, acc=2, resid=2), dict(cin=32, cout=32, taps=11, dil=5, rate=8, cbias=1, resid=1)]


@pytest.mark.parametrize("p", CONV_TORCH, ids=["k3", "k7d3-acc1", "k11d5-acc2-alias", "k11d5-cbias"])
@pytest.mark.parametrize("lname", ["B", "C"])
def test_conv_reference_against_torch(p, lname):
    """F.conv1d(F.leaky_relu(x, slope), w, dilation, padding = dil (k - 1) / 2) per candidate, zero padding at ITS ends; + bias + cbias[voice] + resid; the three acc_modes"""
    c = V.make(CONV, lname, "straddle", seed=3, slope=0.5, **p)
    q, a, lay = c.p, c.a, c.lay
    z = V.reference(c)["z"]
    R = q["rate"]
    for s in range(lay.ns):
        sl = lay.rows(s, R)
        x = F.leaky_relu(_t(a["in_"][sl]).t().unsqueeze(0), 0.5)
        w = _t(a["w"]).permute(2, 1, 0)  # [k][cin][cout] -> torch's [cout][cin][k]
        y = F.conv1d(x, w, _t(a["bias"]), dilation=q["dil"], padding=q["dil"] * (q["taps"] - 1) // 2)[0].t()
        if q["cbias"]:
            y = y + _t(a["cbias"][lay.voice[s]])
        if q["resid"]:
            y = y + _t(a["resid"][sl] if q["resid"] == 1 else a["out0"][sl])
        if q["acc"] == 1:
            y = y + _t(a["out0"][sl])
        if q["acc"] == 2:
            y = (_t(a["out0"][sl]) + y) / 3
        _close(z[sl], y.numpy())
    assert (z[~lay.live(R)] == 0).all()


@pytest.mark.parametrize("u,rate,lname", [(8, 1, "C"), (8, 8, "B"), (2, 57, "B"), (2, 1, "A")])
def test_transposed_reference_against_torch_and_the_scatter_form(u, rate, lname):
    """F.conv_transpose1d(leaky_relu(x), W [cin][cout][2u], stride u, padding u / 2); and the same written as a scatter, then u / 2 samples cropped from either side"""
    c = V.make(CONV, lname, "gauss", seed=4, cin=64, cout=32, taps=2, phases=u, rate=rate, slope=0.5, cbias=1)
    a, lay = c.a, c.lay
    z = V.reference(c)["z"]
    for s in range(lay.ns):
        xs = F.leaky_relu(_t(a["in_"][lay.rows(s, rate)]), 0.5)
        n = xs.shape[0]
        y = F.conv_transpose1d(xs.t().unsqueeze(0), _t(a["w"]), _t(a["bias"]), stride=u, padding=u // 2)[0].t() + _t(a["cbias"][lay.voice[s]])
        assert y.shape[0] == n * u
        _close(z[lay.rows(s, rate * u)], y.numpy())
        full = np.zeros(((n - 1) * u + 2 * u, 32))
        w = a["w"].astype(np.float64)
        for t in range(n):
            for k in range(2 * u):
                full[t * u + k] += xs[t].numpy() @ w[:, :, k]
        _close(z[lay.rows(s, rate * u)], full[u // 2:u // 2 + n * u] + a["bias"].astype(np.float64) + a["cbias"][lay.voice[s]].astype(np.float64))


@pytest.mark.parametrize("u", [8, 2])
def test_repack_feeds_the_kernels_phase_formula(u):
    """output row q u + p = in[q + lo] W[p][0] + in[q + lo + 1] W[p][1] with lo = (p + pad_t) / u - 1, pad_t = u / 2 (hfg_conv_kernel), on the repacked weight,
    is ConvTranspose1d of the PyTorch-layout weight"""
    rs = np.random.RandomState(u)
    wt, x = rs.randn(6, 5, 2 * u), rs.randn(11, 6)
    wk = V.repack_convt(wt, u)
    assert wk.shape == (u, 2, 6, 5)
    want = F.conv_transpose1d(_t(x).t().unsqueeze(0), _t(wt), None, stride=u, padding=u // 2)[0].t().numpy()
    xp = np.concatenate([np.zeros((1, 6)), x, np.zeros((1, 6))])  # rows -1 and n read as zero
    got = np.zeros((11 * u, 5))
    for p in range(u):
        lo = (p + u // 2) // u - 1
        for q in range(11):
            got[q * u + p] = xp[q + lo + 1] @ wk[p, 0] + xp[q + lo + 2] @ wk[p, 1]
    _close(got, want)
    w = rs.randn(5, 6, 7)
    assert V.repack_conv(w).shape == (7, 6, 5) and V.repack_conv(w)[2, 3, 4] == w[4, 3, 2]


def _interp_naive(lat, n_out, inv_scale):
    """one F.interpolate(linear, align_corners=False) step written as a loop: source position (dst + 0.5) / scale - 0.5 clamped at 0, upper neighbour clamped"""
    n_in = len(lat)
    out = np.zeros((n_out,) + lat.shape[1:])
    for d in range(n_out):
        s = max((d + 0.5) * inv_scale - 0.5, 0.0)
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        out[d] = (1 - (s - i0)) * lat[i0] + (s - i0) * lat[i1]
    return out


@pytest.mark.parametrize("lname", ["I", "J", "D"])
def test_interp_reference_against_torch(lname):
    """F.interpolate(scale_factor = 4, linear, align_corners = False), then the same with 24000 / 22050 on the result; a window is a slice of the utterance.
    FINDING: where the second step keeps the length (T = 4 L: L = 1 and L = 2 only) ATen does not interpolate at all, it copies its input. For L = 1 that is the
    same signal; for L = 2 it is NOT the rule DESIGN.md states and hfg_interp_kernel computes (which resamples at (t + 0.5) 0.91875 - 0.5 for every L). The
    reference follows the stated rule; torch's shortcut is asserted here so that the difference is on record, and L = 2 is held to the rule written as a loop."""
    c = V.make(INTERP, lname, "gauss", seed=5)
    lay = c.lay
    z = V.reference(c)["z"]
    for s in range(lay.ns):
        L = lay.L[s]
        lat = _t(c.a["in_"][lay.lat0[s]:lay.lat0[s] + L])
        y1 = F.interpolate(lat.t().unsqueeze(0), scale_factor=4.0, mode="linear", align_corners=False)
        y = F.interpolate(y1, scale_factor=24000 / 22050, mode="linear", align_corners=False)[0].t().numpy()
        assert y.shape[0] == V.frames_of(L)
        if V.frames_of(L) == 4 * L and L > 1:
            assert L == 2 and np.array_equal(y, y1[0].t().numpy())  # the equal-length shortcut
            assert np.abs(z[lay.rows(s)] - y).max() > 0.1             # ... is another signal
        else:
            _close(z[lay.rows(s)], y[lay.w0[s]:lay.w0[s] + lay.W[s]])
        if L <= 3:
            _close(z[lay.rows(s)], _interp_naive(_interp_naive(lat.numpy(), 4 * L, 0.25), V.frames_of(L), 22050.0 / 24000.0)[lay.w0[s]:lay.w0[s] + lay.W[s]])
    assert [l for l in range(1, 501) if V.frames_of(l) == 4 * l] == [1, 2]


def test_interp_of_one_row_is_the_row_within_the_value_roundings():
    c = V.make(INTERP, "I", "outlier", seed=6)
    ref = V.reference(c)
    row = c.a["in_"][0].astype(np.float64)
    assert np.allclose(ref["z"][:4], row[None, :], rtol=1e-15, atol=0) and np.allclose(ref["bound"][:4], 8 * V.U * np.abs(row)[None, :], rtol=1e-12, atol=0)


def test_cond_and_post_references_against_torch():
    c = V.make(COND, "V3", "gauss", seed=7)
    y = F.conv1d(_t(c.a["in_"]).unsqueeze(2), _t(c.a["w"]).unsqueeze(2), _t(c.a["bias"]))[:, :, 0].numpy()
    _close(V.reference(c)["z"], y)
    for lname in ("B", "D"):
        c = V.make(POST, lname, "gauss", seed=8)
        lay, a = c.lay, c.a
        z = V.reference(c)["z"]
        xl = V.leaky32(a["in_"], 0.01)  # 0.01 rounds in f32: the f32 path, checked bit for bit above
        for s in range(lay.ns):
            y = torch.tanh(F.conv1d(_t(xl[lay.rows(s, 256)]).t().unsqueeze(0), _t(a["w"]).t().unsqueeze(0), _t(a["bias"]), padding=3))[0, 0].numpy()
            _close(V.seq_out(c, z, s), y[lay.keep0[s] * 256:(lay.keep0[s] + lay.keep_n[s]) * 256])


# ---------------------------------------------------------------------------------------------------------------- the rule accepts f32, rejects the defects

@pytest.mark.parametrize("kind", KINDS, ids=[V.KIND_NAMES[k] for k in KINDS])
def test_a_float32_restatement_is_accepted_on_every_case(kind):
    worst, exact = 0.0, 0
    for c in V.cases(kind):
        ref = V.reference(c)
        for order in (0, 1):
            out = V.restate32(c, order)
            bad, r = V.judge(out, ref)
            worst = max(worst, r)
            assert bad == 0 and V.guards_ok(c, out), (c.name(), order, bad, r)
            if ref["exact"]:
                assert V.exact_family_is_exact(c, ref), c.name()  # |partial sums| < 2^24 in units of 1/2
                assert V.exact_ok(out, ref), (c.name(), order)
        exact += bool(ref["exact"])
        pz = V.poisoned(c)
        if pz is not None:  # NaN on every row outside the candidates: kernels that check bounds never read them
            assert np.array_equal(V.restate32(pz, 0).view(np.uint32), V.restate32(c, 0).view(np.uint32)), c.name()
    print("%-24s f32 restatement, both orders: worst |err| / bound %.3f (%d exact cases)" % (V.KIND_NAMES[kind], worst, exact))
    assert worst <= 1.0
    assert exact >= (15 if kind == CONV else 10 if kind == CONV_SMALL else 1 if kind == COND else 0)


def test_the_matrix_holds_what_the_issue_names():
    for kind, shapes in ((CONV, V.SYN), (CONV_SMALL, V.SYN_SMALL)):
        m = V.matrix(kind)
        for cin, cout in shapes:
            got = {(p["taps"], p["dil"]) for _, _, p in m if (p["cin"], p["cout"]) == (cin, cout) and p.get("phases", 1) == 1}
            assert got >= {(t, d) for t in (3, 7, 11) for d in (1, 3, 5)}
        tins = {lay_w * p["rate"] for l, _, p in m for lay_w in V.layout(l).W}
        assert {t % 256 for t in tins} >= {0, 1, 255} and min(tins) < 32
        assert {p.get("phases", 1) for _, _, p in m} == {1, 2, 8} and {p.get("acc", 0) for _, _, p in m} == {0, 1, 2}
        assert {f for _, f, _ in m} == set(V.FAMS)
    prod = V.product_convs()
    assert len(prod) == 1 + 4 + 36 + 4 * (2 + 3 + 3) and prod[0] == dict(cin=1024, cout=512, taps=7, dil=1, phases=1, rate=1, slope=1.0, acc=0, cbias=1, resid=0)
    assert [(p["cin"], p["cout"], p["phases"], p["rate"]) for p in prod if p["phases"] > 1] == [(512, 256, 8, 1), (256, 128, 8, 8), (128, 64, 2, 64), (64, 32, 2, 128)]
    assert {(p["rate"], p["cin"]) for p in prod if p["phases"] == 1 and p["rate"] > 1} == {(8, 256), (64, 128), (128, 64), (256, 32)}
    assert all(l in "AB" for l, _, p in V.matrix(CONV) if p in prod)
    assert {V.layout(l).L[0] for l, _, _ in V.matrix(INTERP) if l in "IJ"} == {1, 500} and set(V.layout("I").L) == {1, 2, 3}


DEFECTS = {
    "tap_reversed": CONV, "dil_plus": CONV, "dil_minus": CONV, "lo_plus": CONV, "lo_minus": CONV, "pad_plus": CONV, "pad_minus": CONV, "taps_swapped": CONV,
    "phase_next": CONV, "leaky_after": CONV, "slope_swap": CONV, "cbias_other": CONV, "cbias_none": CONV, "resid_none": CONV, "resid_before_leaky": CONV,
    "acc2_div2": CONV, "acc2_forget": CONV, "neighbour": CONV, "chunks_swapped": CONV,
    "one_step": INTERP, "align_corners": INTERP, "no_upper_clamp": INTERP, "w0_ignored": INTERP,
    "post_6taps": POST, "post_no_leaky": POST, "keep0_ignored": POST, "cond_transposed": COND,
}
POST_SLOPE = "slope_swap"  # the same name on POST: 0.1 for 0.01


def _small(kind):
    """the cases the defects are looked for on: everything but the product shapes and the long layouts (the defect `leaky_after` holds every product in memory)"""
    if kind not in (CONV, CONV_SMALL):
        return V.matrix(kind)
    prod = V.product_convs()
    return [(l, f, p) for l, f, p in V.matrix(kind) if p not in prod and V.layout(l).frames * p["rate"] * p.get("phases", 1) * p["cin"] * p["cout"] <= 1 << 21]


@pytest.mark.parametrize("mut,kind", sorted(DEFECTS.items()) + [(POST_SLOPE, POST)] + [(m, CONV_SMALL) for m, k in sorted(DEFECTS.items()) if k == CONV and m != "chunks_swapped"],
                         ids=lambda v: v if isinstance(v, str) else V.KIND_NAMES[v])
def test_every_defect_is_rejected_on_some_case(mut, kind):
    caught, n = [], 0
    for l, f, p in _small(kind):
        c = V.make(kind, l, f, **p)
        ref = V.reference(c)
        z = V.reference(c, mut=mut)["z"]
        bad, r = V.judge(z, ref)
        n += 1
        if bad:
            caught.append((c.name(), bad, r))
            break
    print("%-20s %-22s rejected on case %d of those tried: %s" % (mut, V.KIND_NAMES[kind], n, caught[:1]))
    assert caught
