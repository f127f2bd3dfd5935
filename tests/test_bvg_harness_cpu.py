"""CPU side of tests/test_bvg_kernels_gpu.py: the harness library builds for gfx950, loads and exports its surface; it refuses every invalid case before any HIP
call; it builds bigvgan_run's candidate table; its restated launches are spelled as in csrc/bigvgan.h; the float64 references of tests/bvg_cases.py agree with
upstream's literal torch form (tests/bigvgan_ref.py) to 1e-12; a float32 restatement of every kernel passes the acceptance rule on every case (the bound is not
too tight); every seeded defect leaves the bound on some case (the bound is sharp); and the loader's host half, read through the harness's probe, takes the three
configurations, pads 48 -> 64 and 24 -> 32 with zeros, and refuses a missing, an extra and a mis-shaped tensor and strides whose product is not 256."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bigvgan_ref as R
import bvg_cases as V
from bvg_cases import ACT, MEL, POST
from tortoise_cpp_amd import synth_weights as sw

f32, i32 = np.float32, np.int32
KINDS = [ACT, MEL, POST]
FMT = -3


def test_harness_library_builds_and_exports_its_surface():
    L = V.harness()  # builds it once if missing; raises otherwise
    for sym in ("tts_bvg_test_run", "tts_bvg_test_validate", "tts_bvg_test_table", "tts_bvg_test_margin", "tts_bvg_test_run_rows", "tts_bvg_test_block_rows",
                "tts_bvg_test_parse", "tts_bvg_test_packed"):
        assert hasattr(L, sym), sym
    assert L.tts_bvg_test_margin() == 4096 and (L.tts_bvg_test_run_rows(), L.tts_bvg_test_block_rows()) == (V.RUN, V.BLOCK)
    src_t = max(os.path.getmtime(p) for p in (V.SRC, os.path.join(V.PKG, "csrc", "hifigan.hip"), os.path.join(V.PKG, "csrc", "bigvgan.h")))
    assert os.path.getmtime(V.LIB) >= src_t or os.environ.get("TTS_BVG_TEST_LIB"), "libtts_bvg_test.so is older than its sources: run make"


def test_harness_is_not_part_of_the_product():
    mk = open(os.path.join(V.PKG, "Makefile")).read()
    assert not os.path.exists(os.path.join(V.PKG, "csrc", "bvg_harness.hip"))
    link = [l for l in mk.splitlines() if "-o $@ $(OBJS)" in l]
    assert len(link) == 1 and "testlib" not in link[0] and "bvg_test" not in link[0]
    rule = [l for l in mk.splitlines() if "testlib/bvg_harness.hip csrc/host_logic.cpp -o $@" in l]
    assert len(rule) == 1 and "vgpr-form" not in rule[0]  # the flags of csrc/hifigan.o
    assert all("libtts_bvg_test.so" in l for l in mk.splitlines() if l.startswith("all:") or l.startswith("\trm -f"))
    src = open(V.SRC).read()
    assert '#include "../csrc/hifigan.hip"' in src and "asm" not in src and "__global__" not in src  # the product's kernels, none of its own
    hfg = open(os.path.join(V.PKG, "csrc", "hifigan.hip")).read()
    assert hfg.endswith('} // namespace tts\n#include "bigvgan.h"\n') and hfg.count("bigvgan") == 1  # included once, as the last line


RESTATED = ["bvg_mel_kernel<<<dim3(maxT, B), 128, 0,", "bvg_post_kernel<<<dim3(maxT, B), 256, 0,", "bvg_act_kernel<<<grid, 256, 0,",
            "const dim3 grid((unsigned)(((size_t)maxT * rate + BVG_ACT_RUNS * BVG_RUN - 1) / (BVG_ACT_RUNS * BVG_RUN)), (unsigned)B, (unsigned)(C / 32));",
            "q[0] = (int)"]


def test_restated_launches_are_spelled_as_in_bigvgan_run():
    src, bvg = open(V.SRC).read(), open(os.path.join(V.PKG, "csrc", "bigvgan.h")).read()
    for expr in RESTATED:
        assert expr in src and expr in bvg, expr
    assert "fpad += (T + 7) / 8 * 8" in bvg and "fpad = start + ceil8(T)" in src
    assert "q[0] = (int)fpad; q[1] = T; q[5] = (int)frames; q[8] = T;" in bvg and "q[0] = (int)start; q[1] = T; q[5] = (int)total; q[8] = T;" in src


def test_table_is_the_one_bigvgan_run_builds():
    L = V.harness()
    for c in (V.make(ACT, (5, 1, 13), 64, 8), V.make(ACT, (5, 1, 13), 64, 8, start=(8, 24, 32), frames=48), V.make(POST, (1, 3)), V.make(MEL, (7, 1, 9))):
        got = np.zeros((c.ns, 9), i32)
        assert L.tts_bvg_test_table(C.byref(V.to_struct(c, V.Guarded(V.out_shape(c)))), got.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(got, c.table()), (c.name(), got)
    c = V.make(ACT, (5, 1, 13), 64, 8)
    assert c.start == [0, 8, 16] and c.frames == 32 and c.before == [0, 5, 6]


def test_every_case_of_the_matrix_validates():
    L = V.harness()
    for kind in KINDS:
        for c in V.cases(kind):
            assert L.tts_bvg_test_validate(C.byref(V.to_struct(c, V.Guarded(V.out_shape(c))))) == 0, c.name()
    assert L.tts_bvg_test_validate(None) == V.HIP_INVALID_VALUE and L.tts_bvg_test_run(None) == V.HIP_INVALID_VALUE


def _valid(kind):
    c = {ACT: lambda: V.make(ACT, (5, 1, 13), 64, 8), MEL: lambda: V.make(MEL, (7, 1, 9)), POST: lambda: V.make(POST, (1, 3))}[kind]()
    return V.to_struct(c, V.Guarded(V.out_shape(c)))


INVALID = [
    ("unknown kind", ACT, dict(kind=3)), ("kind < 0", ACT, dict(kind=-1)), ("no output", ACT, dict(out=None)), ("no input", ACT, dict(in_=None)),
    ("no mel", MEL, dict(in_=None)), ("no input post", POST, dict(in_=None)), ("no frames list", ACT, dict(T=None)), ("no alpha", ACT, dict(alpha=None)),
    ("no inv_beta", ACT, dict(inv_beta=None)), ("post no alpha", POST, dict(alpha=None)), ("post no weights", POST, dict(w=None)), ("post no bias", POST, dict(bias=None)),
    ("C % 32", ACT, dict(C=48)), ("C 0", ACT, dict(C=0)), ("C < 0", ACT, dict(C=-32)), ("C too large", ACT, dict(C=160)), ("C % 32 post", POST, dict(C=33)),
    ("rate 0", ACT, dict(rate=0)), ("rate < 0", ACT, dict(rate=-8)), ("rate 1025", ACT, dict(rate=1025)), ("rows above the cap", ACT, dict(rate=512)),
    ("ns 0", ACT, dict(ns=0)), ("ns 4", ACT, dict(ns=4)), ("ns 0 mel", MEL, dict(ns=0)), ("frames 56", ACT, dict(frames=56)), ("frames % 8", ACT, dict(frames=36)),
    ("frames 0", MEL, dict(frames=0)), ("frames too few", ACT, dict(frames=24)), ("frames too few post", POST, dict(frames=8)),
    ("T 0", ACT, dict(T=np.array([5, 0, 13], i32))), ("T < 0", MEL, dict(T=np.array([7, -1, 9], i32))), ("T past the buffer", ACT, dict(T=np.array([5, 1, 40], i32))),
    ("start % 8", ACT, dict(start=np.array([0, 12, 16], i32))), ("candidates overlap", ACT, dict(start=np.array([0, 0, 8], i32))),
    ("starts out of order", ACT, dict(start=np.array([16, 8, 0], i32))), ("negative start", ACT, dict(start=np.array([-8, 8, 16], i32))),
    ("last candidate past the buffer", ACT, dict(start=np.array([0, 8, 24], i32))), ("start % 8 post", POST, dict(start=np.array([0, 4], i32))),
]


@pytest.mark.parametrize("what,kind,over", INVALID, ids=[w for w, _, _ in INVALID])
def test_invalid_case_is_refused_before_any_hip_call(what, kind, over):
    L, cs = V.harness(), _valid(kind)
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            cs._keep.append(v)
            setattr(cs, k, v.ctypes.data_as(C.c_void_p))
        else:
            setattr(cs, k, v)
    assert L.tts_bvg_test_validate(C.byref(cs)) == V.HIP_INVALID_VALUE
    assert L.tts_bvg_test_run(C.byref(cs)) == V.HIP_INVALID_VALUE  # refused by the run entry too (a HIP call on this machine would return another code)


# ---------------------------------------------------------------------------------------------------------------- references against torch in float64

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def test_act_reference_against_the_literal_form():
    """with the kernel's own numbers (f32 taps, alpha, 1 / beta widened) the reference is upstream's literal form per candidate, replicate at ITS ends"""
    for c in V.cases(ACT):
        z = V.reference(c)["z"]
        al, ib, f = c.a["alpha"].astype(np.float64), c.a["inv_beta"].astype(np.float64), V.TAPS.astype(np.float64)
        for s in range(c.ns):
            x = _t(c.a["in_"][c.rows(s)]).t().unsqueeze(0)
            F = torch.nn.functional
            ft = _t(f).view(1, 1, 12).expand(c.C, 1, 12)
            u = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), ft, stride=2, groups=c.C)[..., 15:-15]
            sn = u + torch.sin(_t(al).view(1, -1, 1) * u) ** 2 * _t(ib).view(1, -1, 1)
            y = F.conv1d(F.pad(sn, (5, 6), mode="replicate"), ft, stride=2, groups=c.C)[0].t().numpy()
            assert np.abs(z[c.rows(s)] - y).max() <= 1e-12 * max(1.0, np.abs(y).max()), c.name()
        assert (z[~c.live()] == 0).all()


def test_post_reference_against_torch():
    for c in V.cases(POST):
        ref = V.reference(c)
        al, ib = c.a["alpha"].astype(np.float64), c.a["inv_beta"].astype(np.float64)
        off = 0
        for s in range(c.ns):
            a, _ = V.act_ref(c.a["in_"], c.rows(s).start, c.T[s] * 256, al, ib)
            y = torch.tanh(torch.nn.functional.conv1d(_t(a).t().unsqueeze(0), _t(c.a["w"]).t().unsqueeze(0), _t(c.a["bias"]), padding=3))[0, 0].numpy()
            assert np.abs(ref["z"][off:off + len(y)] - y).max() <= 1e-12
            off += len(y)


def test_mel_reference_is_the_denormalisation():
    c = V.make(MEL, (7, 1, 9), seed=2)
    z = V.reference(c)["z"]
    for s in range(c.ns):
        m = c.a["in_"][100 * c.before[s]:100 * (c.before[s] + c.T[s])].astype(np.float64).reshape(100, c.T[s]).T
        want = (m + 1) / 2 * (2.3143386840820312 + 11.512925148010254) - 11.512925148010254
        assert np.abs(z[c.rows(s, 1), :100] - want).max() <= 2e-6  # one f32 rounding of a value below 16, and the constants' own
        assert (z[c.rows(s, 1), 100:] == 0).all()
    assert V.mel_exact(np.array([-1.0, 1.0], f32)).tolist() == [float(V.MINV), float(f32(f32(V.MAXV - V.MINV) + V.MINV))]


# ---------------------------------------------------------------------------------------------------------------- the rule accepts f32, rejects the defects

@pytest.mark.parametrize("kind", KINDS, ids=[V.KIND_NAMES[k] for k in KINDS])
def test_a_float32_restatement_is_accepted_on_every_case(kind):
    worst = 0.0
    for c in V.cases(kind):
        ref = V.reference(c)
        out = V.restate32(c)
        bad, r = V.judge(out, ref)
        worst = max(worst, r)
        assert bad == 0 and V.guards_ok(c, out, ref), (c.name(), bad, r)
        p = V.poisoned(c)
        if p is not None:  # NaN on every row outside the candidates: a kernel that clamps to the candidate never reads them
            assert np.array_equal(V.restate32(p).view(np.uint32), out.view(np.uint32)), c.name()
    print("%-16s f32 restatement: worst |err| / bound %.3f over %d cases" % (V.KIND_NAMES[kind], worst, len(V.cases(kind))))
    assert worst <= 1.0


def test_the_matrix_holds_what_the_issue_names():
    acts = V.cases(ACT)
    assert {c.C for c in acts} == {32, 64, 96}
    rows = {c.T[0] * c.rate for c in acts if c.ns == 1}
    assert rows >= {1, 2, 5, 6, 10, 11, 12, V.RUN - 1, V.RUN, V.RUN + 1, V.BLOCK - 1, V.BLOCK, V.BLOCK + 1}
    assert any(c.ns == 3 and not c.explicit_start for c in acts) and any(c.ns == 3 and c.explicit_start for c in acts)
    assert {tuple(c.T) for c in V.cases(MEL) if c.ns == 1} == {(1,), (7,), (8,), (9,)}
    assert any(c.C == 32 and sorted(c.T) == [1, 3] for c in V.cases(POST))
    big = [c for c in acts if c.fam == "big"]
    assert big and max(np.abs(c.a["in_"][c.live()]).max() * c.a["alpha"].max() for c in big) > 100  # the sine's argument leaves the first periods


DEFECTS = [(m, ACT) for m in V.MUTS_ACT] + [(m, POST) for m in V.MUTS_ACT] + [("post_6taps", POST), ("post_no_tanh", POST)]


@pytest.mark.parametrize("mut,kind", DEFECTS, ids=["%s-%s" % (m, V.KIND_NAMES[k]) for m, k in DEFECTS])
def test_every_defect_is_rejected_on_some_case(mut, kind):
    caught, n = [], 0
    for c in V.cases(kind):
        ref = V.reference(c)
        bad, r = V.judge(V.reference(c, mut=mut)["z"], ref)
        n += 1
        if bad:
            caught.append((c.name(), bad, r))
            break
    print("%-14s %-16s rejected on case %d of those tried: %s" % (mut, V.KIND_NAMES[kind], n, caught[:1]))
    assert caught


# ---------------------------------------------------------------------------------------------------------------- the loader's host half

def test_loader_reads_the_configuration_from_the_shapes():
    want = {"tiny": (96, 2, [16, 16, 0, 0, 0, 0], [96, 64, 32, 0, 0, 0, 0]), "base": (512, 4, [8, 8, 2, 2, 0, 0], [512, 256, 128, 64, 32, 0, 0]),
            "six": (384, 6, [4, 4, 2, 2, 2, 2], [384, 192, 96, 64, 32, 32, 32])}
    for name, (c0, n, ups, ch) in want.items():
        rc, out, err = V.parse(R.model(name)[0])
        assert rc == 0 and err == "" and (out[0], out[1]) == (c0, n) and out[2:8].tolist() == ups and out[8:15].tolist() == ch, (name, rc, out, err)


def test_loader_repacks_and_zero_pads():
    path, t = R.model("tiny")
    w = V.packed(path, 2, 0, 1, 0).reshape(7, 64, 64)  # stage 0, k = 7, convs1[0]: [k][cin_p][cout_p] from [cout][cin][k], 48 -> 64
    assert np.array_equal(w[:, :48, :48], t["bigvgan.resblocks.1.convs1.0.weight"].transpose(2, 1, 0)) and not w[:, 48:].any() and not w[:, :, 48:].any()
    pre = V.packed(path, 0).reshape(7, 128, 96)          # 100 mel bands padded to 128
    assert np.array_equal(pre[:, :100], t["bigvgan.conv_pre.weight"].transpose(2, 1, 0)) and not pre[:, 100:].any()
    ups = V.packed(path, 1, 1).reshape(16, 2, 64, 32)    # stage 1: 48 -> 24 channels, stride 16: [phase][2][cin_p][cout_p]
    src = t["bigvgan.ups.1.0.weight"]
    for ph in range(16):
        k0 = (ph + 8) % 16
        assert np.array_equal(ups[ph, 0, :48, :24], src[:, :, k0 + 16]) and np.array_equal(ups[ph, 1, :48, :24], src[:, :, k0])
    assert not ups[:, :, 48:].any() and not ups[:, :, :, 24:].any() and not V.packed(path, 7, 1)[24:].any()
    al, ib = V.packed(path, 4, 0, 2, 5), V.packed(path, 5, 0, 2, 5)
    a, b = t["bigvgan.resblocks.2.activations.5.act.alpha"].astype(np.float64), t["bigvgan.resblocks.2.activations.5.act.beta"].astype(np.float64)
    assert np.array_equal(al[:48], np.exp(a).astype(f32)) and np.array_equal(ib[:48], (1.0 / (np.exp(b) + 1e-9)).astype(f32))
    assert (al[48:] == 1).all() and (ib[48:] == 1).all()  # a = b = 0 on the padded channels, whose input is exactly 0
    post = V.packed(path, 6).reshape(7, 32)
    assert np.array_equal(post[:, :24], t["bigvgan.conv_post.weight"][0].T) and not post[:, 24:].any()


def _write(tmp_path, t):
    p = str(tmp_path / "m.bin")
    w = sw.GgmlWriter(p)
    for k, a in t.items():
        w.add(k, a)
    w.close()
    return p


REFUSALS = [("missing", lambda t: t.pop("bigvgan.resblocks.4.activations.3.act.beta")), ("missing", lambda t: t.pop("bigvgan.ups.1.0.bias")),
            ("unknown tensors", lambda t: t.__setitem__("bigvgan.extra", np.zeros(3, f32))),
            ("unknown tensors", lambda t: t.__setitem__("bigvgan.resblocks.0.activations.0.upsample.filter", np.zeros((1, 1, 12), f32))),
            ("wrong shape", lambda t: t.__setitem__("bigvgan.resblocks.1.convs1.0.weight", t["bigvgan.resblocks.1.convs1.0.weight"].reshape(48, 7, 48))),
            ("wrong shape", lambda t: t.__setitem__("bigvgan.activation_post.act.alpha", np.zeros(25, f32))),
            ("wrong shape", lambda t: t.__setitem__("bigvgan.conv_pre.weight", t["bigvgan.conv_pre.weight"][:, :80])),
            ("multiply to 128", lambda t: t.__setitem__("bigvgan.ups.1.0.weight", t["bigvgan.ups.1.0.weight"][:, :, :16])),
            ("multiply to 16", lambda t: [t.pop(k) for k in list(t) if ".ups.1." in k]),
            ("kernel 6", lambda t: t.__setitem__("bigvgan.ups.0.0.weight", t["bigvgan.ups.0.0.weight"][:, :, :6])),
            ("not a BigVGAN model file", lambda t: t.pop("bigvgan.conv_pre.weight"))]


@pytest.mark.parametrize("what,edit", REFUSALS, ids=["%d-%s" % (i, w) for i, (w, _) in enumerate(REFUSALS)])
def test_loader_refusals(tmp_path, what, edit):
    t = dict(R.model("tiny")[1])
    edit(t)
    rc, _, err = V.parse(_write(tmp_path, t))
    assert rc == FMT and what in err, (rc, err)


def test_reader_messages_have_the_shared_shape(tmp_path):
    import model_io_cases as M

    def load(t):
        rc, _, err = V.parse(_write(tmp_path, t))
        return rc, err
    M.reader_messages(load, R.model("tiny")[1], "BigVGAN", "bigvgan.ups.1.0.bias", FMT)
