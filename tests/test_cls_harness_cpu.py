"""CPU: what tests/test_cls_kernels_gpu.py relies on, checked without a device: the harness refuses every invalid case before any HIP call and builds the tables
classifier_run builds; the float32 restatement of every kernel stays inside the bounds derived from the operands (tests/cls_cases.py) on every case of the matrix;
every seeded defect leaves them on some case; the loader's host half reads the configuration and repacks the weights as the kernels index them."""
import ctypes as C

import numpy as np
import pytest

import classifier_ref as R
import cls_cases as K

CASES = K.all_cases()


def test_library_constants_and_tables():
    L = K.harness()
    assert (L.tts_cls_test_gn_tile(), L.tts_cls_test_down_tile(), L.tts_cls_test_stem_tile()) == (K.GN_TILE, K.DOWN_TILE, K.STEM_TILE)
    assert [L.tts_cls_test_groups(c) for c in (8, 16, 24, 32, 64, 128, 512, 1024)] == [K.groups(c) for c in (8, 16, 24, 32, 64, 128, 512, 1024)] == [8, 8, 8, 16, 16, 32, 32, 32]
    for c in CASES:
        assert K.validate(c) == 0, c.name()
        g = K.Guarded(c.out_shape())
        s, keep = K.struct(c, g.raw)
        tin, tout = np.zeros((c.ns, K.SEQ), np.int32), np.zeros((c.ns, K.SEQ), np.int32)
        assert L.tts_cls_test_table(C.byref(s), tin.ctypes.data_as(C.c_void_p), tout.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(tin, c.table()), c.name()
        if c.kind == K.DOWN:
            assert np.array_equal(tout, c.table(out=True)), c.name()


INVALID = [("kind", dict(kind=7)), ("no clips", dict(ns=0)), ("too many clips", dict(ns=5)), ("rows not a multiple of 8", dict(rows=100)), ("rows past the cap", dict(rows=8192)),
           ("buffer too small", dict(rows=8)), ("channels not a power of two", dict(C=96)), ("channels below 32", dict(C=16)), ("channels above 1024", dict(C=2048)),
           ("null input", dict(in_=None)), ("null output", dict(out=None)), ("null lengths", dict(n=None))]


@pytest.mark.parametrize("what,edit", INVALID, ids=[w for w, _ in INVALID])
def test_invalid_cases_are_refused_before_any_hip_call(what, edit):
    c = K.make(K.GN, (5, 300), 32)
    assert K.validate(c) == 0
    assert K.validate(c, **edit) == K.HIP_INVALID_VALUE
    g = K.Guarded(c.out_shape())
    s, keep = K.struct(c, g.raw, **edit)
    before = g.raw.copy()
    assert K.harness().tts_cls_test_run(C.byref(s)) == K.HIP_INVALID_VALUE and np.array_equal(g.raw, before)  # refused by the same rule, nothing written


def test_invalid_layouts_and_operands_are_refused():
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    c = K.make(K.DOWN, (9, 40), 32, 64)
    assert K.validate(c) == 0
    for start in ([8, 20], [8, 16], [24, 8], [8, 4000]):  # unaligned, overlapping, out of order, outside the buffer
        a = np.array(start, np.int32)
        assert K.validate(c, start=p(a)) == K.HIP_INVALID_VALUE, start
    for start in ([8, 20], [8, 8], [24, 8], [8, 4000]):  # the same on the output side, whose clips have 3 and 10 rows
        a = np.array(start, np.int32)
        assert K.validate(c, start_out=p(a)) == K.HIP_INVALID_VALUE, start
    zero = np.array([9, 0], np.int32)
    assert K.validate(c, n=p(zero)) == K.HIP_INVALID_VALUE
    for edit in (dict(C2=96), dict(C2=32), dict(C2=4096), dict(taps=4), dict(taps=13), dict(stride=1), dict(stride=7), dict(rows_out=4), dict(rows_out=8), dict(w=None),
                 dict(bias=None)):
        assert K.validate(c, **edit) == K.HIP_INVALID_VALUE, edit
    for kind, edits in ((K.STEM, (dict(w=None), dict(bias=None))), (K.GN, (dict(gamma=None), dict(beta=None))), (K.HEAD, (dict(w=None), dict(bias=None))),
                        (K.ATTN, (dict(heads=0), dict(heads=3), dict(heads=1), dict(heads=8)))):
        cc = K.make(kind, (5, 9), 256)
        assert K.validate(cc) == 0
        for edit in edits:
            assert K.validate(cc, **edit) == K.HIP_INVALID_VALUE, (kind, edit)


@pytest.mark.parametrize("c", CASES, ids=[c.name() for c in CASES])
def test_float32_restatement_stays_inside_the_bounds(c):
    worst = 0.0
    for s, (ref, bound) in enumerate(K.reference(c)):
        ok, r = K.judge(K.emulate(c, s), ref, bound)
        worst = max(worst, r)
        assert ok, (c.name(), s, r)
    print("%s: float32 restatement at %.3f of the bound" % (c.name(), worst))


DEFECT_IDS = [(k, m) for k in sorted(K.DEFECTS) for m in K.DEFECTS[k]]


@pytest.mark.parametrize("kind,mut", DEFECT_IDS, ids=["%s-%s" % (K.KIND_NAMES[k], m) for k, m in DEFECT_IDS])
def test_seeded_defects_fall_outside(kind, mut):
    hit = []
    for c in CASES:
        if c.kind != kind or (mut == "groups32" and c.C != 32):
            continue
        good, bad = K.reference(c), K.reference(c, mut)
        for s in range(c.ns):
            if not K.judge(np.asarray(bad[s][0]), good[s][0], good[s][1])[0]:
                hit.append((c.name(), s))
    print("%s / %s: outside the bound on %d clips" % (K.KIND_NAMES[kind], mut, len(hit)))
    assert hit
    if mut in ("unbiased", "eps_outside", "silu_first", "groups32", "scale_once"):  # these move every clip with more than one row
        n_multi = sum(1 for c in CASES if c.kind == kind and (mut != "groups32" or c.C == 32) for v in c.n if v > 1)
        assert len(hit) >= n_multi


def test_offset_case_is_what_it_says():
    c = [c for c in K.gn_cases() if c.fam == "offset"][0]
    x = c.a["in_"][c.clip(0)].astype(np.float64)
    assert abs(abs(x.mean()) / x.std() - 100) < 5
    ref, bound = K.reference(c)[0]
    assert np.median(bound) < 3e-6  # the bound stays a float32 bound: the statistics are charged as doubles
    # a float32 one-pass variance, what double partials are there to avoid, leaves it
    xg = c.a["in_"][c.clip(0)].reshape(c.n[0], K.groups(c.C), -1)
    m32 = xg.mean(axis=(0, 2), keepdims=True, dtype=np.float32)
    v32 = (xg * xg).mean(axis=(0, 2), keepdims=True, dtype=np.float32) - m32 * m32
    v = (((xg - m32) / np.sqrt(np.maximum(v32, 0) + np.float32(1e-5))).reshape(c.n[0], c.C) * c.a["gamma"] + c.a["beta"]).astype(np.float32)
    assert not K.judge((v / (1 + np.exp(-v))).astype(np.float32), ref, bound)[0]


def test_loader_host_half_reads_the_configuration_and_repacks():
    for name, cfg in R.CONFIGS.items():
        path, t = R.model(name)
        rc, out, msg = K.parse(path)
        assert rc == 0, msg
        assert list(out) == [cfg["b0"], cfg["depth"], cfg["K"], cfg["E"], cfg["rb"], cfg["attn"], cfg["F"], cfg["H"]]
    path, t = R.model("tiny")
    E, H = 256, 2
    dh = E // H
    assert np.array_equal(K.packed(path, 0), t["classifier.enc.init.weight"].reshape(-1))
    w = t["classifier.enc.res.0.in_layers.2.weight"]  # [cout][cin][k] -> [k][cin][cout]
    assert np.array_equal(K.packed(path, 1, 0).reshape(5, 32, 32), w.transpose(2, 1, 0))
    assert np.array_equal(K.packed(path, 2, 1).reshape(5, 64, 64), t["classifier.enc.res.2.out_layers.3.weight"].transpose(2, 1, 0))
    assert np.array_equal(K.packed(path, 3, 1).reshape(5, 64, 128), t["classifier.enc.res.3.op.weight"].transpose(2, 1, 0))
    assert np.array_equal(K.packed(path, 4).reshape(128, 256), t["classifier.enc.final.2.weight"][:, :, 0].T)
    qw, qb = t["classifier.enc.attn.0.qkv.weight"][:, :, 0], t["classifier.enc.attn.0.qkv.bias"]
    got_w, got_b = K.packed(path, 5, 0).reshape(E, 3 * E), K.packed(path, 6, 0)
    for h in range(H):
        for tq in range(3):  # upstream's channel head * 3 dh + {q, k, v} * dh + d  ->  column {q, k, v} * E + head * dh + d
            old, new = slice(h * 3 * dh + tq * dh, h * 3 * dh + (tq + 1) * dh), slice(tq * E + h * dh, tq * E + (h + 1) * dh)
            assert np.array_equal(got_w[:, new], qw[old].T) and np.array_equal(got_b[new], qb[old])
    assert np.array_equal(K.packed(path, 8, 0).reshape(E, E), t["classifier.enc.attn.0.proj_out.weight"][:, :, 0].T)
    assert np.array_equal(K.packed(path, 7), t["classifier.head.weight"].reshape(-1))
    # the packed projections reproduce the reference's attention block through the kernels' own index forms (float64)
    x = np.random.RandomState(5).randn(9, E)
    qkv = x @ got_w.astype(np.float64) + got_b
    c = K.Case(K.ATTN, [9], E, heads=H, gap=0)
    c.a["in_"] = np.zeros((c.rows, 3 * E), np.float32)
    c.a["in_"][:9] = qkv.astype(np.float32)
    att = K.ref_attn(c, 0)[0]
    ref_qkv = (x @ qw.T.astype(np.float64) + qb).reshape(9, H, 3, dh)
    want = np.zeros((9, E))
    for h in range(H):
        q, k, v = (ref_qkv[:, h, i] for i in range(3))
        s = (q * dh ** -0.25) @ (k * dh ** -0.25).T
        w_ = np.exp(s - s.max(1, keepdims=True))
        want[:, h * dh:(h + 1) * dh] = (w_ / w_.sum(1, keepdims=True)) @ v
    assert np.abs(att - want).max() < 1e-5  # qkv was rounded to float32 on the way


def test_level_tables_against_an_independent_spelling():
    """cls_levels, the function classifier_run and the harness both call, against tests/model_io_cases.levels: a one-row clip, a clip across a ceil8 boundary
    that downsamples to one row, a clip with a second GroupNorm tile; every level carries its tile start and the clip's first sample."""
    import model_io_cases as M
    L = K.harness()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for n, depth, F in (((1, 9, 257), 2, 4), ((257, 1, 9), 1, 2), ((220000, 8), 3, 4)):
        tab, rows, tiles, max_n = np.zeros((depth + 1, len(n), K.SEQ), np.int32), np.zeros(depth + 1, np.int64), np.zeros(depth + 1, np.int64), np.zeros(depth + 1, np.int32)
        assert L.tts_cls_test_levels(p(np.array(n, np.int32)), len(n), depth, F, p(tab), p(rows), p(tiles), p(max_n)) == 0
        want = M.levels(n, lambda v, l: (v - 1) // F + 1, depth + 1, 8, K.GN_TILE, True)
        for got, ref in zip((tab, rows, tiles, max_n), want):
            assert np.array_equal(got, ref), (n, got, ref)
    assert tab[3, 1, 1] == 1 and not (tab[:, :, 0] % 8).any()


def test_reader_messages_have_the_shared_shape(tmp_path):
    import model_io_cases as M
    from tortoise_cpp_amd import synth_weights as sw

    def load(t):
        w = sw.GgmlWriter(str(tmp_path / "m.bin"))
        for k, a in t.items():
            w.add(k, a)
        w.close()
        rc, _, msg = K.parse(str(tmp_path / "m.bin"))
        return rc, msg
    M.reader_messages(load, R.model("tiny")[1], "classifier", "classifier.enc.final.2.bias", -3)
