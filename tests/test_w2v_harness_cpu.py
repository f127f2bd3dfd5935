"""CPU: what pins the aligner's kernel harness (tests/w2v_cases.py, tortoise.cpp_amd/testlib/w2v_harness.hip) without a GPU. The harness refuses every invalid
case before any HIP call and builds the tables aligner_run builds; the float64 references equal torch.nn.functional restatements; a float32 restatement of each
kernel in another summation order sits inside the derived bound on every case; each seeded defect of the reference falls well outside on some case; the
loader's repack feeds the kernels the layouts they index."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aligner_ref as R
import w2v_cases as K

CASES = K.all_cases()


def _base(kind):
    return {K.STATS: K.make(K.STATS, [100]), K.STEM: K.make(K.STEM, [100, 30], 64), K.LN: K.make(K.LN, [5, 3], 64, mode=1),
            K.POS: K.make(K.POS, [70, 3], 128, 64, taps=8), K.HEAD: K.make(K.HEAD, [9, 2], 128, 29, mode=1)}[kind]


def test_every_case_of_the_matrix_is_valid_and_small():
    assert len(CASES) == len(set(c.name() for c in CASES))
    for c in CASES:
        assert K.validate(c) == 0, c.name()
        assert c.rows * max(c.C, c.C2, 1) <= 1 << 21
    for kind in K.KIND_NAMES:
        assert any(c.kind == kind and c.ns >= 2 for c in CASES) and any(c.kind == kind and c.ns == 1 for c in CASES)
    assert {c.taps % 2 for c in CASES if c.kind == K.POS} == {0, 1} and any(c.C2 % 32 for c in CASES if c.kind == K.HEAD)


@pytest.mark.parametrize("kind,override", K.INVALID, ids=["%s %s" % (K.KIND_NAMES[k], " ".join("%s=%s" % kv for kv in o.items())) for k, o in K.INVALID])
def test_invalid_cases_are_refused_before_any_hip_call(kind, override):
    assert K.validate(_base(kind)) == 0
    assert K.validate(_base(kind), **override) == K.HIP_INVALID_VALUE


def test_invalid_layouts_are_refused():
    p = lambda a: a.ctypes.data_as(K.C.c_void_p)  # noqa: E731
    c = _base(K.LN)
    for start in ([8, 8], [4, 24], [16, 8], [8, c.rows]):  # overlap, not a multiple of 8, out of order, outside the buffer
        a = np.array(start, K.i32)
        assert K.validate(c, start=p(a)) == K.HIP_INVALID_VALUE, start
    for n in ([0, 3], [5, c.rows + 1]):
        a = np.array(n, K.i32)
        assert K.validate(c, n=p(a)) == K.HIP_INVALID_VALUE, n
    short = np.array([100, 9], K.i32)  # a stem clip below one frame
    assert K.validate(_base(K.STEM), n=p(short)) == K.HIP_INVALID_VALUE


def test_tables_are_aligner_runs():
    L = K.harness()
    assert (L.tts_w2v_test_stat_tile(), L.tts_w2v_test_stem_tile(), L.tts_w2v_test_pos_tile(), L.tts_w2v_test_head_tile()) == (K.ST_TILE, K.STEM_TILE, K.POS_TILE, K.HEAD_TILE)
    for c in CASES:
        g, g2 = K._buffers(c)
        s, keep = K.struct(c, g.raw, None if g2 is None else g2.raw)
        tin, tout = np.zeros((c.ns, K.SEQ), K.i32), np.zeros((c.ns, K.SEQ), K.i32)
        assert L.tts_w2v_test_table(K.C.byref(s), tin.ctypes.data_as(K.C.c_void_p), tout.ctypes.data_as(K.C.c_void_p)) == 0
        assert np.array_equal(tin, c.table()), c.name()
        if c.kind == K.STEM:
            assert np.array_equal(tout, c.table(out=True)), c.name()


def test_references_against_torch():
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()  # noqa: E731
    for c in CASES:
        for s, (ref, bound) in enumerate(K.reference(c)):
            x = t64(c.a["in_"][c.clip(s)])
            assert (bound > 0).all()
            if c.kind == K.STATS:
                want = np.array([x.mean().item(), (1 / torch.sqrt(x.var() + 1e-7)).item()])
            elif c.kind == K.STEM:
                mean, r = c.a["stat"][s]
                xn = ((x - mean) * float(np.float32(r))).view(1, 1, -1)
                want = F.conv1d(xn, t64(c.a["w"]).unsqueeze(1), t64(c.a["bias"]), stride=c.stride)[0].T.numpy()
            elif c.kind == K.LN:
                v = x if c.mode == 2 else F.layer_norm(x, (c.C,), t64(c.a["gamma"]), t64(c.a["beta"]), 1e-5)
                want = (F.gelu(v) if c.mode else v).numpy()
            elif c.kind == K.POS:
                G, Kt, cg = c.C // c.C2, c.taps, c.C2
                w = t64(c.a["w"]).permute(0, 3, 2, 1).reshape(c.C, cg, Kt)  # [g][tap][ci][co] -> PyTorch's [g cg + co][ci][tap]
                pos = F.conv1d(x.T.unsqueeze(0), w, t64(c.a["bias"]), padding=Kt // 2, groups=G)
                pos = pos[:, :, :-1] if Kt % 2 == 0 else pos
                want = (x + F.gelu(pos[0].T)).numpy()
            else:
                want = F.linear(x, t64(c.a["w"]).T, t64(c.a["bias"])).numpy()
            assert np.abs(ref - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), (c.name(), s)


@pytest.mark.parametrize("c", CASES, ids=[c.name() for c in CASES])
def test_float32_restatement_inside_the_bound(c):
    worst = 0.0
    for s, (ref, bound) in enumerate(K.reference(c)):
        got = K.emulate(c, s)
        ok, r = K.judge(got, ref, bound)
        worst = max(worst, r)
        assert ok, "%s clip %d: %.3f of the bound" % (c.name(), s, r)
        if c.kind == K.HEAD:
            assert K.ids_accept(c, np.argmax(got, axis=1), ref, bound)
            if c.fam == "exact":
                assert np.array_equal(got.astype(np.float64), ref)
    print("%s: float32 restatement at %.3f of the bound" % (c.name(), worst))


@pytest.mark.parametrize("kind,mut", [(k, m) for k, ms in K.DEFECTS.items() for m in ms], ids=["%s %s" % (K.KIND_NAMES[k], m) for k, ms in K.DEFECTS.items() for m in ms])
def test_seeded_defects_fall_outside(kind, mut):
    worst = 0.0
    for c in CASES:
        if c.kind != kind:
            continue
        for s, ((ref, bound), (bad, _)) in enumerate(zip(K.reference(c), K.reference(c, mut))):
            if kind == K.HEAD:  # the defect is in the choice of the id: it must be refused on a case with ties
                if not K.ids_accept(c, K.ref_ids(ref, mut), ref, bound):
                    worst = np.inf
                assert K.ids_accept(c, K.ref_ids(ref), ref, bound)
                continue
            worst = max(worst, K.judge(bad, ref, bound)[1])
    print("%s %s: %.3g bounds out on its worst case" % (K.KIND_NAMES[kind], mut, worst))
    assert worst > 10


def test_repack_feeds_the_kernels(tmp_path):
    for name, cfg in R.CONFIGS.items():
        path, t = R.model(name)
        rc, arch, msg = K.parse(path)
        assert rc == 0, msg
        assert list(arch) == [cfg["N"], cfg["C"], cfg["D"], cfg["K"], cfg["D"] // cfg["G"], cfg["depth"], cfg["FF"], cfg["V"], cfg["H"], cfg["blank"]]
        Cc, Dm, Kt, cg, V = cfg["C"], cfg["D"], cfg["K"], cfg["D"] // cfg["G"], cfg["V"]
        p = "aligner.feature_extractor.conv_layers."
        assert np.array_equal(K.packed(path, 0, 0), t[p + "0.conv.weight"].reshape(-1))                                          # the stem keeps [C][1][k]
        assert np.array_equal(K.packed(path, 0, 1).reshape(cfg["k"][1], Cc, Cc), t[p + "1.conv.weight"].transpose(2, 1, 0))      # [tap][cin][cout]
        assert np.array_equal(K.packed(path, 1).reshape(Cc, Dm), t["aligner.feature_projection.projection.weight"].T)
        w = t["aligner.encoder.pos_conv_embed.conv.weight"].reshape(Dm // cg, cg, cg, Kt)                                        # [g][co][ci][tap]
        assert np.array_equal(K.packed(path, 2).reshape(Dm // cg, Kt, cg, cg), w.transpose(0, 3, 2, 1))                           # [g][tap][ci][co]
        e = "aligner.encoder.layers.1.attention."
        qkv = K.packed(path, 3, 1).reshape(Dm, 3 * Dm)
        for j, nm in enumerate(("q_proj", "k_proj", "v_proj")):
            assert np.array_equal(qkv[:, j * Dm:(j + 1) * Dm], t[e + nm + ".weight"].T)
            assert np.array_equal(K.packed(path, 4, 1)[j * Dm:(j + 1) * Dm], t[e + nm + ".bias"])
        assert np.array_equal(K.packed(path, 5, 1).reshape(Dm, Dm), t[e + "out_proj.weight"].T)
        assert np.array_equal(K.packed(path, 6, 0).reshape(Dm, cfg["FF"]), t["aligner.encoder.layers.0.feed_forward.intermediate_dense.weight"].T)
        assert np.array_equal(K.packed(path, 7, 0).reshape(cfg["FF"], Dm), t["aligner.encoder.layers.0.feed_forward.output_dense.weight"].T)
        assert np.array_equal(K.packed(path, 8).reshape(Dm, V), t["aligner.lm_head.weight"].T)
    rc, arch, msg = K.parse(str(tmp_path / "nowhere.bin"))
    assert rc < 0 and msg


def test_level_tables_against_an_independent_spelling():
    """w2v_levels, the function aligner_run and the harness both call, against tests/model_io_cases.levels: a one-row clip, a clip across a ceil8 boundary, a
    clip that ends as one frame, a clip with a second statistics tile; the tile start and the first sample on level 0 only."""
    import model_io_cases as M
    L = K.harness()
    p = lambda a: a.ctypes.data_as(K.C.c_void_p)  # noqa: E731
    for n, k, s in (((1, 9, 257), (1, 1), (3, 2)), ((5, 9, K.ST_TILE + 1), (3, 2), (2, 2)), ((400, 16000), (10, 3, 3, 2), (5, 2, 2, 2))):
        N = len(k)
        tab, rows, tiles, max_n = np.zeros((N + 1, len(n), K.SEQ), K.i32), np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64), np.zeros(N + 1, K.i32)
        assert L.tts_w2v_test_levels(p(np.array(n, K.i32)), len(n), N, p(np.array(k, K.i32)), p(np.array(s, K.i32)), p(tab), p(rows), p(tiles), p(max_n)) == 0
        want = M.levels(n, lambda v, l: 0 if v < k[l] else (v - k[l]) // s[l] + 1, N + 1, 8, K.ST_TILE, False)
        assert np.array_equal(tab, want[0]) and np.array_equal(rows, want[1]) and tiles[0] == want[2][0] and np.array_equal(max_n, want[3]), (n, tab, want)
        if n[0] == 5:
            assert tab[2, 0, 1] == 1 and tab[0, 2, 3] == 2 and not tab[1:, :, 3:5].any()


def test_reader_messages_have_the_shared_shape(tmp_path):
    import model_io_cases as M
    from tortoise_cpp_amd import synth_weights as sw

    def load(t):
        w = sw.GgmlWriter(str(tmp_path / "m.bin"))
        for name, a in t.items():
            w.add(name, a)
        w.close()
        rc, _, msg = K.parse(str(tmp_path / "m.bin"))
        return rc, msg
    M.reader_messages(load, R.model(next(iter(R.CONFIGS)))[1], "aligner", "aligner.lm_head.bias", -3)
