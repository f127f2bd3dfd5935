"""CPU: what pins the DVAE encoder (tts_load_dvae / tts_dvae_codes / tts_dvae_codes_audio / tts_ar_latents_for_codes, csrc/dvae.h) without a GPU: two
independent float64 restatements agree; a float32 twin in the kernels' operation order stays inside the derived bounds layer by layer and obeys the code rule,
and each seeded defect falls outside; the decided-row condition holds ON THE REFERENCE ALONE for exactly the inputs the GPU tests use; the writer, the loader's
host half and its repack; every refusal a host-only context can reach; exports, header and bindings; the refusal of every invalid harness case. The model is
stated from memory: unpinned against upstream."""
import ctypes as C
import os

import numpy as np
import pytest

import dvae_ref as R
from dvae_ref import sw

ROOT = R.ROOT
FMT, ARG, HIP, STATE, LIMIT = -3, -1, -4, -5, -6


def _write(path, tensors):
    w = sw.GgmlWriter(str(path))
    for k, v in tensors.items():
        w.add(k, v)
    w.close()
    return str(path).encode()


def test_status_codes_are_the_headers():
    txt = open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read()
    for name, v in (("TTS_ERR_ARG", ARG), ("TTS_ERR_FORMAT", FMT), ("TTS_ERR_HIP", HIP), ("TTS_ERR_STATE", STATE), ("TTS_ERR_LIMIT", LIMIT)):
        assert "%s = %d" % (name, v) in txt.replace("  ", " "), name


@pytest.mark.parametrize("frames", [1, 2, 5, 8])
def test_two_float64_restatements_agree(frames):
    t = R.model("mid")[1]
    a, b = R.forward(t, R.mel(frames)), R.forward_loops(t, R.mel(frames))
    assert a["z"].shape == b["z"].shape == (R.rows(frames), 64)
    assert np.abs(a["z"] - b["z"]).max() < 1e-12 * max(1.0, np.abs(a["z"]).max())
    # |z - E_j|^2 = |z|^2 + (|E_j|^2 - 2 z . E_j): the two forms of the distance
    z2 = (a["z"] ** 2).sum(1)[:, None]
    assert np.abs(a["s"] + z2 - b["d"]).max() < 1e-10 * np.abs(b["d"]).max()
    assert np.array_equal(a["codes"], b["codes"])


@pytest.mark.parametrize("frames", R.MID_FRAMES)
def test_float32_twin_inside_the_bounds_layer_by_layer(frames):
    t = R.model("mid")[1]
    layers, codes = R.twin(t, R.mel(frames))
    assert len(layers) == 2 + 9 + 1
    for name, y, want, bound in layers:
        assert y.shape == want.shape and (bound > 0).all(), name
        ratio = (np.abs(y.astype(np.float64) - want) / bound).max()
        assert ratio <= 1.0, "%s: %.2f of its bound" % (name, ratio)
    z = layers[-1][1]
    s, bound = R.vq64(z, t["dvae.codebook.embed"])
    fails, und = R.judge(codes, s, bound)
    assert not fails, fails[:3]
    # the chained result is close to the end-to-end float64 too (the 1e-3 gate the GPU tests hold z to)
    assert np.abs(z - R.reference("mid", frames)["z"]).max() <= R.GATE


# a ReLU on the FIRST block's input changes nothing (the strided layer in front of it ends in one): the defect shows at the second block
LAYER_OF = {"pad": "down0", "drop_last": "down0", "relu_in": "res1.0", "no_skip": "res0.4"}


@pytest.mark.parametrize("defect", sorted(LAYER_OF))
def test_seeded_layer_defects_fall_outside(defect):
    layers, _ = R.twin(R.model("mid")[1], R.mel(65), defect)
    worst = {name: (np.abs(y.astype(np.float64) - want) / bound).max() for name, y, want, bound in layers}
    assert worst[LAYER_OF[defect]] > 100.0, worst


def _tie_problem():
    c, pl = [x for x in R.vq_cases() if x[0].label == "N%d-R%d" % (R.VQ_SLAB + 64, R.VQ_TILE + 1)][0]
    return c.x[0], c.w, pl


def test_code_rule_accepts_the_twin_and_rejects_the_quantiser_defects():
    z, E, pl = _tie_problem()
    s, bound = R.vq64(z, E)
    assert (pl >= 0).sum() >= 3 and list(pl[[3, 5, 6]]) == [37, 70, 130]
    for r in np.nonzero(pl >= 0)[0]:  # exact ties in float64 as well: the duplicate columns are equal bit for bit
        assert (s[r] == s[r].min()).sum() == 2 and s[r].argmin() == pl[r]
    fails, und = R.judge(R.vq32(z, E), s, bound, pl)
    assert not fails and und <= R.MAX_UNDECIDED
    for defect in ("tie_high", "no_e2", "slab_merge"):
        fails, _ = R.judge(R.vq32(z, E, defect), s, bound, pl)
        assert fails, defect
    # a tie broken to the higher index is caught ONLY by the planted rows; a wrong merge by the rows whose winner lies behind the first slab
    assert not R.judge(R.vq32(z, E, "tie_high"), s, bound, None)[0]
    assert np.array_equal(R.code_norms(E), (E.astype(np.float64) ** 2).sum(0).astype(np.float32)) or np.abs(
        R.code_norms(E).astype(np.float64) - (E.astype(np.float64) ** 2).sum(0)).max() <= 2.0 ** -24 * 1.01 * (E.astype(np.float64) ** 2).sum(0).max()


def test_decided_row_condition_on_the_reference_alone():
    """exactly the inputs of the GPU tests: the kernel cases, the ABI's mid-size clips and the full-size clip. A condition, not a measurement: over the cap,
    change the seed or the scale, never the cap."""
    shares = {}
    for c, pl in R.vq_cases() + [R.vq_full_case()]:
        s, bound = R.vq64(c.x[0], c.w)
        _, und = R.judge(s.argmin(1), s, bound, pl)
        shares[c.name()] = und
    for name, frames in [("mid", f) for f in R.MID_FRAMES] + [("full", R.FULL_FRAMES)]:
        ref = R.reference(name, frames)
        _, und = R.judge(ref["codes"], ref["s"], ref["bound"])
        shares["%s-T%d" % (name, frames)] = und
    for i, f in enumerate(R.RAGGED):
        ref = R.reference("mid", f, 1 + i)
        shares["mid-ragged-%d" % i] = R.judge(ref["codes"], ref["s"], ref["bound"])[1]
    print("undecided share of the reference: max %.4f over %d inputs" % (max(shares.values()), len(shares)))
    assert max(shares.values()) <= R.MAX_UNDECIDED, {k: v for k, v in shares.items() if v > R.MAX_UNDECIDED}


def test_end_to_end_margin_leaves_few_rows_out():
    """the end-to-end rule with the float32 twin's z in the kernel's place: its codes are float64's and the rows the margin leaves out stay under the cap"""
    t = R.model("mid")[1]
    for frames in (130, 65):
        ref = R.reference("mid", frames)
        layers, codes = R.twin(t, R.mel(frames))
        fails, out = R.judge_end_to_end(codes, layers[-1][1], ref["z"], ref["s"], ref["bound"], t["dvae.codebook.embed"])
        assert not fails and out <= R.MAX_UNDECIDED, (frames, out, fails[:3])
    # a z that is off by the whole gate on every channel moves the distances by far more than the margin of most rows: the rule then leaves rows out, it does not fail
    ref = R.reference("mid", 130)
    off = (ref["z"] + R.GATE).astype(np.float32)
    assert not R.judge_end_to_end(ref["codes"], off, ref["z"], ref["s"], ref["bound"], t["dvae.codebook.embed"])[0]


def test_writer_round_trip_and_shapes():
    for name, cfg in R.CONFIGS.items():
        path, t = R.model(name)
        want = sw.dvae_tensor_shapes(**cfg)
        assert list(t) == list(want)
        for k, shape in want.items():
            assert t[k].shape == tuple(shape), k
        assert list(t["dvae.config"]) == [cfg["stride"]]
    u = sw.dvae_tensor_shapes()
    assert len(u) == 4 + 3 * 6 + 2 + 1 + 1
    assert u["dvae.encoder.0.0.weight"] == (512, 80, 3) and u["dvae.encoder.1.0.weight"] == (1024, 512, 3)
    assert u["dvae.encoder.2.net.0.weight"] == (1024, 1024, 3) and u["dvae.encoder.4.net.4.weight"] == (1024, 1024, 1)
    assert u["dvae.encoder.5.weight"] == (512, 1024, 1) and u["dvae.codebook.embed"] == (512, 8192)


def test_loader_host_half_and_repack():
    path, t = R.model("mid")
    rc, cfg, err = R.parse(path)
    assert rc == 0 and list(cfg) == [2, 3, 80, 128, 64, 256, 2], (rc, err)
    w = t["dvae.encoder.1.0.weight"]
    assert np.array_equal(R.packed(path, 0, 1).reshape(3, 64, 128), w.transpose(2, 1, 0))
    assert np.array_equal(R.packed(path, 1, 4).reshape(3, 128, 128), t["dvae.encoder.3.net.2.weight"].transpose(2, 1, 0))
    assert np.array_equal(R.packed(path, 2).reshape(128, 64), t["dvae.encoder.5.weight"][:, :, 0].T)
    assert np.array_equal(R.packed(path, 3).reshape(64, 256), t["dvae.codebook.embed"])
    assert np.array_equal(R.packed(path, 4), R.code_norms(t["dvae.codebook.embed"]))  # double, channels ascending, rounded once
    assert R.harness().tts_dvae_test_stem_tile() == R.STEM_TILE and R.harness().tts_dvae_test_down_tile() == R.DOWN_TILE
    assert R.harness().tts_dvae_test_vq_tile() == R.VQ_TILE and R.harness().tts_dvae_test_vq_slab() == R.VQ_SLAB


def test_level_tables_against_an_independent_spelling():
    """dvae_levels, the function dvae_begin and the harness both call, against tests/model_io_cases.levels: a one-frame clip, odd lengths, clips packed without
    gaps, the first mel float (cin x the frames before the clip) on level 0 only."""
    import model_io_cases as M
    L = R.harness()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for n, layers, stride, cin in (((1, 9, 257), 2, 2, 80), ((2, 1, 3), 1, 4, 7), ((16384,), 3, 3, 128)):
        tab, rows, max_n = np.zeros((layers + 1, len(n), M.SEQ), np.int32), np.zeros(layers + 1, np.int64), np.zeros(layers + 1, np.int32)
        assert L.tts_dvae_test_levels(p(np.array(n, np.int32)), len(n), layers, stride, cin, p(tab), p(rows), p(max_n)) == 0
        want = M.levels(n, lambda v, l: (v - 1) // stride + 1, layers + 1, 1, 0, False, cin)
        assert np.array_equal(tab, want[0]) and np.array_equal(rows, want[1]) and np.array_equal(max_n, want[3]), (n, tab, want)
        if len(n) == 3:
            assert tab[0, 2, 4] == cin * (n[0] + n[1]) and not tab[:, :, 3].any() and not tab[1:, :, 4].any()
        if (layers, stride) == (2, 2):
            assert [R.rows(v) for v in n] == list(tab[2, :, 1])


def test_reader_messages_have_the_shared_shape(tmp_path):
    """The DVAE reads its sizes off the tensors, so a bias of another length is refused in its own words (BROKEN below); the rest is ModelReader's."""
    import model_io_cases as M

    def load(t):
        rc, _, msg = R.parse(_write(tmp_path / "m.bin", t).decode())
        return rc, msg
    M.reader_messages(load, R.model("mid")[1], "DVAE", "dvae.encoder.3.net.2.bias", FMT, extent=False)


BROKEN = [("'dvae.encoder.1.0.bias' missing", lambda t: t.pop("dvae.encoder.1.0.bias")),
          ("'dvae.codebook.embed' missing", lambda t: t.pop("dvae.codebook.embed")),
          ("unknown tensors", lambda t: t.__setitem__("dvae.decoder.0.weight", np.zeros(3, np.float32))),
          ("unknown tensors", lambda t: t.__setitem__("dvae.codebook.cluster_size", np.zeros(256, np.float32))),
          ("an odd kernel size", lambda t: t.__setitem__("dvae.encoder.0.0.weight", np.zeros((64, 80, 4), np.float32))),
          ("the layer before it writes 64", lambda t: t.__setitem__("dvae.encoder.1.0.weight", np.zeros((128, 96, 3), np.float32))),
          ("a multiple of 64", lambda t: (t.__setitem__("dvae.encoder.0.0.weight", np.zeros((48, 80, 3), np.float32)), t.__setitem__("dvae.encoder.0.0.bias", np.zeros(48, np.float32)))),
          ("mel channels", lambda t: t.__setitem__("dvae.encoder.0.0.weight", np.zeros((64, 129, 3), np.float32))),
          ("the residual stream has 128", lambda t: (t.__setitem__("dvae.encoder.2.net.0.weight", np.zeros((64, 128, 3), np.float32)), t.__setitem__("dvae.encoder.2.net.0.bias", np.zeros(64, np.float32)))),
          ("got 127 values", lambda t: t.__setitem__("dvae.encoder.3.net.4.bias", np.zeros(127, np.float32))),
          ("the last convolution has 3 taps", lambda t: t.__setitem__("dvae.encoder.5.weight", np.zeros((64, 128, 3), np.float32))),
          ("the codebook dim a multiple of 32", lambda t: (t.__setitem__("dvae.encoder.5.weight", np.zeros((48, 128, 1), np.float32)), t.__setitem__("dvae.encoder.5.bias", np.zeros(48, np.float32)))),
          ("expected [64][tokens]", lambda t: t.__setitem__("dvae.codebook.embed", np.zeros((32, 256), np.float32))),
          ("tokens (a multiple of 32", lambda t: t.__setitem__("dvae.codebook.embed", np.zeros((64, 250), np.float32))),
          ("non-finite", lambda t: t.__setitem__("dvae.codebook.embed", np.full((64, 256), np.nan, np.float32))),
          ("stride 5", lambda t: t.__setitem__("dvae.config", np.array([5], np.float32))),
          ("{stride}, one integer", lambda t: t.__setitem__("dvae.config", np.array([2.5], np.float32)))]


def test_refusals_on_a_host_only_context(pkg, small_models, tmp_path):
    """The loader parses before it asks for the device: broken files are TTS_ERR_FORMAT even here, a good file and every device call TTS_ERR_HIP."""
    e = pkg.Engine(-1)
    L, h = e.L, e.h
    err = lambda: L.tts_last_error(h).decode()  # noqa: E731
    tensors = R.model("mid")[1]
    for what, edit in BROKEN:
        t = dict(tensors)
        edit(t)
        assert L.tts_load_dvae(h, _write(tmp_path / "bad.bin", t)) == FMT and what in err(), (what, err())
    assert L.tts_load_dvae(h, (small_models + "/ggml-vocoder-model.bin").encode()) == FMT and "is not a DVAE model file" in err()
    assert L.tts_load_dvae(h, str(tmp_path / "nowhere.bin").encode()) in (-2, FMT)
    assert L.tts_load_dvae(h, None) == ARG and L.tts_load_dvae(None, R.model("mid")[0].encode()) == ARG
    t = dict(tensors)
    del t["dvae.config"]  # optional: stride 2
    assert L.tts_load_dvae(h, _write(tmp_path / "noconfig.bin", t)) == HIP
    assert L.tts_load_dvae(h, R.model("mid")[0].encode()) == HIP and "host-only" in err()
    assert L.tts_dvae_tokens(h) == 0 and L.tts_dvae_dim(h) == 0 and L.tts_dvae_tokens(None) == 0
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    m, fr = np.zeros(80 * 10, np.float32), np.array([10], np.int32)
    codes, nc, z = np.full(8, 7, np.int32), np.full(1, 7, np.int32), np.full(8 * 64, 7, np.float32)
    assert L.tts_dvae_codes(h, p(m), p(fr), 1, p(codes), p(nc), 8, p(z)) == HIP and "host-only" in err()
    assert L.tts_dvae_codes(None, p(m), p(fr), 1, p(codes), p(nc), 8, p(z)) == ARG
    x, n, r = np.zeros(3000, np.float32), np.array([3000], np.int64), np.array([22050], np.int32)
    assert L.tts_dvae_codes_audio(h, p(x), p(n), p(r), 1, None, p(codes), p(nc), 8, p(z)) == HIP
    assert L.tts_dvae_codes_audio(None, p(x), p(n), p(r), 1, None, p(codes), p(nc), 8, p(z)) == ARG
    ids, voice, rows, lat = np.array([1, 2, 3], np.int32), np.zeros(1024, np.float32), np.full(1, 7, np.int32), np.full(1024, 7, np.float32)
    assert L.tts_ar_latents_for_codes(h, p(ids), 3, p(voice), p(codes), 8, p(rows), p(lat)) == HIP
    assert L.tts_ar_latents_for_codes(None, p(ids), 3, p(voice), p(codes), 8, p(rows), p(lat)) == ARG
    assert (codes == 7).all() and nc[0] == 7 and (z == 7).all() and rows[0] == 7 and (lat == 7).all(), "a refused call wrote its output"
    e.close()


def test_rows_is_pure_and_matches_the_reference(pkg):
    L = pkg.lib()
    assert L.tts_dvae_rows(0) == ARG and L.tts_dvae_rows(-3) == ARG
    for f in list(range(1, 40)) + [R.FULL_FRAMES, 793, 1723, 16384]:
        assert L.tts_dvae_rows(f) == R.rows(f) == L.tts_cvvp_rows(f) == pkg.Engine.dvae_rows(f)
    for f in R.MID_FRAMES:
        assert R.reference("mid", f)["codes"].shape == (R.rows(f),)


def test_header_exports_and_bindings(pkg):
    names = pkg.header_symbols()
    for n in ("tts_load_dvae", "tts_dvae_rows", "tts_dvae_tokens", "tts_dvae_dim", "tts_dvae_codes", "tts_dvae_codes_audio", "tts_ar_latents_for_codes"):
        assert n in names and hasattr(pkg.lib(), n), n
    for n in ("load_dvae", "dvae_codes", "dvae_codes_audio", "ar_latents_for_codes", "dvae_rows"):
        assert hasattr(pkg.Engine, n), n
    for n in ("dvae_tensor_shapes", "dvae_tensors", "write_dvae"):
        assert hasattr(sw, n), n
    txt = open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read()
    assert "#define TTS_API_VERSION 8" in txt.replace("  ", " ") and "#define TTS_DVAE_MAX_CLIPS 256" in txt and "#define TTS_DVAE_MAX_FRAMES 16384" in txt


# ---- the kernel harness ----
def test_every_case_of_the_matrix_is_valid_and_small():
    cases = R.stem_cases() + R.down_cases() + [c for c, _ in R.vq_cases()] + [R.vq_full_case()[0]]
    assert len(cases) == len(set(c.name() for c in cases))
    for c in cases:
        assert c.validate() == 0, c.name()
    assert sorted(int(c.n[0]) for c in R.stem_cases() if len(c.n) == 1 and c.cin == 80) == [1, 2, 3, 4, 63, 64, 65]
    assert sorted(int(c.n[0]) for c in R.down_cases() if len(c.n) == 1) == [1, 2, 3, 127, 128, 129]
    T, S = R.VQ_TILE, R.VQ_SLAB
    assert sorted(set((c.cout, c.rows) for c, _ in R.vq_cases())) == sorted((n, r) for n in (128, 192, S + 64) for r in (1, T - 1, T, T + 1, 2 * T + 1))
    full = R.vq_full_case()[0]
    assert (full.cin, full.cout, full.rows) == (512, 8192, T + 1)


INVALID = [(R.STEM, dict(kind=3)), (R.STEM, dict(ns=0)), (R.STEM, dict(ns=5)), (R.STEM, dict(cin=0)), (R.STEM, dict(cin=129)), (R.STEM, dict(cout=48)),
           (R.STEM, dict(cout=8192)), (R.STEM, dict(taps=4)), (R.STEM, dict(taps=9)), (R.STEM, dict(stride=0)), (R.STEM, dict(stride=5)), (R.STEM, dict(rows=38)),
           (R.STEM, dict(rows_out=19)), (R.STEM, dict(out=None)), (R.STEM, dict(in_=None)), (R.STEM, dict(w=None)), (R.STEM, dict(bias=None)), (R.STEM, dict(n=None)),
           (R.DOWN, dict(cin=48)), (R.DOWN, dict(cin=80)), (R.DOWN, dict(cout=96)), (R.DOWN, dict(rows=134)), (R.DOWN, dict(rows_out=66)), (R.DOWN, dict(stride=5)),
           (R.VQ, dict(rows=0)), (R.VQ, dict(rows=(1 << 12) + 1)), (R.VQ, dict(cin=48)), (R.VQ, dict(cin=544)), (R.VQ, dict(cout=100)), (R.VQ, dict(cout=0)),
           (R.VQ, dict(cout=65536 + 32)), (R.VQ, dict(ns=2)), (R.VQ, dict(out2=None)), (R.VQ, dict(w=None))]


def _base(kind):
    return {R.STEM: R.stem_cases()[7], R.DOWN: R.down_cases()[6], R.VQ: R.vq_cases()[3][0]}[kind]


@pytest.mark.parametrize("kind,override", INVALID, ids=["%d %s" % (k, " ".join("%s=%s" % kv for kv in o.items())) for k, o in INVALID])
def test_invalid_cases_are_refused_before_any_hip_call(kind, override):
    assert _base(kind).validate() == 0
    assert _base(kind).validate(**override) == R.HIP_INVALID_VALUE


def test_invalid_clip_lengths_are_refused():
    c = _base(R.STEM)
    for n in ([0, 4], [35, 5], [35, -1]):
        a = np.array(n, np.int32)
        assert c.validate(n=a.ctypes.data_as(C.c_void_p)) == R.HIP_INVALID_VALUE, n


# ---- the converter ----
def _state_dict():
    """the model file as upstream's state dict holds it: no dvae. prefix, the decoder and the EMA buffers present"""
    import torch
    sd = {k[len("dvae."):]: torch.from_numpy(v.copy()) for k, v in R.model("mid")[1].items() if k != "dvae.config"}
    sd["decoder.0.0.weight"] = torch.zeros(64, 64, 3)
    sd["decoder.6.bias"] = torch.zeros(80)
    sd["codebook.cluster_size"] = torch.zeros(256)
    sd["codebook.embed_avg"] = torch.zeros(64, 256)
    sd["codebook.initted"] = torch.ones(1)
    return sd


def _convert(tmp_path, sd, extra=(), expect_ok=True):
    import subprocess
    import sys
    import torch
    src = tmp_path / "dvae.pth"
    torch.save(sd, str(src))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--dvae", str(src), "--out", str(tmp_path / "out")] + list(extra),
                       capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == expect_ok, r.stdout + r.stderr
    return r


def test_converter_round_trip(tmp_path):
    r = _convert(tmp_path, _state_dict())
    assert "2 strided layers, 3 ResBlocks of 128 channels, codebook 64 x 256 tokens" in r.stdout
    got, want = sw.read_ggml(str(tmp_path / "out" / "ggml-dvae-model.bin")), R.model("mid")[1]
    assert list(got) == list(want)  # the decoder and the EMA buffers are dropped
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert R.parse(str(tmp_path / "out" / "ggml-dvae-model.bin"))[0] == 0
    _convert(tmp_path, _state_dict(), ["--dvae-stride", "3"])
    assert list(sw.read_ggml(str(tmp_path / "out" / "ggml-dvae-model.bin"))["dvae.config"]) == [3]


def test_converter_refusals(tmp_path):
    import subprocess
    import sys
    import torch
    sd = _state_dict()
    bad = dict(sd)
    bad["encoder.extra.weight"] = torch.zeros(3)
    assert "unexpected tensor 'encoder.extra.weight'" in _convert(tmp_path, bad, (), False).stderr
    bad = dict(sd)
    del bad["encoder.3.net.2.bias"]
    assert "'encoder.3.net.2.bias' is missing" in _convert(tmp_path, bad, (), False).stderr
    bad = dict(sd)
    bad["encoder.5.bias"] = torch.zeros(65)
    assert "'encoder.5.bias' has shape" in _convert(tmp_path, bad, (), False).stderr
    bad = dict(sd)
    del bad["codebook.embed"]
    assert "not a DiscreteVAE state dict" in _convert(tmp_path, bad, (), False).stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--list-expected", "dvae"], capture_output=True, text=True, timeout=120)
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("dvae ")]
    assert r.returncode == 0 and len(rows) == 25 and ["dvae", "codebook.embed", "512x8192"] in rows
    assert rows == [["dvae", k[len("dvae."):], "x".join(map(str, s))] for k, s in sw.dvae_tensor_shapes(config=False).items()]


# ---- the CLI's usage errors: exit 1 with a usage message, before a model is loaded ----
def _wav(pkg, path, seconds, rate=22050):
    n = int(seconds * rate)
    x = (0.1 * np.sin(np.arange(n) * 0.05)).astype(np.float32)
    assert pkg.lib().tts_write_wav(str(path).encode(), x, n, rate) == 0
    return str(path)


CLI_ERRORS = [(["--revoice", "IN"], "--revoice needs --dvae"), (["--codes-from", "IN"], "--codes-from needs --dvae"),
              (["--codes-out", "x.txt", "--dvae", "d.bin"], "--codes-out needs --codes-from"),
              (["--revoice", "IN", "--dvae", "d.bin", "--split-text", "100"], "cannot be combined with --split-text"),
              (["--revoice", "IN", "--dvae", "d.bin", "--candidates", "2"], "cannot be combined with --candidates > 1"),
              (["--revoice", "IN", "--dvae", "d.bin", "--voice", "a.bin", "--voice", "b.bin"], "cannot be combined with several voices"),
              (["--revoice", "IN", "--dvae", "d.bin", "--stream", "--decoder", "hifigan"], "cannot be combined with --stream"),
              (["--revoice", "IN", "--dvae", "d.bin", "--clvp", "c.bin"], "cannot be combined with --clvp / --cvvp"),
              (["--revoice", "IN", "--dvae", "d.bin", "--devices", "2"], "--devices > 1 or --exchange rccl"),
              (["--revoice", "IN", "--dvae", "d.bin", "--codes-from", "IN"], "cannot be combined with --codes-from"),
              (["--revoice", "IN", "--dvae", "d.bin", "--dry-run", "1"], "cannot be combined with --dry-run 1"),
              (["--codes-from", "IN", "--dvae", "d.bin", "--dry-run", "1"], "cannot be combined with --dry-run 1"),
              (["--revoice", "LONG", "--dvae", "d.bin"], "codes, at most 500"), (["--revoice", "nowhere.wav", "--dvae", "d.bin"], "not a readable RIFF WAV"),
              (["--codes-from", "nowhere.wav", "--dvae", "d.bin"], "not a readable RIFF WAV")]


@pytest.mark.parametrize("extra,what", CLI_ERRORS, ids=[" ".join(e) for e, _ in CLI_ERRORS])
def test_cli_usage_errors(pkg, tmp_path, extra, what):
    import subprocess
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    short, long_ = _wav(pkg, tmp_path / "in.wav", 1.0), _wav(pkg, tmp_path / "long.wav", 24.0)  # 24 s: 517 codes
    extra = [{"IN": short, "LONG": long_}.get(e, e) for e in extra]
    r = subprocess.run([exe, "--models", str(tmp_path / "nowhere"), "--message", "hello there", "--output", str(tmp_path / "o.wav")] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and what in r.stderr, r.stderr
    assert ("usage:" in r.stderr or "not a readable" in r.stderr) and "model_load" not in r.stderr and not (tmp_path / "o.wav").exists()  # before a model is loaded
    assert R.rows(int(24.0 * 22050) // 256 + 1) == 517
