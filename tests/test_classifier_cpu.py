"""CPU side of the synthesized-speech classifier (csrc/classifier.h): what pins a stage whose upstream source and weights are not available offline.

  - two float64 spellings of the network, upstream's literal torch form and the index form the kernels implement (tests/classifier_ref.py), agree to 1e-12;
  - a float32 restatement of the whole network stays within 1e-4 of float64 on every weight and clip pair tests/test_classifier_gpu.py uses (what makes its
    1e-3 gate on the logits meaningful), and those logits are of order 1;
  - seeded defects of the network move the logits by more than the gate;
  - tts_classifier_positions against the formula; the writer, the converter, every refusal of tts_load_classifier and tts_classify_audio that a host-only
    context can reach, the CLI's usage errors, the exported, declared and bound symbols.
Unpinned against upstream, unjudged on real audio."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classifier_ref as R
from tortoise_cpp_amd import synth_weights as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(name, n) for name in ("tiny", "upstream") for n in R.GPU_SAMPLES[name]]
ARG, FMT, HIP = -1, -3, -4


@pytest.mark.parametrize("name,n", [("tiny", 1), ("tiny", 5), ("tiny", 1000), ("tiny", 4097), ("upstream", 1025)], ids=lambda v: str(v))
def test_two_float64_spellings_agree(name, n):
    t, x = R.model(name)[1], R.wave(name, n)
    a, b = R.index(t, x), R.literal(t, x)
    assert a.shape == b.shape == (2,) and a.dtype == b.dtype == np.float64
    print("%s n = %d: index form against the literal torch form: %.1e (logits %s)" % (name, n, np.abs(a - b).max(), a))
    assert np.abs(a - b).max() <= 1e-12


@pytest.mark.parametrize("name,n", PAIRS, ids=lambda v: str(v))
def test_float32_restatement_close_to_float64(name, n):
    y32, y64 = R.index(R.model(name)[1], R.wave(name, n), np.float32), R.reference(name, n)
    err = np.abs(y32 - y64).max()
    print("%s n = %d: float32 against float64 on the logits %.2e; logits %s" % (name, n, err, y64))
    assert y32.dtype == np.float32 and err <= 1e-4
    assert 0.05 <= np.abs(y64).max() <= 10.0  # of order 1: the gate is neither met by nothing nor drowned


def _mutated(t, x, mut):
    """the index form with one seeded defect of the network"""
    t2 = dict(t)
    if mut == "no_clamp":
        assert np.abs(x).max() > 1
        return sw.classifier_forward(t, x, clamp=False)
    if mut == "heads_as_upstream":  # the tiny model has 2 heads of 128: 4 heads of 64 is another network
        t2["classifier.config"] = np.array([t["classifier.config"][0], 4], np.float32)
    elif mut == "factor_2":
        t2["classifier.config"] = np.array([2, t["classifier.config"][1]], np.float32)
    elif mut == "zero_module":  # upstream's initial value of out_layers.3 and proj_out: a loader that kept it would drop half the network
        for k in t:
            if "out_layers.3" in k or "proj_out" in k:
                t2[k] = np.zeros_like(t[k])
    elif mut == "group_count":
        keep = sw.classifier_groups
        try:
            sw.classifier_groups = lambda C_: 32
            return sw.classifier_forward(t, x)
        finally:
            sw.classifier_groups = keep
    return sw.classifier_forward(t2, x)


@pytest.mark.parametrize("mut", ["no_clamp", "heads_as_upstream", "factor_2", "zero_module", "group_count"])
def test_network_defects_leave_the_gate(mut):
    t, x = R.model("tiny")[1], R.wave("tiny", 1000)
    d = np.abs(_mutated(t, x, mut) - R.reference("tiny", 1000)).max()
    print("%s: moves the logits by %.2e" % (mut, d))
    assert d > R.GATE


def test_crop_in_both_spellings(monkeypatch):
    assert sw.CLASSIFIER_MAX_SAMPLES == 220000
    monkeypatch.setattr(sw, "CLASSIFIER_MAX_SAMPLES", 3000)  # the rule at a length float64 NumPy walks in a moment; the device test runs the real one
    t, x = R.model("tiny")[1], R.wave("tiny", 3007)
    assert np.array_equal(R.index(t, x), R.index(t, x[:3000])) and np.array_equal(R.literal(t, x), R.literal(t, x[:3000]))
    assert not np.array_equal(R.index(t, x), R.index(t, x[:2999]))


def test_positions_against_the_formula(pkg):
    L = pkg.lib()
    for n in range(1, 4101):
        want = n
        for _ in range(5):
            want = (want - 1) // 4 + 1
        assert L.tts_classifier_positions(n) == want == R.positions(n), n
    assert L.tts_classifier_positions(220000) == L.tts_classifier_positions(220001) == L.tts_classifier_positions(2 ** 31 - 1) == 215
    assert L.tts_classifier_positions(0) == ARG and L.tts_classifier_positions(-3) == ARG
    assert pkg.Engine.classifier_positions(1024) == 1 and pkg.Engine.classifier_positions(1025) == 2


def test_writer_round_trip_and_shapes():
    for name, cfg in R.CONFIGS.items():
        path, t = R.model(name)
        want = sw.classifier_tensor_shapes(**cfg)
        assert list(t) == list(want)
        for k, shape in want.items():
            assert t[k].shape == tuple(shape), k
        assert list(t["classifier.config"]) == [cfg["F"], cfg["H"]]
        for k in t:  # upstream's zero_module convolutions are not zero in a trained file: the synthetic file must exercise them
            if "out_layers.3.weight" in k or "proj_out.weight" in k:
                assert np.abs(t[k]).max() > 0.01, k
    u = sw.classifier_tensor_shapes()
    assert len(u) == 2 + 5 * (2 * 8 + 2) + 4 + 4 * 6 + 2 + 1
    assert u["classifier.enc.init.weight"] == (32, 1, 3) and u["classifier.enc.res.2.op.weight"] == (64, 32, 5) and u["classifier.enc.res.14.op.weight"] == (1024, 512, 5)
    assert u["classifier.enc.res.13.out_layers.3.weight"] == (512, 512, 5) and u["classifier.enc.final.2.weight"] == (512, 1024, 1)
    assert u["classifier.enc.attn.3.qkv.weight"] == (1536, 512, 1) and u["classifier.head.weight"] == (2, 512)
    assert [sw.classifier_groups(c) for c in (8, 16, 24, 32, 64, 128, 1024)] == [8, 8, 8, 16, 16, 32, 32]


def test_header_exports_and_bindings(pkg):
    names = pkg.header_symbols()
    for n in ("tts_load_classifier", "tts_classifier_positions", "tts_classify_audio"):
        assert n in names and hasattr(pkg.lib(), n), n
    for n in ("load_classifier", "classifier_positions", "classify_audio"):
        assert hasattr(pkg.Engine, n), n
    hdr = open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read()
    assert "#define TTS_CLS_MAX_SAMPLES 220000" in hdr and "#define TTS_API_VERSION 8" in hdr.replace("  ", " ")


def _write(path, tensors):
    w = sw.GgmlWriter(str(path))
    for k, a in tensors.items():
        w.add(k, a)
    w.close()
    return str(path).encode()


BROKEN = [("wrong shape", lambda t: t.__setitem__("classifier.enc.res.2.out_layers.3.weight", t["classifier.enc.res.2.out_layers.3.weight"].reshape(64, 5, 64))),
          ("wrong shape", lambda t: t.__setitem__("classifier.head.weight", t["classifier.head.weight"].T.copy())),
          ("missing", lambda t: t.pop("classifier.enc.res.1.op.bias")),
          ("missing", lambda t: t.pop("classifier.enc.attn.0.proj_out.bias")),
          ("unknown tensors", lambda t: t.__setitem__("classifier.extra", np.zeros(3, np.float32))),
          ("head dimension must be 64 or 128", lambda t: t.__setitem__("classifier.config", np.array([4, 8], np.float32))),
          ("head dimension must be 64 or 128", lambda t: t.__setitem__("classifier.config", np.array([4, 3], np.float32))),
          ("head dimension must be 64 or 128", lambda t: t.__setitem__("classifier.config", np.array([4, 1], np.float32))),
          ("downsample factor", lambda t: t.__setitem__("classifier.config", np.array([4.5, 2], np.float32))),
          ("downsample factor", lambda t: t.__setitem__("classifier.config", np.array([9, 2], np.float32))),
          ("wrong shape", lambda t: t.__setitem__("classifier.config", np.array([4, 2, 0], np.float32))),
          ("ResBlocks", lambda t: [t.pop(k) for k in list(t) if k.startswith("classifier.enc.res.3.")]),
          ("embedding dimension", lambda t: t.__setitem__("classifier.enc.final.2.weight", t["classifier.enc.final.2.weight"][:200]))]


def test_refusals_on_a_host_only_context(pkg, small_models, tmp_path):
    """The loader parses before it asks for the device: broken files are TTS_ERR_FORMAT even here, a good file and every tts_classify_audio call TTS_ERR_HIP."""
    e = pkg.Engine(-1)
    L, h = e.L, e.h
    err = lambda: L.tts_last_error(h).decode()  # noqa: E731
    tensors = R.model("tiny")[1]
    for what, edit in BROKEN:
        t = dict(tensors)
        edit(t)
        assert L.tts_load_classifier(h, _write(tmp_path / "bad.bin", t)) == FMT and what in err(), (what, err())
    assert L.tts_load_classifier(h, (small_models + "/ggml-vocoder-model.bin").encode()) == FMT and "is not a classifier model file" in err()
    assert L.tts_load_classifier(h, str(tmp_path / "nowhere.bin").encode()) in (-2, FMT)
    assert L.tts_load_classifier(h, None) == ARG and L.tts_load_classifier(None, R.model("tiny")[0].encode()) == ARG
    t = dict(tensors)
    t.pop("classifier.config")  # without it: upstream's 4 and 4, which at E = 256 is a head dimension of 64
    assert L.tts_load_classifier(h, _write(tmp_path / "noconfig.bin", t)) == HIP and "host-only" in err()
    assert L.tts_load_classifier(h, R.model("tiny")[0].encode()) == HIP and "host-only" in err()
    x, n, r = np.zeros(8, np.float32), np.array([8], np.int64), np.array([24000], np.int32)
    prob, logits = np.full(1, 7.0, np.float32), np.full(2, 7.0, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.tts_classify_audio(h, p(x), p(n), p(r), 1, p(prob), p(logits)) == HIP and "host-only" in err()
    assert L.tts_classify_audio(h, None, p(n), p(r), 0, None, None) == HIP
    assert L.tts_classify_audio(None, p(x), p(n), p(r), 1, p(prob), p(logits)) == ARG
    assert prob[0] == 7.0 and (logits == 7.0).all(), "a refused call wrote its output"
    e.close()


def _state_dict(name):
    return {k[len("classifier."):]: torch.from_numpy(v) for k, v in R.model(name)[1].items() if k != "classifier.config"}


def _convert(tmp_path, sd, extra=(), expect_ok=True):
    src = tmp_path / "classifier.pth"
    torch.save(sd, str(src))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--classifier", str(src), "--out", str(tmp_path / "out")] + list(extra),
                       capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == expect_ok, r.stdout + r.stderr
    return r


def test_converter_round_trip(tmp_path):
    r = _convert(tmp_path, _state_dict("tiny"), ["--classifier-heads", "2"])
    assert "base 32 channels, depth 2, embedding 256, 2 heads" in r.stdout
    got, want = sw.read_ggml(str(tmp_path / "out" / "ggml-classifier-model.bin")), R.model("tiny")[1]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert np.array_equal(R.index(got, R.wave("tiny", 1000)), R.reference("tiny", 1000))


def test_converter_refusals(tmp_path):
    sd = _state_dict("tiny")
    assert "head dimension must be 64 or 128" in _convert(tmp_path, sd, ["--classifier-heads", "3"], False).stderr
    bad = dict(sd)
    bad["enc.res.0.extra.weight"] = torch.zeros(3)
    assert "unexpected tensor 'enc.res.0.extra.weight'" in _convert(tmp_path, bad, ["--classifier-heads", "2"], False).stderr
    bad = dict(sd)
    del bad["enc.attn.0.qkv.bias"]
    assert "'enc.attn.0.qkv.bias' is missing" in _convert(tmp_path, bad, ["--classifier-heads", "2"], False).stderr
    bad = dict(sd)
    bad["head.weight"] = sd["head.weight"].T.contiguous()
    assert "'head.weight' has shape" in _convert(tmp_path, bad, ["--classifier-heads", "2"], False).stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--list-expected", "classifier"], capture_output=True, text=True, timeout=120)
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("classifier ")]
    assert r.returncode == 0 and len(rows) == 122 and ["classifier", "enc.res.14.op.weight", "1024x512x5"] in rows
    assert rows == [["classifier", k[len("classifier."):], "x".join(map(str, s))] for k, s in sw.classifier_tensor_shapes(config=False).items()]


CLI_ERRORS = [(["--detect", "a.wav"], "--detect needs --classifier"), (["--detect", "a.wav", "--classifier", "c.bin", "--dry-run", "1"], "cannot be combined with --dry-run 1"),
              (["--classifier", "c.bin", "--dry-run", "1"], "cannot be combined with --dry-run 1"), (["--classifier", "c.bin", "--devices", "2"], "--devices > 1")]


@pytest.mark.parametrize("extra,what", CLI_ERRORS, ids=[" ".join(e) for e, _ in CLI_ERRORS])
def test_cli_usage_errors(tmp_path, extra, what):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    r = subprocess.run([exe, "--models", str(tmp_path / "nowhere"), "--message", "hi", "--output", str(tmp_path / "o.wav")] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and what in r.stderr, r.stderr
    assert "model_load" not in r.stderr and not (tmp_path / "o.wav").exists()  # before a model is loaded
