"""CPU: what pins the wav2vec2 CTC aligner (csrc/aligner.h) without a GPU. Two independent float64 spellings of the model agree; a float32 twin is measured
against them; the top-two logit margin of the float64 reference exceeds twice the logit gate on EVERY frame of EVERY clip tests/test_aligner_gpu.py uses, so the
device's argmax is compared on every frame with nothing excluded; the host rules (tts_host_ctc_decode / max_alignment / ctc_align / redact_spans) equal a
literal Python restatement on hand-made and seeded random cases; the writer, the converter (with the weight-norm fold against torch's own), the loader's
refusals on a host-only context and the CLI's usage errors. The model and the rules are stated from memory: unpinned against upstream."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import aligner_ref as R
from tortoise_cpp_amd import synth_weights as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, FMT, HIP = -1, -3, -4
CASES = [(name, n) for name in R.CONFIGS for n in R.GPU_SAMPLES[name]]
# every (configuration, samples, wave variant) tests/test_aligner_gpu.py hands to the device at 16 kHz
GPU_CLIPS = [(name, n, 0) for name, n in CASES] + [("even", n, 1 + i) for i, n in enumerate(R.RAGGED)] + [("odd", 2600, 1), ("even", 2600, 3), ("even", 1800, 5)]


@pytest.mark.parametrize("name,n", CASES, ids=["%s-n%d" % c for c in CASES])
def test_two_float64_spellings_agree(name, n):
    a, b = R.reference(name, n), R.literal(R.model(name)[1], R.wave(name, n))
    assert a.shape == (R.frames(name, n), R.CONFIGS[name]["V"]) and a.shape == b.shape
    err = np.abs(a - b).max()
    print("aligner %s n = %d: %d frames, the two float64 spellings differ by %.2e" % (name, n, a.shape[0], err))
    assert err <= 1e-11


@pytest.mark.parametrize("name,n", CASES, ids=["%s-n%d" % c for c in CASES])
def test_float32_restatement_close_to_float64(name, n):
    a, c = R.reference(name, n), R.index(R.model(name)[1], R.wave(name, n), np.float32)
    err = np.abs(a - c).max()
    print("aligner %s n = %d: float32 restatement within %.2e of float64 (logits up to %.1f)" % (name, n, err, np.abs(a).max()))
    assert c.dtype == np.float32 and err <= R.GATE / 4 and np.array_equal(a.argmax(1), c.argmax(1))


@pytest.mark.parametrize("name,n,k", GPU_CLIPS, ids=["%s-n%d-k%d" % c for c in GPU_CLIPS])
def test_margin_exceeds_twice_the_gate_on_every_frame(name, n, k):
    m = R.margin(R.reference(name, n, k))
    print("aligner %s n = %d k = %d: smallest top-two margin %.4f over %d frames" % (name, n, k, m.min(), len(m)))
    assert m.min() > 2 * R.GATE


def test_frames_against_the_reference_shapes(pkg):
    L = pkg.lib()
    up = sw.ALIGNER_UPSTREAM
    for n in (400, 401, 719, 720, 16000, 147200, 1 << 20):
        assert L.tts_aligner_frames(n) == sw.aligner_frames(n, up["k"], up["s"]), n
    assert L.tts_aligner_frames(400) == 1 and L.tts_aligner_frames(147200) == 459
    for n in (399, 1, 0, -5):
        assert L.tts_aligner_frames(n) == ARG
    for name, n in CASES:
        assert R.reference(name, n).shape[0] == R.frames(name, n)


def test_writer_round_trip_and_shapes():
    for name, cfg in R.CONFIGS.items():
        path, t = R.model(name)
        want = sw.aligner_tensor_shapes(**cfg)
        assert list(t) == list(want)
        for k, shape in want.items():
            assert t[k].shape == tuple(shape), k
        assert list(t["aligner.config"]) == [cfg["H"], cfg["blank"]] + list(cfg["s"])
        assert np.array_equal(t["aligner.vocab"], sw.aligner_vocab(cfg["V"]))
        for k in t:
            if "layer_norm.weight" in k:
                assert np.abs(t[k] - 1).max() < 0.3, k
    u = sw.aligner_tensor_shapes()
    assert len(u) == 7 * 4 + 4 + 2 + 24 * 16 + 4 + 2
    assert u["aligner.feature_extractor.conv_layers.0.conv.weight"] == (512, 1, 10) and u["aligner.feature_extractor.conv_layers.6.conv.weight"] == (512, 512, 2)
    assert u["aligner.encoder.pos_conv_embed.conv.weight"] == (1024, 64, 128) and u["aligner.encoder.layers.23.feed_forward.output_dense.weight"] == (1024, 4096)
    assert u["aligner.lm_head.weight"] == (32, 1024) and u["aligner.config"] == (9,) and u["aligner.vocab"] == (32,)
    v = sw.aligner_vocab(33)
    assert v[0] == -1 and v[4] == 32 and v[5] == ord("a") and v[30] == ord("z") and v[31] == ord("'") and v[32] == -1


def test_header_exports_and_bindings(pkg):
    names = pkg.header_symbols()
    for n in ("tts_load_aligner", "tts_aligner_frames", "tts_aligner_ids", "tts_align_audio", "tts_redact_audio", "tts_aligner_vocab", "tts_aligner_clip_frames",
              "tts_host_ctc_decode", "tts_host_max_alignment", "tts_host_ctc_align", "tts_host_redact_spans"):
        assert n in names and hasattr(pkg.lib(), n), n
    for n in ("load_aligner", "aligner_ids", "align_audio", "redact_audio", "aligner_frames"):
        assert hasattr(pkg.Engine, n), n
    for n in ("host_ctc_decode", "host_max_alignment", "host_ctc_align", "host_redact_spans"):
        assert hasattr(pkg, n), n
    assert "#define TTS_API_VERSION 8" in open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read().replace("  ", " ")


# ---- the host rules ----
def _status(fn, *a):
    try:
        fn(*a)
    except Exception as e:  # TtsError carries the C status
        return getattr(e, "status", None)
    return 0


HAND = [("", ""), ("", "abc"), ("abc", ""), ("abc", "abc"), ("a", "a"), ("a", "b"), ("abc", "xyz"), ("hello world", "helo wrld"), ("xhello", "hello"), ("hellox", "hello"),
        ("hello", "xhello"), ("hello", "hellox"), ("aaaa", "aa"), ("aa", "aaaa"), ("abab", "baba"), ("mississippi", "misisipi"), ("the cat", "the the cat cat"),
        ("a b", "ab"), ("ab", "a b"), ("été là", "ete la"), ("naïve", "naïve")]


@pytest.mark.parametrize("s1,s2", HAND)
def test_max_alignment_hand_cases(pkg, s1, s2):
    got = pkg.host_max_alignment(s1, s2)
    assert got == R.max_alignment(s1, s2) and len(got) == len(s1)
    assert all(g in (c, "~") for g, c in zip(got, s1))


def test_max_alignment_known_answers_and_refusal(pkg):
    assert pkg.host_max_alignment("hello world", "helo wrld") == "hel~o w~rld"
    assert pkg.host_max_alignment("abc", "") == "~~~" and pkg.host_max_alignment("", "abc") == "" and pkg.host_max_alignment("abc", "xyz") == "~~~"
    assert pkg.host_max_alignment("xhello", "hello") == "~hello" and pkg.host_max_alignment("hellox", "hello") == "hello~"
    assert _status(pkg.host_max_alignment, "a~b", "ab") == ARG
    with pytest.raises(ValueError):
        R.max_alignment("a~b", "ab")


def test_max_alignment_random_pairs(pkg):
    rng = random.Random(20260)
    for i in range(400):
        alpha = "ab" if i % 3 == 0 else "abc d'" if i % 3 == 1 else "abcdefghij klm"
        a = "".join(rng.choice(alpha) for _ in range(rng.randint(0, 24)))
        b = "".join(rng.choice(alpha) for _ in range(rng.randint(0, 24)))
        if i % 7 == 0:  # near copies: deletions and insertions, what an aligner actually sees
            b = "".join(c for c in a if rng.random() > 0.2) + ("x" if rng.random() > 0.5 else "")
        assert pkg.host_max_alignment(a, b) == R.max_alignment(a, b), (a, b)


VOCAB = sw.aligner_vocab(33)
TOK = {chr(c): i for i, c in enumerate(VOCAB) if c >= 0}


def _ids(s, rng=None, blank=0):
    """frames that CTC-decode to s: every character one or more frames, a blank between equal neighbours and here and there"""
    out = []
    for i, c in enumerate(s):
        if (i and s[i - 1] == c) or (rng and rng.random() < 0.3):
            out += [blank] * (1 + (rng.randint(0, 2) if rng else 0))
        out += [TOK[c]] * (1 + (rng.randint(0, 2) if rng else 0))
    return np.array(out or [blank], np.int32)


def test_ctc_decode(pkg):
    rng = random.Random(3)
    for s in ("", "a", "hello world", "aab b", "it's"):
        ids = _ids(s, rng)
        assert pkg.host_ctc_decode(ids, VOCAB, 0) == s == R.ctc_decode(ids, VOCAB, 0)
    ids = np.array([0, 1, 2, 3, 5, 5, 0, 5, 32, 4, 4, 6], np.int32)  # the special tokens and the trailing -1 token vanish, the delimiter is a space
    assert pkg.host_ctc_decode(ids, VOCAB, 0) == "aa b" == R.ctc_decode(ids, VOCAB, 0)
    assert pkg.host_ctc_decode(ids, VOCAB, 5) == R.ctc_decode(ids, VOCAB, 5)  # another blank id
    assert _status(pkg.host_ctc_decode, np.array([33], np.int32), VOCAB, 0) == ARG and _status(pkg.host_ctc_decode, np.array([-1], np.int32), VOCAB, 0) == ARG


ALIGN_HAND = [("hello", "hello"), ("hello there", "hello there"), ("say hello there", "hello there"), ("hello there now", "hello there"), ("hxello", "hello"),
              ("Hello THERE", "hello there"), ("a", "a"), ("a", "b"), ("aab", "aab"), ("xhello", "hello"), ("hello", "xhello"), ("hexllo wxorld", "hello world"),
              ("hello", "h"), ("hellozz", "hello"), ("zzhello", "hello")]


@pytest.mark.parametrize("text,audio", ALIGN_HAND)
def test_ctc_align_hand_cases(pkg, text, audio):
    ids = _ids(audio, random.Random(len(text)))
    n_samples = 320 * len(ids) + 77
    if text == "a" and audio == "b":  # nothing of the text in the audio: the documented failure
        with pytest.raises(R.Mismatch):
            R.ctc_align(ids, VOCAB, 0, text, n_samples)
        assert _status(pkg.host_ctc_align, ids, VOCAB, 0, text, n_samples) == ARG
        return
    want = R.ctc_align(ids, VOCAB, 0, text, n_samples)
    got = pkg.host_ctc_align(ids, VOCAB, 0, text, n_samples)
    assert list(got) == want and len(want) == len(text) and want[0] == 0
    assert all(0 <= a <= n_samples for a in want) and want == sorted(want)


def test_ctc_align_failures_and_edges(pkg):
    ids = _ids("hello there")
    n = 320 * len(ids)
    for text in ("hello there", "there hello", "h", "hello there hello there"):
        assert list(pkg.host_ctc_align(ids, VOCAB, 0, text, n)) == R.ctc_align(ids, VOCAB, 0, text, n)
    # the text absent from the audio: max_alignment leaves nothing but '~', nothing can be placed - the documented failure, in both statements
    for text in ("quiz", "q", "~"):
        assert _status(pkg.host_ctc_align, ids, VOCAB, 0, text, n) == ARG
    for text in ("quiz", "q"):
        with pytest.raises(R.Mismatch):
            R.ctc_align(ids, VOCAB, 0, text, n)
    # a kept character the walk cannot place: a vocabulary with two tokens for one character, the frames carry the second
    twice = VOCAB.copy()
    twice[6] = ord("a")  # tokens 5 and 6 are both 'a'
    frames = np.array([TOK["c"], 6, TOK["d"]], np.int32)  # decodes to "cad"
    assert pkg.host_ctc_decode(frames, twice, 0) == "cad"
    assert _status(pkg.host_ctc_align, frames, twice, 0, "cad", 960) == ARG
    with pytest.raises(R.Mismatch):
        R.ctc_align(frames, twice, 0, "cad", 960)
    assert list(pkg.host_ctc_align(frames, twice, 0, "cd", 960)) == R.ctc_align(frames, twice, 0, "cd", 960) == [0, 640]
    assert len(pkg.host_ctc_align(ids, VOCAB, 0, "", n)) == 0 and R.ctc_align(ids, VOCAB, 0, "", n) == []
    assert _status(pkg.host_ctc_align, ids, VOCAB, 0, "a~b", n) == ARG
    assert _status(pkg.host_ctc_align, ids, VOCAB, 0, "abc", 0) == ARG


def test_ctc_align_mismatch_is_reached(pkg):
    """at least one seeded case must fail in BOTH statements (the documented status), or the failure path is untested"""
    rng, seen = random.Random(11), 0
    for i in range(300):
        audio = "".join(rng.choice("ab c") for _ in range(rng.randint(1, 8)))
        text = "".join(rng.choice("ab c") for _ in range(rng.randint(1, 8)))
        ids = _ids(audio, rng)
        n = 320 * len(ids) + rng.randint(0, 319)
        try:
            want = R.ctc_align(ids, VOCAB, 0, text, n)
        except R.Mismatch:
            want = None
            seen += 1
        if want is None:
            assert _status(pkg.host_ctc_align, ids, VOCAB, 0, text, n) == ARG, (audio, text)
        else:
            assert list(pkg.host_ctc_align(ids, VOCAB, 0, text, n)) == want, (audio, text)
    print("ctc_align: %d of 300 seeded pairs fail to align in both statements" % seen)
    assert seen > 0


SPANS = [("no brackets", "no brackets", [(0, 10)]), ("", "", []), ("[a]", "a", []), ("[a]bc", "abc", [(1, 2)]), ("ab[c]", "abc", [(0, 1)]), ("ab[c]de", "abcde", [(0, 1), (3, 4)]),
         ("[a][b]c", "abc", [(2, 2)]), ("a[]b", "ab", [(0, 0), (1, 1)]), ("a[b][c]d", "abcd", [(0, 0), (3, 3)]), ("[I am so sad,] the package never came.",
                                                                                                              "I am so sad, the package never came.", [(12, 35)]),
         ("é[à]ü", "éàü", [(0, 0), (2, 2)])]


@pytest.mark.parametrize("text,bare,iv", SPANS, ids=[s[0] or "empty" for s in SPANS])
def test_redact_spans(pkg, text, bare, iv):
    assert pkg.host_redact_spans(text) == (bare, iv) == R.redact_spans(text)


@pytest.mark.parametrize("text", ["a[b", "a]b", "a[b[c]]", "[[a]]", "a]b[", "[a]b]", "[a"])
def test_redact_spans_refusals(pkg, text):
    assert _status(pkg.host_redact_spans, text) == ARG
    with pytest.raises(ValueError):
        R.redact_spans(text)


# ---- the loader's refusals, the converter, the CLI ----
def _write(path, tensors):
    w = sw.GgmlWriter(str(path))
    for k, a in tensors.items():
        w.add(k, a)
    w.close()
    return str(path).encode()


def _drop_ln(t):
    for i in (1, 2):
        t.pop("aligner.feature_extractor.conv_layers.%d.layer_norm.weight" % i)
        t.pop("aligner.feature_extractor.conv_layers.%d.layer_norm.bias" % i)


P, E0 = "aligner.feature_extractor.conv_layers.", "aligner.encoder.layers.0."
BROKEN = [("wrong shape", lambda t: t.__setitem__("aligner.lm_head.weight", t["aligner.lm_head.weight"].T.copy())),
          ("wrong shape", lambda t: t.__setitem__(E0 + "attention.k_proj.weight", t[E0 + "attention.k_proj.weight"][:64])),
          ("wrong shape", lambda t: t.__setitem__("aligner.config", np.array([2, 0, 5, 2], np.float32))),
          ("wrong shape", lambda t: t.__setitem__("aligner.vocab", t["aligner.vocab"][:20])),
          ("missing", lambda t: t.pop(E0 + "feed_forward.output_dense.bias")),
          ("missing", lambda t: t.pop("aligner.encoder.layer_norm.weight")),
          ("missing", lambda t: t.pop("aligner.vocab")),
          ("missing", lambda t: t.pop("aligner.encoder.pos_conv_embed.conv.weight")),
          ("unknown tensors", lambda t: t.__setitem__("aligner.masked_spec_embed", np.zeros(128, np.float32))),
          ("head dimension must be 64", lambda t: t.__setitem__("aligner.config", np.array([4, 0, 5, 2, 2], np.float32))),
          ("head dimension must be 64", lambda t: t.__setitem__("aligner.config", np.array([1, 0, 5, 2, 2], np.float32))),
          ("are integers", lambda t: t.__setitem__("aligner.config", np.array([2, 0, 5, 2.5, 2], np.float32))),
          ("stride", lambda t: t.__setitem__("aligner.config", np.array([2, 0, 5, 9, 2], np.float32))),
          ("blank id", lambda t: t.__setitem__("aligner.config", np.array([2, 40, 5, 2, 2], np.float32))),
          ("group-norm (base-model) variant", _drop_ln),
          ("group-norm (base-model) variant", lambda t: t.pop(P + "1.conv.bias")),
          ("extractor channels", lambda t: [t.__setitem__(k, v[:32]) for k, v in list(t.items()) if k.startswith(P + "0.")]),
          ("positional convolution", lambda t: t.__setitem__("aligner.encoder.pos_conv_embed.conv.weight", np.zeros((128, 32, 8), np.float32))),
          ("feed-forward width", lambda t: t.__setitem__(E0 + "feed_forward.intermediate_dense.weight", np.zeros((96, 128), np.float32))),
          ("a code point or -1", lambda t: t.__setitem__("aligner.vocab", t["aligner.vocab"] + 0.5))]


def test_refusals_on_a_host_only_context(pkg, small_models, tmp_path):
    """The loader parses before it asks for the device: broken files are TTS_ERR_FORMAT even here, a good file and every device call TTS_ERR_HIP."""
    e = pkg.Engine(-1)
    L, h = e.L, e.h
    err = lambda: L.tts_last_error(h).decode()  # noqa: E731
    tensors = R.model("even")[1]
    for what, edit in BROKEN:
        t = dict(tensors)
        edit(t)
        assert L.tts_load_aligner(h, _write(tmp_path / "bad.bin", t)) == FMT and what in err(), (what, err())
    assert L.tts_load_aligner(h, (small_models + "/ggml-vocoder-model.bin").encode()) == FMT and "is not an aligner model file" in err()
    assert L.tts_load_aligner(h, str(tmp_path / "nowhere.bin").encode()) in (-2, FMT)
    assert L.tts_load_aligner(h, None) == ARG and L.tts_load_aligner(None, R.model("even")[0].encode()) == ARG
    for name in R.CONFIGS:
        assert L.tts_load_aligner(h, R.model(name)[0].encode()) == HIP and "host-only" in err()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    x, n, r = np.zeros(2000, np.float32), np.array([2000], np.int64), np.array([16000], np.int32)
    ids, nf, off, out = np.full(200, 7, np.int32), np.full(1, 7, np.int32), np.full(8, 7, np.int64), np.full(2000, 7, np.float32)
    assert L.tts_aligner_ids(h, p(x), p(n), p(r), 1, p(ids), p(nf), 200, None) == HIP and "host-only" in err()
    assert L.tts_aligner_ids(None, p(x), p(n), p(r), 1, p(ids), p(nf), 200, None) == ARG
    assert L.tts_align_audio(h, p(x), 2000, 16000, b"abc", p(off), 8) == HIP and L.tts_align_audio(None, p(x), 2000, 16000, b"abc", p(off), 8) == ARG
    assert L.tts_redact_audio(h, p(x), 2000, 16000, b"a[b]c", p(out), 2000) == HIP and L.tts_redact_audio(None, p(x), 2000, 16000, b"a[b]c", p(out), 2000) == ARG
    assert L.tts_aligner_vocab(h, None, 0, None) == HIP and L.tts_aligner_clip_frames(h, 2000, 16000) == HIP
    assert (ids == 7).all() and nf[0] == 7 and (off == 7).all() and (out == 7).all(), "a refused call wrote its output"
    e.close()


def _hf_state_dict(name, parametrized=False):
    """the model file as HF's state dict holds it: wav2vec2. / lm_head. names, the positional weight as a weight-norm pair, masked_spec_embed present"""
    t = R.model(name)[1]
    sd = {}
    for k, v in t.items():
        if k in ("aligner.config", "aligner.vocab"):
            continue
        k = k[len("aligner."):]
        sd[k if k.startswith("lm_head.") else "wav2vec2." + k] = torch.from_numpy(v.copy())
    w = sd.pop("wav2vec2.encoder.pos_conv_embed.conv.weight").double()
    rs = torch.Generator().manual_seed(5)
    g = w.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
    v = w * (0.5 + torch.rand(1, 1, w.shape[2], generator=rs, dtype=torch.float64))  # any v on the same rays: g v / |v| is w again
    names = ("parametrizations.weight.original0", "parametrizations.weight.original1") if parametrized else ("weight_g", "weight_v")
    sd["wav2vec2.encoder.pos_conv_embed.conv." + names[0]] = g
    sd["wav2vec2.encoder.pos_conv_embed.conv." + names[1]] = v
    sd["wav2vec2.masked_spec_embed"] = torch.zeros(w.shape[0])
    return sd


def _vocab_json(V):
    toks = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(c).upper() for c in range(ord("a"), ord("z") + 1)] + ["'"] + ["<x%d>" % i for i in range(8)]
    return {t: i for i, t in enumerate(toks[:V])}


def _convert(tmp_path, sd, vocab, extra=(), expect_ok=True):
    src, vj = tmp_path / "pytorch_model.bin", tmp_path / "vocab.json"
    torch.save(sd, str(src))
    json.dump(vocab, open(str(vj), "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--aligner", str(src), "--aligner-vocab", str(vj), "--out", str(tmp_path / "out")]
                       + list(extra), capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == expect_ok, r.stdout + r.stderr
    return r


def test_weight_norm_fold_against_torch():
    """the converter's fold, w = g v / |v| with the norm over output and input channels per tap, is torch.nn.utils.weight_norm(conv, dim=2)'s forward weight"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import convert_weights as cw
    conv = torch.nn.utils.weight_norm(torch.nn.Conv1d(128, 128, 8, padding=4, groups=2), name="weight", dim=2).double()
    with torch.no_grad():
        conv.weight_g.mul_(torch.rand_like(conv.weight_g) + 0.5)
    x = torch.randn(1, 128, 20, dtype=torch.float64)
    want = conv(x)
    sd = {"wav2vec2.encoder.pos_conv_embed.conv." + k: v.detach().clone() for k, v in conv.state_dict().items()}
    assert set(k.rsplit(".", 1)[1] for k in sd) >= {"weight_g", "weight_v"} and tuple(conv.weight_g.shape) == (1, 1, 8)
    g, v = sd["wav2vec2.encoder.pos_conv_embed.conv.weight_g"].double(), sd["wav2vec2.encoder.pos_conv_embed.conv.weight_v"].double()
    folded = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
    got = torch.nn.functional.conv1d(x, folded, conv.bias, padding=4, groups=2)
    assert (got - want).abs().max() < 1e-12
    assert cw.convert_aligner.__doc__ and "norm over output and input channels per tap" in cw.convert_aligner.__doc__


@pytest.mark.parametrize("parametrized", [False, True], ids=["weight_g_v", "parametrizations"])
def test_converter_round_trip(tmp_path, parametrized):
    r = _convert(tmp_path, _hf_state_dict("odd", parametrized), _vocab_json(33), ["--aligner-heads", "2", "--aligner-strides", "5,2,2"])
    assert "3 convolution layers of 64 channels, dimension 128, 2 encoder layers, 33 tokens" in r.stdout
    got, want = sw.read_ggml(str(tmp_path / "out" / "ggml-aligner-model.bin")), R.model("odd")[1]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape, k
        if k == "aligner.encoder.pos_conv_embed.conv.weight":
            assert np.abs(got[k] - want[k]).max() < 1e-7  # through the fold
        else:
            assert np.array_equal(got[k], want[k]), k
    assert np.abs(R.index(got, R.wave("odd", 1310)) - R.reference("odd", 1310)).max() < 1e-4


def test_converter_refusals(tmp_path):
    sd, vocab = _hf_state_dict("odd"), _vocab_json(33)
    ok = ["--aligner-heads", "2", "--aligner-strides", "5,2,2"]
    assert "head dimension must be 64" in _convert(tmp_path, sd, vocab, ["--aligner-heads", "4", "--aligner-strides", "5,2,2"], False).stderr
    assert "2 strides for 3 convolution layers" in _convert(tmp_path, sd, vocab, ["--aligner-heads", "2", "--aligner-strides", "5,2"], False).stderr
    bad = dict(sd)
    bad["wav2vec2.encoder.extra.weight"] = torch.zeros(3)
    assert "unexpected tensor 'encoder.extra.weight'" in _convert(tmp_path, bad, vocab, ok, False).stderr
    bad = dict(sd)
    bad["quantizer.codevectors"] = torch.zeros(3)
    assert "unexpected tensor 'quantizer.codevectors'" in _convert(tmp_path, bad, vocab, ok, False).stderr
    bad = dict(sd)
    del bad["wav2vec2.encoder.layers.1.attention.v_proj.bias"]
    assert "'encoder.layers.1.attention.v_proj.bias' is missing" in _convert(tmp_path, bad, vocab, ok, False).stderr
    bad = dict(sd)
    bad["lm_head.bias"] = torch.zeros(34)
    assert "'lm_head.bias' has shape" in _convert(tmp_path, bad, vocab, ok, False).stderr
    bad = dict(sd)
    del bad["wav2vec2.feature_extractor.conv_layers.1.layer_norm.weight"]
    assert "group-norm (base-model) variant" in _convert(tmp_path, bad, vocab, ok, False).stderr
    assert "lm_head has 33 rows" in _convert(tmp_path, sd, _vocab_json(29), ok, False).stderr
    nopad = {("<blank>" if k == "<pad>" else k): v for k, v in vocab.items()}
    assert "no <pad> token" in _convert(tmp_path, sd, nopad, ok, False).stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--list-expected", "aligner"], capture_output=True, text=True, timeout=120)
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("aligner ")]
    assert r.returncode == 0 and len(rows) == 422 and ["aligner", "encoder.pos_conv_embed.conv.weight", "1024x64x128"] in rows
    assert rows == [["aligner", k[len("aligner."):], "x".join(map(str, s))] for k, s in sw.aligner_tensor_shapes(config=False).items() if k != "aligner.vocab"]


CLI_ERRORS = [(["--split-text", "100"], "cannot be combined with --split-text"), (["--voice", "a.bin", "--voice", "b.bin"], "cannot be combined with several voices"),
              (["--stream", "--decoder", "hifigan"], "cannot be combined with --stream"), (["--devices", "2"], "--devices > 1 or --exchange rccl"),
              (["--exchange", "rccl"], "--devices > 1 or --exchange rccl"), (["--dry-run", "1"], "cannot be combined with --dry-run 1")]


@pytest.mark.parametrize("extra,what", CLI_ERRORS, ids=[" ".join(e) for e, _ in CLI_ERRORS])
def test_cli_usage_errors(tmp_path, extra, what):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    r = subprocess.run([exe, "--models", str(tmp_path / "nowhere"), "--message", "[quietly] hi", "--aligner", "a.bin", "--output", str(tmp_path / "o.wav")] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and what in r.stderr and "--aligner" in r.stderr, r.stderr
    assert "model_load" not in r.stderr and not (tmp_path / "o.wav").exists()  # before a model is loaded


@pytest.mark.parametrize("msg", ["[quietly hi", "quietly] hi", "[a [b]] hi"])
def test_cli_refuses_bad_brackets(tmp_path, msg):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    r = subprocess.run([exe, "--models", str(tmp_path / "nowhere"), "--message", msg, "--aligner", "a.bin", "--output", str(tmp_path / "o.wav")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "unbalanced or nested brackets" in r.stderr and not (tmp_path / "o.wav").exists()
