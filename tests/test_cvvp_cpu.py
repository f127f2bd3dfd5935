"""CVVP re-ranking, the part that needs no GPU (tests/test_cvvp_gpu.py holds the engine against the reference pinned here).
No upstream source, weights or fixtures exist offline, so the chain of evidence is CLVP's (tests/test_clvp.py):
  NumPy restatement  ==  torch.nn.functional restatement (tests/cvvp_ref.py, float64, 1e-9)              [here]
  the restatements' encoder layers  ==  tests/torch_ref.py: TorchCLVP.encode on the same tensors           [here]
  NumPy restatement  ~  HIP engine on synthetic weights                                                   [GPU]"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cvvp_ref as CR
import torch_ref as TR
from conftest import ROOT


@pytest.fixture(scope="module")
def small(pkg):
    return CR.synth_file(2)


@pytest.fixture(scope="module")
def both(small):
    """the two restatements on the depth-2 file and the shared inputs: latents and scores, computed once"""
    mels, _ = CR.case_inputs()
    _, codes = CR.case_inputs(lens=(1, 7, 13, 57, 200))
    n, t = CR.NumpyCVVP(small), CR.TorchCVVP(small)
    out = {"mels": mels, "codes": codes, "n": n, "t": t}
    out["vn"], out["vt"] = n.voice(mels), t.voice(mels)
    out["zn"], out["zt"] = n.speech(codes), t.speech(codes)
    out["sn"] = n.score(out["vn"], codes, out["zn"])
    out["st"] = t.score(out["vt"], codes)
    return out


def test_restatements_agree(both):
    """clips of 4, 5, 7, 8, 130 and 517 frames, code lengths 1, 7, 13, 57, 200: 1e-9 absolute on latents and scores, six orders under the GPU gate this supports"""
    dv, dz, ds = np.abs(both["vn"] - both["vt"]).max(), np.abs(both["zn"] - both["zt"]).max(), np.abs(both["sn"] - both["st"]).max()
    print("CVVP NumPy vs torch.nn.functional (f64): max abs diff voice latents %.2e, speech latents %.2e, scores %.2e" % (dv, dz, ds))
    assert both["vn"].shape == (6, 512) and both["zn"].shape == (5, 512)
    assert max(dv, dz, ds) < 1e-9
    assert np.allclose(np.linalg.norm(both["vn"], axis=1), 1.0, atol=1e-12)
    # every clip on its own as well: a clip's latent must not depend on the others
    per_clip = np.array([both["n"].score(both["vn"][k:k + 1], both["codes"], both["zn"]) for k in range(6)])
    per_clip_t = np.array([both["t"].score(both["vt"][k:k + 1], both["codes"]) for k in range(6)])
    assert np.abs(per_clip - per_clip_t).max() < 1e-9


def test_candidates_told_apart(both):
    print("CVVP scores (f64):", both["sn"])
    assert np.ptp(both["sn"]) > 1e-3


def test_mean_over_clips(both):
    one = np.array([both["n"].score(both["vn"][k:k + 1], both["codes"], both["zn"]) for k in range(6)])
    assert np.abs(one.mean(axis=0) - both["sn"]).max() < 1e-12


def test_gpu_cases_have_a_ranking_gap(small):
    """tests/test_cvvp_gpu.py checks the engine's arg-max where the reference's two best scores differ by more than 2e-3: the shared inputs must hold such a case"""
    mels, codes = CR.case_inputs()
    n = CR.NumpyCVVP(small)
    v, z = n.voice(mels), n.speech(codes)
    gaps = []
    for k in list(range(len(mels))) + [None]:
        s = np.sort(n.score(v if k is None else v[k:k + 1], codes, z))[::-1]
        gaps.append(s[0] - s[1])
    print("gaps between the two best reference scores (per clip, then all clips):", np.array(gaps))
    assert max(gaps) > 2e-3


@pytest.mark.parametrize("enc", CR.ENCODERS)
def test_layers_are_clvps(small, both, enc):
    """the restatements' encoder layers (and final LayerNorm) equal TorchCLVP.encode in float64 on the same tensors: 'the same layer as CLVP'"""
    w = both["t"].w
    clvp = object.__new__(TR.TorchCLVP)
    clvp.w, clvp.dtype, clvp.dim, clvp.heads = w, torch.float64, 512, 8
    clvp.depth = CR.depth_of(w, enc)
    assert clvp.depth == 2
    x = torch.from_numpy(np.random.RandomState(1).randn(37, 512))
    want = clvp.encode(enc, x).numpy()
    dn, dt = np.abs(both["n"].layers(enc, x.numpy()) - want).max(), np.abs(both["t"].layers(enc, x).numpy() - want).max()
    print("%s layers vs TorchCLVP.encode: NumPy %.2e, torch.nn.functional %.2e" % (enc, dn, dt))
    assert dn < 1e-9 and dt < 1e-9


def test_rows(pkg):
    L = pkg.lib()
    for T in list(range(1, 65)) + [517]:
        t1 = (T + 2 * 2 - 5) // 2 + 1
        r = (t1 + 2 * 1 - 3) // 2 + 1
        out = torch.nn.functional.conv1d(torch.nn.functional.conv1d(torch.zeros(1, 1, T), torch.zeros(1, 1, 5), stride=2, padding=2), torch.zeros(1, 1, 3), stride=2, padding=1)
        assert L.tts_cvvp_rows(T) == r == out.shape[-1] == CR.rows_of(T) == pkg.Engine.cvvp_rows(T), T
    assert L.tts_cvvp_rows(517) == 130 and (517 - 1) // 2 + 1 == 259
    assert L.tts_cvvp_rows(0) < 0 and L.tts_cvvp_rows(-3) < 0


def test_symbols_exported(pkg):
    L, declared = pkg.lib(), set(pkg.header_symbols())
    for s in ("tts_load_cvvp", "tts_cvvp_latent_dim", "tts_cvvp_rows", "tts_cvvp_voice", "tts_cvvp_voice_audio", "tts_cvvp_score"):
        assert s in declared and hasattr(L, s), s
    assert L.tts_version() == 8
    for m in ("load_cvvp", "cvvp_voice", "cvvp_voice_audio", "cvvp_score", "rerank"):
        assert hasattr(pkg.Engine, m), m


def _convert(tmp_path, sd, name="cvvp.pth"):
    os.makedirs(str(tmp_path / "out"), exist_ok=True)
    torch.save(sd, str(tmp_path / name))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--cvvp", str(tmp_path / name), "--out", str(tmp_path / "out")],
                          capture_output=True, text=True, timeout=300)


def _state_dict(small, wrap):
    from tortoise_cpp_amd import synth_weights as sw
    sd = {}
    for k, v in sw.read_ggml(small).items():
        t = torch.from_numpy(v)
        if k == "temperature":
            t = t.reshape(())  # a 0-dim nn.Parameter
        if wrap and ".attn_layers.layers." in k:  # upstream's checkpoint wrapper around the wrapped blocks
            head, tail = k.split(".attn_layers.layers.")
            n, kind, rest = tail.split(".", 2)
            k = "%s.attn_layers.layers.%s.%s.wrap.%s" % (head, n, kind, rest) if kind == "1" else k
        sd[k] = t
    return sd


@pytest.mark.parametrize("wrap", [False, True])
def test_convert_roundtrip(pkg, small, tmp_path, wrap):
    from tortoise_cpp_amd import synth_weights as sw
    sd = _state_dict(small, wrap)
    assert any(".wrap." in k for k in sd) == wrap
    sd["speech_transformer.transformer.attn_layers.rotary_pos_emb.inv_freq"] = torch.arange(16, dtype=torch.float32)  # a buffer the loader recomputes: kept
    r = _convert(tmp_path, sd)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2 encoder layers per side" in r.stdout
    got, want = sw.read_ggml(str(tmp_path / "out" / "ggml-cvvp-model.bin")), sw.read_ggml(small)
    extra = set(got) - set(want)
    assert extra == {"speech_transformer.transformer.attn_layers.rotary_pos_emb.inv_freq"}
    for k, v in want.items():
        assert got[k].shape == v.shape and (got[k] == v).all(), k
    if not wrap:  # the same bytes as write_cvvp's file, tensor for tensor in its order, when nothing is added
        del sd["speech_transformer.transformer.attn_layers.rotary_pos_emb.inv_freq"]
        r = _convert(tmp_path, sd)
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(str(tmp_path / "out" / "ggml-cvvp-model.bin"), "rb").read() == open(small, "rb").read()


def test_convert_refuses(pkg, small, tmp_path):
    sd = _state_dict(small, False)
    missing = dict(sd)
    del missing["conditioning_transformer.pre_combiner.1.qkv.bias"]
    r = _convert(tmp_path, missing)
    assert r.returncode != 0 and "pre_combiner.1.qkv.bias" in r.stderr and "missing" in r.stderr
    extra = dict(sd)
    extra["speech_transformer.pos_emb.weight"] = torch.zeros(4, 4)
    r = _convert(tmp_path, extra)
    assert r.returncode != 0 and "unexpected tensor 'speech_transformer.pos_emb.weight'" in r.stderr
    shaped = dict(sd)
    shaped["cond_emb.0.weight"] = torch.zeros(256, 80, 3)
    r = _convert(tmp_path, shaped)
    assert r.returncode != 0 and "cond_emb.0.weight" in r.stderr and "shape" in r.stderr
    # a CLVP checkpoint is not a CVVP checkpoint
    r = _convert(tmp_path, {"text_emb.weight": torch.zeros(256, 8), "speech_emb.weight": torch.zeros(8192, 8)})
    assert r.returncode != 0


def test_list_expected_matches_writer(pkg, small):
    from tortoise_cpp_amd import synth_weights as sw
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--list-expected", "cvvp"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("# cvvp: 208 tensors"), r.stdout[:200] + r.stderr  # 8 + 2 x (8 x 11 + 2 + 10) at upstream's depth
    listed = {l.split()[1]: l.split()[2] for l in r.stdout.splitlines()[1:]}
    have = sw.read_ggml(small)
    for k, v in have.items():  # the depth-2 file's tensors are a subset, with the listed shapes
        assert k in listed, k
        assert listed[k] == ("scalar" if k == "temperature" else "x".join(map(str, v.shape))), (k, listed[k], v.shape)


def test_blend_rule(pkg):
    """clvp * (1 - a) + cvvp * a; the side whose weight is 0 is not evaluated"""
    c, v = np.array([0.1, 0.5, -0.2], np.float32), np.array([0.4, -0.1, 0.3], np.float32)

    def never():
        raise AssertionError("the side with weight 0 was evaluated")
    assert (pkg.blend_scores(lambda: c, never, 0.0) == c).all()
    assert (pkg.blend_scores(never, lambda: v, 1.0) == v).all()
    for a in (0.25, 0.5, 0.9):
        got = pkg.blend_scores(lambda: c, lambda: v, a)
        assert got.dtype == np.float32 and np.abs(got - (c.astype(np.float64) * (1 - a) + v.astype(np.float64) * a)).max() < 1e-7
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(pkg.TtsError, match="cvvp_amount"):
            pkg.blend_scores(lambda: c, lambda: v, bad)
