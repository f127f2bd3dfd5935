"""No GPU: the float64 reference of the DVAE decoder (tests/dvae_dec_ref.py) against torch.nn.functional, the converter's --dvae-decoder round trip and
refusals, every refusal a host-only context can reach, tts_dvae_decode_frames, and the CLI's new usage errors (exit 1 before any load)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dvae_dec_ref as R

sw = R.sw
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT, ARG, HIP = -3, -1, -4


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_reference_against_torch_functional(name):
    t = R.model(name)[1]
    nb, L, s = R.layout(t)
    w = lambda n: torch.from_numpy(t[n].astype(np.float64))  # noqa: E731
    conv = lambda x, p: F.conv1d(x, w(p + "weight"), w(p + "bias"), padding=(t[p + "weight"].shape[2] - 1) // 2)  # noqa: E731
    for n in (1, 5, 33):
        codes = R.codes_for(name, n)
        h = conv(w("dvae.codebook.embed")[:, torch.from_numpy(codes).long()][None], "dvae.decoder.0.")
        for j in range(nb):
            p = "dvae.decoder.%d.net." % (1 + j)
            h = h + conv(F.relu(conv(F.relu(conv(h, p + "0.")), p + "2.")), p + "4.")
        for i in range(L):
            h = F.relu(conv(F.interpolate(h, scale_factor=s, mode="nearest"), "dvae.decoder.%d.0.conv." % (1 + nb + i)))
        want = conv(h, "dvae.decoder.%d." % (1 + nb + L))[0].numpy()
        got = R.reference(name, n)
        assert got["mel"].shape == want.shape == (80, n * s ** L)
        assert np.abs(got["mel"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert got["bound"].min() > 0 and np.isfinite(got["bound"]).all()


def _state_dict(name="A"):
    sd = {k[len("dvae."):]: torch.from_numpy(v.copy()) for k, v in R.model(name)[1].items() if k != "dvae.config"}
    sd.update({"encoder.0.0.weight": torch.zeros(64, 80, 3), "codebook.cluster_size": torch.zeros(64), "codebook.embed_avg": torch.zeros(32, 64)})
    return sd


def _convert(tmp_path, sd, extra=(), expect_ok=True):
    torch.save(sd, str(tmp_path / "dvae.pth"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--dvae-decoder", str(tmp_path / "dvae.pth"), "--out", str(tmp_path / "out")]
                       + list(extra), capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == expect_ok, r.stdout + r.stderr
    return r


def test_converter_round_trip_and_refusals(tmp_path):
    r = _convert(tmp_path, _state_dict())
    assert "2 up-sampling layers, 1 ResBlocks of 128 channels, codebook 32 x 64 tokens" in r.stdout
    got, want = sw.read_ggml(str(tmp_path / "out" / "ggml-dvae-decoder-model.bin")), R.model("A")[1]
    assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want)  # the encoder and the EMA buffers are dropped
    _convert(tmp_path, _state_dict("B"), ["--dvae-stride", "4"])
    got = sw.read_ggml(str(tmp_path / "out" / "ggml-dvae-decoder-model.bin"))
    assert list(got["dvae.config"]) == [4] and got["dvae.decoder.2.0.conv.weight"].shape == (128, 64, 7)
    bad = _state_dict()
    bad["decoder.2.0.weight"] = bad.pop("decoder.2.0.conv.weight").transpose(0, 1).contiguous()  # ConvTranspose1d's [cin][cout][k]
    del bad["decoder.2.0.conv.bias"], bad["decoder.3.0.conv.weight"], bad["decoder.3.0.conv.bias"]
    assert "transposed convolution" in _convert(tmp_path, bad, (), False).stderr
    bad = _state_dict()
    del bad["decoder.1.net.2.bias"]
    assert "'decoder.1.net.2.bias' is missing" in _convert(tmp_path, bad, (), False).stderr
    bad = _state_dict()
    bad["decoder.extra"] = torch.zeros(3)
    assert "unexpected tensor 'decoder.extra'" in _convert(tmp_path, bad, (), False).stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--list-expected", "dvae-decoder"], capture_output=True, text=True, timeout=120)
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("dvae-decoder ")]
    assert r.returncode == 0 and rows == [["dvae-decoder", k[len("dvae."):], "x".join(map(str, s))] for k, s in sw.dvae_decoder_tensor_shapes(config=False).items()]
    assert ["dvae-decoder", "decoder.4.0.conv.weight", "1024x1024x3"] in rows and ["dvae-decoder", "decoder.6.weight", "80x512x1"] in rows


def _write(path, t):
    w = sw.GgmlWriter(str(path))
    for k, v in t.items():
        w.add(k, v)
    w.close()
    return str(path).encode()


def test_refusals_on_a_host_only_context(pkg, tmp_path):
    """The loader parses before it asks for the device: a broken file is TTS_ERR_FORMAT even here, a good file and every device call TTS_ERR_HIP."""
    e = pkg.Engine(-1)
    L, h = e.L, e.h
    err = lambda: L.tts_last_error(h).decode()  # noqa: E731
    good = R.model("A")[1]
    edits = {"transposed": (lambda t: t.update({"dvae.decoder.2.0.weight": t.pop("dvae.decoder.2.0.conv.weight")}), "transposed convolution"),
             "no codebook": (lambda t: t.pop("dvae.codebook.embed"), "'dvae.codebook.embed' missing"),
             "even taps": (lambda t: t.update({"dvae.decoder.3.0.conv.weight": np.zeros((64, 128, 4), np.float32)}), "an odd kernel size"),
             "cin": (lambda t: t.update({"dvae.decoder.3.0.conv.weight": np.zeros((64, 64, 3), np.float32)}), "the layer before it writes 128"),
             "channels": (lambda t: t.update({"dvae.decoder.2.0.conv.weight": np.zeros((96, 128, 3), np.float32), "dvae.decoder.2.0.conv.bias": np.zeros(96, np.float32)}),
                          "a multiple of 64"),
             "stride": (lambda t: t.update({"dvae.config": np.array([5], np.float32)}), "stride 5"),
             "bands": (lambda t: t.update({"dvae.decoder.4.weight": np.zeros((129, 64, 1), np.float32), "dvae.decoder.4.bias": np.zeros(129, np.float32)}), "mel channels"),
             "unknown": (lambda t: t.update({"dvae.decoder.9.bias": np.zeros(3, np.float32)}), "unknown tensors"),
             "encoder file": (lambda t: [t.pop(k) for k in list(t) if k.startswith("dvae.decoder.")], "not a DVAE decoder model file")}
    for label, (edit, what) in edits.items():
        t = dict(good)
        edit(t)
        assert L.tts_load_dvae_decoder(h, _write(tmp_path / "bad.bin", t)) == FMT and what in err(), (label, err())
    for name in R.CONFIGS:
        assert L.tts_load_dvae_decoder(h, R.model(name)[0].encode()) == HIP and "host-only" in err()
    assert L.tts_load_dvae_decoder(h, None) == ARG
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    codes, nc, mel, fr, l1 = np.zeros(4, np.int32), np.array([4], np.int32), np.full(8, 7, np.float32), np.full(1, 7, np.int32), np.full(2, 7, np.float32)
    assert L.tts_dvae_decode(h, p(codes), p(nc), 1, 4, p(mel), p(fr), 8) == HIP and "host-only" in err()
    assert L.tts_dvae_reconstruct(h, p(mel), p(nc), 1, p(l1), p(l1), None) == HIP
    x, n, r = np.zeros(3000, np.float32), np.array([3000], np.int64), np.array([22050], np.int32)
    assert L.tts_dvae_reconstruct_audio(h, p(x), p(n), p(r), 1, None, p(l1), p(l1), None, None, 0) == HIP
    assert (mel == 7).all() and fr[0] == 7 and (l1 == 7).all()
    assert L.tts_dvae_decode_frames(h, 10) == 0 and L.tts_dvae_decode_frames(h, 0) == ARG and L.tts_dvae_decoder_channels(h) == 0
    e.close()


CLI_ERRORS = [(["--decode-codes", "c.txt", "--mel-out", "m.bin"], "--decode-codes needs --dvae-decoder"), (["--reconstruct", "IN", "--dvae", "d.bin"], "--reconstruct needs --dvae-decoder"),
              (["--dvae-decoder", "d.bin", "--decode-codes", "CODES"], "--decode-codes needs --mel-out"), (["--dvae-decoder", "d.bin", "--reconstruct", "IN"], "--reconstruct needs --dvae <file>"),
              (["--dvae-decoder", "d.bin"], "--dvae-decoder needs --decode-codes"), (["--mel-out", "m.bin"], "--mel-out needs --decode-codes"),
              (["--dvae-decoder", "d.bin", "--decode-codes", "CODES", "--mel-out", "m.bin", "--reconstruct", "IN"], "cannot be combined"),
              (["--dvae-decoder", "d.bin", "--decode-codes", "CODES", "--mel-out", "m.bin", "--dry-run", "1"], "cannot be combined with --dry-run 1"),
              (["--dvae-decoder", "d.bin", "--dvae", "e.bin", "--reconstruct", "IN", "--codes-from", "IN"], "cannot be combined with --codes-from"),
              (["--dvae-decoder", "d.bin", "--decode-codes", "nowhere.txt", "--mel-out", "m.bin"], "cannot be opened"),
              (["--dvae-decoder", "d.bin", "--decode-codes", "BAD", "--mel-out", "m.bin"], "a line holds space-separated codes"),
              (["--dvae-decoder", "d.bin", "--decode-codes", "EMPTY", "--mel-out", "m.bin"], "no codes"),
              (["--dvae-decoder", "d.bin", "--dvae", "e.bin", "--reconstruct", "nowhere.wav"], "not a readable RIFF WAV")]


@pytest.mark.parametrize("extra,what", CLI_ERRORS, ids=[" ".join(e) for e, _ in CLI_ERRORS])
def test_cli_usage_errors(pkg, tmp_path, extra, what):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    x = (0.1 * np.sin(np.arange(22050) * 0.05)).astype(np.float32)
    assert pkg.lib().tts_write_wav(str(tmp_path / "in.wav").encode(), x, len(x), 22050) == 0
    files = {"IN": str(tmp_path / "in.wav"), "CODES": str(tmp_path / "codes.txt"), "BAD": str(tmp_path / "bad.txt"), "EMPTY": str(tmp_path / "empty.txt")}
    for key, text in (("CODES", "1 2 3\n"), ("BAD", "1 two 3\n"), ("EMPTY", "\n")):
        open(files[key], "w").write(text)
    r = subprocess.run([exe, "--models", str(tmp_path / "nowhere")] + [files.get(a, a) for a in extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and what in r.stderr, r.stderr
    assert ("usage:" in r.stderr or "not a readable" in r.stderr) and "model_load" not in r.stderr and not os.path.exists("m.bin")
