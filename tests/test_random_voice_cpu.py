"""Without a GPU: random voices (upstream's RandomLatentConverter; tts_load_random_voice / tts_random_voice, csrc/random_voice.h).

The model is restated from memory (tests/random_voice_ref.py). Here: the two float64 restatements agree to rounding; a float32 torch module written as upstream's
source, weight * scale inside forward, lies inside the kernel bound of tests/rlg_cases.py layer by layer (layerwise_ratio: every layer on its own input), and so
does a NumPy float32 restatement in the kernels' own order; nine seeded defects of the reference fall at least ten bounds outside; the loader's fold is torch's `weight * scale` and `bias * lr_mul` bit
for bit; the synthetic writer keeps upstream's initialisation with non-zero biases; tools/convert_weights.py round-trips a state dict; tts_host_blend_voices
against a literal restatement with its refusals; every refusal a host-only context can reach; every usage error of the CLI's --voice-random."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import random_voice_ref as R
import rlg_cases as K
from conftest import MODELS, ROOT

ERR_ARG, ERR_IO, ERR_FORMAT, ERR_HIP, ERR_STATE, ERR_LIMIT = -1, -2, -3, -4, -5, -6
EXE = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")


@pytest.fixture(scope="module")
def models(pkg):
    """{dim: (tensors, z [3, dim], float64 reference)}: computed once, shared, never changed"""
    from tortoise_cpp_amd import synth_weights as sw
    out = {}
    for dim, seed in ((256, 31), (1024, 32)):
        t = sw.random_voice_tensors(dim, seed)
        z = np.random.default_rng(dim).standard_normal((3, dim)).astype(np.float32)
        ref = R.forward_torch64(t, z)
        for a in (ref, z):
            a.setflags(write=False)
        out[dim] = (t, z, ref)
    return out


def test_synthetic_weights_are_upstreams_initialisation_with_biases(pkg):
    from tortoise_cpp_amd import synth_weights as sw
    t = sw.random_voice_tensors(256, 5)
    assert list(t) == list(sw.random_voice_tensor_shapes(256, 6)) and R.layers_of(t) == 6
    for l in range(5):
        w, b = t["layers.%d.weight" % l], t["layers.%d.bias" % l]
        assert w.shape == (256, 256) and w.dtype == np.float32 and 9.5 < w.std() < 10.5  # randn / lr_mul
        assert b.shape == (256,) and np.abs(b).min() > 0 and 1.5 < b.std() < 2.5          # not upstream's zeros
    assert np.abs(t["layers.5.weight"]).max() <= 1 / 16.0 and np.abs(t["layers.5.bias"]).min() > 0
    assert sw.random_voice_tensors(256, 5)["layers.3.weight"].tobytes() == t["layers.3.weight"].tobytes()
    assert sw.random_voice_tensors(256, 6)["layers.3.weight"].tobytes() != t["layers.3.weight"].tobytes()
    assert sw.random_voice_tensor_shapes(2048, 3) == {"layers.%d.%s" % (l, k): s for l in range(3) for k, s in (("weight", (2048, 2048)), ("bias", (2048,)))}


@pytest.mark.parametrize("dim", [256, 1024])
def test_two_float64_restatements_agree_to_rounding(models, dim):
    t, z, a = models[dim]
    b = R.forward_loops64(t, z[:2] if dim == 1024 else z)
    scale = np.abs(a).max()
    assert np.abs(a[:len(b)] - b).max() <= 1e-12 * scale
    assert scale > 0.1 and np.isfinite(a).all()
    assert max(K.layerwise_ratio(t, z, R.forward_torch64(t, z, all_layers=True))) < 1e-6  # the judge's own float64 layers are a third spelling


@pytest.mark.parametrize("dim", [256, 1024])
def test_upstreams_float32_module_is_inside_the_kernel_bound(models, dim):
    t, z, ref = models[dim]
    outs = R.forward_upstream32(t, z, all_layers=True)
    assert outs[-1].dtype == np.float32 and (outs[-1] == R.forward_upstream32(t, z)).all()
    ratios = K.layerwise_ratio(t, z, outs)
    print("dim %d: upstream's float32 module, worst error / bound per layer %s; final latent %.2e of its largest value from float64"
          % (dim, " ".join("%.3f" % r for r in ratios), np.abs(outs[-1] - ref).max() / np.abs(ref).max()))
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("dim", [256, 1024])
def test_float32_in_the_kernels_order_is_inside_the_bound(models, dim):
    t, z, ref = models[dim]
    zz = z[:1] if dim == 1024 else z
    outs = K.model_kernel_order32(t, zz)
    ratios = K.layerwise_ratio(t, zz, outs)
    print("dim %d: kernel-order float32, worst error / bound per layer %s; final latent %.2e of its largest value from float64"
          % (dim, " ".join("%.3f" % r for r in ratios), np.abs(outs[-1] - ref[:len(zz)]).max() / np.abs(ref).max()))
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_fall_ten_bounds_outside(models, defect):
    t, z, ref = models[256]
    ratios = K.layerwise_ratio(t, z, R.forward_torch64(t, z, mut=defect, all_layers=True))
    assert max(ratios) >= 10.0, (defect, ratios)
    assert sum(r >= 10.0 for r in ratios) <= (5 if defect in ("slope_0.1", "no_sqrt2", "scale_without_lr_mul", "lr_mul_twice", "bias_before_scale") else 1), (defect, ratios)


def test_defect_list_is_the_issues():
    assert len(R.DEFECTS) == 9 and len(set(R.DEFECTS)) == 9


@pytest.mark.parametrize("dim", [256, 1024, 2048])
def test_loaders_fold_is_torchs_product_bit_for_bit(pkg, dim):
    import torch
    r = np.random.default_rng(dim)
    w = (r.standard_normal((dim, dim)) * 10).astype(np.float32)
    b = (r.standard_normal(dim) * 2).astype(np.float32)
    wo, bo = pkg.host_random_voice_fold(w, b, True)
    lr_mul = 0.1
    for scale in (lr_mul / math.sqrt(dim), (1 / math.sqrt(dim)) * lr_mul):  # the issue's spelling and rosinality's: the same float32
        assert (torch.as_tensor(w) * scale).numpy().tobytes() == wo.tobytes()
    assert (torch.as_tensor(b) * lr_mul).numpy().tobytes() == bo.tobytes()
    wk, bk = K.fold32({"layers.0.weight": w, "layers.0.bias": b, "layers.1.weight": w, "layers.1.bias": b})[0]
    assert wk.tobytes() == wo.tobytes() and bk.tobytes() == bo.tobytes()  # the tests' own fold is the loader's
    wl, bl = pkg.host_random_voice_fold(w, b, False)
    assert wl.tobytes() == w.tobytes() and bl.tobytes() == b.tobytes()    # the last layer is not folded
    L = pkg.lib()
    assert L.tts_host_random_voice_fold(None, b.ctypes.data, dim, 1, wo.ctypes.data, bo.ctypes.data) == ERR_ARG
    assert L.tts_host_random_voice_fold(w.ctypes.data, b.ctypes.data, 0, 1, wo.ctypes.data, bo.ctypes.data) == ERR_ARG


# ---- converter ----------------------------------------------------------------------------------------------------------------------------------------

def _convert(tmp_path, sd, flag="--random-voice", expect_ok=True):
    import torch
    src = tmp_path / "rlg.pth"
    torch.save(sd, str(src))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), flag, str(src), "--out", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == expect_ok, r.stdout + r.stderr
    return r


def test_converter_round_trip_and_refusals(pkg, models, tmp_path):
    import torch
    from tortoise_cpp_amd import synth_weights as sw
    t = models[256][0]
    m = R.upstream_module(t)
    sd = m.state_dict()
    assert list(sd) == list(t)  # the module written as upstream's source names its tensors as the file does
    r = _convert(tmp_path, sd)
    assert "6 layers of 256 channels" in r.stdout
    back = sw.read_ggml(str(tmp_path / "out" / "ggml-random-voice-model.bin"))
    assert list(back) == list(t) and all(back[k].tobytes() == t[k].tobytes() and back[k].shape == t[k].shape for k in t)
    ref = tmp_path / "direct.bin"
    sw.write_random_voice(str(ref), 256, 31)
    assert ref.read_bytes() == (tmp_path / "out" / "ggml-random-voice-model.bin").read_bytes()
    _convert(tmp_path, sd, "--random-diffusion-voice")
    assert (tmp_path / "out" / "ggml-random-diffusion-voice-model.bin").read_bytes() == ref.read_bytes()
    for what, edit in (("unexpected", lambda d: d.update(extra=torch.zeros(3))), ("missing", lambda d: d.pop("layers.2.bias")),
                       ("shape", lambda d: d.update({"layers.1.weight": torch.zeros(256, 128)})), ("layers", lambda d: [d.pop(k) for k in list(d) if not k.startswith("layers.0.")])):
        bad = dict(sd)
        edit(bad)
        r = _convert(tmp_path, bad, expect_ok=False)
        assert "convert_random_voice" in r.stderr, (what, r.stderr)


def test_list_expected(pkg):
    from tortoise_cpp_amd import synth_weights as sw
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), "--list-expected", "random_voice"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("random_voice ")]
    want = [["random_voice", "(rlg_auto)", k, "x".join(map(str, s))] for k, s in sw.random_voice_tensor_shapes(1024, 6).items()] + \
           [["random_voice", "(rlg_diffuser)", k, "x".join(map(str, s))] for k, s in sw.random_voice_tensor_shapes(2048, 6).items()]
    assert rows == want and len(rows) == 24


# ---- the blend ----------------------------------------------------------------------------------------------------------------------------------------

def test_blend_voices_against_the_literal_restatement(pkg):
    one = np.array([[1.0, -2.0, 0.5]], np.float32)
    assert pkg.host_blend_voices(one).tolist() == [1.0, -2.0, 0.5]
    two = np.array([[1.0, 3.0], [3.0, 4.0]], np.float32)
    assert pkg.host_blend_voices(two).tolist() == [2.0, 3.5]                       # the mean: upstream's load_voices
    assert pkg.host_blend_voices(two, [3, 1]).tolist() == [1.5, 3.25]
    assert pkg.host_blend_voices(two, [0, 2]).tolist() == [3.0, 4.0]               # a zero weight is legal while the sum is positive
    assert pkg.host_blend_voices(two, [-1, 2]).tolist() == [5.0, 5.0]
    third = np.array([[0.1], [0.2], [0.4]], np.float32)
    assert pkg.host_blend_voices(third)[0] == np.float32((float(np.float32(0.1)) + float(np.float32(0.2)) + float(np.float32(0.4))) / 3.0)  # double sum, one rounding
    rs = np.random.RandomState(12)
    for trial in range(6):
        n, dim = int(rs.randint(1, 7)), int(rs.choice([1, 5, 1024, 2048]))
        x = (rs.randn(n, dim) * 10 ** rs.uniform(-3, 3)).astype(np.float32)
        w = None if trial % 2 == 0 else rs.uniform(0.1, 3.0, n).astype(np.float32)
        assert pkg.host_blend_voices(x, w).tobytes() == R.blend_literal(x, w).tobytes(), trial


def test_blend_voices_refusals(pkg):
    L = pkg.lib()
    x = np.ones((2, 4), np.float32)
    w = np.ones(2, np.float32)
    out = np.full(4, 7.0, np.float32)

    def call(lat=x, wt=w, n=2, dim=4, o=out):
        return L.tts_host_blend_voices(None if lat is None else lat.ctypes.data, None if wt is None else wt.ctypes.data, n, dim, None if o is None else o.ctypes.data)
    assert call() == 0 and out.tolist() == [1.0] * 4
    out[:] = 7.0
    bad_x = x.copy()
    bad_x[1, 2] = np.inf
    nan_x = x.copy()
    nan_x[0, 0] = np.nan
    for name, rc in (("no latents", call(lat=None)), ("no out", call(o=None)), ("n 0", call(n=0)), ("dim 0", call(dim=0)), ("n negative", call(n=-1)),
                     ("inf latent", call(lat=bad_x)), ("nan latent", call(lat=nan_x)), ("zero sum", call(wt=np.array([1, -1], np.float32))),
                     ("negative sum", call(wt=np.array([-1, -1], np.float32))), ("nan weight", call(wt=np.array([np.nan, 1], np.float32))),
                     ("inf weight", call(wt=np.array([np.inf, 1], np.float32))), ("all zero", call(wt=np.zeros(2, np.float32)))):
        assert rc == ERR_ARG, name
    assert out.tolist() == [7.0] * 4  # a refused call writes nothing
    for bad in (lambda: pkg.host_blend_voices(np.ones(4, np.float32)), lambda: pkg.host_blend_voices(x, [1.0]), lambda: pkg.host_blend_voices(x, [1.0, -1.0])):
        with pytest.raises(pkg.TtsError):
            bad()


# ---- a host-only context ------------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_a_host_only_context_can_reach(pkg, tmp_path):
    from tortoise_cpp_amd import synth_weights as sw
    e = pkg.Engine(-1)
    L, h = e.L, e.h
    err = lambda: L.tts_last_error(h).decode()  # noqa: E731
    try:
        good = sw.random_voice_tensors(256, 3)

        def write(name, tensors):
            p = str(tmp_path / name)
            w = sw.GgmlWriter(p)
            for k, v in tensors.items():
                w.add(k, v)
            w.close()
            return p.encode()
        ok = write("ok.bin", good)
        broken = {
            "non-square": dict(good, **{"layers.2.weight": np.zeros((256, 512), np.float32)}),
            "other size": dict(good, **{"layers.3.weight": np.zeros((512, 512), np.float32), "layers.3.bias": np.zeros(512, np.float32)}),
            "bias size": dict(good, **{"layers.1.bias": np.zeros(128, np.float32)}),
            "missing bias": {k: v for k, v in good.items() if k != "layers.4.bias"},
            "one layer": {k: v for k, v in good.items() if k.startswith("layers.0.")},
            "no layers": {"something.else": np.zeros(4, np.float32)},
            "unknown tensor": dict(good, extra=np.zeros(4, np.float32)),
            "a gap in the layers": {k: v for k, v in good.items() if not k.startswith("layers.3.")},
            "dim below the smallest": {"layers.%d.%s" % (l, k): np.zeros((128, 128) if k == "weight" else (128,), np.float32) for l in range(2) for k in ("weight", "bias")},
            "dim not a multiple of 256": {"layers.%d.%s" % (l, k): np.zeros((384, 384) if k == "weight" else (384,), np.float32) for l in range(2) for k in ("weight", "bias")},
            "weight with three dims": dict(good, **{"layers.0.weight": np.zeros((256, 256, 1), np.float32)}),
        }
        for name, tensors in broken.items():
            p = write("bad.bin", tensors)
            assert L.tts_load_random_voice(h, p, None) == ERR_FORMAT, (name, err())
            assert L.tts_load_random_voice(h, None, p) == ERR_FORMAT, (name, err())
            assert L.tts_load_random_voice(h, ok, p) == ERR_FORMAT, (name, err())  # the good side does not hide the broken one
        assert L.tts_load_random_voice(h, ok, None) == ERR_HIP and "host-only" in err()   # parsed, then no device
        assert L.tts_load_random_voice(h, ok, ok) == ERR_HIP
        assert L.tts_load_random_voice(h, None, None) == ERR_ARG
        assert L.tts_load_random_voice(h, str(tmp_path / "missing.bin").encode(), None) == ERR_IO
        (tmp_path / "garbage.bin").write_bytes(b"not a model file at all")
        assert L.tts_load_random_voice(h, str(tmp_path / "garbage.bin").encode(), None) in (ERR_FORMAT, ERR_IO)
        assert L.tts_load_random_voice(None, ok, None) == ERR_ARG
        for side in (0, 1, 2, -1):
            assert L.tts_random_voice_dim(h, side) == 0
        assert L.tts_random_voice_dim(None, 0) == 0
        seeds = np.array([1], np.uint64)
        out = np.full(2048, 3.0, np.float32)
        assert L.tts_random_voice(h, seeds.ctypes.data, 1, None, None, out.ctypes.data, None) == ERR_HIP
        assert L.tts_random_voice(None, seeds.ctypes.data, 1, None, None, out.ctypes.data, None) == ERR_ARG
        assert L.tts_random_voice_noise(h, 1, 0, out.ctypes.data, 2048) == ERR_HIP
        assert (out == 3.0).all()
        with pytest.raises(pkg.TtsError, match="status -4"):
            e.random_voice([1, 2])
        with pytest.raises(pkg.TtsError, match="status -3"):
            e.load_random_voice(auto=str(tmp_path / "bad.bin"))
        with pytest.raises(pkg.TtsError):
            e.random_voice([1], sides=("auto", "left"))
        assert e.random_voice_dim("auto") == 0 and e.random_voice_dim("diffusion") == 0
    finally:
        e.close()


def test_exports(pkg):
    L = pkg.lib()
    syms = pkg.header_symbols()
    for s in ("tts_load_random_voice", "tts_random_voice_dim", "tts_random_voice", "tts_random_voice_noise", "tts_host_blend_voices", "tts_host_random_voice_fold"):
        assert s in syms and hasattr(L, s), s
    assert L.tts_version() == 8
    hdr = open(pkg.HEADER).read()
    assert "#define TTS_RANDOM_VOICE_MAX 4096" in hdr and "stated from memory" in hdr


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------------

def cli(args, dry=False):
    assert os.path.exists(EXE), "the CLI is not built (__graft_entry__.build())"
    return subprocess.run([EXE, "--models", MODELS, "--seed", "11", "--codes", "9", "--message", "hello there."] + (["--dry-run", "1"] if dry else []) + args,
                          capture_output=True, text=True, timeout=120)


def test_cli_usage_errors_exit_1_before_any_model(tmp_path):
    f, g, wav = str(tmp_path / "f.bin"), str(tmp_path / "g.bin"), str(tmp_path / "out.wav")
    v, d = str(tmp_path / "v.bin"), str(tmp_path / "d.bin")
    np.zeros(1024, np.float32).tofile(v)
    np.zeros(2048, np.float32).tofile(d)
    both = ["--random-voice-model", f, "--random-diffusion-voice-model", g]
    cases = [
        (["--voice-random", "7"], False, "--random-voice-model"),                                                   # a missing model file
        (["--voice-random", "7", "--random-voice-model", f], False, "--random-diffusion-voice-model"),             # the diffusion decoder needs G
        (["--voice-random", "7"] + both, True, "--dry-run"),
        (["--voice-random", "7", "--devices", "2"] + both, False, "--devices"),
        (["--voice-random", "7", "--exchange", "rccl"] + both, False, "--exchange rccl"),
        (["--voice-random", "7", "--save-voice", "a", "--save-voice", "b"] + both, False, "--save-voice"),          # two prefixes for one voice
        (["--voice-random", "7", "--voice-random", "8", "--save-voice", "a"] + both, False, "--save-voice"),        # one prefix for two voices
        (["--voice-random", "7", "--voice", v] + both, False, "--diffusion-latent"),                                # the file voice beside it needs its latent
        (["--voice", v, "--diffusion-latent", d, "--diffusion-latent", d, "--voice-random", "7"] + both, False, "--diffusion-latent"),
        (["--random-voice-model", f], False, "--voice-random"),                                                     # the model without a voice
        (["--voice", v, "--random-diffusion-voice-model", g], False, "--voice-random"),
    ]
    for seed in ("-1", "x", "", "1.5", "0x10", "18446744073709551616", "7 ", "+7"):
        cases.append((["--voice-random", seed] + both, False, "unsigned 64-bit"))
    for args, dry, text in cases:
        r = cli(args + ["--output", wav], dry)
        assert r.returncode == 1 and text in r.stderr and r.stdout == "", (args, r.stdout, r.stderr)
    assert not os.path.exists(wav) and not os.path.exists("a.bin")


def test_cli_existing_command_lines_keep_their_meaning(tmp_path):
    """--voice random is still a FILE named `random`; --save-voice without a made voice still belongs to --voice-clips"""
    wav = str(tmp_path / "out.wav")
    r = subprocess.run([EXE, "--dry-run", "1", "--models", MODELS, "--seed", "11", "--codes", "9", "--message", "a.\n1|b.", "--voice", str(tmp_path / "random"),
                        "--voice", str(tmp_path / "random"), "--output", wav], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 1 and "Unable to" in r.stderr and str(tmp_path / "random") in r.stderr  # read as a file, and the file is not there
    np.zeros(1024, np.float32).tofile(str(tmp_path / "random"))
    r = subprocess.run([EXE, "--dry-run", "1", "--models", MODELS, "--seed", "11", "--codes", "9", "--message", "a.\n1|b.", "--voice", "random", "--voice", "random",
                        "--output", wav], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.splitlines()[0].startswith("chunk 0: voice 0"), r.stdout + r.stderr
    r = cli(["--save-voice", str(tmp_path / "p"), "--output", wav])
    assert r.returncode == 1 and "--voice-clips" in r.stderr
    # the largest seed is legal: the run gets past the usage checks (and fails later here, where there is no device or no such model file)
    r = cli(["--voice-random", "18446744073709551615", "--random-voice-model", str(tmp_path / "f.bin"), "--random-diffusion-voice-model", str(tmp_path / "g.bin"),
             "--output", wav])
    assert "unsigned 64-bit" not in r.stderr and r.returncode != 0
