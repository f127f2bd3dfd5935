"""Size-independent properties of the device path at sizes the CPU oracle cannot reach in seconds: run-to-run
determinism (no atomics, no races in the pipelined kernels), batch invariance (a candidate's result does not
depend on who shares the batch), and the bench-sized shapes end to end (mid-size weights, 16 candidates)."""
import numpy as np
import pytest

from conftest import DEFAULT_TOKENS

pytestmark = pytest.mark.gpu


def _latents(L, seed):
    return np.random.RandomState(seed).randn(L, 1024).astype(np.float32)


def test_decode_is_batch_invariant_and_deterministic(engine, mid_models, voice):
    """16 candidates fed identical tokens produce bit-identical logits rows, twice in a row."""
    engine.load(ar=mid_models + "/ggml-model.bin")
    runs = []
    for _ in range(2):
        engine.ar_begin(DEFAULT_TOKENS, voice, 16, 12)
        lg = [engine.ar_prefill()]
        for i in range(10):
            lg.append(engine.ar_step(np.full(16, 37 + i, np.int32), i))
        runs.append(np.stack(lg))
    a, b = runs
    assert np.isfinite(a).all()
    assert (a == b).all(), "decode is not run-to-run deterministic"
    assert (a == a[:, :1]).all(), "identical candidates got different logits"
    # one candidate alone sees the same numbers as inside the batch
    engine.ar_begin(DEFAULT_TOKENS, voice, 1, 12)
    solo = [engine.ar_prefill()]
    for i in range(10):
        solo.append(engine.ar_step(np.full(1, 37 + i, np.int32), i))
    assert (np.stack(solo)[:, 0] == a[:, 0]).all(), "batch of 1 differs from batch of 16"


def test_stream_cus_partition_does_not_change_results(pkg, small_models, voice):
    """Option stream_cus confines a context's stream to n CUs of every XCD (n > 0) or keeps it off them (n < 0): two contexts of one
    process can split the chip. No kernel may depend on how many CUs it runs on: ids, latents and mel are bit-identical."""
    lat = _latents(9, 3)
    outs = []
    for cus in (0, 2, -2):
        e = pkg.Engine(0)
        e.set_option("stream_cus", cus)
        e.load(small_models)
        with pytest.raises(pkg.TtsError, match="before the models are loaded"):
            e.set_option("stream_cus", 1)
        e.seed(11)
        codes, rows, lats, _ = e.autoregressive(DEFAULT_TOKENS, voice, 3, 12, mask_stop=True)
        mel = e.diffusion([lat], n_steps=4, noise_mode=pkg.NOISE_DEVICE)[0]
        outs.append((codes, np.concatenate(lats), mel))
        e.close()
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert (x == y).all()
    e = pkg.Engine(0)
    with pytest.raises(pkg.TtsError, match="CUs per XCD"):
        e.set_option("stream_cus", 32)
    e.close()


def test_autoregressive_driver_bench_shape(engine, mid_models, voice):
    """tts_autoregressive at the bench's shape (16 candidates, stop masked): reproducible for a fixed seed, different
    across candidates, and the latent rows follow the trim rule."""
    engine.load(ar=mid_models + "/ggml-model.bin")
    out = []
    for _ in range(2):
        engine.seed(5)
        codes, rows, lats, steps = engine.autoregressive(DEFAULT_TOKENS, voice, 16, 48, mask_stop=True)
        out.append((codes.copy(), rows.copy(), [l.copy() for l in lats]))
    assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all()
    for x, y in zip(out[0][2], out[1][2]):
        assert (x == y).all()
    codes, rows, lats = out[0]
    assert codes.shape == (16, 502) and (codes[:, 0] == 8192).all() and (codes[:, -1] == 8193).all()
    assert len({tuple(c) for c in codes}) > 1, "all candidates sampled the same sequence"
    for c in range(16):
        assert lats[c].shape == (rows[c], 1024) and np.isfinite(lats[c]).all()


@pytest.mark.parametrize("noise_mode", ["explicit", "device"])
def test_diffusion_batch_invariance(engine, mid_models, pkg, noise_mode):
    """A candidate's mel does not depend on the other sequences packed into the batch (guard rows, per-sequence
    GroupNorm / attention, row-shifted conv segments), and the loop is deterministic."""
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    lats = [_latents(61, 1), _latents(200, 2), _latents(17, 3), _latents(130, 4)]  # T = 265, 870, 74, 565
    n_steps = 3
    if noise_mode == "explicit":
        rs = np.random.RandomState(8)
        noise = [rs.randn(n_steps + 1, 100 * engine.frames(len(l))).astype(np.float32) for l in lats]
        batch = engine.diffusion(lats, n_steps=n_steps, noise=noise)
        again = engine.diffusion(lats, n_steps=n_steps, noise=noise)
        for c in range(len(lats)):
            assert (batch[c] == again[c]).all(), "diffusion is not deterministic"
            solo = engine.diffusion([lats[c]], n_steps=n_steps, noise=[noise[c]])[0]
            err = np.abs(solo - batch[c]).max()
            assert err < 1e-4, (c, err)  # same math per row; only tile/row placement differs
    else:
        engine.seed(3)
        a = engine.diffusion(lats, n_steps=n_steps, noise_mode=pkg.NOISE_DEVICE)
        engine.seed(3)
        b = engine.diffusion(lats, n_steps=n_steps, noise_mode=pkg.NOISE_DEVICE)
        for x, y in zip(a, b):
            assert (x == y).all() and np.isfinite(x).all() and np.abs(x).max() <= 1.0 + 1e-6


def test_diffusion_shared_unconditioned_integrator(engine, mid_models):
    """Unconditioned sequences of equal length share one evaluation of the conditioning_timestep_integrator layers
    (option share_uncond, default on). Same math per row: the mel must agree with the unshared evaluation and with a
    batch of one to rounding level."""
    engine.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    lats = [_latents(61, 1), _latents(61, 5), _latents(130, 4), _latents(61, 6)]  # T = 265, 265, 565, 265
    n_steps = 3
    rs = np.random.RandomState(9)
    noise = [rs.randn(n_steps + 1, 100 * engine.frames(len(l))).astype(np.float32) for l in lats]
    try:
        engine.set_option("share_uncond", 1)
        shared = engine.diffusion(lats, n_steps=n_steps, noise=noise)
        engine.set_option("share_uncond", 0)
        plain = engine.diffusion(lats, n_steps=n_steps, noise=noise)
    finally:
        engine.set_option("share_uncond", 1)
    for c in range(len(lats)):
        assert np.isfinite(shared[c]).all()
        err = np.abs(shared[c] - plain[c]).max()
        assert err < 1e-4, (c, err)
        solo = engine.diffusion([lats[c]], n_steps=n_steps, noise=[noise[c]])[0]
        err = np.abs(solo - shared[c]).max()
        assert err < 1e-4, (c, err)
    assert np.abs(shared[0] - shared[1]).max() > 1e-3  # different latents and noise: the candidates are not copies


def test_vocoder_batch_invariance(engine, mid_models):
    engine.load(vocoder=mid_models + "/ggml-vocoder-model.bin")
    rs = np.random.RandomState(4)
    Ts = [870, 33, 265, 1]
    mels = [np.clip(rs.randn(100, T) * 0.5, -1, 1).astype(np.float32) for T in Ts]
    noise = [rs.randn(64, T + 10).astype(np.float32) for T in Ts]
    batch = engine.vocoder(mels, noise=noise)
    again = engine.vocoder(mels, noise=noise)
    for c, T in enumerate(Ts):
        assert batch[c].shape == ((T + 10) * 256 - 6,)
        assert (batch[c] == again[c]).all(), "vocoder is not deterministic"
        solo = engine.vocoder([mels[c]], noise=[noise[c]])[0]
        scale = np.abs(solo).max()
        assert np.abs(solo - batch[c]).max() <= 1e-5 * scale, c


def test_cli_end_to_end(small_models, tmp_path):
    """The drop-in CLI (reference flags + --models/--codes) writes a 24 kHz float WAV; same seed -> same bytes."""
    import os, shutil, struct, subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    if not os.path.exists(exe):
        pytest.skip("CLI binary not built")
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    outs = []
    for k in range(2):
        out = tmp_path / ("out%d.wav" % k)
        r = subprocess.run([exe, "--models", str(d), "--message", "this is a test message.", "--voice",
                            os.path.join(ROOT, "models", "mol.bin"), "--seed", "0", "--codes", "24", "--steps", "4",
                            "--output", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append(out.read_bytes())
    b = outs[0]
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE"
    fmt_tag, channels, rate = struct.unpack("<HHI", b[20:28])
    assert (fmt_tag, channels, rate) == (3, 1, 24000)  # IEEE float, mono, 24 kHz (main.cpp:4821-4868)
    assert len(b) > 44 + 4 * 24000 // 10 and outs[0] == outs[1]


def test_bench_contract_quick():
    """bench.py --full prints ONE JSON line with the contract's keys (tiny layer counts: plumbing only, not a measurement)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--quick", "--steps", "1", "--warmup", "1", "--candidates", "4",
                        "--decode-steps", "24", "--diff-steps", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["value"] > 0 and d["n_gpus"] == 1 and d["steps"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] > 0 and rf["achieved"] > 0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and "traffic" in rf
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == d["unit"] and cb["sample"]


def test_bench_plain_quick_dumps_outputs(tmp_path):
    """A plain bench.py run (no --full): the headline keys only, and --dump-outputs writes the last timed pass's codes, latents, mels and audio
    (tiny layer counts: plumbing only, not a measurement)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--quick", "--steps", "2", "--warmup", "1", "--candidates", "4",
                        "--decode-steps", "24", "--diff-steps", "4", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "stage_ms_per_step", "load_ms"):
        assert k in out, k
    for k in ("roofline", "roofline_decode", "cpu_baseline", "other_share_uncond_setting", "ragged_batch", "clvp_ms"):
        assert k not in out, k
    assert out["steps"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0 and out["diffusion_time_mlp_retries"] == 0
    a = {k: np.load(d / (k + ".npy")) for k in ("codes", "latent_rows", "latents", "mel_frames", "mel", "audio_samples", "audio")}
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in a) and set(out["dump_outputs"]) == set(a)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert a["codes"].shape[0] == 4 and (a["codes"] >= 0).all() and (a["codes"] < 8194).all()
    rows, T, n = (a[k].astype(int) for k in ("latent_rows", "mel_frames", "audio_samples"))
    assert a["latents"].shape == (4, rows.max(), 1024) and a["mel"].shape == (4, 100, T.max()) and a["audio"].shape == (4, n.max())
    assert all(np.abs(a["audio"][i, :n[i]]).max() > 0 and np.abs(a["mel"][i, :, :T[i]]).max() > 0 for i in range(4))
