"""GPU: the DDIM sampler of the diffusion stage (options "diff_sampler" = 1, "ddim_eta", "cond_free_k"; diffusion.hip: step_update_kernel, ddim_step_value).

The reference and the oracle have no DDIM. The yardstick is a host-driven loop over the engine's own network: per step two tts_diffusion_forward calls (conditioned and
conditioning-free) at the step's timestep, then the numpy float32 restatement of the update (tests/test_ddim_cpu.py: ddim_update, pinned there on a hand-checkable
case) with the scalars of the two host probes. The same loop drives the ancestral sampler (ddpm_update: main.cpp:5970-6030), which is the parent's behaviour — that
distance is the yardstick's self-check. Gate for both: conftest.loop_gate("small"), the distance the project accepts between two correct f32 evaluations of this loop.

Measured on an MI355X (profiles/ddim_sampler.txt): both distances are 0.0 — the device loop and the host-driven loop agree bit for bit, for both samplers.

Everything else is a bit-identity property the ancestral sampler already has (np.array_equal)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import loop_gate
from test_ddim_cpu import ddim_update, ddpm_update

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DEFAULTS = {"diff_sampler": 0, "ddim_eta": 0, "cond_free_k": 2.0, "share_uncond": 1, "hoist_integrator": 1, "diff_graph": 1, "latency_mode": 0,
            "rng_shard_offset": 0, "rng_shard_total": 0}


@pytest.fixture(scope="module")
def eng(pkg, small_models):
    e = pkg.Engine(0)
    e.load(small_models)
    yield e
    e.close()


class options:
    """engine options for the length of a with block; every one goes back to its default afterwards"""

    def __init__(self, e, **kw):
        self.e, self.kw = e, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.e.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.e.set_option(k, DEFAULTS[k])


def _latents(L, seed):
    return np.random.RandomState(seed).randn(L, 1024).astype(np.float32)


def host_loop(eng, pkg, lat, n, sampler, x_T, step_noise=None, eta=0.0, zero_k=False):
    """The sampling loop run from the host. x_T [100*T]; step_noise [n, 100*T] (vector idx is read by step idx) or None."""
    tm, s = pkg.host_schedule(n)
    d = pkg.host_schedule_ddim(n, eta)
    T = eng.frames(len(lat))
    x = np.ascontiguousarray(x_T, f32).reshape(100, T).copy()
    for idx in range(n):
        t = n - 1 - idx
        out_c = eng.diffusion_forward(lat, x, int(tm[t]), False)
        out_u = eng.diffusion_forward(lat, x, int(tm[t]), True)
        nz = None if step_noise is None else step_noise[idx].reshape(100, T)
        if sampler == "ddim":
            cfk = f32(0) if zero_k else s["cfk"][t]
            x = ddim_update(x, out_c[:100], out_u[:100], cfk, s["sqrt_recip"][t], s["sqrt_recipm1"][t], d["c_x0"][t], d["c_eps"][t], d["sigma"][t], t == 0, nz)
        else:
            assert not zero_k
            x = ddpm_update(x, out_c[:100], out_c[100:], out_u[:100], s, t, nz)
        x = np.ascontiguousarray(x, f32)
    return x


# ---- 5. / 6. / 9. the update rule, through the loop ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_steps", [12, 30])
def test_host_driven_loop(eng, pkg, n_steps):
    lat = _latents(43, 43)
    T = eng.frames(43)
    noise = np.random.RandomState(n_steps).randn(n_steps + 1, 100 * T).astype(np.float32)
    gate = loop_gate("small")
    with options(eng, diff_sampler=1, ddim_eta=0):
        got = eng.diffusion([lat], n_steps=n_steps, noise=[noise[0]])[0]
    want = host_loop(eng, pkg, lat, n_steps, "ddim", noise[0])
    d_ddim = float(np.abs(got - want).max())
    got_p = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    want_p = host_loop(eng, pkg, lat, n_steps, "ddpm", noise[0], noise[1:])
    d_ddpm = float(np.abs(got_p - want_p).max())
    print("host-driven loop, %d steps, L = 43 (T = %d): DDIM eta 0 max abs %.3e, DDPM (self-check) max abs %.3e, gate %.3e" % (n_steps, T, d_ddim, d_ddpm, gate))
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0  # the last step returns the clipped x0
    assert np.abs(got - got_p).max() > 1e-3  # two samplers
    assert d_ddpm <= gate, (d_ddpm, gate)
    assert d_ddim <= gate, (d_ddim, gate)


def test_eta_half_with_explicit_noise(eng, pkg):
    n_steps, lat = 12, _latents(43, 43)
    T = eng.frames(43)
    noise = np.random.RandomState(5).randn(n_steps + 1, 100 * T).astype(np.float32)
    with options(eng, diff_sampler=1, ddim_eta=0.5):
        got = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
        last = noise.copy()
        last[n_steps] = 7.0  # the last vector is drawn and unused, as in the ancestral sampler
        assert np.array_equal(got, eng.diffusion([lat], n_steps=n_steps, noise=[last])[0])
    want = host_loop(eng, pkg, lat, n_steps, "ddim", noise[0], noise[1:], eta=0.5)
    dist = float(np.abs(got - want).max())
    print("host-driven loop, 12 steps, eta 0.5, explicit noise: max abs %.3e, gate %.3e" % (dist, loop_gate("small")))
    assert dist <= loop_gate("small")
    with options(eng, diff_sampler=1, ddim_eta=0):
        det = eng.diffusion([lat], n_steps=n_steps, noise=[noise[0]])[0]
    assert np.abs(det - got).max() > 1e-3  # eta is live


@pytest.mark.parametrize("rows", [[43], [43, 12]], ids=["one candidate", "two candidates"])
def test_eta_zero_reference_noise_is_x_T_alone(eng, pkg, rows):
    """eta = 0: TTS_NOISE_REFERENCE draws exactly 100 T_c normals per candidate, candidate after candidate, and nothing else (one candidate: the pipelined-draw path)."""
    n_steps, lats = 12, [_latents(L, L) for L in rows]
    sizes = [100 * eng.frames(L) for L in rows]
    eng.seed(321)
    x_T = [eng.rng_normal(n) for n in sizes]
    u_want = eng.rng_uniform()
    with options(eng, diff_sampler=1, ddim_eta=0):
        explicit = eng.diffusion(lats, n_steps=n_steps, noise=x_T)
        eng.seed(321)
        drawn = eng.diffusion(lats, n_steps=n_steps, noise_mode=pkg.NOISE_REFERENCE)
        u_got = eng.rng_uniform()
    for a, b in zip(explicit, drawn):
        assert np.array_equal(a, b), float(np.abs(a - b).max())
    assert u_got == u_want, (u_got, u_want)


def test_cond_free_k_is_live(eng, pkg):
    n_steps, lat = 12, _latents(43, 43)
    T = eng.frames(43)
    noise = np.random.RandomState(6).randn(n_steps + 1, 100 * T).astype(np.float32)
    ddpm2 = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    with options(eng, cond_free_k=0):
        ddpm0 = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    with options(eng, diff_sampler=1):
        ddim2 = eng.diffusion([lat], n_steps=n_steps, noise=[noise[0]])[0]
        with options(eng, cond_free_k=0):
            ddim0 = eng.diffusion([lat], n_steps=n_steps, noise=[noise[0]])[0]
    assert np.abs(ddpm0 - ddpm2).max() > 1e-3 and np.abs(ddim0 - ddim2).max() > 1e-3
    want = host_loop(eng, pkg, lat, n_steps, "ddim", noise[0], zero_k=True)
    dist = float(np.abs(ddim0 - want).max())
    print("host-driven loop, 12 steps, cond_free_k = 0: max abs %.3e, gate %.3e" % (dist, loop_gate("small")))
    assert dist <= loop_gate("small")


# ---- 7. bit-identity properties ---------------------------------------------------------------------------------------------------------------------------

RAGGED = [12, 43, 43, 7, 100]
N_PROP = 8


def _ragged(eng):
    lats = [_latents(L, 10 + i) for i, L in enumerate(RAGGED)]
    rs = np.random.RandomState(77)
    x_T = [rs.randn(100 * eng.frames(L)).astype(np.float32) for L in RAGGED]
    return lats, x_T


def test_ragged_batch_equals_each_candidate_alone(eng):
    lats, x_T = _ragged(eng)
    with options(eng, diff_sampler=1):
        batch = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
        for c in range(len(lats)):
            alone = eng.diffusion([lats[c]], n_steps=N_PROP, noise=[x_T[c]])[0]
            assert np.array_equal(batch[c], alone), (c, float(np.abs(batch[c] - alone).max()))
        again = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)  # two consecutive calls
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))
    assert np.abs(batch[1] - batch[2]).max() > 1e-3  # same length, other latents and x_T


@pytest.mark.parametrize("opt", ["diff_graph", "hoist_integrator", "share_uncond"])
@pytest.mark.parametrize("eta", [0, 0.5])
def test_option_changes_no_bit(eng, opt, eta):
    lats, x_T = _ragged(eng)
    rs = np.random.RandomState(78)
    noise = x_T if eta == 0 else [np.concatenate([x, rs.randn(N_PROP * len(x)).astype(np.float32)]) for x in x_T]
    with options(eng, diff_sampler=1, ddim_eta=eta):
        on = eng.diffusion(lats, n_steps=N_PROP, noise=noise)
        with options(eng, **{opt: 0}):
            off = eng.diffusion(lats, n_steps=N_PROP, noise=noise)
    for c in range(len(lats)):
        assert np.array_equal(on[c], off[c]), (opt, c, float(np.abs(on[c] - off[c]).max()))


def test_multi_voice_equals_each_candidate_alone_with_its_voice(eng, small_models):
    from test_multi_voice_gpu import diff_voices
    vlat, own = diff_voices(small_models, 2)
    lats, x_T = _ragged(eng)
    vmap = [1, 0, 1, 1, 0]
    with options(eng, diff_sampler=1):
        multi = eng.diffusion(lats, n_steps=N_PROP, noise=x_T, voice_latents=vlat, voice_of_candidate=vmap)
        plain = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
        try:
            for c in range(len(lats)):
                eng.set_diffusion_conditioning_latent(vlat[vmap[c]])
                alone = eng.diffusion([lats[c]], n_steps=N_PROP, noise=[x_T[c]])[0]
                assert np.array_equal(multi[c], alone), (c, float(np.abs(multi[c] - alone).max()))
                assert np.abs(multi[c] - plain[c]).max() > 1e-3, c
        finally:
            eng.set_diffusion_conditioning_latent(own)


def test_latency_mode_batch_of_two_equals_the_same_mode_alone(eng):
    lats, x_T = _ragged(eng)
    lats, x_T = lats[1:3], x_T[1:3]
    with options(eng, diff_sampler=1, latency_mode=1):
        pair = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
        for c in range(2):
            alone = eng.diffusion([lats[c]], n_steps=N_PROP, noise=[x_T[c]])[0]
            assert np.array_equal(pair[c], alone), (c, float(np.abs(pair[c] - alone).max()))


@pytest.mark.parametrize("eta", [0, 0.5])
def test_device_noise_shards_reproduce_one_batch(eng, pkg, eta):
    lats = [_latents(L, 30 + i) for i, L in enumerate([43, 12, 43, 20])]
    eng.seed(99)
    with options(eng, diff_sampler=1, ddim_eta=eta):
        whole = eng.diffusion(lats, n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
        parts = []
        for r in range(2):
            with options(eng, rng_shard_offset=2 * r, rng_shard_total=4):
                parts += eng.diffusion(lats[2 * r:2 * r + 2], n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
    for c in range(4):
        assert np.array_equal(whole[c], parts[c]), (c, float(np.abs(whole[c] - parts[c]).max()))
    assert np.abs(whole[0] - whole[2]).max() > 1e-3  # same length: the candidates' streams differ


# ---- 8. nothing existing moved -----------------------------------------------------------------------------------------------------------------------------

def test_ddpm_bits_after_ddim_equal_a_fresh_context(eng, pkg, small_models):
    n_steps, lat = 80, _latents(12, 3)
    T = eng.frames(12)
    noise = np.random.RandomState(4).randn(n_steps + 1, 100 * T).astype(np.float32)
    with options(eng, diff_sampler=1, ddim_eta=0.5, cond_free_k=1.0):
        eng.diffusion([lat], n_steps=20, noise=[noise[:21]])
    after = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    eng.set_option("cond_free_k", 2.0)
    explicit = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    fresh = pkg.Engine(0)
    try:
        fresh.load(diffusion=small_models + "/ggml-diffusion-model.bin")
        want = fresh.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    finally:
        fresh.close()
    assert np.array_equal(after, want) and np.array_equal(explicit, want)


# ---- 10. end to end through the CLI -----------------------------------------------------------------------------------------------------------------------

def test_cli_sampler_ddim(eng, pkg, small_models, voice, tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    msg = "this is a test message."
    wavs = {}
    for sampler in ("ddim", "ddpm"):
        out = tmp_path / (sampler + ".wav")
        r = subprocess.run([exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--seed", "3", "--codes", "40",
                            "--sampler", sampler, "--steps", "20", "--timing", "1", "--output", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "[timing] sampler %s, ddim-eta 0, cond-free-k 2, steps 20\n" % sampler in r.stderr
        raw = out.read_bytes()
        assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
        wavs[sampler] = np.frombuffer(raw[44:], np.float32)
    # the same pipeline through the Python wrapper: the CLI's seed and RNG order (one candidate: reference-order noise from the context's generator)
    eng.tokenizer_load(str(d / "tokenizer.json"))
    eng.seed(3)
    codes, rows, lats, _ = eng.autoregressive(eng.tokenize(msg), voice, 1, 40, mask_stop=True)
    with options(eng, diff_sampler=1):
        mels = eng.diffusion(lats, n_steps=20)
    audio = eng.vocoder(mels)[0]
    assert len(wavs["ddim"]) == len(audio) == len(wavs["ddpm"])
    assert np.array_equal(wavs["ddim"], audio)
    assert np.abs(wavs["ddim"] - wavs["ddpm"]).max() > 1e-4
