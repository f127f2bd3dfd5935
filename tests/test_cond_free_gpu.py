"""GPU: unguided sampling (option "cond_free" 0) and the diffusion temperature (option "diff_temperature") of the diffusion stage (diffusion.hip: step_xt_kernel,
step_update_kernel, step_eps, scale_xT_kernel).

Upstream tortoise-tts' p_mean_variance with conditioning_free=False takes the conditioned output as eps; the reference and the oracle always guide. The yardstick
is tests/test_ddim_gpu.py's host-driven loop with ONE tts_diffusion_forward call per step (the conditioned branch) and the numpy float32 restatements of the three
updates called with eps_u = eps_c and cfk = 0, which return eps_c exactly. Gate: conftest.loop_gate("small"), the distance the project accepts between two correct
f32 evaluations of this loop (the guided loops measure 0.0 there).

Measured on an MI355X (profiles/cond_free.txt): all four distances are 0.0.

Everything else is a bit-identity property (np.array_equal): against the guided run at k = 0 (the mixing expression at cfk = 0 returns eps_c for every finite eps_u
up to the sign of an exact zero, which == ignores), against each candidate alone, across the options that must not change a bit, and for the temperature against
a caller who scaled x_T with one float32 multiply. Shapes: L = 43 (T = 187: 512 packed rows guided, 256 unguided) with 12 steps for loops;
RAGGED with 8 steps for properties."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import loop_gate
from test_ddim_cpu import ddim_update, ddpm_update
from test_dpmpp_cpu import dpmpp_update

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DEFAULTS = {"diff_sampler": 0, "ddim_eta": 0, "cond_free_k": 2.0, "cond_free": 1, "diff_temperature": 1.0, "share_uncond": 1, "hoist_integrator": 1, "diff_graph": 1,
            "latency_mode": 0, "rng_shard_offset": 0, "rng_shard_total": 0}
RAGGED = [12, 43, 43, 7, 100]
N_PROP = 8
N_LOOP = 12
# (id, options, per-step noise)
SAMPLERS = [("ddpm", dict(diff_sampler=0), True), ("ddim_eta0", dict(diff_sampler=1, ddim_eta=0), False), ("ddim_eta0.5", dict(diff_sampler=1, ddim_eta=0.5), True),
            ("dpmpp2m", dict(diff_sampler=3), False)]


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


def _noise(eng, rows, n_steps, per_step, seed):
    """tts_diffusion's layout: per candidate x_T, then (per_step) one vector per step."""
    rs = np.random.RandomState(seed)
    return [rs.randn((n_steps + 1) if per_step else 1, 100 * eng.frames(L)).astype(np.float32) for L in rows]


def _ragged(eng, per_step=False):
    return [_latents(L, 10 + i) for i, L in enumerate(RAGGED)], _noise(eng, RAGGED, N_PROP, per_step, 77)


# ---- 1. the branch is gone ------------------------------------------------------------------------------------------------------------------------------------

def test_the_unconditioned_branch_is_gone(eng, pkg):
    lat = _latents(43, 43)
    x_T = _noise(eng, [43], 2, False, 1)
    with options(eng, diff_sampler=1):
        eng.diffusion([lat], n_steps=2, noise=x_T)
        assert eng.diffusion_last_layout() == (pkg.host_diff_packed_rows([43]), 2)
        with options(eng, cond_free=0):
            eng.diffusion([lat], n_steps=2, noise=x_T)
            assert eng.diffusion_last_layout() == (pkg.host_diff_packed_rows([43], cond_free=False), 1)
            assert pkg.host_diff_packed_rows([43], cond_free=False) < pkg.host_diff_packed_rows([43])
            lats, nz = _ragged(eng)
            eng.diffusion(lats, n_steps=2, noise=nz)
            assert eng.diffusion_last_layout() == (pkg.host_diff_packed_rows(RAGGED, cond_free=False), 5)
        with options(eng, cond_free_k=0):  # guided at k = 0 still evaluates both branches
            eng.diffusion([lat], n_steps=2, noise=x_T)
            assert eng.diffusion_last_layout() == (pkg.host_diff_packed_rows([43]), 2)


def test_last_layout_before_a_call(pkg, small_models):
    fresh = pkg.Engine(0)
    try:
        fresh.load(diffusion=small_models + "/ggml-diffusion-model.bin")
        with pytest.raises(pkg.TtsError, match=r"status -5"):
            fresh.diffusion_last_layout()
    finally:
        fresh.close()


# ---- 2. the independent yardstick: a host-driven loop -------------------------------------------------------------------------------------------------------

def unguided_host_loop(eng, pkg, lat, n, sampler, x_T, step_noise=None, eta=0.0):
    """The unguided sampling loop run from the host: ONE network evaluation per step. x_T [100*T]; step_noise [n, 100*T] (vector idx is read by step idx) or None."""
    tm, s = pkg.host_schedule(n)
    s0 = dict(s, cfk=np.zeros_like(s["cfk"]))
    d = pkg.host_schedule_ddim(n, 0.0 if sampler == "dpmpp2m" else eta)
    p = pkg.host_schedule_dpmpp(n)
    T = eng.frames(len(lat))
    x = np.ascontiguousarray(x_T, f32).reshape(100, T).copy()
    hist = None
    for idx in range(n):
        t = n - 1 - idx
        out_c = eng.diffusion_forward(lat, x, int(tm[t]), False)
        eps_c = out_c[:100]
        nz = None if step_noise is None else step_noise[idx].reshape(100, T)
        if sampler == "ddim":
            x = ddim_update(x, eps_c, eps_c, f32(0), s["sqrt_recip"][t], s["sqrt_recipm1"][t], d["c_x0"][t], d["c_eps"][t], d["sigma"][t], t == 0, nz)
        elif sampler == "dpmpp2m":
            x, hist = dpmpp_update(x, eps_c, eps_c, f32(0), s["sqrt_recip"][t], s["sqrt_recipm1"][t], d["c_x0"][t], d["c_eps"][t], p["a"][t], p["b"][t], p["c"][t],
                                   int(p["order"][t]), t == 0, hist)
        else:
            x = ddpm_update(x, eps_c, out_c[100:], eps_c, s0, t, nz)
        x = np.ascontiguousarray(x, f32)
    return x


@pytest.mark.parametrize("name,opts,per_step", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_host_driven_loop(eng, pkg, name, opts, per_step):
    lat = _latents(43, 43)
    noise = _noise(eng, [43], N_LOOP, per_step, 5)
    gate = loop_gate("small")
    with options(eng, cond_free=0, **opts):
        got = eng.diffusion([lat], n_steps=N_LOOP, noise=noise)[0]
    kind = "ddpm" if name == "ddpm" else "dpmpp2m" if name == "dpmpp2m" else "ddim"
    want = unguided_host_loop(eng, pkg, lat, N_LOOP, kind, noise[0][0], noise[0][1:] if per_step else None, eta=opts.get("ddim_eta", 0.0))
    dist = float(np.abs(got - want).max())
    print("unguided host-driven loop, %s, %d steps, L = 43 (T = %d): max abs %.3e, gate %.3e" % (name, N_LOOP, eng.frames(43), dist, gate))
    assert np.isfinite(got).all()
    if name != "ddpm":
        assert np.abs(got).max() <= 1.0  # the last step returns the clipped x0
    assert dist <= gate, (name, dist, gate)


# ---- 3. unguided = guided at k = 0 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,opts,per_step", SAMPLERS, ids=[s[0] for s in SAMPLERS])
def test_unguided_equals_guided_at_k_zero(eng, name, opts, per_step):
    lat = _latents(43, 43)
    noise = _noise(eng, [43], N_LOOP, per_step, 6)
    with options(eng, **opts):
        k2 = eng.diffusion([lat], n_steps=N_LOOP, noise=noise)[0]
        with options(eng, cond_free_k=0):
            k0 = eng.diffusion([lat], n_steps=N_LOOP, noise=noise)[0]
        with options(eng, cond_free=0):
            off = eng.diffusion([lat], n_steps=N_LOOP, noise=noise)[0]
            with options(eng, cond_free_k=7.5):  # validated and not read
                off_k = eng.diffusion([lat], n_steps=N_LOOP, noise=noise)[0]
    assert np.array_equal(off, k0), (name, float(np.abs(off - k0).max()))
    assert np.array_equal(off, off_k), name
    assert np.abs(off - k2).max() > 1e-3 and np.abs(k0 - k2).max() > 1e-3, name


# ---- 4. bit-identity properties under cond_free 0 -----------------------------------------------------------------------------------------------------------

def test_ragged_batch_equals_each_candidate_alone(eng):
    lats, x_T = _ragged(eng)
    with options(eng, diff_sampler=1, cond_free=0):
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
    lats, noise = _ragged(eng, per_step=eta != 0)
    with options(eng, diff_sampler=1, ddim_eta=eta, cond_free=0):
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
    with options(eng, diff_sampler=1, cond_free=0):
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


@pytest.mark.parametrize("eta", [0, 0.5])
def test_device_noise_shards_reproduce_one_batch(eng, pkg, eta):
    lats = [_latents(L, 30 + i) for i, L in enumerate([43, 12, 43, 20])]
    eng.seed(99)
    with options(eng, diff_sampler=1, ddim_eta=eta, cond_free=0):
        whole = eng.diffusion(lats, n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
        parts = []
        for r in range(2):
            with options(eng, rng_shard_offset=2 * r, rng_shard_total=4):
                parts += eng.diffusion(lats[2 * r:2 * r + 2], n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
    for c in range(4):
        assert np.array_equal(whole[c], parts[c]), (c, float(np.abs(whole[c] - parts[c]).max()))
    assert np.abs(whole[0] - whole[2]).max() > 1e-3  # same length: the candidates' streams differ


def test_latency_mode_pair_of_100_rows_equals_the_same_mode_alone(eng, pkg):
    """latency_mode 1 on two unguided 100-row utterances (896 packed rows: under the mode's row limit): the pair equals each alone in the same mode"""
    lats = [_latents(100, 50), _latents(100, 51)]
    x_T = _noise(eng, [100, 100], N_PROP, False, 52)
    assert pkg.host_diff_packed_rows([100, 100], cond_free=False) == 896
    with options(eng, diff_sampler=1, cond_free=0, latency_mode=1):
        pair = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
        for c in range(2):
            alone = eng.diffusion([lats[c]], n_steps=N_PROP, noise=[x_T[c]])[0]
            assert np.array_equal(pair[c], alone), (c, float(np.abs(pair[c] - alone).max()))
    assert np.isfinite(pair[0]).all()


# ---- 5. temperature, in each noise mode ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,opts,per_step", SAMPLERS[:2], ids=[s[0] for s in SAMPLERS[:2]])
@pytest.mark.parametrize("cond_free", [1, 0])
def test_temperature_explicit_noise(eng, name, opts, per_step, cond_free):
    rows = [43, 12]
    lats = [_latents(L, L) for L in rows]
    noise = _noise(eng, rows, N_LOOP, per_step, 8)
    scaled = [n.copy() for n in noise]
    for n in scaled:
        n[0] = f32(0.7) * n[0]  # block 0 only: the step blocks are never scaled
    with options(eng, cond_free=cond_free, **opts):
        one = eng.diffusion(lats, n_steps=N_LOOP, noise=noise)
        want = eng.diffusion(lats, n_steps=N_LOOP, noise=scaled)
        with options(eng, diff_temperature=0.7):
            got = eng.diffusion(lats, n_steps=N_LOOP, noise=noise)
    for c in range(len(rows)):
        assert np.array_equal(got[c], want[c]), (name, c, float(np.abs(got[c] - want[c]).max()))
        assert np.abs(got[c] - one[c]).max() > 1e-3, (name, c)


@pytest.mark.parametrize("rows", [[43], [43, 12]], ids=["one candidate (pipelined draws)", "two candidates"])
@pytest.mark.parametrize("name,opts,per_step", SAMPLERS[:2], ids=[s[0] for s in SAMPLERS[:2]])
def test_temperature_reference_noise(eng, pkg, rows, name, opts, per_step):
    n_steps, lats = N_LOOP, [_latents(L, L) for L in rows]
    n_vec = n_steps + 1 if per_step else 1
    eng.seed(321)
    drawn = [np.stack([eng.rng_normal(100 * eng.frames(L)) for _ in range(n_vec)]) for L in rows]  # candidate after candidate
    u_want = eng.rng_uniform()
    with options(eng, diff_temperature=0.7, **opts):
        explicit = eng.diffusion(lats, n_steps=n_steps, noise=drawn)
        eng.seed(321)
        got = eng.diffusion(lats, n_steps=n_steps, noise_mode=pkg.NOISE_REFERENCE)
        u_got = eng.rng_uniform()
    with options(eng, **opts):
        plain = eng.diffusion(lats, n_steps=n_steps, noise=drawn)
    for a, b, p in zip(explicit, got, plain):
        assert np.array_equal(a, b), float(np.abs(a - b).max())
        assert np.abs(a - p).max() > 1e-3
    assert u_got == u_want, (u_got, u_want)  # consumption unchanged


def test_temperature_device_noise(eng, pkg):
    rows = [43, 12]
    lats = [_latents(L, L) for L in rows]
    zeros = [np.zeros((1, 100 * eng.frames(L)), np.float32) for L in rows]
    with options(eng, diff_sampler=1, ddim_eta=0):
        want0 = eng.diffusion(lats, n_steps=N_PROP, noise=zeros)
        eng.seed(5)
        t1 = eng.diffusion(lats, n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
        with options(eng, diff_temperature=0):
            eng.seed(5)
            t0 = eng.diffusion(lats, n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
        with options(eng, diff_temperature=0.5):
            eng.seed(5)
            th = eng.diffusion(lats, n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
    for c in range(len(rows)):
        assert np.array_equal(t0[c], want0[c]), (c, float(np.abs(t0[c] - want0[c]).max()))
        assert np.abs(th[c] - t1[c]).max() > 1e-3 and np.abs(th[c] - t0[c]).max() > 1e-3, c


# ---- 6. nothing existing moved ------------------------------------------------------------------------------------------------------------------------------

def test_ddpm_bits_after_unguided_equal_a_fresh_context(eng, pkg, small_models):
    n_steps, lat = 80, _latents(12, 3)
    T = eng.frames(12)
    noise = np.random.RandomState(4).randn(n_steps + 1, 100 * T).astype(np.float32)
    with options(eng, cond_free=0, diff_temperature=0.5):
        eng.diffusion([lat], n_steps=20, noise=[noise[:21]])
    after = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    fresh = pkg.Engine(0)
    try:
        fresh.load(diffusion=small_models + "/ggml-diffusion-model.bin")
        want = fresh.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    finally:
        fresh.close()
    assert np.array_equal(after, want)


# ---- 7. end to end through the CLI ----------------------------------------------------------------------------------------------------------------------------

def test_cli_cond_free_0(eng, pkg, small_models, voice, tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    msg = "this is a test message."
    wavs = {}
    for flag in ("0", "1"):
        out = tmp_path / ("cond_free_%s.wav" % flag)
        r = subprocess.run([exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--seed", "3", "--codes", "40",
                            "--sampler", "ddim", "--steps", "20", "--cond-free", flag, "--timing", "1", "--output", str(out)], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "[timing] cond-free %s, diffusion-temperature 1\n" % flag in r.stderr
        assert "[timing] sampler ddim, ddim-eta 0, cond-free-k 2, steps 20\n" in r.stderr
        raw = out.read_bytes()
        assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
        wavs[flag] = np.frombuffer(raw[44:], np.float32)
    # the same pipeline through the Python wrapper: the CLI's seed and RNG order (one candidate: reference-order noise from the context's generator)
    eng.tokenizer_load(str(d / "tokenizer.json"))
    eng.seed(3)
    codes, rows, lats, _ = eng.autoregressive(eng.tokenize(msg), voice, 1, 40, mask_stop=True)
    with options(eng, diff_sampler=1, cond_free=0):
        mels = eng.diffusion(lats, n_steps=20)
    audio = eng.vocoder(mels)[0]
    assert len(wavs["0"]) == len(audio) == len(wavs["1"])
    assert np.array_equal(wavs["0"], audio)
    assert np.abs(wavs["0"] - wavs["1"]).max() > 1e-4
