"""GPU: the DPM-Solver++(2M) sampler of the diffusion stage (option "diff_sampler" = 3; diffusion.hip: step_update_kernel, dpmpp_step_value).

The reference and the oracle have no such sampler. The yardstick is tests/test_ddim_gpu.py's: a host-driven loop over the engine's own network, per step two
tts_diffusion_forward calls (conditioned and conditioning-free) at the step's timestep, then the numpy float32 restatement of the update (tests/test_dpmpp_cpu.py:
dpmpp_update, pinned there on a hand-checkable case) with the scalars of the host probes. The DDIM loop runs alongside as the yardstick's self-check. Gate for both:
conftest.loop_gate("small"), the distance the project accepts between two correct f32 evaluations of this loop.

Measured on an MI355X (profiles/dpmpp_sampler.txt): both distances are 0.0 at 5 and at 12 steps — the device loop and the host-driven loop agree bit for bit.

Everything else is a bit-identity property the other two samplers already have (np.array_equal). Shapes: L = 43 (T = 187) beside L = 12 (T = 52): two tiles and
one, ragged; 6 steps = first order, three second-order steps, first order twice."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import loop_gate
from test_ddim_gpu import _latents, host_loop, options
from test_diff_session_gpu import admit, alone, req, run_session
from test_dpmpp_cpu import dpmpp_update

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N_PROP = 6
RAGGED = [43, 12, 43]


@pytest.fixture(scope="module")
def eng(pkg, small_models):
    e = pkg.Engine(0)
    e.load(small_models)
    yield e
    e.close()


def dpmpp_host_loop(eng, pkg, lat, n, x_T):
    """The sampling loop run from the host. x_T [100*T]."""
    tm, s = pkg.host_schedule(n)
    d = pkg.host_schedule_ddim(n, 0.0)
    p = pkg.host_schedule_dpmpp(n)
    T = eng.frames(len(lat))
    x = np.ascontiguousarray(x_T, f32).reshape(100, T).copy()
    hist = None
    for idx in range(n):
        t = n - 1 - idx
        out_c = eng.diffusion_forward(lat, x, int(tm[t]), False)
        out_u = eng.diffusion_forward(lat, x, int(tm[t]), True)
        x, hist = dpmpp_update(x, out_c[:100], out_u[:100], s["cfk"][t], s["sqrt_recip"][t], s["sqrt_recipm1"][t], d["c_x0"][t], d["c_eps"][t],
                               p["a"][t], p["b"][t], p["c"][t], int(p["order"][t]), t == 0, hist)
        x = np.ascontiguousarray(x, f32)
    return x


def _ragged(eng):
    lats = [_latents(L, 10 + i) for i, L in enumerate(RAGGED)]
    rs = np.random.RandomState(77)
    x_T = [rs.randn(100 * eng.frames(L)).astype(np.float32) for L in RAGGED]
    return lats, x_T


# ---- the update rule, through the loop --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_steps", [5, 12])
def test_host_driven_loop(eng, pkg, n_steps):
    """5 steps: the smallest count at which a second-order step reads a history that a second-order step wrote."""
    lat = _latents(43, 43)
    T = eng.frames(43)
    x_T = np.random.RandomState(n_steps).randn(100 * T).astype(np.float32)
    gate = loop_gate("small")
    with options(eng, diff_sampler=3):
        got = eng.diffusion([lat], n_steps=n_steps, noise=[x_T])[0]
    want = dpmpp_host_loop(eng, pkg, lat, n_steps, x_T)
    d_dpm = float(np.abs(got - want).max())
    with options(eng, diff_sampler=1, ddim_eta=0):
        got_i = eng.diffusion([lat], n_steps=n_steps, noise=[x_T])[0]
    want_i = host_loop(eng, pkg, lat, n_steps, "ddim", x_T)
    d_ddim = float(np.abs(got_i - want_i).max())
    print("host-driven loop, %d steps, L = 43 (T = %d): DPM-Solver++(2M) max abs %.3e, DDIM eta 0 (self-check) max abs %.3e, gate %.3e; 2M vs DDIM max abs %.3e"
          % (n_steps, T, d_dpm, d_ddim, gate, float(np.abs(got - got_i).max())))
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0  # the last step returns the clipped x0
    if n_steps == 12:
        assert np.abs(got - got_i).max() > 1e-3  # two samplers
    assert d_ddim <= gate, (d_ddim, gate)
    assert d_dpm <= gate, (d_dpm, gate)


# ---- bit-identity properties --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_steps", [2, 3])
def test_two_and_three_steps_are_ddim(eng, n_steps):
    """no second-order step exists: every step is the DDIM eta-0 step, bit for bit"""
    lats, x_T = _ragged(eng)
    with options(eng, diff_sampler=3):
        got = eng.diffusion(lats[:2], n_steps=n_steps, noise=x_T[:2])
    with options(eng, diff_sampler=1, ddim_eta=0):
        want = eng.diffusion(lats[:2], n_steps=n_steps, noise=x_T[:2])
    for c in range(2):
        assert np.array_equal(got[c], want[c]), (c, float(np.abs(got[c] - want[c]).max()))


def test_ragged_batch_equals_each_candidate_alone(eng):
    lats = [_latents(43, 10), _latents(12, 11)]
    rs = np.random.RandomState(77)
    x_T = [rs.randn(100 * eng.frames(L)).astype(np.float32) for L in (43, 12)]
    with options(eng, diff_sampler=3):
        batch = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
        for c in range(2):
            alone_c = eng.diffusion([lats[c]], n_steps=N_PROP, noise=[x_T[c]])[0]
            assert np.array_equal(batch[c], alone_c), (c, float(np.abs(batch[c] - alone_c).max()))
        again = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)  # two consecutive calls: the history of the first does not reach the second
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))
    with options(eng, diff_sampler=1):
        ddim = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
    assert np.abs(batch[0] - ddim[0]).max() > 1e-3  # the second-order steps are live


@pytest.mark.parametrize("opt", ["diff_graph", "hoist_integrator", "share_uncond"])
def test_option_changes_no_bit(eng, opt):
    lats, x_T = _ragged(eng)
    with options(eng, diff_sampler=3):
        with options(eng, **{opt: 1}):
            on = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
        with options(eng, **{opt: 0}):
            off = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
    for c in range(len(lats)):
        assert np.array_equal(on[c], off[c]), (opt, c, float(np.abs(on[c] - off[c]).max()))


def test_ddim_eta_is_not_read(eng, pkg):
    """eta = 0.5: no bit changes, and TTS_NOISE_REFERENCE still draws exactly 100 T_c normals per candidate, candidate after candidate, and nothing else"""
    lats, x_T = _ragged(eng)
    sizes = [len(x) for x in x_T]
    with options(eng, diff_sampler=3):
        want = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
    for rows in (slice(0, 3), slice(0, 1)):  # one candidate: the pipelined-draw path
        eng.seed(321)
        drawn_T = [eng.rng_normal(n) for n in sizes[rows]]
        u_want = eng.rng_uniform()
        with options(eng, diff_sampler=3, ddim_eta=0.5):
            explicit = eng.diffusion(lats[rows], n_steps=N_PROP, noise=drawn_T)
            eng.seed(321)
            drawn = eng.diffusion(lats[rows], n_steps=N_PROP, noise_mode=pkg.NOISE_REFERENCE)
            u_got = eng.rng_uniform()
            half = eng.diffusion(lats[rows], n_steps=N_PROP, noise=x_T[rows])
        for a, b in zip(explicit, drawn):
            assert np.array_equal(a, b), float(np.abs(a - b).max())
        assert u_got == u_want, (u_got, u_want)
        for a, b in zip(half, want[rows]):
            assert np.array_equal(a, b), float(np.abs(a - b).max())


def test_multi_voice_equals_each_candidate_alone_with_its_voice(eng, small_models):
    from test_multi_voice_gpu import diff_voices
    vlat, own = diff_voices(small_models, 2)
    lats, x_T = _ragged(eng)
    vmap = [1, 0, 1]
    with options(eng, diff_sampler=3):
        multi = eng.diffusion(lats, n_steps=N_PROP, noise=x_T, voice_latents=vlat, voice_of_candidate=vmap)
        plain = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
        try:
            for c in range(len(lats)):
                eng.set_diffusion_conditioning_latent(vlat[vmap[c]])
                alone_c = eng.diffusion([lats[c]], n_steps=N_PROP, noise=[x_T[c]])[0]
                assert np.array_equal(multi[c], alone_c), (c, float(np.abs(multi[c] - alone_c).max()))
                assert np.abs(multi[c] - plain[c]).max() > 1e-3, c
        finally:
            eng.set_diffusion_conditioning_latent(own)


def test_latency_mode_batch_of_two_equals_the_same_mode_alone(eng):
    lats, x_T = _ragged(eng)
    lats, x_T = lats[:2], x_T[:2]
    with options(eng, diff_sampler=3, latency_mode=1):
        pair = eng.diffusion(lats, n_steps=N_PROP, noise=x_T)
        for c in range(2):
            alone_c = eng.diffusion([lats[c]], n_steps=N_PROP, noise=[x_T[c]])[0]
            assert np.array_equal(pair[c], alone_c), (c, float(np.abs(pair[c] - alone_c).max()))


def test_device_noise_shards_reproduce_one_batch(eng, pkg):
    lats = [_latents(L, 30 + i) for i, L in enumerate([43, 12, 43, 20])]
    eng.seed(99)
    with options(eng, diff_sampler=3):
        whole = eng.diffusion(lats, n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
        parts = []
        for r in range(2):
            with options(eng, rng_shard_offset=2 * r, rng_shard_total=4):
                parts += eng.diffusion(lats[2 * r:2 * r + 2], n_steps=N_PROP, noise_mode=pkg.NOISE_DEVICE)
    for c in range(4):
        assert np.array_equal(whole[c], parts[c]), (c, float(np.abs(whole[c] - parts[c]).max()))
    assert np.abs(whole[0] - whole[2]).max() > 1e-3  # same length: the candidates' streams differ
    with options(eng, diff_sampler=1):  # the x_T stream of the other samplers: n = 2 is DDIM from the same x_T
        eng.seed(99)
        ddim2 = eng.diffusion(lats[:1], n_steps=2, noise_mode=pkg.NOISE_DEVICE)[0]
    with options(eng, diff_sampler=3):
        eng.seed(99)
        assert np.array_equal(eng.diffusion(lats[:1], n_steps=2, noise_mode=pkg.NOISE_DEVICE)[0], ddim2)


def test_other_samplers_after_it_equal_a_fresh_context(eng, pkg, small_models):
    """no history and no table leaks: a DDPM call, then a DDIM call, after a sampler-3 call"""
    n_steps, lat = 8, _latents(12, 3)
    T = eng.frames(12)
    noise = np.random.RandomState(4).randn(n_steps + 1, 100 * T).astype(np.float32)
    with options(eng, diff_sampler=3, cond_free_k=1.0):
        eng.diffusion([lat], n_steps=n_steps, noise=[noise[0]])
    ddpm = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    with options(eng, diff_sampler=1, ddim_eta=0.5):
        ddim = eng.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    fresh = pkg.Engine(0)
    try:
        fresh.load(diffusion=small_models + "/ggml-diffusion-model.bin")
        want_ddpm = fresh.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
        fresh.set_option("diff_sampler", 1)
        fresh.set_option("ddim_eta", 0.5)
        want_ddim = fresh.diffusion([lat], n_steps=n_steps, noise=[noise])[0]
    finally:
        fresh.close()
    assert np.array_equal(ddpm, want_ddpm) and np.array_equal(ddim, want_ddim)


# ---- sessions -----------------------------------------------------------------------------------------------------------------------------------------------

def dpm_req(pkg, rows, n_steps, noise="explicit", **kw):
    """tests/test_diff_session_gpu.py's request with sampler 3: explicit noise is x_T alone"""
    r = req(pkg, rows, n_steps, sampler=3, noise=noise, **kw)
    if r["noise"] is not None:
        r["noise"] = [z[:1] for z in r["noise"]]
    return r


def _assert_alone(eng, pkg, reqs, out, which):
    for i in which:
        ref = alone(eng, pkg, reqs[i])
        assert len(out[i]) == len(ref)
        for c in range(len(ref)):
            assert np.array_equal(out[i][c], ref[c]), ("request", i, "candidate", c, float(np.abs(out[i][c] - ref[c]).max()))
        assert np.isfinite(ref[0]).all()


def test_session_beside_ddpm_and_ddim(eng, pkg):
    """P (7 steps) runs its steps 0 (first order) and 1 (second order: writes d_prev) before Q is admitted: the layout is rebuilt between that write and step 2's
    read. Q starts with its own first-order step while P is in its second-order steps; B joins at 1 and A, B, Q, P leave at 6, 5, 7, 7."""
    reqs = [req(pkg, [17], 6, tag=1),                                        # A: ancestral
            req(pkg, [25], 4, sampler=1, eta=0.0, k=1.0, at=1, tag=2),       # B: DDIM
            dpm_req(pkg, [43], 7, tag=3),                                    # P
            dpm_req(pkg, [12, 30], 5, noise=None, seed=7, at=2, tag=4)]      # Q: two candidates of other lengths, device noise, 5 steps
    out, captures, changed = run_session(eng, reqs, 4096)
    _assert_alone(eng, pkg, reqs, out, range(4))
    assert changed == 5 and captures == changed, (captures, changed)  # {A, P}, + B, + Q, - B, - A
    with options(eng, diff_sampler=1):
        ddim = eng.diffusion(reqs[2]["latents"], n_steps=7, noise=reqs[2]["noise"])[0]
    assert np.abs(out[2][0] - ddim).max() > 1e-3  # P's second-order steps are live


def test_session_cancel_mid_run(eng, pkg):
    keep, drop, other = dpm_req(pkg, [21], 6, tag=1), dpm_req(pkg, [33], 7, tag=2), req(pkg, [9], 5, tag=3)
    eng.diff_session_open(4096, 4)
    try:
        k, d, o = admit(eng, keep), admit(eng, drop), admit(eng, other)
        for _ in range(3):  # `drop` has run a first-order and two second-order steps
            assert eng.diff_session_step() == 3
        eng.diff_session_cancel(d)
        while eng.diff_session_step():
            pass
        assert sorted(eng.diff_session_finished()) == sorted([k, o])
        got = {0: eng.diff_session_collect(k), 2: eng.diff_session_collect(o)}
    finally:
        eng.diff_session_close()
    _assert_alone(eng, pkg, [keep, drop, other], got, (0, 2))


def test_session_request_init_takes_the_pinned_sampler(eng, pkg):
    r = dpm_req(pkg, [14], 4, tag=5)
    with options(eng, diff_sampler=3):
        eng.diff_session_open(1024, 2)
    try:
        rid = eng.diff_session_admit(r["latents"], n_steps=4, noise=r["noise"])  # sampler left to tts_diff_request_init
        while eng.diff_session_step():
            pass
        got = eng.diff_session_collect(rid)
    finally:
        eng.diff_session_close()
    assert np.array_equal(got[0], alone(eng, pkg, r)[0])


# ---- end to end through the CLI -----------------------------------------------------------------------------------------------------------------------------

def test_cli_sampler_dpmpp2m(eng, pkg, small_models, voice, tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    d = tmp_path / "models"
    d.mkdir()
    for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
        os.symlink(os.path.join(small_models, f), d / f)
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    msg = "this is a test message."
    out = tmp_path / "dpmpp2m.wav"
    r = subprocess.run([exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--seed", "3", "--codes", "40",
                        "--sampler", "dpmpp2m", "--steps", "12", "--timing", "1", "--output", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[timing] sampler dpmpp2m, ddim-eta 0, cond-free-k 2, steps 12\n" in r.stderr
    raw = out.read_bytes()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
    wav = np.frombuffer(raw[44:], np.float32)
    # the same pipeline through the Python wrapper: the CLI's seed and RNG order (one candidate: reference-order noise from the context's generator)
    eng.tokenizer_load(str(d / "tokenizer.json"))
    eng.seed(3)
    codes, rows, lats, _ = eng.autoregressive(eng.tokenize(msg), voice, 1, 40, mask_stop=True)
    with options(eng, diff_sampler=3):
        mels = eng.diffusion(lats, n_steps=12)
    audio = eng.vocoder(mels)[0]
    assert len(wav) == len(audio) and np.array_equal(wav, audio)
