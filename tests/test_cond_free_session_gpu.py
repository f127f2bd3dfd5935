"""GPU: guided and unguided requests side by side in one diffusion session (tts_diff_request.cond_free / .temperature; diffusion.hip: diff_session_admit,
diff_session_rebuild). A guided request brings its conditioned sequences and their unconditioned copies, an unguided one its conditioned sequences only; the
contract is the session's: every collected mel is bit for bit the mel of that request run ALONE through the single calls under its controls (np.array_equal, no
tolerance). Every scenario runs in a session opened with "hoist_integrator" 1 and again with 0.

Shapes: rows [2, 9] (T = 8 and 39: the guard-row cases of the packed layout), [43] (T = 187: 512 packed rows guided, 256 unguided),
[210] (T = 914: the second GroupNorm kernel class) beside [12]; 3 - 8 steps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULTS = {"diff_sampler": 0, "ddim_eta": 0, "cond_free_k": 2.0, "cond_free": 1, "diff_temperature": 1.0, "hoist_integrator": 1}


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


@pytest.fixture(scope="module")
def eng(pkg, small_models):
    e = pkg.Engine(0)
    e.load(small_models)
    yield e
    e.close()


def _latents(L, seed):
    return np.random.RandomState(seed).randn(L, 1024).astype(np.float32)


def _voice(seed):
    return (0.3 * np.random.RandomState(seed).randn(2048)).astype(np.float32)


def req(pkg, rows, n_steps, sampler=0, eta=0.0, cond_free=1, temperature=1.0, voice=None, noise="explicit", seed=0, at=0, tag=0):
    """One request: latents RandomState(100 * tag + row count + index) per candidate; noise "explicit" = tts_diffusion's layout from a RandomState, None = the device
    generator under `seed`. at: session steps that have run when it is admitted."""
    lats = [_latents(L, 100 * tag + L + c) for c, L in enumerate(rows)]
    n_vec = 1 if sampler == 3 or (sampler == 1 and eta == 0) else n_steps + 1
    nz = None
    if noise == "explicit":
        rs = np.random.RandomState(1000 + 7 * tag + n_steps)
        nz = [rs.randn(n_vec, 100 * pkg.Engine.frames(L)).astype(np.float32) for L in rows]
    return dict(rows=rows, latents=lats, n_steps=n_steps, sampler=sampler, eta=eta, cond_free=cond_free, temperature=temperature, voice=voice, noise=nz, seed=seed,
                at=at)


def packed(pkg, r):
    return pkg.host_diff_packed_rows(r["rows"], cond_free=bool(r["cond_free"]))


def alone(eng, pkg, r):
    """The request through the single calls, under its controls."""
    with options(eng, diff_sampler=r["sampler"], ddim_eta=r["eta"], cond_free=r["cond_free"], diff_temperature=r["temperature"]):
        kw = {}
        if r["voice"] is not None:
            kw = dict(voice_latents=r["voice"].reshape(1, 2048), voice_of_candidate=[0] * len(r["latents"]))
        if r["noise"] is None:
            eng.seed(r["seed"])
            out = eng.diffusion(r["latents"], n_steps=r["n_steps"], noise=None, noise_mode=pkg.NOISE_DEVICE, **kw)
        else:
            out = eng.diffusion(r["latents"], n_steps=r["n_steps"], noise=r["noise"], **kw)
        assert eng.diffusion_last_layout() == (packed(pkg, r), (2 if r["cond_free"] else 1) * len(r["rows"]))
    return out


def admit(eng, r):
    return eng.diff_session_admit(r["latents"], n_steps=r["n_steps"], sampler=r["sampler"], ddim_eta=r["eta"], voice_latent=r["voice"], noise=r["noise"],
                                  seed=r["seed"], cond_free=r["cond_free"], temperature=r["temperature"])


def run_session(eng, pkg, reqs, max_rows, max_requests=8):
    """Admits reqs[i] once `at` steps have run and collects every request on the step it finishes; the room is checked against the probe at every change."""
    eng.diff_session_open(max_rows, max_requests)
    try:
        out, rid_of, left_of = {}, {}, {}
        pending = sorted(range(len(reqs)), key=lambda i: reqs[i]["at"])
        step, used = 0, 0
        while pending or rid_of:
            assert step < 100
            while pending and reqs[pending[0]]["at"] <= step:
                i = pending.pop(0)
                rid_of[i] = admit(eng, reqs[i])
                left_of[i] = reqs[i]["n_steps"]
                used += packed(pkg, reqs[i])
                assert eng.diff_session_room() == max_rows - used, (i, eng.diff_session_room(), max_rows, used)
            left = eng.diff_session_step()
            step += 1
            for i in list(rid_of):
                left_of[i] -= 1
            done = sorted(i for i in rid_of if left_of[i] == 0)
            assert left == len(rid_of) - len(done)
            for i in done:
                used -= packed(pkg, reqs[i])  # a finished request holds no rows
            assert eng.diff_session_room() == max_rows - used
            for i in done:
                out[i] = eng.diff_session_collect(rid_of.pop(i))
        assert eng.diff_session_room() == max_rows and eng.diff_session_step() == 0
    finally:
        eng.diff_session_close()
    return out


def assert_each_alone(eng, pkg, reqs, out, what=""):
    for i, r in enumerate(reqs):
        ref = alone(eng, pkg, r)
        assert len(out[i]) == len(ref)
        for c in range(len(ref)):
            assert out[i][c].shape == ref[c].shape and np.array_equal(out[i][c], ref[c]), (what, "request", i, "candidate", c,
                                                                                          float(np.abs(out[i][c] - ref[c]).max()))
        assert np.isfinite(ref[0]).all()


HOIST = pytest.mark.parametrize("hoist", [1, 0])


@HOIST
def test_staggered_mix_of_guided_and_unguided(eng, pkg, hoist):
    reqs = [req(pkg, [2, 9], 6, sampler=1, cond_free=0, tag=1),                                                          # unguided DDIM from explicit x_T
            req(pkg, [43], 8, at=2, tag=2),                                                                             # guided ancestral, explicit noise
            req(pkg, [43], 6, sampler=3, cond_free=0, temperature=0.7, voice=_voice(5), noise=None, seed=7, at=3, tag=3)]  # unguided DPM-Solver++, cooler, own voice
    max_rows = sum(packed(pkg, r) for r in reqs)  # the three fill the session exactly
    assert [packed(pkg, r) for r in reqs] == [128, 512, 256]
    with options(eng, hoist_integrator=hoist):
        out = run_session(eng, pkg, reqs, max_rows)
        assert_each_alone(eng, pkg, reqs, out, "hoist %d" % hoist)
    # the controls are live: the third request differs from its guided and from its temperature-1 form
    for change in (dict(cond_free=1), dict(temperature=1.0)):
        other = alone(eng, pkg, dict(reqs[2], **change))[0]
        assert np.abs(other - out[2][0]).max() > 1e-3, change


@HOIST
def test_room_counts_by_the_flag(eng, pkg, hoist):
    e = eng
    keep = req(pkg, [21], 5, sampler=1, cond_free=0, tag=1)
    drop = req(pkg, [33], 6, tag=2)
    need = [packed(pkg, keep), packed(pkg, drop)]
    assert need == [pkg.host_diff_packed_rows([21], cond_free=False), pkg.host_diff_packed_rows([33])]
    with options(e, hoist_integrator=hoist):
        e.diff_session_open(sum(need), 4)
        try:
            assert e.diff_session_room() == sum(need)
            k = admit(e, keep)
            assert e.diff_session_room() == need[1]
            d = admit(e, drop)
            assert e.diff_session_room() == 0
            assert e.diff_session_step() == 2
            e.diff_session_cancel(d)  # mid-flight: its rows are free again
            assert e.diff_session_room() == need[1]
            while e.diff_session_step():
                pass
            assert e.diff_session_room() == sum(need)  # finished: holds none
            got_keep = e.diff_session_collect(k)
        finally:
            e.diff_session_close()
        assert np.array_equal(got_keep[0], alone(e, pkg, keep)[0])
        # a session of exactly the unguided count: the guided form of the same request is refused before any device work, and nothing changes
        r0 = req(pkg, [43], 4, sampler=1, cond_free=0, tag=3)
        rows0 = pkg.host_diff_packed_rows([43], cond_free=False)
        e.diff_session_open(rows0, 2)
        try:
            with pytest.raises(pkg.TtsError, match=r"status -6"):
                admit(e, dict(r0, cond_free=1))
            assert e.diff_session_room() == rows0 and e.diff_session_step() == 0
            rid = admit(e, r0)
            assert e.diff_session_room() == 0
            with pytest.raises(pkg.TtsError, match=r"status -6"):
                admit(e, dict(r0, cond_free=1))
            while e.diff_session_step():
                pass
            got = e.diff_session_collect(rid)
        finally:
            e.diff_session_close()
        assert np.array_equal(got[0], alone(e, pkg, r0)[0])


@HOIST
def test_two_groupnorm_classes(eng, pkg, hoist):
    """T = 914 > 896: alone on the second GroupNorm kernel, unguided; T = 52 beside it, guided: alone on the first"""
    reqs = [req(pkg, [210], 3, cond_free=0, tag=9), req(pkg, [12], 3, at=1, tag=10)]
    with options(eng, hoist_integrator=hoist):
        out = run_session(eng, pkg, reqs, 4096)
        assert_each_alone(eng, pkg, reqs, out, "hoist %d" % hoist)


@HOIST
def test_a_72_byte_descriptor_runs_under_the_pinned_values(eng, pkg, hoist):
    """An older caller's descriptor ends before temperature and cond_free: admitted into a session opened under cond_free 0 (and temperature 0.7) it runs
    unguided at that temperature; what lies behind its 72 bytes is not read."""
    e, L = eng, eng.L
    r = req(pkg, [43], 4, sampler=1, cond_free=0, temperature=0.7, tag=4)
    lat = np.ascontiguousarray(r["latents"][0])
    rows = np.array([43], np.int32)
    nz = np.ascontiguousarray(r["noise"][0].reshape(-1))
    T = e.frames(43)
    vp = C.c_void_p
    with options(e, hoist_integrator=hoist):
        with options(e, cond_free=0, diff_temperature=0.7):
            e.diff_session_open(pkg.host_diff_packed_rows([43], cond_free=False), 1)
        try:  # the options are back at their defaults: the session pinned them
            d = pkg.DiffRequest()
            d.struct_size = 72
            d.temperature, d.cond_free = float("nan"), 1  # behind the caller's struct: must stay unread
            assert L.tts_diff_request_init(e.h, C.byref(d)) == 0
            assert d.cond_free == 1 and d.temperature != d.temperature  # ... and unwritten
            d.n_cand, d.latents, d.rows, d.n_steps, d.sampler = 1, lat.ctypes.data_as(vp), rows.ctypes.data_as(vp), r["n_steps"], 1
            d.noise = nz.ctypes.data_as(vp)
            rid = L.tts_diff_session_admit(e.h, C.byref(d))
            assert rid >= 0, e.last_error() if hasattr(e, "last_error") else rid
            assert e.diff_session_room() == 0
            while e.diff_session_step():
                pass
            mel = np.empty(100 * T, np.float32)
            assert L.tts_diff_session_collect(e.h, rid, mel.ctypes.data_as(vp)) == 0
            # a full-size descriptor's defaults are the pinned values
            full = pkg.DiffRequest()
            full.struct_size = C.sizeof(pkg.DiffRequest)
            assert L.tts_diff_request_init(e.h, C.byref(full)) == 0
            assert (full.cond_free, full.temperature) == (0, 0.7)
        finally:
            e.diff_session_close()
        want = alone(e, pkg, r)[0]
        assert np.array_equal(mel.reshape(100, T), want), float(np.abs(mel.reshape(100, T) - want).max())
        guided = alone(e, pkg, dict(r, cond_free=1))[0]
        assert np.abs(guided - want).max() > 1e-3
