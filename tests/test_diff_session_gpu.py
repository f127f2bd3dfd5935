"""GPU: in-flight batching of the diffusion stage (tts_diff_session_*). Requests join a running layout at any step and leave at any step, each with its own step
count, sampler, eta, guidance strength, voice latent and noise; the contract is that of every batching feature here: a request's mel is bit for bit the mel of that
request run ALONE through the single calls (tts_set_option of its sampler / eta / k, its voice, then tts_diffusion with its noise, or tts_seed + device noise).
Nothing below has a tolerance: every comparison is np.array_equal against the single-call path, which this feature does not change.

Shapes are the smallest at which a path can go wrong: 2 - 6 steps; frame counts T with T % 8 == 0 and T % 8 == 7 (the guard-row cases of the packed layout), T = 4
(one latent row), a joint layout that crosses 128 rows only with its second request, equal lengths (the alone call shares its unconditioned integrator, the joint
layout holds every copy), and T = 914 beside T = 87: two GroupNorm kernel classes in one layout (the single call picks the kernel by the layout's longest
sequence; the session normalises class by class)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_LIMIT = -1, -5, -6
DEFAULTS = {"diff_sampler": 0, "ddim_eta": 0, "cond_free_k": 2.0, "share_uncond": 1, "hoist_integrator": 1, "diff_graph": 1, "latency_mode": 0, "attn_f32": 0}


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
def eng_mid(pkg, mid_models):
    e = pkg.Engine(0)
    e.load(diffusion=mid_models + "/ggml-diffusion-model.bin")
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_small(pkg, small_models):
    e = pkg.Engine(0)
    e.load(small_models)
    yield e
    e.close()


def _latents(L, seed):
    return np.random.RandomState(seed).randn(L, 1024).astype(np.float32)


def _voice(seed):
    return (0.3 * np.random.RandomState(seed).randn(2048)).astype(np.float32)


def req(pkg, rows, n_steps, sampler=0, eta=0.0, k=2.0, voice=None, noise="explicit", seed=0, at=0, tag=0):
    """One request: latents RandomState(100 * tag + row count).randn(L, 1024) per candidate; noise "explicit" = tts_diffusion's layout from a RandomState, None = the
    device generator under `seed`. at: session steps that have run when it is admitted."""
    lats = [_latents(L, 100 * tag + L + c) for c, L in enumerate(rows)]
    n_vec = 1 if sampler == 1 and eta == 0 else n_steps + 1
    nz = None
    if noise == "explicit":
        rs = np.random.RandomState(1000 + 7 * tag + n_steps)
        nz = [rs.randn(n_vec, 100 * pkg.Engine.frames(L)).astype(np.float32) for L in rows]
    return dict(latents=lats, n_steps=n_steps, sampler=sampler, eta=eta, k=k, voice=voice, noise=nz, seed=seed, at=at)


def alone(eng, pkg, r):
    """The request through the single calls."""
    with options(eng, diff_sampler=r["sampler"], ddim_eta=r["eta"], cond_free_k=r["k"]):
        kw = {}
        if r["voice"] is not None:
            kw = dict(voice_latents=r["voice"].reshape(1, 2048), voice_of_candidate=[0] * len(r["latents"]))
        if r["noise"] is None:
            eng.seed(r["seed"])
            return eng.diffusion(r["latents"], n_steps=r["n_steps"], noise=None, noise_mode=pkg.NOISE_DEVICE, **kw)
        return eng.diffusion(r["latents"], n_steps=r["n_steps"], noise=r["noise"], **kw)


def admit(eng, r):
    return eng.diff_session_admit(r["latents"], n_steps=r["n_steps"], sampler=r["sampler"], ddim_eta=r["eta"], cond_free_k=r["k"], voice_latent=r["voice"],
                                  noise=r["noise"], seed=r["seed"])


def run_session(eng, reqs, max_rows, max_requests=8, close=True, on_step=None):
    """Admits reqs[i] once `at` steps have run, collects every request on the step it finishes. Returns
    ({i: list of mel}, captures, number of steps whose membership differed from the previous step's)."""
    eng.diff_session_open(max_rows, max_requests)
    out, rid_of, left_of = {}, {}, {}
    pending = sorted(range(len(reqs)), key=lambda i: reqs[i]["at"])
    step, changed, prev = 0, 0, frozenset()
    while pending or rid_of:
        assert step < 100
        while pending and reqs[pending[0]]["at"] <= step:
            i = pending.pop(0)
            rid_of[i] = admit(eng, reqs[i])
            left_of[i] = reqs[i]["n_steps"]
        members = frozenset(rid_of)
        changed += members != prev
        left = eng.diff_session_step()
        step += 1
        for i in list(rid_of):
            left_of[i] -= 1
        done = sorted(i for i in rid_of if left_of[i] == 0)
        assert left == len(rid_of) - len(done)
        assert sorted(eng.diff_session_finished()) == sorted(rid_of[i] for i in done)
        for i in done:
            out[i] = eng.diff_session_collect(rid_of.pop(i))
        prev = members
        if on_step:
            on_step(step, rid_of)
    captures = eng.diff_session_captures()
    assert eng.diff_session_room() == max_rows and eng.diff_session_finished() == [] and eng.diff_session_step() == 0
    if close:
        eng.diff_session_close()
    return out, captures, changed


def assert_each_alone(eng, pkg, reqs, out, what=""):
    for i, r in enumerate(reqs):
        ref = alone(eng, pkg, r)
        assert len(out[i]) == len(ref)
        for c in range(len(ref)):
            assert out[i][c].shape == ref[c].shape and np.array_equal(out[i][c], ref[c]), (what, "request", i, "candidate", c,
                                                                                          float(np.abs(out[i][c] - ref[c]).max()))
        assert np.isfinite(ref[0]).all()


# ---- 1. / 2. staggered arrivals, mixed controls; the option matrix --------------------------------------------------------------------------------------

def staggered(pkg):
    a = req(pkg, [43, 17], 6, tag=1)                                                    # ancestral, explicit noise, two candidates
    b = req(pkg, [61], 4, sampler=1, eta=0.0, k=1.0, voice=_voice(5), at=2, tag=2)      # deterministic DDIM from an explicit x_T, k = 1, a second voice
    c = req(pkg, [30], 5, noise=None, seed=7, at=6, tag=3)                              # device generator; admitted on the step at which A and B finish
    d = req(pkg, [25], 3, sampler=1, eta=0.5, at=6, tag=4)                              # stochastic DDIM; admitted after A was collected, into its rows
    return [a, b, c, d]


def staggered_rows(pkg):
    # A and B fill the session exactly: C and D fit only into the rows A and B leave
    return pkg.host_diff_packed_rows([43, 17]) + pkg.host_diff_packed_rows([61])


def test_staggered_arrivals_mixed_controls(eng_mid, pkg):
    reqs = staggered(pkg)
    seen = {}

    def on_step(step, rid_of):
        seen[step] = eng_mid.diff_session_room()

    out, captures, changed = run_session(eng_mid, reqs, staggered_rows(pkg), on_step=on_step)
    assert seen[3] == 0  # A and B running: full
    assert_each_alone(eng_mid, pkg, reqs, out)
    # A alone (steps 1-2), A + B (3-6), C + D (7-9), C (10-11)
    assert changed == 4 and captures == changed, (captures, changed)
    assert np.abs(out[0][0] - out[1][0][:, :out[0][0].shape[1]]).max() > 1e-3  # different requests give different mels


@pytest.mark.parametrize("opt", ["attn_f32", "share_uncond", "hoist_integrator", "diff_graph"])
def test_option_matrix(eng_mid, pkg, opt):
    reqs = staggered(pkg)
    value = 1 if opt == "attn_f32" else 0
    with options(eng_mid, **{opt: value}):
        out, captures, changed = run_session(eng_mid, reqs, staggered_rows(pkg))
        assert_each_alone(eng_mid, pkg, reqs, out, opt)
    assert captures == (0 if opt == "diff_graph" else changed), (opt, captures, changed)


def test_options_are_pinned_at_open(eng_mid, pkg):
    """what tts_set_option stores while the session is open does not reach its requests"""
    r = req(pkg, [17], 3, tag=9)
    eng_mid.diff_session_open(1024, 2)
    try:
        with options(eng_mid, attn_f32=1, diff_sampler=1, latency_mode=1, hoist_integrator=0):
            rid = admit(eng_mid, r)
            while eng_mid.diff_session_step():
                pass
            got = eng_mid.diff_session_collect(rid)
    finally:
        eng_mid.diff_session_close()
    assert np.array_equal(got[0], alone(eng_mid, pkg, r)[0])


# ---- 3. layout edges --------------------------------------------------------------------------------------------------------------------------------------

def edge_cases(pkg):
    return {
        # T = 8 (T % 8 == 0) and T = 39 / 47 (T % 8 == 7): the guard row of a sequence is the last row of its chunk / opens a chunk of its own
        "guard_rows": [req(pkg, [2, 9], 3, tag=1), req(pkg, [11], 3, sampler=1, eta=1.0, at=1, tag=2)],
        # 120 rows (one 128-row tile) with the first request, 136 (two tiles) with the second
        "crosses_128": [req(pkg, [12], 4, tag=3), req(pkg, [1], 3, at=1, tag=4)],
        # equal lengths: the two-candidate request alone shares one unconditioned integrator sequence; the joint layout holds three
        "equal_lengths": [req(pkg, [13, 13], 3, tag=5), req(pkg, [13], 3, noise=None, seed=3, at=1, tag=6)],
        "one_row_two_steps": [req(pkg, [1], 2, tag=7), req(pkg, [3], 2, sampler=1, at=1, tag=8)],
        # T = 914 > 896: alone on the second GroupNorm kernel; T = 87 beside it: alone on the first
        "two_gn_classes": [req(pkg, [20], 4, tag=9), req(pkg, [210], 3, at=1, tag=10)],
    }


@pytest.mark.parametrize("hoist", [1, 0])
@pytest.mark.parametrize("case", ["guard_rows", "crosses_128", "equal_lengths", "one_row_two_steps", "two_gn_classes"])
def test_layout_edges(eng_small, pkg, case, hoist):
    reqs = edge_cases(pkg)[case]
    if case == "crosses_128":
        first, both = pkg.host_diff_packed_rows([12]), 8 + 2 * 56 + 2 * 8
        assert first == 128 and both > 128
    with options(eng_small, hoist_integrator=hoist):
        out, captures, changed = run_session(eng_small, reqs, 4096)
        assert_each_alone(eng_small, pkg, reqs, out, case)
    assert captures == changed


# ---- 4. time-shift invariance -------------------------------------------------------------------------------------------------------------------------------

def test_time_shift_invariance(eng_small, pkg):
    busy = req(pkg, [37], 9, tag=1)
    r0 = req(pkg, [22, 9], 4, tag=2)
    r3 = dict(r0, at=3)
    reqs = [busy, r0, r3, req(pkg, [15], 3, sampler=1, eta=0.5, at=4, tag=3)]
    out, _, _ = run_session(eng_small, reqs, 4096)
    for c in range(2):
        assert np.array_equal(out[1][c], out[2][c])
    assert_each_alone(eng_small, pkg, reqs, out)


# ---- 5. closed batch ----------------------------------------------------------------------------------------------------------------------------------------

def test_closed_batch_equals_tts_diffusion(eng_small, pkg):
    rows, n = [43, 17, 29], 5
    reqs = [req(pkg, [L], n, tag=i + 1) for i, L in enumerate(rows)]
    out, captures, _ = run_session(eng_small, reqs, 4096)
    assert captures == 1
    batch = eng_small.diffusion([r["latents"][0] for r in reqs], n_steps=n, noise=[r["noise"][0] for r in reqs])
    for i in range(len(rows)):
        assert np.array_equal(out[i][0], batch[i]), i


# ---- 6. cancel, close, reopen -------------------------------------------------------------------------------------------------------------------------------

def test_cancel_limits_and_reopen(eng_small, pkg):
    e = eng_small
    keep, drop = req(pkg, [21], 5, tag=1), req(pkg, [33], 6, sampler=1, eta=0.3, tag=2)
    lat, nz = _latents(19, 19), np.random.RandomState(19).randn(5, 100 * e.frames(19)).astype(np.float32)
    before = e.diffusion([lat], n_steps=4, noise=[nz])[0]
    need = [pkg.host_diff_packed_rows([21]), pkg.host_diff_packed_rows([33])]
    e.diff_session_open(sum(need), 2)
    try:
        assert e.diff_session_room() == sum(need)
        k, d = admit(e, keep), admit(e, drop)
        assert e.diff_session_room() == 0
        # no room / no free request: TTS_ERR_LIMIT, and the session goes on
        with pytest.raises(pkg.TtsError, match=r"status -6"):
            admit(e, req(pkg, [1], 2, tag=3))
        assert e.diff_session_step() == 2
        # a running request cannot be collected; the single calls refuse while the session is open
        with pytest.raises(pkg.TtsError, match=r"status -5"):
            e.diff_session_collect(k)
        with pytest.raises(pkg.TtsError, match=r"status -5"):
            e.diffusion([lat], n_steps=4, noise=[nz])
        with pytest.raises(pkg.TtsError, match=r"status -5"):
            e.diffusion_forward(lat, nz[0].reshape(100, -1), 10, False)
        assert e.diff_session_step() == 2
        e.diff_session_cancel(d)  # mid-flight
        assert e.diff_session_room() == need[1]
        with pytest.raises(pkg.TtsError, match=r"status -1"):
            e.diff_session_cancel(d)
        late = req(pkg, [33], 2, tag=4)
        l = admit(e, late)  # into the cancelled request's rows and slot
        while e.diff_session_step():
            pass
        assert sorted(e.diff_session_finished()) == sorted([k, l])
        got_keep, got_late = e.diff_session_collect(k), e.diff_session_collect(l)
        with pytest.raises(pkg.TtsError, match=r"status -1"):
            e.diff_session_collect(k)
    finally:
        e.diff_session_close()
    with pytest.raises(pkg.TtsError, match=r"status -5"):
        e.diff_session_step()
    assert np.array_equal(got_keep[0], alone(e, pkg, keep)[0])
    assert np.array_equal(got_late[0], alone(e, pkg, late)[0])
    # after close the single call is what it was; a reopened session starts empty
    assert np.array_equal(e.diffusion([lat], n_steps=4, noise=[nz])[0], before)
    out, captures, _ = run_session(e, [keep], 1024)
    assert captures == 1 and np.array_equal(out[0][0], got_keep[0])


def test_max_requests_and_hoisting_bound(eng_small, pkg):
    """TTS_ERR_LIMIT for a full request table while rows are free, and for a request above the hoisting bound; both before any device work, the session goes on"""
    e = eng_small
    r = req(pkg, [9], 3, tag=1)
    e.diff_session_open(4096, 1)
    try:
        rid = admit(e, r)
        assert e.diff_session_room() >= pkg.host_diff_packed_rows([9])
        with pytest.raises(pkg.TtsError, match=r"holds 1 requests.*status -6"):
            admit(e, req(pkg, [9], 2, tag=2))
        while e.diff_session_step():
            pass
        got = e.diff_session_collect(rid)
        rid2 = admit(e, r)  # the slot is free again
        e.diff_session_cancel(rid2)
    finally:
        e.diff_session_close()
    assert np.array_equal(got[0], alone(e, pkg, r)[0])
    with options(e, hoist_integrator=256):  # hoisting for layouts of at most 256 packed rows
        e.diff_session_open(4096, 4)
        try:
            assert pkg.host_diff_packed_rows([30]) == 384
            with pytest.raises(pkg.TtsError, match=r"at most 256.*status -6"):
                admit(e, req(pkg, [30], 2, tag=3))
            small = req(pkg, [20], 2, tag=4)
            rid = admit(e, small)
            while e.diff_session_step():
                pass
            got = e.diff_session_collect(rid)
        finally:
            e.diff_session_close()
        assert np.array_equal(got[0], alone(e, pkg, small)[0])


def test_collect_on_an_engine_without_session(eng_small, pkg):
    with pytest.raises(pkg.TtsError, match=r"status -5"):
        eng_small.diff_session_collect(0)
    with pytest.raises(pkg.TtsError, match=r"status -5"):
        eng_small.diff_session_cancel(0)


# ---- 7. pipeline: AR session -> diffusion session -----------------------------------------------------------------------------------------------------------

def test_ar_session_feeds_diffusion_session(eng_small, pkg, voice):
    e = eng_small
    toks = np.array([255, 147, 2, 54, 2, 14, 2, 136, 63, 2, 80, 32, 150, 112, 9, 0], np.int32)
    e.ar_session_open(4, 2, 32, 16, mask_stop=True, retire=True)
    e.diff_session_open(2048, 4)
    try:
        first = e.ar_session_admit(toks, voice, 1, 3, [12])
        second = e.ar_session_admit(toks[::-1].copy(), voice, 1, 4, [15])
        n, ar_steps = 4, 0
        while first not in e.ar_session_finished():
            e.ar_session_step()
            ar_steps += 1
            assert ar_steps <= 16
        codes, rows, lats, steps, stopped = e.ar_session_collect(first)
        lat = lats[0]
        noise = np.random.RandomState(1).randn(n + 1, 100 * e.frames(len(lat))).astype(np.float32)
        rid = e.diff_session_admit([lat], n_steps=n, noise=[noise])
        running = 1
        while running:  # the AR session stays open and steps on beside the diffusion session
            if second not in e.ar_session_finished():
                e.ar_session_step()
            running = e.diff_session_step()
        assert e.diff_session_finished() == [rid]
        mel = e.diff_session_collect(rid)[0]
        while second not in e.ar_session_finished():
            e.ar_session_step()
        assert len(e.ar_session_collect(second)[2][0]) > 0
    finally:
        e.diff_session_close()
        e.ar_session_close()
    assert np.array_equal(mel, e.diffusion([lat], n_steps=n, noise=[noise])[0])
