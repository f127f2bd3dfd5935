#!/usr/bin/env python3
"""SHA-256 digests of every mel the diffusion stage's front ends return, for comparing two builds of the library bit for bit (profiles/diff_step_refactor.txt).

The tests' small (1 + 1 + 1 + 1 blocks) and mid (2 + 1 + 3 + 1) synthetic diffusion models, fixed latents, noise and seeds. Every case runs in a fresh process; the
build is selected with TTS_LIB_PATH, so the comparison is two runs of this script and a diff of their outputs:

  TTS_LIB_PATH=/path/to/parent/libtortoise_mi355x.so python tools/diff_step_identity.py > parent.txt
  python tools/diff_step_identity.py > new.txt && diff parent.txt new.txt

Shapes are those of tests/test_diff_session_gpu.py: latent rows 2 (T = 8, T % 8 == 0), 9 and 11 (T = 39 and 47, T % 8 == 7), 1 (T = 4); two candidates of equal
(13, 13) and of different length; 2 steps (never captured), 3 and 6.

Cases (one line each, "<case> <sha256>"):
  single <sampler> <noise> <rows> n<steps>   tts_diffusion: anc / ddim0 / ddim0.5 (ancestral, DDIM eta 0, DDIM eta 0.5) x caller noise / device noise under a seed
  ref <sampler> <rows> pipe<0|1>             TTS_NOISE_REFERENCE: one candidate (the pipelined draw, noise_pipeline 1 and 0) and two; the RNG state afterwards
  opt <option>                               share_uncond 0, hoist_integrator 0, diff_graph 0, one at a time
  latency                                    latency_mode 1, one short utterance, device noise
  voices                                     tts_diffusion_multi_voice with two voices
  forward cond / forward uncond              tts_diffusion_forward on either branch
  prof                                       6 steps while the diff_gemm family is profiled, prof_eager_every 2: eager and replayed steps alternate
  session hoist<1|0>                         the staggered requests of test_diff_session_gpu.py on the mid model (a join, two finishes on one step, mixed samplers,
                                             a voice, the device generator) plus a request that is cancelled mid-flight: every collected mel, the steps at which
                                             they were collected, tts_diff_session_room after every step and tts_diff_session_captures

  python tools/diff_step_identity.py [--case NAME] [--work DIR]"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLERS = {"anc": (0, 0.0), "ddim0": (1, 0.0), "ddim0.5": (1, 0.5)}
SINGLE = [(s, nz, "2,9", 3) for s in SAMPLERS for nz in ("caller", "device")]
SINGLE += [("anc", "caller", "13,13", 6), ("anc", "device", "1", 2), ("ddim0", "device", "13,13", 2), ("ddim0.5", "caller", "1,11", 6)]
REF = [("anc", "9", 1), ("anc", "9", 0), ("ddim0.5", "11", 1), ("ddim0", "9", 1), ("anc", "2,9", 1)]


def case_names():
    names = ["single %s %s %s n%d" % c for c in SINGLE]
    names += ["ref %s %s pipe%d" % c for c in REF]
    names += ["opt share_uncond", "opt hoist_integrator", "opt diff_graph", "latency", "voices", "forward cond", "forward uncond", "prof"]
    return names + ["session hoist1", "session hoist0"]


def models(work):
    """The diffusion weights of the tests' small_models and mid_models."""
    from tortoise_cpp_amd import synth_weights as SW
    os.makedirs(work, exist_ok=True)
    small, mid = os.path.join(work, "small.bin"), os.path.join(work, "mid.bin")
    if not os.path.exists(os.path.join(work, ".done")):
        SW.write_diffusion(small, 1, 1, 1, 1, 4322)
        SW.write_diffusion(mid, 3, 1, 1, 2, 778)
        open(os.path.join(work, ".done"), "w").write("ok")
    return small, mid


def latents(rows, tag=0):
    return [np.random.RandomState(100 * tag + L + c).randn(L, 1024).astype(np.float32) for c, L in enumerate(rows)]


def caller_noise(pkg, rows, n_steps, sampler, eta, tag=0):
    n_vec = 1 if sampler == 1 and eta == 0 else n_steps + 1
    rs = np.random.RandomState(1000 + 7 * tag + n_steps)
    return [rs.randn(n_vec, 100 * pkg.Engine.frames(L)).astype(np.float32) for L in rows]


def voice(seed):
    return (0.3 * np.random.RandomState(seed).randn(2048)).astype(np.float32)


def add(h, *items):
    for x in items:
        if isinstance(x, (list, tuple)):
            add(h, *x)
        elif isinstance(x, np.ndarray):
            h.update(str((x.dtype, x.shape)).encode() + np.ascontiguousarray(x).tobytes())
        else:
            h.update(repr(x).encode())


def rng_state(e):
    with tempfile.TemporaryDirectory() as d:
        e.rng_save_state(os.path.join(d, "rng"))
        return open(os.path.join(d, "rng")).read()


def sample(e, pkg, sampler, noise, rows, n_steps, **kw):
    s, eta = SAMPLERS[sampler]
    e.set_option("diff_sampler", s)
    e.set_option("ddim_eta", eta)
    if noise == "caller":
        return e.diffusion(latents(rows), n_steps=n_steps, noise=caller_noise(pkg, rows, n_steps, s, eta), **kw)
    e.seed(11)
    return e.diffusion(latents(rows), n_steps=n_steps, noise=None, noise_mode=pkg.NOISE_DEVICE if noise == "device" else pkg.NOISE_REFERENCE, **kw)


def session(e, pkg, h):
    def req(rows, n_steps, sampler=0, eta=0.0, k=2.0, voice=None, explicit=True, seed=0, at=0, tag=0):
        return dict(latents=latents(rows, tag), n_steps=n_steps, sampler=sampler, ddim_eta=eta, cond_free_k=k, voice_latent=voice, seed=seed, at=at,
                    noise=caller_noise(pkg, rows, n_steps, sampler, eta, tag) if explicit else None)
    reqs = [req([43, 17], 6, tag=1), req([61], 4, sampler=1, k=1.0, voice=voice(5), at=2, tag=2), req([30], 5, explicit=False, seed=7, at=6, tag=3),
            req([25], 3, sampler=1, eta=0.5, at=6, tag=4), req([9], 6, at=7, tag=5)]
    cancel_at = {4: 9}  # request 4 leaves after step 9, mid-flight
    e.diff_session_open(pkg.host_diff_packed_rows([43, 17]) + pkg.host_diff_packed_rows([61]), 4)
    rid_of, left_of, pending, step = {}, {}, list(range(len(reqs))), 0
    while pending or rid_of:
        while pending and reqs[pending[0]]["at"] <= step:
            i = pending.pop(0)
            r = dict(reqs[i])
            r.pop("at")
            rid_of[i] = e.diff_session_admit(r.pop("latents"), **r)
            left_of[i] = reqs[i]["n_steps"]
        left = e.diff_session_step()
        step += 1
        for i in sorted(rid_of):
            left_of[i] -= 1
            if left_of[i] == 0:
                add(h, "collected", i, step, e.diff_session_collect(rid_of.pop(i)))
            elif cancel_at.get(i) == step:
                e.diff_session_cancel(rid_of.pop(i))
        add(h, step, left, e.diff_session_room(), e.diff_session_finished())
        assert step < 40
    add(h, "captures", e.diff_session_captures())
    e.diff_session_close()


def run_case(name, work):
    import tortoise_cpp_amd_loader
    pkg = tortoise_cpp_amd_loader.load()
    small, mid = models(work)
    h = hashlib.sha256()
    e = pkg.Engine(0)
    part = name.split()
    e.load(diffusion=mid if part[0] == "session" else small)
    rows = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    if part[0] == "single":
        add(h, sample(e, pkg, part[1], part[2], rows(part[3]), int(part[4][1:])))
    elif part[0] == "ref":
        e.set_option("noise_pipeline", int(part[3][4:]))
        add(h, sample(e, pkg, part[1], "reference", rows(part[2]), 3), rng_state(e))
    elif part[0] == "opt":
        e.set_option(part[1], 0)
        add(h, sample(e, pkg, "anc", "caller", [13, 13], 3), sample(e, pkg, "ddim0.5", "device", [2, 9], 3))
    elif name == "latency":
        e.set_option("latency_mode", 1)
        add(h, sample(e, pkg, "anc", "device", [9], 3))
    elif name == "voices":
        add(h, sample(e, pkg, "anc", "caller", [2, 9], 3, voice_latents=np.stack([voice(5), voice(6)]), voice_of_candidate=[1, 0]))
    elif part[0] == "forward":
        x_t = np.random.RandomState(3).randn(100, pkg.Engine.frames(9)).astype(np.float32)
        add(h, e.diffusion_forward(latents([9])[0], x_t, 10, part[1] == "uncond"))
    elif name == "prof":
        e.set_option("prof_only:diff_gemm", 1)
        e.set_option("prof_eager_every", 2)
        e.prof_reset(True)
        add(h, sample(e, pkg, "anc", "caller", [2, 9], 6))
        e.prof_reset(False)
    elif part[0] == "session":
        e.set_option("hoist_integrator", int(part[1][5:]))
        session(e, pkg, h)
    else:
        raise SystemExit("unknown case %r" % name)
    e.close()
    print("%-32s %s" % (name, h.hexdigest()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--work", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "diff_step_identity"))
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.work)
    for name in case_names():  # a fresh process per case; a case that fails ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--work", a.work], timeout=120)
        if r.returncode != 0:
            raise SystemExit("case %r ended with status %d" % (name, r.returncode))


if __name__ == "__main__":
    main()
