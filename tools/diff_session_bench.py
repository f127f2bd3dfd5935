#!/usr/bin/env python3
"""In-flight batching of the diffusion stage against static batching on one arrival list, and what a session step costs against a tts_diffusion step.

Full-size synthetic diffusion weights (4 + 3 + 10 + 3 blocks), one process, one loaded model, a fixed list of requests: latent rows, step count, sampler and
arrival time. The clock of both schedulers is virtual: it advances by the measured host time of every synchronous call and jumps to the next arrival when
nothing runs, so the list is replayed without sleeping and both schedulers see the same arrivals.
  (a) static batching: an arrival waits for the running tts_diffusion call; when it returns, the queued requests that share the first one's controls (step count,
      sampler, eta, k: one closed batch runs under one set) form the next batch, at most --rows packed rows
  (b) the session: tts_diff_session_admit as soon as a request has arrived and its packed rows are free, tts_diff_session_collect as soon as it has finished
For each: mean and 95th percentile of the time from arrival to mel, and the makespan of the list.
  (c) a session step with every request at the same step (--cand one-candidate requests of --lat-rows rows admitted together) against tts_diffusion's step at
      the same packed shape: tts_diffusion is timed at two step counts and the difference divided by the difference in steps, which leaves its setup out; the
      session's figure is the median tts_diff_session_step call after the capturing one. Both alternate --rounds times in this process.
--single-only: the tts_diffusion half of (c) alone. With TTS_LIB_PATH pointing at a build of the parent commit, and run in two or more processes, this is the
      parent's own step time and its process-to-process spread, next to which (c)'s difference is to be read.

  python tools/diff_session_bench.py [--requests 12] [--seed 1] [--rows 8192] [--cand 4] [--lat-rows 120] [--rounds 3] [--single-only] [--models DIR] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

CONTROLS = [dict(n_steps=80, sampler=0, eta=0.0, k=2.0), dict(n_steps=30, sampler=1, eta=0.0, k=2.0)]


def make_requests(n, seed):
    """one candidate each, 60 .. 200 latent rows, alternately 80 ancestral and 30 DDIM steps, arrivals ~ one per 150 ms"""
    rs = np.random.RandomState(seed)
    out, t = [], 0.0
    for k in range(n):
        L = int(rs.randint(60, 201))
        out.append(dict(lat=rs.randn(L, 1024).astype(np.float32), rows=L, at=t, seed=1000 + k, **CONTROLS[k % 2]))
        t += float(rs.exponential(0.150))
    return out


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(np.ceil(q * len(xs))) - 1)]


def set_controls(e, r):
    e.set_option("diff_sampler", r["sampler"])
    e.set_option("ddim_eta", r["eta"])
    e.set_option("cond_free_k", r["k"])


def static_batching(e, pkg, reqs, max_rows):
    clock, done, queue = 0.0, {}, list(range(len(reqs)))
    while queue:
        clock = max(clock, reqs[queue[0]]["at"])  # idle until the next arrival
        first = reqs[queue[0]]
        batch = []
        for k in queue:
            r = reqs[k]
            same = all(r[f] == first[f] for f in ("n_steps", "sampler", "eta", "k"))
            if r["at"] <= clock and same and pkg.host_diff_packed_rows([reqs[j]["rows"] for j in batch + [k]]) <= max_rows:
                batch.append(k)
        set_controls(e, first)
        e.seed(7)
        t0 = time.perf_counter()
        e.diffusion([reqs[k]["lat"] for k in batch], n_steps=first["n_steps"], noise=None, noise_mode=pkg.NOISE_DEVICE)
        clock += time.perf_counter() - t0
        for k in batch:
            done[k] = clock - reqs[k]["at"]
            queue.remove(k)
    set_controls(e, CONTROLS[0])
    return done, clock


def session(e, pkg, reqs, max_rows):
    e.diff_session_open(max_rows, len(reqs))
    clock, done, rid_of = 0.0, {}, {}
    waiting = list(range(len(reqs)))
    while waiting or rid_of:
        if not rid_of:
            clock = max(clock, reqs[waiting[0]]["at"])
        t0 = time.perf_counter()
        for k in list(waiting):
            r = reqs[k]
            if r["at"] <= clock and pkg.host_diff_packed_rows([r["rows"]]) <= e.diff_session_room():
                rid_of[k] = e.diff_session_admit([r["lat"]], n_steps=r["n_steps"], sampler=r["sampler"], ddim_eta=r["eta"], cond_free_k=r["k"], seed=r["seed"])
                waiting.remove(k)
        e.diff_session_step()
        fin = e.diff_session_finished()
        for k in [k for k, rid in rid_of.items() if rid in fin]:
            e.diff_session_collect(rid_of.pop(k))
            done[k] = None
        clock += time.perf_counter() - t0
        for k in done:
            if done[k] is None:
                done[k] = clock - reqs[k]["at"]
    captures = e.diff_session_captures()
    e.diff_session_close()
    return done, clock, captures


def single_step_ms(e, pkg, lats, n_lo=10, n_hi=30):
    t = {}
    for n in (n_lo, n_hi, n_lo, n_hi):
        e.seed(3)
        t0 = time.perf_counter()
        e.diffusion(lats, n_steps=n, noise=None, noise_mode=pkg.NOISE_DEVICE)
        t.setdefault(n, []).append(time.perf_counter() - t0)
    return 1e3 * (min(t[n_hi]) - min(t[n_lo])) / (n_hi - n_lo)


def session_step_ms(e, pkg, lats, n_steps=30):
    e.diff_session_open(pkg.host_diff_packed_rows([len(l) for l in lats]) * len(lats), len(lats))
    for i, l in enumerate(lats):
        e.diff_session_admit([l], n_steps=n_steps, seed=i)
    ms = []
    for _ in range(n_steps):
        t0 = time.perf_counter()
        e.diff_session_step()
        ms.append(1e3 * (time.perf_counter() - t0))
    e.diff_session_close()
    return statistics.median(ms[2:]), ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=12)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cand", type=int, default=4)
    ap.add_argument("--lat-rows", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--models", default=os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = tortoise_cpp_amd_loader.load()
    from tortoise_cpp_amd import synth_weights as sw
    os.makedirs(a.models, exist_ok=True)
    path = os.path.join(a.models, "ggml-diffusion-model.bin")
    if not os.path.exists(path):
        sw.write_diffusion(path, 10, 3, 3, 4, 1235)
    e = pkg.Engine(0)
    e.load(diffusion=path)
    lines = ["diff_session_bench: full-size synthetic diffusion weights, library %s" % pkg.LIB_PATH]
    rs = np.random.RandomState(5)
    lats = [rs.randn(a.lat_rows, 1024).astype(np.float32) for _ in range(a.cand)]
    shape = "%d candidates x %d latent rows" % (a.cand, a.lat_rows)
    e.diffusion(lats, n_steps=4, noise=None, noise_mode=pkg.NOISE_DEVICE)  # warm: code objects, allocations
    if a.single_only:
        xs = [single_step_ms(e, pkg, lats) for _ in range(a.rounds)]
        lines.append("tts_diffusion step, %s: %s ms (median %.3f, min %.3f .. max %.3f)" % (shape, " ".join("%.3f" % x for x in xs), statistics.median(xs), min(xs), max(xs)))
    else:
        reqs = make_requests(a.requests, a.seed)
        e.diffusion([reqs[0]["lat"]], n_steps=4, noise=None, noise_mode=pkg.NOISE_DEVICE)
        st, st_span = static_batching(e, pkg, reqs, a.rows)
        se, se_span, captures = session(e, pkg, reqs, a.rows)
        lines.append("(a)/(b) %d requests (one candidate, 60 .. 200 rows; 80 ancestral / 30 DDIM steps alternately; arrivals ~ one per 150 ms), %d packed rows" % (len(reqs), a.rows))
        lines.append("scheduler          arrival -> mel: mean s    p95 s    makespan s")
        for name, d, span in (("static batching", st, st_span), ("session", se, se_span)):
            v = list(d.values())
            lines.append("%-18s %22.3f %8.3f %13.3f" % (name, statistics.mean(v), pct(v, 0.95), span))
        lines.append("session: %d step graphs captured" % captures)
        single, sess, first = [], [], []
        for _ in range(a.rounds):
            single.append(single_step_ms(e, pkg, lats))
            m, f = session_step_ms(e, pkg, lats)
            sess.append(m)
            first.append(f)
        lines.append("(c) step time, %s, %d alternating rounds in this process" % (shape, a.rounds))
        lines.append("tts_diffusion step:        %s ms (median %.3f, min %.3f .. max %.3f)" % (" ".join("%.3f" % x for x in single), statistics.median(single), min(single), max(single)))
        lines.append("tts_diff_session_step:     %s ms (median %.3f, min %.3f .. max %.3f); its first call, with layout build and capture: %s ms" % (
            " ".join("%.3f" % x for x in sess), statistics.median(sess), min(sess), max(sess), " ".join("%.1f" % x for x in first)))
    e.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
