#!/usr/bin/env python3
"""In-flight batching against static batching on one arrival list, and what a session step costs against a plain step.

Full-size synthetic weights (30 GPT-2 layers), one process, one loaded model, a fixed list of requests: text length, number of codes (through stop_at, with
TTS_AR_MASK_STOP | TTS_AR_RETIRE) and arrival step. The clock of both schedulers is the decode step: a request "arrives" once that many steps have run.
  (a) static batching: whatever has queued when the previous batch ends runs through tts_autoregressive_multi (at most --slots rows per batch, in arrival order);
      a batch occupies the clock for as many steps as its longest request
  (b) the session: tts_ar_session_admit as soon as a request has arrived and a run of free slots exists, tts_ar_session_collect as soon as it is finished
For each: mean and 95th percentile of steps and of wall time from arrival to collected latents, and codes per second over the whole list. The wall time of a request
is the host clock from the moment the scheduler's step counter reached its arrival step.
  (c) a full session step (every slot live, all rows at the same step) alternated with tts_ar_step_sample at the same B: what the per-row block costs per step
Host clock around synchronous calls; the two variants of (c) alternate in blocks, WARM untimed steps in front of each block, then the median and min .. max.

--audio STRIDE (session audio: tts_ar_session_enable_audio, synthetic HiFi-GAN weights) replaces (a) .. (c) by
  (d) the session with audio at that stride, drained after every step: per request the wall time from arrival to its first and to its last samples, and the
      mean time of a tts_ar_session_step call (the audio passes included)
  (e) the same session without audio: the mean time of a step, and arrival -> collected latents
  (f) the static baseline: the same requests through tts_hifigan_stream at the same stride, one after another in arrival order

--row-controls (sessions opened with TTS_AR_ROW_CONTROLS: the step ends with the per-row prefilter) replaces (a) .. (c) by the same arrival list through
  (g) a uniform session (every request under the session's controls: the step ends with the uniform prefilter)
  (h) a rows session whose requests all carry the session's own controls: the work is identical, only the step's last node differs
  (i) a rows session with mixed controls (a quarter of the requests each: the session's; temperature 1.3, top_k 5, top_p 0.5, penalty 1.2; scope 1, penalty 3,
      top_k 100; scope 1, top_k 200, whose rows take the full-row path). Other codes are sampled, the stop schedule keeps the lengths: the same number of steps.
(g) and (h) alternate --rounds times; per run the mean and median time of a tts_ar_session_step call, then per kind the median over the runs and the run-to-run
spread (min .. max of the runs' means). --uniform-only: (g) alone (the same list on another build of the library, through TTS_LIB_PATH).

  python tools/ar_session_bench.py [--slots 16] [--requests 24] [--seed 1] [--steps 200] [--warm 20] [--audio STRIDE | --row-controls [--rounds 3] | --uniform-only]
                                   [--models DIR] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

MAX_STEPS = 500


def make_requests(n, seed):
    """(text ids, n_cand, codes, arrival step): utterances of 60 .. 400 codes, prompts of 12 .. 200 ids, one candidate each, arrivals ~ one per 40 steps"""
    rs = np.random.RandomState(seed)
    out, t = [], 0
    for k in range(n):
        n_text = int(rs.randint(12, 201))
        tok = np.concatenate([[255], rs.randint(1, 250, n_text - 2), [0]]).astype(np.int32)
        out.append(dict(tokens=tok, n_cand=1, codes=int(rs.randint(60, 401)), at=t, seed=1000 + k))
        t += int(rs.exponential(40.0))
    return out


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(np.ceil(q * len(xs))) - 1)]


def static_batching(e, reqs, voice, slots):
    clock, t_arr, done = 0, {}, {}
    queue = list(range(len(reqs)))
    t0 = time.perf_counter()
    while queue:
        if reqs[queue[0]]["at"] > clock:
            clock = reqs[queue[0]]["at"]  # idle until the next arrival
        now = time.perf_counter()
        for k in queue:
            if reqs[k]["at"] <= clock:
                t_arr.setdefault(k, now)
        batch = [k for k in queue if reqs[k]["at"] <= clock][:slots]
        e.set_stop_schedule([reqs[k]["codes"] for k in batch])
        e.seed(7)
        _, _, _, steps = e.autoregressive_multi([reqs[k]["tokens"] for k in batch], voice, [1] * len(batch), MAX_STEPS, mask_stop=True, retire=True)
        e.set_stop_schedule(None)
        clock += steps
        now = time.perf_counter()
        for k in batch:
            done[k] = (clock - reqs[k]["at"], now - t_arr[k])
            queue.remove(k)
    return done, time.perf_counter() - t0


MIXED_CONTROLS = [None, dict(temperature=1.3, top_k=5, top_p=0.5, penalty=1.2, scope=0), dict(scope=1, penalty=3.0, top_k=100), dict(scope=1, top_k=200)]


def session(e, reqs, voice, slots, audio=0, stats=None, rows=None):
    """audio: the stride of tts_ar_session_enable_audio (0: a session without audio). stats, when given, receives step_ms (every tts_ar_session_step call) and
    first / last ({request: seconds from arrival to its first / last samples}). rows: None = a uniform session; "own" = a rows session, every request
    admitted with the session's own controls through tts_ar_session_admit_ex; "mixed" = request k under MIXED_CONTROLS[k % 4]."""
    clock, t_arr, done, rid_of = 0, {}, {}, {}
    queue = list(range(len(reqs)))
    step_ms, first, last = [], {}, {}
    if rows:
        e.ar_session_open(slots, 1, max(len(r["tokens"]) for r in reqs), MAX_STEPS, mask_stop=True, retire=True, row_controls=True)
    else:
        e.ar_session_open(slots, 1, max(len(r["tokens"]) for r in reqs), MAX_STEPS, mask_stop=True, retire=True)
    if audio:
        e.ar_session_enable_audio(audio)
    t0 = time.perf_counter()
    try:
        while queue or rid_of:
            now = time.perf_counter()
            for k in queue:
                if reqs[k]["at"] <= clock:
                    t_arr.setdefault(k, now)
            for rid in e.ar_session_finished():
                k = rid_of.pop(rid)
                e.ar_session_collect(rid)
                done[k] = (clock - reqs[k]["at"], time.perf_counter() - t_arr[k])
            while queue and reqs[queue[0]]["at"] <= clock and e.ar_session_room() >= reqs[queue[0]]["n_cand"]:
                k = queue.pop(0)
                kw = dict(controls=(MIXED_CONTROLS[k % 4] or {}) if rows == "mixed" else {}) if rows else {}
                rid_of[e.ar_session_admit(reqs[k]["tokens"], voice, 1, reqs[k]["seed"], [reqs[k]["codes"]], **kw)] = k
            if rid_of:
                t1 = time.perf_counter()
                e.ar_session_step()
                t2 = time.perf_counter()
                step_ms.append((t2 - t1) * 1e3)
                clock += 1
                if audio:
                    for rid, k in rid_of.items():
                        samples, _ = e.ar_session_audio(rid)
                        if len(samples):
                            now = time.perf_counter()
                            first.setdefault(k, now - t_arr[k])
                            last[k] = now - t_arr[k]
            elif queue:
                clock = max(clock, reqs[queue[0]]["at"])
    finally:
        e.ar_session_close()
    if stats is not None:
        stats.update(step_ms=step_ms, first=first, last=last)
    return done, time.perf_counter() - t0


def static_stream(e, reqs, voice, stride):
    """the requests one after another through tts_hifigan_stream, in arrival order; returns {request: (seconds from the call's start to its first samples,
    to its last)}. A request that arrives while an earlier call runs waits for it: that queueing delay is not in these numbers."""
    out = {}
    for k, r in enumerate(reqs):
        times = []

        def on_chunk(samples, is_last):
            times.append(time.perf_counter())
        e.set_stop_schedule([r["codes"]])
        e.seed(r["seed"])
        t0 = time.perf_counter()
        e.hifigan_stream(r["tokens"], voice, MAX_STEPS, 3, stride, on_chunk=on_chunk)
        e.set_stop_schedule(None)
        out[k] = (times[0] - t0, times[-1] - t0)
    return out


def audio_mode(e, reqs, voice, slots, stride, say):
    session(e, reqs[:min(4, len(reqs))], voice, slots, audio=stride)  # warm-up (untimed): graphs, buffers
    a, b = {}, {}
    _, wall_a = session(e, reqs, voice, slots, audio=stride, stats=a)
    done_b, wall_b = session(e, reqs, voice, slots, stats=b)
    say("(d) session, audio stride %d: tts_ar_session_step mean %.3f ms median %.3f ms over %d steps (%.2f s in all)" %
        (stride, statistics.mean(a["step_ms"]), statistics.median(a["step_ms"]), len(a["step_ms"]), wall_a))
    say("(e) session, no audio      : tts_ar_session_step mean %.3f ms median %.3f ms over %d steps (%.2f s in all); arrival -> latents mean %.1f ms" %
        (statistics.mean(b["step_ms"]), statistics.median(b["step_ms"]), len(b["step_ms"]), wall_b, statistics.mean(d[1] * 1e3 for d in done_b.values())))
    t0 = time.perf_counter()
    st = static_stream(e, reqs, voice, stride)
    wall_f = time.perf_counter() - t0
    say("(f) static tts_hifigan_stream, stride %d, one request after another: %.2f s in all" % (stride, wall_f))
    say("    request  codes  ids | session: first audio  last audio | stream alone: first audio  last audio   (ms from arrival; the stream's from its own start)")
    for k, r in enumerate(reqs):
        say("    %7d  %5d  %3d | %20.1f  %10.1f | %25.1f  %10.1f" % (k, r["codes"], len(r["tokens"]), a["first"].get(k, float("nan")) * 1e3,
                                                                    a["last"].get(k, float("nan")) * 1e3, st[k][0] * 1e3, st[k][1] * 1e3))
    fa, la = [a["first"][k] * 1e3 for k in a["first"]], [a["last"][k] * 1e3 for k in a["last"]]
    say("    session: first audio mean %.1f ms p95 %.1f ms, last audio mean %.1f ms p95 %.1f ms" % (statistics.mean(fa), pct(fa, 0.95), statistics.mean(la), pct(la, 0.95)))
    say("    stream : first audio mean %.1f ms, last audio mean %.1f ms (each from its own start: the queueing behind earlier requests is on top)" %
        (statistics.mean(v[0] * 1e3 for v in st.values()), statistics.mean(v[1] * 1e3 for v in st.values())))


def row_controls_mode(e, reqs, voice, slots, rounds, say, uniform_only=False):
    kinds = [("(g) uniform session", None)] if uniform_only else [("(g) uniform session", None), ("(h) rows session, own controls", "own")]
    for _, rows in kinds:  # warm-up (untimed): graphs, buffers
        session(e, reqs[:min(4, len(reqs))], voice, slots, rows=rows)
    means = {name: [] for name, _ in kinds}
    say("    %-34s %5s  %6s  %12s  %12s  %10s  %9s" % ("session kind", "round", "steps", "step mean ms", "step med. ms", "fallbacks", "wall s"))

    def one(name, rows, rnd):
        st = {}
        _, wall = session(e, reqs, voice, slots, stats=st, rows=rows)
        say("    %-34s %5d  %6d  %12.4f  %12.4f  %10d  %9.2f" % (name, rnd, len(st["step_ms"]), statistics.mean(st["step_ms"]), statistics.median(st["step_ms"]),
                                                               e.topk_fallbacks(), wall))
        return statistics.mean(st["step_ms"])

    for rnd in range(rounds):
        for name, rows in kinds:
            means[name].append(one(name, rows, rnd))
    if not uniform_only:
        session(e, reqs[:min(4, len(reqs))], voice, slots, rows="mixed")
        means["(i) rows session, mixed controls"] = [one("(i) rows session, mixed controls", "mixed", rnd) for rnd in range(rounds)]
    for name, m in means.items():
        say("    %-34s step mean over %d runs: median %.4f ms, run-to-run min %.4f .. max %.4f (spread %.4f ms = %.2f %%)" %
            (name, len(m), statistics.median(m), min(m), max(m), max(m) - min(m), 100.0 * (max(m) - min(m)) / statistics.median(m)))
    if not uniform_only:
        u, r = statistics.median(means["(g) uniform session"]), statistics.median(means["(h) rows session, own controls"])
        say("    rows (own controls) - uniform: %+.4f ms per step (%+.2f %%); uniform run-to-run spread %.4f ms" %
            (r - u, 100.0 * (r - u) / u, max(means["(g) uniform session"]) - min(means["(g) uniform session"])))


def step_cost(e, voice, B, steps, warm, rounds=4):
    """blocks of tts_ar_step_sample steps and of session steps with every slot live, alternated (a session excludes tts_ar_step* while it is open, so the
    alternation is by block, not by step); every block starts from a fresh begin / a fresh session, so both run the same context lengths"""
    tok = np.concatenate([[255], np.arange(1, 15), [0]]).astype(np.int32)
    n = max(1, steps // rounds)
    ts, tp = [], []
    for _ in range(rounds):
        e.ar_begin(tok, voice, B, warm + n + 1)
        e.ar_prefill()
        prev = np.full(B, 100, np.int32)
        for i in range(warm + n):
            t0 = time.perf_counter()
            prev = e.ar_step_sample(prev, i, mask_stop=True)
            t1 = time.perf_counter()
            if i >= warm:
                tp.append((t1 - t0) * 1e3)
        e.ar_session_open(B, 1, len(tok), warm + n + 2, mask_stop=True, retire=True)
        try:
            for b in range(B):
                e.ar_session_admit(tok, voice, 1, b, None)
            for i in range(warm + n):
                t0 = time.perf_counter()
                e.ar_session_step()
                t1 = time.perf_counter()
                if i >= warm:
                    ts.append((t1 - t0) * 1e3)
        finally:
            e.ar_session_close()
    return tp, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--requests", type=int, default=24)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--audio", type=int, default=0, metavar="STRIDE")
    ap.add_argument("--row-controls", action="store_true")
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", default=os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = tortoise_cpp_amd_loader.load()
    from tortoise_cpp_amd import synth_weights as sw
    os.makedirs(a.models, exist_ok=True)
    ar_path = os.path.join(a.models, "ggml-model.bin")
    if not os.path.exists(ar_path):
        sw.write_ar(ar_path, 30, seed=1234)
    e = pkg.Engine(0)
    e.load(ar=ar_path)
    voice = np.fromfile(os.path.join(ROOT, "models", "mol.bin"), np.float32)
    reqs = make_requests(a.requests, a.seed)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("tools/ar_session_bench.py: %d requests (seed %d), %d slots, codes %d .. %d, arrivals over %d steps" %
        (len(reqs), a.seed, a.slots, min(r["codes"] for r in reqs), max(r["codes"] for r in reqs), reqs[-1]["at"]))
    if a.audio:
        hfg = os.path.join(a.models, "ggml-hifigan-model.bin")
        if not os.path.exists(hfg):
            sw.write_hifigan(hfg, seed=77)
        e.load_hifigan(hfg)
        audio_mode(e, reqs, voice, a.slots, a.audio, say)
        e.close()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n" + "\n".join(lines) + "\n")
        return
    if a.row_controls or a.uniform_only:
        row_controls_mode(e, reqs, voice, a.slots, a.rounds, say, uniform_only=a.uniform_only)
        e.close()
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n" + "\n".join(lines) + "\n")
        return
    total_codes = sum(r["codes"] for r in reqs)
    for name, fn in (("warm-up (untimed)", static_batching), ("(a) static batching", static_batching), ("(b) session", session)):
        done, wall = fn(e, reqs, voice, a.slots)
        if name.startswith("warm"):
            continue
        st, wt = [d[0] for d in done.values()], [d[1] * 1e3 for d in done.values()]
        say("%-20s arrival -> latents: steps mean %7.1f p95 %5d | wall mean %8.1f ms p95 %8.1f ms | %7.1f codes/s (%.2f s in all)" %
            (name, statistics.mean(st), pct(st, 0.95), statistics.mean(wt), pct(wt, 0.95), total_codes / wall, wall))
    tp, ts = step_cost(e, voice, a.slots, a.steps, a.warm)
    say("(c) B = %d, %d steps each, every row live at the same step (host clock around the synchronous call):" % (a.slots, a.steps))
    say("    tts_ar_step_sample   median %.3f ms (min %.3f .. max %.3f)" % (statistics.median(tp), min(tp), max(tp)))
    say("    tts_ar_session_step  median %.3f ms (min %.3f .. max %.3f)" % (statistics.median(ts), min(ts), max(ts)))
    e.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
