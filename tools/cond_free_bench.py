"""Developer tool: wall time of the diffusion stage call (tts_diffusion, synchronous) guided (option cond_free 1, the default) against unguided (cond_free 0),
benchmark weights and benchmark length (L = 200 latent rows, T = 870 frames), and of a replayed diffusion-session step, all requests guided against all
unguided. The method of tools/ddim_sampler_bench.py: calls timed on the host after two warm-ups; every configuration is run `--runs` times (default 3), guided and
unguided alternating, and every run's median is printed with the spread over the runs. The record of one run is profiles/cond_free.txt.

  python tools/cond_free_bench.py [--calls 3] [--runs 3] [--out FILE]

16 candidates, device noise: 80 DDPM, 30 DDIM (eta 0) and 15 DPM-Solver++(2M) steps. One utterance, reference-order noise from the context's generator (what
./tortoise runs): the same three, with latency_mode 0 and 1. Session: 4 one-candidate requests of 120 latent rows admitted together, 30 DDIM steps; the figure is
the median tts_diff_session_step call after the capturing one."""
import argparse
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

pkg = tortoise_cpp_amd_loader.load()
import bench  # noqa: E402

SAMPLERS = ((0, "DDPM", 80), (1, "DDIM", 30), (3, "2M", 15))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models")
    bench.ensure_models(d, False, True)
    eng = pkg.Engine(0)
    eng.load(diffusion=d + "/ggml-diffusion-model.bin")
    L = 200
    lines = ["host %s, %s, %d runs per configuration (guided and unguided alternating), each the median of %d timed tts_diffusion calls after 2 warm-ups, "
             "L = %d (T = %d), benchmark weights" % (socket.gethostname(), time.strftime("%Y-%m-%d"), a.runs, a.calls, L, eng.frames(L))]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def stage_ms(lats, steps, mode):
        eng.seed(0)
        ts = []
        for _ in range(2 + a.calls):
            t0 = time.perf_counter()
            eng.diffusion(lats, n_steps=steps, noise_mode=mode)
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts[2:])

    def compare(B, sampler, name, steps, mode, latency):
        lats = [np.random.RandomState(c).randn(L, 1024).astype(np.float32) for c in range(B)]
        eng.set_option("diff_sampler", sampler)
        eng.set_option("latency_mode", latency)
        ms, layout = {1: [], 0: []}, {}
        for _ in range(a.runs):
            for cf in (1, 0):
                eng.set_option("cond_free", cf)
                ms[cf].append(stage_ms(lats, steps, mode))
                layout[cf] = eng.diffusion_last_layout()
        eng.set_option("cond_free", 1)
        eng.set_option("latency_mode", 0)
        eng.set_option("diff_sampler", 0)
        g, u = statistics.median(ms[1]), statistics.median(ms[0])
        say("B = %2d  %-4s %3d steps  %-15s latency_mode %d  guided %s ms (%d rows, %d seq)  unguided %s ms (%d rows, %d seq)  medians %.1f -> %.1f ms, quotient %.3f"
            % (B, name, steps, "device noise" if mode == pkg.NOISE_DEVICE else "reference noise", latency, " / ".join("%.1f" % x for x in ms[1]), layout[1][0],
               layout[1][1], " / ".join("%.1f" % x for x in ms[0]), layout[0][0], layout[0][1], g, u, u / g))

    for sampler, name, steps in SAMPLERS:
        compare(16, sampler, name, steps, pkg.NOISE_DEVICE, 0)
    for latency in (0, 1):
        for sampler, name, steps in SAMPLERS:
            compare(1, sampler, name, steps, pkg.NOISE_REFERENCE, latency)

    # a replayed session step: 4 requests x 120 rows at the same step
    rs = np.random.RandomState(5)
    lats = [rs.randn(120, 1024).astype(np.float32) for _ in range(4)]

    def session_step_ms(cond_free, n_steps=30):
        eng.diff_session_open(4 * pkg.host_diff_packed_rows([120]), 4)
        for i, l in enumerate(lats):
            eng.diff_session_admit([l], n_steps=n_steps, sampler=1, seed=i, cond_free=cond_free)
        used = 4 * pkg.host_diff_packed_rows([120]) - eng.diff_session_room()
        ms = []
        for _ in range(n_steps):
            t0 = time.perf_counter()
            eng.diff_session_step()
            ms.append(1e3 * (time.perf_counter() - t0))
        eng.diff_session_close()
        return statistics.median(ms[2:]), used

    sess, used = {1: [], 0: []}, {}
    for _ in range(a.runs):
        for cf in (1, 0):
            m, used[cf] = session_step_ms(cf)
            sess[cf].append(m)
    say("session step, 4 requests x 120 latent rows, DDIM, replayed graph: all guided %s ms (%d rows admitted)  all unguided %s ms (%d rows admitted)  medians %.3f -> %.3f ms, "
        "quotient %.3f" % (" / ".join("%.3f" % x for x in sess[1]), used[1], " / ".join("%.3f" % x for x in sess[0]), used[0], statistics.median(sess[1]),
                           statistics.median(sess[0]), statistics.median(sess[0]) / statistics.median(sess[1])))
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
