"""Developer tool: wall time of the diffusion stage call (tts_diffusion, synchronous) under the three samplers, by the method of tools/ddim_sampler_bench.py:
benchmark weights and benchmark length (L = 200 latent rows, T = 870 frames), median of `--calls` timed calls after two warm-ups. The record of one run is
profiles/dpmpp_sampler.txt.

  python tools/dpmpp_sampler_bench.py [--calls 5] [--out FILE]

Batch of 16 candidates, device noise: DDPM at 80 steps, DDIM (eta 0) at 80, DPM-Solver++(2M) at 80, 20, 15 and 10 steps, DDPM at 80 again. One candidate,
reference-order noise from the context's generator (what ./tortoise runs): DDPM at 80 steps, DPM-Solver++(2M) at 20, 15 and 10."""
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

NAMES = {0: "DDPM", 1: "DDIM", 3: "2M"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models")
    bench.ensure_models(d, False, True)
    eng = pkg.Engine(0)
    eng.load(diffusion=d + "/ggml-diffusion-model.bin")
    L = 200
    lines = ["host %s, %s, median of %d timed tts_diffusion calls after 2 warm-ups, L = %d (T = %d), benchmark weights" %
             (socket.gethostname(), time.strftime("%Y-%m-%d"), a.calls, L, eng.frames(L))]

    def run(B, sampler, steps, mode):
        lats = [np.random.RandomState(c).randn(L, 1024).astype(np.float32) for c in range(B)]
        eng.set_option("diff_sampler", sampler)
        eng.seed(0)
        ts = []
        for i in range(2 + a.calls):
            t0 = time.perf_counter()
            eng.diffusion(lats, n_steps=steps, noise_mode=mode)
            ts.append(1e3 * (time.perf_counter() - t0))
        ts = ts[2:]
        med = statistics.median(ts)
        lines.append("B = %2d  %-4s %3d steps  %-16s  median %8.1f ms  (min %8.1f max %8.1f)  %7.3f ms/step" %
                     (B, NAMES[sampler], steps, "device noise" if mode == pkg.NOISE_DEVICE else "reference noise", med, min(ts), max(ts), med / steps))
        print(lines[-1], flush=True)
        return med / steps

    per = {}
    for sampler, steps in ((0, 80), (1, 80), (3, 80), (3, 20), (3, 15), (3, 10), (0, 80)):  # DDPM-80 twice, first and last: the run-to-run noise on this box
        per.setdefault((sampler, steps), []).append(run(16, sampler, steps, pkg.NOISE_DEVICE))
    lo, hi = sorted(per[(0, 80)])
    for sampler in (3, 1):
        v = per[(sampler, 80)][0]
        lines.append("per-step %s-80 at B = 16: %.3f ms, quotient to the mean DDPM-80 %.4f; the two DDPM-80 runs: %.3f and %.3f ms/step (quotients %.4f and %.4f): %s" %
                     (NAMES[sampler], v, v / statistics.mean((lo, hi)), per[(0, 80)][0], per[(0, 80)][1], lo / statistics.mean((lo, hi)), hi / statistics.mean((lo, hi)),
                      "inside their spread" if lo <= v <= hi else "outside their spread"))
        print(lines[-1], flush=True)
    run(1, 0, 80, pkg.NOISE_REFERENCE)
    for steps in (20, 15, 10):
        run(1, 3, steps, pkg.NOISE_REFERENCE)
    eng.set_option("diff_sampler", 0)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
