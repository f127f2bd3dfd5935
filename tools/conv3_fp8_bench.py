#!/usr/bin/env python3
"""A/B of option conv3_fp8 at the benchmark's diffusion layout: 16 candidates of 200 latent rows (28 032 packed rows), 80 steps, full-depth synthetic weights.

One process, two engines (one loaded with conv3_fp8 = 1, one with 0, so that the default engine holds no fp8 images), the two options interleaved call by call:
warm-up calls, then --calls timed calls each (host clock around tts_diffusion, which ends in a device synchronise). A second, shorter pass with the profiler on
and graphs off gives the per-launch device time of the k = 3 class: diff_gemm_k3r (fp16) against diff_conv3_f8 + diff_quant_f8. Prints medians with their ranges;
a gain is claimed only where the ranges do not touch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cand", type=int, default=16)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", default=os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"))
    a = ap.parse_args()
    import tortoise_cpp_amd_loader
    pkg = tortoise_cpp_amd_loader.load()
    from tortoise_cpp_amd import synth_weights as sw
    path = os.path.join(a.models, "ggml-diffusion-model.bin")
    if not os.path.exists(path):
        os.makedirs(a.models, exist_ok=True)
        sw.write_diffusion(path, seed=1235)
    eng = {}
    for m in (0, 1):
        eng[m] = e = pkg.Engine(0)
        e.set_option("conv3_fp8", m)
        e.load(diffusion=path)
    rs = np.random.RandomState(0)
    lats = [rs.randn(a.rows, 1024).astype(np.float32) * 0.5 for _ in range(a.cand)]
    T = eng[0].frames(a.rows)
    noise = [rs.randn(a.steps + 1, 100 * T).astype(np.float32) for _ in range(a.cand)]
    print("layout: %d candidates x %d latent rows (%d frames), %d steps; packed rows %s" % (a.cand, a.rows, T, a.steps, "see diffusion_last_layout"))
    times = {0: [], 1: []}
    for i in range(a.warmup + a.calls):
        for m in (0, 1):
            t0 = time.perf_counter()
            eng[m].diffusion(lats, n_steps=a.steps, noise=noise)
            if i >= a.warmup:
                times[m].append((time.perf_counter() - t0) * 1e3)
    for m in (0, 1):
        t = np.array(times[m])
        print("conv3_fp8 %d  tts_diffusion  median %9.2f ms  (min %9.2f .. max %9.2f, %d calls)  layout %s" % (m, np.median(t), t.min(), t.max(), len(t), eng[m].diffusion_last_layout()))
    fams = {0: ["diff_gemm_k3r"], 1: ["diff_conv3_f8", "diff_quant_f8", "diff_gemm_k3r"]}
    for m in (0, 1):
        e = eng[m]
        e.set_option("diff_graph", 0)
        e.prof_reset(True)
        e.diffusion(lats, n_steps=min(a.steps, 8), noise=[n[:min(a.steps, 8) + 1] for n in noise])
        for f in fams[m]:
            ms, n, work = e.prof_get(f)
            if n:
                print("conv3_fp8 %d  %-14s %5d launches  %8.1f us per launch  %7.1f %s" % (m, f, n, 1e3 * ms / n, work / ms / (1e6 if f == "diff_quant_f8" else 1e9),
                                                                                     "GB/s" if f == "diff_quant_f8" else "TFLOP/s"))
        e.prof_reset(False)
        e.set_option("diff_graph", 1)
    for e in eng.values():
        e.close()


if __name__ == "__main__":
    main()
