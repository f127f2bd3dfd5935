#!/usr/bin/env python3
"""Whole-call times of tts_diffusion at the two ends of the single call's range, for comparing two builds of the library (profiles/diff_step_refactor.txt; the
build is selected with TTS_LIB_PATH). Full-size synthetic diffusion weights, 80 ancestral steps, host clock around the synchronous call, the median of --calls
calls after --warm warm-ups:
  hoisted8     eight utterances of the most latent rows whose packed layout is still hoisted (HOIST_MAX_ROWS = 16384 rows), device noise
  ref1         one utterance of 200 latent rows, TTS_NOISE_REFERENCE: the host draw pipelined beside the device loop
  latency1     the same utterance, device noise, latency_mode 1
Prints one line: "hoisted8 <ms> ref1 <ms> latency1 <ms>".

  python tools/diff_step_bench.py [--calls 5] [--warm 2] [--models DIR]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

HOIST_MAX_ROWS = 16384


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--models", default=os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"))
    a = ap.parse_args()
    pkg = tortoise_cpp_amd_loader.load()
    from tortoise_cpp_amd import synth_weights as sw
    os.makedirs(a.models, exist_ok=True)
    path = os.path.join(a.models, "ggml-diffusion-model.bin")
    if not os.path.exists(path):
        sw.write_diffusion(path, 10, 3, 3, 4, 1235)
    e = pkg.Engine(0)
    e.load(diffusion=path)
    rs = np.random.RandomState(5)
    L8 = max(L for L in range(1, 501) if pkg.host_diff_packed_rows([L] * 8) <= HOIST_MAX_ROWS)
    many = [rs.randn(L8, 1024).astype(np.float32) for _ in range(8)]
    one = [rs.randn(200, 1024).astype(np.float32)]

    def timed(lats, mode, **opts):
        for k, v in opts.items():
            e.set_option(k, v)
        ms = []
        for _ in range(a.warm + a.calls):
            e.seed(3)
            t0 = time.perf_counter()
            e.diffusion(lats, n_steps=80, noise=None, noise_mode=mode)
            ms.append(1e3 * (time.perf_counter() - t0))
        for k in opts:
            e.set_option(k, 0)
        return statistics.median(ms[a.warm:])

    cols = [("hoisted8", timed(many, pkg.NOISE_DEVICE)), ("ref1", timed(one, pkg.NOISE_REFERENCE)), ("latency1", timed(one, pkg.NOISE_DEVICE, latency_mode=1))]
    e.close()
    print(" ".join("%s %.2f" % c for c in cols), "(8 x %d latent rows = %d packed rows)" % (L8, pkg.host_diff_packed_rows([L8] * 8)), flush=True)


if __name__ == "__main__":
    main()
