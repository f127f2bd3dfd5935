#!/usr/bin/env python3
"""What the autoregressive sampler's controls cost per decode step.

Workload: full-size synthetic AR weights (30 layers, the benchmark's seed), 16 candidates, 192 decode steps with the stop token masked, through
tts_autoregressive without the latent pass. A measurement is the wall time of a 194-code call minus that of a 2-code call (begin + prompt pass + one decode
step, the fastest of three: the first of them captures the step graph) over 192: decode step + list transfer + host tail, what a caller waits for. The configurations are measured interleaved, --repeat times each:

  default   penalty scope 0, the reference's literals (what the parent commit runs)
  scope1    ar_penalty_scope = 1: history bitmap on the device, penalising prefilter
  topk100   ar_top_k = 100: the widest keep window (114 .. 128)
  typ09     ar_typical_mass = 0.9: the typical body in the prefilter (sample_prefilter_typical_kernel), a large typical set
  typ02     ar_typical_mass = 0.2: the same, a small set

--prefilter adds, per configuration, the prefilter kernel's own time: one more 34-code call with the "ar_prefilter" family profiled (the step then runs
eagerly between event pairs; that call is not part of the step timing), reported as microseconds per launch.

--lib PATH loads another build of libtortoise_mi355x.so through the C ABI (e.g. the parent commit's, which only knows `default`), so that branch and parent
can be run alternately on one box:  for i in 1 2 3; do ar_sampler_bench.py --lib <parent .so> --configs default --repeat 1; ar_sampler_bench.py --repeat 1; done
One JSON line per run."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = {"default": {}, "scope1": {"ar_penalty_scope": 1}, "topk100": {"ar_top_k": 100}, "typ09": {"ar_typical_mass": 0.9},
           "typ02": {"ar_typical_mass": 0.2}}
RESET = {"ar_penalty_scope": 0, "ar_top_k": 50, "ar_typical_mass": 0}
TOKENS = np.array([255, 147, 2, 54, 2, 14, 2, 136, 63, 2, 80, 32, 150, 112, 9, 0], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "tortoise.cpp_amd", "libtortoise_mi355x.so"))
    ap.add_argument("--models", default=os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"))
    ap.add_argument("--configs", default="default,scope1,topk100")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--steps", type=int, default=192)
    ap.add_argument("--prefilter", action="store_true")
    a = ap.parse_args()
    ar_path = os.path.join(a.models, "ggml-model.bin")
    if not os.path.exists(ar_path):  # only the AR file is needed here; bench.py's own stamp stays untouched
        import tortoise_cpp_amd_loader
        tortoise_cpp_amd_loader.load()
        from tortoise_cpp_amd import synth_weights as sw
        os.makedirs(a.models, exist_ok=True)
        sw.write_ar(ar_path, 30, 1234)
    L = C.CDLL(a.lib)
    L.tts_create.restype = C.c_void_p
    L.tts_last_error.restype = C.c_char_p
    vp = C.c_void_p
    L.tts_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    L.tts_load_ar.argtypes = [vp, C.c_char_p]
    L.tts_seed.argtypes = [vp, C.c_uint32]
    L.tts_destroy.argtypes = [vp]
    L.tts_last_error.argtypes = [vp]
    L.tts_ar_topk_fallbacks.argtypes = [vp]
    L.tts_autoregressive.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint, vp, vp, vp, vp]
    L.tts_prof_reset.argtypes = [vp, C.c_int]
    L.tts_prof_get.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    h = L.tts_create(0)
    if not h:
        sys.exit("tts_create(0) failed: no HIP device")

    def ck(rc):
        if rc < 0:
            sys.exit("%s (status %d)" % (L.tts_last_error(h).decode(), rc))

    ck(L.tts_load_ar(h, ar_path.encode()))
    voice = np.fromfile(os.path.join(ROOT, "models", "mol.bin"), np.float32)[:1024].copy()
    B = a.candidates
    codes, rows, steps = np.empty((B, 502), np.int32), np.empty(B, np.int32), np.zeros(1, np.int32)

    def run(n_codes):
        L.tts_seed(h, 7)
        t0 = time.perf_counter()
        ck(L.tts_autoregressive(h, TOKENS.ctypes.data, len(TOKENS), voice.ctypes.data, B, n_codes, 1, codes.ctypes.data, rows.ctypes.data, None, steps.ctypes.data))
        return (time.perf_counter() - t0) * 1e3

    names = a.configs.split(",")
    res = {n: [] for n in names}
    fallbacks, prefilter_us = {}, {}
    for rep in range(a.repeat + 1):  # round 0 warms up: graph capture, pinned buffers, the sampler pool
        for n in names:
            if names != ["default"]:  # (a build that only knows `default` is never asked for an option)
                for k, v in {**RESET, **CONFIGS[n]}.items():
                    ck(L.tts_set_option(h, k.encode(), float(v)))
            base = min(run(2) for _ in range(3))
            full = run(a.steps + 2)
            fallbacks[n] = L.tts_ar_topk_fallbacks(h)
            if rep:
                res[n].append((full - base) / a.steps)
            if a.prefilter and rep == a.repeat:
                ck(L.tts_set_option(h, b"prof_only:ar_prefilter", 1.0))
                ck(L.tts_prof_reset(h, 1))
                run(34)
                ms, launches = C.c_double(0), C.c_int64(0)
                ck(L.tts_prof_get(h, b"ar_prefilter", C.byref(ms), C.byref(launches), None))
                ck(L.tts_prof_reset(h, 0))
                ck(L.tts_set_option(h, b"prof_only:ar_prefilter", 0.0))
                prefilter_us[n] = round(1e3 * ms.value / max(1, launches.value), 2)
    L.tts_destroy(h)
    print(json.dumps({"lib": os.path.relpath(a.lib, ROOT), "candidates": B, "steps": a.steps,
                      "ms_per_step": {n: [round(x, 4) for x in v] for n, v in res.items()}, "topk_fallbacks": fallbacks,
                      **({"prefilter_us_per_launch": prefilter_us} if a.prefilter else {})}))


if __name__ == "__main__":
    main()
