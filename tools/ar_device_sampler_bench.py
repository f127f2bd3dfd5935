#!/usr/bin/env python3
"""Decode-step time of the AR stage under the host sampler (ar_sampler 0) and the device sampler (ar_sampler 1 at ar_sync_steps 1 and 8), and the two sampler
kernels alone (profiler families ar_prefilter / ar_sample). Full-size synthetic weights, B = 1 and 16, 200 steps, 7 calls per configuration after one warm-up
call; every figure is printed as min / median / max of the 7. --parent-tree <a built checkout of the parent commit> adds that build at ar_sampler 0 to the
same run. Each build runs in a child process of its own (the package is chosen at import), one after the other.

    python tools/ar_device_sampler_bench.py [--parent-tree DIR] [--steps 200] [--calls 7] > profiles/ar_device_sampler.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("ar_sampler 0", 0, 1), ("ar_sampler 1, ar_sync_steps 1", 1, 1), ("ar_sampler 1, ar_sync_steps 8", 1, 8)]


def child(args):
    sys.path.insert(0, args.root or ROOT)
    import tortoise_cpp_amd_loader
    pkg = tortoise_cpp_amd_loader.load()
    from tortoise_cpp_amd import synth_weights as sw
    path = os.path.join(os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"), "ggml-model.bin")
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        sw.write_ar(path, n_layers=30, seed=1234)
    voice = np.fromfile(os.path.join(ROOT, "models", "mol.bin"), np.float32)
    toks = np.array([255, 147, 2, 54, 2, 14, 2, 136, 63, 2, 80, 32, 150, 112, 9, 0], np.int32)
    eng = pkg.Engine(0)
    eng.load(ar=path)
    out = []
    for name, sampler, sync in CONFIGS[:1] if args.only_host else CONFIGS:
        if sampler:
            eng.set_option("ar_sampler", sampler)
            eng.set_option("ar_sync_steps", sync)
        for B in (1, 16):
            ms = []
            for call in range(args.calls + 1):  # the first call captures the graph: not timed
                eng.seed(call)
                t0 = time.perf_counter()
                steps = eng.autoregressive(toks, voice, B, args.steps, mask_stop=True, want_latents=False)[3]
                ms.append((time.perf_counter() - t0) * 1e3 / steps)
            out.append(dict(config=name, B=B, ms_per_step=sorted(ms[1:])))
    for fam, sampler in ([("ar_prefilter", 0)] if args.only_host else [("ar_prefilter", 0), ("ar_sample", 1)]):  # the kernels alone: event pairs around every launch
        if not args.only_host:
            eng.set_option("ar_sampler", sampler)
        eng.set_option("prof_only:" + fam, 1)
        for B in (1, 16):
            us = []
            for call in range(args.calls):
                eng.prof_reset(True)
                eng.autoregressive(toks, voice, B, 50, mask_stop=True, want_latents=False)
                t, n, _ = eng.prof_get(fam)
                us.append(1e3 * t / max(n, 1))
            out.append(dict(config=fam + " kernel alone", B=B, us_per_launch=sorted(us)))
        eng.prof_reset(False)
        eng.set_option("prof_only:" + fam, 0)
    eng.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--root")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only-host", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    builds = [("this build", None)] + ([("parent build", args.parent_tree)] if args.parent_tree else [])
    print("decode step of the AR stage, full-size synthetic weights, %d steps, %d calls each: min / median / max" % (args.steps, args.calls))
    for label, tree in builds:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--calls", str(args.calls)]
        if tree:
            cmd += ["--only-host", "--root", os.path.abspath(tree)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in r.stdout.split("\n") if l.startswith("RESULT ")]
        if r.returncode or not line:
            sys.exit("%s failed:\n%s%s" % (label, r.stdout, r.stderr))
        for e in json.loads(line[0][7:]):
            v, unit = (e["ms_per_step"], "ms / step") if "ms_per_step" in e else (e["us_per_launch"], "us / launch")
            print("%-13s %-32s B %2d   %8.3f / %8.3f / %8.3f %s" % (label, e["config"], e["B"], v[0], v[len(v) // 2], v[-1], unit))


if __name__ == "__main__":
    main()
