#!/usr/bin/env python3
"""The BigVGAN vocoder stage against UnivNet, in one process, on synthetic weights: writes profiles/bigvgan.txt.

For the base (512 channels, strides 8 8 2 2) and the large (1536 channels, strides 4 4 2 2 2 2) configuration, with 16 candidates and with one candidate of the
bench length (L = 200 latent rows: T = tts_diffusion_frames(200) mel frames each):
  - tts_bigvgan and tts_vocoder on the same mels, alternating, --calls timed calls each after --warm untimed ones: the median and min .. max of the host clock
    around the synchronous call (upload, launch sequence, download);
  - the engine profiler's device time per kernel family for one tts_bigvgan call (hfg_conv, bvg_act, bvg_post, bvg_mel) and their shares;
  - the compiler's resource summary of the three new kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/hifigan.hip, device code only).
No time is a pass condition.

  python tools/bigvgan_bench.py [--calls 7] [--warm 2] [--rows 200] [--skip-large] [--models DIR] [--out profiles/bigvgan.txt]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

pkg = tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

FAMILIES = ("hfg_conv", "bvg_act", "bvg_post", "bvg_mel")


def resources():
    """{kernel: (VGPRs, SGPRs, scratch bytes, occupancy, LDS bytes)} of the three new kernels"""
    src = os.path.join(ROOT, "tortoise.cpp_amd", "csrc", "hifigan.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.dirname(src),
                            "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "x.o")],
                           capture_output=True, text=True, timeout=900)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(bvg_\w+?_kernel)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        if "Function Name:" in line:
            cur = None
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def timed(fn, calls, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def fmt(ts):
    return "median %8.2f ms  (min %8.2f .. max %8.2f, %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--models", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "bigvgan_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigvgan.txt"))
    a = ap.parse_args()
    os.makedirs(a.models, exist_ok=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    voc = os.path.join(a.models, "ggml-vocoder-model.bin")
    if not os.path.exists(voc):
        sw.write_vocoder(voc)
    configs = [("base", sw.BIGVGAN_BASE)] + ([] if a.skip_large else [("large", sw.BIGVGAN_LARGE)])
    eng = pkg.Engine(0)
    eng.load(vocoder=voc)
    T = eng.frames(a.rows)
    say("BigVGAN vocoder stage (tts_bigvgan) against UnivNet (tts_vocoder), one process, synthetic weights, tools/bigvgan_bench.py")
    say("candidate length: L = %d latent rows = %d mel frames = %.2f s of audio; host clock around the synchronous call; the two stages alternate" % (a.rows, T, 256 * T / 24000.0))
    for name, (c0, rates) in configs:
        path = os.path.join(a.models, "ggml-bigvgan-%s.bin" % name)
        if not os.path.exists(path + ".done"):
            t0 = time.time()
            sw.write_bigvgan(path, c0, rates, seed=1260)
            open(path + ".done", "w").write("ok")
            print("wrote %s in %.0f s" % (path, time.time() - t0), flush=True)
        eng.load_bigvgan(path)
        say()
        say("== %s: C0 = %d, strides %s, %.0f MB of weights" % (name, c0, rates, os.path.getsize(path) / 1e6))
        for B in (16, 1):
            mels = [sw.bigvgan_test_mel(T, 100 + i) for i in range(B)]
            tb, tv = [], []
            for _ in range(a.warm):
                eng.bigvgan(mels); eng.vocoder(mels, noise_mode=pkg.NOISE_DEVICE)
            for _ in range(a.calls):
                tb += timed(lambda: eng.bigvgan(mels), 1, 0)
                tv += timed(lambda: eng.vocoder(mels, noise_mode=pkg.NOISE_DEVICE), 1, 0)
            say("  %2d candidates  tts_bigvgan  %s" % (B, fmt(tb)))
            say("  %2d candidates  tts_vocoder  %s   (device noise)" % (B, fmt(tv)))
            say("                  audio-seconds per second, tts_bigvgan: %.0f" % (B * 256 * T / 24000.0 / (statistics.median(tb) / 1e3)))
            eng.set_option("prof_stride", 1)
            eng.prof_reset(True)
            eng.bigvgan(mels)
            got = {f: eng.prof_get(f) for f in FAMILIES}
            eng.prof_reset(False)
            tot = sum(v[0] for v in got.values())
            say("                  profiler, one call (every launch bracketed by an event pair, which drains the pipeline: the sum exceeds the unprofiled call):")
            for f in FAMILIES:
                ms, n, work = got[f]
                rate = "%.1f TFLOP/s" % (work / ms / 1e9) if f == "hfg_conv" else "%.0f GB/s" % (work / ms / 1e6)
                say("                    %-9s %8.2f ms  %5.1f %%  %4d launches  %s" % (f, ms, 100 * ms / tot, n, rate))
    eng.close()
    say()
    say("compiler resource summary (gfx950, -O3):")
    for k, v in sorted(resources().items()):
        say("  %-16s VGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  LDS %d B/workgroup"
            % (k, v.get("VGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("Occupancy", -1), v.get("LDS Size", -1)))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
