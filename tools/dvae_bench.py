#!/usr/bin/env python3
"""The DVAE encoder (tts_dvae_codes_audio: audio -> speech codes) at upstream's full size (80 -> 512 -> 1024 channels, 3 ResBlocks, codebook 512 x 8192), on
synthetic weights: writes profiles/dvae.txt.

For one 9.2 s clip, 16 such clips, and 64 clips of 20 s (the shape of a fine-tuning dataset job), all at 22 050 Hz:
  - --calls timed calls after --warm untimed ones: the median and min .. max of the host clock around the synchronous call (upload, the audio front end's mel,
    the launch sequence, download), and audio-seconds per second;
  - the engine profiler's device time per kernel family for one call (dvae_conv, dvae_vq, and the front end's afe_mel), and the rate of each over the algorithmic
    FLOPs the stage counts: the quantiser's TFLOP/s is dvae_vq's;
  - with --resources 1 the compiler's resource summary of the new kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/hifigan.hip, device code only);
    --resources 2 appends that summary alone to --out and needs no GPU.
There is no earlier implementation to compare with, and no time is a pass condition. A run without a GPU fails at Engine(0): nothing falls back.

  python tools/dvae_bench.py [--calls 7] [--warm 2] [--models DIR] [--resources 0|1|2] [--out profiles/dvae.txt]"""
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

FAMILIES = ("dvae_conv", "dvae_vq", "afe_mel")
RATE = 22050
SHAPES = ((1, 9.2), (16, 9.2), (64, 20.0))


def flops(frames, channels=80, hidden=512, layers=2, blocks=3, dim=512, tokens=8192, k=3, stride=2):
    """(convolution FLOPs, quantiser FLOPs, codes) of one clip of `frames` mel frames, as the dvae_conv and dvae_vq families count them"""
    total, n, cin = 0.0, frames, channels
    for i in range(layers):
        n = (n - 1) // stride + 1
        total += 2.0 * n * k * cin * hidden * 2 ** i
        cin = hidden * 2 ** i
    total += 2.0 * n * (blocks * (2 * k + 1) * cin * cin + cin * dim)
    return total, 2.0 * n * dim * tokens, n


def clip(n, seed):
    r = np.random.default_rng(seed)
    i = np.arange(n)
    return (0.2 * r.standard_normal(n) + 0.3 * np.sin(i * 2 * np.pi * 220.0 / RATE) + 0.1 * np.sin(i * 2 * np.pi * 1300.0 / RATE)).astype(np.float32)


def resources():
    """{kernel: resource figures} of the DVAE's kernels"""
    src = os.path.join(ROOT, "tortoise.cpp_amd", "csrc", "hifigan.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.dirname(src),
                            "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "x.o")],
                           capture_output=True, text=True, timeout=900)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(dvae_\w+?_kernel)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        if "Function Name:" in line:
            cur = None
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def resource_lines():
    lines = ["", "compiler resource summary (gfx950, -O3; the LDS of dvae_stem_kernel and dvae_vq_kernel is dynamic: the launch asks for it, the summary shows 0):"]
    for k, v in sorted(resources().items()):
        lines.append("  %-24s VGPRs %3d  AGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  static LDS %d B/workgroup"
                     % (k, v.get("VGPRs", -1), v.get("AGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("Occupancy", -1), v.get("LDS Size", -1)))
    lines.append("  dvae_stem_kernel: 16 output rows x 256 output channels per workgroup, one channel per thread; dynamic LDS = bands x ((16 - 1) stride + taps) x 4 B"
                 " = 80 x 33 x 4 = 10 560 B at upstream's sizes")
    lines.append("  dvae_vq_kernel: 64 rows x one slab of 256 codes per workgroup (4 waves; a wave holds two 32 x 32 f32 MFMA tiles per 32-code tile and walks 2 of"
                 " the slab's 8); dynamic LDS = 64 x (dim + 1) x 4 B for the rows of z + 2 048 B for the waves' minima = 133 376 B at dim 512: one workgroup per CU")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--models", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "dvae_bench"))
    ap.add_argument("--resources", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvae.txt"))
    a = ap.parse_args()
    if a.resources == 2:
        with open(a.out, "a") as f:
            f.write("\n".join(resource_lines()) + "\n")
        return
    os.makedirs(a.models, exist_ok=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    path = os.path.join(a.models, "ggml-dvae-model.bin")
    if not os.path.exists(path + ".done"):
        sw.write_dvae(path, seed=1283)
        open(path + ".done", "w").write("ok")
    eng = pkg.Engine(0)
    eng.load_dvae(path)
    say("DVAE encoder (tts_dvae_codes_audio), upstream's full size, synthetic weights, f32 throughout, tools/dvae_bench.py")
    say("%.0f MB of weights; unpinned against upstream; nothing is claimed about code accuracy on real audio. There is no earlier implementation: no ratio is claimed."
        % (os.path.getsize(path) / 1e6))
    say("host clock around the synchronous call (one upload, the front end's mel, one launch sequence, one download)")
    for B, sec in SHAPES:
        n = int(sec * RATE)
        frames = n // 256 + 1
        conv, vq, codes = flops(frames)
        clips = [clip(n, 50 + i) for i in range(B)]
        for _ in range(a.warm):
            eng.dvae_codes_audio(clips, RATE)
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            eng.dvae_codes_audio(clips, RATE)
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        say()
        say("  %2d clips of %.1f s (%d samples, %d mel frames, %d codes each; convolutions %.2f GFLOP, quantiser %.2f GFLOP per clip)" % (B, sec, n, frames, codes, conv / 1e9, vq / 1e9))
        say("            tts_dvae_codes_audio  median %8.2f ms  (min %8.2f .. max %8.2f, %d calls)   %.0f audio-seconds per second over the whole call"
            % (med, min(ts), max(ts), len(ts), B * sec / (med / 1e3)))
        eng.set_option("prof_stride", 1)
        eng.prof_reset(True)
        eng.dvae_codes_audio(clips, RATE)
        got = {f: eng.prof_get(f) for f in FAMILIES}
        eng.prof_reset(False)
        say("            profiler, one call (every entry bracketed by an event pair, which drains the pipeline: the sum exceeds the unprofiled call):")
        for f in FAMILIES:
            ms, cnt, work = got[f]
            rate = "" if f == "afe_mel" or ms <= 0 else "%.1f TFLOP/s" % (work / ms / 1e9)
            say("              %-9s %8.3f ms  %4d entries  %s" % (f, ms, cnt, rate))
    eng.close()
    if a.resources:
        for l in resource_lines():
            say(l)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
