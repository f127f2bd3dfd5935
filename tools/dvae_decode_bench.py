#!/usr/bin/env python3
"""The DVAE decoder (tts_dvae_decode: speech codes -> 80-band mel) at upstream's full size (codebook 512 x 8192, 512 -> 1024 channels, 3 ResBlocks, two k 3 /
x 2 up-sampling layers 1024 -> 1024 -> 512, 512 -> 80), on synthetic weights: writes the timing table of profiles/dvae_decoder.txt and keeps the file's
hand-kept part, from the line "ACCURACY" on (the figures the GPU tests print).

For one clip of 200 codes, 16 such clips, and 64 clips of 430 codes:
  - --calls timed calls after --warm untimed ones: the median and min .. max of the host clock around the synchronous call (upload of the codes, one launch
    sequence, download of the mel);
  - the engine profiler's device time per kernel family for one call and the rate of each over the FLOPs the stage counts. dvae_dec_up counts the
    multiplications it makes (the folded slots: 4 per input row at k 3 / x 2, where the up-sampled convolution makes 6); dvae_dec_res is hfg_conv_kernel at the
    same channel counts (1024 -> 1024, k 3 and k 1) in the same process: the yardstick the issue names for the up-sampling convolution;
  - with --resources 1 the compiler's resource summary of the new kernels; --resources 2 appends that summary alone to --out and needs no GPU.
There is no earlier implementation to compare with, and no time is a pass condition. A run without a GPU fails at Engine(0): nothing falls back.

  python tools/dvae_decode_bench.py [--calls 7] [--warm 2] [--models DIR] [--resources 0|1|2] [--out profiles/dvae_decoder.txt]"""
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

FAMILIES = ("dvae_dec_embed", "dvae_dec_res", "dvae_dec_up", "dvae_dec_head")
SHAPES = ((1, 200), (16, 200), (64, 430))


def resources():
    """{kernel instance: resource figures} of the decoder's kernels"""
    src = os.path.join(ROOT, "tortoise.cpp_amd", "csrc", "hifigan.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.dirname(src),
                            "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "x.o")],
                           capture_output=True, text=True, timeout=900)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(dvae_(?:embed|up|head|err|err_reduce)_kernel)(?:ILi(\d)E)?", line)
        if m:
            cur = m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")
            out[cur] = {}
            continue
        if "Function Name:" in line:
            cur = None
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def resource_lines():
    lines = ["", "compiler resource summary (gfx950, -O3; the LDS of dvae_up_kernel is dynamic, (128 + offsets - 1) x 33 x 4 B = 17 160 B at k 3 / x 2: the summary shows 0):"]
    for k, v in sorted(resources().items()):
        lines.append("  %-26s VGPRs %3d  AGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  static LDS %d B/workgroup"
                     % (k, v.get("VGPRs", -1), v.get("AGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("Occupancy", -1), v.get("LDS Size", -1)))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--models", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "dvae_bench"))
    ap.add_argument("--resources", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvae_decoder.txt"))
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
    path = os.path.join(a.models, "ggml-dvae-decoder-model.bin")
    if not os.path.exists(path + ".done"):
        sw.write_dvae_decoder(path, seed=1294)
        open(path + ".done", "w").write("ok")
    eng = pkg.Engine(0)
    eng.load_dvae_decoder(path)
    say("DVAE decoder (tts_dvae_decode), upstream's full size, synthetic weights, f32 throughout, tools/dvae_decode_bench.py")
    say("%.0f MB of weights; unpinned against upstream. There is no earlier implementation: no ratio is claimed." % (os.path.getsize(path) / 1e6))
    say("host clock around the synchronous call (one upload of the codes, one launch sequence, one download of the mel)")
    r = np.random.default_rng(3)
    for B, n in SHAPES:
        codes = [r.integers(0, 8192, n).astype(np.int32) for _ in range(B)]
        for _ in range(a.warm):
            eng.dvae_decode(codes)
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            eng.dvae_decode(codes)
            ts.append((time.perf_counter() - t0) * 1e3)
        say()
        say("  %2d clips of %d codes (%d mel frames each)" % (B, n, eng.dvae_decode_frames(n)))
        say("            tts_dvae_decode  median %8.2f ms  (min %8.2f .. max %8.2f, %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts)))
        eng.set_option("prof_stride", 1)
        eng.prof_reset(True)
        eng.dvae_decode(codes)
        got = {f: eng.prof_get(f) for f in FAMILIES}
        eng.prof_reset(False)
        say("            profiler, one call (every entry bracketed by an event pair, which drains the pipeline: the sum exceeds the unprofiled call):")
        for f in FAMILIES:
            ms, cnt, work = got[f]
            say("              %-15s %8.3f ms  %4d entries  %s" % (f, ms, cnt, "" if ms <= 0 else "%.1f TFLOP/s" % (work / ms / 1e9)))
    eng.close()
    if a.resources:
        for l in resource_lines():
            say(l)
    kept = open(a.out).read() if os.path.exists(a.out) else ""
    kept = kept[kept.index("\nACCURACY"):] if "\nACCURACY" in kept else ""
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
