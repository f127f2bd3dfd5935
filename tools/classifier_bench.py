#!/usr/bin/env python3
"""The synthesized-speech classifier (tts_classify_audio) under upstream's configuration, on synthetic weights: writes profiles/classifier.txt.

For 1 clip and for 16 clips of 220 000 samples at 24 kHz (9.17 s each, the crop):
  - --calls timed calls after --warm untimed ones: the median and min .. max of the host clock around the synchronous call (upload, launch sequence, download);
  - the engine profiler's device time per kernel family for one call (cls_conv, cls_gn, cls_attn), their shares, and the convolutions' rate over the algorithmic
    FLOPs the stage counts (2 x rows x taps x cin x cout per launch);
  - the compiler's resource summary of the new kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/hifigan.hip, device code only).
There is no earlier implementation to compare with, and no time is a pass condition. A run without a GPU fails at Engine(0): nothing falls back.

  python tools/classifier_bench.py [--calls 7] [--warm 2] [--models DIR] [--out profiles/classifier.txt]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

pkg = tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

FAMILIES = ("cls_conv", "cls_gn", "cls_attn")
N = sw.CLASSIFIER_MAX_SAMPLES


def conv_flops(n, b0=32, depth=5, K=5, E=512, rb=2, attn=4, F=4, **_):
    """algorithmic FLOPs of the convolutions of one clip of n samples, as the cls_conv family counts them (rows padded to 8 aside)"""
    total = 2.0 * n * 3 * b0
    for l in range(depth):
        C = b0 << l
        total += 2.0 * n * K * C * C * 2 * rb
        n = (n - 1) // F + 1
        total += 2.0 * n * 5 * C * 2 * C
    return total + 2.0 * n * (b0 << depth) * E


def resources():
    """{kernel: resource figures} of the classifier's kernels"""
    src = os.path.join(ROOT, "tortoise.cpp_amd", "csrc", "hifigan.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.dirname(src),
                            "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "x.o")],
                           capture_output=True, text=True, timeout=900)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(cls_\w+?_kernel(?:ILi\d+E)?)", line)
        if m:
            cur = m.group(1).replace("ILi", "<").replace("E", ">") if "ILi" in m.group(1) else m.group(1)
            out[cur] = {}
            continue
        if "Function Name:" in line:
            cur = None
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--models", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "classifier_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classifier.txt"))
    a = ap.parse_args()
    os.makedirs(a.models, exist_ok=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    path = os.path.join(a.models, "ggml-classifier-model.bin")
    if not os.path.exists(path + ".done"):
        sw.write_classifier(path, seed=1262)
        open(path + ".done", "w").write("ok")
    eng = pkg.Engine(0)
    eng.load_classifier(path)
    per_clip = conv_flops(N, **sw.CLASSIFIER_UPSTREAM)
    say("Synthesized-speech classifier (tts_classify_audio), upstream's configuration, synthetic weights, tools/classifier_bench.py")
    say("clip: %d samples at 24 kHz = %.2f s = %d positions in the attention blocks; convolutions %.1f GFLOP per clip; %.0f MB of weights; unpinned against upstream, "
        "unjudged on real audio" % (N, N / 24000.0, eng.classifier_positions(N), per_clip / 1e9, os.path.getsize(path) / 1e6))
    say("host clock around the synchronous call (one upload, one launch sequence, one download)")
    for B in (1, 16):
        clips = [sw.classifier_test_wave(N, 50 + i) for i in range(B)]
        for _ in range(a.warm):
            eng.classify_audio(clips, 24000)
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            eng.classify_audio(clips, 24000)
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        say()
        say("  %2d clips  tts_classify_audio  median %8.2f ms  (min %8.2f .. max %8.2f, %d calls)   %.0f audio-seconds per second, %.1f TFLOP/s of convolutions over the whole call"
            % (B, med, min(ts), max(ts), len(ts), B * N / 24000.0 / (med / 1e3), B * per_clip / med / 1e9))
        eng.set_option("prof_stride", 1)
        eng.prof_reset(True)
        eng.classify_audio(clips, 24000)
        got = {f: eng.prof_get(f) for f in FAMILIES}
        eng.prof_reset(False)
        tot = sum(v[0] for v in got.values())
        say("            profiler, one call (every entry bracketed by an event pair, which drains the pipeline: the sum exceeds the unprofiled call):")
        for f in FAMILIES:
            ms, n, work = got[f]
            rate = "%.0f GB/s" % (work / ms / 1e6) if f == "cls_gn" else "%.1f TFLOP/s" % (work / ms / 1e9)
            say("              %-9s %8.2f ms  %5.1f %%  %4d entries  %s" % (f, ms, 100 * ms / tot, n, rate))
    eng.close()
    say()
    say("compiler resource summary (gfx950, -O3):")
    for k, v in sorted(resources().items()):
        say("  %-24s VGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  LDS %d B/workgroup"
            % (k, v.get("VGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("Occupancy", -1), v.get("LDS Size", -1)))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
