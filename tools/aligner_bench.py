#!/usr/bin/env python3
"""The wav2vec2 CTC aligner (tts_aligner_ids) at upstream's full size (7 convolution layers of 512 channels, dimension 1024, 24 encoder layers, K = 128 in 16
groups), on synthetic weights: writes profiles/aligner.txt.

For 1 clip and for 16 clips of 147 200 samples at 16 kHz (9.2 s each):
  - --calls timed calls after --warm untimed ones: the median and min .. max of the host clock around the synchronous call (upload, launch sequence, download);
  - the engine profiler's device time per kernel family for one call (w2v_conv, w2v_attn, w2v_row), their shares, and the rate of the convolutions and Linears
    over the algorithmic FLOPs the stage counts, beside the classifier's cls_conv figure measured in the same process;
  - with --resources 1 the compiler's resource summary of the new kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/hifigan.hip, device code only).
There is no earlier implementation to compare with, and no time is a pass condition. A run without a GPU fails at Engine(0): nothing falls back.

  python tools/aligner_bench.py [--calls 7] [--warm 2] [--models DIR] [--resources 0|1] [--out profiles/aligner.txt]"""
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

FAMILIES = ("w2v_conv", "w2v_attn", "w2v_row")
N = 147200


def flops(n, N=7, C=512, k=(), s=(), D=1024, K=128, G=16, depth=24, FF=4096, V=32, **_):
    """(convolution + Linear FLOPs, attention FLOPs, frames) of one clip of n samples, as the w2v_conv and w2v_attn families count them"""
    total = 0.0
    for i in range(N):
        n = (n - k[i]) // s[i] + 1
        total += 2.0 * n * k[i] * (C if i else 1) * C
    total += 2.0 * n * (C * D + K * (D // G) * D + depth * (4 * D * D + 2 * D * FF) + D * V)
    return total, depth * 4.0 * n * n * D, n


def resources():
    """{kernel: resource figures} of the aligner's kernels"""
    src = os.path.join(ROOT, "tortoise.cpp_amd", "csrc", "hifigan.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.dirname(src),
                            "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "x.o")],
                           capture_output=True, text=True, timeout=900)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(w2v_\w+?_kernel)", line)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--models", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "aligner_bench"))
    ap.add_argument("--resources", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligner.txt"))
    a = ap.parse_args()
    os.makedirs(a.models, exist_ok=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    path, cpath = os.path.join(a.models, "ggml-aligner-model.bin"), os.path.join(a.models, "ggml-classifier-model.bin")
    if not os.path.exists(path + ".done"):
        sw.write_aligner(path, seed=1273)
        open(path + ".done", "w").write("ok")
    if not os.path.exists(cpath + ".done"):
        sw.write_classifier(cpath, seed=1262)
        open(cpath + ".done", "w").write("ok")
    eng = pkg.Engine(0)
    eng.load_aligner(path)
    lin, att, frames = flops(N, **sw.ALIGNER_UPSTREAM)
    say("wav2vec2 CTC aligner (tts_aligner_ids), upstream's full size, synthetic weights, f32 throughout, tools/aligner_bench.py")
    say("clip: %d samples at 16 kHz = %.2f s = %d frames; convolutions and Linears %.1f GFLOP per clip, attention %.2f GFLOP; %.0f MB of weights; unpinned against "
        "upstream, nothing is claimed about alignment quality" % (N, N / 16000.0, frames, lin / 1e9, att / 1e9, os.path.getsize(path) / 1e6))
    say("host clock around the synchronous call (one upload, one launch sequence, one download)")
    for B in (1, 16):
        clips = [sw.aligner_test_wave(N, 50 + i) for i in range(B)]
        for _ in range(a.warm):
            eng.aligner_ids(clips, 16000)
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            eng.aligner_ids(clips, 16000)
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        say()
        say("  %2d clips  tts_aligner_ids  median %8.2f ms  (min %8.2f .. max %8.2f, %d calls)   %.0f audio-seconds per second, %.1f TFLOP/s of convolutions and Linears over the whole call"
            % (B, med, min(ts), max(ts), len(ts), B * N / 16000.0 / (med / 1e3), B * lin / med / 1e9))
        eng.set_option("prof_stride", 1)
        eng.prof_reset(True)
        eng.aligner_ids(clips, 16000)
        got = {f: eng.prof_get(f) for f in FAMILIES}
        eng.prof_reset(False)
        tot = sum(v[0] for v in got.values())
        say("            profiler, one call (every entry bracketed by an event pair, which drains the pipeline: the sum exceeds the unprofiled call):")
        for f in FAMILIES:
            ms, n, work = got[f]
            rate = "%.0f GB/s" % (work / ms / 1e6) if f == "w2v_row" else "%.1f TFLOP/s" % (work / ms / 1e9)
            say("              %-9s %8.2f ms  %5.1f %%  %4d entries  %s" % (f, ms, 100 * ms / tot, n, rate))
    # the classifier's convolutions in the same process: the figure the reused kernels reach on their own stage
    eng.load_classifier(cpath)
    clips = [sw.classifier_test_wave(sw.CLASSIFIER_MAX_SAMPLES, 50 + i) for i in range(16)]
    for _ in range(a.warm):
        eng.classify_audio(clips, 24000)
    eng.set_option("prof_stride", 1)
    eng.prof_reset(True)
    eng.classify_audio(clips, 24000)
    ms, n, work = eng.prof_get("cls_conv")
    eng.prof_reset(False)
    say()
    say("beside it, same process: the classifier's cls_conv family on 16 clips of 220 000 samples: %.2f ms, %d entries, %.1f TFLOP/s" % (ms, n, work / ms / 1e9))
    eng.close()
    if a.resources:
        say()
        say("compiler resource summary (gfx950, -O3):")
        for k, v in sorted(resources().items()):
            say("  %-24s VGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  LDS %d B/workgroup"
                % (k, v.get("VGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("Occupancy", -1), v.get("LDS Size", -1)))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
