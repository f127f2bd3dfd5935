#!/usr/bin/env python3
"""The wav2vec2 CTC aligner (tts_aligner_ids) at upstream's full size (7 convolution layers of 512 channels, dimension 1024, 24 encoder layers, K = 128 in 16
groups), on synthetic weights: writes profiles/aligner.txt.

For 1 clip and for 16 clips of 147 200 samples at 16 kHz (9.2 s each):
  - --calls timed calls after --warm untimed ones: the median and min .. max of the host clock around the synchronous call (upload, launch sequence, download);
  - the engine profiler's device time per kernel family for one call (w2v_conv, w2v_attn, w2v_row), their shares, and the rate of the convolutions and Linears
    over the algorithmic FLOPs the stage counts, beside the classifier's cls_conv figure measured in the same process;
  - with --resources 1 the compiler's resource summary of the new kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/hifigan.hip, device code only).
There is no earlier implementation to compare with, and no time is a pass condition. A run without a GPU fails at Engine(0): nothing falls back.

--precision M[,M..]: instead, option aligner_precision at each listed value (0 f32, 1 fp16, 2 split fp16 pairs; csrc/w2v_linear_h.h) in ONE process: one engine
per mode (the option is read at the load), the modes interleaved call by call, --calls timed calls each after --warm; the w2v_conv family's device time and
TFLOP/s per mode; every mode's largest logit distance from the float64 restatement (synth_weights.aligner_forward) on a --distance-samples clip at full size; the
resource summary of w2v_linear_h_kernel. Writes profiles/aligner_f16.txt.

--attn M[,M..]: instead, option addon_attn_precision at each listed value (0 f32 cls_attn_kernel, 1 fp16, 2 split fp16 pairs; csrc/addon_attn_h.h) on ONE engine
loaded with aligner_precision 2 (the option is read at call time), the modes interleaved call by call; the w2v_attn family's device time per mode; every mode's
largest logit distance from float64. Printed, and written where --out names a file (profiles/addon_attn.txt holds it beside the classifier's).

--conv-precision M[,M..]: instead, option addon_conv_precision at each listed value (0 f32 cls_down_kernel, 1 fp16, 2 split fp16 pairs; csrc/cls_down_h.h) in ONE
process: one engine per value, each loaded with it and with aligner_precision 2, and called with addon_attn_precision 2, so the extractor is what moves; the
values interleaved call by call; the w2v_conv family's device time per value; every value's largest logit distance from float64. Printed, and written where
--out names a file (profiles/addon_conv.txt holds it beside the classifier's).

  python tools/aligner_bench.py [--calls 7] [--warm 2] [--models DIR] [--resources 0|1] [--precision 0,1,2] [--attn 0,1,2] [--conv-precision 0,1,2] [--out FILE]"""
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
    """{kernel: resource figures} of the aligner's kernels (a template's instantiations: the largest of each figure, the smallest occupancy)"""
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
            out.setdefault(cur, {})
            continue
        if "Function Name:" in line:
            cur = None
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            key, val = m.group(1).split(" [")[0], int(m.group(2))
            out[cur][key] = (min if key == "Occupancy" else max)(out[cur].get(key, val), val)
    return out


def precision(a, modes, path, say):
    import numpy as np
    lin, att, frames = flops(N, **sw.ALIGNER_UPSTREAM)
    engs = {}
    for m in modes:
        engs[m] = pkg.Engine(0)
        engs[m].set_option("aligner_precision", m)
        engs[m].load_aligner(path)
    say("wav2vec2 CTC aligner (tts_aligner_ids), upstream's full size, synthetic weights: option aligner_precision 0 (f32, hfg_conv_kernel) | 1 (fp16 operands) | "
        "2 (fp16 hi + lo pairs), csrc/w2v_linear_h.h; tools/aligner_bench.py --precision %s" % ",".join(map(str, modes)))
    say("clip: %d samples at 16 kHz = %d frames; one engine per mode in one process, the modes interleaved call by call, %d timed calls each after %d untimed; "
        "host clock around the synchronous call" % (N, frames, a.calls, a.warm))
    for B in (1, 16):
        clips = [sw.aligner_test_wave(N, 50 + i) for i in range(B)]
        ts = {m: [] for m in modes}
        for i in range(a.warm + a.calls):
            for m in modes:
                t0 = time.perf_counter()
                engs[m].aligner_ids(clips, 16000)
                if i >= a.warm:
                    ts[m].append((time.perf_counter() - t0) * 1e3)
        say()
        for m in modes:
            say("  %2d clips  aligner_precision %d  tts_aligner_ids  median %8.2f ms  (min %8.2f .. max %8.2f, %d calls)"
                % (B, m, statistics.median(ts[m]), min(ts[m]), max(ts[m]), len(ts[m])))
        for m in modes:
            engs[m].set_option("prof_stride", 1)
            engs[m].prof_reset(True)
            engs[m].aligner_ids(clips, 16000)
            ms, n, work = engs[m].prof_get("w2v_conv")
            engs[m].prof_reset(False)
            say("  %2d clips  aligner_precision %d  w2v_conv %8.2f ms on the device, %4d entries, %.1f TFLOP/s" % (B, m, ms, n, work / ms / 1e9))
    wave = sw.aligner_test_wave(a.distance_samples, 77)
    want = sw.aligner_forward(sw.read_ggml(path), wave, np.float64)
    say()
    say("largest logit distance from float64 (synth_weights.aligner_forward) on a clip of %d samples (%d frames), logits up to %.1f, smallest top-two margin %.4f:"
        % (len(wave), want.shape[0], np.abs(want).max(), np.diff(np.sort(want, axis=1)[:, -2:], axis=1).min()))
    for m in modes:
        ids, lg = engs[m].aligner_ids([wave], 16000, logits=True)
        say("  aligner_precision %d  %.2e   ids that differ from the float64 argmax: %d of %d" % (m, np.abs(lg[0] - want).max(), int((ids[0] != want.argmax(1)).sum()), len(ids[0])))
    for e in engs.values():
        e.close()
    if a.resources:
        say()
        say("compiler resource summary (gfx950, -O3; the largest of the kernel's instantiations):")
        for k, v in sorted(resources().items()):
            if k == "w2v_linear_h_kernel":
                say("  %-24s VGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  LDS %d B/workgroup"
                    % (k, v.get("VGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("Occupancy", -1), v.get("LDS Size", -1)))


def attention(a, modes, path, say):
    """option addon_attn_precision (read at call time) on ONE engine loaded with aligner_precision 2: the modes interleaved call by call"""
    import numpy as np
    lin, att, frames = flops(N, **sw.ALIGNER_UPSTREAM)
    eng = pkg.Engine(0)
    eng.set_option("aligner_precision", 2)
    eng.load_aligner(path)
    say("wav2vec2 CTC aligner (tts_aligner_ids), upstream's full size, synthetic weights, aligner_precision 2: option addon_attn_precision 0 (f32, cls_attn_kernel) | "
        "1 (fp16 operands) | 2 (fp16 hi + lo pairs), csrc/addon_attn_h.h; tools/aligner_bench.py --attn %s" % ",".join(map(str, modes)))
    say("clip: %d samples at 16 kHz = %d frames, attention %.2f GFLOP per clip; one engine, the modes interleaved call by call, %d timed calls each after %d untimed; "
        "host clock around the synchronous call" % (N, frames, att / 1e9, a.calls, a.warm))
    for B in (1, 16):
        clips = [sw.aligner_test_wave(N, 50 + i) for i in range(B)]
        ts = {m: [] for m in modes}
        for i in range(a.warm + a.calls):
            for m in modes:
                eng.set_option("addon_attn_precision", m)
                t0 = time.perf_counter()
                eng.aligner_ids(clips, 16000)
                if i >= a.warm:
                    ts[m].append((time.perf_counter() - t0) * 1e3)
        say()
        for m in modes:
            say("  %2d clips  addon_attn_precision %d  tts_aligner_ids  median %8.2f ms  (min %8.2f .. max %8.2f, %d calls)"
                % (B, m, statistics.median(ts[m]), min(ts[m]), max(ts[m]), len(ts[m])))
        eng.set_option("prof_stride", 1)
        for m in modes:
            eng.set_option("addon_attn_precision", m)
            eng.prof_reset(True)
            eng.aligner_ids(clips, 16000)
            ms, n, work = eng.prof_get("w2v_attn")
            eng.prof_reset(False)
            say("  %2d clips  addon_attn_precision %d  w2v_attn %8.2f ms on the device, %4d entries, %.1f TFLOP/s" % (B, m, ms, n, work / ms / 1e9))
    wave = sw.aligner_test_wave(a.distance_samples, 77)
    want = sw.aligner_forward(sw.read_ggml(path), wave, np.float64)
    say()
    say("largest logit distance from float64 (synth_weights.aligner_forward) on a clip of %d samples (%d frames), logits up to %.1f, smallest top-two margin %.4f:"
        % (len(wave), want.shape[0], np.abs(want).max(), np.diff(np.sort(want, axis=1)[:, -2:], axis=1).min()))
    for m in modes:
        eng.set_option("addon_attn_precision", m)
        ids, lg = eng.aligner_ids([wave], 16000, logits=True)
        say("  addon_attn_precision %d  %.2e   ids that differ from the float64 argmax: %d of %d" % (m, np.abs(lg[0] - want).max(), int((ids[0] != want.argmax(1)).sum()), len(ids[0])))
    eng.close()


def convolutions(a, modes, path, say):
    """option addon_conv_precision: one engine per value, each loaded with it and aligner_precision 2 and called with addon_attn_precision 2"""
    import numpy as np
    lin, att, frames = flops(N, **sw.ALIGNER_UPSTREAM)
    engs = {}
    for m in modes:
        engs[m] = pkg.Engine(0)
        engs[m].set_option("aligner_precision", 2)
        engs[m].set_option("addon_attn_precision", 2)
        engs[m].set_option("addon_conv_precision", m)
        engs[m].load_aligner(path)
    say("wav2vec2 CTC aligner (tts_aligner_ids), upstream's full size, synthetic weights, aligner_precision 2 and addon_attn_precision 2: option addon_conv_precision "
        "0 (f32, cls_down_kernel) | 1 (fp16 operands) | 2 (fp16 hi + lo pairs), csrc/cls_down_h.h; tools/aligner_bench.py --conv-precision %s" % ",".join(map(str, modes)))
    say("clip: %d samples at 16 kHz = %d frames; one engine per value in one process, the values interleaved call by call, %d timed calls each after %d untimed; "
        "host clock around the synchronous call" % (N, frames, a.calls, a.warm))
    for B in (1, 16):
        clips = [sw.aligner_test_wave(N, 50 + i) for i in range(B)]
        ts = {m: [] for m in modes}
        for i in range(a.warm + a.calls):
            for m in modes:
                t0 = time.perf_counter()
                engs[m].aligner_ids(clips, 16000)
                if i >= a.warm:
                    ts[m].append((time.perf_counter() - t0) * 1e3)
        say()
        for m in modes:
            say("  %2d clips  addon_conv_precision %d  tts_aligner_ids  median %8.2f ms  (min %8.2f .. max %8.2f, %d calls)"
                % (B, m, statistics.median(ts[m]), min(ts[m]), max(ts[m]), len(ts[m])))
        for m in modes:
            engs[m].set_option("prof_stride", 1)
            engs[m].prof_reset(True)
            engs[m].aligner_ids(clips, 16000)
            ms, n, work = engs[m].prof_get("w2v_conv")
            engs[m].prof_reset(False)
            say("  %2d clips  addon_conv_precision %d  w2v_conv (stem, extractor, Linears, positional convolution, head) %8.2f ms on the device, %4d entries" % (B, m, ms, n))
    wave = sw.aligner_test_wave(a.distance_samples, 77)
    want = sw.aligner_forward(sw.read_ggml(path), wave, np.float64)
    say()
    say("largest logit distance from float64 (synth_weights.aligner_forward) on a clip of %d samples (%d frames), logits up to %.1f, smallest top-two margin %.4f:"
        % (len(wave), want.shape[0], np.abs(want).max(), np.diff(np.sort(want, axis=1)[:, -2:], axis=1).min()))
    for m in modes:
        ids, lg = engs[m].aligner_ids([wave], 16000, logits=True)
        say("  addon_conv_precision %d  %.2e   ids that differ from the float64 argmax: %d of %d" % (m, np.abs(lg[0] - want).max(), int((ids[0] != want.argmax(1)).sum()), len(ids[0])))
    for e in engs.values():
        e.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--models", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "aligner_bench"))
    ap.add_argument("--resources", type=int, default=1)
    ap.add_argument("--precision", default="")
    ap.add_argument("--attn", default="")
    ap.add_argument("--conv-precision", default="")
    ap.add_argument("--distance-samples", type=int, default=32000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not a.attn and not a.conv_precision:
        a.out = a.out or os.path.join(ROOT, "profiles", "aligner_f16.txt" if a.precision else "aligner.txt")
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
    if a.conv_precision:  # printed; written only where --out names a file (profiles/addon_conv.txt is put together from this and tools/classifier_bench.py --conv-precision)
        convolutions(a, [int(m) for m in a.conv_precision.split(",")], path, say)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.attn:  # printed; written only where --out names a file (profiles/addon_attn.txt is put together from this and tools/classifier_bench.py --attn)
        attention(a, [int(m) for m in a.attn.split(",")], path, say)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.precision:
        precision(a, [int(m) for m in a.precision.split(",")], path, say)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
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
