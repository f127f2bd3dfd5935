#!/usr/bin/env python3
"""Random voices (tts_random_voice) at upstream's sizes, on synthetic weights: writes profiles/random_voice.txt.

For 1, 16 and 64 voices, both sides (1024 and 2048 channels, six layers each) in one call:
  - --calls timed calls after --warm untimed ones: the median and min .. max of the host clock around the synchronous call (seed upload, one noise fill and six
    dependent launches per side, download);
  - the weight-read rate that time implies: the bytes of f32 weights the layer kernels read from memory, 6 x D x D x 4 per side and per batch tile, over the call's
    time, against the 8.0 TB/s HBM3E peak (6.29 TB/s measured with a float4 copy) of the MI355X;
  - the engine profiler's device time of the two kernel families for one call (rlg_layer, rlg_noise);
  - the compiler's resource summary of the two kernels (hipcc -Rpass-analysis=kernel-resource-usage on testlib/rlg_harness.hip, device code only).
A record, not a gate: nothing on the parent commit does this work. A run without a GPU fails at Engine(0): nothing falls back. --resources-only writes the
resource summary alone (needs no GPU).

  python tools/random_voice_bench.py [--calls 7] [--warm 2] [--models DIR] [--out profiles/random_voice.txt] [--resources-only]"""
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

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
TILE = 8  # csrc/random_voice.h: RLG_TILE
DIMS = (("auto", 1024), ("diffusion", 2048))


def resources():
    """{kernel: resource figures} of the two kernels"""
    src = os.path.join(ROOT, "tortoise.cpp_amd", "testlib", "rlg_harness.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "tortoise.cpp_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "include"), "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                            "-x", "hip", "-c", src, "-o", os.path.join(d, "x.o")], capture_output=True, text=True, timeout=900)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(rlg_\w+?_kernel)", line)
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
    ap.add_argument("--models", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "rlg"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_voice.txt"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("Random voices (tts_random_voice): upstream's RandomLatentConverter at its two sizes, synthetic weights, tools/random_voice_bench.py")
    weights = sum(6 * d * d * 4 for _, d in DIMS)
    say("both sides per call: 6 layers x 1024 x 1024 and 6 layers x 2048 x 2048 of f32 = %.1f MB of weights, read once per batch tile of %d voices; f32 throughout"
        % (weights / 1e6, TILE))
    if a.resources_only:
        say("no timing exists: this file was written without a GPU run (tools/random_voice_bench.py --resources-only)")
    else:
        os.makedirs(a.models, exist_ok=True)
        paths = {}
        for (side, dim), name, seed in zip(DIMS, ("ggml-random-voice-model.bin", "ggml-random-diffusion-voice-model.bin"), (1270, 1271)):
            paths[side] = os.path.join(a.models, name)
            if not os.path.exists(paths[side] + ".done"):
                sw.write_random_voice(paths[side], dim, seed)
                open(paths[side] + ".done", "w").write("ok")
        eng = pkg.Engine(0)
        eng.load_random_voice(auto=paths["auto"], diffusion=paths["diffusion"])
        say("host clock around the synchronous call (seed upload, per side one noise fill + six dependent launches, download); one MI355X, one process")
        for n in (1, 16, 64):
            seeds = list(range(100, 100 + n))
            for _ in range(a.warm):
                eng.random_voice(seeds)
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                eng.random_voice(seeds)
                ts.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median(ts)
            read = weights * ((n + TILE - 1) // TILE)
            say()
            say("  %2d voices  tts_random_voice  median %7.3f ms  (min %7.3f .. max %7.3f, %d calls)   %d batch tile(s): %.0f MB of weight reads = %.2f TB/s over the whole "
                "call = %.0f %% of the 8.0 TB/s HBM peak (%.0f %% of the 6.29 TB/s a float4 copy reaches)"
                % (n, med, min(ts), max(ts), len(ts), (n + TILE - 1) // TILE, read / 1e6, read / (med / 1e3) / 1e12, 100 * read / (med / 1e3) / HBM_PEAK,
                   100 * read / (med / 1e3) / HBM_COPY))
            eng.set_option("prof_stride", 1)
            eng.prof_reset(True)
            eng.random_voice(seeds)
            got = {f: eng.prof_get(f) for f in ("rlg_layer", "rlg_noise")}
            eng.prof_reset(False)
            for f, (ms, cnt, work) in got.items():
                say("             profiler, one call: %-9s %7.3f ms  %2d launches  %.2f TB/s%s"
                    % (f, ms, cnt, work / ms / 1e9 if ms > 0 else 0.0, "  (several tiles re-read a matrix the 256 MB Infinity Cache holds: not all of it is HBM traffic)" if f == "rlg_layer" and n > TILE else ""))
        eng.close()
        say()
        say("not measured: other voice counts, one side alone, the z path (an upload in place of the noise fill), the CLI")
    say()
    say("compiler resource summary (gfx950, -O3; LDS is dynamic: %d voices x D x 4 bytes = 32 KB at 1024 channels, 64 KB at 2048, two workgroups per CU of 160 KB):" % TILE)
    for k, v in sorted(resources().items()):
        say("  %-18s VGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  static LDS %d B/workgroup"
            % (k, v.get("VGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("Occupancy", -1), v.get("LDS Size", -1)))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
