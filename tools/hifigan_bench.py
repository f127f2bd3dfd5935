"""Developer tool: wall time of the HiFi-GAN decoder call (tts_hifigan_decode, synchronous) against the decoder path it replaces (tts_diffusion, 80 steps, device
noise, + tts_vocoder) on the same box in the same run: benchmark length (L = 200 latent rows, T = 870 frames), 16 candidates and one candidate. Median of `--calls`
timed calls after two warm-ups; the "hfg_conv" profiler family's device time and achieved FLOP rate from a separate profiled call (event pairs drain the
pipeline, so the profiled call is not one of the timed ones). The record of one run is profiles/hifigan_decoder.txt.

  python tools/hifigan_bench.py [--calls 5] [--out FILE] [--no-diffusion 1]

The HiFi-GAN weights are synthetic (tortoise.cpp_amd/synth_weights.py: write_hifigan), the diffusion and vocoder weights the benchmark's."""
import argparse
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

pkg = tortoise_cpp_amd_loader.load()
import bench  # noqa: E402
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-diffusion", type=int, default=0)
    a = ap.parse_args()
    d = os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models")
    hp = os.path.join(d, "ggml-hifigan-model.bin")
    if not a.no_diffusion:
        bench.ensure_models(d, False, True)
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(hp + ".done"):
        sw.write_hifigan(hp, seed=77)
        open(hp + ".done", "w").write("ok")
    eng = pkg.Engine(0)
    eng.load_hifigan(hp)
    L = 200
    T = eng.frames(L)
    lines = ["host %s, %s, median of %d timed calls after 2 warm-ups, L = %d (T = %d frames, %.2f s of audio per candidate)" %
             (socket.gethostname(), time.strftime("%Y-%m-%d"), a.calls, L, T, 256 * T / 24000.0)]
    voice = np.random.RandomState(99).randn(1024).astype(np.float32)

    def timed(what, fn):
        ts = []
        for _ in range(2 + a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        ts = ts[2:]
        lines.append("%-58s median %8.1f ms  (min %8.1f max %8.1f)" % (what, statistics.median(ts), min(ts), max(ts)))
        print(lines[-1], flush=True)
        return statistics.median(ts)

    res = {}
    for B in (16, 1):
        lats = [np.random.RandomState(c).randn(L, 1024).astype(np.float32) for c in range(B)]
        res[("hfg", B)] = timed("B = %2d  tts_hifigan_decode" % B, lambda: eng.hifigan_decode(lats, voice))
        eng.prof_reset(True)
        eng.hifigan_decode(lats, voice)
        ms, n, work = eng.prof_get("hfg_conv")
        eng.prof_reset(False)
        lines.append("B = %2d  hfg_conv family: %d launches, %.1f ms on the device, %.3f TFLOP -> %.1f TFLOP/s (f32-input MFMA peak 157.3)" %
                     (B, n, ms, work / 1e12, work / ms / 1e9))
        print(lines[-1], flush=True)
    if not a.no_diffusion:
        eng.load(diffusion=d + "/ggml-diffusion-model.bin", vocoder=d + "/ggml-vocoder-model.bin")
        eng.seed(0)
        for B in (16, 1):
            lats = [np.random.RandomState(c).randn(L, 1024).astype(np.float32) for c in range(B)]
            res[("diff", B)] = timed("B = %2d  tts_diffusion (80 steps, device noise) + tts_vocoder" % B,
                                     lambda: eng.vocoder(eng.diffusion(lats, n_steps=80, noise_mode=pkg.NOISE_DEVICE), noise_mode=pkg.NOISE_DEVICE))
        for B in (16, 1):
            lines.append("B = %2d  diffusion path / HiFi-GAN decoder: %.1f x" % (B, res[("diff", B)] / res[("hfg", B)]))
            print(lines[-1], flush=True)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
