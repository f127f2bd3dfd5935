"""Developer tool: wall time from samples in memory to both voice latents, tts_voice_from_audio (everything on the device) against the host route it stands beside
(tts_host_mel_voice80 + tts_host_mel_diffusion100 on the CPU, then tts_voice_latent + tts_diffusion_conditioning_latent), on the same box in the same run:
1, 2 and 4 clips of 6 s at 44.1 kHz, upstream's windows, full-depth synthetic encoders (6 and 5 attention blocks). `--runs` timed calls after two warm-ups
per case; median, minimum, maximum and the spread (max - min) / median. The host route needs its clips at 22.05 and 24 kHz: tools/make_voice.py's resampler
(scipy.signal.resample_poly) is timed on its own line and the host figure is given with and without it (without scipy: without only). The device time of the
front-end's kernel families ("afe_finite", "afe_resample", "afe_mel") comes from a separate profiled call; the compiler's resource summary of the kernels is
appended (hipcc -Rpass-analysis=kernel-resource-usage, compile only). The record of one run is profiles/voice_from_audio.txt.

  python tools/voice_audio_bench.py [--runs 5] [--out FILE] [--ratios FILE]

--ratios: the worst |err| / bound table tests/test_afe_kernels_gpu.py writes under TTS_AFE_REPORT, appended to the record."""
import argparse
import os
import socket
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

pkg = tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402


def resources():
    """the compiler's view of the front-end's kernels: VGPRs, SGPRs, scratch, occupancy, LDS"""
    src = os.path.join(ROOT, "tortoise.cpp_amd", "csrc", "audio_frontend.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I" + os.path.dirname(src),
           "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.TimeoutExpired) as e:
        return ["resource summary: not available (%s)" % e]
    out, keep = [], ("Function Name", "VGPRs:", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size")
    for ln in r.stderr.splitlines():
        if "remark:" in ln and any(k in ln for k in keep):
            out.append("  " + ln.split("remark:", 1)[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").rstrip())
    return out or ["resource summary: not available (hipcc exit %d)" % r.returncode]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ratios", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        sys.exit("--runs: at least 5 (the spread is part of the record)")
    d = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "voice_audio_bench")
    os.makedirs(d, exist_ok=True)
    vp, dp = os.path.join(d, "ggml-conditioning-model.bin"), os.path.join(d, "ggml-diffusion-conditioning-model.bin")
    for p, write, blocks, seed in ((vp, sw.write_voice_encoder, 6, 56), (dp, sw.write_diffusion_conditioning_encoder, 5, 75)):
        if not os.path.exists(p + ".done"):
            write(p, blocks=blocks, seed=seed)
            open(p + ".done", "w").write("ok")
    eng = pkg.Engine(0)
    eng.load_voice_encoder(vp)
    eng.load_diffusion_conditioning_encoder(dp)
    rate, secs = 44100, 6.0
    rs = np.random.RandomState(5)
    t = np.arange(int(rate * secs)) / rate
    clips = [(0.3 * np.sin(2 * np.pi * (140 + 30 * i) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.03 * rs.randn(len(t))).astype(np.float32) for i in range(4)]
    try:
        from scipy.signal import resample_poly
    except ImportError:
        resample_poly = None
    lines = ["host %s, %s: %d timed calls after 2 warm-ups per case; clips of %.0f s at %d Hz; encoders of 6 / 5 attention blocks (synthetic weights)" %
             (socket.gethostname(), time.strftime("%Y-%m-%d"), a.runs, secs, rate)]

    def timed(what, fn):
        ts = []
        for _ in range(2 + a.runs):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        ts = ts[2:]
        med = statistics.median(ts)
        lines.append("%-66s median %9.2f ms  (min %9.2f max %9.2f, spread %5.1f %%)" % (what, med, min(ts), max(ts), 100 * (max(ts) - min(ts)) / med))
        print(lines[-1], flush=True)
        return med, min(ts), max(ts)

    for n in (1, 2, 4):
        cs = clips[:n]
        dev = timed("%d clip(s): tts_voice_from_audio" % n, lambda: eng.voice_from_audio(cs, rate))
        if resample_poly is not None:
            timed("%d clip(s): host resampling to 22.05 k and 24 k (scipy resample_poly)" % n,
                  lambda: [(resample_poly(x, 1, 2), resample_poly(x, 80, 147)) for x in cs])
            a22 = [resample_poly(x, 1, 2).astype(np.float32)[:132300] for x in cs]
            a24 = [resample_poly(x, 80, 147).astype(np.float32)[:102400] for x in cs]
        else:  # the host mels' cost does not depend on the samples' values: the source cut to the windows stands in for its resampled form
            a22, a24 = [x[:132300] for x in cs], [x[:102400] for x in cs]
        timed("%d clip(s): tts_host_mel_voice80 + tts_host_mel_diffusion100" % n, lambda: ([pkg.host_mel_voice80(x) for x in a22], [pkg.host_mel_diffusion100(x) for x in a24]))
        m80, m100 = [pkg.host_mel_voice80(x) for x in a22], [pkg.host_mel_diffusion100(x) for x in a24]
        timed("%d clip(s): tts_voice_latent + tts_diffusion_conditioning_latent" % n, lambda: (eng.voice_latent(m80), eng.diffusion_conditioning_latent(m100)))
        host = timed("%d clip(s): host route without resampling (mels + encoders)" % n,
                     lambda: (eng.voice_latent([pkg.host_mel_voice80(x) for x in a22]), eng.diffusion_conditioning_latent([pkg.host_mel_diffusion100(x) for x in a24])))
        # a gain is stated only when the two ranges do not touch
        verdict = "faster beyond the spread" if dev[2] < host[1] else "slower beyond the spread" if dev[1] > host[2] else "inside the run-to-run spread"
        lines.append("%d clip(s): device / host medians %.3f: %s" % (n, dev[0] / host[0], verdict))
        print(lines[-1], flush=True)
    # device time of the front-end's kernels: a profiled call of its own (event pairs drain the pipeline)
    eng.prof_reset(True)
    eng.voice_from_audio(clips, rate)
    for fam in ("afe_finite", "afe_resample", "afe_mel", "gemm"):
        ms, launches, work = eng.prof_get(fam)
        if launches:
            lines.append("profiled call, 4 clips: family %-14s %8.3f ms in %d launches" % (fam, ms, launches))
    eng.prof_reset(False)
    eng.close()
    lines.append("compiler resource summary (csrc/audio_frontend.hip, gfx950):")
    lines += resources()
    if a.ratios and os.path.exists(a.ratios):
        lines.append("worst |err| / bound per kernel and input family (tests/test_afe_kernels_gpu.py, TTS_AFE_REPORT):")
        lines += ["  " + ln.rstrip() for ln in open(a.ratios)]
    print("\n".join(lines[-12:]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
