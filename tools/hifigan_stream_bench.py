#!/usr/bin/env python3
"""Time to first audio of the HiFi-GAN decoder: tts_autoregressive + tts_hifigan_decode against tts_hifigan_stream, and the chunk path's two tiles.

Full-size synthetic weights (30 GPT-2 layers, the HiFi-GAN generator), one candidate, N codes with the stop token masked, everything in one process and run:
  (a) tts_autoregressive + tts_hifigan_decode: time until the first sample exists (= the whole of both calls)
  (b) tts_hifigan_stream at stride 8, 16, 32: time to the first callback
  (c) total time of (b) against (a)
  (d) one 32-frame and one 87-frame chunk alone, option hfg_small_m at 0 (the 256-row tile everywhere) and at each threshold of --small-m: with a window of
      80 / 135 frames, 256 moves conv_pre and the first transposed convolution to the small-M tile, 2048 stage 0's ResBlocks too, 16384 stage 1 as well
Host clock around synchronous calls; WARM untimed repeats first, then the median and the min .. max of REPS repeats, the variants interleaved.

  python tools/hifigan_stream_bench.py [--codes 200] [--reps 7] [--warm 2] [--small-m 256,2048,16384] [--models DIR] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

MSG = "this is a test message."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--models", default=os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"))
    ap.add_argument("--small-m", default="256,2048,16384")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = tortoise_cpp_amd_loader.load()
    from tortoise_cpp_amd import synth_weights as sw
    os.makedirs(a.models, exist_ok=True)
    ar_path, hfg_path = os.path.join(a.models, "ggml-model.bin"), os.path.join(a.models, "ggml-hifigan-model.bin")
    if not os.path.exists(ar_path):
        sw.write_ar(ar_path, 30, seed=1234)
    if not os.path.exists(hfg_path):
        sw.write_hifigan(hfg_path)
    e = pkg.Engine(0)
    e.load(ar=ar_path)
    e.load_hifigan(hfg_path)
    e.tokenizer_load(os.path.join(ROOT, "models", "tokenizer.json"))
    voice = np.fromfile(os.path.join(ROOT, "models", "mol.bin"), np.float32)
    tok = e.tokenize(MSG)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def stat(xs):
        return "%8.2f ms  (min %.2f .. max %.2f, %d runs)" % (statistics.median(xs), min(xs), max(xs), len(xs))

    def whole():
        e.seed(1)
        t0 = time.perf_counter()
        _, _, lats, _ = e.autoregressive(tok, voice, 1, a.codes, mask_stop=True)
        t1 = time.perf_counter()
        audio = e.hifigan_decode(lats, voice)[0]
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, audio

    def stream(stride):
        e.seed(1)
        first = []
        t0 = time.perf_counter()
        _, _, _, chunks, _ = e.hifigan_stream(tok, voice, a.codes, pkg.AR_MASK_STOP, stride, on_chunk=lambda s, last: first.append(time.perf_counter()) and False)
        t1 = time.perf_counter()
        return (first[0] - t0) * 1e3, (t1 - t0) * 1e3, chunks

    strides = (8, 16, 32)
    res = {"a": [], "ar": [], "dec": []}
    res.update({("first", s): [] for s in strides})
    res.update({("total", s): [] for s in strides})
    same = True
    for rep in range(a.warm + a.reps):
        tot, t_ar, t_dec, audio = whole()
        runs = {s: stream(s) for s in strides}
        for s in strides:
            same = same and np.concatenate([c[0] for c in runs[s][2]]).tobytes() == audio.tobytes()
        if rep < a.warm:
            continue
        res["a"].append(tot); res["ar"].append(t_ar); res["dec"].append(t_dec)
        for s in strides:
            res["first", s].append(runs[s][0]); res["total", s].append(runs[s][1])
    say("hifigan_stream_bench: %d codes, 1 candidate, %d text ids, 30-layer synthetic AR weights, %d warm + %d timed runs, host clock" % (a.codes, len(tok), a.warm, a.reps))
    say("(a) tts_autoregressive + tts_hifigan_decode, first sample: " + stat(res["a"]))
    say("      of which tts_autoregressive                         " + stat(res["ar"]))
    say("               tts_hifigan_decode                         " + stat(res["dec"]))
    for s in strides:
        say("(b) tts_hifigan_stream stride %2d, first callback:        %s   %d callbacks" % (s, stat(res["first", s]), len(runs[s][2])))
    for s in strides:
        say("(c) tts_hifigan_stream stride %2d, total:                 %s   %+.1f %% against (a)" %
            (s, stat(res["total", s]), 100.0 * (statistics.median(res["total", s]) / statistics.median(res["a"]) - 1.0)))
    say("    streamed audio identical to (a)'s, all runs: %s" % same)
    # (d) one chunk alone: frames [24, 24 + n) of a 60-row utterance (a halo on either side: 80 and 135 frames evaluated)
    rs = np.random.RandomState(7)
    lat, v = rs.randn(60, 1024).astype(np.float32), rs.randn(1024).astype(np.float32)
    opts = [0] + [int(x) for x in a.small_m.split(",")]
    for n in (32, 87):
        t = {o: [] for o in opts}
        for rep in range(a.warm + 3 * a.reps):
            for opt in opts:
                e.set_option("hfg_small_m", opt)
                t0 = time.perf_counter()
                e.hifigan_chunk([lat], v, [24], [n])
                if rep >= a.warm:
                    t[opt].append((time.perf_counter() - t0) * 1e3)
        for opt in opts:
            say("(d) one %2d-frame chunk (%3d frames evaluated), %-34s %s" %
                (n, n + 48, "256-row tile everywhere:" if opt == 0 else "small-M tile up to %5d rows:" % opt, stat(t[opt])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    e.close()


if __name__ == "__main__":
    main()
