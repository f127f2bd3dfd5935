#!/usr/bin/env python3
"""CVVP timings (profiles/cvvp.txt): tts_cvvp_voice_audio of one 6 s 44.1 kHz clip and tts_cvvp_score of 16 candidates x 200 codes on a depth-8 file, beside
tts_clvp_score at tests/test_clvp.py's bench shape in the same process. Every case is warmed 3 times, then the range of 7 calls: a host clock around calls that
end in a stream synchronise. Needs an MI355X; prints the table (and writes it to the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

pkg = tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402


def synth(sub, name, write, **kw):
    d = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), sub)
    os.makedirs(d, exist_ok=True)
    p = os.path.join(d, name)
    if not os.path.exists(p + ".done"):
        write(p, **kw)
        open(p + ".done", "w").write("ok")
    return p



def timed(fn, n=7, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts)), max(ts)


e = pkg.Engine(0)
e.load_cvvp(synth("cvvp", "ggml-cvvp-model-bench.bin", sw.write_cvvp, depth=8, seed=85))
rs = np.random.RandomState(0)
t = np.arange(6 * 44100) / 44100.0
clip = (0.3 * np.sin(2 * np.pi * 180 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.03 * rs.randn(len(t))).astype(np.float32)
lat = e.cvvp_voice_audio([clip], 44100)
mel = e.audio_mel(clip, 44100, 80)
c16 = [rs.randint(0, 8192, 200).astype(np.int32) for _ in range(16)]
rows = []
rows.append(("tts_cvvp_voice_audio, one 6 s 44.1 kHz clip (517 frames -> 130 rows), depth 8", timed(lambda: e.cvvp_voice_audio([clip], 44100))))
rows.append(("tts_cvvp_voice of that clip's mel (no front-end)", timed(lambda: e.cvvp_voice([mel]))))
rows.append(("tts_audio_mel of that clip, 80 bands (the front-end alone)", timed(lambda: e.audio_mel(clip, 44100, 80))))
rows.append(("tts_cvvp_score, 16 candidates x 200 codes against one clip, depth 8", timed(lambda: e.cvvp_score(lat, c16))))
e.load_clvp(synth("clvp", "ggml-clvp-model-full.bin", sw.write_clvp, depth=20, seed=119))
rs9 = np.random.RandomState(9)
t66, k16 = rs9.randint(0, 256, 66).astype(np.int32), [rs9.randint(0, 8192, 200).astype(np.int32) for _ in range(16)]
rows.append(("tts_clvp_score, 16 candidates x 200 codes against 66 text ids, depth 20 (tests/test_clvp.py's bench shape)", timed(lambda: e.clvp_score(t66, k16))))
lines = ["%-110s min %7.2f  median %7.2f  max %7.2f ms" % (name, lo, med, hi) for name, (lo, med, hi) in rows]
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
e.close()
