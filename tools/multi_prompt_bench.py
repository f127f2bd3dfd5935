"""AR stage of 8 distinct prompts (bench.py synthetic_prompt(p)): one tts_autoregressive_multi call against 8 tts_autoregressive calls, alternating in one process.
66 text ids per prompt, full-size synthetic weights (bench.py's), 192 masked codes, 1 and 16 candidates per prompt.
The 8 single-prompt calls run with the RNG shard of their candidates (rng_shard_offset = p n, rng_shard_total = 8 n), so both forms sample the same codes:
checked on every repetition. The per-phase split (begin / prefill / loop / latents) is the driver's own TTS_TIMING breakdown, summed over the calls.
    python tools/multi_prompt_bench.py [--reps 5] [--shapes 1,16] [--out profiles/multi_prompt_bench.json]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

os.environ["TTS_TIMING"] = "1"  # read once by the library: the driver's host-side phase breakdown on stderr
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import bench  # noqa: E402
import tortoise_cpp_amd_loader  # noqa: E402

PHASE_RE = re.compile(r"\[tts timing\] AR: begin ([\d.]+) ms, prefill ([\d.]+), loop ([\d.]+) .*latents ([\d.]+), total ([\d.]+)")


class StderrCapture:
    """the C library's stderr (fd 2) of the calls inside the block"""

    def __enter__(self):
        sys.stderr.flush()
        self.f = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.text = self.f.read().decode(errors="replace")
        self.f.close()


def phases(text):
    tot = np.zeros(5)
    for m in PHASE_RE.finditer(text):
        tot += np.array([float(x) for x in m.groups()])
    return dict(zip(("begin", "prefill", "loop", "latents", "total"), np.round(tot, 1).tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1,16", help="candidates per prompt")
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--codes", type=int, default=192)
    ap.add_argument("--models", default=os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = tortoise_cpp_amd_loader.load()
    bench.ensure_models(a.models, False, True)
    voice = np.fromfile(os.path.join(ROOT, "models", "mol.bin"), np.float32)
    eng = pkg.Engine(0)
    eng.load(ar=os.path.join(a.models, "ggml-model.bin"))
    prompts = [bench.synthetic_prompt(p) for p in range(a.prompts)]
    G, S = len(prompts), a.codes
    result = {"what": __doc__.splitlines()[0] + " (full-size synthetic weights, %d masked codes)" % S, "prompts": G, "text_ids_per_prompt": len(prompts[0]), "codes": S, "reps": a.reps, "shapes": {}}

    def run_multi(n):
        eng.seed(11)
        with StderrCapture() as cap:
            t0 = time.perf_counter()
            codes, _, _, _ = eng.autoregressive_multi(prompts, voice, [n] * G, S, mask_stop=True)
            ms = (time.perf_counter() - t0) * 1e3
        return ms, np.concatenate(codes), phases(cap.text)

    def run_seq(n):
        out = []
        try:
            with StderrCapture() as cap:
                t0 = time.perf_counter()
                for p in range(G):
                    eng.set_option("rng_shard_offset", p * n)
                    eng.set_option("rng_shard_total", G * n)
                    eng.seed(11)
                    codes, _, _, _ = eng.autoregressive(prompts[p], voice, n, S, mask_stop=True)
                    out.append(codes)
                ms = (time.perf_counter() - t0) * 1e3
        finally:
            eng.set_option("rng_shard_offset", 0)
            eng.set_option("rng_shard_total", 0)
        return ms, np.concatenate(out), phases(cap.text)

    for n in [int(x) for x in a.shapes.split(",")]:
        run_multi(n), run_seq(n)  # warm-up: graph capture, buffer growth, sampler pool
        multi, seq, same = [], [], True
        for r in range(a.reps):
            m = run_multi(n)
            s = run_seq(n)
            multi.append(m)
            seq.append(s)
            same = same and bool((m[1] == s[1]).all())
        mm = [x[0] for x in multi]
        ss = [x[0] for x in seq]
        best_m, best_s = int(np.argmin(mm)), int(np.argmin(ss))
        result["shapes"]["%dx%d" % (G, n)] = {
            "candidates_per_prompt": n, "batch": G * n,
            "multi_ms": {"median": round(float(np.median(mm)), 1), "min": round(min(mm), 1), "max": round(max(mm), 1)},
            "sequential_ms": {"median": round(float(np.median(ss)), 1), "min": round(min(ss), 1), "max": round(max(ss), 1)},
            "speedup_median": round(float(np.median(ss) / np.median(mm)), 2),
            "phases_ms_multi_best": multi[best_m][2], "phases_ms_sequential_best": seq[best_s][2],
            "codes_identical": same,
        }
        print(json.dumps({"%dx%d" % (G, n): result["shapes"]["%dx%d" % (G, n)]}), flush=True)
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
