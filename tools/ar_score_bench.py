#!/usr/bin/env python3
"""Teacher-forced AR scoring (tts_ar_score_codes, csrc/ar_score.h): writes profiles/ar_score.txt.

  1. the kernel pair through the test harness on the cases of tests/ar_score_cases.py: the worst ratio of every output to its operand-derived bound;
  2. the engine on the small synthetic weights (2 layers), the candidates of tests/test_ar_score_gpu.py: TRAIN mode's worst ratio to the kernel's bound on the
     engine's own latents, DECODE mode's worst distance from the oracle's decode steps against its gate, and TRAIN mode's distance on the same input;
  3. on the full-size synthetic weights (30 layers, bench.py's): tts_ar_score_codes at 1 and 16 candidates x 200 codes, --calls timed calls after --warm untimed
     ones (median, min .. max of the host clock around the synchronous call); the "ar_score" profiler family's device time and TFLOP/s for one call; and the
     same scores through the only route the library had before: tts_ar_step in mode 0, one code at a time, 32 KB of logits per candidate and step to the host and
     a host log-softmax there;
  4. with --resources 1 the compiler's resource summary of the two kernels (device code of csrc/ar.hip only); --resources 2 appends that summary alone to --out
     and needs no GPU.
No time is a pass condition. A run without a GPU fails at Engine(0): nothing falls back.

  python tools/ar_score_bench.py [--calls 7] [--warm 2] [--models DIR] [--small DIR] [--resources 0|1|2] [--out profiles/ar_score.txt]"""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tortoise_cpp_amd_loader  # noqa: E402

pkg = tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

TOKENS = np.array([255, 147, 2, 54, 2, 14, 2, 136, 63, 2, 80, 32, 150, 112, 9, 0], np.int32)
KEYS = ("logp", "stop_logp", "lse")
N_CODES = 200


def resources():
    src = os.path.join(ROOT, "tortoise.cpp_amd", "csrc", "ar.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.dirname(src),
                            "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "x.o")],
                           capture_output=True, text=True, timeout=900)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(ar_score_\w*?kernel)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        if "Function Name:" in line:
            cur = None
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def resource_lines():
    lines = ["", "compiler resource summary (gfx950, -O3; ar_score_kernel's LDS is dynamic: the launch asks for it, the summary shows 0):"]
    for k, v in sorted(resources().items()):
        lines.append("  %-24s VGPRs %3d  AGPRs %3d  SGPRs %3d  scratch %d B/lane  occupancy %d waves/SIMD  static LDS %d B/workgroup"
                     % (k, v.get("VGPRs", -1), v.get("AGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1), v.get("Occupancy", -1), v.get("LDS Size", -1)))
    lines.append("  ar_score_kernel: 64 rows x one slab of 256 columns per workgroup (4 waves; a wave holds two 32-row MFMA tiles for each of its two 32-column tiles:"
                 " 64 accumulator registers); dynamic LDS = 64 x (512 + 1) x 4 B for one half of the rows' channels (K = 1024 is staged in two halves into the same"
                 " accumulators) + 3 328 B for the waves' (max, sum, argmax) and the targets = 134 656 B: one workgroup per CU (the compiler's occupancy figure counts"
                 " registers only)")
    return lines


def kernel_ratios(say):
    import ar_score_cases as A
    full = A.full_case()
    cases = [(full.first(130), full.reference()), (A.small_case(), None), (A.tail_tie_case(), None), (A.extreme_case(A.SMALL), None), (A.extreme_case(A.FULL), None)]
    say("1. the kernel pair against float64, one launch per case (tests/ar_score_cases.py), worst |kernel - float64| / bound over the rows:")
    for c, ref in cases:
        ref = ref or c.reference()
        rc, g = c.run()
        assert rc == 0, rc
        got = {k: v.payload for k, v in g.items()}
        ratios = ref.ratios(got)
        fails = ref.argmax_failures(got["greedy"], c.planted)
        free = c.planted < 0
        say("     %-16s %4d rows  N %4d  K %4d   %s   argmax rule: %d failures, %d planted ties, %.3f of the other rows under the margin"
            % (c.label, c.R, c.N, c.K, "  ".join("%s %.4f" % kv for kv in ratios.items()), len(fails), int((c.planted >= 0).sum()),
               float((~ref.decided[free]).mean()) if free.any() else 0.0))


def engine_small(say, small, voice):
    import ar_score_ref as R
    import oracle as O
    O.build()
    path = os.path.join(small, "ggml-model.bin")
    if not os.path.exists(os.path.join(small, ".done")):
        sw.write_all(small, ar_layers=2, diff_main=1, diff_tail=1, diff_integ=1, diff_lc=1, seed=4321)
        open(os.path.join(small, ".done"), "w").write("ok")
    eng = pkg.Engine(0)
    eng.load(ar=path)
    cands = R.candidates()
    trn, dec = eng.ar_score_codes(TOKENS, voice, cands, "train"), eng.ar_score_codes(TOKENS, voice, cands, "decode")
    eng.ar_begin(TOKENS, voice, len(cands), 1)
    eng.ar_prefill()
    lat = eng.ar_latents(R.padded502(cands), 41)
    W, b = R.head(O.Model(path))
    worst = 0.0
    for i, c in enumerate(cands):
        ref = R.Ref(lat[i, :len(c) + 1], W, b, np.concatenate([c, [8193]]).astype(np.int32), 8194)
        worst = max(worst, max(ref.ratios({k: trn[i][k] for k in KEYS}).values()))
    ol = R.oracle_decode_logits(O, path, TOKENS, voice, cands)
    lp = R.log_softmax64(ol)
    gate = 2.0 * R.DECODE_GATE * float(np.abs(ol).max())
    d_dec, d_trn = 0.0, np.inf
    for i, c in enumerate(cands):
        n, t = len(c), np.concatenate([c, [8193]])
        want = {"logp": lp[i, np.arange(n + 1), t], "stop_logp": lp[i, :n + 1, 8193], "lse": R.direct64(ol[i, :n + 1].astype(np.float64))}
        d_dec = max(d_dec, max(float(np.abs(dec[i][k] - want[k]).max()) for k in KEYS))
        d_trn = min(d_trn, float(np.abs(trn[i]["logp"][1:] - want["logp"][1:]).max()))
    eng.close()
    say()
    say("2. the engine on the small synthetic weights (2 layers), candidates of 5, 12 and 40 codes in one call (tests/test_ar_score_gpu.py):")
    say("     TRAIN mode against the float64 head on the engine's own tts_ar_latents rows: at most %.4f of the kernel's bound" % worst)
    say("     DECODE mode against float64 log-softmax of the oracle's prefill() / step(): worst distance %.3e, gate 2 x 1e-4 x max |oracle logit| = %.3e" % (d_dec, gate))
    say("     TRAIN mode against that same oracle (the position quirk seen from the other side): %.3e at the closest candidate" % d_trn)


def step_route(eng, voice, cands):
    """the scores through tts_ar_step, mode 0: one decode step and one [B][8194] logits copy per code, log-softmax on the host"""
    B = len(cands)
    eng.ar_begin(TOKENS, voice, B, N_CODES + 1)
    rows = [eng.ar_prefill()]
    for i in range(N_CODES):
        rows.append(eng.ar_step(np.array([c[i] for c in cands], np.int32), i))
    l = np.stack(rows, 1).astype(np.float64)
    m = l.max(2, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(l - m).sum(2))
    t = np.stack([np.concatenate([c, [8193]]) for c in cands])
    return np.take_along_axis(l, t[..., None], 2)[..., 0] - lse


def bench_full(say, a, voice):
    d = a.models
    if not os.path.exists(os.path.join(d, ".done")):
        sw.write_all(d, seed=1234)
        open(os.path.join(d, ".done"), "w").write("ok")
    eng = pkg.Engine(0)
    eng.load(ar=os.path.join(d, "ggml-model.bin"))
    say()
    say("3. full-size synthetic weights (30 layers), %d text ids, candidates of %d codes; host clock around the synchronous call" % (len(TOKENS), N_CODES))
    g = np.random.default_rng(7)
    for B in (1, 16):
        cands = [g.integers(0, 8192, N_CODES).astype(np.int32) for _ in range(B)]
        rows = B * (N_CODES + 1)
        for _ in range(a.warm):
            got = eng.ar_score_codes(TOKENS, voice, cands, "decode")
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            eng.ar_score_codes(TOKENS, voice, cands, "decode")
            ts.append((time.perf_counter() - t0) * 1e3)
        eng.set_option("prof_stride", 1)
        eng.prof_reset(True)
        eng.ar_score_codes(TOKENS, voice, cands, "decode")
        ms, cnt, work = eng.prof_get("ar_score")
        eng.prof_reset(False)
        for _ in range(1 if B > 1 else a.warm):
            via = step_route(eng, voice, cands)
        tr = []
        for _ in range(3):
            t0 = time.perf_counter()
            step_route(eng, voice, cands)
            tr.append((time.perf_counter() - t0) * 1e3)
        diff = max(float(np.abs(got[b]["logp"] - via[b]).max()) for b in range(B))
        med, medr = statistics.median(ts), statistics.median(tr)
        say()
        say("  %2d candidates (%d scored rows, head %.1f GFLOP)" % (B, rows, 2.0 * rows * 1024 * 8194 / 1e9))
        say("     tts_ar_score_codes (prompt pass + latent pass + fused head)  median %9.2f ms  (min %9.2f .. max %9.2f, %d calls)" % (med, min(ts), max(ts), len(ts)))
        say("     profiler family ar_score, one call                          %9.3f ms  %d entries  %.1f TFLOP/s" % (ms, cnt, work / ms / 1e9 if ms > 0 else 0.0))
        say("     tts_ar_step mode 0 x %d + host log-softmax                  median %9.2f ms  (min %9.2f .. max %9.2f, 3 calls)   %.1f x the scoring call"
            % (N_CODES, medr, min(tr), max(tr), medr / med))
        say("     largest difference between the two routes' log-probs %.2e (two f32 evaluations in different summation orders)" % diff)
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--models", default=os.environ.get("TTS_BENCH_MODELS", "/tmp/tts_bench_models"))
    ap.add_argument("--small", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "small"))
    ap.add_argument("--resources", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ar_score.txt"))
    a = ap.parse_args()
    if a.resources == 2:
        with open(a.out, "a") as f:
            f.write("\n".join(resource_lines()) + "\n")
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    voice = np.fromfile(os.path.join(ROOT, "models", "mol.bin"), np.float32)
    say("Teacher-forced AR scoring (tts_ar_score_codes; csrc/ar_score.h: ar_score_kernel + ar_score_reduce_kernel), synthetic weights, f32 throughout, tools/ar_score_bench.py")
    say("The weights are untrained: the scores themselves mean nothing; what is recorded is arithmetic against float64 and time.")
    say()
    kernel_ratios(say)
    engine_small(say, a.small, voice)
    bench_full(say, a, voice)
    if a.resources:
        for l in resource_lines():
            say(l)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
