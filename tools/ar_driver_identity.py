#!/usr/bin/env python3
"""SHA-256 digests of everything the AR front ends return, for comparing two builds of the library bit for bit (profiles/ar_driver_refactor.txt).

The synthetic 2-layer AR model of the tests (small_models), a prompt of 3 ids, fixed seeds. Every case runs in a fresh process; the build is selected with
TTS_LIB_PATH, so the comparison is two runs of this script and a diff of their outputs:

  TTS_LIB_PATH=/path/to/parent/libtortoise_mi355x.so python tools/ar_driver_identity.py > parent.txt
  python tools/ar_driver_identity.py > new.txt && diff parent.txt new.txt

Cases (one line each, "<case> <sha256>"):
  ar f<flags> topk<0|1> scope<0|1>   tts_autoregressive, B = 3, flags 0 / MASK_STOP / MASK_STOP|RETIRE (the last with a stop schedule): codes, rows, latents, steps,
                                     stop status, fallbacks, the RNG state afterwards. The synthetic weights never sample the stop token, so the strict calls
                                     (flags 0) run on a head that answers it about every second time (lm_head weight 0, bias[8193] = 6.5 beside 8 ids of
                                     3.5 .. 4.5): with seed 25 the three candidates sample it in one iteration after 5 (scope 0) and 17 (scope 1) iterations
  multi                              tts_autoregressive_multi, 2 prompts x 2 candidates, stop schedule
  strict_limit                       a strict call that reaches max_steps = 4: status and tts_last_error text
  step_sample                        tts_ar_begin + tts_ar_prefill + tts_sample, then tts_ar_step_sample six times by hand
  stream s<stride> <codes>           tts_hifigan_stream at stride 1 and 7 with stop schedules of 12, 31 and 40 codes, and "stop": a model whose head always answers
                                     the stop token (lm_head weight 0, bias[8193] = 50), strict: codes, rows, latents, audio, chunk sizes, recaptures
  session                            4 slots, audio at stride 3, TTS_AR_ROW_CONTROLS: three staggered requests of 1, 2, 1 candidates (the second under its own
                                     controls), a cancelled request whose slot the next one takes; then a strict session whose request reaches its own max_steps = 4:
                                     collect outputs, drained audio, recaptures, fallbacks

  python tools/ar_driver_identity.py [--case NAME] [--work DIR]"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOKENS = np.array([17, 203, 88], np.int32)
TOKENS_B = np.array([5, 140, 61], np.int32)
STREAM = {"12": [12], "31": [31], "40": [40], "stop": None}


def case_names():
    names = ["ar f%d topk%d scope%d" % (f, t, s) for f in (0, 1, 3) for t in (0, 1) for s in (0, 1)]
    names += ["multi", "strict_limit", "step_sample"]
    names += ["stream s%d %s" % (st, k) for st in (1, 7) for k in STREAM]
    return names + ["session"]


def models(work):
    """The AR weights of the tests' small_models, the same with a head that always / about every second time answers 8193, and the tests' HiFi-GAN weights."""
    from tortoise_cpp_amd import synth_weights as SW
    os.makedirs(work, exist_ok=True)
    ar, stop, half, hfg = (os.path.join(work, n) for n in ("ar.bin", "ar_stop.bin", "ar_half.bin", "hifigan.bin"))
    if not os.path.exists(os.path.join(work, ".done")):
        SW.write_ar(ar, 2, 4321)
        t = SW.read_ggml(ar)
        t["inference_model.lm_head.1.weight"][:] = 0
        rs = np.random.RandomState(41)
        often = (rs.randn(8194) * 0.1).astype(np.float32)
        often[rs.choice(np.arange(2, 8190), 8, replace=False)] = rs.uniform(3.5, 4.5, 8).astype(np.float32)
        often[8193] = 6.5
        always = np.zeros(8194, np.float32)
        always[8193] = 50
        for path, bias in ((stop, always), (half, often)):
            t["inference_model.lm_head.1.bias"][:] = bias
            w = SW.GgmlWriter(path)
            for name, arr in t.items():
                w.add(name, arr)
            w.close()
        SW.write_hifigan(hfg, seed=77)
        open(os.path.join(work, ".done"), "w").write("ok")
    return ar, stop, half, hfg


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, *items):
        for x in items:
            if isinstance(x, (list, tuple)):
                self.add(*x)
            elif isinstance(x, np.ndarray):
                self.h.update(str((x.dtype, x.shape)).encode() + np.ascontiguousarray(x).tobytes())
            else:
                self.h.update(repr(x).encode())


def rng_state(e):
    with tempfile.TemporaryDirectory() as d:
        e.rng_save_state(os.path.join(d, "rng"))
        return open(os.path.join(d, "rng")).read()


def run_case(name, work):
    import tortoise_cpp_amd_loader
    pkg = tortoise_cpp_amd_loader.load()
    ar, stop, half, hfg = models(work)
    voice = np.fromfile(os.path.join(ROOT, "models", "mol.bin"), np.float32)
    d = Digest()
    e = pkg.Engine(0)
    part = name.split()
    if part[0] == "ar":
        flags, topk, scope = int(part[1][1:]), int(part[2][4:]), int(part[3][5:])
        e.set_option("device_topk", topk)
        e.set_option("ar_penalty_scope", scope)
        e.load(ar=ar if flags else half)
        if flags == 3:
            e.set_stop_schedule([9, 14, 11])
        e.seed(21 if flags else 25)
        d.add(e.autoregressive(TOKENS, voice, 3, 16 if flags else 40, mask_stop=bool(flags & 1), retire=bool(flags & 2)), e.ar_stop_status(3), e.topk_fallbacks(), rng_state(e))
    elif name == "multi":
        e.load(ar=ar)
        e.set_stop_schedule([7, 12, 10, 5])
        e.seed(22)
        d.add(e.autoregressive_multi([TOKENS, TOKENS_B], voice, [2, 2], 16, mask_stop=True, retire=True), e.ar_stop_status(4), e.topk_fallbacks(), rng_state(e))
    elif name == "strict_limit":
        e.load(ar=ar)
        e.seed(23)
        codes, rows, steps = np.zeros((3, 502), np.int32), np.zeros(3, np.int32), np.zeros(1, np.int32)
        rc = e.L.tts_autoregressive(e.h, TOKENS, len(TOKENS), voice, 3, 4, 0, codes.reshape(-1), rows, None, steps)
        d.add(rc, e.L.tts_last_error(e.h).decode(), rng_state(e))
    elif name == "step_sample":
        e.load(ar=ar)
        e.seed(24)
        e.ar_begin(TOKENS, voice, 3, 16)
        ids = np.ones((3, len(TOKENS) + 2), np.int32)
        ids[:, -1] = 8192
        prev = e.sample(e.ar_prefill(), ids)
        d.add(prev)
        for i in range(6):
            prev = e.ar_step_sample(prev, i, mask_stop=(i % 2 == 0))
            d.add(prev, e.topk_fallbacks())
        d.add(rng_state(e))
    elif part[0] == "stream":
        stride, sched = int(part[1][1:]), STREAM[part[2]]
        e.load(ar=stop if sched is None else ar)
        e.load_hifigan(hfg)
        if sched is not None:
            e.set_stop_schedule(sched)
        e.seed(25)
        codes, rows, lat, chunks, steps = e.hifigan_stream(TOKENS, voice, 10 if sched is None else 60, 0 if sched is None else 3, stride)
        d.add(codes, rows, lat, steps, [len(c[0]) for c in chunks], [c[1] for c in chunks], e.hifigan_stream_recaptures(), rng_state(e))
        d.add(np.concatenate([c[0] for c in chunks]) if chunks else None)
    elif name == "session":
        e.load(ar=ar)
        e.load_hifigan(hfg)
        e.ar_session_open(4, 2, 8, 24, mask_stop=True, retire=True, row_controls=True)
        e.ar_session_enable_audio(3)
        own = dict(temperature=1.2, top_k=7, top_p=0.6, penalty=1.5, scope=1)
        plan = {0: [("admit", "a", dict(tokens=TOKENS, n_cand=1, seed=31, stop_at=[9]))],
                2: [("admit", "b", dict(tokens=TOKENS_B, n_cand=2, seed=32, stop_at=[6, 14], controls=own))],
                3: [("admit", "x", dict(tokens=TOKENS, n_cand=1, seed=33, stop_at=[20]))],
                5: [("cancel", "x", None), ("admit", "c", dict(tokens=TOKENS_B, n_cand=1, seed=34, stop_at=[5], max_steps=12))]}
        ids, pcm, collected = {}, {}, set()
        for clock in range(40):
            for what, key, kw in plan.get(clock, []):
                if what == "admit":
                    ids[key] = e.ar_session_admit(kw.pop("tokens"), voice, kw.pop("n_cand"), kw.pop("seed"), **kw)
                    d.add("admitted", key, ids[key])
                else:
                    e.ar_session_cancel(ids.pop(key))
            live = e.ar_session_step()
            for key, rid in ids.items():
                if key not in collected and key != "b":  # one candidate: audio
                    a, last = e.ar_session_audio(rid)
                    pcm.setdefault(key, []).append(a)
                    d.add("audio", key, clock, len(a), last)
            for rid in e.ar_session_finished():
                key = [k for k, v in ids.items() if v == rid][0]
                d.add("collected", key, clock, e.ar_session_collect(rid))
                collected.add(key)
            d.add(clock, live, e.ar_session_room())
            if live == 0 and clock > 5:
                break
        d.add([np.concatenate(pcm[k]) for k in sorted(pcm)], e.ar_session_recaptures(), e.topk_fallbacks())
        e.ar_session_close()
        # a strict session: these weights never sample the stop token, the request reaches its own max_steps
        e.ar_session_open(2, 1, 8, 24)
        rid = e.ar_session_admit(TOKENS, voice, 1, 35, max_steps=4)
        while e.ar_session_step():
            pass
        d.add(e.ar_session_finished())
        try:
            e.ar_session_collect(rid)
            d.add("collected")
        except pkg.TtsError as err:
            d.add(str(err))
        d.add(e.ar_session_room(), e.ar_session_recaptures(), e.topk_fallbacks())
        e.ar_session_close()
    else:
        raise SystemExit("unknown case %r" % name)
    e.close()
    print("%-24s %s" % (name, d.h.hexdigest()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--work", default=os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "ar_driver_identity"))
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.work)
    for name in case_names():  # a fresh process per case; a case that fails ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--work", a.work], timeout=120)
        if r.returncode != 0:
            raise SystemExit("case %r ended with status %d" % (name, r.returncode))


if __name__ == "__main__":
    main()
