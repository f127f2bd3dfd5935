#!/usr/bin/env python3
"""bench.py — end-to-end throughput of the hot path (AR decode -> diffusion -> vocoder) on MI355X.

Metric (BASELINE.json): audio-seconds/sec end-to-end, 16 AR candidates x 80 diffusion steps per GPU.
One "step" = one full pass over one batch: tts_autoregressive (prefill + 192 sampled codes + latent pass)
-> tts_diffusion (80 steps, cond+uncond) -> tts_vocoder for every candidate, weights resident in HBM,
synthetic 64-token prompt, stock mol.bin voice, full-size synthetic weights in the reference file format
(the trained weights are not available offline).

Workloads (--config, SURVEY 8d numbering; the name in BASELINE.json is given in the JSON line):
  3 (default) = BASELINE configs[2]: 16 candidates per GPU, 80 steps; N > 1: every rank its own 16 (weak scaling)
  4           = BASELINE configs[3]: ONE batch of 64 candidates sharded 64/N per GPU, 80 steps (strong scaling); the RNG stream
                partition (options rng_shard_offset / rng_shard_total) makes N x 64/N reproduce the ids of 1 x 64
  5           = BASELINE configs[4]: 8 distinct prompts x 16 candidates, 200 diffusion steps, prompts dealt round-robin to ranks
                (strong scaling)
Multi-GPU: one process per GPU. `python bench.py --gpus N` launches itself under torch.distributed.run when it is not already
running under it (WORLD_SIZE unset); RCCL (backend "nccl") broadcasts the prompt ids / voice latent from rank 0 and gathers
the audio on rank 0. No collective sits inside the data path: candidates never interact.

Prints ONE JSON line (rank 0). A plain run sets up, warms up, times --steps steps, writes the last timed step's outputs when
--dump-outputs DIR is given and prints the headline (`value`, `ms_per_step`, `stage_ms_per_step`, `load_ms`, `per_rank`, ...).
With --full the line also carries: `roofline` = the dominant kernel family (fp16 MFMA GEMMs of the diffusion stage, HIP-event timed on
the engine's stream inside the timed region), `roofline_decode` = the HBM-bound decode step (one event pair per hipGraph replay),
`cpu_baseline` = the oracle (CPU restatement of the reference path) on a bounded sample at 4 threads and at all host cores, and the
A/B passes after the timed region (other share_uncond setting, reference precision, AR weight modes, ragged batch, one utterance,
first audio, CLVP).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

MFMA_F16_DENSE_PEAK_TFLOPS = 2500.0  # /opt/skills/guides/MI355X_MICROARCH.md: ~2.5 PF dense fp16/bf16
HBM_PEAK_GBS = 8000.0                # same guide: 8 TB/s spec (6.29 TB/s measured copy)
HBM_ACHIEVABLE_GBS = 6290.0          # same guide: float4 copy, the rate a streaming kernel can reach
# Shape classes of the diffusion stage's fp16 MFMA GEMMs (diffusion.hip: gemm()): (N, K, output bytes per element, residual read)
GEMM_FAMILIES = {
    "diff_gemm_k3r": (1024, 3072, 4, True),    # ResBlock out_layers conv k = 3 + residual
    "diff_gemm_qkv": (3072, 1024, 2, False),   # AttentionBlock qkv projection, fp16 out (V transposed)
    "diff_gemm_k1": (1024, 1024, 4, False),    # ResBlock in_layers conv k = 1
    "diff_gemm_k1r": (1024, 1024, 4, True),    # AttentionBlock proj_out + residual
    "diff_gemm_k3": (1024, 3072, 4, False),    # latent conditioner conv k = 3 (once per utterance)
    "diff_gemm_misc": (None, None, 4, False),  # inp_block (K = 3 x 128), integrating conv (K = 2048), out head (N = 256)
}


def gemm_kernel_table(per_kernel):
    """Per shape class: measured HIP-event time per launch against max(MFMA floor, algorithmic bytes / achievable HBM rate) — the
    k = 1 convolutions with an f32 residual stream are bound by their own bytes, not by the matrix pipe."""
    rows = []
    for fam, (N, K, ob, resid) in GEMM_FAMILIES.items():
        ms, n, fl = per_kernel.get(fam, (0.0, 0, 0.0))
        if n <= 0:
            continue
        us, gf = 1e3 * ms / n, fl / n / 1e9
        tflops = gf / us * 1e3  # GFLOP per microsecond = PFLOP/s
        row = {"family": fam, "launches_timed": int(n), "avg_launch_us": round(us, 1), "gflop_per_launch": round(gf, 2),
               "tflops": round(tflops, 1), "frac_of_mfma_peak": round(tflops / MFMA_F16_DENSE_PEAK_TFLOPS, 4)}
        if N:
            m_rows = fl / n / (2.0 * N * K)                                   # valid rows of the launch
            byts = m_rows * (2.0 * K / (3 if K == 3072 else 1) + N * ob + (N * 4 if resid else 0)) + 2.0 * N * K  # A once (the 3 taps share it), out, resid, W
            t_mfma, t_hbm = gf / MFMA_F16_DENSE_PEAK_TFLOPS * 1e3, byts / (HBM_ACHIEVABLE_GBS * 1e9) * 1e6  # microseconds
            row.update(algorithmic_mb=round(byts / 1e6, 1), mfma_floor_us=round(t_mfma, 1), hbm_floor_us=round(t_hbm, 1),
                       bound="hbm" if t_hbm > t_mfma else "mfma", frac_of_bound=round(max(t_mfma, t_hbm) / us, 4))
        rows.append(row)
    return rows


def synthetic_prompt(p=0):
    # ids 255, (3 + 7j mod 250) for j < 64, 0  -> n = 66 text ids, P = 68 prompt positions; p > 0: the distinct
    # prompts of config 5 (same length, shifted ids)
    return np.array([255] + [3 + (7 * j + 11 * p) % 250 for j in range(64)] + [0], np.int32)


DUMP_LIMIT_BYTES = 60 * 1000 * 1000  # --dump-outputs: under 64 MB however a megabyte is counted


def _stack_padded(arrs, dtype):
    """[n, max shape...] with every array of the list in its leading corner, zeros elsewhere (candidates may differ in length)."""
    shp = tuple(max(x.shape[d] for x in arrs) for d in range(arrs[0].ndim))
    out = np.zeros((len(arrs),) + shp, dtype)
    for i, x in enumerate(arrs):
        out[(i,) + tuple(slice(0, n) for n in x.shape)] = x
    return out


def dump_outputs(path, pass_out):
    """--dump-outputs: what the stages returned in the last timed pass, every prompt's candidates in order, as DIR/<name>.npy (float32 for the
    computed values, float64 for ids and lengths). Above DUMP_LIMIT_BYTES in all, every array of more than 1 MB is replaced by a fixed sample
    of its flattened elements (seed 0, sorted indices) so that the files stay within the limit. Returns {name: description} for the JSON line."""
    arrays = {"codes": np.concatenate([np.asarray(o["codes"]).reshape(len(o["audio"]), -1) for o in pass_out]).astype(np.float64)}
    if "latents" in pass_out[0]:
        lats = [np.asarray(x, np.float32) for o in pass_out for x in o["latents"]]
        mels = [np.asarray(x, np.float32) for o in pass_out for x in o["mel"]]
        arrays["latent_rows"] = np.concatenate([np.asarray(o["latent_rows"]) for o in pass_out]).astype(np.float64)
        arrays["latents"] = _stack_padded(lats, np.float32)
        arrays["mel_frames"] = np.array([m.shape[1] for m in mels], np.float64)
        arrays["mel"] = _stack_padded(mels, np.float32)
    audio = [np.asarray(x, np.float32) for o in pass_out for x in o["audio"]]
    arrays["audio_samples"] = np.array([len(x) for x in audio], np.float64)
    arrays["audio"] = _stack_padded(audio, np.float32)
    total = sum(v.nbytes for v in arrays.values())
    big = {k for k, v in arrays.items() if v.nbytes > 1000 * 1000}
    keep = 1.0
    if total > DUMP_LIMIT_BYTES:
        small = sum(v.nbytes for k, v in arrays.items() if k not in big)
        keep = 0.99 * (DUMP_LIMIT_BYTES - small) / sum(arrays[k].nbytes for k in big)
    os.makedirs(path, exist_ok=True)
    info = {}
    for k, v in arrays.items():
        desc = {"shape": list(v.shape), "dtype": str(v.dtype)}
        if keep < 1.0 and k in big:
            idx = np.sort(np.random.default_rng(0).choice(v.size, int(v.size * keep), replace=False, shuffle=False))
            v = v.reshape(-1)[idx]
            desc = {"shape": list(v.shape), "dtype": str(v.dtype), "sample_of_shape": desc["shape"], "sample": "flat indices: sorted numpy default_rng(0).choice"}
        np.save(os.path.join(path, k + ".npy"), v)
        info[k] = desc
    return info


def ensure_models(path, quick, rank_is_writer, wait_s=1800):
    """Synthetic weights in the reference's file format, written once per node by local rank 0 BEFORE torch.distributed is initialised
    (2.4 GB, about a minute: no rank sits in a collective with a timeout while they are generated); the other ranks poll the stamp."""
    stamp = os.path.join(path, ".done")
    if rank_is_writer and not os.path.exists(stamp):
        from tortoise_cpp_amd import synth_weights as sw
        if quick:
            sw.write_all(path, ar_layers=2, diff_main=1, diff_tail=1, diff_integ=1, diff_lc=1, seed=1234)
        else:
            sw.write_all(path, seed=1234)  # 30-layer GPT-2, 4+3+10+3 diffusion blocks, UnivNet
        open(stamp, "w").write("ok")
    t0 = time.time()
    while not os.path.exists(stamp):
        if time.time() - t0 > wait_s:
            sys.exit("bench.py: weights were not generated at %s within %d s" % (path, wait_s))
        time.sleep(0.5)


def _omp_set_threads(n):
    import ctypes
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(int(n))
        return True
    except OSError:
        return False


def cpu_baseline_once(model_dir, voice, toks, S, L_bench, n_diff_steps, quick, threads):
    """Oracle (CPU restatement) on a bounded sample of the same workload at `threads` OpenMP threads, extrapolated with the
    algorithmic-work formulae of SURVEY §8d to one candidate of the bench workload."""
    import oracle as O
    _omp_set_threads(threads)
    n = len(toks)
    t_all = time.time()
    ar = O.AR(O.Model(os.path.join(model_dir, "ggml-model.bin")))
    nstep = 24 if not quick else 4
    ar.start(toks, voice, 1, n + 2 + nstep + 1)
    t0 = time.time(); ar.prefill(); t_prefill = time.time() - t0
    t0 = time.time()
    for i in range(nstep):
        ar.step(np.array([100 + i], np.int32), i)
    t_step = (time.time() - t0) / nstep
    row_s = t_prefill / (n + 2)                                   # seconds per transformer row (dense part)
    t_ar = t_prefill + S * t_step + (n + 1 + L_bench) * row_s     # + latent pass over the needed prefix
    del ar
    # diffusion: conditioner + cond and uncond forward at the bench's own size (L=200, T=870): only the number of repetitions
    # (diffusion steps) is extrapolated
    od = O.Diffusion(O.Model(os.path.join(model_dir, "ggml-diffusion-model.bin")))
    Ls = L_bench if not quick else 12
    Ts = od.T_of(Ls)
    lat = np.random.RandomState(0).randn(Ls, 1024).astype(np.float32)
    x = np.random.RandomState(1).randn(100, Ts).astype(np.float32)
    t0 = time.time(); ce = od.code_embedding(lat, Ts); t_cond = time.time() - t0
    npair = 2 if not quick else 1
    t0 = time.time()
    for ts in (3999, 51)[:npair]:
        od.forward(ce, x, ts); od.forward(None, x, ts)
    t_pair = (time.time() - t0) / npair
    fl = lambda T: 249307136.0 * T + 53248.0 * T * T              # per forward
    Tb = od.T_of(L_bench)
    t_diff = t_cond + n_diff_steps * t_pair * fl(Tb) / fl(Ts)     # conditioner once per utterance
    del od
    ov = O.Vocoder(O.Model(os.path.join(model_dir, "ggml-vocoder-model.bin")))
    mel = np.clip(np.random.RandomState(2).randn(100, Ts) * 0.5, -1, 1).astype(np.float32)
    t0 = time.time(); ov.run(mel, rng=O.Rng(0)); t_voc_s = time.time() - t0
    t_voc = t_voc_s * (Tb + 10) / (Ts + 10)
    audio_s = Tb * 256 / 24000.0                                  # the 10 silent pad frames are not counted
    return {"value": round(audio_s / (t_ar + t_diff + t_voc), 5), "threads": threads,
            "measured_s": {"prefill_P%d" % (n + 2): round(t_prefill, 3), "decode_step": round(t_step, 4), "diffusion_pair_T%d" % Ts: round(t_pair, 3),
                           "conditioner": round(t_cond, 3), "vocoder_T%d" % Ts: round(t_voc_s, 3), "sample_total": round(time.time() - t_all, 1)},
            "extrapolated_s_per_candidate": {"ar": round(t_ar, 1), "diffusion": round(t_diff, 1), "vocoder": round(t_voc, 2)}, "audio_s": round(audio_s, 3)}


def cpu_baseline(model_dir, voice, toks, S, L_bench, n_diff_steps, quick):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    nproc = os.cpu_count() or 1
    # 4 threads = ggml's default team (what ./tortoise would use); 16 = the largest team that still scales for this restatement. A team of ALL
    # host cores is NOT run by default: on the 256-thread GPU-box host it measured 0.00076 audio-s/s (30x slower than 4 threads: 33 s per decode
    # step of fork/join overhead) and took 17 minutes; TTS_BENCH_CPU_ALL_CORES=1 adds it.
    teams = sorted({min(4, nproc), min(16, nproc)} | ({nproc} if os.environ.get("TTS_BENCH_CPU_ALL_CORES") else set()))
    runs = [cpu_baseline_once(model_dir, voice, toks, S, L_bench, n_diff_steps, quick, th) for th in teams]
    best = max(runs, key=lambda r: r["value"])
    return {
        "value": best["value"], "unit": "audio-seconds/sec", "cores": best["threads"], "kind": "port", "host_nproc": nproc,
        "runs": runs,
        "sample": "oracle (f32 C++/OpenMP restatement of the ggml graphs; the reference itself cannot be built: ggml submodule absent), "
                  "B=1, at 4 OpenMP threads (ggml's default, what ./tortoise would use) and at 16 (host: %d hardware threads; a team of all of them "
                  "was measured 30x SLOWER than 4 threads on the 256-thread GPU-box host, DESIGN.md section 5); `value`/`cores` = the faster run. Measured per run: prompt pass, 24 decode steps, latent conditioner + two cond+uncond forward pairs at "
                  "the workload's own L=%d/T, the vocoder at the same T; extrapolated by repetition counts only (S=%d decode steps, %d "
                  "diffusion steps) to one candidate. Audio seconds = T*256/24000 (SURVEY 8d)" % (nproc, L_bench, S, n_diff_steps),
    }


def self_launch(a):
    """`python bench.py --gpus N` outside torchrun: re-exec under torch.distributed.run, one rank per GPU (RCCL over xGMI)."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: required for RCCL on this host driver
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, default=3, choices=[3, 4, 5], help="workload, SURVEY 8d numbering (3 = BASELINE configs[2], the metric's)")
    ap.add_argument("--candidates", type=int, default=None, help="AR candidates per GPU (config 3) / in total (config 4) / per prompt (config 5)")
    ap.add_argument("--diff-steps", type=int, default=None)
    ap.add_argument("--decode-steps", type=int, default=192, help="sampled codes per candidate (stop token masked) -> L=200, T=870")
    ap.add_argument("--quick", action="store_true", help="tiny layer counts (plumbing check only; NOT the benchmark)")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: roofline event timing inside the timed region, "
                                                          "the A/B passes after it and the CPU baseline (off by default)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last timed step computed (codes, latents, "
                                                                        "mels, audio; float32 / float64) as DIR/<name>.npy, under 64 MB in all (rank 0's own outputs)")
    ap.add_argument("--prof-stride", type=int, default=13, help="with --full: 1 GEMM launch in N (hashed decimation per shape class) is bracketed by a HIP event pair (roofline timing)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-share-uncond", action="store_true", help="headline pass with the unconditioned integrator layers evaluated per candidate")
    ap.add_argument("--no-ab", action="store_true", help="with --full: skip the extra passes after the timed region (other share_uncond setting, option A/Bs)")
    ap.add_argument("--latency-mode", action="store_true", help="option latency_mode for the headline pass too (it only acts on diffusion batches of <= 2 048 packed rows: "
                    "--candidates 1); the single-utterance A/B below always measures both settings")
    ap.add_argument("--engine-option", action="append", default=[], metavar="KEY=VALUE", help="tts_set_option on every rank's engine before the run (A/B of an option, e.g. hoist_integrator=0)")
    ap.add_argument("--no-diff-graph", action="store_true", help="A/B: launch every diffusion step eagerly instead of replaying the captured step graph")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo for the CPU plumbing test with --dry-engine)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed (and run every collective of the N > 1 path) even for ONE rank: "
                                                               "RCCL init, broadcast, all_gather, gather and all_reduce on a one-GPU box")
    ap.add_argument("--dry-engine", action="store_true", help="no device work: host-only contexts, fake stage outputs (tests of the launch / collective plumbing)")
    ap.add_argument("--models", default=None)
    ap.add_argument("--device-map", default=None, help="comma list: HIP device of each local rank (default: LOCAL_RANK). `--backend gloo --device-map 0,0` "
                                                       "runs two real engines on one GPU (test of the N > 1 path on a one-GPU box; RCCL needs one GPU per rank)")
    ap.add_argument("--allow-shared-device", action="store_true", help="let two ranks create their engine on ONE GPU (unsupported form; one-GPU test boxes only)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        sys.exit("bench.py: --steps must be >= 1 and --warmup >= 0")

    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    device = local_rank
    if a.device_map:
        dm = [int(x) for x in a.device_map.split(",")]
        if len(dm) <= local_rank:
            sys.exit("bench.py: --device-map has %d entries, local rank %d" % (len(dm), local_rank))
        if a.backend == "nccl" and len(set(dm)) != len(dm):
            sys.exit("bench.py: RCCL needs a distinct GPU per rank (--device-map %s); use --backend gloo to share a device" % a.device_map)
        if len(set(dm)) != len(dm) and not (a.allow_shared_device or a.dry_engine):
            sys.exit("bench.py: --device-map %s puts two engine processes on one GPU: unsupported (DESIGN.md section 6); --allow-shared-device to run anyway" % a.device_map)
        device = dm[local_rank]
    pkg = tortoise_cpp_amd_loader.load()
    model_dir = a.models or ("/tmp/tts_bench_models_quick" if a.quick else "/tmp/tts_bench_models")
    if not a.dry_engine:
        ensure_models(model_dir, a.quick, local_rank == 0)  # before the rendezvous: see ensure_models
    dist = None
    dev = None
    collective_ranks = 1
    if world > 1 or a.force_dist:
        import torch
        import torch.distributed as dist
        if a.force_dist and "RANK" not in os.environ:  # plain `python bench.py --force-dist`: a one-rank rendezvous of its own
            s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port_ = s_.getsockname()[1]; s_.close()
            os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK=str(local_rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port_))
        if a.backend == "nccl":
            torch.cuda.set_device(device)
            dev = torch.device("cuda", device)
            dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI
        else:
            dev = torch.device("cpu")
            dist.init_process_group(a.backend)
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)  # the collective backend has seen every rank: reported as `collective_ranks` in the JSON line
        collective_ranks = int(round(float(ones.item())))

    # ---- workload ---------------------------------------------------------------------------------------------------
    n_diff = a.diff_steps or (200 if a.config == 5 else 80)
    if a.config == 3:
        B = a.candidates or 16                      # per GPU
        my_prompts, cand0, cand_total, scaling = [0], 0, 0, "weak"
        name = "configs[2]"
    elif a.config == 4:
        total = a.candidates or 64
        if total % world:
            sys.exit("config 4: %d candidates do not divide over %d GPUs" % (total, world))
        B = total // world
        my_prompts, cand0, cand_total, scaling = [0], rank * B, total, "strong"
        name = "configs[3]"
    else:
        B = a.candidates or 16
        my_prompts, cand0, cand_total, scaling = [p for p in range(8) if p % world == rank], 0, 0, "strong"
        name = "configs[4]"

    S = a.decode_steps
    voice = np.fromfile(os.path.join(ROOT, "models", "mol.bin"), np.float32)
    prompts = {p: synthetic_prompt(p) for p in range(8)}
    if dist:  # prompt ids + conditioning come from rank 0 (broadcast), results are gathered on rank 0
        import torch
        tt = torch.from_numpy(np.stack([prompts[p] for p in range(8)])).to(dev)
        tv = torch.from_numpy(voice.copy()).to(dev)
        if rank != 0:
            tt.zero_(); tv.zero_()
        dist.broadcast(tt, 0)
        dist.broadcast(tv, 0)
        voice = tv.cpu().numpy()
        prompts = {p: tt[p].cpu().numpy() for p in range(8)}

    load_ms = {}
    placement = {"node": -1, "cpulist": "", "cpus": 0}  # NUMA node of this rank's GPU / CPUs the rank was pinned to (0: not pinned)
    if a.dry_engine:
        eng = pkg.Engine.__new__(pkg.Engine)
        eng.L = pkg.lib()
        eng.h = eng.L.tts_create(-1)
    else:
        eng = pkg.Engine(device)  # raises without the HIP library/device: there is no fallback path
        if world > 1:
            # N processes share the host: each rank — its Python thread and the sampler pool it creates — stays on the CPUs of its own GPU's NUMA node (the sampler's
            # top-k lists and the logits fallback rows arrive in pinned memory next to that GPU), and the pool takes its share of those cores
            placement["cpus"] = eng.pin_to_numa_node()
            ncpu = placement["cpus"] or (os.cpu_count() or 8) // world
            eng.set_option("sampler_threads", max(0, min(7, ncpu - 2)))
        placement["node"], placement["cpulist"] = eng.numa_node()
        # model loads, timed (not part of the metric: weights are resident when the timed region starts; round 6 parallelised the loaders, profiles/r6_cli_wall.txt)
        for _k, _f in (("ar", "ggml-model.bin"), ("diffusion", "ggml-diffusion-model.bin"), ("vocoder", "ggml-vocoder-model.bin")):
            _t0 = time.perf_counter()
            eng.load(**{_k: os.path.join(model_dir, _f)})
            load_ms[_k] = round(1e3 * (time.perf_counter() - _t0), 1)
    if a.no_diff_graph and not a.dry_engine:
        eng.set_option("diff_graph", 0)
    if a.latency_mode and not a.dry_engine:
        eng.set_option("latency_mode", 1)
    for kv in ([] if a.dry_engine else a.engine_option):
        k_, v_ = kv.split("=", 1)
        eng.set_option(k_, float(v_))
    if cand_total:
        eng.set_option("rng_shard_offset", cand0)
        eng.set_option("rng_shard_total", cand_total)

    stage_ms = {"ar": 0.0, "diffusion": 0.0, "vocoder": 0.0}
    shape = {}
    last_pass = []  # per prompt: what the stages of the latest pass returned (--dump-outputs)

    def one_pass(it, record=True):
        audio_s, n_audio = 0.0, 0
        chunks = []
        pass_out = []
        for p in my_prompts:
            # config 3: distinct candidates per rank and per pass; configs 4/5: one seed for the whole (sharded) batch
            eng.seed(1000 * it + (rank if a.config == 3 else 17 * p))
            if a.dry_engine:  # plumbing only: the host sampler on fixed logits stands in for the three stages
                logits = np.random.RandomState(7).randn(B, 8194).astype(np.float32) * 3
                ids = eng.sample(logits, np.tile(np.array([1] * 17 + [8192], np.int32), (B, 1)))
                audio = [np.full(100 + int(i) % 7, float(i), np.float32) for i in ids]
                rows, Ts = np.full(B, 200), [870] * B
                shape.update(L=200, T=870, ids=[int(i) for i in ids])
                # one os.write per line: the ranks share stderr, and print() may split a line into several writes that interleave with the other rank's
                os.write(2, ("DRY_IDS rank %d prompt %d pass %d: %s\n" % (rank, p, it, " ".join(str(int(i)) for i in ids))).encode())
                pass_out.append({"codes": ids, "audio": audio})
            else:
                t_a = time.time()
                codes, rows, lats, steps = eng.autoregressive(prompts[p], voice, B, S, mask_stop=True)
                t_b = time.time()
                mels = eng.diffusion(lats, n_steps=n_diff, noise_mode=pkg.NOISE_DEVICE)
                t_c = time.time()
                audio = eng.vocoder(mels, noise_mode=pkg.NOISE_DEVICE)
                t_d = time.time()
                if record:
                    stage_ms["ar"] += 1e3 * (t_b - t_a); stage_ms["diffusion"] += 1e3 * (t_c - t_b); stage_ms["vocoder"] += 1e3 * (t_d - t_c)
                Ts = [m.shape[1] for m in mels]
                shape.update(L=int(rows[0]), T=int(Ts[0]))
                pass_out.append({"codes": codes, "latent_rows": rows, "latents": lats, "mel": mels, "audio": audio})
            audio_s += sum(t * 256 for t in Ts) / 24000.0  # T*256/24000 per candidate (the 10 pad frames are not counted)
            n_audio += sum(len(x) for x in audio)
            chunks += audio
        last_pass[:] = pass_out
        if dist:
            import torch
            flat = torch.from_numpy(np.concatenate(chunks) if chunks else np.zeros(0, np.float32)).to(dev)
            sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
            dist.all_gather(sizes, torch.tensor([flat.numel()], dtype=torch.int64, device=dev))
            mx = int(max(s.item() for s in sizes))
            pad = torch.zeros(mx, device=dev)
            pad[:flat.numel()] = flat
            outs = [torch.zeros(mx, device=dev) for _ in range(world)] if rank == 0 else None
            dist.gather(pad, outs, dst=0)
            if rank == 0:
                shape["gathered_samples"] = int(sum(int(s.item()) for s in sizes))
        return audio_s, n_audio

    def sync():
        if dist:
            dist.barrier()
            if a.backend == "nccl":
                import torch
                torch.cuda.synchronize()
        # every engine call is synchronous (ends with hipStreamSynchronize on its stream)

    per_rank = []

    def timed(steps, share):
        if not a.dry_engine:
            eng.set_option("share_uncond", 1 if share else 0)
        for k in stage_ms:
            stage_ms[k] = 0.0
        sync()
        t0 = time.time()
        audio_s = 0.0
        for k in range(steps):
            audio_s += one_pass(k)[0]
        sync()
        dt = time.time() - t0
        if dist:
            import torch
            mine = torch.tensor([dt, float(placement["node"]), float(placement["cpus"])], dtype=torch.float64, device=dev)
            every = [torch.zeros(3, dtype=torch.float64, device=dev) for _ in range(world)]
            dist.all_gather(every, mine)  # every rank's own time: a straggler is visible in the line, not only the maximum
            per_rank.clear()
            per_rank.extend({"rank": r, "ms_per_step": round(1e3 * float(e[0].item()) / steps, 2), "numa_node": int(e[1].item()), "pinned_cpus": int(e[2].item())}
                            for r, e in enumerate(every))
            t = torch.tensor([dt, 0.0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t[0].item())
            s = torch.tensor([audio_s], dtype=torch.float64, device=dev)
            dist.all_reduce(s, op=dist.ReduceOp.SUM)
            audio_s = float(s.item())
        return audio_s, dt, {k: round(v / steps, 1) for k, v in stage_ms.items()}

    share = not a.no_share_uncond
    for w in range(a.warmup):
        one_pass(-1 - w, record=False)
    if a.full and not a.dry_engine:
        # 1 GEMM launch in 13 is bracketed by a HIP event pair (a hash of each shape class's launch counter decides: every launch position is sampled
        # equally often whatever the number of launches per step — round 5: with exactly 13 QKV launches per step a plain stride of 13 bracketed the same
        # layer every time). An event pair drains the pipeline around its launch: bracketing all ~9 600 launches of the timed region cost 5 % of the pass,
        # 1 in 7 0.5 %, 1 in 29 nothing measurable. The decode step is ONE hipGraph replay per event pair.
        for fam in GEMM_FAMILIES:
            eng.set_option("prof_only:" + fam, 1)
        eng.set_option("prof_only:ar_decode_step", 1)
        eng.set_option("prof_stride", a.prof_stride)
        eng.prof_reset(True)
    audio_s, dt, stages = timed(a.steps, share)
    dumped = dump_outputs(a.dump_outputs, last_pass) if a.dump_outputs and rank == 0 else None
    g_ms = g_n = g_flops = d_ms = d_n = d_bytes = 0.0
    per_kernel = {}
    if a.full and not a.dry_engine:
        per_kernel = {fam: eng.prof_get(fam) for fam in GEMM_FAMILIES}
        g_ms, g_n, g_flops = (sum(v[i] for v in per_kernel.values()) for i in range(3))
        d_ms, d_n, d_bytes = eng.prof_get("ar_decode_step")
    # the other share_uncond setting, one pass, outside the timed region (both numbers belong in the line: the sharing only exists
    # because the masked stop token gives every candidate the same length) — under the SAME profiling setting as the headline pass
    # (event pairs on every 13th GEMM launch, every 8th diffusion step eager), so the two values are comparable
    other = None
    if a.full and not a.no_ab and not a.dry_engine:
        o_audio, o_dt, o_stages = timed(1, not share)
        other = {"uncond_integrator_shared": not share, "value": round(o_audio / o_dt, 3), "ms_per_step": round(1000.0 * o_dt, 2),
                 "stage_ms_per_step": o_stages}
        eng.set_option("share_uncond", 1 if share else 0)  # (rounds 1-4 left the other setting on for the option passes below)
    if a.full and not a.dry_engine:
        eng.prof_reset(False)
    # the reference-precision mode of the diffusion stage (option attn_f32 = 1: F32 AttentionBlock as main.cpp:3848-3875 on split-fp16 MFMA
    # operands + exact SiLU; the parity tests' mode), one pass outside the timed region: what the mode costs
    ref_prec = None
    if world == 1 and a.full and not a.no_ab and not a.dry_engine:
        eng.seed(99)
        _, _, lats_rp, _ = eng.autoregressive(prompts[0], voice, B, S, mask_stop=True)
        times = {}
        for mode, opts in ((0, {"attn_f32": 0}), (1, {"attn_f32": 1}), (2, {"attn_f32": 0, "attn_proj_f16": 1, "lc_attn_f32": 0})):
            for k_, v_ in opts.items():
                eng.set_option(k_, v_)
            eng.diffusion(lats_rp, n_steps=4, noise_mode=pkg.NOISE_DEVICE)  # warm-up of this mode's buffers
            t0 = time.time()
            eng.diffusion(lats_rp, n_steps=n_diff, noise_mode=pkg.NOISE_DEVICE)
            times[mode] = 1e3 * (time.time() - t0)
        for k_, v_ in (("attn_f32", 0), ("attn_proj_f16", 0), ("lc_attn_f32", 1)):
            eng.set_option(k_, v_)
        ref_prec = {"diffusion_ms_attn_f32": round(times[1], 1), "diffusion_ms_default": round(times[0], 1), "ratio": round(times[1] / times[0], 3),
                    "diffusion_ms_all_fp16_block_of_rounds_1_to_4": round(times[2], 1), "default_over_all_fp16": round(times[0] / times[2], 3),
                    "note": "option attn_f32 = 1: QK^T, softmax, PV and proj_out evaluated to f32 accuracy (three fp16 MFMAs per product on hi + lo operand "
                            "pairs) and SiLU with libm expf + IEEE division; the 80-step loop then sits at the distance two f32 evaluations of the reference's graph keep "
                            "from each other (tests/golden/parity_floor.json: gate_f32)"}
    # throughput options ar_weights = 1 (fp16: 0.77 GB instead of 1.54 GB of weights per decode step) and 2 (OCP fp8 e4m3 with a
    # power-of-two scale per output column: 0.39 GB), measured beside the default f32 mode on the same prompt and seed:
    # AR stage time, decode-step bandwidth, first sampled id that differs from the f32 run
    f16 = fp8 = f32_rerun = topk = None
    if world == 1 and a.full and not a.no_ab and not a.dry_engine:
        eng.seed(4242)
        t0 = time.time()
        c32, _, _, _ = eng.autoregressive(prompts[0], voice, B, S, mask_stop=True)
        t32 = time.time() - t0
        # the default f32 mode against ITSELF (same seed, second run): the decode step is deterministic (fixed summation trees, no atomics), so
        # every sampled id must repeat
        eng.seed(4242)
        c32b, _, _, _ = eng.autoregressive(prompts[0], voice, B, S, mask_stop=True)
        d32 = np.argwhere(c32[:, 1:1 + S] != c32b[:, 1:1 + S])
        f32_rerun = {"first_divergent_step_vs_first_f32_run": int(d32[:, 1].min()) if len(d32) else None,
                     "candidates_identical_through_all_steps": int((c32[:, 1:1 + S] == c32b[:, 1:1 + S]).all(axis=1).sum())}
        # option device_topk (default 1: the sampler's top-k runs on the device, lists instead of logits cross PCIe) against 0 (the reference's
        # full-logits hand-over): same seed -> the codes must be identical; each setting is timed on its second call (the first re-captures the graph)
        tk = {}
        for on in (0, 1):
            eng.set_option("device_topk", on)
            for rep in range(2):
                eng.seed(4242)
                t0 = time.time()
                ck, _, _, _ = eng.autoregressive(prompts[0], voice, B, S, mask_stop=True)
                tk[on] = time.time() - t0
            if on == 0:
                c_off = ck
        topk = {"ar_stage_ms_device_topk": round(1e3 * tk[1], 1), "ar_stage_ms_full_logits": round(1e3 * tk[0], 1),
                "codes_identical": bool((ck == c_off).all() and (ck == c32).all()), "full_row_fallbacks": int(eng.topk_fallbacks()),
                "d2h_bytes_per_step": {"device_topk": B * 1040, "full_logits": B * 8194 * 4}}
        reports = {}
        for mode, tag in ((1, "f16"), (2, "fp8")):
            e2 = pkg.Engine(device)
            e2.set_option("ar_weights", mode)
            e2.load(ar=os.path.join(model_dir, "ggml-model.bin"))
            e2.seed(4242)
            e2.autoregressive(prompts[0], voice, B, S, mask_stop=True)  # warm-up (graph capture, pinned buffers)
            e2.set_option("prof_only:ar_decode_step", 1)
            e2.prof_reset(True)
            e2.seed(4242)
            t0 = time.time()
            cq, _, _, _ = e2.autoregressive(prompts[0], voice, B, S, mask_stop=True)
            tq = time.time() - t0
            q_ms, q_n, q_bytes = e2.prof_get("ar_decode_step")
            e2.close()
            diff = np.argwhere(c32[:, 1:1 + S] != cq[:, 1:1 + S])
            first = int(diff[:, 1].min()) if len(diff) else None
            reports[tag] = {"ar_stage_ms_f32": round(1e3 * t32, 1), "ar_stage_ms_%s" % tag: round(1e3 * tq, 1),
                            "decode_step_us_%s" % tag: round(1e3 * q_ms / max(q_n, 1), 1),
                            "decode_gbs_%s" % tag: round(q_bytes / max(q_ms, 1e-9) / 1e6, 1), "first_divergent_step_vs_f32": first,
                            "candidates_identical_through_all_steps": int((c32[:, 1:1 + S] == cq[:, 1:1 + S]).all(axis=1).sum()),
                            "note": {"f16": "fp16 decode weights change the logits by ~1e-3",
                                     "fp8": "fp8 e4m3 decode weights change the logits by ~5e-2"}[tag] +
                                    ": sampled ids follow the f32 run until the first draw that lands on the other side of a CDF edge"}
        f16, fp8 = reports["f16"], reports["fp8"]
    # ---- what a real batch looks like, outside the headline's timed region like the other A/B passes -------------------------
    ragged = single_ms = single_lat = first_audio = clvp = None
    if world == 1 and a.full and not a.no_ab and not a.dry_engine and a.config == 3:
        eng.set_option("share_uncond", 1)
        # (a) RAGGED batch: trained weights stop every candidate at its own step (main.cpp:5188-5249); random-init ones never stop, so a stop SCHEDULE
        # (tts_ar_set_stop_schedule) ends candidate b after 0.61 S .. S codes. Decode steps then carry retired candidates (TTS_AR_RETIRE), the latent pass,
        # the diffusion row space (no two unconditioned sequences of one length to share) and the vocoder batch have B different lengths.
        stop_at = [int(round(S * (0.61 + 0.39 * b / max(1, B - 1)))) for b in range(B)]
        eng.set_stop_schedule(stop_at)
        try:
            for rep in range(2):  # the first pass sizes the buffers and captures the graphs of these shapes
                eng.seed(777)
                t_a = time.time()
                codes_r, rows_r, lats_r, steps_r = eng.autoregressive(prompts[0], voice, B, S, mask_stop=True, retire=True)
                t_b = time.time()
                mels_r = eng.diffusion(lats_r, n_steps=n_diff, noise_mode=pkg.NOISE_DEVICE)
                t_c = time.time()
                eng.vocoder(mels_r, noise_mode=pkg.NOISE_DEVICE)
                t_d = time.time()
        finally:
            eng.set_stop_schedule(None)
        Ts_r = [int(m.shape[1]) for m in mels_r]
        aud_r = sum(t * 256 for t in Ts_r) / 24000.0
        ragged = {"value": round(aud_r / (t_d - t_a), 3), "unit": "audio-seconds/sec", "ms_per_step": round(1e3 * (t_d - t_a), 2),
                  "stage_ms": {"ar": round(1e3 * (t_b - t_a), 1), "diffusion": round(1e3 * (t_c - t_b), 1), "vocoder": round(1e3 * (t_d - t_c), 1)},
                  "codes_per_candidate": stop_at, "latent_rows": [int(r) for r in rows_r], "mel_frames": Ts_r, "decode_iterations": int(steps_r),
                  "audio_seconds": round(aud_r, 3),
                  "note": "16 candidates stopped by schedule after 0.61 S .. S codes (TTS_AR_MASK_STOP | TTS_AR_RETIRE): ragged decode, latent pass, diffusion and "
                          "vocoder shapes; second of two passes. tests/test_ragged_gpu.py: every candidate of this batch equals the candidate run alone"}
        # (b) ONE utterance (what ./tortoise runs, main.cpp:6570), (c) time to the first audio: AR + the whole diffusion loop (GroupNorm and attention are global
        # over the utterance: no chunked diffusion) + ONE vocoder window of 32 frames (tts_vocoder_chunk, 0.34 s of audio) instead of the full vocoder pass
        def one_utterance(reps):
            out = []
            for rep in range(reps):
                eng.seed(31)
                t_a = time.time()
                _, _, lats_1, _ = eng.autoregressive(prompts[0], voice, 1, S, mask_stop=True)
                t_b = time.time()
                mels_1 = eng.diffusion(lats_1, n_steps=n_diff, noise_mode=pkg.NOISE_DEVICE)
                t_c = time.time()
                eng.vocoder(mels_1, noise_mode=pkg.NOISE_DEVICE)
                t_d = time.time()
                nz1 = np.random.RandomState(3).randn(64, mels_1[0].shape[1] + 10).astype(np.float32)
                t_e = time.time()
                first = eng.vocoder_chunk(mels_1[0], nz1, 0, 32)
                t_f = time.time()
                out.append((t_d - t_a, t_b - t_a, t_c - t_b, t_d - t_c, t_f - t_e))
            return out, first, mels_1
        eng.set_option("latency_mode", 0)
        tl, first, mels_def = one_utterance(3)
        # the same utterance with option latency_mode (GroupNorm statistics from the GEMM epilogues; opt-in: not bit-identical to the batch path, same oracle gates)
        eng.set_option("latency_mode", 1)
        tl_lat, _, mels_lat = one_utterance(3)
        eng.set_option("latency_mode", 1 if a.latency_mode else 0)
        bl = min(tl_lat[1:])
        single_lat = {"ms": round(1e3 * bl[0], 1), "stage_ms": {"ar": round(1e3 * bl[1], 1), "diffusion": round(1e3 * bl[2], 1), "vocoder": round(1e3 * bl[3], 1)},
                      "mel_max_abs_diff_vs_default": float(np.abs(mels_lat[0] - mels_def[0]).max()),
                      "note": "option latency_mode = 1: same seed, same device noise; the mel differs from the default path's by the chaos of 80 steps (both sit inside the "
                              "same oracle gates: tests/test_latency_mode_gpu.py)"}
        best = min(tl[1:])
        single_ms = round(1e3 * best[0], 1)
        first_audio = {"one_utterance_ms": round(1e3 * (best[1] + best[2] + best[4]), 1),
                       "batch_of_%d_ms" % B: round(stages["ar"] + stages["diffusion"] + 1e3 * best[4], 1),
                       "stage_ms_one_utterance": {"ar": round(1e3 * best[1], 1), "diffusion": round(1e3 * best[2], 1), "vocoder_full": round(1e3 * best[3], 1),
                                                  "vocoder_first_window": round(1e3 * best[4], 2)},
                       "first_window": "%d samples = %.3f s of audio (32 frames + halo)" % (len(first), len(first) / 24000.0),
                       "note": "AR stage + all %d diffusion steps + the first tts_vocoder_chunk window; the diffusion loop is not chunked (DESIGN.md section 7)" % n_diff}
        # (d) CLVP re-ranking of the batch (16 candidates only mean something with it; not in the reference): full-size synthetic CLVP weights
        clvp_path = os.path.join(model_dir, "ggml-clvp-model.bin")
        if not os.path.exists(clvp_path + ".done"):
            from tortoise_cpp_amd import synth_weights as sw
            sw.write_clvp(clvp_path, depth=2 if a.quick else 20, seed=1237)
            open(clvp_path + ".done", "w").write("ok")
        eng.load_clvp(clvp_path)
        eng.seed(1000 * (a.steps - 1))
        codes_c, _, _, _ = eng.autoregressive(prompts[0], voice, B, S, mask_stop=True, want_latents=False)
        cl = [codes_c[b, 1:1 + S] for b in range(B)]
        text_c = prompts[0][prompts[0] < 256]
        eng.clvp_score(text_c, cl)
        t0 = time.time()
        for rep in range(3):
            sc = eng.clvp_score(text_c, cl)
        clvp = {"ms": round(1e3 * (time.time() - t0) / 3, 2), "candidates": B, "codes_per_candidate": S, "kept": int(np.argmax(sc)),
                "note": "tts_clvp_score over the batch's codes (two 20-layer encoders, synthetic weights); not part of the metric"}
    if rank != 0:
        if dist:
            dist.destroy_process_group()
        return
    L, T = shape.get("L", 0), shape.get("T", 0)
    n_prompts = len(my_prompts) if a.config != 5 else 8
    out = {
        "metric": "audio-seconds/sec end-to-end (AR+diffusion+vocoder), 16 cands x 80 steps",
        "value": round(audio_s / dt, 3), "unit": "audio-seconds/sec", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(1000.0 * dt / a.steps, 2), "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
        "dtype": "f16 MFMA inputs / f32 accumulate (diffusion, vocoder convs); f32 weights, f16 KV (AR)", "data": "synthetic",
        "config": {"workload": "%s: synthetic 64-token prompt%s (n=66), mol.bin voice, %d AR candidates %s x %d sampled codes (stop token masked: "
                               "L=%d latent rows, T=%d mel frames), %d diffusion steps (cond+uncond batched), UnivNet vocoder; full-size synthetic "
                               "weights%s" % (name, "s (8 distinct)" if a.config == 5 else "", B if a.config != 4 else cand_total,
                                              {3: "per GPU", 4: "in one batch sharded over the GPUs", 5: "per prompt"}[a.config], S, L, T, n_diff,
                                              " [QUICK: reduced layer counts]" if a.quick else ""),
                   "candidates_per_gpu": B * (len(my_prompts) if a.config == 5 else 1), "prompts": n_prompts, "diffusion_steps": n_diff, "decode_steps": S,
                   "parallelism": "candidate-parallel x%d (one process per GPU, replicated weights, RCCL broadcast of prompt/voice + gather of audio)" % world,
                   # the unconditioned branch's integrator layers (input independent of the candidate) are evaluated once per distinct
                   # sequence length; with the stop token masked all candidates have one length (option share_uncond)
                   # arithmetic of the timed diffusion stage: the mode the parity tests gate at the f32-vs-f32 floor
                   "diffusion_arithmetic": "default: fp16 q/k/v/P/attention-output MFMA operands, proj_out on a split-precision (F32-accurate) weight, latent conditioner "
                                           "in reference precision; f32 accumulate everywhere (options attn_f32 = 0, attn_proj_f16 = 0, lc_attn_f32 = 1)",
                   "uncond_integrator_shared": share,
                   "audio_seconds": "T*256/24000 per candidate = %.3f s (SURVEY 8d; the vocoder also emits 10 silent pad frames: %.3f s of samples)"
                                    % (T * 256 / 24000.0, ((T + 10) * 256 - 6) / 24000.0)},
        "stage_ms_per_step": stages,
        # evaluations of the diffusion timestep MLP that disagreed with their repetition (the evaluate-twice guard): 0 unless another
        # process shares this GPU
        "diffusion_time_mlp_retries": (None if a.dry_engine else int(eng.time_mlp_retries())),
        "load_ms": load_ms,
        # the collective backend has seen this many ranks (all_reduce of ones) and rank 0 has gathered this many audio samples in the last pass
        "per_rank": (per_rank if per_rank else [{"rank": 0, "ms_per_step": None, "numa_node": placement["node"], "pinned_cpus": placement["cpus"]}]),
        "collective_ranks": collective_ranks, "collective_backend": (a.backend if dist else None), "gathered_samples": shape.get("gathered_samples"),
    }
    if a.full:
        achieved = g_flops / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0
        dec_gbs = d_bytes / (d_ms * 1e-3) / 1e9 if d_ms > 0 else 0.0
        # HBM bytes per GEMM launch from the committed PMC profile (FETCH_SIZE + WRITE_SIZE, separate rocprofv3 passes, calibration in the
        # file's note); null when the profile is absent. bench.py does not run rocprofv3 itself.
        traffic, traffic_src = None, None
        for prof_name in ("r6_pmc_hbm_traffic.json", "r5_pmc_hbm_traffic.json", "r4_pmc_hbm_traffic.json", "r3_pmc_hbm_traffic.json", "r2_pmc_hbm_traffic.json", "r1_pmc_hbm_traffic.json"):
            try:
                prof = json.load(open(os.path.join(ROOT, "profiles", prof_name)))["kernels"]
                gk = [v for k, v in prof.items() if "gemm_f16" in k]
                traffic = int(sum(v["dispatches"] * v["hbm_bytes_per_launch"] for v in gk) / max(1, sum(v["dispatches"] for v in gk)))
                traffic_src = "profiles/" + prof_name
                break
            except Exception:
                pass
        # second denominator: the fp16 MFMA peak at the shader clock the chip actually sustains under these kernels (PMC pass: GRBM_GUI_ACTIVE
        # over the kernel's duration; 1.95-2.2 GHz under MFMA load against the 2.4 GHz the 2.5 PF figure assumes), launch-weighted over the GEMM kernels
        sus_clk, sus_src = None, None
        for prof_name in ("r6_pmc_mfma_util.json", "r5_pmc_mfma_util.json", "r4_pmc_mfma_util.json"):
            try:
                prof = json.load(open(os.path.join(ROOT, "profiles", prof_name)))["kernels"]
                gk = [v for k, v in prof.items() if "gemm_f16" in k and v.get("dispatches", 0) >= 20]
                sus_clk = sum(v["dispatches"] * v["avg_us"] * v["shader_clock_MHz"] for v in gk) / max(1e-9, sum(v["dispatches"] * v["avg_us"] for v in gk))
                sus_src = "profiles/" + prof_name
                break
            except Exception:
                pass
        dec_traffic, dec_traffic_src = None, None  # L2-miss bytes fetched per decode step (PMC FETCH_SIZE pass over the decode launches, committed profile)
        for prof_name, what in (("r6_pmc_decode_traffic.json", "round-6 pass"), ("r5_pmc_decode_traffic.json", "round-5 pass"), ("r4_pmc_decode_traffic.json", "round-4 kernels"), ("r2_pmc_decode_traffic.json", "round-2 pass: the same slabs are streamed")):
            try:
                dec_traffic = int(json.load(open(os.path.join(ROOT, "profiles", prof_name)))["fetch_bytes_per_step"])
                dec_traffic_src = "profiles/%s (%s)" % (prof_name, what)
                break
            except Exception:
                pass
        out.update({
            "other_share_uncond_setting": other,
            "ar_f32_default_rerun": f32_rerun,
            "ar_device_topk_option": topk,
            "ar_weights_f16_option": f16,
            "ar_weights_fp8_option": fp8,
            "reference_precision_option": ref_prec,
            "ragged_batch": ragged, "single_utterance_ms": single_ms, "single_utterance_latency_mode": single_lat, "first_audio_ms": first_audio, "clvp_ms": clvp,
            "roofline": {"kernel": "gemm_f16_vh_kernel + gemm_f16_conv3_vh_kernel (diffusion convs/projections)", "bound": "mfma",
                         "achieved": round(achieved, 1), "peak": MFMA_F16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / MFMA_F16_DENSE_PEAK_TFLOPS, 4),
                         "sustained_shader_clock_MHz": (round(sus_clk) if sus_clk else None), "sustained_clock_source": sus_src,
                         "frac_of_sustained_clock_peak": (round(achieved / (MFMA_F16_DENSE_PEAK_TFLOPS * sus_clk / 2400.0), 4) if sus_clk else None),
                         "sustained_clock_caveat": "the clock comes from a rocprofv3 PMC pass (GRBM_GUI_ACTIVE / kernel time), and a chip under counter collection clocks "
                                                   "LOWER than in the un-profiled run this line times (1.89-1.95 vs ~2.02 GHz without counters): this fraction is biased high "
                                                   "by a few per cent; `frac` (against the 2.4 GHz peak) is the figure to quote",
                         "traffic": traffic, "traffic_source": traffic_src, "launches_timed": int(g_n),
                         "launch_sampling": "1 launch in %d of every shape class (hashed decimation of the class's launch counter: no period to resonate with the "
                                            "13 / 16 launches per sampling step) is bracketed by HIP events" % a.prof_stride,
                         "avg_launch_us": round(1000.0 * g_ms / max(g_n, 1), 2), "algorithmic_gflop_per_launch": round(g_flops / max(g_n, 1) / 1e9, 2),
                         # per shape class: its own bound = max(MFMA floor at 2.5 PF, algorithmic bytes at the 6.29 TB/s a streaming kernel reaches)
                         "kernels": gemm_kernel_table(per_kernel)},
            "roofline_decode": {"kernel": "AR decode step (one hipGraph replay: 151 kernels streaming every weight once)", "bound": "hbm",
                                "achieved": round(dec_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(dec_gbs / HBM_PEAK_GBS, 4),
                                "traffic": dec_traffic, "traffic_source": dec_traffic_src, "steps_timed": int(d_n), "avg_step_us": round(1000.0 * d_ms / max(d_n, 1), 1),
                                "algorithmic_mb_per_step": round(d_bytes / max(d_n, 1) / 1e6, 1)},
        })
    if dumped is not None:
        out["dump_outputs"] = dumped
    if a.dry_engine:
        out["dry_engine"] = {"ids": shape.get("ids"), "gathered_samples": shape.get("gathered_samples")}
    if world == 1 and a.full and not a.no_cpu_baseline and not a.dry_engine:
        out["cpu_baseline"] = cpu_baseline(model_dir, voice, prompts[0], S, L, n_diff, a.quick)
    print(json.dumps(out))
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
