// Random voices: upstream tortoise-tts' RandomLatentConverter (tortoise/models/random_latent_generator.py with rlg_auto.pth / rlg_diffuser.pth), the model
// get_random_conditioning_latents() runs when a caller gives neither clips nor latents. Part of extras.hip's translation unit (its last line), beside the
// voice encoder; it depends on common.h alone, so the test harness (testlib/rlg_harness.hip) includes it by itself.
//
// The model, stated from memory (upstream's source is not at hand): L - 1 EqualLinear(D, D, lr_mul = 0.1) layers and one plain
// Linear(D, D), on z = randn(1, D). D = 1024 (rlg_auto: the AR conditioning latent) or 2048 (rlg_diffusion: the diffusion conditioning latent), L = 6.
//   EqualLinear:  y = leaky_relu(W' x + b', 0.2) * sqrt(2)   with W' = fl(W * scale), scale = lr_mul / sqrt(D), b' = fl(b * lr_mul)
//   Linear:       y = W x + b
// W' and b' are made ONCE at load, one f32 multiply per element (host_logic.cpp: rlg_fold): the rounding torch's `weight * scale` and `bias * lr_mul`
// perform, so the kernel's operands are upstream's bits. scale, lr_mul, 0.2 and sqrt(2) are constructor constants of upstream, not tensors; D and L are read
// from the tensor names and shapes.
//
// Device path: ONE f32 kernel per layer (rlg_layer_kernel), L dependent launches per side on the context's stream after at most one noise fill
// (rlg_noise_kernel) - no persistent kernel, no barrier across workgroups. The work is weight reads (6 x 4 MB + 6 x 16 MB of f32): a workgroup owns
// RLG_ROWS output rows and one batch tile of RLG_TILE voices, holds the tile's activations in LDS (RLG_TILE * D * 4 bytes: 64 KB at D = 2048, two
// workgroups per CU of gfx950's 160 KB) and reads each of its weight rows ONCE for the whole tile, lanes striding the row with 16-byte loads.
// A voice's dot product is one fixed chain: lane l accumulates elements 4 l + 256 i + {0, 1, 2, 3}, i ascending, with fmaf from 0; the 64 lane sums are
// added in a fixed xor butterfly (32, 16, 8, 4, 2, 1). No float atomics. The chain does not know which slot of the tile the voice sits in, how many voices the
// tile holds or what the other slots hold: a voice's bits depend on its input row only (alone == any position of any batch).
#pragma once
#include "common.h"
#include <cmath>

namespace tts {

constexpr int RLG_TILE = 8;       // voices per batch tile (the harness exports it: tts_rlg_test_tile)
constexpr int RLG_ROWS = 8;       // output rows per workgroup: two per wave
constexpr int RLG_MIN_DIM = 256;  // a row is read as 64 lanes x float4: D is a multiple of 256
constexpr int RLG_MAX_DIM = 2048; // the tile's activations fill 64 KB of LDS at 2048
constexpr int RLG_MAX_VOICES = 4096;
constexpr uint32_t RLG_PHILOX_TAG = 0x7717u; // counter word 3: the diffusion stage has 0x7715, the vocoder 0x7716
inline bool rlg_dim_ok(int64_t D) { return D >= RLG_MIN_DIM && D <= RLG_MAX_DIM && D % 256 == 0; }

namespace {

// Philox4x32-10 + Box-Muller: diffusion.hip's philox_normal with this stage's counter tag. counter = {idx >> 1, 0, side, RLG_PHILOX_TAG}, key = the voice's seed.
__device__ __forceinline__ float rlg_philox_normal(uint64_t seed, uint32_t side, uint32_t idx) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  uint32_t c0 = idx >> 1, c1 = 0u, c2 = side, c3 = RLG_PHILOX_TAG, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const float u1 = ((float)c0 + 1.0f) * 2.3283064365386963e-10f, u2 = (float)c1 * 2.3283064365386963e-10f;
  const float rad = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  return (idx & 1) ? rad * sn : rad * cs;
}

// z[b][i] = normal(seeds[b], side, i): grid (ceil(D / 256), n)
__global__ __launch_bounds__(256) void rlg_noise_kernel(const unsigned long long *__restrict__ seeds, uint32_t side, int D, float *__restrict__ z) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i < D) z[(size_t)b * D + i] = rlg_philox_normal(seeds[b], side, (uint32_t)i);
}

// y[b][o] = act(sum_k w[o][k] x[b][k] + bias[o]) for the voices b of batch tile blockIdx.y and the rows o of blockIdx.x. grid (D / RLG_ROWS, ceil(n / RLG_TILE)),
// 256 threads, RLG_TILE * D * 4 bytes of dynamic LDS. Rows of x at or beyond n are never read; slots beyond n hold zeros and are never stored.
__global__ __launch_bounds__(256) void rlg_layer_kernel(const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ x, int n, int D,
                                                        int act, float *__restrict__ y) {
  extern __shared__ float4 rlg_xs[]; // [RLG_TILE][D / 4]
  constexpr int RW = RLG_ROWS / 4;   // rows per wave
  constexpr int UN = 4;              // row strides whose loads are in flight together
  const int b0 = blockIdx.y * RLG_TILE, nt = min(RLG_TILE, n - b0), D4 = D >> 2;
  for (int i = threadIdx.x; i < RLG_TILE * D4; i += 256) {
    const int t = i / D4;
    rlg_xs[i] = t < nt ? ((const float4 *)(x + (size_t)b0 * D))[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, o0 = blockIdx.x * RLG_ROWS + wave * RW;
  float acc[RW][RLG_TILE];
#pragma unroll
  for (int r = 0; r < RW; r++)
#pragma unroll
    for (int t = 0; t < RLG_TILE; t++) acc[r][t] = 0.f;
  const float4 *wr = (const float4 *)(w + (size_t)o0 * D);
  const int ns = D >> 8; // strides of 64 float4 in a row
  for (int s0 = 0; s0 < ns; s0 += UN) { // UN strides of 64 float4 at a time: their 16-byte loads are all issued before the first is used
    float4 wv[UN][RW];
#pragma unroll
    for (int u = 0; u < UN; u++)
      if (s0 + u < ns) {
#pragma unroll
        for (int r = 0; r < RW; r++) wv[u][r] = wr[(size_t)r * D4 + (s0 + u) * 64 + lane];
      }
#pragma unroll
    for (int u = 0; u < UN; u++)
      if (s0 + u < ns) {
#pragma unroll
        for (int t = 0; t < RLG_TILE; t++) {
          const float4 xv = rlg_xs[t * D4 + (s0 + u) * 64 + lane];
#pragma unroll
          for (int r = 0; r < RW; r++) { // one chain per voice and row: k ascending, x y z w inside a float4
            float a = acc[r][t];
            a = fmaf(wv[u][r].x, xv.x, a);
            a = fmaf(wv[u][r].y, xv.y, a);
            a = fmaf(wv[u][r].z, xv.z, a);
            a = fmaf(wv[u][r].w, xv.w, a);
            acc[r][t] = a;
          }
        }
      }
  }
#pragma unroll
  for (int r = 0; r < RW; r++)
#pragma unroll
    for (int t = 0; t < RLG_TILE; t++) {
      float v = acc[r][t];
#pragma unroll
      for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
      acc[r][t] = v;
    }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RW; r++) {
      const float bv = bias[o0 + r];
#pragma unroll
      for (int t = 0; t < RLG_TILE; t++)
        if (t < nt) {
          float v = acc[r][t] + bv;
          if (act) v = (v > 0.f ? v : v * 0.2f) * 1.41421356237309504880f; // leaky_relu(., 0.2) * sqrt(2)
          y[(size_t)(b0 + t) * D + o0 + r] = v;
        }
    }
  }
}

inline hipError_t rlg_launch_layer(const float *w, const float *bias, const float *x, int n, int D, int act, float *y, hipStream_t s) {
  rlg_layer_kernel<<<dim3((unsigned)(D / RLG_ROWS), (unsigned)((n + RLG_TILE - 1) / RLG_TILE)), 256, (size_t)RLG_TILE * D * sizeof(float), s>>>(w, bias, x, n, D, act, y);
  return hipGetLastError();
}
inline hipError_t rlg_launch_noise(const unsigned long long *seeds, uint32_t side, int n, int D, float *z, hipStream_t s) {
  rlg_noise_kernel<<<dim3((unsigned)((D + 255) / 256), (unsigned)n), 256, 0, s>>>(seeds, side, D, z);
  return hipGetLastError();
}

} // namespace

#ifndef TTS_RLG_KERNELS_ONLY
struct RlgSide {
  int D = 0, L = 0;
  DevBuf w, b; // [L][D][D] folded, [L][D] folded
  DevBuf xa, xb, seeds;
};
struct RandomVoiceState { RlgSide side[2]; }; // 0: auto (AR conditioning latent), 1: diffusion
void random_voice_free(RandomVoiceState *s) { delete s; }

// One side's file -> folded host arrays. TTS_ERR_FORMAT for anything but layers.{0..L-1}.weight [D][D] / .bias [D] with L >= 2, one D for all, D a size the
// kernel takes.
static int rlg_parse(tts_ctx *ctx, const char *path, int &D, int &L, std::vector<float> &w, std::vector<float> &b) {
  WeightFile wf;
  std::string err;
  const int rc = read_weight_file(path, wf, err);
  if (rc != TTS_OK) return fail(ctx, rc, "tts_load_random_voice: %s", err.c_str());
  L = 0;
  while (wf.has("layers." + std::to_string(L) + ".weight")) L++;
  if (L < 2) return fail(ctx, TTS_ERR_FORMAT, "'%s' is not a random-voice file: %d layers.N.weight tensors (at least 2 expected)", path, L);
  const HostTensor &w0 = wf.t["layers.0.weight"];
  D = (int)w0.ne[0];
  if (!rlg_dim_ok(w0.ne[0]))
    return fail(ctx, TTS_ERR_FORMAT, "'%s': %lld channels (a multiple of 256 from %d to %d expected)", path, (long long)w0.ne[0], RLG_MIN_DIM, RLG_MAX_DIM);
  w.resize((size_t)L * D * D);
  b.resize((size_t)L * D);
  for (int l = 0; l < L; l++) {
    const std::string p = "layers." + std::to_string(l);
    const HostTensor &wt = wf.t[p + ".weight"];
    if (wt.n_dims != 2 || wt.ne[0] != wt.ne[1]) return fail(ctx, TTS_ERR_FORMAT, "'%s': %s.weight is not square (%lld x %lld)", path, p.c_str(), (long long)wt.ne[1], (long long)wt.ne[0]);
    if (wt.ne[0] != D) return fail(ctx, TTS_ERR_FORMAT, "'%s': %s.weight has %lld channels, layers.0.weight %d", path, p.c_str(), (long long)wt.ne[0], D);
    if (!wf.has(p + ".bias")) return fail(ctx, TTS_ERR_FORMAT, "'%s': %s.bias is missing", path, p.c_str());
    const HostTensor &bt = wf.t[p + ".bias"];
    if (bt.n_dims != 1 || bt.ne[0] != D) return fail(ctx, TTS_ERR_FORMAT, "'%s': %s.bias has %lld elements, %d expected", path, p.c_str(), (long long)bt.nelem(), D);
    rlg_fold(wt.data.data(), bt.data.data(), D, l < L - 1, w.data() + (size_t)l * D * D, b.data() + (size_t)l * D);
  }
  if ((int)wf.t.size() != 2 * L) return fail(ctx, TTS_ERR_FORMAT, "unknown tensors in random-voice file '%s' (%d tensors, %d expected)", path, (int)wf.t.size(), 2 * L);
  return TTS_OK;
}

// Both files are parsed before the device is asked for: a host-only context tells a broken file (TTS_ERR_FORMAT) from a good one (TTS_ERR_HIP).
int random_voice_load(tts_ctx *ctx, const char *auto_path, const char *diff_path) {
  if (!auto_path && !diff_path) return fail(ctx, TTS_ERR_ARG, "tts_load_random_voice: both paths are NULL");
  const char *paths[2] = {auto_path, diff_path};
  int D[2] = {0, 0}, L[2] = {0, 0};
  std::vector<float> w[2], b[2];
  for (int s = 0; s < 2; s++)
    if (paths[s])
      if (int rc = rlg_parse(ctx, paths[s], D[s], L[s], w[s], b[s])) return rc;
  if (ctx->device < 0) return fail(ctx, TTS_ERR_HIP, "host-only context: no HIP device, no CPU fallback");
  (void)hipSetDevice(ctx->device);
  if (!ctx->rlg) ctx->rlg = new RandomVoiceState();
  for (int s = 0; s < 2; s++) {
    if (!paths[s]) continue;
    RlgSide &sd = ctx->rlg->side[s];
    sd.D = 0; sd.L = 0;
    TTS_HIP(ctx, hipStreamSynchronize(ctx->stream)); // a running call still reads the buffers reserve() may replace
    TTS_HIP(ctx, sd.w.reserve(w[s].size() * 4));
    TTS_HIP(ctx, sd.b.reserve(b[s].size() * 4));
    TTS_HIP(ctx, hipMemcpy(sd.w.p, w[s].data(), w[s].size() * 4, hipMemcpyHostToDevice));
    TTS_HIP(ctx, hipMemcpy(sd.b.p, b[s].data(), b[s].size() * 4, hipMemcpyHostToDevice));
    sd.D = D[s]; sd.L = L[s];
  }
  return TTS_OK;
}

int random_voice_dim(const tts_ctx *ctx, int side) { return (ctx && ctx->rlg && (side == 0 || side == 1)) ? ctx->rlg->side[side].D : 0; }

// the launches of one side for n voices: noise fill or upload of z, then L layers ping-ponging between xa and xb; the result is left in *d_out
static int rlg_side_run(tts_ctx *ctx, RlgSide &sd, uint32_t side, const uint64_t *seeds, int n, const float *z, float **d_out) {
  const int D = sd.D;
  TTS_HIP(ctx, sd.xa.reserve((size_t)n * D * 4));
  TTS_HIP(ctx, sd.xb.reserve((size_t)n * D * 4));
  float *cur = sd.xa.as<float>(), *nxt = sd.xb.as<float>();
  if (z) {
    TTS_HIP(ctx, hipMemcpyAsync(cur, z, (size_t)n * D * 4, hipMemcpyHostToDevice, ctx->stream));
  } else {
    TTS_HIP(ctx, sd.seeds.reserve((size_t)n * 8));
    TTS_HIP(ctx, hipMemcpyAsync(sd.seeds.p, seeds, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    ProfScope ps(ctx, "rlg_noise", (double)n * D * 4);
    TTS_HIP(ctx, rlg_launch_noise(sd.seeds.as<unsigned long long>(), side, n, D, cur, ctx->stream));
  }
  for (int l = 0; l < sd.L; l++) {
    ProfScope ps(ctx, "rlg_layer", (double)D * D * 4 * ((n + RLG_TILE - 1) / RLG_TILE));
    TTS_HIP(ctx, rlg_launch_layer(sd.w.as<float>() + (size_t)l * D * D, sd.b.as<float>() + (size_t)l * D, cur, n, D, l < sd.L - 1, nxt, ctx->stream));
    std::swap(cur, nxt);
  }
  *d_out = cur;
  return TTS_OK;
}

int random_voice_run(tts_ctx *ctx, const uint64_t *seeds, int n, const float *z_auto, const float *z_diff, float *out_auto, float *out_diff) {
  float *outs[2] = {out_auto, out_diff};
  const float *zs[2] = {z_auto, z_diff};
  if (!out_auto && !out_diff) return fail(ctx, TTS_ERR_ARG, "tts_random_voice: both outputs are NULL");
  if (n < 1) return fail(ctx, TTS_ERR_ARG, "tts_random_voice: %d voices", n);
  if (n > RLG_MAX_VOICES) return fail(ctx, TTS_ERR_LIMIT, "tts_random_voice: %d voices (at most %d per call)", n, RLG_MAX_VOICES);
  for (int s = 0; s < 2; s++) {
    if (!outs[s]) continue;
    if (!ctx->rlg || !ctx->rlg->side[s].D) return fail(ctx, TTS_ERR_STATE, "tts_random_voice: the %s side is not loaded (tts_load_random_voice)", s ? "diffusion" : "auto");
    if (!zs[s] && !seeds) return fail(ctx, TTS_ERR_ARG, "tts_random_voice: neither seeds nor z for the %s side", s ? "diffusion" : "auto");
  }
  for (int s = 0; s < 2; s++) {
    if (!outs[s] || !zs[s]) continue;
    const size_t cnt = (size_t)n * ctx->rlg->side[s].D;
    for (size_t i = 0; i < cnt; i++)
      if (!std::isfinite(zs[s][i])) return fail(ctx, TTS_ERR_ARG, "tts_random_voice: z of the %s side holds a non-finite value (voice %d)", s ? "diffusion" : "auto", (int)(i / ctx->rlg->side[s].D));
  }
  float *d_out[2] = {nullptr, nullptr};
  for (int s = 0; s < 2; s++)
    if (outs[s])
      if (int rc = rlg_side_run(ctx, ctx->rlg->side[s], (uint32_t)s, seeds, n, zs[s], &d_out[s])) return rc;
  for (int s = 0; s < 2; s++)
    if (outs[s]) TTS_HIP(ctx, hipMemcpyAsync(outs[s], d_out[s], (size_t)n * ctx->rlg->side[s].D * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TTS_OK;
}

// the generator's output for one seed and side: the row rlg_side_run's noise fill writes for that voice. Returns D.
int random_voice_noise(tts_ctx *ctx, uint64_t seed, int side, float *out, int cap) {
  if (side != 0 && side != 1) return fail(ctx, TTS_ERR_ARG, "tts_random_voice_noise: side %d (0 = auto, 1 = diffusion)", side);
  if (!ctx->rlg || !ctx->rlg->side[side].D) return fail(ctx, TTS_ERR_STATE, "tts_random_voice_noise: the %s side is not loaded (tts_load_random_voice)", side ? "diffusion" : "auto");
  RlgSide &sd = ctx->rlg->side[side];
  if (!out || cap < sd.D) return fail(ctx, TTS_ERR_ARG, "tts_random_voice_noise: room for %d floats, %d needed", out ? cap : 0, sd.D);
  TTS_HIP(ctx, sd.xa.reserve((size_t)sd.D * 4));
  TTS_HIP(ctx, sd.seeds.reserve(8));
  TTS_HIP(ctx, hipMemcpyAsync(sd.seeds.p, &seed, 8, hipMemcpyHostToDevice, ctx->stream));
  TTS_HIP(ctx, rlg_launch_noise(sd.seeds.as<unsigned long long>(), (uint32_t)side, 1, sd.D, sd.xa.as<float>(), ctx->stream));
  TTS_HIP(ctx, hipMemcpyAsync(out, sd.xa.p, (size_t)sd.D * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return sd.D;
}
#endif // TTS_RLG_KERNELS_ONLY

} // namespace tts
