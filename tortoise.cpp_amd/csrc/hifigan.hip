// HiFi-GAN decoder on MI355X (gfx950): autoregressive latents + speaker latent -> 24 kHz waveform      tts_load_hifigan / tts_hifigan_decode / tts_hifigan_chunk
//
// The reference has one decoder (80 diffusion steps + UnivNet). Upstream tortoise-tts has a second one, the api_fast.py path: a HiFi-GAN
// generator taken from XTTS that reads the autoregressive stage's latents and the speaker latent and writes the waveform directly — no
// diffusion, no noise, no vocoder. Upstream's source and weights are NOT available offline: the contract of this file is the arithmetic
// stated in DESIGN.md ("What pins the HiFi-GAN decoder"), checked against a torch restatement (tests/hifigan_ref.py) in float64; like CLVP
// it is unpinned against upstream and pinned between independent implementations. The tensor names are the table in hifigan_load
// = synth_weights.hifigan_tensor_shapes(); correct both when a checkpoint shows different ones.
//
//   z = latents^T [1024][L] -> linear interpolation x 4 -> linear interpolation x 24000 / 22050 (two steps)     T = tts_diffusion_frames(L)
//   conv_pre 1024 -> 512 (k 7) + cond_layer(g) on every frame
//   4 stages (512 -> 256 -> 128 -> 64 -> 32 channels; x 8, 8, 2, 2 in time): leaky_relu(0.1), ConvTranspose1d(stride u, kernel 2u,
//     padding u / 2), then the mean of three ResBlocks (k = 3, 7, 11), each  x += conv2(lrelu(conv1_d(lrelu(x))))  for d = 1, 3, 5
//   leaky_relu(0.01), conv_post 32 -> 1 (k 7), tanh                                                             256 T samples
//
// Device layout: activations are time-major f32 rows [row][channels]; candidate s owns the rows [start_s * R, (start_s + T_s) * R) of a level
// with R rows per frame, start_s a multiple of 8 frames. A tap of a convolution is a row offset; rows outside the candidate read as zero
// (the staging loop predicates them: there are no guard rows to keep clean, and no load or store leaves a candidate's rows).
// Every convolution of the generator is ONE kernel, hfg_conv_kernel: an implicit GEMM  out[t][co] = sum_{tap, ci} act(in[t + lo + tap d][ci]) W[tap][ci][co]
// on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulation), with
//   - the leaky_relu of its input fused into the staging of the operand,
//   - bias, the per-voice conditioning vector, the residual add and the three-ResBlock mean fused into the epilogue,
//   - a transposed convolution run as its u phases: phase p of the output is a 2-tap convolution of the input (grid z), written with row stride u.
// The residual stream stays f32. Operand precision: f32 everywhere. The gate is 1e-3 on the waveform after 4 x (1 + 18) chained convolutions;
// f32 MFMA holds it with two orders of magnitude to spare (measured 4e-6) at 1/16 of the fp16 MFMA rate, and the stage is still 7 x cheaper than the
// diffusion path it replaces (118 against 872 ms for 16 candidates x 9.3 s: profiles/hifigan_decoder.txt). fp16 or split-pair operands for the 256- and 128-channel levels are the next step.
//
// A call is one launch sequence for the whole ragged batch: one upload (latents, voice table, candidate table), 1 + 1 + 1 + 4 x 19 + 1 launches,
// one download. Nothing of it depends on the batch: a candidate's samples are the same bits alone or in any batch.
// tts_hifigan_chunk runs the same sequence over a window of every candidate (hifigan_run); every output element is summed in hfg_conv_kernel's order whatever
// the window and the tile, so the chunks of any partition are the bits of the whole call.
#include "common.h"
#include <cmath>

namespace tts {

namespace {
constexpr int HFG_LAT = 1024, HFG_C0 = 512, HFG_STAGES = 4, HFG_MAX_ROWS = 500, HFG_MAX_CAND = 4096;
constexpr int HFG_UP[HFG_STAGES] = {8, 8, 2, 2};         // stride u of the transposed convolutions (kernel 2 u, padding u / 2)
constexpr int HFG_RK[3] = {3, 7, 11}, HFG_RD[3] = {1, 3, 5}; // ResBlock kernel sizes / dilations of convs1
constexpr int HFG_TM = 256;                              // output rows of a workgroup: 4 waves x 64
constexpr int HFG_TS = 32;                               // output rows of a workgroup of the small-M variant: one MFMA tile, the 4 waves tile the channels
// ints per candidate in the table: {start frame in the buffers, frames evaluated W, voice, L, first latent row, output frames before it, w0, keep0, keep_n}.
// tts_hifigan_decode: W = T, w0 = keep0 = 0, keep_n = T. tts_hifigan_chunk: the window [w0, w0 + W) of the utterance is evaluated (w0 = its absolute first
// frame, which only the interpolation reads) and conv_post writes the frames [keep0, keep0 + keep_n) of the window. Nine, not the eight of the whole-utterance
// table with its two spare ints: the window needs w0 and, for conv_post, which of its frames to keep and how many.
constexpr int HFG_SEQ = 9;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// Receptive field of one output sample, in frames on either side (the halo of tts_hifigan_chunk's window, and what the tests' locality check uses):
// the two interpolations reach 9 frames back from the last latent row ((1.5 + 4 + 1) / 0.91875 + 1.5), conv_pre 3, and stage i adds
// (1 + 60) rows at R_i rows per frame (one input row of the transposed convolution; ResBlock k = 11: sum_d (5 d + 5) = 60 rows), conv_post 3 / 256:
// 9 + 3 + 61 / 8 + 61 / 64 + 61 / 128 + 61 / 256 + 3 / 256 = 21.3.
static_assert(9 + 3 + (61 * 32 + 61 * 4 + 61 * 2 + 61 + 3 + 255) / 256 <= TTS_HFG_HALO_FRAMES, "TTS_HFG_HALO_FRAMES does not cover the receptive field");

struct HfgConv {
  const float *in;    // [rows_in][cin]
  float *out;         // [rows_in * phases][cout]; never the same buffer as `in`
  const float *resid; // null or [rows_out][cout] (may be `out`: an element is read and written by the same thread)
  const float *w;     // [phase][tap][cin][cout]
  const float *bias;  // [cout]
  const float *cbias; // null or [voice][cout]
  const int *seq;     // candidate table
  int cin, cout, taps, dil, lo; // input row of tap j for output row t (phases = 1): t + lo + j dil
  int phases, pad_t;            // phases > 1: transposed convolution of stride `phases`, padding pad_t, 2 taps per phase
  int rate;                     // input rows per frame
  float slope;                  // leaky_relu slope applied to the input (1 = none)
  int acc_mode;                 // 0: out = v, 1: out += v, 2: out = (out + v) / 3
};

// One workgroup: 256 input-rate rows of one candidate x 32 NT output channels (x one phase). A wave owns 64 rows: two 32 x 32 MFMA tiles per
// 32-column group share every weight fragment. The input window (256 + (taps - 1) dil rows) is staged through LDS 32 channels at a time,
// row stride 33 floats (the A fragment reads 32 consecutive rows at one channel: conflict-free); the weights are read from global memory in
// fragment order (32 consecutive output channels per half-wave: 128-byte lines that every workgroup of the launch shares in L2).
template <int NT>
__global__ __launch_bounds__(256) void hfg_conv_kernel(const HfgConv a) {
  extern __shared__ float sx[];
  const int s = blockIdx.y;
  const int f0 = a.seq[HFG_SEQ * s], T = a.seq[HFG_SEQ * s + 1], voice = a.seq[HFG_SEQ * s + 2];
  const int Tin = T * a.rate, t0 = blockIdx.x * HFG_TM;
  if (t0 >= Tin) return;
  const int phase = blockIdx.z % a.phases, n0 = (blockIdx.z / a.phases) * 32 * NT;
  int lo = a.lo;
  const float *w = a.w;
  if (a.phases > 1) { // output row q u + p = in[q + s_p - 1] W[.., k0 + u] + in[q + s_p] W[.., k0], p + pad = s_p u + k0 (the loader stores the two taps in this order)
    lo = (phase + a.pad_t) / a.phases - 1;
    w += (size_t)phase * a.taps * a.cin * a.cout;
  }
  const int win = HFG_TM + (a.taps - 1) * a.dil;
  const float *in = a.in + (size_t)f0 * a.rate * a.cin;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  f32x16 acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;
  for (int c0 = 0; c0 < a.cin; c0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < win * 8; idx += 256) {
      const int r = idx >> 3, q = (idx & 7) * 4, t = t0 + lo + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t >= 0 && t < Tin) v = *(const float4 *)(in + (size_t)t * a.cin + c0 + q);
      float *d = sx + r * 33 + q;
      d[0] = v.x < 0.f ? v.x * a.slope : v.x;
      d[1] = v.y < 0.f ? v.y * a.slope : v.y;
      d[2] = v.z < 0.f ? v.z * a.slope : v.z;
      d[3] = v.w < 0.f ? v.w * a.slope : v.w;
    }
    __syncthreads();
    for (int tap = 0; tap < a.taps; tap++) {
      const float *xr = sx + (wave * 64 + lr + tap * a.dil) * 33 + lk;
      const float *wr = w + (size_t)(tap * a.cin + c0 + lk) * a.cout + n0 + lr;
#pragma unroll 4
      for (int k = 0; k < 32; k += 2) { // lane half lk holds channel c0 + k + lk of both operands
        const float a0 = xr[k], a1 = xr[32 * 33 + k];
#pragma unroll
        for (int n = 0; n < NT; n++) {
          const float b = wr[(size_t)k * a.cout + n * 32];
          acc[0][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0][n], 0, 0, 0);
          acc[1][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1][n], 0, 0, 0);
        }
      }
    }
  }
  const size_t obase = (size_t)f0 * a.rate * a.phases * a.cout;
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int n = 0; n < NT; n++) {
      const int col = n0 + n * 32 + lr;
      float bv = a.bias[col];
      if (a.cbias) bv += a.cbias[(size_t)voice * a.cout + col];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int t = t0 + wave * 64 + m * 32 + 8 * (r >> 2) + 4 * lk + (r & 3); // C/D map of the 32 x 32 MFMA: column on the lane
        if (t < Tin) {
          const size_t o = obase + ((size_t)t * a.phases + phase) * a.cout + col;
          float v = acc[m][n][r] + bv;
          if (a.resid) v += a.resid[o];
          if (a.acc_mode == 1) v += a.out[o];
          else if (a.acc_mode == 2) v = (a.out[o] + v) / 3.0f;
          a.out[o] = v;
        }
      }
    }
}

// The small-M variant (tts_hifigan_chunk's low-rate levels: a streaming window is ~80 frames, 80 rows at conv_pre and 640 in stage 0, where the 256-row tile
// idles most of its waves on a handful of CUs). One workgroup: 32 rows x 128 output channels (x one phase); the four waves tile the CHANNELS, one 32 x 32 MFMA
// tile each, so a short window spreads over 8 x as many row blocks and no wave multiplies rows that are predicated away. Staging (33-float rows, leaky_relu on
// the way in, zero predication), the per-element order (channel chunks ascending, taps, k pairs on the same MFMA with the same lane-half split) and the epilogue
// are hfg_conv_kernel's: every output element is the same chain of the same instructions on the same operands, hence the same bits.
__global__ __launch_bounds__(256) void hfg_conv_small_kernel(const HfgConv a) {
  extern __shared__ float sx[];
  const int s = blockIdx.y;
  const int f0 = a.seq[HFG_SEQ * s], T = a.seq[HFG_SEQ * s + 1], voice = a.seq[HFG_SEQ * s + 2];
  const int Tin = T * a.rate, t0 = blockIdx.x * HFG_TS;
  if (t0 >= Tin) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int phase = blockIdx.z % a.phases, n0 = (blockIdx.z / a.phases) * 128 + wave * 32;
  int lo = a.lo;
  const float *w = a.w;
  if (a.phases > 1) {
    lo = (phase + a.pad_t) / a.phases - 1;
    w += (size_t)phase * a.taps * a.cin * a.cout;
  }
  const int win = HFG_TS + (a.taps - 1) * a.dil;
  const float *in = a.in + (size_t)f0 * a.rate * a.cin;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  for (int c0 = 0; c0 < a.cin; c0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < win * 8; idx += 256) {
      const int r = idx >> 3, q = (idx & 7) * 4, t = t0 + lo + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t >= 0 && t < Tin) v = *(const float4 *)(in + (size_t)t * a.cin + c0 + q);
      float *d = sx + r * 33 + q;
      d[0] = v.x < 0.f ? v.x * a.slope : v.x;
      d[1] = v.y < 0.f ? v.y * a.slope : v.y;
      d[2] = v.z < 0.f ? v.z * a.slope : v.z;
      d[3] = v.w < 0.f ? v.w * a.slope : v.w;
    }
    __syncthreads();
    for (int tap = 0; tap < a.taps; tap++) {
      const float *xr = sx + (lr + tap * a.dil) * 33 + lk;
      const float *wr = w + (size_t)(tap * a.cin + c0 + lk) * a.cout + n0 + lr;
#pragma unroll 8
      for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[k], wr[(size_t)k * a.cout], acc, 0, 0, 0);
    }
  }
  const size_t obase = (size_t)f0 * a.rate * a.phases * a.cout;
  const int col = n0 + lr;
  float bv = a.bias[col];
  if (a.cbias) bv += a.cbias[(size_t)voice * a.cout + col];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int t = t0 + 8 * (r >> 2) + 4 * lk + (r & 3);
    if (t < Tin) {
      const size_t o = obase + ((size_t)t * a.phases + phase) * a.cout + col;
      float v = acc[r] + bv;
      if (a.resid) v += a.resid[o];
      if (a.acc_mode == 1) v += a.out[o];
      else if (a.acc_mode == 2) v = (a.out[o] + v) / 3.0f;
      a.out[o] = v;
    }
  }
}

// z[t][c] of every candidate: F.interpolate(scale_factor = 4, linear, align_corners = False) then the same with 24000 / 22050 on the result
// (source position (dst + 0.5) / scale - 0.5 clamped at 0, upper neighbour clamped at the last element: 1 / scale = 0.25 and 0.91875)
__global__ __launch_bounds__(256) void hfg_interp_kernel(const float *__restrict__ lat, const int *__restrict__ seq, float *__restrict__ z) {
  const int s = blockIdx.y, t = blockIdx.x;
  const int f0 = seq[HFG_SEQ * s], T = seq[HFG_SEQ * s + 1], L = seq[HFG_SEQ * s + 3];
  if (t >= T) return;
  const float *lp = lat + (size_t)seq[HFG_SEQ * s + 4] * HFG_LAT;
  const int ta = seq[HFG_SEQ * s + 6] + t; // the frame's index in the whole utterance: a frame is a function of it and of L alone, so a window needs no halo here
  const float src2 = fmaxf(((float)ta + 0.5f) * 0.91875f - 0.5f, 0.f);
  const int i0 = min((int)src2, 4 * L - 1), i1 = min(i0 + 1, 4 * L - 1);
  const float l2 = src2 - (float)i0;
  const float sa = fmaxf(((float)i0 + 0.5f) * 0.25f - 0.5f, 0.f), sb = fmaxf(((float)i1 + 0.5f) * 0.25f - 0.5f, 0.f);
  const int a0 = min((int)sa, L - 1), a1 = min(a0 + 1, L - 1), b0 = min((int)sb, L - 1), b1 = min(b0 + 1, L - 1);
  const float la = sa - (float)a0, lb = sb - (float)b0;
  for (int c = threadIdx.x; c < HFG_LAT; c += 256) {
    const float va = (1.0f - la) * lp[(size_t)a0 * HFG_LAT + c] + la * lp[(size_t)a1 * HFG_LAT + c];
    const float vb = (1.0f - lb) * lp[(size_t)b0 * HFG_LAT + c] + lb * lp[(size_t)b1 * HFG_LAT + c];
    z[((size_t)f0 + t) * HFG_LAT + c] = (1.0f - l2) * va + l2 * vb;
  }
}

// cond[v][co] = cond_layer(g_v): one wave per output channel
__global__ __launch_bounds__(256) void hfg_cond_kernel(const float *__restrict__ w /*[512][1024]*/, const float *__restrict__ b, const float *__restrict__ g,
                                                       float *__restrict__ cond) {
  const int co = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, v = blockIdx.y;
  float sum = 0.f;
  for (int c = lane; c < HFG_LAT; c += 64) sum += w[(size_t)co * HFG_LAT + c] * g[(size_t)v * HFG_LAT + c];
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) cond[(size_t)v * HFG_C0 + co] = sum + b[co];
}

// audio = tanh(conv_post(leaky_relu(x, 0.01))): 32 -> 1 channels, k 7; one thread per sample (224 multiply-adds: the stage is bound by reading x).
// Only the kept frames of the evaluated window are written (the whole utterance for tts_hifigan_decode).
__global__ __launch_bounds__(256) void hfg_post_kernel(const float *__restrict__ x, const float *__restrict__ w /*[7][32]*/, const float *__restrict__ b,
                                                       const int *__restrict__ seq, float *__restrict__ audio) {
  __shared__ float sw[7 * 32];
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], T = seq[HFG_SEQ * s + 1], before = seq[HFG_SEQ * s + 5], keep0 = seq[HFG_SEQ * s + 7], keep_n = seq[HFG_SEQ * s + 8];
  const int n = T * 256, j = blockIdx.x * 256 + threadIdx.x, t = keep0 * 256 + j;
  if ((int)blockIdx.x >= keep_n) return;
  if (threadIdx.x < 7 * 32) sw[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  const float *xp = x + (size_t)f0 * 256 * 32;
  float sum = b[0];
  for (int tap = 0; tap < 7; tap++) {
    const int ti = t + tap - 3;
    if (ti < 0 || ti >= n) continue;
    const float4 *xr = (const float4 *)(xp + (size_t)ti * 32);
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const float4 v = xr[q];
      const float *wq = sw + tap * 32 + q * 4;
      sum += (v.x < 0.f ? v.x * 0.01f : v.x) * wq[0];
      sum += (v.y < 0.f ? v.y * 0.01f : v.y) * wq[1];
      sum += (v.z < 0.f ? v.z * 0.01f : v.z) * wq[2];
      sum += (v.w < 0.f ? v.w * 0.01f : v.w) * wq[3];
    }
  }
  audio[(size_t)before * 256 + j] = tanhf(sum);
}
} // namespace
} // namespace tts
#include "model_io.h" // ModelReader, DevWeights, the level tables and the clip ingest of every model of this translation unit
namespace tts {

struct HifiganState {
  HfgLayer pre, cond, post, ups[HFG_STAGES], c1[HFG_STAGES][3][3], c2[HFG_STAGES][3][3];
  DevWeights dev;
  DevBuf in, z, cb, x, u, t, m, audio;
};
void hifigan_free(HifiganState *s) { delete s; }

// Every tensor is uploaded as it is parsed: a broken file reports whichever fails first, the tensor or an upload before it.
int hifigan_load(tts_ctx *ctx, const char *path) {
  WeightFile wf;
  std::string err;
  int rc = read_weight_file(path, wf, err);
  if (rc != TTS_OK) return fail(ctx, rc, "hifigan_load: %s", err.c_str());
  if (!wf.has("hifigan.conv_pre.weight")) return fail(ctx, TTS_ERR_FORMAT, "'%s' is not a HiFi-GAN model file", path);
  std::unique_ptr<HifiganState> st(new HifiganState());
  ModelReader rd{wf, ctx, "HiFi-GAN"};
  HostLayer h;
  auto conv = [&](const std::string &p, int cout, int cin, int k, HfgLayer &l) -> int {
    const int e = rd.conv(p, cout, cin, k, h);
    return e ? e : st->dev.up(ctx, h, l);
  };
  if ((rc = conv("hifigan.conv_pre", HFG_C0, HFG_LAT, 7, st->pre))) return rc;
  // cond_layer stays [cout][cin]: a matrix-vector product per voice
  if ((rc = rd.raw("hifigan.cond_layer", HFG_C0, HFG_LAT, 1, h)) || (rc = st->dev.up(ctx, h, st->cond))) return rc;
  int ch = HFG_C0;
  for (int i = 0; i < HFG_STAGES; i++) {
    const int u = HFG_UP[i], ku = 2 * u, pad = u / 2, cin = ch, cout = ch / 2;
    const std::string p = "hifigan.ups." + std::to_string(i);
    const HostTensor *w, *b;
    if (!(w = rd.need(p + ".weight", cin, cout, ku)) || !(b = rd.need(p + ".bias", cout, 0, 0))) return TTS_ERR_FORMAT;
    // ConvTranspose1d [cin][cout][ku] -> [phase][2][cin][cout]: tap 0 = kernel index k0 + u (input row q + s_p - 1), tap 1 = k0 (row q + s_p)
    std::vector<float> r((size_t)u * 2 * cin * cout);
    for (int ph = 0; ph < u; ph++) {
      const int k0 = (ph + pad) % u;
      for (int j = 0; j < 2; j++)
        for (int ci = 0; ci < cin; ci++)
          for (int co = 0; co < cout; co++) r[(((size_t)ph * 2 + j) * cin + ci) * cout + co] = w->data[((size_t)ci * cout + co) * ku + k0 + (1 - j) * u];
    }
    if ((rc = st->dev.up(ctx, r, &st->ups[i].w)) || (rc = st->dev.up(ctx, b->data, &st->ups[i].b))) return rc;
    ch = cout;
    for (int j = 0; j < 3; j++)
      for (int n = 0; n < 3; n++) {
        const std::string rb = "hifigan.resblocks." + std::to_string(3 * i + j);
        if ((rc = conv(rb + ".convs1." + std::to_string(n), ch, ch, HFG_RK[j], st->c1[i][j][n]))) return rc;
        if ((rc = conv(rb + ".convs2." + std::to_string(n), ch, ch, HFG_RK[j], st->c2[i][j][n]))) return rc;
      }
  }
  // conv_post [1][32][7] -> [7][32]
  if ((rc = conv("hifigan.conv_post", 1, 32, 7, st->post)) || (rc = rd.finish(path))) return rc;
  if (ctx->hifigan) hifigan_free(ctx->hifigan);
  ctx->hifigan = st.release();
  return TTS_OK;
}

// tts_hifigan_decode (frame0 == n_frames == nullptr: every candidate's whole utterance, the 256-row tile everywhere) and tts_hifigan_chunk (candidate c's
// frames [frame0[c], frame0[c] + n_frames[c]): the window of TTS_HFG_HALO_FRAMES more on either side, clipped to the utterance, goes through the same launch
// sequence as a sequence of its own; where the window touches an end of the utterance the convolutions' zero predication IS the boundary condition, at a cut it
// is wrong within the halo only, and conv_post does not write the halo).
static int hifigan_run(tts_ctx *ctx, const char *who, const float *latents, const int32_t *rows, int B, const float *voices, int n_voices, const int32_t *voice_of,
                       const int32_t *frame0, const int32_t *n_frames, float *audio_out) {
  HifiganState *st = ctx->hifigan;
  const bool chunk = frame0 != nullptr;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_hifigan not called");
  if (!latents || !rows || !voices || !audio_out || B < 1) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", who);
  if (n_voices < 1 || n_voices > (1 << 20)) return fail(ctx, TTS_ERR_ARG, "%s: %d voices", who, n_voices);
  if (B > HFG_MAX_CAND) return fail(ctx, TTS_ERR_LIMIT, "%s: %d candidates (at most %d per call)", who, B, HFG_MAX_CAND);
  std::vector<int> seq((size_t)HFG_SEQ * B, 0);
  int64_t lat_rows = 0, frames = 0, fpad = 0, wframes = 0;
  int maxW = 0, maxKeep = 0;
  for (int c = 0; c < B; c++) {
    if (rows[c] < 1) return fail(ctx, TTS_ERR_ARG, "%s: candidate %d has %d latent rows", who, c, rows[c]);
    if (rows[c] > HFG_MAX_ROWS) return fail(ctx, TTS_ERR_LIMIT, "%s: candidate %d has %d latent rows (at most %d)", who, c, rows[c], HFG_MAX_ROWS);
    const int v = voice_of ? voice_of[c] : 0;
    if (v < 0 || v >= n_voices) return fail(ctx, TTS_ERR_ARG, "%s: candidate %d names voice %d of %d", who, c, v, n_voices);
    const int T = tts_diffusion_frames(rows[c]);
    int w0 = 0, w1 = T, keep0 = 0, keep_n = T;
    if (chunk) {
      if (frame0[c] < 0 || n_frames[c] < 1) return fail(ctx, TTS_ERR_ARG, "%s: candidate %d asks for %d frames from frame %d", who, c, n_frames[c], frame0[c]);
      if ((int64_t)frame0[c] + n_frames[c] > T)
        return fail(ctx, TTS_ERR_ARG, "%s: candidate %d asks for frames [%d, %lld) of %d", who, c, frame0[c], (long long)frame0[c] + n_frames[c], T);
      w0 = std::max(0, frame0[c] - TTS_HFG_HALO_FRAMES); w1 = std::min(T, frame0[c] + n_frames[c] + TTS_HFG_HALO_FRAMES);
      keep0 = frame0[c] - w0; keep_n = n_frames[c];
    }
    const int W = w1 - w0;
    int *q = &seq[(size_t)HFG_SEQ * c];
    q[0] = (int)fpad; q[1] = W; q[2] = v; q[3] = rows[c]; q[4] = (int)lat_rows; q[5] = (int)frames; q[6] = w0; q[7] = keep0; q[8] = keep_n;
    lat_rows += rows[c]; frames += keep_n; wframes += W; fpad += (W + 7) / 8 * 8; maxW = std::max(maxW, W); maxKeep = std::max(maxKeep, keep_n);
  }
  const size_t n_lat = (size_t)lat_rows * HFG_LAT, n_voice = (size_t)n_voices * HFG_LAT;
  for (size_t i = 0; i < n_lat; i++)
    if (!std::isfinite(latents[i])) return fail(ctx, TTS_ERR_ARG, "%s: latent row %d holds a non-finite value", who, (int)(i / HFG_LAT));
  for (size_t i = 0; i < n_voice; i++)
    if (!std::isfinite(voices[i])) return fail(ctx, TTS_ERR_ARG, "%s: voice %d holds a non-finite value", who, (int)(i / HFG_LAT));
  // one upload: latents | voice table | candidate table
  std::vector<float> up(n_lat + n_voice + seq.size());
  memcpy(up.data(), latents, n_lat * 4);
  memcpy(up.data() + n_lat, voices, n_voice * 4);
  memcpy(up.data() + n_lat + n_voice, seq.data(), seq.size() * 4);
  const size_t act = (size_t)fpad * 8192; // floats of one activation buffer: 8 x 256, 64 x 128, 128 x 64 and 256 x 32 per frame are all <= 8192
  TTS_HIP(ctx, st->in.reserve(up.size() * 4));
  TTS_HIP(ctx, st->z.reserve((size_t)fpad * HFG_LAT * 4));
  TTS_HIP(ctx, st->cb.reserve(n_voices * (size_t)HFG_C0 * 4));
  TTS_HIP(ctx, st->x.reserve(act * 4));
  TTS_HIP(ctx, st->u.reserve(act * 4));
  TTS_HIP(ctx, st->t.reserve(act * 4));
  TTS_HIP(ctx, st->m.reserve(act * 4));
  TTS_HIP(ctx, st->audio.reserve((size_t)frames * 256 * 4));
  TTS_HIP(ctx, hipMemcpyAsync(st->in.p, up.data(), up.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  const float *d_lat = st->in.as<float>(), *d_voice = d_lat + n_lat;
  const int *d_seq = (const int *)(d_voice + n_voice);
  float *z = st->z.as<float>(), *cb = st->cb.as<float>(), *x = st->x.as<float>(), *u = st->u.as<float>(), *t = st->t.as<float>(), *m = st->m.as<float>();
  hfg_interp_kernel<<<dim3(maxW, B), 256, 0, ctx->stream>>>(d_lat, d_seq, z);
  hfg_cond_kernel<<<dim3(HFG_C0 / 4, n_voices), 256, 0, ctx->stream>>>(st->cond.w, st->cond.b, d_voice, cb);
  // Option "hfg_small_m": a chunked call runs a convolution on the small-M variant when its longest window has at most that many rows at the convolution's
  // level and the output channels fill the four waves (0: never). The whole-utterance call keeps the 256-row tile.
  const int small_rows = chunk ? ctx->hfg_small_m : 0;
  auto conv = [&](const float *in, float *out, const float *resid, const HfgLayer &l, int cin, int cout, int taps, int dil, int phases, int rate, float slope,
                  int acc_mode, const float *cbias) {
    HfgConv a{};
    a.in = in; a.out = out; a.resid = resid; a.w = l.w; a.bias = l.b; a.cbias = cbias; a.seq = d_seq;
    a.cin = cin; a.cout = cout; a.taps = taps; a.dil = dil; a.lo = -dil * (taps - 1) / 2; a.phases = phases; a.pad_t = phases / 2; a.rate = rate;
    a.slope = slope; a.acc_mode = acc_mode;
    ProfScope ps(ctx, "hfg_conv", 2.0 * (double)wframes * rate * phases * taps * cin * cout);
    if (cout % 128 == 0 && (int64_t)maxW * rate <= small_rows) {
      const dim3 grid((unsigned)(((size_t)maxW * rate + HFG_TS - 1) / HFG_TS), (unsigned)B, (unsigned)(cout / 128 * phases));
      hfg_conv_small_kernel<<<grid, 256, (size_t)(HFG_TS + (taps - 1) * dil) * 33 * 4, ctx->stream>>>(a);
      return;
    }
    const int nt = cout >= 64 ? 2 : 1;
    const dim3 grid((unsigned)(((size_t)maxW * rate + HFG_TM - 1) / HFG_TM), (unsigned)B, (unsigned)(cout / (32 * nt) * phases));
    const size_t lds = (size_t)(HFG_TM + (taps - 1) * dil) * 33 * 4;
    if (nt == 2) hfg_conv_kernel<2><<<grid, 256, lds, ctx->stream>>>(a);
    else hfg_conv_kernel<1><<<grid, 256, lds, ctx->stream>>>(a);
  };
  conv(z, x, nullptr, st->pre, HFG_LAT, HFG_C0, 7, 1, 1, 1, 1.0f, 0, cb);
  const float *cur = x;
  int ch = HFG_C0, rate = 1;
  for (int i = 0; i < HFG_STAGES; i++) {
    conv(cur, u, nullptr, st->ups[i], ch, ch / 2, 2, 1, HFG_UP[i], rate, 0.1f, 0, nullptr);
    ch /= 2; rate *= HFG_UP[i];
    for (int j = 0; j < 3; j++) {
      const float *r = u; // the ResBlock's stream: u for the first dilation, then x
      for (int n = 0; n < 3; n++) {
        conv(r, t, nullptr, st->c1[i][j][n], ch, ch, HFG_RK[j], HFG_RD[n], 1, rate, 0.1f, 0, nullptr);
        if (n < 2) conv(t, x, r, st->c2[i][j][n], ch, ch, HFG_RK[j], 1, 1, rate, 0.1f, 0, nullptr);
        else conv(t, m, r, st->c2[i][j][n], ch, ch, HFG_RK[j], 1, 1, rate, 0.1f, j, nullptr); // the mean of the three ResBlocks: =, +=, (+) / 3
        r = x;
      }
    }
    cur = m;
  }
  hfg_post_kernel<<<dim3(maxKeep, B), 256, 0, ctx->stream>>>(cur, st->post.w, st->post.b, d_seq, st->audio.as<float>());
  TTS_HIP(ctx, hipGetLastError());
  TTS_HIP(ctx, hipMemcpyAsync(audio_out, st->audio.p, (size_t)frames * 256 * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TTS_OK;
}

int hifigan_decode(tts_ctx *ctx, const float *latents, const int32_t *rows, int B, const float *voices, int n_voices, const int32_t *voice_of, float *audio_out) {
  return hifigan_run(ctx, "tts_hifigan_decode", latents, rows, B, voices, n_voices, voice_of, nullptr, nullptr, audio_out);
}

int hifigan_chunk(tts_ctx *ctx, const float *latents, const int32_t *rows, int B, const float *voices, int n_voices, const int32_t *voice_of, const int32_t *frame0,
                  const int32_t *n_frames, float *audio_out) {
  if (!ctx->hifigan) return fail(ctx, TTS_ERR_STATE, "tts_load_hifigan not called");
  if (!frame0 || !n_frames) return fail(ctx, TTS_ERR_ARG, "tts_hifigan_chunk: bad argument");
  return hifigan_run(ctx, "tts_hifigan_chunk", latents, rows, B, voices, n_voices, voice_of, frame0, n_frames, audio_out);
}

} // namespace tts
#include "bigvgan.h"
