// BigVGAN vocoder on MI355X (gfx950): 100-band log-mel -> 24 kHz waveform                         tts_load_bigvgan / tts_bigvgan / tts_bigvgan_config
//
// Included once, as the last line of hifigan.hip (whose host half starts with model_io.h: the tensor reader and the weight store): BigVGAN (v1: bigvgan_base_24khz_100band, bigvgan_24khz_100band) is HiFi-GAN's generator with every
// leaky ReLU replaced by an anti-aliased periodic activation and no activation in front of the transposed convolutions, so its convolutions ARE
// hfg_conv_kernel<1|2> with slope 1, no conditioning vector and voice 0, on HfgConv / HFG_SEQ candidate tables exactly as hifigan_run builds them.
// New here: the mel front end, the activation and conv_post. NVIDIA's source and weights are not available offline: the contract is the arithmetic of
// DESIGN.md ("What pins the BigVGAN vocoder"), checked between two float64 spellings (tests/bigvgan_ref.py); unpinned against upstream.
//
//   x = conv_pre(denorm(mel))                                  100 (padded to 128) -> C0, k 7
//   stage i: x = ConvTranspose1d(x) (stride u_i, kernel 2 u_i, padding u_i / 2; NO activation before it), then the mean over k = 3, 7, 11 of the
//            AMP blocks   x += convs2[n](act[2n+1](convs1[n](act[2n](x))))   n = 0, 1, 2 with dilations 1, 3, 5 on convs1
//   audio = tanh(conv_post(act_post(x)))                       256 T samples
//   act = 2 x up-sample (12-tap Kaiser-windowed sinc, replicate boundary) -> v + sin^2(alpha v) / (beta + 1e-9) -> 2 x down-sample (same filter)
//
// The boundary is replicate for the activation and zero for the convolutions, both at the CANDIDATE's ends: no kernel reads or writes a row outside
// the candidate it works on. Channel counts that are no multiple of 32 (the large model's 48 and 24) are zero-padded at load — weights, biases and
// a = b = 0: snake(0) = 0 and 0 w adds exactly nothing, so the real channels keep their values.
#pragma once

namespace tts {

namespace {
constexpr int BVG_MEL = 100, BVG_MEL_PAD = 128, BVG_MAX_STAGES = 6, BVG_MAX_FRAMES = 4096, BVG_MAX_CAND = 4096;
constexpr int BVG_RUN = 64;     // consecutive rows one thread of bvg_act_kernel walks
constexpr int BVG_ACT_RUNS = 8; // runs of a workgroup: 8 x 32 channels = 256 threads, 512 rows

// kaiser_window(12, beta = 0.1102 (A - 8.7), A = 2.285 * 5 * pi * 1.2 + 7.95) * 0.5 sinc(0.5 t), t = -5.5 .. 5.5, divided by its sum; f[k] = f[11 - k]
__constant__ float BVG_F[12] = {0.0020289664498962f, 0.0093894639440679f, -0.0255434640652947f, -0.0576573754753650f, 0.1285726090813288f, 0.4432098000653667f,
                                0.4432098000653667f, 0.1285726090813288f, -0.0576573754753650f, -0.0255434640652947f, 0.0093894639440679f, 0.0020289664498962f};

// mel [100][T] per candidate (normalised, candidates back to back) -> de-normalised time-major rows [f0 + t][128], channels 100 .. 127 zero
__global__ __launch_bounds__(128) void bvg_mel_kernel(const float *__restrict__ mel, const int *__restrict__ seq, float *__restrict__ out) {
  const int s = blockIdx.y, t = blockIdx.x, ch = threadIdx.x;
  const int f0 = seq[HFG_SEQ * s], T = seq[HFG_SEQ * s + 1];
  if (t >= T) return;
  float v = 0.f;
  if (ch < BVG_MEL) {
    const float MAXV = 2.3143386840820312f, MINV = -11.512925148010254f;
    const float m = mel[(size_t)seq[HFG_SEQ * s + 5] * BVG_MEL + (size_t)ch * T + t]; // seq[5]: frames of the candidates before this one
    v = __fmaf_rn(__fmul_rn(__fadd_rn(m, 1.0f), 0.5f), __fsub_rn(MAXV, MINV), MINV);
  }
  out[((size_t)f0 + t) * BVG_MEL_PAD + ch] = v;
}

__device__ __forceinline__ float bvg_snake(float v, float alpha, float inv_beta) {
  const float sn = sinf(__fmul_rn(alpha, v)); // the accurate sine: alpha v is unbounded on trained weights
  return __fmaf_rn(__fmul_rn(sn, sn), inv_beta, v);
}
// u[2 q] and u[2 q + 1] of the up-sampler from x[q - 3 .. q + 3]; X[i] = x[q - 3 + i] (already clamped to the candidate)
__device__ __forceinline__ float bvg_up_even(const float *X) { // taps f[1], f[3] .. f[11] on x[q + 2] .. x[q - 3]
  float a = __fmul_rn(X[5], BVG_F[1]);
  a = __fmaf_rn(X[4], BVG_F[3], a); a = __fmaf_rn(X[3], BVG_F[5], a); a = __fmaf_rn(X[2], BVG_F[7], a);
  a = __fmaf_rn(X[1], BVG_F[9], a); a = __fmaf_rn(X[0], BVG_F[11], a);
  return __fmul_rn(2.0f, a);
}
__device__ __forceinline__ float bvg_up_odd(const float *X) { // taps f[0], f[2] .. f[10] on x[q + 3] .. x[q - 2]
  float a = __fmul_rn(X[6], BVG_F[0]);
  a = __fmaf_rn(X[5], BVG_F[2], a); a = __fmaf_rn(X[4], BVG_F[4], a); a = __fmaf_rn(X[3], BVG_F[6], a);
  a = __fmaf_rn(X[2], BVG_F[8], a); a = __fmaf_rn(X[1], BVG_F[10], a);
  return __fmul_rn(2.0f, a);
}
__device__ __forceinline__ float bvg_down(const float *S) {
  float a = __fmul_rn(BVG_F[0], S[0]);
#pragma unroll
  for (int k = 1; k < 12; k++) a = __fmaf_rn(BVG_F[k], S[k], a);
  return a;
}

// The activation of rows [t0, t1) of one channel of one candidate (R rows, row stride C floats from xp), handed row by row to put(t, value). With
// cl(i, n) = min(max(i, 0), n - 1):   u[m] = 2 sum_j x[cl(j, R)] f[m + 5 - 2 j]  (m = 0 .. 2 R - 1),   y[t] = sum_k f[k] snake(u[cl(2 t + k - 5, 2 R)]).
// The 11 x values x[t - 5 .. t + 5] and the 12 snake values of the window stay in registers: per output one load, two new u, two sines, one 12-tap dot.
// Every value is the same chain of the same operations whatever t0 is, so a row's bits do not depend on where a run starts. 0 <= t0 < t1 <= R.
template <class Put>
__device__ __forceinline__ void bvg_act_run(const float *__restrict__ xp, int C, int R, int t0, int t1, float al, float ib, Put put) {
  const int last = 2 * R - 1;
  float X[12], S[12]; // X[0] is never read: bvg_up_odd(X) of row t0 - 3 reads x[t0 - 5 .. t0] = X[1 .. 6]
  X[0] = 0.f;
#pragma unroll
  for (int i = 0; i < 11; i++) X[1 + i] = xp[(size_t)min(max(t0 - 5 + i, 0), R - 1) * C];
  // the window of t0: u[2 t0 - 5 .. 2 t0 + 6] = odd(t0 - 3), even and odd of t0 - 2 .. t0 + 2, even(t0 + 3)
  S[0] = bvg_up_odd(X);
#pragma unroll
  for (int q = 0; q < 5; q++) { S[1 + 2 * q] = bvg_up_even(X + 1 + q); S[2 + 2 * q] = bvg_up_odd(X + 1 + q); }
  S[11] = bvg_up_even(X + 6);
#pragma unroll
  for (int k = 0; k < 12; k++) S[k] = bvg_snake(S[k], al, ib);
  // u's clamp: an index below 0 is u[0], one above 2 R - 1 is u[2 R - 1]; both are in the window whenever they are needed
#pragma unroll
  for (int k = 4; k >= 0; k--) if (2 * t0 - 5 + k < 0) S[k] = S[k + 1];
#pragma unroll
  for (int k = 1; k < 12; k++) if (2 * t0 - 5 + k > last) S[k] = S[k - 1];
  for (int t = t0;;) {
    put(t, bvg_down(S));
    if (++t >= t1) break;
#pragma unroll
    for (int i = 1; i < 11; i++) X[i] = X[i + 1];
    X[11] = xp[(size_t)min(t + 5, R - 1) * C];
#pragma unroll
    for (int k = 0; k < 10; k++) S[k] = S[k + 2];
    // u[2 t + 5] = odd(t + 2) and u[2 t + 6] = even(t + 3), both from x[t .. t + 5] = X[6 .. 11]
    const float so = bvg_snake(bvg_up_odd(X + 5), al, ib), se = bvg_snake(bvg_up_even(X + 6), al, ib);
    S[10] = 2 * t + 5 > last ? S[9] : so;
    S[11] = 2 * t + 6 > last ? S[10] : se;
  }
}

// y = Activation1d(SnakeBeta)(x) on time-major f32 rows [row][C] of every candidate. A thread owns a channel (the 32 lanes of a half-wave read one 128-byte
// line of a row) and walks BVG_RUN rows. The clamps are on the candidate's own row range: no row of another candidate (or of the padding between them) is
// read, and only rows of the candidate are written. x and y never alias.
__global__ __launch_bounds__(256) void bvg_act_kernel(const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ alpha,
                                                      const float *__restrict__ inv_beta, const int *__restrict__ seq, int C, int rate) {
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], T = seq[HFG_SEQ * s + 1];
  const int R = T * rate;
  const int t0 = (blockIdx.x * BVG_ACT_RUNS + (threadIdx.x >> 5)) * BVG_RUN;
  if (t0 >= R) return;
  const int c = blockIdx.z * 32 + (threadIdx.x & 31);
  const size_t base = (size_t)f0 * rate * C + c;
  float *yp = y + base;
  bvg_act_run(x + base, C, R, t0, min(t0 + BVG_RUN, R), alpha[c], inv_beta[c], [&](int t, float v) { yp[(size_t)t * C] = v; });
}

// audio = tanh(conv_post(act_post(x))): C -> 1 channels, k 7, at 256 rows per frame. One workgroup per frame, one thread per sample, hfg_post_kernel's
// structure with the anti-aliased Snake where that kernel has its leaky ReLU: the workgroup first evaluates the activation of the frame's 256 + 6 rows,
// 32 channels at a time, into LDS (thread = channel x one of 8 runs of 33 rows, bvg_act_run), then every thread sums its sample's 7 x 32 products.
// Rows outside the candidate are the convolution's zero padding; the activation's replicate clamp is the candidate's too.
constexpr int BVG_POST_ROWS = 256 + 6, BVG_POST_RUN = (BVG_POST_ROWS + 7) / 8;
__global__ __launch_bounds__(256) void bvg_post_kernel(const float *__restrict__ x, const float *__restrict__ w /*[7][C]*/, const float *__restrict__ b,
                                                       const float *__restrict__ alpha, const float *__restrict__ inv_beta, const int *__restrict__ seq,
                                                       float *__restrict__ audio, int C) {
  __shared__ float sa[BVG_POST_ROWS * 33];
  __shared__ float sw[7 * 32];
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], T = seq[HFG_SEQ * s + 1], before = seq[HFG_SEQ * s + 5];
  if ((int)blockIdx.x >= T) return;
  const int n = T * 256, j0 = blockIdx.x * 256, j = j0 + threadIdx.x;
  const int ch = threadIdx.x & 31, run = threadIdx.x >> 5;
  float sum = b[0];
  for (int c0 = 0; c0 < C; c0 += 32) {
    __syncthreads();
    if (threadIdx.x < 7 * 32) sw[threadIdx.x] = w[(threadIdx.x >> 5) * C + c0 + (threadIdx.x & 31)];
    const int r0 = run * BVG_POST_RUN, r1 = min(r0 + BVG_POST_RUN, BVG_POST_ROWS); // LDS rows of this thread; LDS row r is the candidate's row j0 - 3 + r
    const int ta = max(j0 - 3 + r0, 0), tb = min(j0 - 3 + r1, n);
    for (int r = r0; r < r1; r++)
      if (j0 - 3 + r < 0 || j0 - 3 + r >= n) sa[r * 33 + ch] = 0.f;
    if (ta < tb)
      bvg_act_run(x + (size_t)f0 * 256 * C + c0 + ch, C, n, ta, tb, alpha[c0 + ch], inv_beta[c0 + ch], [&](int t, float v) { sa[(t - j0 + 3) * 33 + ch] = v; });
    __syncthreads();
    for (int tap = 0; tap < 7; tap++) {
      const float *ar = sa + (threadIdx.x + tap) * 33, *wr = sw + tap * 32;
#pragma unroll
      for (int q = 0; q < 32; q++) sum = __fmaf_rn(ar[q], wr[q], sum);
    }
  }
  audio[(size_t)before * 256 + j] = tanhf(sum);
}

int bvg_pad32(int c) { return (c + 31) / 32 * 32; }
} // namespace

// The model as the loader's host half leaves it: the configuration read from the tensor shapes, every tensor repacked and zero-padded for the kernels.
// bigvgan_parse makes it without a device call (the tests read its table through a host probe); bigvgan_load uploads it.
using BvgHostAct = HostLayer; // w: alpha = exp(a), b: inv_beta = 1 / (exp(b) + 1e-9), evaluated in double, rounded once
struct BvgHost {
  int c0 = 0, n_stages = 0, up[BVG_MAX_STAGES] = {0, 0, 0, 0, 0, 0};
  int ch[BVG_MAX_STAGES + 1] = {0, 0, 0, 0, 0, 0, 0}; // padded channels: ch[0] after conv_pre, ch[i + 1] after stage i
  HostLayer pre, post, ups[BVG_MAX_STAGES], c1[BVG_MAX_STAGES][3][3], c2[BVG_MAX_STAGES][3][3];
  BvgHostAct act[BVG_MAX_STAGES][3][6], act_post;
};

int bigvgan_parse(tts_ctx *ctx, const WeightFile &wf, const char *path, BvgHost &h) {
  if (!wf.has("bigvgan.conv_pre.weight")) return fail(ctx, TTS_ERR_FORMAT, "'%s' is not a BigVGAN model file", path);
  ModelReader rd{wf, ctx, "BigVGAN"};
  // the configuration: C0 from conv_pre.weight, the stages from the ups.* weights (ConvTranspose1d [cin][cout][2 u])
  {
    const HostTensor *t = rd.peek("bigvgan.conv_pre.weight", 3);
    if (!t || t->ne[2] < 2 || t->ne[2] > 8192) return fail(ctx, TTS_ERR_FORMAT, "tensor 'bigvgan.conv_pre.weight' has wrong shape in BigVGAN model file");
    h.c0 = (int)t->ne[2];
  }
  int64_t prod = 1;
  while (h.n_stages < BVG_MAX_STAGES) {
    const std::string name = "bigvgan.ups." + std::to_string(h.n_stages) + ".0.weight";
    if (!rd.has(name)) break;
    const HostTensor *t = rd.peek(name, 3);
    const int64_t ku = t ? t->ne[0] : 0;
    if (ku < 4 || ku % 4 || ku > 512) return fail(ctx, TTS_ERR_FORMAT, "BigVGAN model file: ups.%d has kernel %d (twice an even stride)", h.n_stages, (int)ku);
    h.up[h.n_stages++] = (int)(ku / 2);
    prod *= ku / 2;
  }
  if (prod != 256) return fail(ctx, TTS_ERR_FORMAT, "BigVGAN model file: the strides of its %d stages multiply to %lld, not to the 256 samples of a mel frame", h.n_stages, (long long)prod);
  if (h.c0 % (1 << h.n_stages)) return fail(ctx, TTS_ERR_FORMAT, "BigVGAN model file: %d channels cannot be halved %d times", h.c0, h.n_stages);
  // every Conv1d through rd.conv: [k][cin_p][cout_p], zero where a padded channel is an operand or a result
  auto act = [&](const std::string &p, int c, int cp, BvgHostAct &a) -> int {
    HostLayer raw; // the file's a and b
    if (rd.vec_pair(p, ".act.alpha", ".act.beta", c, raw)) return TTS_ERR_FORMAT;
    a.w.assign(cp, 1.f); a.b.assign(cp, 1.f); // a = b = 0 on the padded channels (whose input is exactly 0)
    for (int i = 0; i < c; i++) {
      a.w[i] = (float)std::exp((double)raw.w[i]);
      a.b[i] = (float)(1.0 / (std::exp((double)raw.b[i]) + 1e-9));
      if (!std::isfinite(a.w[i]) || !std::isfinite(a.b[i])) return fail(ctx, TTS_ERR_FORMAT, "tensor '%s.act': channel %d has no finite alpha, 1 / beta", p.c_str(), i);
    }
    return TTS_OK;
  };
  int rc;
  h.ch[0] = bvg_pad32(h.c0);
  if ((rc = rd.conv("bigvgan.conv_pre", h.c0, BVG_MEL, 7, h.pre, h.ch[0], BVG_MEL_PAD))) return rc;
  int c = h.c0;
  for (int i = 0; i < h.n_stages; i++) {
    const int u = h.up[i], ku = 2 * u, pad = u / 2, cin = c, cout = c / 2, cinp = h.ch[i], coutp = bvg_pad32(cout);
    h.ch[i + 1] = coutp;
    const std::string p = "bigvgan.ups." + std::to_string(i) + ".0";
    const HostTensor *w, *b;
    if (!(w = rd.need(p + ".weight", cin, cout, ku)) || !(b = rd.need(p + ".bias", cout, 0, 0))) return TTS_ERR_FORMAT;
    // ConvTranspose1d [cin][cout][ku] -> [phase][2][cin_p][cout_p]: tap 0 = kernel index k0 + u (input row q + s_p - 1), tap 1 = k0 (row q + s_p)
    HostLayer &l = h.ups[i];
    l.w.assign((size_t)u * 2 * cinp * coutp, 0.f);
    for (int ph = 0; ph < u; ph++) {
      const int k0 = (ph + pad) % u;
      for (int j = 0; j < 2; j++)
        for (int ci = 0; ci < cin; ci++)
          for (int co = 0; co < cout; co++) l.w[(((size_t)ph * 2 + j) * cinp + ci) * coutp + co] = w->data[((size_t)ci * cout + co) * ku + k0 + (1 - j) * u];
    }
    l.b.assign(coutp, 0.f);
    std::copy(b->data.begin(), b->data.end(), l.b.begin());
    c = cout;
    for (int j = 0; j < 3; j++) {
      const std::string rb = "bigvgan.resblocks." + std::to_string(3 * i + j);
      for (int n = 0; n < 3; n++) {
        if ((rc = rd.conv(rb + ".convs1." + std::to_string(n), c, c, HFG_RK[j], h.c1[i][j][n], coutp, coutp))) return rc;
        if ((rc = rd.conv(rb + ".convs2." + std::to_string(n), c, c, HFG_RK[j], h.c2[i][j][n], coutp, coutp))) return rc;
      }
      for (int n = 0; n < 6; n++)
        if ((rc = act(rb + ".activations." + std::to_string(n), c, coutp, h.act[i][j][n]))) return rc;
    }
  }
  if ((rc = act("bigvgan.activation_post", c, h.ch[h.n_stages], h.act_post))) return rc;
  // conv_post [1][c][7] -> [7][c_p]
  if ((rc = rd.conv("bigvgan.conv_post", 1, c, 7, h.post, 1, h.ch[h.n_stages]))) return rc;
  return rd.finish(path);
}

using BvgAct = HfgLayer; // w: alpha, b: inv_beta
struct BigvganState {
  int c0 = 0, n_stages = 0, up[BVG_MAX_STAGES] = {0, 0, 0, 0, 0, 0}, ch[BVG_MAX_STAGES + 1] = {0, 0, 0, 0, 0, 0, 0};
  HfgLayer pre, post, ups[BVG_MAX_STAGES], c1[BVG_MAX_STAGES][3][3], c2[BVG_MAX_STAGES][3][3];
  BvgAct act[BVG_MAX_STAGES][3][6], act_post;
  DevWeights dev;
  DevBuf in, mel, x, u, t, m, a, audio;
};
void bigvgan_free(BigvganState *s) { delete s; }

int bigvgan_load(tts_ctx *ctx, const char *path) {
  WeightFile wf;
  std::string err;
  int rc = read_weight_file(path, wf, err);
  if (rc != TTS_OK) return fail(ctx, rc, "bigvgan_load: %s", err.c_str());
  std::unique_ptr<BvgHost> h(new BvgHost());
  if ((rc = bigvgan_parse(ctx, wf, path, *h))) return rc;
  std::unique_ptr<BigvganState> st(new BigvganState());
  auto up = [&](const HostLayer &s, HfgLayer &d) { return st->dev.up(ctx, s, d); };
  st->c0 = h->c0; st->n_stages = h->n_stages;
  for (int i = 0; i < BVG_MAX_STAGES; i++) st->up[i] = h->up[i];
  for (int i = 0; i <= BVG_MAX_STAGES; i++) st->ch[i] = h->ch[i];
  if ((rc = up(h->pre, st->pre)) || (rc = up(h->post, st->post)) || (rc = up(h->act_post, st->act_post))) return rc;
  for (int i = 0; i < h->n_stages; i++) {
    if ((rc = up(h->ups[i], st->ups[i]))) return rc;
    for (int j = 0; j < 3; j++) {
      for (int n = 0; n < 3; n++)
        if ((rc = up(h->c1[i][j][n], st->c1[i][j][n])) || (rc = up(h->c2[i][j][n], st->c2[i][j][n]))) return rc;
      for (int n = 0; n < 6; n++)
        if ((rc = up(h->act[i][j][n], st->act[i][j][n]))) return rc;
    }
  }
  if (ctx->bigvgan) bigvgan_free(ctx->bigvgan);
  ctx->bigvgan = st.release();
  return TTS_OK;
}

int bigvgan_config(tts_ctx *ctx, int32_t *out8) {
  const BigvganState *st = ctx->bigvgan;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_bigvgan not called");
  if (!out8) return fail(ctx, TTS_ERR_ARG, "tts_bigvgan_config: bad argument");
  out8[0] = st->c0; out8[1] = st->n_stages;
  for (int i = 0; i < BVG_MAX_STAGES; i++) out8[2 + i] = st->up[i];
  return TTS_OK;
}

// One upload (mel, candidate table), one launch sequence for the whole ragged batch (1 + 1 + sum over the stages of (1 + 18 convolutions + 18 activations) + 1
// launches), one download. Nothing of it depends on the batch: a candidate's samples are the same bits alone or in any batch. The stage owns its buffers and
// touches no AR or diffusion state, so it is legal while sessions are open.
int bigvgan_run(tts_ctx *ctx, const float *mel, const int32_t *frames_in, int B, float *audio_out) {
  BigvganState *st = ctx->bigvgan;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_bigvgan not called");
  if (!mel || !frames_in || !audio_out || B < 1) return fail(ctx, TTS_ERR_ARG, "tts_bigvgan: bad argument");
  if (B > BVG_MAX_CAND) return fail(ctx, TTS_ERR_LIMIT, "tts_bigvgan: %d candidates (at most %d per call)", B, BVG_MAX_CAND);
  std::vector<int> seq((size_t)HFG_SEQ * B, 0);
  int64_t frames = 0, fpad = 0;
  int maxT = 0;
  for (int c = 0; c < B; c++) {
    const int T = frames_in[c];
    if (T < 1) return fail(ctx, TTS_ERR_ARG, "tts_bigvgan: candidate %d has %d frames", c, T);
    if (T > BVG_MAX_FRAMES) return fail(ctx, TTS_ERR_LIMIT, "tts_bigvgan: candidate %d has %d frames (at most %d)", c, T, BVG_MAX_FRAMES);
    int *q = &seq[(size_t)HFG_SEQ * c]; // hifigan_run's record: {start frame, frames, voice 0, -, -, frames before, 0, 0, frames}
    q[0] = (int)fpad; q[1] = T; q[5] = (int)frames; q[8] = T;
    frames += T; fpad += (T + 7) / 8 * 8; maxT = std::max(maxT, T);
  }
  const size_t n_mel = (size_t)frames * BVG_MEL;
  for (size_t i = 0; i < n_mel; i++)
    if (!std::isfinite(mel[i])) return fail(ctx, TTS_ERR_ARG, "tts_bigvgan: the mel holds a non-finite value (element %lld)", (long long)i);
  std::vector<float> up(n_mel + seq.size());
  memcpy(up.data(), mel, n_mel * 4);
  memcpy(up.data() + n_mel, seq.data(), seq.size() * 4);
  size_t per_frame = BVG_MEL_PAD; // floats of one frame at the widest level
  for (int i = 0, r = 1; i <= st->n_stages; i++) {
    per_frame = std::max(per_frame, (size_t)r * st->ch[i]);
    if (i < st->n_stages) r *= st->up[i];
  }
  const size_t act = (size_t)fpad * per_frame;
  TTS_HIP(ctx, st->in.reserve(up.size() * 4));
  TTS_HIP(ctx, st->mel.reserve((size_t)fpad * BVG_MEL_PAD * 4));
  TTS_HIP(ctx, st->x.reserve(act * 4));
  TTS_HIP(ctx, st->u.reserve(act * 4));
  TTS_HIP(ctx, st->t.reserve(act * 4));
  TTS_HIP(ctx, st->m.reserve(act * 4));
  TTS_HIP(ctx, st->a.reserve(act * 4));
  TTS_HIP(ctx, st->audio.reserve((size_t)frames * 256 * 4));
  TTS_HIP(ctx, hipMemcpyAsync(st->in.p, up.data(), up.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  const float *d_mel = st->in.as<float>();
  const int *d_seq = (const int *)(d_mel + n_mel);
  float *x = st->x.as<float>(), *u = st->u.as<float>(), *t = st->t.as<float>(), *m = st->m.as<float>(), *av = st->a.as<float>();
  {
    ProfScope ps(ctx, "bvg_mel", (double)frames * (BVG_MEL + BVG_MEL_PAD) * 4);
    bvg_mel_kernel<<<dim3(maxT, B), 128, 0, ctx->stream>>>(d_mel, d_seq, st->mel.as<float>());
  }
  // hfg_conv_kernel as hifigan_run launches it, with slope 1 (no leaky ReLU), no conditioning vector; two column groups per workgroup where they divide cout
  auto conv = [&](const float *in, float *out, const float *resid, const HfgLayer &l, int cin, int cout, int taps, int dil, int phases, int rate, int acc_mode) {
    HfgConv a{};
    a.in = in; a.out = out; a.resid = resid; a.w = l.w; a.bias = l.b; a.cbias = nullptr; a.seq = d_seq;
    a.cin = cin; a.cout = cout; a.taps = taps; a.dil = dil; a.lo = -dil * (taps - 1) / 2; a.phases = phases; a.pad_t = phases / 2; a.rate = rate;
    a.slope = 1.0f; a.acc_mode = acc_mode;
    ProfScope ps(ctx, "hfg_conv", 2.0 * (double)frames * rate * phases * taps * cin * cout);
    const int nt = cout % 64 == 0 ? 2 : 1;
    const dim3 grid((unsigned)(((size_t)maxT * rate + HFG_TM - 1) / HFG_TM), (unsigned)B, (unsigned)(cout / (32 * nt) * phases));
    const size_t lds = (size_t)(HFG_TM + (taps - 1) * dil) * 33 * 4;
    if (nt == 2) hfg_conv_kernel<2><<<grid, 256, lds, ctx->stream>>>(a);
    else hfg_conv_kernel<1><<<grid, 256, lds, ctx->stream>>>(a);
  };
  auto actv = [&](const float *in, float *out, const BvgAct &p, int C, int rate) {
    ProfScope ps(ctx, "bvg_act", 2.0 * (double)frames * rate * C * 4);
    const dim3 grid((unsigned)(((size_t)maxT * rate + BVG_ACT_RUNS * BVG_RUN - 1) / (BVG_ACT_RUNS * BVG_RUN)), (unsigned)B, (unsigned)(C / 32));
    bvg_act_kernel<<<grid, 256, 0, ctx->stream>>>(in, out, p.w, p.b, d_seq, C, rate);
  };
  conv(st->mel.as<float>(), x, nullptr, st->pre, BVG_MEL_PAD, st->ch[0], 7, 1, 1, 1, 0);
  const float *cur = x;
  int rate = 1;
  for (int i = 0; i < st->n_stages; i++) {
    conv(cur, u, nullptr, st->ups[i], st->ch[i], st->ch[i + 1], 2, 1, st->up[i], rate, 0);
    const int ch = st->ch[i + 1];
    rate *= st->up[i];
    for (int j = 0; j < 3; j++) {
      const float *r = u; // the AMP block's stream: u for the first dilation, then x
      for (int n = 0; n < 3; n++) {
        actv(r, av, st->act[i][j][2 * n], ch, rate);
        conv(av, t, nullptr, st->c1[i][j][n], ch, ch, HFG_RK[j], HFG_RD[n], 1, rate, 0);
        actv(t, av, st->act[i][j][2 * n + 1], ch, rate);
        if (n < 2) conv(av, x, r, st->c2[i][j][n], ch, ch, HFG_RK[j], 1, 1, rate, 0);
        else conv(av, m, r, st->c2[i][j][n], ch, ch, HFG_RK[j], 1, 1, rate, j); // the mean of the three AMP blocks: =, +=, (+) / 3
        r = x;
      }
    }
    cur = m;
  }
  {
    ProfScope ps(ctx, "bvg_post", (double)frames * 256 * (st->ch[st->n_stages] + 1) * 4);
    bvg_post_kernel<<<dim3(maxT, B), 256, 0, ctx->stream>>>(cur, st->post.w, st->post.b, st->act_post.w, st->act_post.b, d_seq, st->audio.as<float>(),
                                                           st->ch[st->n_stages]);
  }
  TTS_HIP(ctx, hipGetLastError());
  TTS_HIP(ctx, hipMemcpyAsync(audio_out, st->audio.p, (size_t)frames * 256 * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TTS_OK;
}

} // namespace tts
#include "classifier.h" // tortoise-detect: the same translation unit, the same convolution kernel
