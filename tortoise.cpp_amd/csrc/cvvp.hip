// CVVP candidate re-ranking on MI355X (gfx950): do these codes sound like this speaker?          tts_load_cvvp / tts_cvvp_voice / tts_cvvp_voice_audio / tts_cvvp_score
// The reference has none (main.cpp:6575 writes candidate 0) and neither had this tree until the audio front-end (audio_frontend.hip) could hand the engine the
// conditioning clip's 80-band mel. Upstream tortoise-tts ranks the autoregressive candidates by CLVP (extras.hip) and CVVP (tortoise/models/cvvp.py) and blends the two
// with cvvp_amount. Upstream's source was not at hand when this was written: the model below is RESTATED FROM MEMORY, as the audio front-end was,
// and checked against two independent float64 restatements (tests/cvvp_ref.py): parity is unpinned against upstream, pinned between independent restatements.
//
// CVVP(model_dim 512, heads 8, mel_codes 8192, depth 8 + 8, latent_multiplier 1) at inference:
//   conditioning side  mel [80][T] -> Conv1d(80, dim/2, k 5, stride 2, padding 2) -> Conv1d(dim/2, dim, k 3, stride 2, padding 1) (no activation between) -> rows [R][dim]
//   speech side        codes (< 8192) -> rows of speech_emb.emb.weight
//   both               CollapsingTransformer = CLVP's encoder layers (ff = dim, no positional embedding; encoder.h: enc_run_layers), final LayerNorm per row,
//                      pre_combiner = Conv1d(dim, dim, 1), AttentionBlock(dim, heads of 64), Conv1d(dim, dim, 1); mean over the rows; bias-free latent projection;
//                      L2 normalise
//   score[c] = mean over the clips of <conditioning latent[clip], speech latent[c]> exp(temperature)
//
// Device layout: extras.hip's (packed sequences, 128-row padding kept finite, fp16-operand GEMMs with f32 accumulation, f32 residual stream). New here: the stem's
// k = 5 im2col, the per-row final LayerNorm (CLVP fuses it with the mean; here pre_combiner sits between them) and the mean over a sequence's rows. pre_combiner.2 is a
// k = 1 convolution followed by the mean, both linear: the mean is taken on the device and pre_combiner.2 then runs beside the latent projection on the host, in double
// on the f32 weights (n_seq x 2 dim^2 multiply-adds), as CLVP's projection does. Once per voice or once per utterance: written for clarity, not for the roofline.
#include "common.h"
#include "gemm_f16.h"
#include "encoder.h"
#include <cmath>

namespace tts {

namespace {
__device__ __forceinline__ float cvvp_block_sum(float v, float *red) { // 256 threads
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// im2col of a k = 5, stride 2, padding 2 convolution over the caller's channel-major mel [cin][T] of every clip (mel_off): output row (clip, t) =
// [x[2t-2] | x[2t-1] | x[2t] | x[2t+1] | x[2t+2]] (zeros outside the clip), fp16, row length kpad >= 5 cin (zero padded). The sibling of dcond_im2col_kernel (k = 3).
__global__ __launch_bounds__(256) void cvvp_im2col5_kernel(const float *__restrict__ mel, const long long *__restrict__ mel_off, const int *__restrict__ in_len,
                                                           const int *__restrict__ out_start, const int *__restrict__ out_len, int cin, int kpad,
                                                           __half *__restrict__ a16) {
  const int s = blockIdx.y, t = blockIdx.x;
  if (t >= out_len[s]) return;
  const int Tin = in_len[s];
  __half *dst = a16 + (size_t)(out_start[s] + t) * kpad;
  for (int k = threadIdx.x; k < kpad; k += 256) {
    const int tap = k / cin, c = k - tap * cin, ti = 2 * t + tap - 2;
    float v = 0.f;
    if (tap < 5 && ti >= 0 && ti < Tin) v = mel[mel_off[s] + (size_t)c * Tin + ti];
    dst[k] = __float2half_rn(v);
  }
}

// LayerNorm (eps 1e-5, weight and bias) of one row -> fp16: the A operand of pre_combiner.0
__global__ __launch_bounds__(256) void cvvp_rownorm_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ b, int dim,
                                                           __half *__restrict__ y) {
  __shared__ float red[4];
  const float *xr = x + (size_t)blockIdx.x * dim;
  float sum = 0.f;
  for (int c = threadIdx.x; c < dim; c += 256) sum += xr[c];
  const float mean = cvvp_block_sum(sum, red) / dim;
  float sq = 0.f;
  for (int c = threadIdx.x; c < dim; c += 256) sq += (xr[c] - mean) * (xr[c] - mean);
  const float rstd = rsqrtf(cvvp_block_sum(sq, red) / dim + 1e-5f);
  for (int c = threadIdx.x; c < dim; c += 256) y[(size_t)blockIdx.x * dim + c] = __float2half_rn((xr[c] - mean) * rstd * w[c] + b[c]);
}

// pooled[seq][c] = mean over the sequence's rows of x[row][c]; one thread per column, rows ascending: the sum depends on the sequence alone
__global__ __launch_bounds__(256) void cvvp_rowmean_kernel(const float *__restrict__ x, const int *__restrict__ seq_start, const int *__restrict__ seq_len, int dim,
                                                           float *__restrict__ pooled) {
  const int s = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x, n = seq_len[s];
  if (c >= dim) return;
  const float *xc = x + (size_t)seq_start[s] * dim + c;
  float acc = 0.f;
  for (int r = 0; r < n; r++) acc += xc[(size_t)r * dim];
  pooled[(size_t)s * dim + c] = acc / n;
}
} // namespace

struct CvvpSide { // conditioning_transformer / speech_transformer
  std::vector<EncLayer> L;
  float *norm_w = nullptr, *norm_b = nullptr, *b_pc0 = nullptr;
  __half *w_pc0 = nullptr;
  AttnBlockW blk;
  std::vector<float> pc2_w, pc2_b, proj; // pre_combiner.2 and the latent projection [latent][dim]: on the host
};
struct CvvpState {
  int dim = 0, half = 0, inner = 0, ff = 0, latent = 0, n_speech = 0, k0pad = 0;
  float temperature = 0.f;
  float *emb = nullptr, *b_c0 = nullptr, *b_c1 = nullptr;
  __half *w_c0 = nullptr, *w_c1 = nullptr; // cond_emb as GEMM weights: [half][k0pad] (k = tap * 80 + c), [dim][3 half]
  CvvpSide side[2];                        // 0 conditioning, 1 speech
  std::vector<void *> owned;
  DevBuf x, h1, y16, qkv16, att16, u32, a16, pooled, meta, mel;
  // the layout cvvp_voice_begin made, for cvvp_voice_run: [n] frames | [n] first row of h1 | [n] T1 | [n] first row of x | [n] R
  std::vector<int> meta_h;
  std::vector<long long> moff_h;
  int n_clips = 0, r1 = 0, r2 = 0, max0 = 0;
  ~CvvpState() { for (void *p : owned) (void)hipFree(p); }
};
void cvvp_free(CvvpState *s) { delete s; }
int cvvp_latent_dim(const tts_ctx *ctx) { return ctx->cvvp ? ctx->cvvp->latent : TTS_ERR_STATE; }

int cvvp_load(tts_ctx *ctx, const char *path) {
  WeightFile wf;
  std::string err;
  int rc = read_weight_file(path, wf, err);
  if (rc != TTS_OK) return fail(ctx, rc, "cvvp_load: %s", err.c_str());
  if (!wf.has("cond_emb.0.weight") || !wf.has("speech_emb.emb.weight") || !wf.has("to_conditioning_latent.weight"))
    return fail(ctx, TTS_ERR_FORMAT, "'%s' is not a CVVP model file", path);
  std::unique_ptr<CvvpState> st(new CvvpState());
  auto get = [&](const std::string &name, int64_t nelem) -> const HostTensor * {
    auto it = wf.t.find(name);
    if (it == wf.t.end()) { fail(ctx, TTS_ERR_FORMAT, "tensor '%s' missing from CVVP model file", name.c_str()); return nullptr; }
    if (it->second.nelem() != nelem) { fail(ctx, TTS_ERR_FORMAT, "tensor '%s' has %lld elements in CVVP model file, %lld expected", name.c_str(), (long long)it->second.nelem(), (long long)nelem); return nullptr; }
    return &it->second;
  };
  const char *encs[2] = {"conditioning_transformer", "speech_transformer"}, *projs[2] = {"to_conditioning_latent.weight", "to_speech_latent.weight"};
  const std::string lp = ".transformer.attn_layers.layers.";
  const int d = st->dim = (int)wf.t.at("speech_emb.emb.weight").ne[0];
  st->n_speech = (int)wf.t.at("speech_emb.emb.weight").ne[1];
  st->half = d / 2;
  if (!wf.has(std::string(encs[1]) + lp + "0.1.to_q.weight") || !wf.has(std::string(encs[1]) + lp + "1.1.net.3.weight"))
    return fail(ctx, TTS_ERR_FORMAT, "no encoder layers in CVVP model file '%s'", path);
  const int in = st->inner = (int)wf.t.at(std::string(encs[1]) + lp + "0.1.to_q.weight").ne[1];
  const int ff = st->ff = (int)wf.t.at(std::string(encs[1]) + lp + "1.1.net.3.weight").ne[0];
  st->latent = (int)wf.t.at("to_conditioning_latent.weight").ne[1];
  // the GroupNorm widths that are instantiated (venc_groupnorm_kernel<512 | 1024>), heads of 64
  if ((d != 512 && d != 1024) || in != d || ff < 128 || ff % 128 || st->latent < 1 || st->n_speech < 1)
    return fail(ctx, TTS_ERR_FORMAT, "CVVP dims %d / %d / %d: model dim 512 or 1024 with dim / 64 heads and a feed-forward width that is a multiple of 128 expected", d, in, ff);
  st->k0pad = (5 * 80 + 63) / 64 * 64;
  const HostTensor *t, *tb;
  if (!(t = get("temperature", 1))) return TTS_ERR_FORMAT;
  st->temperature = t->data[0];
  size_t known = 1;
  { // the stem: Conv1d weights [cout][cin][k] -> GEMM weights [cout][kpad], k = tap * cin + c (the im2col order)
    const int hf = st->half, k0 = st->k0pad;
    if (!(t = get("cond_emb.0.weight", (int64_t)hf * 80 * 5)) || !(tb = get("cond_emb.0.bias", hf))) return TTS_ERR_FORMAT;
    std::vector<float> w0((size_t)hf * k0, 0.f);
    for (int n = 0; n < hf; n++)
      for (int c = 0; c < 80; c++)
        for (int tap = 0; tap < 5; tap++) w0[(size_t)n * k0 + tap * 80 + c] = t->data[((size_t)n * 80 + c) * 5 + tap];
    if ((rc = enc_up16(ctx, st->owned, {&w0}, &st->w_c0)) || (rc = enc_up(ctx, st->owned, tb->data, &st->b_c0))) return rc;
    if (!(t = get("cond_emb.1.weight", (int64_t)d * hf * 3)) || !(tb = get("cond_emb.1.bias", d))) return TTS_ERR_FORMAT;
    std::vector<float> w1((size_t)d * 3 * hf);
    for (int n = 0; n < d; n++)
      for (int c = 0; c < hf; c++)
        for (int tap = 0; tap < 3; tap++) w1[(size_t)n * 3 * hf + tap * hf + c] = t->data[((size_t)n * hf + c) * 3 + tap];
    if ((rc = enc_up16(ctx, st->owned, {&w1}, &st->w_c1)) || (rc = enc_up(ctx, st->owned, tb->data, &st->b_c1))) return rc;
    known += 4;
  }
  if (!(t = get("speech_emb.emb.weight", (int64_t)d * st->n_speech)) || (rc = enc_up(ctx, st->owned, t->data, &st->emb))) return rc ? rc : TTS_ERR_FORMAT;
  known += 1;
  for (int e = 0; e < 2; e++) {
    CvvpSide &sd = st->side[e];
    const std::string E = encs[e];
    int depth = 0;
    while (wf.has(E + lp + std::to_string(2 * depth) + ".0.g")) depth++;
    if (depth < 1) return fail(ctx, TTS_ERR_FORMAT, "no %s layers in CVVP model file '%s'", encs[e], path);
    if ((rc = enc_load_layers(ctx, wf, E, "CVVP", depth, d, in, ff, st->owned, sd.L))) return rc;
    known += 11 * (size_t)depth;
    if (!(t = get(E + ".transformer.norm.weight", d)) || (rc = enc_up(ctx, st->owned, t->data, &sd.norm_w))) return rc ? rc : TTS_ERR_FORMAT;
    if (!(t = get(E + ".transformer.norm.bias", d)) || (rc = enc_up(ctx, st->owned, t->data, &sd.norm_b))) return rc ? rc : TTS_ERR_FORMAT;
    const std::string pc = E + ".pre_combiner.";
    if (!(t = get(pc + "0.weight", (int64_t)d * d)) || (rc = enc_up16(ctx, st->owned, {&t->data}, &sd.w_pc0))) return rc ? rc : TTS_ERR_FORMAT;
    if (!(t = get(pc + "0.bias", d)) || (rc = enc_up(ctx, st->owned, t->data, &sd.b_pc0))) return rc ? rc : TTS_ERR_FORMAT;
    const HostTensor *g, *gb, *qw, *qb, *pw, *pb;
    if (!(g = get(pc + "1.norm.weight", d)) || !(gb = get(pc + "1.norm.bias", d)) || !(qw = get(pc + "1.qkv.weight", (int64_t)3 * d * d)) || !(qb = get(pc + "1.qkv.bias", 3 * d)) ||
        !(pw = get(pc + "1.proj_out.weight", (int64_t)d * d)) || !(pb = get(pc + "1.proj_out.bias", d)))
      return TTS_ERR_FORMAT;
    // QKVAttentionLegacy: output channel = head * 192 + {q, k, v} * 64 + j -> q | k | v blocks with head h at columns h * 64 (the voice encoder's permutation)
    std::vector<float> w((size_t)3 * d * d), bq(3 * d);
    for (int h = 0; h < d / 64; h++)
      for (int tq = 0; tq < 3; tq++)
        for (int j = 0; j < 64; j++) {
          const int o = h * 192 + tq * 64 + j, n = tq * d + h * 64 + j;
          bq[n] = qb->data[o];
          memcpy(&w[(size_t)n * d], &qw->data[(size_t)o * d], (size_t)d * 4);
        }
    if ((rc = enc_up(ctx, st->owned, g->data, &sd.blk.g)) || (rc = enc_up(ctx, st->owned, gb->data, &sd.blk.b)) || (rc = enc_up16(ctx, st->owned, {&w}, &sd.blk.w_qkv)) ||
        (rc = enc_up(ctx, st->owned, bq, &sd.blk.b_qkv)) || (rc = enc_up16(ctx, st->owned, {&pw->data}, &sd.blk.w_proj)) || (rc = enc_up(ctx, st->owned, pb->data, &sd.blk.b_proj)))
      return rc;
    if (!(t = get(pc + "2.weight", (int64_t)d * d)) || !(tb = get(pc + "2.bias", d))) return TTS_ERR_FORMAT;
    sd.pc2_w = t->data; sd.pc2_b = tb->data;
    if (!(t = get(projs[e], (int64_t)d * st->latent))) return TTS_ERR_FORMAT;
    sd.proj = t->data;
    known += 13;
  }
  // every tensor in the file must be known, as in the CLVP loader; the rotary inv_freq buffers of the upstream state dict are recomputed and may be present
  size_t extra = 0;
  for (auto &kv : wf.t)
    if (kv.first.find("rotary_pos_emb.inv_freq") != std::string::npos) extra++;
  if (wf.t.size() != known + extra) return fail(ctx, TTS_ERR_FORMAT, "unknown tensors in CVVP model file '%s' (%d tensors, %d expected)", path, (int)wf.t.size(), (int)(known + extra));
  if (ctx->cvvp) cvvp_free(ctx->cvvp);
  ctx->cvvp = st.release();
  return TTS_OK;
}

// scratch of one encoder pass over M padded rows; rows past the last one are multiplied like the others (128-row GEMM tiles) and never read back: kept finite
static int cvvp_scratch(tts_ctx *ctx, CvvpState *st, int M, int nseq, bool zero_x) {
  const int d = st->dim, ff = st->ff;
  TTS_HIP(ctx, st->x.reserve((size_t)M * d * 4));
  TTS_HIP(ctx, st->y16.reserve((size_t)M * std::max(d, ff) * 2));
  TTS_HIP(ctx, st->qkv16.reserve((size_t)M * 3 * d * 2));
  TTS_HIP(ctx, st->att16.reserve((size_t)M * d * 2));
  TTS_HIP(ctx, st->u32.reserve((size_t)M * 2 * ff * 4));
  TTS_HIP(ctx, st->pooled.reserve((size_t)nseq * d * 4));
  if (zero_x) TTS_HIP(ctx, hipMemsetAsync(st->x.p, 0, (size_t)M * d * 4, ctx->stream));
  TTS_HIP(ctx, hipMemsetAsync(st->y16.p, 0, (size_t)M * std::max(d, ff) * 2, ctx->stream));
  TTS_HIP(ctx, hipMemsetAsync(st->att16.p, 0, (size_t)M * d * 2, ctx->stream));
  TTS_HIP(ctx, hipMemsetAsync(st->u32.p, 0, (size_t)M * 2 * ff * 4, ctx->stream));
  return TTS_OK;
}

// The CollapsingTransformer of side e over the sequences st->x holds, then the latent projection and the normalisation: lat_out [nseq][latent]
static int cvvp_collapse(tts_ctx *ctx, CvvpState *st, int e, int nseq, int rows, int maxlen, const int *d_start, const int *d_len, std::vector<float> &lat_out) {
  const int d = st->dim, M = (rows + 127) / 128 * 128;
  const CvvpSide &sd = st->side[e];
  EncWork w;
  w.d_start = d_start; w.d_len = d_len; w.nseq = nseq; w.rows = rows; w.maxlen = maxlen; w.M = M;
  w.x = st->x.as<float>(); w.u = st->u32.as<float>(); w.y = st->y16.as<__half>(); w.qkv = st->qkv16.as<__half>(); w.att = st->att16.as<__half>();
  int rc = enc_run_layers(ctx, sd.L, d, st->inner, st->ff, w);
  if (rc) return rc;
  {
    ProfScope ps(ctx, "cvvp_collapse", 2.0 * rows * 5.0 * d * d);
    cvvp_rownorm_kernel<<<rows, 256, 0, ctx->stream>>>(w.x, sd.norm_w, sd.norm_b, d, w.y);
    GemmArgs g{}; // pre_combiner.0: the normed rows -> x (the residual stream the AttentionBlock works on)
    for (int i = 0; i < 3; i++) { g.A[i] = w.y; g.row_off[i] = 0; }
    g.nseg = 1; g.kseg = d; g.lda = d; g.W = sd.w_pc0; g.M = M; g.N = d; g.bias = sd.b_pc0; g.mode = GEMM_OUT_F32; g.outF = w.x; g.ldo = d;
    TTS_HIP(ctx, launch_gemm_f16(g, ctx->stream));
    if ((rc = attn_block_run(ctx, d, sd.blk, w))) return rc;
    cvvp_rowmean_kernel<<<dim3(nseq, (d + 255) / 256), 256, 0, ctx->stream>>>(w.x, d_start, d_len, d, st->pooled.as<float>());
  }
  TTS_HIP(ctx, hipGetLastError());
  std::vector<float> pooled((size_t)nseq * d);
  TTS_HIP(ctx, hipMemcpyAsync(pooled.data(), st->pooled.p, pooled.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // pre_combiner.2 (a k = 1 convolution commutes with the mean), the bias-free latent projection and the L2 normalisation on the host, in double
  lat_out.assign((size_t)nseq * st->latent, 0.f);
  std::vector<double> m(d), z(st->latent);
  for (int s = 0; s < nseq; s++) {
    const float *p = &pooled[(size_t)s * d];
    for (int o = 0; o < d; o++) {
      double a = sd.pc2_b[o];
      const float *wr = &sd.pc2_w[(size_t)o * d];
      for (int c = 0; c < d; c++) a += (double)wr[c] * p[c];
      m[o] = a;
    }
    double nn = 0;
    for (int o = 0; o < st->latent; o++) {
      double a = 0;
      const float *wr = &sd.proj[(size_t)o * d];
      for (int c = 0; c < d; c++) a += (double)wr[c] * m[c];
      z[o] = a; nn += a * a;
    }
    const double inv = 1.0 / std::max(std::sqrt(nn), 1e-12);
    for (int o = 0; o < st->latent; o++) lat_out[(size_t)s * st->latent + o] = (float)(z[o] * inv);
  }
  return TTS_OK;
}

// tts_cvvp_voice in two halves, as voice_enc_begin / voice_enc_run: the layout and the buffers, then (once the mel buffer is filled: an upload in cvvp_voice, the audio
// front-end's kernels in tts_cvvp_voice_audio) the stem and the encoder.
int cvvp_voice_begin(tts_ctx *ctx, const int32_t *frames, int n_clips, float **d_mel) {
  CvvpState *st = ctx->cvvp;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_cvvp not called");
  if (!frames || n_clips < 1 || !d_mel) return fail(ctx, TTS_ERR_ARG, "tts_cvvp_voice: bad arguments");
  for (int s = 0; s < n_clips; s++) {
    if (frames[s] < 1) return fail(ctx, TTS_ERR_ARG, "clip %d: %d mel frames (at least 1 expected)", s, frames[s]);
    if (frames[s] > TTS_CVVP_MAX_FRAMES) return fail(ctx, TTS_ERR_LIMIT, "clip %d: %d mel frames, at most %d", s, frames[s], TTS_CVVP_MAX_FRAMES);
  }
  if (n_clips > 4096) return fail(ctx, TTS_ERR_LIMIT, "%d clips, at most 4096", n_clips);
  std::vector<int> meta(5 * n_clips);
  std::vector<long long> moff(n_clips);
  int r1 = 0, r2 = 0, max0 = 0;
  long long off = 0;
  for (int s = 0; s < n_clips; s++) {
    const int T1 = (frames[s] - 1) / 2 + 1, T2 = (T1 - 1) / 2 + 1;
    meta[s] = frames[s];
    meta[n_clips + s] = r1; meta[2 * n_clips + s] = T1;
    meta[3 * n_clips + s] = r2; meta[4 * n_clips + s] = T2;
    moff[s] = off;
    off += (long long)80 * frames[s]; r1 += T1; r2 += T2; max0 = std::max(max0, frames[s]);
  }
  const int M1 = (r1 + 127) / 128 * 128, M2 = (r2 + 127) / 128 * 128;
  TTS_HIP(ctx, st->h1.reserve((size_t)M1 * st->half * 4));
  TTS_HIP(ctx, st->a16.reserve(std::max((size_t)M1 * st->k0pad, (size_t)M2 * 3 * st->half) * 2));
  TTS_HIP(ctx, st->meta.reserve((size_t)5 * n_clips * 4 + (size_t)n_clips * 8 + 16));
  TTS_HIP(ctx, st->mel.reserve((size_t)off * 4));
  TTS_HIP(ctx, st->x.reserve((size_t)M2 * st->dim * 4));
  st->meta_h.swap(meta); st->moff_h.swap(moff); // both outlive this call: the copies below are asynchronous
  int *dm = st->meta.as<int>();
  long long *d_moff = (long long *)(st->meta.as<char>() + (((size_t)5 * n_clips * 4 + 7) & ~(size_t)7));
  TTS_HIP(ctx, hipMemcpyAsync(dm, st->meta_h.data(), st->meta_h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  TTS_HIP(ctx, hipMemcpyAsync(d_moff, st->moff_h.data(), st->moff_h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  st->n_clips = n_clips; st->r1 = r1; st->r2 = r2; st->max0 = max0;
  *d_mel = st->mel.as<float>();
  return TTS_OK;
}

int cvvp_voice_run(tts_ctx *ctx, float *latents_out) {
  CvvpState *st = ctx->cvvp;
  const int n_clips = st->n_clips, r1 = st->r1, r2 = st->r2, d = st->dim, hf = st->half, k0 = st->k0pad;
  const int max1 = (st->max0 - 1) / 2 + 1, max2 = (max1 - 1) / 2 + 1;
  const int M1 = (r1 + 127) / 128 * 128, M2 = (r2 + 127) / 128 * 128;
  int rc = cvvp_scratch(ctx, st, M2, n_clips, false);
  if (rc) return rc;
  const int *dm = st->meta.as<int>();
  const long long *d_moff = (const long long *)(st->meta.as<char>() + (((size_t)5 * n_clips * 4 + 7) & ~(size_t)7));
  float *h1 = st->h1.as<float>(), *x = st->x.as<float>();
  __half *a16 = st->a16.as<__half>();
  auto gemm = [&](const __half *A, int K, const __half *W, int M, int N, const float *bias, float *out) {
    GemmArgs g{};
    for (int i = 0; i < 3; i++) { g.A[i] = A; g.row_off[i] = 0; }
    g.nseg = 1; g.kseg = K; g.lda = K; g.W = W; g.M = M; g.N = N; g.bias = bias; g.mode = GEMM_OUT_F32; g.outF = out; g.ldo = N;
    return g;
  };
  {
    ProfScope ps(ctx, "cvvp_stem", 2.0 * ((double)r1 * 400 * hf + (double)r2 * 3 * hf * d));
    TTS_HIP(ctx, hipMemsetAsync(a16, 0, (size_t)M1 * k0 * 2, ctx->stream));
    cvvp_im2col5_kernel<<<dim3(max1, n_clips), 256, 0, ctx->stream>>>(st->mel.as<float>(), d_moff, dm, dm + n_clips, dm + 2 * n_clips, 80, k0, a16);
    TTS_HIP(ctx, launch_gemm_f16(gemm(a16, k0, st->w_c0, M1, hf, st->b_c0, h1), ctx->stream));
    TTS_HIP(ctx, hipMemsetAsync(a16, 0, (size_t)M2 * 3 * hf * 2, ctx->stream));
    im2col3_rows(ctx, h1, dm + n_clips, dm + 2 * n_clips, dm + 3 * n_clips, dm + 4 * n_clips, max2, n_clips, hf, 3 * hf, a16);
    TTS_HIP(ctx, launch_gemm_f16(gemm(a16, 3 * hf, st->w_c1, M2, d, st->b_c1, x), ctx->stream));
  }
  std::vector<float> lat;
  if ((rc = cvvp_collapse(ctx, st, 0, n_clips, r2, max2, dm + 3 * n_clips, dm + 4 * n_clips, lat))) return rc;
  memcpy(latents_out, lat.data(), lat.size() * 4);
  return TTS_OK;
}

int cvvp_voice(tts_ctx *ctx, const float *mel, const int32_t *frames, int n_clips, float *latents_out) {
  if (!ctx->cvvp) return fail(ctx, TTS_ERR_STATE, "tts_load_cvvp not called");
  if (!mel || !frames || n_clips < 1 || !latents_out) return fail(ctx, TTS_ERR_ARG, "tts_cvvp_voice: bad arguments");
  long long total = 0;
  for (int s = 0; s < n_clips; s++) {
    if (frames[s] < 1) return fail(ctx, TTS_ERR_ARG, "clip %d: %d mel frames (at least 1 expected)", s, frames[s]);
    if (frames[s] > TTS_CVVP_MAX_FRAMES) return fail(ctx, TTS_ERR_LIMIT, "clip %d: %d mel frames, at most %d", s, frames[s], TTS_CVVP_MAX_FRAMES);
    total += 80LL * frames[s];
  }
  for (long long i = 0; i < total; i++)
    if (!std::isfinite(mel[i])) return fail(ctx, TTS_ERR_ARG, "tts_cvvp_voice: the mel holds a non-finite value (float %lld)", i);
  float *d_mel = nullptr;
  const int rc = cvvp_voice_begin(ctx, frames, n_clips, &d_mel);
  if (rc) return rc;
  TTS_HIP(ctx, hipMemcpyAsync(d_mel, mel, (size_t)total * 4, hipMemcpyHostToDevice, ctx->stream));
  return cvvp_voice_run(ctx, latents_out);
}

int cvvp_score(tts_ctx *ctx, const float *voice_latents, int n_clips, const int32_t *codes, const int32_t *code_len, int n_candidates, int code_stride,
               float *scores_out) {
  CvvpState *st = ctx->cvvp;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_cvvp not called");
  if (!voice_latents || n_clips < 1 || !codes || !code_len || n_candidates < 1 || !scores_out) return fail(ctx, TTS_ERR_ARG, "tts_cvvp_score: bad arguments");
  for (long long i = 0; i < (long long)n_clips * st->latent; i++)
    if (!std::isfinite(voice_latents[i])) return fail(ctx, TTS_ERR_ARG, "tts_cvvp_score: the voice latents hold a non-finite value (float %lld)", i);
  std::vector<int> tok, meta(2 * n_candidates);
  int rows = 0, maxlen = 0;
  for (int c = 0; c < n_candidates; c++) {
    if (code_len[c] < 1 || code_len[c] > code_stride) return fail(ctx, TTS_ERR_ARG, "candidate %d: %d codes (1 .. %d expected)", c, code_len[c], code_stride);
    for (int j = 0; j < code_len[c]; j++) {
      const int v = codes[(size_t)c * code_stride + j];
      if (v < 0 || v >= st->n_speech) return fail(ctx, TTS_ERR_ARG, "candidate %d: mel code %d out of range (start / stop tokens are not scored)", c, v);
      tok.push_back(v);
    }
    meta[c] = rows; meta[n_candidates + c] = code_len[c];
    rows += code_len[c]; maxlen = std::max(maxlen, code_len[c]);
  }
  const int M = (rows + 127) / 128 * 128;
  int rc = cvvp_scratch(ctx, st, M, n_candidates, true);
  if (rc) return rc;
  TTS_HIP(ctx, st->meta.reserve((size_t)(2 * n_candidates + rows) * 4));
  int *d_start = st->meta.as<int>(), *d_len = d_start + n_candidates, *d_tok = d_len + n_candidates;
  TTS_HIP(ctx, hipMemcpyAsync(d_start, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  TTS_HIP(ctx, hipMemcpyAsync(d_tok, tok.data(), (size_t)rows * 4, hipMemcpyHostToDevice, ctx->stream));
  enc_embed(ctx, st->emb, d_tok, st->dim, rows, st->x.as<float>());
  std::vector<float> zs;
  if ((rc = cvvp_collapse(ctx, st, 1, n_candidates, rows, maxlen, d_start, d_len, zs))) return rc; // synchronises: meta and tok may go
  const double temp = std::exp((double)st->temperature);
  for (int c = 0; c < n_candidates; c++) {
    double a = 0; // upstream accumulates one CVVP evaluation per conditioning clip and divides by the clip count
    for (int k = 0; k < n_clips; k++) {
      double dot = 0;
      for (int o = 0; o < st->latent; o++) dot += (double)voice_latents[(size_t)k * st->latent + o] * zs[(size_t)c * st->latent + o];
      a += dot * temp;
    }
    scores_out[c] = (float)(a / n_clips);
  }
  return TTS_OK;
}

} // namespace tts
