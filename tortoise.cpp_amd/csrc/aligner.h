// wav2vec2 CTC aligner on MI355X (gfx950): a waveform -> one token id per 20 ms frame             tts_load_aligner / tts_aligner_ids / tts_align_audio / tts_redact_audio
//
// Included once, as the last line of classifier.h (hifigan.hip's translation unit; its loader and clip ingest are model_io.h's): Wav2Vec2ForCTC in the "stable layer norm" configuration upstream tortoise-tts
// loads for Wav2VecAlignment. Upstream's source and weights are not available offline: the contract is the arithmetic below ("What pins the
// aligner"), checked between two float64 spellings (tests/aligner_ref.py); unpinned against upstream. f32 throughout: alignment rests on a per-frame argmax.
//
//   x = (clip at 16 kHz - mean) / sqrt(var + 1e-7), var unbiased, over the whole clip      w2v_stat_partial_kernel + w2v_stat_finish_kernel, applied in the stem's load
//   h = GELU(LN_C(Conv1d(1 -> C, k_0, stride s_0)(x)))                                     w2v_stem_kernel, w2v_ln_kernel
//   layer i = 1 .. N - 1:  h = GELU(LN_C(Conv1d(C -> C, k_i, stride s_i)(h)))              cls_down_kernel (pad 0), w2v_ln_kernel
//   h = Linear(C -> D)(LN_C(h))                                                            w2v_ln_kernel, hfg_conv_kernel (k 1)
//   h = h + GELU(Conv1d(D -> D, K, padding K / 2, groups G)(h))[: frames]                  w2v_pos_kernel
//   depth x:  h = h + out(attn(qkv(LN(h))));  h = h + W2 GELU(W1 LN(h))                    w2v_ln_kernel, hfg_conv_kernel, cls_attn_kernel<64>, w2v_gelu_kernel
//   ids = argmax(Linear(D -> V)(LN(h))), the lowest index on a tie                         w2v_ln_kernel, w2v_head_kernel
//
// Device layout: time-major f32 rows [row][channels]; clip s owns the rows [start_s, start_s + n_s) of a level, start_s a multiple of 8. Level 0 of the table is
// the clip's samples, level i the output of convolution i - 1; everything behind the extractor shares level N. No kernel reads or writes a row outside the clip
// it works on; none uses atomics: two runs agree bit for bit and a clip alone gives the bits of the clip in a batch.
//
// What the reused kernels can tile (aligner_parse refuses everything else, TTS_ERR_FORMAT): C and D multiples of 64 up to 1024 (cls_down_kernel's 64-column
// tiles, w2v_ln_kernel's 16 values per lane), the feed-forward width a multiple of 64, D / heads = 64 (cls_attn_kernel<64>), D / G a multiple of 64 with the
// positional window (64 + K - 1 rows of D / G + 1 floats) inside 64 KB of LDS, k_0 <= 64 with s_0 <= 8, k_i <= 16 with s_i <= 4 (cls_down_kernel's window inside 64 KB), V <= 1024.
#pragma once

namespace tts {

namespace {
constexpr int W2V_ST_TILE = 4096;  // samples of a statistics tile
constexpr int W2V_STEM_ROWS = 64;  // rows of a w2v_stem_kernel workgroup
constexpr int W2V_ROW_TILE = 64;   // rows of a w2v_gelu_kernel workgroup
constexpr int W2V_PTM = 64;        // output rows of a w2v_pos_kernel workgroup: 2 row halves x 2 column groups of 32 over its 4 waves
constexpr int W2V_HEAD_ROWS = 8;   // rows of a w2v_head_kernel workgroup: 2 per wave
constexpr int W2V_MAX_C = 1024, W2V_MAX_V = 1024, W2V_MAX_CONV = 16, W2V_MAX_CLIPS = 256;

__device__ __forceinline__ float w2v_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// Partial sums of one tile of one clip's samples in double: thread j adds samples j, j + 256, .. of the tile ascending, thread 0 the 256 sums ascending.
// seq record (level 0): {-, samples, 0, first tile of the clip, first sample of the clip in x}
__global__ __launch_bounds__(256) void w2v_stat_partial_kernel(const float *__restrict__ x, const int *__restrict__ seq, double2 *__restrict__ part) {
  __shared__ double ss[256], sq[256];
  const int s = blockIdx.y;
  const int n = seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * W2V_ST_TILE;
  if (t0 >= n) return;
  const float *xs = x + (size_t)seq[HFG_SEQ * s + 4];
  const int t1 = min(t0 + W2V_ST_TILE, n);
  double a = 0, a2 = 0;
  for (int i = t0 + threadIdx.x; i < t1; i += 256) { const double d = xs[i]; a += d; a2 += d * d; }
  ss[threadIdx.x] = a; sq[threadIdx.x] = a2;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sm = 0, s2 = 0;
    for (int j = 0; j < 256; j++) { sm += ss[j]; s2 += sq[j]; }
    part[(size_t)seq[HFG_SEQ * s + 3] + blockIdx.x] = make_double2(sm, s2);
  }
}

// stat[s] = {mean, 1 / sqrt(var + eps)}, var the UNBIASED variance (n - 1) as torch.var: thread j adds tiles j, j + 64, .. ascending, thread 0 the 64 sums ascending
__global__ __launch_bounds__(64) void w2v_stat_finish_kernel(const double2 *__restrict__ part, const int *__restrict__ seq, double eps, double2 *__restrict__ stat) {
  __shared__ double rs[64], rq[64];
  const int s = blockIdx.x;
  const int n = seq[HFG_SEQ * s + 1], tiles = (n + W2V_ST_TILE - 1) / W2V_ST_TILE;
  const double2 *p = part + (size_t)seq[HFG_SEQ * s + 3];
  double sm = 0, s2 = 0;
  for (int t = threadIdx.x; t < tiles; t += 64) { const double2 v = p[t]; sm += v.x; s2 += v.y; }
  rs[threadIdx.x] = sm; rq[threadIdx.x] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    sm = 0; s2 = 0;
    for (int j = 0; j < 64; j++) { sm += rs[j]; s2 += rq[j]; }
    const double mean = sm / (double)n;
    const double var = n > 1 ? fmax((s2 - sm * mean) / (double)(n - 1), 0.0) : 0.0;
    stat[s] = make_double2(mean, 1.0 / sqrt(var + eps));
  }
}

// h[t][c] = b[c] + sum_k w[c][k] xn[t stride + k], k ascending, one fmaf per tap; xn = (float)(x - mean) * (float)rstd: the double mean is subtracted from the
// widened sample before it rounds. The workgroup's window of normalised samples goes through LDS once.
__global__ __launch_bounds__(256) void w2v_stem_kernel(const float *__restrict__ x, const double2 *__restrict__ stat, const float *__restrict__ w,
                                                       const float *__restrict__ b, const int *__restrict__ seq_in, const int *__restrict__ seq_out, int C, int taps,
                                                       int stride, float *__restrict__ out) {
  extern __shared__ float sx[];
  const int s = blockIdx.y;
  const int n = seq_in[HFG_SEQ * s + 1], fo = seq_out[HFG_SEQ * s], T = seq_out[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * W2V_STEM_ROWS;
  if (t0 >= T) return;
  const float *xs = x + (size_t)seq_in[HFG_SEQ * s + 4];
  const int rows = min(W2V_STEM_ROWS, T - t0), win = (rows - 1) * stride + taps;
  const double mean = stat[s].x;
  const float rstd = (float)stat[s].y;
  for (int i = threadIdx.x; i < win; i += 256) {
    const int j = t0 * stride + i;
    sx[i] = j < n ? __fmul_rn((float)((double)xs[j] - mean), rstd) : 0.f;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < rows * C; idx += 256) {
    const int t = idx / C, c = idx % C;
    float acc = b[c];
    for (int k = 0; k < taps; k++) acc = __fmaf_rn(w[c * taps + k], sx[t * stride + k], acc);
    out[((size_t)fo + t0 + t) * C + c] = acc;
  }
}

// LayerNorm over the C channels of a row (biased variance, eps 1e-5), optionally followed by the exact erf GELU. One wave per row, the row in registers (lane j
// holds channels j, j + 64, ..): pass 1 the mean, pass 2 the variance of the centred values; each sum lane-local ascending, then the xor tree. x may be y.
__global__ __launch_bounds__(256) void w2v_ln_kernel(const float *x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                     const int *__restrict__ seq, int C, int gelu, float *y) {
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= n) return;
  const int npl = C >> 6;
  const float *xr = x + ((size_t)f0 + t) * C;
  float v[16];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    v[i] = i < npl ? xr[i * 64 + lane] : 0.f;
    sum += v[i];
  }
  for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
  const float mean = sum / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    v[i] = i < npl ? v[i] - mean : 0.f;
    sq = __fmaf_rn(v[i], v[i], sq);
  }
  for (int d = 32; d; d >>= 1) sq += __shfl_xor(sq, d);
  const float rstd = 1.0f / sqrtf(sq / (float)C + 1e-5f);
  float *yr = y + ((size_t)f0 + t) * C;
#pragma unroll
  for (int i = 0; i < 16; i++)
    if (i < npl) {
      const int c = i * 64 + lane;
      const float o = __fmaf_rn(__fmul_rn(v[i], rstd), gamma[c], beta[c]);
      yr[c] = gelu ? w2v_gelu(o) : o;
    }
}

// x = GELU(x) on the rows of every clip (the feed-forward's activation), C a multiple of 4
__global__ __launch_bounds__(256) void w2v_gelu_kernel(float *__restrict__ x, const int *__restrict__ seq, int C) {
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * W2V_ROW_TILE;
  if (t0 >= n) return;
  const int rows = min(W2V_ROW_TILE, n - t0), qpr = C / 4;
  float4 *p = (float4 *)(x + ((size_t)f0 + t0) * C);
  for (int idx = threadIdx.x; idx < rows * qpr; idx += 256) {
    const float4 v = p[idx];
    p[idx] = make_float4(w2v_gelu(v.x), w2v_gelu(v.y), w2v_gelu(v.z), w2v_gelu(v.w));
  }
}

struct W2vPos {
  const float *in;   // [rows][D]: the convolution's input and the residual
  float *out;        // [rows][D]; never the same buffer as `in` (a workgroup reads its neighbours' rows)
  const float *w;    // [group][tap][cin of the group][cout of the group]
  const float *bias; // [D]
  const int *seq;
  int D, cg, K;      // cg = D / groups; input row of tap j for output row t: t - K / 2 + j
};
inline size_t w2v_pos_lds(int cg, int K) { return (size_t)(W2V_PTM + K - 1) * (cg + 1) * 4; }

// The grouped positional convolution: an implicit GEMM per group (M = frames, N = D / G, reduction = taps x D / G) on the f32-input MFMA with
// cls_down_kernel's staging scheme at stride 1. One workgroup: 64 output rows x 64 output channels of ONE group (blockIdx.z = group x column block); wave w
// owns the 32 x 32 tile (row half w & 1, column group w >> 1). The window (64 + K - 1 rows) holds ALL cg input channels of the group, cg + 1 floats per row (the
// 32 rows of an A fragment at one channel fall on 32 banks), so the summation order is taps outer, channels inner. Rows outside the clip read as zero (the
// convolution's padding, by predication); for an even K PyTorch's extra last output row is never computed. Epilogue: out = in + GELU(acc + bias).
__global__ __launch_bounds__(256) void w2v_pos_kernel(const W2vPos a) {
  extern __shared__ float sx[];
  const int s = blockIdx.y;
  const int f0 = a.seq[HFG_SEQ * s], T = a.seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * W2V_PTM;
  if (t0 >= T) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int nb = a.cg / 64, g = blockIdx.z / nb;
  const int m0 = (wave & 1) * 32, n0 = (blockIdx.z % nb) * 64 + (wave >> 1) * 32; // n0: the column inside the group
  const int ld = a.cg + 1, win = W2V_PTM + a.K - 1, qpr = a.cg / 4;
  const int base = t0 - a.K / 2; // the clip's row under window row 0
  const float *in = a.in + (size_t)f0 * a.D + (size_t)g * a.cg;
  for (int idx = threadIdx.x; idx < win * qpr; idx += 256) {
    const int r = idx / qpr, q = (idx % qpr) * 4, t = base + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= 0 && t < T) v = *(const float4 *)(in + (size_t)t * a.D + q);
    float *d = sx + r * ld + q;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  for (int tap = 0; tap < a.K; tap++) {
    const float *xr = sx + (m0 + lr + tap) * ld + lk;
    const float *wr = a.w + ((size_t)(g * a.K + tap) * a.cg + lk) * a.cg + n0 + lr;
    for (int c0 = 0; c0 < a.cg; c0 += 64) // cg is a multiple of 64
#pragma unroll 8
      for (int k = c0; k < c0 + 64; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[k], wr[(size_t)k * a.cg], acc, 0, 0, 0);
  }
  const int col = g * a.cg + n0 + lr;
  const float bv = a.bias[col];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int t = t0 + m0 + 8 * (r >> 2) + 4 * lk + (r & 3);
    if (t < T) {
      const size_t o = ((size_t)f0 + t) * a.D + col;
      a.out[o] = a.in[o] + w2v_gelu(acc[r] + bv);
    }
  }
}

// The CTC head: logits = W x + b for any V <= 1024 and the argmax of every row, the lowest index on a tie. One workgroup: 8 rows staged in LDS, 2 per wave;
// lane j owns the columns j, j + 64, .. (the weights [D][V]: a wave reads consecutive columns), each logit one fmaf per channel, channels ascending, plus the
// bias; a lane keeps the best of its columns ascending, the xor tree then prefers the larger value and, on equal values, the lower index.
// ids [row], logits null or [row][V], both indexed by the level's row.
__global__ __launch_bounds__(256) void w2v_head_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ b,
                                                       const int *__restrict__ seq, int D, int V, int *__restrict__ ids, float *__restrict__ logits) {
  extern __shared__ float sx[];
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * W2V_HEAD_ROWS;
  if (t0 >= n) return;
  const int rows = min(W2V_HEAD_ROWS, n - t0);
  for (int idx = threadIdx.x; idx < W2V_HEAD_ROWS * D; idx += 256) sx[idx] = idx / D < rows ? x[((size_t)f0 + t0) * D + idx] : 0.f;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float *x0 = sx + (wave * 2) * D, *x1 = x0 + D;
  const int r0 = wave * 2, r1 = r0 + 1;
  float best0 = -INFINITY, best1 = -INFINITY;
  int bi0 = 0x7fffffff, bi1 = 0x7fffffff;
  for (int c = lane; c < V; c += 64) {
    float a0 = 0.f, a1 = 0.f;
    for (int d = 0; d < D; d++) {
      const float wv = w[(size_t)d * V + c];
      a0 = __fmaf_rn(x0[d], wv, a0);
      a1 = __fmaf_rn(x1[d], wv, a1);
    }
    a0 += b[c]; a1 += b[c];
    if (logits) {
      if (r0 < rows) logits[((size_t)f0 + t0 + r0) * V + c] = a0;
      if (r1 < rows) logits[((size_t)f0 + t0 + r1) * V + c] = a1;
    }
    if (a0 > best0) { best0 = a0; bi0 = c; }
    if (a1 > best1) { best1 = a1; bi1 = c; }
  }
  for (int d = 32; d; d >>= 1) {
    const float o0 = __shfl_xor(best0, d), o1 = __shfl_xor(best1, d);
    const int i0 = __shfl_xor(bi0, d), i1 = __shfl_xor(bi1, d);
    if (o0 > best0 || (o0 == best0 && i0 < bi0)) { best0 = o0; bi0 = i0; }
    if (o1 > best1 || (o1 == best1 && i1 < bi1)) { best1 = o1; bi1 = i1; }
  }
  if (lane == 0) {
    if (r0 < rows) ids[(size_t)f0 + t0 + r0] = bi0 < V ? bi0 : 0;
    if (r1 < rows) ids[(size_t)f0 + t0 + r1] = bi1 < V ? bi1 : 0;
  }
}

// ---- the launches, stated once for aligner_run and for the test harness (testlib/w2v_harness.hip) ----
// part: [tiles of all clips] double2; stat: [B] double2
void w2v_launch_stats(const float *x, const int *d_seq0, int max_n, int B, double2 *part, double2 *stat, hipStream_t st) {
  w2v_stat_partial_kernel<<<dim3((unsigned)((max_n + W2V_ST_TILE - 1) / W2V_ST_TILE), (unsigned)B), 256, 0, st>>>(x, d_seq0, part);
  w2v_stat_finish_kernel<<<(unsigned)B, 64, 0, st>>>(part, d_seq0, 1e-7, stat);
}
void w2v_launch_stem(const float *x, const double2 *stat, const float *w, const float *b, const int *d_seq0, const int *d_seq1, int C, int taps, int stride,
                     int max_out, int B, float *out, hipStream_t st) {
  const size_t lds = (size_t)((W2V_STEM_ROWS - 1) * stride + taps) * 4;
  w2v_stem_kernel<<<dim3((unsigned)((max_out + W2V_STEM_ROWS - 1) / W2V_STEM_ROWS), (unsigned)B), 256, lds, st>>>(x, stat, w, b, d_seq0, d_seq1, C, taps, stride, out);
}
void w2v_launch_ln(const float *x, float *y, const float *gamma, const float *beta, const int *d_seq, int C, int gelu, int max_n, int B, hipStream_t st) {
  w2v_ln_kernel<<<dim3((unsigned)((max_n + 3) / 4), (unsigned)B), 256, 0, st>>>(x, gamma, beta, d_seq, C, gelu, y);
}
void w2v_launch_gelu(float *x, const int *d_seq, int C, int max_n, int B, hipStream_t st) {
  w2v_gelu_kernel<<<dim3((unsigned)((max_n + W2V_ROW_TILE - 1) / W2V_ROW_TILE), (unsigned)B), 256, 0, st>>>(x, d_seq, C);
}
void w2v_launch_pos(const W2vPos &a, int max_n, int B, hipStream_t st) {
  const dim3 grid((unsigned)((max_n + W2V_PTM - 1) / W2V_PTM), (unsigned)B, (unsigned)(a.D / 64));
  w2v_pos_kernel<<<grid, 256, w2v_pos_lds(a.cg, a.K), st>>>(a);
}
void w2v_launch_head(const float *x, const float *w, const float *b, const int *d_seq, int D, int V, int max_n, int B, int *ids, float *logits, hipStream_t st) {
  const dim3 grid((unsigned)((max_n + W2V_HEAD_ROWS - 1) / W2V_HEAD_ROWS), (unsigned)B);
  w2v_head_kernel<<<grid, 256, (size_t)W2V_HEAD_ROWS * D * 4, st>>>(x, w, b, d_seq, D, V, ids, logits);
}
// what the reused and the new kernels can tile: the head of this file states the rule
bool w2v_channels_ok(int c) { return c >= 64 && c <= W2V_MAX_C && c % 64 == 0; }
inline int w2v_conv_frames(int64_t n, int k, int s) { return n < k ? 0 : (int)((n - k) / s + 1); }
// The tables of aligner_run (and of the test harness): level 0 = the samples, level i the output of convolution i - 1 (k[i - 1] taps, stride s[i - 1], no
// padding); a clip's first row a multiple of 8; level 0 carries the clip's first statistics tile and its first sample at 16 kHz
template <class T>
LevelTable w2v_levels(const T *n, int B, int N, const int *k, const int *s) {
  return level_table(n, B, N + 1, [k, s](int64_t v, int l) { return w2v_conv_frames(v, k[l], s[l]); }, 8, W2V_ST_TILE, false);
}
} // namespace

// The model as the loader's host half leaves it (no device call): the configuration from the tensor shapes, every tensor repacked for the kernels.
// HostLayer w: a Linear's [cin][cout], a convolution's [tap][cin][cout], a LayerNorm's gamma
struct W2vHostLayer { HostLayer n1, n2, qkv, out, w1, w2; }; // qkv: [D][3 D], q | k | v, head h at columns h * 64 of each
struct W2vHost {
  int N = 0, C = 0, D = 0, K = 0, cg = 0, depth = 0, FF = 0, V = 0, H = 16, blank = 0;
  std::vector<int> k, s;
  std::vector<HostLayer> conv, conv_n; // conv[0] keeps PyTorch's [C][1][k_0]
  HostLayer proj_n, enc_n;
  HostLayer proj, pos, head; // pos: [group][tap][cin][cout]; head: [D][V]
  std::vector<W2vHostLayer> layers;
  std::vector<int32_t> vocab;
};

int aligner_parse(tts_ctx *ctx, const WeightFile &wf, const char *path, W2vHost &h) {
  const std::string P = "aligner.", FE = P + "feature_extractor.conv_layers.", EN = P + "encoder.";
  if (!wf.has(FE + "0.conv.weight")) return fail(ctx, TTS_ERR_FORMAT, "'%s' is not an aligner model file", path);
  ModelReader rd{wf, ctx, "aligner"};
  // the configuration: N, C and k_i from the convolutions; D from the projection; K and D / G from pos_conv; depth and the width from the layers; V from lm_head
  while (wf.has(FE + std::to_string(h.N) + ".conv.weight")) h.N++;
  if (h.N > W2V_MAX_CONV) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: %d convolution layers (at most %d)", h.N, W2V_MAX_CONV);
  for (int i = 0; i < h.N; i++) {
    const HostTensor *t = rd.peek(FE + std::to_string(i) + ".conv.weight", 3);
    if (!t) return fail(ctx, TTS_ERR_FORMAT, "tensor '%s%d.conv.weight' has wrong shape in aligner model file (3 dims)", FE.c_str(), i);
    if (i == 0) h.C = (int)t->ne[2];
    h.k.push_back((int)t->ne[0]);
    // the base model: a GroupNorm behind the first convolution only, no convolution bias
    if (!wf.has(FE + std::to_string(i) + ".layer_norm.weight") || !wf.has(FE + std::to_string(i) + ".conv.bias"))
      return fail(ctx, TTS_ERR_FORMAT, "aligner model file: convolution layer %d has no LayerNorm or no bias: the group-norm (base-model) variant is not supported", i);
  }
  if (!w2v_channels_ok(h.C)) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: %d extractor channels (a multiple of 64, 64 .. %d)", h.C, W2V_MAX_C);
  if (h.k[0] < 1 || h.k[0] > 64) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: first kernel size %d (1 .. 64)", h.k[0]);
  for (int i = 1; i < h.N; i++)
    if (h.k[i] < 1 || h.k[i] > 16) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: kernel size %d of convolution layer %d (1 .. 16)", h.k[i], i);
  {
    const HostTensor *t = rd.peek(P + "feature_projection.projection.weight", 2);
    h.D = t ? (int)t->ne[1] : 0;
    if (!w2v_channels_ok(h.D)) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: model dimension %d (a multiple of 64, 64 .. %d)", h.D, W2V_MAX_C);
  }
  {
    const HostTensor *t = rd.peek(EN + "pos_conv_embed.conv.weight", 3);
    if (!t) return fail(ctx, TTS_ERR_FORMAT,
                        "tensor '%spos_conv_embed.conv.weight' missing from aligner model file (the converter folds weight_g / weight_v into it)", EN.c_str());
    h.K = (int)t->ne[0]; h.cg = (int)t->ne[1];
    if (h.cg < 64 || h.cg % 64 || h.D % h.cg || h.K < 1 || w2v_pos_lds(h.cg, h.K) > 65536)
      return fail(ctx, TTS_ERR_FORMAT, "aligner model file: positional convolution with %d taps over groups of %d channels (groups a multiple of 64 that divides %d, "
                  "(63 + taps) x (group + 1) floats inside 64 KB)", h.K, h.cg, h.D);
  }
  while (wf.has(EN + "layers." + std::to_string(h.depth) + ".layer_norm.weight")) h.depth++;
  if (h.depth < 1) return fail(ctx, TTS_ERR_FORMAT, "tensor '%slayers.0.layer_norm.weight' missing from aligner model file", EN.c_str());
  {
    const HostTensor *t = rd.peek(EN + "layers.0.feed_forward.intermediate_dense.weight", 2);
    h.FF = t ? (int)t->ne[1] : 0;
    if (h.FF < 64 || h.FF % 64) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: feed-forward width %d (a multiple of 64)", h.FF);
    t = rd.peek(P + "lm_head.weight", 2);
    h.V = t ? (int)t->ne[1] : 0;
    if (h.V < 1 || h.V > W2V_MAX_V) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: vocabulary of %d tokens (1 .. %d)", h.V, W2V_MAX_V);
  }
  h.s.assign(h.N, 2);
  h.s[0] = 5;
  if (wf.has(P + "config")) { // what no shape holds: {heads, blank id, s_0 .. s_{N-1}}, integers
    const HostTensor *t = rd.need(P + "config", 2 + h.N, 0, 0);
    if (!t) return TTS_ERR_FORMAT;
    for (float v : t->data)
      if (v != (float)(int)v) return fail(ctx, TTS_ERR_FORMAT, "tensor 'aligner.config' holds %g: {heads, blank id, strides} are integers", (double)v);
    h.H = (int)t->data[0]; h.blank = (int)t->data[1];
    for (int i = 0; i < h.N; i++) h.s[i] = (int)t->data[2 + i];
  }
  for (int i = 0; i < h.N; i++)
    if (h.s[i] < 1 || h.s[i] > (i ? 4 : 8)) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: stride %d of convolution layer %d (1 .. %d)", h.s[i], i, i ? 4 : 8);
  if (h.H < 1 || h.D % h.H || h.D / h.H != 64)
    return fail(ctx, TTS_ERR_FORMAT, "aligner model file: %d channels in %d heads: the head dimension must be 64", h.D, h.H);
  if (h.blank < 0 || h.blank >= h.V) return fail(ctx, TTS_ERR_FORMAT, "aligner model file: blank id %d outside the vocabulary of %d", h.blank, h.V);
  {
    const HostTensor *t = rd.need(P + "vocab", h.V, 0, 0);
    if (!t) return TTS_ERR_FORMAT;
    h.vocab.resize(h.V);
    for (int i = 0; i < h.V; i++) {
      const float v = t->data[i];
      if (v != (float)(int)v || v < -1 || v > 0x10ffff) return fail(ctx, TTS_ERR_FORMAT, "tensor 'aligner.vocab' holds %g: a code point or -1", (double)v);
      h.vocab[i] = (int)v;
    }
  }
  int rc;
  h.conv.resize(h.N); h.conv_n.resize(h.N);
  for (int i = 0; i < h.N; i++) {
    const std::string p = FE + std::to_string(i);
    if ((rc = i ? rd.conv(p + ".conv", h.C, h.C, h.k[i], h.conv[i]) : rd.raw(p + ".conv", h.C, 1, h.k[0], h.conv[0])) ||
        (rc = rd.norm(p + ".layer_norm", h.C, h.conv_n[i])))
      return rc;
  }
  if ((rc = rd.norm(P + "feature_projection.layer_norm", h.C, h.proj_n)) || (rc = rd.linear(P + "feature_projection.projection", h.D, h.C, h.proj))) return rc;
  { // the grouped convolution [g cg + cout][cin][k] -> [g][k][cin][cout]
    const int D = h.D, cg = h.cg, K = h.K;
    HostLayer raw;
    if ((rc = rd.raw(EN + "pos_conv_embed.conv", D, cg, K, raw))) return rc;
    h.pos.w.resize((size_t)D * cg * K);
    for (int g = 0; g < D / cg; g++)
      for (int co = 0; co < cg; co++)
        for (int ci = 0; ci < cg; ci++)
          for (int j = 0; j < K; j++) h.pos.w[(((size_t)g * K + j) * cg + ci) * cg + co] = raw.w[((size_t)(g * cg + co) * cg + ci) * K + j];
    h.pos.b = raw.b;
  }
  h.layers.resize(h.depth);
  for (int l = 0; l < h.depth; l++) {
    const std::string p = EN + "layers." + std::to_string(l);
    W2vHostLayer &y = h.layers[l];
    const int D = h.D;
    HostLayer q[3];
    if ((rc = rd.norm(p + ".layer_norm", D, y.n1)) || (rc = rd.linear(p + ".attention.q_proj", D, D, q[0])) || (rc = rd.linear(p + ".attention.k_proj", D, D, q[1])) ||
        (rc = rd.linear(p + ".attention.v_proj", D, D, q[2])) || (rc = rd.linear(p + ".attention.out_proj", D, D, y.out)) ||
        (rc = rd.norm(p + ".final_layer_norm", D, y.n2)) || (rc = rd.linear(p + ".feed_forward.intermediate_dense", h.FF, D, y.w1)) ||
        (rc = rd.linear(p + ".feed_forward.output_dense", D, h.FF, y.w2)))
      return rc;
    y.qkv.w.resize((size_t)3 * D * D); y.qkv.b.resize((size_t)3 * D); // the q | k | v blocks cls_attn_kernel reads
    for (int j = 0; j < 3; j++) {
      for (int ci = 0; ci < D; ci++) memcpy(&y.qkv.w[(size_t)ci * 3 * D + (size_t)j * D], &q[j].w[(size_t)ci * D], (size_t)D * 4);
      memcpy(&y.qkv.b[(size_t)j * D], q[j].b.data(), (size_t)D * 4);
    }
  }
  if ((rc = rd.norm(EN + "layer_norm", h.D, h.enc_n)) || (rc = rd.linear(P + "lm_head", h.V, h.D, h.head))) return rc;
  return rd.finish(path);
}

struct W2vLayer { HfgLayer n1, n2, qkv, out, w1, w2; };
struct AlignerState {
  int N = 0, C = 0, D = 0, K = 0, cg = 0, depth = 0, FF = 0, V = 0, H = 16, blank = 0;
  std::vector<int> k, s;
  std::vector<int32_t> vocab;
  std::vector<HfgLayer> conv, conv_n;
  HfgLayer proj_n, enc_n;
  HfgLayer proj, pos, head;
  std::vector<W2vLayer> layers;
  DevWeights dev;
  DevBuf in, wav, part, stat, a, t, h, h2, y, qkv, att, ff, ids, logits;
};
void aligner_free(AlignerState *s) { delete s; }

// The file is parsed before the device is asked for: a host-only context reports a broken file as TTS_ERR_FORMAT and a good one as TTS_ERR_HIP.
int aligner_load(tts_ctx *ctx, const char *path) {
  if (!path) return fail(ctx, TTS_ERR_ARG, "tts_load_aligner: bad argument");
  WeightFile wf;
  std::string err;
  int rc = read_weight_file(path, wf, err);
  if (rc != TTS_OK) return fail(ctx, rc, "aligner_load: %s", err.c_str());
  std::unique_ptr<W2vHost> h(new W2vHost());
  if ((rc = aligner_parse(ctx, wf, path, *h))) return rc;
  if (ctx->device < 0) return fail(ctx, TTS_ERR_HIP, "host-only context: no HIP device, no CPU fallback");
  (void)hipSetDevice(ctx->device);
  std::unique_ptr<AlignerState> st(new AlignerState());
  st->N = h->N; st->C = h->C; st->D = h->D; st->K = h->K; st->cg = h->cg; st->depth = h->depth; st->FF = h->FF; st->V = h->V; st->H = h->H; st->blank = h->blank;
  st->k = h->k; st->s = h->s; st->vocab = h->vocab;
  auto up = [&](const HostLayer &s, HfgLayer &d) { return st->dev.up(ctx, s, d); };
  st->conv.resize(h->N); st->conv_n.resize(h->N); st->layers.resize(h->depth);
  for (int i = 0; i < h->N; i++)
    if ((rc = up(h->conv[i], st->conv[i])) || (rc = up(h->conv_n[i], st->conv_n[i]))) return rc;
  if ((rc = up(h->proj_n, st->proj_n)) || (rc = up(h->proj, st->proj)) || (rc = up(h->pos, st->pos)) || (rc = up(h->enc_n, st->enc_n)) ||
      (rc = up(h->head, st->head)))
    return rc;
  for (int l = 0; l < h->depth; l++) {
    const W2vHostLayer &s = h->layers[l];
    W2vLayer &d = st->layers[l];
    if ((rc = up(s.n1, d.n1)) || (rc = up(s.n2, d.n2)) || (rc = up(s.qkv, d.qkv)) || (rc = up(s.out, d.out)) || (rc = up(s.w1, d.w1)) || (rc = up(s.w2, d.w2)))
      return rc;
  }
  if (ctx->aligner) aligner_free(ctx->aligner);
  ctx->aligner = st.release();
  return TTS_OK;
}

// V, the blank id and the code point of every token (-1: no single character), for the host-side decode and alignment
int aligner_vocab(tts_ctx *ctx, int32_t *vocab_out, int cap, int32_t *blank_out) {
  const AlignerState *st = ctx->aligner;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_aligner not called");
  if (vocab_out) {
    if (cap < st->V) return fail(ctx, TTS_ERR_ARG, "tts_aligner_vocab: room for %d of %d tokens", cap, st->V);
    memcpy(vocab_out, st->vocab.data(), (size_t)st->V * 4);
  }
  if (blank_out) *blank_out = st->blank;
  return st->V;
}

// Frames of a clip of n samples at `rate` Hz under the loaded configuration (what tts_aligner_ids will write for it), or a negative status
int aligner_clip_frames(tts_ctx *ctx, int64_t n, int rate) {
  const AlignerState *st = ctx->aligner;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_aligner not called");
  if (n < 1) return fail(ctx, TTS_ERR_ARG, "tts_aligner_clip_frames: %lld samples", (long long)n);
  if (n > (1 << 26)) return fail(ctx, TTS_ERR_LIMIT, "tts_aligner_clip_frames: %lld samples, at most 2^26", (long long)n);
  AfeResampleGeom g;
  if (rate < 1 || afe_resample_geometry(rate, 16000, &g) != TTS_OK)
    return fail(ctx, TTS_ERR_ARG, "tts_aligner_clip_frames: sample rate %d is outside the audio front end's range", rate);
  int64_t f = rate == 16000 ? n : afe_resample_len(g, n);
  for (int i = 0; i < st->N; i++) f = w2v_conv_frames(f, st->k[i], st->s[i]);
  if (f < 1) return fail(ctx, TTS_ERR_ARG, "tts_aligner_clip_frames: %lld samples at %d Hz leave less than one frame", (long long)n, rate);
  return (int)f;
}

// One upload (samples, tables), one launch sequence for the whole ragged batch, one download. Nothing of it depends on the batch: a clip's ids and logits are
// the same bits alone or in any batch. The stage owns its buffers and touches no AR or diffusion state, so it is legal while sessions are open.
// ids_out [B][frame_stride], logits_out null or [B][frame_stride][V]: the first n_frames_out[s] entries of a clip are written, the rest is left alone.
int aligner_run(tts_ctx *ctx, const float *audio, const int64_t *n_samples, const int32_t *rates, int B, int32_t *ids_out, int32_t *n_frames_out, int frame_stride,
                float *logits_out, ClsResampleFn resample) {
  const char *fn = "tts_aligner_ids";
  AlignerState *st = ctx->aligner;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_aligner not called");
  if (!audio || !n_samples || !rates || !ids_out || !n_frames_out || !resample || B < 1 || frame_stride < 1) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", fn);
  if (B > W2V_MAX_CLIPS) return fail(ctx, TTS_ERR_LIMIT, "%s: %d clips (at most %d per call)", fn, B, W2V_MAX_CLIPS);
  const int N = st->N, C = st->C, D = st->D, V = st->V;
  ClipIngest clips;
  std::vector<int> frames(B);
  int rc = clip_ingest(ctx, fn, audio, n_samples, rates, B, 16000, 0, clips, [&](int s, int64_t n16) {
    int64_t f = n16;
    for (int i = 0; i < N; i++) f = w2v_conv_frames(f, st->k[i], st->s[i]);
    if (f < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %lld samples at 16 kHz leave less than one frame", fn, s, (long long)n16);
    if (f > frame_stride) return fail(ctx, TTS_ERR_ARG, "%s: clip %d has %d frames, frame_stride is %d", fn, s, (int)f, frame_stride);
    frames[s] = (int)f;
    return (int)TTS_OK;
  });
  if (rc) return rc;
  const LevelTable lt = w2v_levels(clips.n_dst.data(), B, N, st->k.data(), st->s.data());
  const std::vector<int64_t> &rows = lt.rows;
  const std::vector<int> &max_n = lt.max_n;
  const int64_t R = rows[N], total16 = clips.total_dst;
  TTS_HIP(ctx, st->in.reserve(clip_upload_floats(clips, lt) * 4));
  TTS_HIP(ctx, st->wav.reserve((size_t)total16 * 4));
  TTS_HIP(ctx, st->part.reserve((size_t)lt.tiles[0] * sizeof(double2)));
  TTS_HIP(ctx, st->stat.reserve((size_t)B * sizeof(double2)));
  TTS_HIP(ctx, st->a.reserve((size_t)rows[1] * C * 4));
  TTS_HIP(ctx, st->t.reserve((size_t)rows[1] * C * 4));
  TTS_HIP(ctx, st->h.reserve((size_t)R * D * 4));
  TTS_HIP(ctx, st->h2.reserve((size_t)R * D * 4));
  TTS_HIP(ctx, st->y.reserve((size_t)R * D * 4));
  TTS_HIP(ctx, st->qkv.reserve((size_t)R * 3 * D * 4));
  TTS_HIP(ctx, st->att.reserve((size_t)R * D * 4));
  TTS_HIP(ctx, st->ff.reserve((size_t)R * st->FF * 4));
  TTS_HIP(ctx, st->ids.reserve((size_t)R * 4));
  if (logits_out) TTS_HIP(ctx, st->logits.reserve((size_t)R * V * 4));
  hipStream_t sm = ctx->stream;
  float *wav = st->wav.as<float>();
  const int *d_tab = nullptr;
  if ((rc = clip_upload(ctx, clips, lt, audio, rates, 16000, st->in, wav, resample, &d_tab))) return rc;
  auto seq = [&](int l) { return d_tab + (size_t)l * B * HFG_SEQ; };
  float *a = st->a.as<float>(), *t = st->t.as<float>(), *h = st->h.as<float>(), *h2 = st->h2.as<float>(), *y = st->y.as<float>();
  float *qkv = st->qkv.as<float>(), *att = st->att.as<float>(), *ff = st->ff.as<float>();
  double2 *stat = st->stat.as<double2>();
  auto ln = [&](const float *x, float *out, const HfgLayer &p, int l, int ch, int gelu) {
    ProfScope ps(ctx, "w2v_row", (double)rows[l] * ch * 4 * 2);
    w2v_launch_ln(x, out, p.w, p.b, seq(l), ch, gelu, max_n[l], B, sm);
  };
  auto linear = [&](const float *in, float *out, const float *resid, const HfgLayer &w, int cin, int cout) {
    ProfScope ps(ctx, "w2v_conv", 2.0 * (double)R * cin * cout);
    cls_launch_conv(in, out, resid, w.w, w.b, seq(N), cin, cout, 1, max_n[N], B, sm);
  };
  {
    ProfScope ps(ctx, "w2v_row", (double)total16 * 4);
    w2v_launch_stats(wav, seq(0), max_n[0], B, st->part.as<double2>(), stat, sm);
  }
  {
    ProfScope ps(ctx, "w2v_conv", 2.0 * (double)rows[1] * st->k[0] * C);
    w2v_launch_stem(wav, stat, st->conv[0].w, st->conv[0].b, seq(0), seq(1), C, st->k[0], st->s[0], max_n[1], B, a, sm);
  }
  ln(a, a, st->conv_n[0], 1, C, 1);
  for (int i = 1; i < N; i++) {
    ClsDown d{};
    d.in = a; d.out = t; d.w = st->conv[i].w; d.bias = st->conv[i].b; d.seq_in = seq(i); d.seq_out = seq(i + 1);
    d.cin = C; d.cout = C; d.taps = st->k[i]; d.stride = st->s[i]; d.pad = 0;
    {
      ProfScope ps(ctx, "w2v_conv", 2.0 * (double)rows[i + 1] * st->k[i] * C * C);
      cls_launch_down(d, max_n[i + 1], B, sm);
    }
    ln(t, t, st->conv_n[i], i + 1, C, 1);
    std::swap(a, t);
  }
  ln(a, t, st->proj_n, N, C, 0);
  linear(t, h, nullptr, st->proj, C, D);
  {
    W2vPos p{};
    p.in = h; p.out = h2; p.w = st->pos.w; p.bias = st->pos.b; p.seq = seq(N); p.D = D; p.cg = st->cg; p.K = st->K;
    ProfScope ps(ctx, "w2v_conv", 2.0 * (double)R * st->K * st->cg * D);
    w2v_launch_pos(p, max_n[N], B, sm);
    std::swap(h, h2);
  }
  for (const W2vLayer &l : st->layers) {
    ln(h, y, l.n1, N, D, 0);
    linear(y, qkv, nullptr, l.qkv, D, 3 * D);
    {
      ProfScope ps(ctx, "w2v_attn", 4.0 * (double)R * max_n[N] * D);
      cls_launch_attn(qkv, att, seq(N), D, st->H, max_n[N], B, sm);
    }
    linear(att, h, h, l.out, D, D); // the residual add in the epilogue: an element is read and written by the same thread
    ln(h, y, l.n2, N, D, 0);
    linear(y, ff, nullptr, l.w1, D, st->FF);
    {
      ProfScope ps(ctx, "w2v_row", (double)R * st->FF * 4 * 2);
      w2v_launch_gelu(ff, seq(N), st->FF, max_n[N], B, sm);
    }
    linear(ff, h, h, l.w2, st->FF, D);
  }
  ln(h, y, st->enc_n, N, D, 0);
  {
    ProfScope ps(ctx, "w2v_conv", 2.0 * (double)R * D * V);
    w2v_launch_head(y, st->head.w, st->head.b, seq(N), D, V, max_n[N], B, st->ids.as<int>(), logits_out ? st->logits.as<float>() : nullptr, sm);
  }
  TTS_HIP(ctx, hipGetLastError());
  std::vector<int32_t> ids((size_t)R);
  std::vector<float> lg(logits_out ? (size_t)R * V : 0);
  TTS_HIP(ctx, hipMemcpyAsync(ids.data(), st->ids.p, ids.size() * 4, hipMemcpyDeviceToHost, sm));
  if (logits_out) TTS_HIP(ctx, hipMemcpyAsync(lg.data(), st->logits.p, lg.size() * 4, hipMemcpyDeviceToHost, sm));
  TTS_HIP(ctx, hipStreamSynchronize(sm));
  for (int s = 0; s < B; s++) {
    const size_t f0 = (size_t)lt.rec(N, s)[0];
    n_frames_out[s] = frames[s];
    memcpy(ids_out + (size_t)s * frame_stride, &ids[f0], (size_t)frames[s] * 4);
    if (logits_out) memcpy(logits_out + (size_t)s * frame_stride * V, &lg[f0 * V], (size_t)frames[s] * V * 4);
  }
  return TTS_OK;
}

} // namespace tts

#include "dvae.h" // the DVAE encoder: the same translation unit, the classifier's strided convolution and hfg_conv_kernel
