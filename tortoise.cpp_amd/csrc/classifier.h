// tortoise-detect on MI355X (gfx950): a 24 kHz waveform -> "probability that the clip came from Tortoise"      tts_load_classifier / tts_classify_audio
//
// Included once, as the last line of bigvgan.h (itself the last line of hifigan.hip, whose model_io.h holds the tensor reader, the weight store, the level
// tables and the clip ingest used here): upstream's AudioMiniEncoderWithClassifierHead is a convolutional encoder on the raw
// waveform whose C -> C convolutions ARE hfg_conv_kernel<1|2> with slope 1, no conditioning vector and voice 0, on HFG_SEQ records with one row per "frame"
// (rate 1), one table per level. Upstream's source and weights are not available offline: the contract is the arithmetic of DESIGN.md ("What pins the
// classifier"), checked between two float64 spellings (tests/classifier_ref.py); unpinned against upstream, unjudged on real audio.
//
//   x = clamp(clip at 24 kHz, -1, 1)[: 220 000]                                        n rows of 1 channel
//   h = Conv1d(1 -> B0, k 3, pad 1)(x)                                                 cls_stem_kernel
//   level l = 0 .. depth - 1, C = B0 2^l:
//     resnet_blocks x   h = h + conv_b(SiLU(GN(conv_a(SiLU(GN(h))))))                  cls_gn_* + hfg_conv_kernel (k K, zero padding at the clip's ends)
//     h = Conv1d(C -> 2C, k 5, stride F, pad 2)(h)                                     cls_down_kernel, n -> (n - 1) / F + 1
//   h = Conv1d(B0 2^depth -> E, k 1)(SiLU(GN(h)))                                      cls_gn_* + hfg_conv_kernel
//   attn_blocks x   h = h + proj_out(QKVAttentionLegacy(qkv(GN32(h))))                 cls_gn_* (no SiLU), hfg_conv_kernel (k 1), cls_attn_kernel<64 | 128>
//   logits = Linear(E -> 2)(h[position 0]), p = softmax(logits)[0]                     cls_head_kernel
//
// Device layout: time-major f32 rows [row][C]; clip s owns the rows [start_s, start_s + n_s) of a level, start_s a multiple of 8. No kernel reads or writes a
// row outside the clip it works on (the convolutions predicate their staging loads; the GroupNorm tiles end at the clip's end).
//
// GroupNorm over up to 220 000 rows of a group that is 2 channels wide: per-tile partial sums in DOUBLE (cls_gn_partial_kernel: sum and sum of squares of
// CLS_GN_TILE rows, each thread's rows ascending, then the threads of a group in one fixed order), reduced over the tiles in one fixed order by
// cls_gn_finish_kernel, which leaves mean and 1 / sqrt(var + eps) per (clip, group) in double; cls_gn_silu_kernel subtracts the double mean from the widened
// sample before it rounds. No atomics: two runs agree bit for bit, and the tiles of a clip are the clip's own, so a clip alone equals the clip in a batch.
// Double partials rather than shifted or pairwise f32 sums: a product of two f32 is exact in double and 2 x 220 000 of them lose under 2^-34 relative, so
// var = E[x^2] - mean^2 keeps 2^-34 (mean / deviation)^2 — 6e-7 of the variance at |mean| = 100 deviations — with no second pass over the rows.
//
// The attention blocks are f32 throughout (the projections on hfg_conv_kernel's exact-f32 MFMA, scores, softmax and P V in f32 registers), NOT attn_block_run
// (encoder.h), whose GEMM operands are fp16: with fp16 operands the logits sat 4e-4 .. 1.7e-3 from float64 on an MI355X, outside the 1e-3 gate
// ("What pins the classifier"). At 215 positions per clip they are under 2 % of the stage's arithmetic either way.
#pragma once

namespace tts {

namespace {
constexpr int CLS_GN_TILE = 256;  // rows of a GroupNorm partial-sum tile (and of a cls_gn_silu_kernel workgroup)
constexpr int CLS_STEM_ROWS = 64; // rows of a cls_stem_kernel workgroup
constexpr int CLS_DTM = 64;       // output rows of a cls_down_kernel workgroup: 2 row halves x 2 column groups of 32 over its 4 waves
constexpr int CLS_MAX_C = 1024, CLS_MAX_DEPTH = 8, CLS_MAX_CLIPS = 256;

// GroupNorm32's group count as upstream's normalization(): 32, or 16 if C <= 64, or 8 if C <= 16, halved while it does not divide C
__host__ __device__ inline int cls_groups(int C) {
  int g = C <= 16 ? 8 : C <= 64 ? 16 : 32;
  while (C % g) g /= 2;
  return g;
}

// h[t][c] = b[c] + sum_k w[c][k] clamp(x[t - 1 + k]), k ascending, one fmaf per tap; x outside the clip is the convolution's zero padding.
// seq record: {first row, rows, 0, first GroupNorm tile, first sample of the clip in x}
__global__ __launch_bounds__(256) void cls_stem_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ b,
                                                       const int *__restrict__ seq, int C, float *__restrict__ out) {
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * CLS_STEM_ROWS;
  if (t0 >= n) return;
  const float *xs = x + (size_t)seq[HFG_SEQ * s + 4];
  const int rows = min(CLS_STEM_ROWS, n - t0);
  for (int idx = threadIdx.x; idx < rows * C; idx += 256) {
    const int t = t0 + idx / C, c = idx % C;
    float acc = b[c];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int i = t - 1 + k;
      const float v = (i >= 0 && i < n) ? fminf(fmaxf(xs[i], -1.0f), 1.0f) : 0.f;
      acc = __fmaf_rn(w[c * 3 + k], v, acc);
    }
    out[((size_t)f0 + t) * C + c] = acc;
  }
}

// Partial sums of one tile of one clip: part[(first tile of the clip + tile) * G + g] = {sum, sum of squares} over the tile's rows and the group's channels,
// in double. A thread owns 4 consecutive channels and every (1024 / C)-th row of the tile; thread g < G then adds the group's terms channel by channel, row
// phase by row phase. C: a power of two, 32 .. 1024.
__global__ __launch_bounds__(256) void cls_gn_partial_kernel(const float *__restrict__ x, const int *__restrict__ seq, int C, int G, double2 *__restrict__ part) {
  __shared__ double ssum[256 * 4], ssq[256 * 4];
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * CLS_GN_TILE;
  if (t0 >= n) return;
  const int t1 = min(t0 + CLS_GN_TILE, n), qpr = C / 4, rpp = 256 / qpr; // quads per row, rows per pass
  const int q = threadIdx.x % qpr, r = threadIdx.x / qpr;
  double a[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
  for (int t = t0 + r; t < t1; t += rpp) {
    const float4 v = *(const float4 *)(x + ((size_t)f0 + t) * C + 4 * q);
    const double d0 = v.x, d1 = v.y, d2 = v.z, d3 = v.w;
    a[0] += d0; a[1] += d1; a[2] += d2; a[3] += d3;
    a2[0] += d0 * d0; a2[1] += d1 * d1; a2[2] += d2 * d2; a2[3] += d3 * d3;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) { ssum[threadIdx.x * 4 + i] = a[i]; ssq[threadIdx.x * 4 + i] = a2[i]; }
  __syncthreads();
  if ((int)threadIdx.x < G) {
    const int cg = C / G, g = threadIdx.x;
    double sm = 0, sq = 0;
    for (int c = g * cg; c < (g + 1) * cg; c++)
      for (int p = 0; p < rpp; p++) {
        const int i = (p * qpr + c / 4) * 4 + (c & 3);
        sm += ssum[i]; sq += ssq[i];
      }
    part[((size_t)seq[HFG_SEQ * s + 3] + blockIdx.x) * G + g] = make_double2(sm, sq);
  }
}

// stat[s * G + g] = {mean, 1 / sqrt(var + eps)} (biased variance) from the clip's tiles: thread j adds tiles j, j + 64, .. ascending, thread 0 the 64 sums ascending
__global__ __launch_bounds__(64) void cls_gn_finish_kernel(const double2 *__restrict__ part, const int *__restrict__ seq, int C, int G, double eps,
                                                          double2 *__restrict__ stat) {
  __shared__ double rs[64], rq[64];
  const int s = blockIdx.y, g = blockIdx.x;
  const int n = seq[HFG_SEQ * s + 1], tiles = (n + CLS_GN_TILE - 1) / CLS_GN_TILE;
  const double2 *p = part + (size_t)seq[HFG_SEQ * s + 3] * G + g;
  double sm = 0, sq = 0;
  for (int t = threadIdx.x; t < tiles; t += 64) { const double2 v = p[(size_t)t * G]; sm += v.x; sq += v.y; }
  rs[threadIdx.x] = sm; rq[threadIdx.x] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    sm = 0; sq = 0;
    for (int j = 0; j < 64; j++) { sm += rs[j]; sq += rq[j]; }
    const double cnt = (double)(C / G) * (double)n, mean = sm / cnt;
    const double var = fmax(sq / cnt - mean * mean, 0.0);
    stat[(size_t)s * G + g] = make_double2(mean, 1.0 / sqrt(var + eps));
  }
}

__device__ __forceinline__ float cls_silu(float v) { return v / (1.0f + expf(-v)); }

// y = SiLU(((float)(x - mean) * rstd) * gamma + beta): the convolution's operand (silu 0: the attention blocks' GroupNorm, no activation). x and y never alias.
__global__ __launch_bounds__(256) void cls_gn_silu_kernel(const float *__restrict__ x, const double2 *__restrict__ stat, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, const int *__restrict__ seq, int C, int G, int silu,
                                                          float *__restrict__ y) {
  __shared__ double smean[32];
  __shared__ float srstd[32];
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * CLS_GN_TILE;
  if (t0 >= n) return;
  if ((int)threadIdx.x < G) { const double2 v = stat[(size_t)s * G + threadIdx.x]; smean[threadIdx.x] = v.x; srstd[threadIdx.x] = (float)v.y; }
  __syncthreads();
  const int rows = min(CLS_GN_TILE, n - t0), qpr = C / 4, cg = C / G;
  for (int idx = threadIdx.x; idx < rows * qpr; idx += 256) {
    const int t = t0 + idx / qpr, c = 4 * (idx % qpr);
    const size_t o = ((size_t)f0 + t) * C + c;
    const float4 v = *(const float4 *)(x + o), ga = *(const float4 *)(gamma + c), be = *(const float4 *)(beta + c);
    const float in[4] = {v.x, v.y, v.z, v.w}, gg[4] = {ga.x, ga.y, ga.z, ga.w}, bb[4] = {be.x, be.y, be.z, be.w};
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int g = (c + i) / cg;
      const float d = (float)((double)in[i] - smean[g]);
      const float v = __fmaf_rn(__fmul_rn(d, srstd[g]), gg[i], bb[i]);
      r[i] = silu ? cls_silu(v) : v;
    }
    *(float4 *)(y + o) = make_float4(r[0], r[1], r[2], r[3]);
  }
}

struct ClsDown {
  const float *in;   // [rows_in][cin]
  float *out;        // [rows_out][cout]
  const float *w;    // [tap][cin][cout]
  const float *bias; // [cout]
  const int *seq_in, *seq_out;
  int cin, cout, taps, stride, pad; // input row of tap j for output row t: t stride - pad + j
};
inline int cls_down_rph(int taps, int stride) { return CLS_DTM + (taps - 1) / stride + 1; } // LDS rows per residue of the stride
inline size_t cls_down_lds(int taps, int stride) { return (size_t)stride * cls_down_rph(taps, stride) * 33 * 4; }

// The strided convolution: hfg_conv_kernel's implicit GEMM on the f32-input MFMA with the input row index multiplied by the stride. One workgroup: 64 output
// rows x 64 output channels; wave w owns the 32 x 32 tile (row half w & 1, column group w >> 1). The input window ((64 - 1) stride + taps rows) is staged 32
// channels at a time and DE-INTERLEAVED by the residue of the window row modulo the stride (row r at LDS row (r % stride) * rph + r / stride, 33 floats each), so
// the 32 rows of an A fragment, stride apart in the window, are consecutive in LDS: conflict-free as in hfg_conv_kernel. Rows outside the clip read as zero.
__global__ __launch_bounds__(256) void cls_down_kernel(const ClsDown a) {
  extern __shared__ float sx[];
  const int s = blockIdx.y;
  const int fi = a.seq_in[HFG_SEQ * s], Tin = a.seq_in[HFG_SEQ * s + 1], fo = a.seq_out[HFG_SEQ * s], Tout = a.seq_out[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * CLS_DTM;
  if (t0 >= Tout) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int m0 = (wave & 1) * 32, n0 = blockIdx.z * 64 + (wave >> 1) * 32;
  const int F = a.stride, win = (CLS_DTM - 1) * F + a.taps, rph = CLS_DTM + (a.taps - 1) / F + 1;
  const int base = t0 * F - a.pad; // the clip's row under window row 0
  const float *in = a.in + (size_t)fi * a.cin;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  for (int c0 = 0; c0 < a.cin; c0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < win * 8; idx += 256) {
      const int r = idx >> 3, q = (idx & 7) * 4, t = base + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t >= 0 && t < Tin) v = *(const float4 *)(in + (size_t)t * a.cin + c0 + q);
      float *d = sx + ((r % F) * rph + r / F) * 33 + q;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    for (int tap = 0; tap < a.taps; tap++) {
      const float *xr = sx + ((tap % F) * rph + m0 + lr + tap / F) * 33 + lk;
      const float *wr = a.w + (size_t)(tap * a.cin + c0 + lk) * a.cout + n0 + lr;
#pragma unroll 8
      for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[k], wr[(size_t)k * a.cout], acc, 0, 0, 0);
    }
  }
  const int col = n0 + lr;
  const float bv = a.bias[col];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int t = t0 + m0 + 8 * (r >> 2) + 4 * lk + (r & 3);
    if (t < Tout) a.out[((size_t)fo + t) * a.cout + col] = acc[r] + bv;
  }
}

// QKVAttentionLegacy of one (clip, head) in f32: out[t] = softmax_s((q[t] c) . (k[s] c)) v[s], c = DH^-1/4 on q and on k as upstream applies it, no mask, no
// position bias. qkv: rows [row][3 E] = q | k | v, head h at columns h * DH of each (the loader's order). One workgroup = 256 queries; a thread owns one query
// (q and the output row in registers), the keys stream through LDS 4096 / DH at a time, every lane reading the same key element (a broadcast); the softmax is the
// running-maximum form, keys ascending: a query's bits depend on its clip alone.
template <int DH>
__global__ __launch_bounds__(256) void cls_attn_kernel(const float *__restrict__ qkv, const int *__restrict__ seq, int E, float *__restrict__ out) {
  constexpr int KC = 4096 / DH;
  __shared__ float sk[KC * DH], sv[KC * DH];
  const int s = blockIdx.x, h = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  if ((int)blockIdx.z * 256 >= n) return;
  const int qi = blockIdx.z * 256 + threadIdx.x, ld = 3 * E;
  const bool live = qi < n;
  const float c = DH == 64 ? 0.35355339059327379f : 0.29730177875068026f; // DH^-1/4
  float q[DH], acc[DH];
  {
    const float *qp = qkv + ((size_t)f0 + (live ? qi : 0)) * ld + h * DH;
#pragma unroll
    for (int d = 0; d < DH; d++) { q[d] = __fmul_rn(qp[d], c); acc[d] = 0.f; }
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < n; k0 += KC) {
    const int kn = min(KC, n - k0);
    __syncthreads();
    for (int idx = threadIdx.x; idx < kn * DH; idx += 256) {
      const float *kp = qkv + ((size_t)f0 + k0 + idx / DH) * ld + E + h * DH + idx % DH;
      sk[idx] = __fmul_rn(kp[0], c);
      sv[idx] = kp[E];
    }
    __syncthreads();
    for (int j = 0; j < kn; j++) {
      float sc = 0.f;
#pragma unroll
      for (int d = 0; d < DH; d++) sc = __fmaf_rn(q[d], sk[j * DH + d], sc);
      const float mn = fmaxf(m, sc), a = expf(m - mn), p = expf(sc - mn);
      l = __fmaf_rn(l, a, p);
#pragma unroll
      for (int d = 0; d < DH; d++) acc[d] = __fmaf_rn(acc[d], a, __fmul_rn(p, sv[j * DH + d]));
      m = mn;
    }
  }
  if (live) {
    float *op = out + ((size_t)f0 + qi) * E + h * DH;
#pragma unroll
    for (int d = 0; d < DH; d++) op[d] = acc[d] / l;
  }
}

// logits = W h[position 0] + b and the two-class softmax, one wave per clip: lane j adds channels j, j + 64, .. ascending (one fmaf each), then the xor tree.
// out[s] = {logit 0, logit 1, softmax(logits)[0]}
__global__ __launch_bounds__(64) void cls_head_kernel(const float *__restrict__ x, const int *__restrict__ seq, const float *__restrict__ w,
                                                     const float *__restrict__ b, int E, float *__restrict__ out) {
  const int s = blockIdx.x;
  const float *xr = x + (size_t)seq[HFG_SEQ * s] * E;
  float a0 = 0.f, a1 = 0.f;
  for (int c = threadIdx.x; c < E; c += 64) { a0 = __fmaf_rn(w[c], xr[c], a0); a1 = __fmaf_rn(w[E + c], xr[c], a1); }
  for (int d = 32; d; d >>= 1) { a0 += __shfl_xor(a0, d); a1 += __shfl_xor(a1, d); }
  if (threadIdx.x == 0) {
    const float l0 = a0 + b[0], l1 = a1 + b[1], m = fmaxf(l0, l1);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m);
    out[3 * s] = l0; out[3 * s + 1] = l1; out[3 * s + 2] = e0 / (e0 + e1);
  }
}

// ---- the launches, stated once for classifier_run and for the test harness (testlib/cls_harness.hip) ----
void cls_launch_stem(const float *x, const float *w, const float *b, const int *d_seq, int C, int max_n, int B, float *out, hipStream_t st) {
  cls_stem_kernel<<<dim3((unsigned)((max_n + CLS_STEM_ROWS - 1) / CLS_STEM_ROWS), (unsigned)B), 256, 0, st>>>(x, w, b, d_seq, C, out);
}
// part: [tiles of all clips][G] double2; stat: [B][G] double2
void cls_launch_gn_silu(const float *x, float *y, const float *gamma, const float *beta, const int *d_seq, int C, int max_n, int B, double2 *part, double2 *stat,
                        hipStream_t st, int silu = 1) {
  const int G = cls_groups(C);
  const dim3 tiles((unsigned)((max_n + CLS_GN_TILE - 1) / CLS_GN_TILE), (unsigned)B);
  cls_gn_partial_kernel<<<tiles, 256, 0, st>>>(x, d_seq, C, G, part);
  cls_gn_finish_kernel<<<dim3((unsigned)G, (unsigned)B), 64, 0, st>>>(part, d_seq, C, G, 1e-5, stat);
  cls_gn_silu_kernel<<<tiles, 256, 0, st>>>(x, stat, gamma, beta, d_seq, C, G, silu, y);
}
void cls_launch_attn(const float *qkv, float *out, const int *d_seq, int E, int heads, int max_n, int B, hipStream_t st) {
  const dim3 grid((unsigned)B, (unsigned)heads, (unsigned)((max_n + 255) / 256));
  if (E / heads == 64) cls_attn_kernel<64><<<grid, 256, 0, st>>>(qkv, d_seq, E, out);
  else cls_attn_kernel<128><<<grid, 256, 0, st>>>(qkv, d_seq, E, out);
}
void cls_launch_down(const ClsDown &a, int max_out, int B, hipStream_t st) {
  const dim3 grid((unsigned)((max_out + CLS_DTM - 1) / CLS_DTM), (unsigned)B, (unsigned)(a.cout / 64));
  cls_down_kernel<<<grid, 256, cls_down_lds(a.taps, a.stride), st>>>(a);
}
// a C -> C (or the final k = 1) convolution on hfg_conv_kernel, as bigvgan_run launches it; rate 1
void cls_launch_conv(const float *in, float *out, const float *resid, const float *w, const float *bias, const int *d_seq, int cin, int cout, int taps, int max_n,
                     int B, hipStream_t st) {
  HfgConv a{};
  a.in = in; a.out = out; a.resid = resid; a.w = w; a.bias = bias; a.cbias = nullptr; a.seq = d_seq;
  a.cin = cin; a.cout = cout; a.taps = taps; a.dil = 1; a.lo = -(taps - 1) / 2; a.phases = 1; a.pad_t = 0; a.rate = 1; a.slope = 1.0f; a.acc_mode = 0;
  const int nt = cout % 64 == 0 ? 2 : 1;
  const dim3 grid((unsigned)((max_n + HFG_TM - 1) / HFG_TM), (unsigned)B, (unsigned)(cout / (32 * nt)));
  const size_t lds = (size_t)(HFG_TM + taps - 1) * 33 * 4;
  if (nt == 2) hfg_conv_kernel<2><<<grid, 256, lds, st>>>(a);
  else hfg_conv_kernel<1><<<grid, 256, lds, st>>>(a);
}
bool cls_pow2_channels(int c) { return c >= 32 && c <= CLS_MAX_C && (c & (c - 1)) == 0; }
// The tables of classifier_run (and of the test harness): levels 0 .. depth, a Downsample (k 5, stride F, pad 2) between two; every level's records carry
// {first row, rows, 0, first GroupNorm tile, first sample of the clip at 24 kHz}, a clip's first row a multiple of 8
template <class T>
LevelTable cls_levels(const T *n, int B, int depth, int F) {
  return level_table(n, B, depth + 1, [F](int64_t v, int) { return (v - 1) / F + 1; }, 8, CLS_GN_TILE, true);
}
} // namespace

// The model as the loader's host half leaves it (no device call): the configuration from the tensor names and shapes, every tensor repacked for the kernels.
// (w, b of a norm: gamma, beta, here and in ClassifierState)
struct ClsHostRes { HostLayer n1, n2, ca, cb; };
struct ClsHostAttn { HostLayer n, qkv, proj; }; // qkv: [E][3 E] with the output channels in q | k | v order, head h at columns h * dh of each
struct ClsHost {
  int b0 = 0, depth = 0, K = 0, E = 0, rb = 0, n_attn = 0, F = 4, H = 4;
  HostLayer stem, fin, head, fin_n;
  std::vector<ClsHostRes> res; // [depth][rb]
  std::vector<HostLayer> down;
  std::vector<ClsHostAttn> attn;
};

int classifier_parse(tts_ctx *ctx, const WeightFile &wf, const char *path, ClsHost &h) {
  if (!wf.has("classifier.enc.init.weight")) return fail(ctx, TTS_ERR_FORMAT, "'%s' is not a classifier model file", path);
  ModelReader rd{wf, ctx, "classifier"};
  // the configuration: B0 from init.weight; enc.res.{i} is a ResBlock (in_layers / out_layers) or a Downsample (op); E from final.2.weight
  {
    const HostTensor *t = rd.peek("classifier.enc.init.weight", 3);
    if (!t || !cls_pow2_channels((int)t->ne[2])) return fail(ctx, TTS_ERR_FORMAT, "tensor 'classifier.enc.init.weight' has wrong shape in classifier model file (base channels: a power of two, 32 .. 1024)");
    h.b0 = (int)t->ne[2];
  }
  int n_res = 0;
  for (int i = 0;; i++) {
    const std::string p = "classifier.enc.res." + std::to_string(i);
    if (wf.has(p + ".op.weight")) {
      if (h.depth == 0) h.rb = n_res;
      if (n_res != h.rb * (h.depth + 1)) return fail(ctx, TTS_ERR_FORMAT, "classifier model file: level %d has another number of ResBlocks than level 0 (%d)", h.depth, h.rb);
      h.depth++;
    } else if (wf.has(p + ".in_layers.2.weight")) {
      if (n_res == 0) {
        const HostTensor *t = rd.peek(p + ".in_layers.2.weight", 3);
        h.K = t ? (int)t->ne[0] : 0;
      }
      n_res++;
    } else break;
  }
  if (h.depth < 1 || h.depth > CLS_MAX_DEPTH || h.rb < 1 || n_res != h.rb * h.depth)
    return fail(ctx, TTS_ERR_FORMAT, "classifier model file: %d ResBlocks and %d Downsamples under enc.res (the same number of blocks, at least one, before each of 1 .. %d Downsamples)", n_res, h.depth, CLS_MAX_DEPTH);
  if (h.K < 1 || h.K > 11 || h.K % 2 == 0) return fail(ctx, TTS_ERR_FORMAT, "classifier model file: ResBlock kernel size %d (odd, 1 .. 11)", h.K);
  if (!cls_pow2_channels(h.b0 << h.depth)) return fail(ctx, TTS_ERR_FORMAT, "classifier model file: %d channels after %d levels (at most %d)", h.b0 << h.depth, h.depth, CLS_MAX_C);
  {
    const HostTensor *t = rd.peek("classifier.enc.final.2.weight", 3);
    h.E = t ? (int)t->ne[2] : 0;
    if (h.E != 256 && h.E != 512 && h.E != 1024) return fail(ctx, TTS_ERR_FORMAT, "classifier model file: embedding dimension %d (256, 512 or 1024)", h.E);
  }
  while (wf.has("classifier.enc.attn." + std::to_string(h.n_attn) + ".norm.weight")) h.n_attn++;
  if (wf.has("classifier.config")) { // what the shapes cannot give: {downsample factor, attention heads}
    const HostTensor *t = rd.need("classifier.config", 2, 0, 0);
    if (!t) return TTS_ERR_FORMAT;
    h.F = (int)t->data[0]; h.H = (int)t->data[1];
    if ((float)h.F != t->data[0] || (float)h.H != t->data[1] || h.F < 2 || h.F > 6 || h.H < 1)
      return fail(ctx, TTS_ERR_FORMAT, "tensor 'classifier.config' holds downsample factor %g (2 .. 6) and %g heads", (double)t->data[0], (double)t->data[1]);
  }
  if (h.E % h.H || (h.E / h.H != 64 && h.E / h.H != 128))
    return fail(ctx, TTS_ERR_FORMAT, "classifier model file: %d channels in %d heads: the head dimension must be 64 or 128", h.E, h.H);
  int rc;
  if ((rc = rd.raw("classifier.enc.init", h.b0, 1, 3, h.stem))) return rc; // the stem keeps PyTorch's [B0][1][3]
  h.res.resize((size_t)h.depth * h.rb);
  h.down.resize(h.depth);
  for (int l = 0, i = 0; l < h.depth; l++) {
    const int C = h.b0 << l;
    for (int j = 0; j < h.rb; j++, i++) {
      const std::string p = "classifier.enc.res." + std::to_string(i);
      ClsHostRes &r = h.res[(size_t)l * h.rb + j];
      if ((rc = rd.norm(p + ".in_layers.0", C, r.n1)) || (rc = rd.conv(p + ".in_layers.2", C, C, h.K, r.ca)) || (rc = rd.norm(p + ".out_layers.0", C, r.n2)) ||
          (rc = rd.conv(p + ".out_layers.3", C, C, h.K, r.cb)))
        return rc;
    }
    if ((rc = rd.conv("classifier.enc.res." + std::to_string(i++) + ".op", 2 * C, C, 5, h.down[l]))) return rc;
  }
  const int Cf = h.b0 << h.depth;
  if ((rc = rd.norm("classifier.enc.final.0", Cf, h.fin_n)) || (rc = rd.conv("classifier.enc.final.2", h.E, Cf, 1, h.fin))) return rc;
  h.attn.resize(h.n_attn);
  const int E = h.E, dh = E / h.H;
  for (int i = 0; i < h.n_attn; i++) {
    const std::string p = "classifier.enc.attn." + std::to_string(i);
    ClsHostAttn &a = h.attn[i];
    HostLayer q; // both k = 1 convolutions [cout][cin][1] -> hfg_conv_kernel's [cin][cout]
    if ((rc = rd.norm(p + ".norm", E, a.n)) || (rc = rd.conv(p + ".qkv", 3 * E, E, 1, q)) || (rc = rd.conv(p + ".proj_out", E, E, 1, a.proj))) return rc;
    // QKVAttentionLegacy: output channel = head * 3 dh + {q, k, v} * dh + d  ->  the q | k | v blocks cls_attn_kernel reads, head hd at columns hd * dh
    a.qkv.w.resize((size_t)3 * E * E); a.qkv.b.resize((size_t)3 * E);
    for (int hd = 0; hd < h.H; hd++)
      for (int tq = 0; tq < 3; tq++)
        for (int d = 0; d < dh; d++) {
          const int o = hd * 3 * dh + tq * dh + d, n = tq * E + hd * dh + d;
          a.qkv.b[n] = q.b[o];
          for (int ci = 0; ci < E; ci++) a.qkv.w[(size_t)ci * 3 * E + n] = q.w[(size_t)ci * 3 * E + o];
        }
  }
  if ((rc = rd.raw("classifier.head", 2, E, 0, h.head))) return rc;
  return rd.finish(path);
}

struct ClsRes { HfgLayer n1, n2, ca, cb; };
struct ClsAttn { HfgLayer n, qkv, proj; };
struct ClassifierState {
  int b0 = 0, depth = 0, K = 0, E = 0, rb = 0, F = 4, H = 4;
  HfgLayer stem, fin, head, fin_n;
  std::vector<ClsRes> res;
  std::vector<HfgLayer> down;
  std::vector<ClsAttn> attn;
  DevWeights dev;
  DevBuf in, wav, h, a, t, part, stat, x, y, qkv, att, out;
};
void classifier_free(ClassifierState *s) { delete s; }

// The file is parsed before the device is asked for: a host-only context reports a broken file as TTS_ERR_FORMAT and a good one as TTS_ERR_HIP.
int classifier_load(tts_ctx *ctx, const char *path) {
  if (!path) return fail(ctx, TTS_ERR_ARG, "tts_load_classifier: bad argument");
  WeightFile wf;
  std::string err;
  int rc = read_weight_file(path, wf, err);
  if (rc != TTS_OK) return fail(ctx, rc, "classifier_load: %s", err.c_str());
  std::unique_ptr<ClsHost> h(new ClsHost());
  if ((rc = classifier_parse(ctx, wf, path, *h))) return rc;
  if (ctx->device < 0) return fail(ctx, TTS_ERR_HIP, "host-only context: no HIP device, no CPU fallback");
  (void)hipSetDevice(ctx->device);
  std::unique_ptr<ClassifierState> st(new ClassifierState());
  st->b0 = h->b0; st->depth = h->depth; st->K = h->K; st->E = h->E; st->rb = h->rb; st->F = h->F; st->H = h->H;
  auto up = [&](const HostLayer &s, HfgLayer &d) { return st->dev.up(ctx, s, d); };
  if ((rc = up(h->stem, st->stem)) || (rc = up(h->fin, st->fin)) || (rc = up(h->head, st->head)) || (rc = up(h->fin_n, st->fin_n))) return rc;
  st->res.resize(h->res.size()); st->down.resize(h->down.size()); st->attn.resize(h->attn.size());
  for (size_t i = 0; i < h->res.size(); i++)
    if ((rc = up(h->res[i].n1, st->res[i].n1)) || (rc = up(h->res[i].n2, st->res[i].n2)) || (rc = up(h->res[i].ca, st->res[i].ca)) ||
        (rc = up(h->res[i].cb, st->res[i].cb)))
      return rc;
  for (size_t i = 0; i < h->down.size(); i++)
    if ((rc = up(h->down[i], st->down[i]))) return rc;
  for (size_t i = 0; i < h->attn.size(); i++)
    if ((rc = up(h->attn[i].n, st->attn[i].n)) || (rc = up(h->attn[i].qkv, st->attn[i].qkv)) || (rc = up(h->attn[i].proj, st->attn[i].proj))) return rc;
  if (ctx->classifier) classifier_free(ctx->classifier);
  ctx->classifier = st.release();
  return TTS_OK;
}

// One upload (samples, tables), one launch sequence for the whole ragged batch, one download. Nothing of it depends on the batch: a clip's logits are the same
// bits alone or in any batch. The stage owns its buffers and touches no AR or diffusion state, so it is legal while sessions are open.
int classifier_run(tts_ctx *ctx, const float *audio, const int64_t *n_samples, const int32_t *rates, int B, float *prob_out, float *logits_out, ClsResampleFn resample) {
  const char *fn = "tts_classify_audio";
  ClassifierState *st = ctx->classifier;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_classifier not called");
  if (!audio || !n_samples || !rates || !prob_out || !resample || B < 1) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", fn);
  if (B > CLS_MAX_CLIPS) return fail(ctx, TTS_ERR_LIMIT, "%s: %d clips (at most %d per call)", fn, B, CLS_MAX_CLIPS);
  const int depth = st->depth, F = st->F, L = depth + 1;
  ClipIngest clips; // the crop: only TTS_CLS_MAX_SAMPLES of a clip are ever computed
  int rc = clip_ingest(ctx, fn, audio, n_samples, rates, B, 24000, TTS_CLS_MAX_SAMPLES, clips, [](int, int64_t) { return TTS_OK; });
  if (rc) return rc;
  const LevelTable lt = cls_levels(clips.n_dst.data(), B, depth, F);
  const std::vector<int64_t> &rows = lt.rows;
  const std::vector<int> &max_n = lt.max_n;
  const int E = st->E;
  size_t act = 0; // floats of the widest level: level 0 unless the clips are a few samples long
  for (int l = 0; l < L; l++) act = std::max(act, (size_t)rows[l] * (st->b0 << l));
  TTS_HIP(ctx, st->in.reserve(clip_upload_floats(clips, lt) * 4));
  TTS_HIP(ctx, st->wav.reserve((size_t)clips.total_dst * 4));
  TTS_HIP(ctx, st->h.reserve(act * 4));
  TTS_HIP(ctx, st->a.reserve(act * 4));
  TTS_HIP(ctx, st->t.reserve(act * 4));
  TTS_HIP(ctx, st->part.reserve((size_t)lt.tiles[0] * 32 * sizeof(double2)));
  TTS_HIP(ctx, st->stat.reserve((size_t)B * 32 * sizeof(double2)));
  TTS_HIP(ctx, st->x.reserve((size_t)rows[depth] * E * 4));
  TTS_HIP(ctx, st->y.reserve((size_t)rows[depth] * E * 4));
  TTS_HIP(ctx, st->qkv.reserve((size_t)rows[depth] * 3 * E * 4));
  TTS_HIP(ctx, st->att.reserve((size_t)rows[depth] * E * 4));
  TTS_HIP(ctx, st->out.reserve((size_t)B * 3 * 4));
  hipStream_t sm = ctx->stream;
  float *wav = st->wav.as<float>();
  const int *d_tab = nullptr;
  if ((rc = clip_upload(ctx, clips, lt, audio, rates, 24000, st->in, wav, resample, &d_tab))) return rc;
  auto seq = [&](int l) { return d_tab + (size_t)l * B * HFG_SEQ; };
  float *h = st->h.as<float>(), *av = st->a.as<float>(), *t = st->t.as<float>();
  double2 *part = st->part.as<double2>(), *stat = st->stat.as<double2>();
  auto gn = [&](const float *x, const HfgLayer &p, int l, int C) {
    ProfScope ps(ctx, "cls_gn", (double)rows[l] * C * 4 * 3);
    cls_launch_gn_silu(x, av, p.w, p.b, seq(l), C, max_n[l], B, part, stat, sm);
  };
  auto conv = [&](const float *in, float *out, const float *resid, const HfgLayer &w, int l, int cin, int cout, int taps) {
    ProfScope ps(ctx, "cls_conv", 2.0 * (double)rows[l] * taps * cin * cout);
    cls_launch_conv(in, out, resid, w.w, w.b, seq(l), cin, cout, taps, max_n[l], B, sm);
  };
  {
    ProfScope ps(ctx, "cls_conv", 2.0 * (double)rows[0] * 3 * st->b0);
    cls_launch_stem(wav, st->stem.w, st->stem.b, seq(0), st->b0, max_n[0], B, h, sm);
  }
  for (int l = 0; l < depth; l++) {
    const int C = st->b0 << l;
    for (int j = 0; j < st->rb; j++) {
      const ClsRes &r = st->res[(size_t)l * st->rb + j];
      gn(h, r.n1, l, C);
      conv(av, t, nullptr, r.ca, l, C, C, st->K);
      gn(t, r.n2, l, C);
      conv(av, h, h, r.cb, l, C, C, st->K); // the residual add in the epilogue: an element is read and written by the same thread
    }
    ClsDown d{};
    d.in = h; d.out = t; d.w = st->down[l].w; d.bias = st->down[l].b; d.seq_in = seq(l); d.seq_out = seq(l + 1);
    d.cin = C; d.cout = 2 * C; d.taps = 5; d.stride = F; d.pad = 2;
    {
      ProfScope ps(ctx, "cls_conv", 2.0 * (double)rows[l + 1] * 5 * C * 2 * C);
      cls_launch_down(d, max_n[l + 1], B, sm);
    }
    std::swap(h, t);
  }
  const int Cf = st->b0 << depth;
  gn(h, st->fin_n, depth, Cf);
  float *x = st->x.as<float>(), *y = st->y.as<float>(), *qkv = st->qkv.as<float>(), *att = st->att.as<float>();
  conv(av, x, nullptr, st->fin, depth, Cf, E, 1);
  for (const ClsAttn &b : st->attn) { // one profiler entry per block: GroupNorm, the two projections and the attention between them
    ProfScope ps(ctx, "cls_attn", 2.0 * (double)rows[depth] * E * (4.0 * E + 2.0 * max_n[depth]));
    cls_launch_gn_silu(x, y, b.n.w, b.n.b, seq(depth), E, max_n[depth], B, part, stat, sm, 0);
    cls_launch_conv(y, qkv, nullptr, b.qkv.w, b.qkv.b, seq(depth), E, 3 * E, 1, max_n[depth], B, sm);
    cls_launch_attn(qkv, att, seq(depth), E, st->H, max_n[depth], B, sm);
    cls_launch_conv(att, x, x, b.proj.w, b.proj.b, seq(depth), E, E, 1, max_n[depth], B, sm);
  }
  {
    ProfScope ps(ctx, "cls_attn", 2.0 * (double)B * 2 * E);
    cls_head_kernel<<<B, 64, 0, sm>>>(x, seq(depth), st->head.w, st->head.b, E, st->out.as<float>());
  }
  TTS_HIP(ctx, hipGetLastError());
  std::vector<float> res((size_t)B * 3);
  TTS_HIP(ctx, hipMemcpyAsync(res.data(), st->out.p, res.size() * 4, hipMemcpyDeviceToHost, sm));
  TTS_HIP(ctx, hipStreamSynchronize(sm));
  for (int s = 0; s < B; s++) {
    prob_out[s] = res[(size_t)3 * s + 2];
    if (logits_out) { logits_out[2 * s] = res[(size_t)3 * s]; logits_out[2 * s + 1] = res[(size_t)3 * s + 1]; }
  }
  return TTS_OK;
}

} // namespace tts
#include "aligner.h" // the wav2vec2 CTC aligner: the same translation unit, the classifier's strided convolution and attention
