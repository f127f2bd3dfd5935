// Teacher-forced scores under the AR head (included by ar.hip): for every row r of hn [R][K] (the latent pass's output behind ln_f and lm_head.0's LayerNorm)
// and a target id tgt[r]
//   logit[r][v] = b[v] + hn[r] . W[:, v], v < N       in accumulators only: the [R][N] matrix (263 MB at 16 candidates x 501 rows) is never written
//   lse[r] = log sum_v exp(logit[r][v]),  logit[r][tgt[r]],  logit[r][N - 1] (the stop token),  argmax_v logit[r][v] (the lowest index on a tie)
// ar_score_kernel: one workgroup = 64 rows x one slab of 256 columns; ar_score_reduce_kernel merges the slabs of a row in ascending order. No atomics: a row's
// bits depend on that row of hn, its target and the head alone (not on R, the row's place in the batch or its neighbours). The weights are the loader's unfolded
// f32 head as it lies (ArState::lm_w, strip-major [NPAD / 64][K][64], and lm_b [NPAD]); the columns N .. NPAD - 1 are padding and never enter the sum, the
// maximum or the argmax, whatever they hold. dvae_vq_kernel (dvae.h) is the same shape of problem and the same operand maps.
#pragma once
#include <climits>

namespace tts {

namespace {
constexpr int ARS_TM = 64;     // rows of a workgroup: two 32-row MFMA tiles per wave share every weight fragment
constexpr int ARS_SLAB = 256;  // columns of a workgroup: 8 tiles of 32, tiles w and w + 4 on wave w
constexpr int ARS_KC = 512;    // channels staged in LDS at once (64 rows x 513 floats = 131 KB): K = 1024 goes through in two halves into the same accumulators
constexpr int ARS_MAX_K = 4096;
using ars_f32x16 = __attribute__((ext_vector_type(16))) float;

struct ArScore {
  const float *hn;  // [R][K]
  const float *w;   // strip-major [NPAD / 64][K][64]: W[k][v] at ((v / 64) K + k) 64 + v % 64
  const float *b;   // [NPAD]
  const int *tgt;   // [R], 0 <= tgt[r] < N
  float *ws;        // ar_score_ws_floats(R, N) floats: pm | ps | pi [slabs][R] (a row's maximum, sum exp(l - max) and argmax over a slab), tl | sl [R]
  int R, K, N, NPAD;
};
struct ArScoreOut { // each [R]
  float *lse, *logp /* logit[tgt] - lse */, *stop_logp /* logit[N - 1] - lse */;
  int *greedy;
  float *tgt_logit, *stop_logit; // null or [R]: the two logits themselves (the test harness)
};
inline int ar_score_slabs(int N) { return (N + ARS_SLAB - 1) / ARS_SLAB; }
inline size_t ar_score_ws_floats(int R, int N) { return ((size_t)3 * ar_score_slabs(N) + 2) * R; }
inline int ar_score_kc(int K) { return K < ARS_KC ? K : ARS_KC; }
inline size_t ar_score_lds(int K) { return ((size_t)ARS_TM * (ar_score_kc(K) + 1) + (size_t)3 * 4 * ARS_TM + ARS_TM) * 4; }
// the shapes the kernel tiles: whole 32-channel MFMA steps, whole staged halves, whole 64-column strips that hold every valid column
inline bool ar_score_shape_ok(int R, int K, int N, int NPAD) {
  return R >= 1 && K >= 32 && K % 32 == 0 && K <= ARS_MAX_K && (K <= ARS_KC || K % ARS_KC == 0) && N >= 1 && NPAD >= N && NPAD % 64 == 0 &&
         (int64_t)R * K < ((int64_t)1 << 31);
}

// Per output element one fmaf per channel from 0, channels ascending (the f32-input MFMA: bitwise an fmaf chain), then + b[v]. A lane holds column j0 + (lane & 31)
// of its wave's two tiles for 32 rows; per row: the maximum and its index over the lane's two columns (the lower tile first, a strict ">": the lower index stays),
// the xor tree over the 32 columns of a lane half on (value, index) pairs, sum exp(l - wave maximum) over the same tree (every lane adds the same pairs: one
// result), the four waves through LDS (ascending, rescaled to the workgroup's maximum), one (max, sum, argmax) per row and slab to the workspace. The lane that
// holds a row's target column, and the one that holds column N - 1, store that logit. Rows past R are staged as zeros and never written; a wave whose tiles lie
// past N (the tail slab) contributes (-inf, 0, INT_MAX).
__global__ __launch_bounds__(256) void ar_score_kernel(const ArScore a) {
  extern __shared__ float sx[];
  const int r0 = blockIdx.x * ARS_TM, c0 = blockIdx.y * ARS_SLAB;
  const int kc = min(a.K, ARS_KC), ld = kc + 1, rows = min(ARS_TM, a.R - r0), qpr = kc / 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  float *rm = sx + ARS_TM * ld, *rs = rm + 4 * ARS_TM; // [wave][row] behind the staged rows
  int *ri = (int *)(rs + 4 * ARS_TM), *stgt = ri + 4 * ARS_TM;
  if (threadIdx.x < ARS_TM) stgt[threadIdx.x] = (int)threadIdx.x < rows ? a.tgt[r0 + threadIdx.x] : -1;
  ars_f32x16 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[t][m][r] = 0.f;
  const int j0[2] = {c0 + wave * 32, c0 + wave * 32 + ARS_SLAB / 2};
  for (int kb = 0; kb < a.K; kb += kc) {
    if (kb) __syncthreads(); // every wave has read the half before
    for (int idx = threadIdx.x; idx < ARS_TM * qpr; idx += 256) {
      const int r = idx / qpr, q = (idx % qpr) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) v = *(const float4 *)(a.hn + ((size_t)r0 + r) * a.K + kb + q);
      float *d = sx + r * ld + q;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    const float *xr = sx + lr * ld + lk;
#pragma unroll
    for (int t = 0; t < 2; t++) {
      if (j0[t] >= a.N) continue; // wave-uniform; a tile that holds a valid column lies below NPAD whole (NPAD a multiple of 64)
      const float *wr = a.w + ((size_t)(j0[t] >> 6) * a.K + kb + lk) * 64 + (j0[t] & 63) + lr;
      for (int k0 = 0; k0 < kc; k0 += 32)
#pragma unroll 8
        for (int k = k0; k < k0 + 32; k += 2) { // lane half lk holds channel kb + k + lk of both operands
          const float b = wr[(size_t)k * 64];
          acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[k], b, acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[32 * ld + k], b, acc[t][1], 0, 0, 0);
        }
    }
  }
  const int col0 = j0[0] + lr, col1 = j0[1] + lr;
  const bool ok0 = col0 < a.N, ok1 = col1 < a.N;
  const float b0 = ok0 ? a.b[col0] : 0.f, b1 = ok1 ? a.b[col1] : 0.f;
  float *tl = a.ws + (size_t)3 * gridDim.y * a.R, *sl = tl + a.R;
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = m * 32 + 8 * (r >> 2) + 4 * lk + (r & 3); // the C/D map keeps the row on (register, lane half)
      const float l0 = ok0 ? acc[0][m][r] + b0 : -INFINITY, l1 = ok1 ? acc[1][m][r] + b1 : -INFINITY;
      float v = l0;
      int i = ok0 ? col0 : INT_MAX;
      if (l1 > v) { v = l1; i = col1; }
#pragma unroll
      for (int d = 16; d; d >>= 1) {
        const float ov = __shfl_xor(v, d);
        const int oi = __shfl_xor(i, d);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
      }
      float e = 0.f;
      if (j0[0] < a.N) { // the wave holds a valid column: v is finite
        e = (ok0 ? expf(l0 - v) : 0.f) + (ok1 ? expf(l1 - v) : 0.f);
#pragma unroll
        for (int d = 16; d; d >>= 1) e += __shfl_xor(e, d);
      }
      if (row < rows) {
        const int t = stgt[row];
        if (ok0 && col0 == t) tl[r0 + row] = l0;
        if (ok1 && col1 == t) tl[r0 + row] = l1;
        if (col0 == a.N - 1) sl[r0 + row] = l0;
        if (col1 == a.N - 1) sl[r0 + row] = l1;
      }
      if (lr == 0) { rm[wave * ARS_TM + row] = v; rs[wave * ARS_TM + row] = e; ri[wave * ARS_TM + row] = i; }
    }
  __syncthreads();
  if ((int)threadIdx.x < rows) {
    float M = rm[threadIdx.x]; // wave 0 always holds a valid column
    int I = ri[threadIdx.x];
    for (int w = 1; w < 4; w++) {
      const float ov = rm[w * ARS_TM + threadIdx.x];
      const int oi = ri[w * ARS_TM + threadIdx.x];
      if (ov > M || (ov == M && oi < I)) { M = ov; I = oi; }
    }
    float S = 0.f;
    for (int w = 0; w < 4; w++) {
      const float mw = rm[w * ARS_TM + threadIdx.x];
      if (mw > -INFINITY) S += rs[w * ARS_TM + threadIdx.x] * expf(mw - M);
    }
    const size_t o = (size_t)blockIdx.y * a.R + r0 + threadIdx.x, n = (size_t)gridDim.y * a.R;
    a.ws[o] = M; a.ws[n + o] = S; ((int *)a.ws)[2 * n + o] = I;
  }
}

// A row's slabs in ascending order: M = max m_s (the lowest index on a tie), S = sum s_s exp(m_s - M), lse = M + log S.
__global__ __launch_bounds__(256) void ar_score_reduce_kernel(const float *__restrict__ ws, int R, int slabs, int N, const ArScoreOut o) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const size_t n = (size_t)slabs * R;
  const float *pm = ws, *ps = ws + n, *tl = ws + 3 * n, *sl = tl + R;
  const int *pi = (const int *)(ws + 2 * n);
  float M = pm[r];
  int I = pi[r];
  for (int s = 1; s < slabs; s++) {
    const float ov = pm[(size_t)s * R + r];
    const int oi = pi[(size_t)s * R + r];
    if (ov > M || (ov == M && oi < I)) { M = ov; I = oi; }
  }
  float S = 0.f;
  for (int s = 0; s < slabs; s++) S += ps[(size_t)s * R + r] * expf(pm[(size_t)s * R + r] - M);
  const float lse = M + logf(S);
  o.lse[r] = lse;
  o.logp[r] = tl[r] - lse;
  o.stop_logp[r] = sl[r] - lse;
  o.greedy[r] = I >= 0 && I < N ? I : 0;
  if (o.tgt_logit) o.tgt_logit[r] = tl[r];
  if (o.stop_logit) o.stop_logit[r] = sl[r];
}

// The one launch site, for ar_score_rows and for the test harness (testlib/ar_score_harness.hip). The caller has checked ar_score_shape_ok and the targets.
hipError_t ar_score_launch(const ArScore &a, const ArScoreOut &o, hipStream_t st) {
  static bool raised = false; // more than 64 KB of dynamic LDS
  if (!raised) {
    const hipError_t e = hipFuncSetAttribute((const void *)ar_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ar_score_lds(ARS_KC));
    if (e != hipSuccess) return e;
    raised = true;
  }
  const int slabs = ar_score_slabs(a.N);
  ar_score_kernel<<<dim3((unsigned)((a.R + ARS_TM - 1) / ARS_TM), (unsigned)slabs), 256, ar_score_lds(a.K), st>>>(a);
  ar_score_reduce_kernel<<<(unsigned)((a.R + 255) / 256), 256, 0, st>>>(a.ws, a.R, slabs, a.N, o);
  return hipGetLastError();
}

} // namespace
} // namespace tts
