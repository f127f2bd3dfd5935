// The attention of the classifier and of the wav2vec2 aligner on the fp16 MFMA (option "addon_attn_precision" 1 and 2): addon_attn_h_kernel<DH, SPLIT>.
//
// Included once, at the top of classifier.h (hifigan.hip's translation unit: HFG_SEQ, f32x16, hfg_conv_h.h's HFG_H_MAX, HFG_H_NOPK and vector types);
// cls_launch_attn_h (classifier.h) launches it. It computes what cls_attn_kernel<DH> computes, by that kernel's rule: non-causal, unmasked, bias-free attention of
// one (clip, head), out[t] = softmax_s((q[t] c) . (k[s] c)) v[s] with c = DH^-1/4 multiplied into q and into k in f32 (__fmul_rn) BEFORE any rounding to fp16;
// qkv f32 rows [row][3 E] = q | k | v, head h at columns h * DH; out f32 [row][E]; clips by the HFG_SEQ table.
//
// Operands, made on the fly from the f32 buffer as the Linears of w2v_linear_h.h make theirs: v clamped to +-65504, hi = rn_f16(v), lo = rn_f16(v - hi).
// SPLIT = false (mode 1) multiplies hi hi only; SPLIT = true (mode 2) lo hi, hi lo, then hi hi (the small terms first) for Q K^T, and the same three for P V,
// with P split after the exponential and V split at staging. Both products run on v_mfma_f32_32x32x16_f16 with f32 accumulators.
// Subnormals: P is multiplied by 2^14 (exact) before it is rounded, so neither half of a weight above 2^-28 of the row's running maximum is an fp16 subnormal,
// and the output is multiplied by 2^-14 (exact) before the division. The low halves of q, k and v are NOT rescaled: that they reach the matrix pipe unflushed is
// what the "small" family of tests/test_addon_attn_kernels_gpu.py proves (operands of 2^-10, whose low halves are all subnormal, against a float64 reference
// that keeps them, under the accumulation bound alone).
//
// Work split. One workgroup: at most 64 queries of one (clip, head) on 4 waves; a 459-frame clip at 16 heads is 8 x 16 = 128 workgroups. Wave w owns the 32
// queries of query half w & 1 and, of every tile of 64 keys, the 32 keys of key half w >> 1. K and V tiles are staged ONCE per workgroup as fp16 planes,
// converted (K scaled by c) on the way: K as [key][DH + 8], V TRANSPOSED as [d][64 + 4] (a thread loads a 4 key x 4 channel block and stores four 8-byte rows),
// in a ring of two slots: a thread loads its share of tile t + 1 from global memory before the MFMAs of tile t and converts and stores it behind them, so one
// barrier per tile is enough (the slot written in iteration t was last read in iteration t - 1, which every wave has left). Q lives in registers, loaded from
// global memory once in B-operand shape.
// A wave computes S^T (keys x queries): A = K rows from LDS, B = Q. In the 32 x 32 accumulator the lane (query = lane & 31, half = lane >> 5) then holds 16
// scores OF ONE QUERY (keys 8 (r >> 2) + 4 half + (r & 3)): the tile's maximum and sum are a register reduction plus one exchange with lane ^ 32, and the
// exponentiated registers 8 j .. 8 j + 7 ARE the B operand of K step j of O^T = V^T P^T, with the MFMA's k index 8 half + i standing for key
// 16 j + 8 (i >> 2) + 4 half + (i & 3). The A operand (V^T, row d) is read from LDS under that same permutation: two 8-byte reads of 4 consecutive keys. P never
// goes through LDS. The softmax is the running-maximum form in f32, key tiles ascending. After the last tile the waves of key half 1 leave (m, l, O) in LDS and
// the waves of key half 0 merge: m = max(m0, m1), l = l0 e^(m0 - m) + l1 e^(m1 - m), O likewise, always in that order.
// No atomics, no split over workgroups: the order of every sum depends on the clip's own length alone, so a clip's bits are the same alone or in any batch and
// two runs agree. A key behind the clip's end gets the score -inf before the maximum and its row is never read (zeros in LDS); a wave whose 32 keys all lie
// behind the end skips the tile; a query behind the end is neither read nor stored.
// LDS: 2 slots x planes x (64 (DH + 8) + DH 68) halves: 35 KB (DH 64) .. 136 KB (DH 128, SPLIT) of gfx950's 160 KB, dynamic. Registers (profiles/addon_attn.txt):
// no scratch, no spills at either DH.
#pragma once

namespace tts {
namespace {

constexpr int AAH_TQ = 64, AAH_TK = 64; // queries of a workgroup, keys of a staged tile
constexpr int AAH_LDV = AAH_TK + 4;     // halves of a row of the transposed V plane
constexpr float AAH_PSCALE = 16384.f, AAH_PUNSCALE = 1.0f / 16384.f; // 2^14 on P, 2^-14 on O
template <int DH, bool SPLIT>
constexpr size_t aah_lds_bytes() { return (size_t)2 * (SPLIT ? 2 : 1) * (AAH_TK * (DH + 8) + DH * AAH_LDV) * sizeof(_Float16); }

__device__ __forceinline__ void aah_pair(float v, _Float16 &hi, _Float16 &lo) {
  v = fminf(fmaxf(v, -HFG_H_MAX), HFG_H_MAX);
  hi = (_Float16)v;
  lo = (_Float16)__fsub_rn(v, (float)hi);
}

template <int DH, bool SPLIT>
__global__ HFG_H_NOPK __launch_bounds__(256) void addon_attn_h_kernel(const float *__restrict__ qkv, const int *__restrict__ seq, int E, float *__restrict__ out) {
  extern __shared__ __align__(16) _Float16 aah_lds[];
  constexpr int NP = SPLIT ? 2 : 1, LDK = DH + 8, LDV = AAH_LDV;
  constexpr int KPL = AAH_TK * LDK, VPL = DH * LDV, SLOT = NP * (KPL + VPL); // halves: slot = K planes | V planes
  constexpr int QD = DH / 4, RP = 256 / QD;                                  // float4 of a row; rows of a staging pass
  constexpr int NK = AAH_TK / RP, NV = AAH_TK / 4 / RP;                      // a thread's float4 of K and 4 x 4 blocks of V per tile
  constexpr int KS = DH / 16, DB = DH / 32;
  static_assert((size_t)(DH + 4) * 64 * sizeof(float) <= aah_lds_bytes<DH, SPLIT>(), "the merge area lies inside the ring");
  const int s = blockIdx.z, h = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  const int q0 = blockIdx.x * AAH_TQ;
  if (q0 >= n) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int qh = wave & 1, kh = wave >> 1;
  const size_t ld = (size_t)3 * E;
  const float c = DH == 64 ? 0.35355339059327379f : 0.29730177875068026f; // DH^-1/4
  const float *base = qkv + (size_t)f0 * ld + h * DH;
  const int qrow = q0 + qh * 32 + lr;
  const bool qlive = qrow < n, live = q0 + qh * 32 < n; // a wave whose 32 queries all lie behind the clip stages its share and multiplies nothing
  const int sr = threadIdx.x / QD, sq = (threadIdx.x % QD) * 4;

  hfg_h8 qhi[KS], qlo[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ks++) {
    hfg_f4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
    if (qlive) {
      const float *qp = base + (size_t)qrow * ld + ks * 16 + lk * 8;
      a = *(const hfg_f4 *)qp;
      b = *(const hfg_f4 *)(qp + 4);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      _Float16 hi, lo;
      aah_pair(__fmul_rn(a[i], c), hi, lo); qhi[ks][i] = hi; qlo[ks][i] = lo;
      aah_pair(__fmul_rn(b[i], c), hi, lo); qhi[ks][4 + i] = hi; qlo[ks][4 + i] = lo;
    }
  }

  hfg_f4 kx[NK], vx[NV][4];
  // a thread's share of the tile at key k0: K rows sr + RP j, channels sq .. sq + 3; V keys 4 (sr + RP j) .. + 3, the same channels; a row behind the clip is not read
  auto gload = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NK; j++) {
      const int r = k0 + sr + RP * j;
      kx[j] = hfg_f4{0.f, 0.f, 0.f, 0.f};
      if (r < n) kx[j] = *(const hfg_f4 *)(base + (size_t)r * ld + E + sq);
    }
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int r = k0 + 4 * (sr + RP * j) + i;
        vx[j][i] = hfg_f4{0.f, 0.f, 0.f, 0.f};
        if (r < n) vx[j][i] = *(const hfg_f4 *)(base + (size_t)r * ld + 2 * E + sq);
      }
  };
  auto store = [&](int slot) __attribute__((always_inline)) {
    _Float16 *kp = aah_lds + slot * SLOT, *vp = kp + NP * KPL;
#pragma unroll
    for (int j = 0; j < NK; j++) {
      hfg_h4 hi, lo;
#pragma unroll
      for (int i = 0; i < 4; i++) { _Float16 a, b; aah_pair(__fmul_rn(kx[j][i], c), a, b); hi[i] = a; lo[i] = b; }
      const int o = (sr + RP * j) * LDK + sq;
      *(hfg_h4 *)(kp + o) = hi;
      if (SPLIT) *(hfg_h4 *)(kp + KPL + o) = lo;
    }
#pragma unroll
    for (int j = 0; j < NV; j++)
#pragma unroll
      for (int d = 0; d < 4; d++) { // channel sq + d: the 4 keys of the block side by side
        hfg_h4 hi, lo;
#pragma unroll
        for (int i = 0; i < 4; i++) { _Float16 a, b; aah_pair(vx[j][i][d], a, b); hi[i] = a; lo[i] = b; }
        const int o = (sq + d) * LDV + 4 * (sr + RP * j);
        *(hfg_h4 *)(vp + o) = hi;
        if (SPLIT) *(hfg_h4 *)(vp + VPL + o) = lo;
      }
  };

  f32x16 o[DB];
#pragma unroll
  for (int b = 0; b < DB; b++)
#pragma unroll
    for (int r = 0; r < 16; r++) o[b][r] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int tiles = (n + AAH_TK - 1) / AAH_TK;
  gload(0);
  store(0);
  __syncthreads();
  for (int t = 0; t < tiles; t++) {
    const bool more = t + 1 < tiles;
    if (more) gload((t + 1) * AAH_TK); // in flight under this tile's MFMAs
    const int kw = t * AAH_TK + kh * 32; // the wave's first key of the tile
    if (live && kw < n) {
      const _Float16 *kp = aah_lds + (t & 1) * SLOT + (kh * 32 + lr) * LDK + lk * 8;
      const _Float16 *vp = aah_lds + (t & 1) * SLOT + NP * KPL + lr * LDV + kh * 32 + 4 * lk;
      f32x16 sc;
#pragma unroll
      for (int r = 0; r < 16; r++) sc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        const hfg_h8 a = *(const hfg_h8 *)(kp + ks * 16);
        if (SPLIT) {
          const hfg_h8 al = *(const hfg_h8 *)(kp + KPL + ks * 16);
          sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, qhi[ks], sc, 0, 0, 0);
          sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qlo[ks], sc, 0, 0, 0);
        }
        sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qhi[ks], sc, 0, 0, 0);
      }
      if (kw + 32 > n) { // the clip ends inside the wave's keys
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (kw + 8 * (r >> 2) + 4 * lk + (r & 3) >= n) sc[r] = -INFINITY;
      }
      float tm = sc[0];
#pragma unroll
      for (int r = 1; r < 16; r++) tm = fmaxf(tm, sc[r]);
      tm = fmaxf(tm, __shfl_xor(tm, 32));
      const float mn = fmaxf(m, tm), alpha = expf(m - mn); // the wave's key 0 of the tile is live: mn is finite
      float ts = 0.f;
#pragma unroll
      for (int r = 0; r < 16; r++) { sc[r] = expf(sc[r] - mn); ts += sc[r]; }
      ts += __shfl_xor(ts, 32);
      l = __fmaf_rn(l, alpha, ts);
      m = mn;
#pragma unroll
      for (int b = 0; b < DB; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[b][r] *= alpha;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        hfg_h8 ph, pl;
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const float ps = __fmul_rn(sc[8 * j + i], AAH_PSCALE);
          ph[i] = (_Float16)ps;
          pl[i] = (_Float16)__fsub_rn(ps, (float)ph[i]);
        }
#pragma unroll
        for (int b = 0; b < DB; b++) {
          const _Float16 *vr = vp + b * 32 * LDV + 16 * j;
          const hfg_h4 v0 = *(const hfg_h4 *)vr, v1 = *(const hfg_h4 *)(vr + 8);
          const hfg_h8 vh = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
          if (SPLIT) {
            const hfg_h4 w0 = *(const hfg_h4 *)(vr + VPL), w1 = *(const hfg_h4 *)(vr + VPL + 8);
            const hfg_h8 vl = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
            o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o[b], 0, 0, 0);
            o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, o[b], 0, 0, 0);
          }
          o[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o[b], 0, 0, 0);
        }
      }
    }
    if (more) {
      store((t + 1) & 1);
      __syncthreads();
    }
  }

  // the merge of the two key halves, through the ring's memory: [query half][register | m | l][lane]
  __syncthreads();
  float *mg = (float *)aah_lds + (size_t)qh * (DH / 2 + 2) * 64 + lane;
  if (kh == 1) {
#pragma unroll
    for (int b = 0; b < DB; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) mg[(b * 16 + r) * 64] = o[b][r];
    mg[(DH / 2) * 64] = m;
    mg[(DH / 2 + 1) * 64] = l;
  }
  __syncthreads();
  if (kh == 1 || !qlive) return;
  const float m1 = mg[(DH / 2) * 64], l1 = mg[(DH / 2 + 1) * 64];
  const float mm = fmaxf(m, m1), a0 = expf(m - mm), a1 = expf(m1 - mm); // m is finite (key 0 is this half's); an idle half 1 left m1 = -inf, l1 = 0, O = 0
  const float lt = __fmaf_rn(l1, a1, __fmul_rn(l, a0));
  float *op = out + ((size_t)f0 + qrow) * E + h * DH + 4 * lk;
#pragma unroll
  for (int b = 0; b < DB; b++)
#pragma unroll
    for (int g = 0; g < 4; g++) { // registers 4 g .. 4 g + 3: channels 32 b + 8 g + 4 lk .. + 3
      hfg_f4 v;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int r = 4 * g + i;
        v[i] = __fmul_rn(__fmaf_rn(mg[(b * 16 + r) * 64], a1, __fmul_rn(o[b][r], a0)), AAH_PUNSCALE) / lt;
      }
      *(hfg_f4 *)(op + b * 32 + 8 * g) = v;
    }
}

// One launch for the whole ragged batch; grid: query tiles of the longest clip x heads x clips
template <int DH, bool SPLIT>
inline void addon_attn_h_go(const float *qkv, float *out, const int *d_seq, int E, int heads, int max_n, int B, hipStream_t st) {
  constexpr size_t lds = aah_lds_bytes<DH, SPLIT>();
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)addon_attn_h_kernel<DH, SPLIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const dim3 grid((unsigned)((max_n + AAH_TQ - 1) / AAH_TQ), (unsigned)heads, (unsigned)B);
  addon_attn_h_kernel<DH, SPLIT><<<grid, 256, lds, st>>>(qkv, d_seq, E, out);
}

} // namespace
} // namespace tts
