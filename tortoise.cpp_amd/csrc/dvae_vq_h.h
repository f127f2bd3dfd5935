// The DVAE quantiser on the fp16 MFMA (option "dvae_precision" 1 and 2): dvae_vq_h_kernel<SPLIT>.
//
// Included once, in dvae.h right behind dvae_vq_kernel, whose contract it keeps (hifigan.hip's translation unit: f32x16, hfg_conv_h.h's HFG_H_MAX, HFG_H_NOPK,
// vector types and weight packer; DVQ_TM, DVQ_SLAB and dvae_vq_reduce_kernel are dvae.h's). dvae_launch_vq_h (below) launches it.
//   code[t] = argmin_j d_j,  d_j = fmaf(-2 / s_j, acc_j, |E_j|^2),  acc_j = sum_k (E_kj s_j) z_k on v_mfma_f32_32x32x16_f16,  the lowest index on a tie
// dvae_vq_kernel multiplies on v_mfma_f32_32x32x2_f32, 1/16 of the fp16 MFMA rate. The operands here are hfg_conv_h_kernel's:
//   SPLIT = false (mode 1)  z clamped to +-65504 and E s rounded to fp16, one MFMA per K step of 16, f32 accumulation
//   SPLIT = true  (mode 2)  z = zh + zl and E s = eh + el, each half an fp16 number; eh zl, el zh, then eh zh per K step (the small terms first, el zl dropped)
// The codebook planes are hfg_pack_launch's with pt = 1 on the tensor [dim][tokens] as it lies: [dim / 16][tokens / 32][lane][8] and one power-of-two scale s_j
// per code (its largest |E_kj s_j| in [2^12, 2^13)). That order serves either MFMA operand: lane l holds the 8 channels 16 ks + 8 (l / 32) .. + 7 of code
// 32 ct + l % 32. |E_j|^2 is dvae_code_norms' (double over the f32 codebook, rounded once); -2 / s_j is a power of two, so d_j rounds once.
//
// Work split. One workgroup of 4 waves: 64 rows of z x `spw` consecutive slabs of 256 codes, one (minimum, index) per row and SLAB written, so
// dvae_vq_reduce_kernel merges the slabs as it does for dvae_vq_kernel and the bits do not depend on spw (the launcher picks it so that a large batch stages a z
// tile once per 2 .. 8 slabs and a single clip still fills the chip).
// THE CODEBOOK IS THE A OPERAND AND z THE B OPERAND: an accumulator block is [32 codes][32 rows], and the C/D map puts a block's column - a row of z - on the lane
// (l % 32) and 16 of its 32 codes in the lane's registers. The running minimum of a row is therefore two scalars per lane and accumulator, updated register by
// register in ascending code order with a strict "<" (the earlier, lower index stays: "strictly smaller, or equal and lower index" in that order); the only
// cross-lane step is between the two lanes l and l ^ 32 that share a row (one ds_bpermute pair), then the four waves through LDS in wave order, every merge by
// (value, index). dvae_vq_kernel, with z as the A operand, keeps 32 running pairs per lane and runs a five-step xor tree over each.
// Staging. The z tile (64 x D, rows past R as zeros) is clamped and converted ONCE per workgroup into fp16 planes [row][D + 8] in LDS (66.5 KB a plane at D = 512;
// the 8 halves of padding put the 16-byte fragment reads of 8 consecutive rows on the 32 banks once) and held for all its slabs; there is no barrier in the K loop.
// A wave owns the code tiles w and w + 4 of a slab and both 32-row halves: four accumulators, so every codebook fragment (global memory -> registers, one K step
// ahead of the MFMAs, no LDS) is used twice and every z fragment (LDS -> registers) twice: per K step 2 (4) 16-byte global loads and 2 (4) LDS reads feed 4 (12) MFMAs.
// Order per distance: K steps ascending, the (up to three) MFMAs of a step; no split-K, no atomics: a row's result depends on that row alone, so a clip alone
// equals the clip in a batch and two runs agree. A NaN distance never wins; a row whose every distance is NaN gets code 0 (dvae_vq_reduce_kernel).
// D a multiple of 32 up to DVAE_MAX_DIM, N a multiple of 32 (dvae_parse); a slab's tail of fewer than 8 tiles is walked by the waves that own a tile of it.
#pragma once

namespace tts {
namespace {

struct DvaeVqH {
  const float *z;          // [R][D]
  const _Float16 *eh, *el; // the codebook planes [D / 16][N / 32][64][8]: hi, lo (hfg_pack_launch, pt = 1)
  const float *es;         // [N]: 1 / s_j
  const float *e2;         // [N]: |E_j|^2 (dvae_code_norms)
  float *pv;               // [slabs][R]
  int *pi;                 // [slabs][R]
  int R, D, N, spw;        // spw: slabs of a workgroup
};
// dynamic LDS: the planes of the z tile and, behind them, two slots of [wave][row] (value, index) for the merge over the waves
inline size_t dvae_vq_h_lds(bool split, int D) { return (size_t)(split ? 2 : 1) * DVQ_TM * (D + 8) * sizeof(_Float16) + (size_t)2 * 4 * DVQ_TM * 8; }

#define DVQH_SYNC()                                       \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
    __builtin_amdgcn_s_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); \
  } while (0)
// the wave's codebook fragments of K step ks_: tiles ct0 and ct1, one 16-byte load per lane, tile and plane
#define DVQH_ELOAD(ks_, h0_, l0_, h1_, l1_)                                                                                     \
  do {                                                                                                                          \
    const size_t o_ = (size_t)(ks_) * ctn * 512 + lane * 8;                                                                     \
    h0_ = *(const hfg_h8 *)(a.eh + o_ + (size_t)ct0 * 512);                                                                     \
    h1_ = *(const hfg_h8 *)(a.eh + o_ + (size_t)ct1 * 512);                                                                     \
    if (SPLIT) {                                                                                                                \
      l0_ = *(const hfg_h8 *)(a.el + o_ + (size_t)ct0 * 512);                                                                   \
      l1_ = *(const hfg_h8 *)(a.el + o_ + (size_t)ct1 * 512);                                                                   \
    }                                                                                                                           \
  } while (0)
// the distances of one accumulator block (tile ct_, row half m_) into the lane's running minimum: registers ascending = codes ascending
#define DVQH_MIN(acc_, ct_, m_)                                                                                                 \
  _Pragma("unroll") for (int g = 0; g < 4; g++) {                                                                               \
    const int j_ = (ct_) * 32 + 8 * g + 4 * lk; /* C/D map of the 32 x 32 MFMA: block row 8 (r >> 2) + 4 lk + (r & 3) */        \
    const hfg_f4 s_ = *(const hfg_f4 *)(a.es + j_), n_ = *(const hfg_f4 *)(a.e2 + j_);                                          \
    _Pragma("unroll") for (int i = 0; i < 4; i++) {                                                                             \
      const float d_ = __builtin_fmaf(__fmul_rn(-2.0f, s_[i]), acc_[4 * g + i], n_[i]);                                         \
      if (d_ < best[m_]) { best[m_] = d_; bi[m_] = j_ + i; }                                                                    \
    }                                                                                                                           \
  }

template <bool SPLIT>
__global__ HFG_H_NOPK __launch_bounds__(256) void dvae_vq_h_kernel(const DvaeVqH a) {
  extern __shared__ __align__(16) _Float16 dvqh_lds[];
  const int r0 = blockIdx.x * DVQ_TM, rows = min(DVQ_TM, a.R - r0);
  const int LD = a.D + 8, plane = DVQ_TM * LD, qpr = a.D / 4;
  for (int idx = threadIdx.x; idx < DVQ_TM * qpr; idx += 256) { // the z tile, once: rows past R are zeros and are never written
    const int r = idx / qpr, q = (idx - r * qpr) * 4;
    hfg_f4 x = {0.f, 0.f, 0.f, 0.f};
    if (r < rows) x = *(const hfg_f4 *)(a.z + ((size_t)r0 + r) * a.D + q);
    hfg_h4 h, l;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float v = fminf(fmaxf(x[j], -HFG_H_MAX), HFG_H_MAX);
      h[j] = (_Float16)v;
      l[j] = (_Float16)__fsub_rn(v, (float)h[j]);
    }
    *(hfg_h4 *)(dvqh_lds + r * LD + q) = h;
    if (SPLIT) *(hfg_h4 *)(dvqh_lds + plane + r * LD + q) = l;
  }
  DVQH_SYNC();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int ksn = a.D / 16, ctn = a.N / 32, slabs = (a.N + DVQ_SLAB - 1) / DVQ_SLAB;
  const _Float16 *zb = dvqh_lds + lr * LD + lk * 8; // lane half lk holds channels 16 ks + 8 lk .. + 7 of both operands; the lane's rows of z: lr and 32 + lr
  float *rv = (float *)(dvqh_lds + (SPLIT ? 2 : 1) * plane); // [slot][wave][row], then the indices
  int *ri = (int *)(rv + 2 * 4 * DVQ_TM);
  const int s_end = min(slabs, ((int)blockIdx.y + 1) * a.spw);
  for (int sl = blockIdx.y * a.spw, it = 0; sl < s_end; sl++, it++) {
    const int t_end = min(ctn, (sl + 1) * (DVQ_SLAB / 32));        // tiles of this slab: [8 sl, t_end)
    const int ct0 = sl * (DVQ_SLAB / 32) + wave;
    const int ct1 = ct0 + 4 < t_end ? ct0 + 4 : ct0;               // a tail slab without tile w + 4: tile w twice, the same (value, index) twice
    float best[2] = {INFINITY, INFINITY};
    int bi[2] = {0x7fffffff, 0x7fffffff};
    if (ct0 < t_end) {
      f32x16 acc00, acc01, acc10, acc11; // [tile][row half]
#pragma unroll
      for (int r = 0; r < 16; r++) { acc00[r] = 0.f; acc01[r] = 0.f; acc10[r] = 0.f; acc11[r] = 0.f; }
      hfg_h8 h0 = {0, 0, 0, 0, 0, 0, 0, 0}, l0 = h0, h1 = h0, l1 = h0, nh0 = h0, nl0 = h0, nh1 = h0, nl1 = h0;
      DVQH_ELOAD(0, h0, l0, h1, l1);
      for (int ks = 0; ks < ksn; ks++) {
        if (ks + 1 < ksn) DVQH_ELOAD(ks + 1, nh0, nl0, nh1, nl1);
        const hfg_h8 z0 = *(const hfg_h8 *)(zb + ks * 16), z1 = *(const hfg_h8 *)(zb + 32 * LD + ks * 16);
        if (SPLIT) { // the small terms first
          const hfg_h8 y0 = *(const hfg_h8 *)(zb + plane + ks * 16), y1 = *(const hfg_h8 *)(zb + plane + 32 * LD + ks * 16);
          acc00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h0, y0, acc00, 0, 0, 0);
          acc01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h0, y1, acc01, 0, 0, 0);
          acc10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, y0, acc10, 0, 0, 0);
          acc11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, y1, acc11, 0, 0, 0);
          acc00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(l0, z0, acc00, 0, 0, 0);
          acc01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(l0, z1, acc01, 0, 0, 0);
          acc10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(l1, z0, acc10, 0, 0, 0);
          acc11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(l1, z1, acc11, 0, 0, 0);
        }
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h0, z0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h0, z1, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, z0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, z1, acc11, 0, 0, 0);
        h0 = nh0; h1 = nh1;
        if (SPLIT) { l0 = nl0; l1 = nl1; }
      }
      DVQH_MIN(acc00, ct0, 0);
      DVQH_MIN(acc01, ct0, 1);
      DVQH_MIN(acc10, ct1, 0);
      DVQH_MIN(acc11, ct1, 1);
    }
    // the two lanes of a row (lk 0 holds block rows 0-3, 8-11, .., lk 1 the others), then the wave's 64 rows into its line of the slot
    const int slot = (it & 1) * 4 * DVQ_TM;
#pragma unroll
    for (int m = 0; m < 2; m++) {
      const float ov = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ 32) * 4, __builtin_bit_cast(int, best[m])));
      const int oi = __builtin_amdgcn_ds_bpermute((lane ^ 32) * 4, bi[m]);
      if (ov < best[m] || (ov == best[m] && oi < bi[m])) { best[m] = ov; bi[m] = oi; }
      if (lk == 0) { rv[slot + wave * DVQ_TM + m * 32 + lr] = best[m]; ri[slot + wave * DVQ_TM + m * 32 + lr] = bi[m]; }
    }
    DVQH_SYNC(); // one barrier per slab: the slot written now was last read two slabs ago, behind the barrier of the slab between
    if ((int)threadIdx.x < rows) {
      float v = rv[slot + threadIdx.x];
      int i = ri[slot + threadIdx.x];
      for (int w = 1; w < 4; w++) {
        const float ov = rv[slot + w * DVQ_TM + threadIdx.x];
        const int oi = ri[slot + w * DVQ_TM + threadIdx.x];
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
      }
      const size_t o = (size_t)sl * a.R + r0 + threadIdx.x;
      a.pv[o] = v; a.pi[o] = i;
    }
  }
}

#undef DVQH_MIN
#undef DVQH_ELOAD
#undef DVQH_SYNC

// slabs of a workgroup: 1 until the launch has 512 workgroups (two per compute unit) without it, then 2, 4, 8 while that stays so. The result's bits do not depend on it.
inline int dvae_vq_h_spw(int R, int N) {
  const int rt = (R + DVQ_TM - 1) / DVQ_TM, slabs = (N + DVQ_SLAB - 1) / DVQ_SLAB;
  int spw = 1;
  while (spw < 8 && (int64_t)rt * ((slabs + 2 * spw - 1) / (2 * spw)) >= 512) spw *= 2;
  return spw;
}

// what the kernel tiles (dvae_parse admits nothing else)
inline bool dvae_vq_h_ok(const DvaeVqH &a) {
  return a.z && a.eh && a.el && a.es && a.e2 && a.pv && a.pi && a.R >= 1 && a.D >= 32 && a.D % 32 == 0 && a.D <= DVAE_MAX_DIM && a.N >= 32 && a.N % 32 == 0 && a.N <= DVAE_MAX_TOKENS &&
         (a.R + DVQ_TM - 1) / DVQ_TM <= (1 << 24);
}

// The quantiser in modes 1 / 2: the kernel, then dvae_vq_reduce_kernel over its slabs. a.spw is set here. best: null or [R].
inline hipError_t dvae_launch_vq_h(DvaeVqH a, bool split, int *codes, float *best, hipStream_t st) {
  if (!dvae_vq_h_ok(a)) return hipErrorInvalidValue;
  static bool raised[2] = {false, false}; // more than 64 KB of dynamic LDS at the full codebook dim
  if (!raised[split]) {
    const void *f = split ? (const void *)dvae_vq_h_kernel<true> : (const void *)dvae_vq_h_kernel<false>;
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dvae_vq_h_lds(split, DVAE_MAX_DIM));
    if (e != hipSuccess) return e;
    raised[split] = true;
  }
  const int slabs = (a.N + DVQ_SLAB - 1) / DVQ_SLAB;
  a.spw = dvae_vq_h_spw(a.R, a.N);
  const dim3 grid((unsigned)((a.R + DVQ_TM - 1) / DVQ_TM), (unsigned)((slabs + a.spw - 1) / a.spw));
  if (split) dvae_vq_h_kernel<true><<<grid, 256, dvae_vq_h_lds(true, a.D), st>>>(a);
  else dvae_vq_h_kernel<false><<<grid, 256, dvae_vq_h_lds(false, a.D), st>>>(a);
  dvae_vq_reduce_kernel<<<(unsigned)((a.R + 255) / 256), 256, 0, st>>>(a.pv, a.pi, a.R, slabs, a.N, codes, best);
  return hipSuccess;
}

} // namespace
} // namespace tts
