// The Linears of the wav2vec2 aligner's encoder on the fp16 MFMA (option "aligner_precision" 1 and 2): short, ragged row panels.
//
// Included once, as the last line of hfg_conv_h.h (hifigan.hip's translation unit; its operand contract, weight packer, HFG_H_NOPK and vector types; HFG_SEQ and f32x16 are hifigan.hip's);
// aligner.h launches it. hfg_conv_h_kernel is shaped for long convolutions: 256 rows per workgroup, so a 460-frame clip is two row tiles per column block and
// most of the chip idles. This kernel computes
//   out[r][n] = epi((sum_k x[r][k] W[k][n]) / s_n + b_n)          on the live rows of a ragged batch (clip s: rows [start_s, start_s + n_s) of the HFG_SEQ table)
// with exactly that kernel's operands: W packed at load by hfg_pack_launch with pt = 1 (two fp16 planes in fragment order [cin / 16][cout / 32][lane][8], one
// power-of-two scale per column), x f32 in global memory, clamped to +-65504 and converted on the way into LDS: xh = rn_f16(x), with SPLIT also xl = rn_f16(x - xh).
// Per K step of 16 on v_mfma_f32_32x32x16_f16: SPLIT = false one MFMA; SPLIT = true xl wh, xh wl, then xh wh (the small terms first); f32 accumulation.
//
// One workgroup: 64 rows of one clip x 64 columns on 4 waves, each wave ONE 32 x 32 accumulator (row half wave & 1, column tile wave >> 1): a 460-row clip at
// cout 1024 is 8 x 16 = 128 workgroups. The A panel goes through LDS in K chunks of 64 channels as padded fp16 planes [64][64 + 8] (the row stride of 144 bytes
// lets the 16-byte fragment reads of 8 rows cover the 32 banks once), in a ring of two slots: a thread loads its 4 float4 of chunk c + 1 from global memory
// before the MFMAs of chunk c and converts and stores them behind those MFMAs, so one barrier per chunk is enough (the slot written in iteration c was last
// read in iteration c - 1, which every wave has left). The B fragments come from global memory (L2) straight into registers one K step ahead, across chunk
// edges. No split-K, no atomics: per output element the order is K ascending, then the (up to three) MFMAs of a step, whatever the tile, so a clip's bits are
// the same alone or in any batch and two runs agree. No row outside the clips is loaded or stored: a tile's rows behind its clip are zeros in LDS.
// Epilogue, in this order: acc * (1 / s) (exact), + bias, [GELU], [+ resid]; resid may be out (an element is read and written by the same thread).
// cin and cout multiples of 64 (what aligner_parse accepts for C, D and the feed-forward width); the launcher refuses everything else.
#pragma once

namespace tts {
namespace {

constexpr int W2V_H_TM = 64, W2V_H_TN = 64; // rows and columns of a workgroup
constexpr int W2V_H_CK = 64;                // channels of a staging chunk: 4 K steps
constexpr int W2V_H_LD = W2V_H_CK + 8;      // halves of an LDS row
enum { W2V_EPI_BIAS = 0, W2V_EPI_GELU = 1, W2V_EPI_RESID = 2 };

// the exact erf GELU of the aligner (w2v_ln_kernel, w2v_gelu_kernel, w2v_pos_kernel and the GELU epilogue below)
__device__ __forceinline__ float w2v_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

struct W2vLinearH {
  const float *in;    // [rows][cin]
  float *out;         // [rows][cout]
  const float *resid; // W2V_EPI_RESID: [rows][cout], may be `out`
  const float *bias;  // [cout]
  const int *seq;     // the level's HFG_SEQ records: {first row, rows, ..}
  int cin, cout;
};

#define W2V_H_SYNC()                                      \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
    __builtin_amdgcn_s_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); \
  } while (0)
// a thread's share of chunk c0 .. c0 + 63: rows sr + 16 j, channels sq .. sq + 3; a row behind the clip is not read
#define W2V_H_GLOAD(c0_)                                                                                                       \
  _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                              \
    const int r_ = sr + 16 * j;                                                                                                \
    x[j] = hfg_f4{0.f, 0.f, 0.f, 0.f};                                                                                         \
    if (t0 + r_ < T) x[j] = *(const hfg_f4 *)(in + (size_t)r_ * a.cin + (c0_) + sq);                                           \
  }
#define W2V_H_STORE(slot_)                                                                                                     \
  _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                              \
    hfg_h4 h_, l_;                                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 4; i++) {                                                                            \
      const float v_ = fminf(fmaxf(x[j][i], -HFG_H_MAX), HFG_H_MAX);                                                           \
      h_[i] = (_Float16)v_;                                                                                                    \
      l_[i] = (_Float16)__fsub_rn(v_, (float)h_[i]);                                                                           \
    }                                                                                                                          \
    *(hfg_h4 *)(&lds[slot_][0][(sr + 16 * j) * W2V_H_LD + sq]) = h_;                                                           \
    if (SPLIT) *(hfg_h4 *)(&lds[slot_][SPLIT ? 1 : 0][(sr + 16 * j) * W2V_H_LD + sq]) = l_;                                    \
  }
// the wave's B fragments of K step ksg_: one 16-byte load per lane and plane
#define W2V_H_BLOAD(ksg_, bh_, bl_)                                                                                            \
  do {                                                                                                                         \
    const size_t o_ = ((size_t)(ksg_) * ctn + ct) * 512 + lane * 8;                                                            \
    bh_ = *(const hfg_h8 *)(wh + o_);                                                                                          \
    if (SPLIT) bl_ = *(const hfg_h8 *)(wl + o_);                                                                               \
  } while (0)

template <bool SPLIT, int EPI>
__global__ HFG_H_NOPK __launch_bounds__(256) void w2v_linear_h_kernel(const W2vLinearH a, const _Float16 *__restrict__ wh, const _Float16 *__restrict__ wl,
                                                                      const float *__restrict__ ws) {
  __shared__ __align__(16) _Float16 lds[2][SPLIT ? 2 : 1][W2V_H_TM * W2V_H_LD]; // [slot][plane][row][W2V_H_LD]: 18 KB, 36 KB with SPLIT
  const int s = blockIdx.y;
  const int f0 = a.seq[HFG_SEQ * s], T = a.seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * W2V_H_TM;
  if (t0 >= T) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int m0 = (wave & 1) * 32, ct = blockIdx.z * (W2V_H_TN / 32) + (wave >> 1);
  const int ksn = a.cin / 16, ctn = a.cout / 32, chunks = a.cin / W2V_H_CK;
  const bool live = t0 + m0 < T; // a wave whose 32 rows all lie behind the clip stages its share and multiplies nothing
  const float *in = a.in + ((size_t)f0 + t0) * a.cin;
  const int sr = threadIdx.x >> 4, sq = (threadIdx.x & 15) * 4;
  hfg_f4 x[4];
  hfg_h8 bh = {0, 0, 0, 0, 0, 0, 0, 0}, bl = bh, nh = bh, nl = bh;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  W2V_H_GLOAD(0);
  if (live) W2V_H_BLOAD(0, bh, bl);
  W2V_H_STORE(0);
  W2V_H_SYNC();
  for (int c = 0; c < chunks; c++) {
    const bool more = c + 1 < chunks;
    if (more) { // in flight under this chunk's MFMAs
      W2V_H_GLOAD((c + 1) * W2V_H_CK);
    }
    if (live) {
      const _Float16 *ph = &lds[c & 1][0][(m0 + lr) * W2V_H_LD + lk * 8]; // lane half lk holds channels 16 ks + 8 lk .. + 7 of both operands
      const _Float16 *pl = &lds[c & 1][SPLIT ? 1 : 0][(m0 + lr) * W2V_H_LD + lk * 8];
#pragma unroll
      for (int ks = 0; ks < W2V_H_CK / 16; ks++) {
        const int ksg = c * (W2V_H_CK / 16) + ks;
        if (ksg + 1 < ksn) W2V_H_BLOAD(ksg + 1, nh, nl);
        const hfg_h8 a0 = *(const hfg_h8 *)(ph + ks * 16);
        if (SPLIT) { // the small terms first
          const hfg_h8 l0 = *(const hfg_h8 *)(pl + ks * 16);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(l0, bh, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, bl, acc, 0, 0, 0);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, bh, acc, 0, 0, 0);
        bh = nh;
        if (SPLIT) bl = nl;
      }
    }
    if (more) {
      W2V_H_STORE((c + 1) & 1);
      W2V_H_SYNC();
    }
  }
  if (!live) return;
  const int col = ct * 32 + lr;
  const float inv_s = ws[col], bv = a.bias[col];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int t = t0 + m0 + 8 * (r >> 2) + 4 * lk + (r & 3); // C/D map of the 32 x 32 MFMA: column on the lane
    if (t < T) {
      const size_t o = ((size_t)f0 + t) * a.cout + col;
      float v = __fmul_rn(acc[r], inv_s) + bv; // the scale is a power of two: the product is exact
      if (EPI == W2V_EPI_GELU) v = w2v_gelu(v);
      if (EPI == W2V_EPI_RESID) v += a.resid[o];
      a.out[o] = v;
    }
  }
}

#undef W2V_H_BLOAD
#undef W2V_H_STORE
#undef W2V_H_GLOAD
#undef W2V_H_SYNC

// what the kernel tiles; the launcher refuses everything else
inline bool w2v_linear_h_ok(const W2vLinearH &a, const _Float16 *wh, const _Float16 *wl, const float *ws, int epi, int max_n, int B) {
  return a.in && a.out && a.bias && a.seq && wh && wl && ws && a.cin >= W2V_H_CK && a.cin % W2V_H_CK == 0 && a.cout >= W2V_H_TN && a.cout % W2V_H_TN == 0 &&
         epi >= W2V_EPI_BIAS && epi <= W2V_EPI_RESID && (epi != W2V_EPI_RESID || a.resid) && max_n >= 1 && B >= 1 && B <= 65535 && a.cout / W2V_H_TN <= 65535;
}

// One launch for the whole ragged batch (max_n: the longest clip's rows). wh, wl, ws: the layer's packed planes and scales (hfg_pack_launch, pt = 1).
// false: a shape the kernel does not tile; nothing was launched.
inline bool w2v_linear_h_launch(hipStream_t stream, const W2vLinearH &a, const _Float16 *wh, const _Float16 *wl, const float *ws, bool split, int epi, int max_n, int B) {
  if (!w2v_linear_h_ok(a, wh, wl, ws, epi, max_n, B)) return false;
  const dim3 grid((unsigned)((max_n + W2V_H_TM - 1) / W2V_H_TM), (unsigned)B, (unsigned)(a.cout / W2V_H_TN));
#define W2V_H_GO(S, E) w2v_linear_h_kernel<S, E><<<grid, 256, 0, stream>>>(a, wh, wl, ws)
  if (split) {
    if (epi == W2V_EPI_BIAS) W2V_H_GO(true, W2V_EPI_BIAS);
    else if (epi == W2V_EPI_GELU) W2V_H_GO(true, W2V_EPI_GELU);
    else W2V_H_GO(true, W2V_EPI_RESID);
  } else {
    if (epi == W2V_EPI_BIAS) W2V_H_GO(false, W2V_EPI_BIAS);
    else if (epi == W2V_EPI_GELU) W2V_H_GO(false, W2V_EPI_GELU);
    else W2V_H_GO(false, W2V_EPI_RESID);
  }
#undef W2V_H_GO
  return true;
}

} // namespace
} // namespace tts
