// The convolutions of the HiFi-GAN decoder and of the vocoder that shares its kernel on the fp16 MFMA (option "hfg_precision" 1 and 2).
//
// Included once, in hifigan.hip behind its f32 kernels (HfgConv, HFG_SEQ, HFG_TM and f32x16 are declared there). hfg_conv_kernel multiplies on
// v_mfma_f32_32x32x2_f32, 1/16 of the fp16 MFMA rate; hfg_conv_h_kernel keeps its contract (f32 activations in global memory, the same HfgConv, the same
// candidate table, zero predication at a candidate's ends, the same epilogue) and multiplies on v_mfma_f32_32x32x16_f16:
//   SPLIT = false (hfg_precision 1)  act(x) and W rounded to fp16, one MFMA per K step, f32 accumulation
//   SPLIT = true  (hfg_precision 2)  act(x) = xh + xl and W s = wh + wl, each half an fp16 number; xl wh, xh wl, then xh wh per K step (the small terms first,
//                                    xl wl dropped: 2^-22 of the term), f32 accumulation
// Weights are packed at load (hfg_pack_*_kernel) into two fp16 planes in MFMA-fragment order,
//   [phase][tap][cin / 16][cout / 32][lane 0 .. 63][8]    lane = 32 (k / 8 % 2) + column % 32: the 8 consecutive input channels a lane multiplies,
// so a wave's B operand of one K step and one 32-column tile is one 16-byte load per lane of a contiguous KiB. Every output channel has one power-of-two scale s:
// its largest |w| s lies in [2^12, 2^13), so the low half of a weight 2^-14 of the column's largest still has all its bits above fp16's subnormal quantum; the
// epilogue multiplies the sum by 1 / s, exactly.
//
// One workgroup: 256 rows of one candidate x 32 NT output channels (x one phase), a wave owns 64 rows (hfg_conv_kernel's split). The input window
// (256 + (taps - 1) dil rows) goes through LDS once per chunk of CW channels (64; 32 with SPLIT, whose two planes then cost the same LDS), activated in f32 exactly
// as hfg_conv_kernel does it, clamped to +-65504 and converted on the way in: fp16 planes [row][CW + 8]. The 8 halves of padding make the row stride 144 / 80
// bytes, so the 16-byte A-fragment reads of 8 consecutive rows cover the 32 banks once; a tap is a row offset into the same window. The B fragments come
// straight from global memory (L2: every workgroup of the launch reads the same KiBs) into registers one K step ahead of the MFMAs that use them.
// Per output element the order is fixed: channel chunks ascending, taps, K steps of 16, the (up to three) MFMAs of a step; no split-K, no atomics. Hence a chunk's
// samples are the bits of the whole call and a candidate's are the same alone or in a batch, as in the f32 mode. cin % 32 == 0 and cout % 32 == 0, like the f32 kernel.
#pragma once

namespace tts {
namespace {

constexpr int HFG_H_EXP = 12;       // a column's largest |w| s lies in [2^HFG_H_EXP, 2^(HFG_H_EXP + 1))
constexpr float HFG_H_MAX = 65504.f; // the largest fp16 number: the activation is clamped to it before it is rounded
// The kernels of this file use no packed f32 arithmetic (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: the Makefile's note on PK) whatever the build's flags say; the
// rest of the translation unit keeps the build's code generation, bit for bit.
#if defined(__HIP_DEVICE_COMPILE__)
#define HFG_H_NOPK __attribute__((target("no-packed-fp32-ops")))
#else
#define HFG_H_NOPK
#endif
// (a header's device function is not inlined into a kernel whose target features differ from the build's: the barrier and the float4 are spelled with builtins)
#define HFG_H_SYNC()                                      \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
    __builtin_amdgcn_s_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); \
  } while (0)
typedef float hfg_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 hfg_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 hfg_h4 __attribute__((ext_vector_type(4)));

// ws[col] = 1 / s, ws[cout + col] = s for s = 2^(HFG_H_EXP - floor(log2 max |w[..][col]|)) (an all-zero column: s = 1); w is [rows][cout]
__global__ HFG_H_NOPK __launch_bounds__(64) void hfg_pack_scale_kernel(const float *__restrict__ w, int rows, int cout, float *__restrict__ ws) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= cout) return;
  float m = 0.f;
  for (int r = 0; r < rows; r++) m = fmaxf(m, fabsf(w[(size_t)r * cout + col]));
  const int e = m > 0.f ? max(ilogbf(m), -100) - HFG_H_EXP : 0;
  ws[col] = ldexpf(1.0f, e);
  ws[cout + col] = ldexpf(1.0f, -e);
}

// hi = rn_f16(w s), lo = rn_f16(w s - hi) in fragment order; one thread per lane of a fragment. w is [pt][cin][cout], pt = phases x taps.
__global__ HFG_H_NOPK __launch_bounds__(256) void hfg_pack_kernel(const float *__restrict__ w, const float *__restrict__ ws, int pt, int cin, int cout,
                                                       _Float16 *__restrict__ hi, _Float16 *__restrict__ lo) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int ksn = cin / 16, ctn = cout / 32;
  if (g >= (size_t)pt * ksn * ctn * 64) return;
  const int lane = (int)(g & 63);
  size_t rest = g >> 6;
  const int ct = (int)(rest % ctn); rest /= ctn;
  const int ks = (int)(rest % ksn), p = (int)(rest / ksn);
  const int col = ct * 32 + (lane & 31), k0 = ks * 16 + (lane >> 5) * 8;
  const float s = ws[cout + col];
  hfg_h8 h, l;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const float v = __fmul_rn(w[((size_t)p * cin + k0 + j) * cout + col], s);
    h[j] = (_Float16)v;
    l[j] = (_Float16)__fsub_rn(v, (float)h[j]);
  }
  *(hfg_h8 *)(hi + g * 8) = h;
  *(hfg_h8 *)(lo + g * 8) = l;
}

// both planes and the scales of one layer, on `stream`; hi, lo: pt cin cout halves each, ws: 2 cout floats
inline void hfg_pack_launch(hipStream_t stream, const float *w, int pt, int cin, int cout, _Float16 *hi, _Float16 *lo, float *ws) {
  hfg_pack_scale_kernel<<<(cout + 63) / 64, 64, 0, stream>>>(w, pt * cin, cout, ws);
  const size_t lanes = (size_t)pt * (cin / 16) * (cout / 32) * 64;
  hfg_pack_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, stream>>>(w, ws, pt, cin, cout, hi, lo);
}

template <bool SPLIT> constexpr int hfg_h_chunk() { return SPLIT ? 32 : 64; } // channels of a staging chunk
// dynamic LDS of a launch: the window's rows x (chunk + 8) halves, one plane or two
inline size_t hfg_conv_h_lds(bool split, int taps, int dil) {
  return (size_t)(HFG_TM + (taps - 1) * dil) * ((split ? 32 : 64) + 8) * 2 * (split ? 2 : 1);
}

template <bool SPLIT, int NT>
__global__ HFG_H_NOPK __launch_bounds__(256) void hfg_conv_h_kernel(const HfgConv a, const _Float16 *__restrict__ wh, const _Float16 *__restrict__ wl,
                                                         const float *__restrict__ ws) {
  extern __shared__ __align__(16) unsigned char hfg_h_lds[];
  constexpr int CW = hfg_h_chunk<SPLIT>(), LD = CW + 8;
  const int s = blockIdx.y;
  const int f0 = a.seq[HFG_SEQ * s], T = a.seq[HFG_SEQ * s + 1], voice = a.seq[HFG_SEQ * s + 2];
  const int Tin = T * a.rate, t0 = blockIdx.x * HFG_TM;
  if (t0 >= Tin) return;
  const int phase = blockIdx.z % a.phases, n0 = (blockIdx.z / a.phases) * 32 * NT;
  const int lo = a.phases > 1 ? (phase + a.pad_t) / a.phases - 1 : a.lo; // hfg_conv_kernel's rule for the phases of a transposed convolution
  const int win = HFG_TM + (a.taps - 1) * a.dil;
  const float *in = a.in + (size_t)f0 * a.rate * a.cin;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  _Float16 *ph = (_Float16 *)hfg_h_lds, *pl = ph + (size_t)win * LD;
  const int ksn = a.cin / 16, ctn = a.cout / 32;
  const bool live = t0 + wave * 64 < Tin; // a wave whose 64 rows all lie behind the candidate stages its share and multiplies nothing
  // the B fragments of K step ksg of tap `tap`: NT (x 2) 16-byte loads
#define HFG_H_BLOAD(tap_, ksg_, bh_, bl_)                                                                                   \
  do {                                                                                                                      \
    const size_t o_ = ((((size_t)phase * a.taps + (tap_)) * ksn + (ksg_)) * ctn + n0 / 32) * 512 + lane * 8;                \
    _Pragma("unroll") for (int n = 0; n < NT; n++) {                                                                        \
      bh_[n] = *(const hfg_h8 *)(wh + o_ + n * 512);                                                                        \
      if (SPLIT) bl_[n] = *(const hfg_h8 *)(wl + o_ + n * 512);                                                             \
    }                                                                                                                       \
  } while (0)
  f32x16 acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;
  for (int c0 = 0; c0 < a.cin; c0 += CW) {
    const int cw = min(CW, a.cin - c0), ks_n = cw / 16, sh = cw == 64 ? 4 : 3; // a chunk is 64 or 32 channels: 16 or 8 float4 per row
    hfg_h8 bh[NT], bl[NT], nh[NT], nl[NT];
    if (live) HFG_H_BLOAD(0, c0 / 16, bh, bl); // in flight while the window is staged
    HFG_H_SYNC();
    for (int idx = threadIdx.x; idx < (win << sh); idx += 256) {
      const int r = idx >> sh, q = (idx - (r << sh)) * 4, t = t0 + lo + r;
      hfg_f4 x = {0.f, 0.f, 0.f, 0.f};
      if (t >= 0 && t < Tin) x = *(const hfg_f4 *)(in + (size_t)t * a.cin + c0 + q);
      hfg_h4 h, l;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        x[j] = x[j] < 0.f ? x[j] * a.slope : x[j];
        x[j] = fminf(fmaxf(x[j], -HFG_H_MAX), HFG_H_MAX);
        h[j] = (_Float16)x[j];
        l[j] = (_Float16)__fsub_rn(x[j], (float)h[j]);
      }
      *(hfg_h4 *)(ph + r * LD + q) = h;
      if (SPLIT) *(hfg_h4 *)(pl + r * LD + q) = l;
    }
    HFG_H_SYNC();
    if (!live) continue;
    const int steps = a.taps * ks_n;
    for (int i = 0, tap = 0, ks = 0; i < steps; i++) {
      int ntap = tap, nks = ks + 1;
      if (nks == ks_n) { nks = 0; ntap++; }
      if (i + 1 < steps) HFG_H_BLOAD(ntap, c0 / 16 + nks, nh, nl);
      const int xo = (wave * 64 + lr + tap * a.dil) * LD + ks * 16 + lk * 8; // lane half lk holds channels c0 + 16 ks + 8 lk .. + 7 of both operands
      const hfg_h8 a0 = *(const hfg_h8 *)(ph + xo), a1 = *(const hfg_h8 *)(ph + xo + 32 * LD);
      if (SPLIT) {
        const hfg_h8 l0 = *(const hfg_h8 *)(pl + xo), l1 = *(const hfg_h8 *)(pl + xo + 32 * LD);
#pragma unroll
        for (int n = 0; n < NT; n++) { // the small terms first
          acc[0][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l0, bh[n], acc[0][n], 0, 0, 0);
          acc[1][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l1, bh[n], acc[1][n], 0, 0, 0);
          acc[0][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, bl[n], acc[0][n], 0, 0, 0);
          acc[1][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, bl[n], acc[1][n], 0, 0, 0);
        }
      }
#pragma unroll
      for (int n = 0; n < NT; n++) {
        acc[0][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, bh[n], acc[0][n], 0, 0, 0);
        acc[1][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, bh[n], acc[1][n], 0, 0, 0);
      }
#pragma unroll
      for (int n = 0; n < NT; n++) { bh[n] = nh[n]; if (SPLIT) bl[n] = nl[n]; }
      tap = ntap; ks = nks;
    }
  }
  if (!live) return;
  const size_t obase = (size_t)f0 * a.rate * a.phases * a.cout;
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int n = 0; n < NT; n++) {
      const int col = n0 + n * 32 + lr;
      const float inv_s = ws[col];
      float bv = a.bias[col];
      if (a.cbias) bv += a.cbias[(size_t)voice * a.cout + col];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int t = t0 + wave * 64 + m * 32 + 8 * (r >> 2) + 4 * lk + (r & 3); // C/D map of the 32 x 32 MFMA: column on the lane
        if (t < Tin) {
          const size_t o = obase + ((size_t)t * a.phases + phase) * a.cout + col;
          float v = __fmul_rn(acc[m][n][r], inv_s) + bv; // the scale is a power of two: the product is exact
          if (a.resid) v += a.resid[o];
          if (a.acc_mode == 1) v += a.out[o];
          else if (a.acc_mode == 2) v = (a.out[o] + v) / 3.0f;
          a.out[o] = v;
        }
      }
    }
}

#undef HFG_H_BLOAD
#undef HFG_H_SYNC

// One launch of the family for the whole ragged batch: hfg_conv_kernel's grid (max_rows: the longest candidate's input rows), two column tiles per workgroup
// where they divide cout. wh, wl, ws: the layer's packed planes and scales (hfg_pack_launch).
inline void hfg_conv_h_launch(hipStream_t stream, const HfgConv &a, const _Float16 *wh, const _Float16 *wl, const float *ws, bool split, size_t max_rows, int B) {
  const int nt = a.cout % 64 == 0 ? 2 : 1;
  const dim3 grid((unsigned)((max_rows + HFG_TM - 1) / HFG_TM), (unsigned)B, (unsigned)(a.cout / (32 * nt) * a.phases));
  const size_t lds = hfg_conv_h_lds(split, a.taps, a.dil);
  if (split) {
    if (nt == 2) hfg_conv_h_kernel<true, 2><<<grid, 256, lds, stream>>>(a, wh, wl, ws);
    else hfg_conv_h_kernel<true, 1><<<grid, 256, lds, stream>>>(a, wh, wl, ws);
  } else {
    if (nt == 2) hfg_conv_h_kernel<false, 2><<<grid, 256, lds, stream>>>(a, wh, wl, ws);
    else hfg_conv_h_kernel<false, 1><<<grid, 256, lds, stream>>>(a, wh, wl, ws);
  }
}

} // namespace
} // namespace tts

#include "w2v_linear_h.h" // w2v_linear_h_kernel: the aligner's Linears on the same operands (option "aligner_precision")
