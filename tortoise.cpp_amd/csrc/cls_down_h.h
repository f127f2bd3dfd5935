// The strided convolutions of the classifier (the five C -> 2C Downsamples) and of the wav2vec2 aligner (the 512 -> 512 extractor layers) on the fp16 MFMA
// (option "addon_conv_precision" 1 and 2): cls_down_h_kernel<SPLIT>.
//
// Included once, in classifier.h right behind cls_down_kernel, whose argument (ClsDown) and contract it keeps (hifigan.hip's translation unit: HFG_SEQ, f32x16,
// hfg_conv_h.h's HFG_H_MAX, HFG_H_NOPK, vector types and weight packer); cls_launch_down_h (below) launches it. Time-major f32 rows in and out, seq_in / seq_out
// records; output row t of a clip reads the clip's input rows t stride - pad + tap, a row outside the clip reads as zero, no store leaves the clip's output rows,
// the epilogue adds the bias. cls_down_kernel multiplies on v_mfma_f32_32x32x2_f32, 1/16 of the fp16 MFMA rate; this kernel multiplies on
// v_mfma_f32_32x32x16_f16 with hfg_conv_h_kernel's arithmetic:
//   SPLIT = false (mode 1)  x clamped to +-65504 and W s rounded to fp16, one MFMA per K step of 16, f32 accumulation
//   SPLIT = true  (mode 2)  x = xh + xl and W s = wh + wl, each half an fp16 number; xl wh, xh wl, then xh wh per K step (the small terms first), f32 accumulation
// The weight planes are hfg_pack_launch's with pt = taps on the [tap][cin][cout] tensor as it lies: [tap][cin / 16][cout / 32][lane][8] and one power-of-two
// scale s per output channel; the epilogue multiplies the sum by 1 / s, exactly, and adds the bias.
//
// Work split. One workgroup: CDH_TM = 64 output rows of one clip x 64 output channels on 4 waves; wave w owns the 32 x 32 tile (row half w & 1, column group
// w >> 1), one accumulator. 64 rows, not 128: the window of a 128-row tile at stride 4 is 520 LDS rows, 75 KB (83 KB in two planes with SPLIT), and the ring
// below holds two of them, which gfx950's 160 KB cannot (SPLIT) or can for one workgroup only; at 64 rows the ring is 75 KB / 83 KB at the classifier's
// (k 5, stride 4: two workgroups per compute unit, one with SPLIT) and 37 KB / 42 KB at the aligner's (k 3, stride 2: four, three with SPLIT), so a workgroup's
// barrier is hidden by its neighbours nearly everywhere. The compiler's resource summary (profiles/addon_conv.txt): 146 / 114 VGPRs, 16 AGPRs, occupancy 3,
// no scratch and no spill in either instantiation, so registers never limit what LDS admits.
// Staging. The input window ((64 - 1) stride + taps rows) goes through LDS per chunk of 64 channels (32 with SPLIT, whose two planes then cost the same LDS),
// clamped and converted on the way: fp16 planes [row][chunk + 8]. As in cls_down_kernel the rows are DE-INTERLEAVED by their residue modulo the stride: window row
// r lies at LDS row (r % stride) rph + r / stride, rph = 64 + (taps - 1) / stride. The 32 rows of an A fragment, `stride` apart in the window, are then
// consecutive LDS rows, and tap j is the plane j % stride at the row offset j / stride. The 8 halves of padding make the row stride 144 / 80 bytes, so a lane's A
// operand is one 16-byte read and 8 consecutive rows cover the 32 banks once (hfg_conv_h_kernel's layout). Where taps < stride only the residues 0 .. taps - 1
// exist in LDS: the rows of the other residues are never read, not even from global memory.
// The ring has two slots. A thread knows its share of the window once (the input row of each of its float4, or none); it issues the loads of chunk c + 1 into
// registers before the MFMAs of chunk c and converts and stores them into the other slot behind them: one barrier per chunk (the slot written in iteration c was
// last read in iteration c - 1, which every wave has left), where cls_down_kernel has two with nothing in flight between them. The B fragments come straight
// from the packed planes in global memory (L2: every row tile of the launch reads the same KiBs) into registers one K step ahead of the MFMAs that use them,
// across tap and chunk edges.
// Per output element the order is fixed: channel chunks ascending, taps, K steps of 16, the (up to three) MFMAs of a step; no split-K, no atomics: two runs
// agree bit for bit and a clip has the same bits alone and in a batch.
// Shapes: cin % 32 == 0, cout % 64 == 0, taps >= 1, stride >= 1, pad >= 0 with at most CDH_MAX_ROWS LDS rows of window (min(stride, taps) x rph: every
// geometry the two models use, strides up to 6 at k 5); cls_launch_down_h returns false for everything else and the caller takes cls_down_kernel.
#pragma once

namespace tts {
namespace {

constexpr int CDH_TM = 64;         // output rows of a workgroup: 2 row halves x 2 column groups of 32 over its 4 waves
constexpr int CDH_MAX_ROWS = 320;  // LDS rows of a staged window, at most: what a thread's CDH_MAX_ROWS / 16 staging registers (float4) cover
template <bool SPLIT> constexpr int cdh_chunk() { return SPLIT ? 32 : 64; } // channels of a staging chunk
inline int cdh_rph(int taps, int stride) { return CDH_TM + (taps - 1) / stride; }                   // LDS rows per residue of the stride
inline int cdh_rows(int taps, int stride) { return (stride < taps ? stride : taps) * cdh_rph(taps, stride); } // LDS rows of a window
// dynamic LDS of a launch: two slots x (one plane or two) x the window's rows x (chunk + 8) halves
inline size_t cdh_lds(bool split, int taps, int stride) { return (size_t)2 * (split ? 2 : 1) * cdh_rows(taps, stride) * ((split ? 32 : 64) + 8) * sizeof(_Float16); }

#define CDH_SYNC()                                        \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
    __builtin_amdgcn_s_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); \
  } while (0)
// a thread's share of chunk c0_: the channels c0_ + sq .. + 3 of its NL window rows; a row outside the clip (or outside the window) and, in the 32-channel
// tail chunk of a 64-channel tiling, the upper half of a row are not read (the empty asm: the row is tested again in every chunk, a VALU compare, instead of
// NL lane masks that live in scalar registers across the chunk loop and spill)
#define CDH_GLOAD(c0_)                                                                                                          \
  _Pragma("unroll") for (int i = 0; i < NL; i++) {                                                                              \
    int t_ = trow[i];                                                                                                           \
    asm volatile("" : "+v"(t_));                                                                                                \
    x[i] = hfg_f4{0.f, 0.f, 0.f, 0.f};                                                                                          \
    if (t_ >= 0 && (c0_) + sq < a.cin) x[i] = *(const hfg_f4 *)(in + (size_t)t_ * a.cin + (c0_) + sq);                          \
  }
#define CDH_STORE(slot_)                                                                                                        \
  _Pragma("unroll") for (int i = 0; i < NL; i++) {                                                                              \
    const int lrow_ = sr + RP * i;                                                                                              \
    if (lrow_ < nrows) {                                                                                                        \
      hfg_h4 h_, l_;                                                                                                            \
      _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                           \
        const float v_ = fminf(fmaxf(x[i][j], -HFG_H_MAX), HFG_H_MAX);                                                          \
        h_[j] = (_Float16)v_;                                                                                                   \
        l_[j] = (_Float16)__fsub_rn(v_, (float)h_[j]);                                                                          \
      }                                                                                                                         \
      _Float16 *d_ = cdh_lds_mem + (size_t)(slot_) * slot + lrow_ * LD + sq;                                                    \
      *(hfg_h4 *)d_ = h_;                                                                                                       \
      if (SPLIT) *(hfg_h4 *)(d_ + plane) = l_;                                                                                  \
    }                                                                                                                           \
  }
// the wave's B fragments of K step ksg_ of tap tap_: one 16-byte load per lane and plane
#define CDH_BLOAD(tap_, ksg_, bh_, bl_)                                                                                         \
  do {                                                                                                                          \
    const size_t o_ = (((size_t)(tap_) * ksn + (ksg_)) * ctn + ct) * 512 + lane * 8;                                            \
    bh_ = *(const hfg_h8 *)(wh + o_);                                                                                           \
    if (SPLIT) bl_ = *(const hfg_h8 *)(wl + o_);                                                                                \
  } while (0)

template <bool SPLIT>
__global__ HFG_H_NOPK __launch_bounds__(256) void cls_down_h_kernel(const ClsDown a, const _Float16 *__restrict__ wh, const _Float16 *__restrict__ wl,
                                                                   const float *__restrict__ ws) {
  extern __shared__ __align__(16) _Float16 cdh_lds_mem[];
  constexpr int CW = cdh_chunk<SPLIT>(), LD = CW + 8, QPR = CW / 4, RP = 256 / QPR, NL = CDH_MAX_ROWS / RP; // float4 of a row; rows of a staging pass; passes
  const int s = blockIdx.y;
  const int fi = a.seq_in[HFG_SEQ * s], Tin = a.seq_in[HFG_SEQ * s + 1], fo = a.seq_out[HFG_SEQ * s], Tout = a.seq_out[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * CDH_TM;
  if (t0 >= Tout) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int m0 = (wave & 1) * 32, ct = blockIdx.z * 2 + (wave >> 1);
  const int F = a.stride, win = (CDH_TM - 1) * F + a.taps, rph = CDH_TM + (a.taps - 1) / F, nrows = min(F, a.taps) * rph;
  const int plane = nrows * LD, slot = (SPLIT ? 2 : 1) * plane; // halves
  const int ksn = a.cin / 16, ctn = a.cout / 32;
  const bool live = t0 + m0 < Tout; // a wave whose 32 rows all lie behind the clip stages its share and multiplies nothing
  const float *in = a.in + (size_t)fi * a.cin;
  const int sr = threadIdx.x / QPR, sq = (threadIdx.x % QPR) * 4;
  // the thread's window rows, once: LDS row sr + RP i holds window row r = (row within the residue) stride + residue, the clip's row base + r
  int trow[NL];
  {
    const int base = t0 * F - a.pad;
#pragma unroll
    for (int i = 0; i < NL; i++) {
      const int lrow = sr + RP * i, p = lrow / rph, r = (lrow - p * rph) * F + p, t = base + r;
      trow[i] = lrow < nrows && r < win && t >= 0 && t < Tin ? t : -1;
    }
  }
  hfg_f4 x[NL];
  hfg_h8 bh = {0, 0, 0, 0, 0, 0, 0, 0}, bl = bh, nh = bh, nl = bh;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  CDH_GLOAD(0);
  if (live) CDH_BLOAD(0, 0, bh, bl);
  CDH_STORE(0);
  CDH_SYNC();
  for (int c0 = 0, c = 0; c0 < a.cin; c0 += CW, c++) {
    const bool more = c0 + CW < a.cin;
    if (more) { // in flight under this chunk's MFMAs
      CDH_GLOAD(c0 + CW);
    }
    if (live) {
      const int ks_n = min(CW, a.cin - c0) / 16;
      const _Float16 *ph = cdh_lds_mem + (size_t)(c & 1) * slot + (m0 + lr) * LD + lk * 8; // lane half lk holds channels 16 ks + 8 lk .. + 7 of both operands
      for (int tap = 0, tp = 0, tq = 0; tap < a.taps; tap++) { // tp = tap % stride: the plane; tq = tap / stride: the row offset
        const _Float16 *pa = ph + (tp * rph + tq) * LD;
        for (int ks = 0; ks < ks_n; ks++) {
          // the next step's fragments: the next K step, the next tap's first, or the next chunk's first
          if (ks + 1 < ks_n) CDH_BLOAD(tap, c0 / 16 + ks + 1, nh, nl);
          else if (tap + 1 < a.taps) CDH_BLOAD(tap + 1, c0 / 16, nh, nl);
          else if (more) CDH_BLOAD(0, (c0 + CW) / 16, nh, nl);
          const hfg_h8 a0 = *(const hfg_h8 *)(pa + ks * 16);
          if (SPLIT) { // the small terms first
            const hfg_h8 l0 = *(const hfg_h8 *)(pa + plane + ks * 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(l0, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, bl, acc, 0, 0, 0);
          }
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, bh, acc, 0, 0, 0);
          bh = nh;
          if (SPLIT) bl = nl;
        }
        if (++tp == F) { tp = 0; tq++; }
      }
    }
    if (more) {
      CDH_STORE((c + 1) & 1);
      CDH_SYNC();
    }
  }
  if (!live) return;
  const int col = ct * 32 + lr;
  const float inv_s = ws[col], bv = a.bias[col];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int t = t0 + m0 + 8 * (r >> 2) + 4 * lk + (r & 3); // C/D map of the 32 x 32 MFMA: column on the lane
    if (t < Tout) a.out[((size_t)fo + t) * a.cout + col] = __fmul_rn(acc[r], inv_s) + bv; // the scale is a power of two: the product is exact
  }
}

#undef CDH_BLOAD
#undef CDH_STORE
#undef CDH_GLOAD
#undef CDH_SYNC

// what the kernel tiles; the launcher refuses everything else
inline bool cls_down_h_ok(const ClsDown &a, const _Float16 *wh, const _Float16 *wl, const float *ws, int max_out, int B) {
  return a.in && a.out && a.bias && a.seq_in && a.seq_out && wh && wl && ws && a.cin >= 32 && a.cin % 32 == 0 && a.cout >= 64 && a.cout % 64 == 0 &&
         a.cout / 64 <= 65535 && a.taps >= 1 && a.taps <= 64 && a.stride >= 1 && a.stride <= 64 && a.pad >= 0 && a.pad <= 65536 &&
         cdh_rows(a.taps, a.stride) <= CDH_MAX_ROWS && max_out >= 1 && max_out <= (1 << 24) && B >= 1 && B <= 65535;
}

// One launch for the whole ragged batch (max_out: the longest clip's output rows). wh, wl, ws: the layer's packed planes and scales (hfg_pack_launch, pt = taps).
// false: a shape the kernel does not tile; nothing was launched and the caller takes cls_launch_down.
inline bool cls_launch_down_h(const ClsDown &a, const _Float16 *wh, const _Float16 *wl, const float *ws, bool split, int max_out, int B, hipStream_t st) {
  if (!cls_down_h_ok(a, wh, wl, ws, max_out, B)) return false;
  const dim3 grid((unsigned)((max_out + CDH_TM - 1) / CDH_TM), (unsigned)B, (unsigned)(a.cout / 64));
  const size_t lds = cdh_lds(split, a.taps, a.stride);
  if (split) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)cls_down_h_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    cls_down_h_kernel<true><<<grid, 256, lds, st>>>(a, wh, wl, ws);
  } else {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)cls_down_h_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    cls_down_h_kernel<false><<<grid, 256, lds, st>>>(a, wh, wl, ws);
  }
  return true;
}

} // namespace
} // namespace tts
