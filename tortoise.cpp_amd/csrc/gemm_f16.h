// fp16 x fp16 -> f32 MFMA GEMM for gfx950 (v_mfma_f32_16x16x32_f16), used by the diffusion and
// vocoder stages for every convolution (the reference's conv1d IS an fp16 im2col GEMM with f32
// accumulation), for the attention projections, and (with split-precision operands) by the
// multi-row passes of the autoregressive stage.
//
//   C[m][n] = sum_seg sum_k A_seg[m + row_off_seg][k] * W[n][seg*kseg + k]
//
// A "segment" is one convolution tap (same activation buffer, row offset -1/0/+1: sequences are
// packed along M with a zero guard row between them, so a k=3 convolution needs no im2col and no
// boundary masking) or one half of a channel concat (two buffers, offset 0).
//
// Kernels. All of them: (16 h) x 128 x 64 tiles (h = 1..8 sixteen-row blocks, a launch parameter), 4 waves, the tile walk of gemm_vh_tile, operands staged
// by direct global->LDS DMA (global_load_lds_dwordx4) into a lane-linear image whose 16-byte chunks are XOR-swizzled on the SOURCE
// address, so ds_read_b128 fragment reads spread over all banks, f32 accumulators that may start from the residual, and one epilogue family (gemm_epilogue_vh for the
// 2 x 2 kernels, its copies gemm_epilogue_wreg / gemm_epilogue_conv3_wreg for the 1 x 4 layout). gemm_dma_off gives the DMA offsets of the vh, dual-B and wreg bodies and gemm_acc_start the
// accumulator start of the vh and wreg bodies; the dual-B start, the k = 3 offsets, the dual-B body and the wreg epilogue are copies, kept apart for the registers
// unifying them cost (see the comment at each; profiles/gemm_refactor_isa.txt). The three 2 x 2 kernels run one body per number of 16-row blocks of the calling
// wave (gemm_for_my_mi). What differs:
//   gemm_f16_vh_kernel        any segment structure; one LDS stage, 4 workgroups per CU overlap each other; KU K tiles per barrier pair for small problems
//   gemm_f16_vh_dualb_kernel  the hi | lo halves of ONE weight over one activation operand: both weight tiles of a K tile staged side by side, every A fragment feeds two products
//   gemm_f16_conv3_vh_kernel  the k=3 convolution: one activation slab shared by the three taps, weight tiles double-buffered (counted vmcnt + raw barriers)
//   gemm_f16_wreg_kernel      one K segment, 128-row tiles, F32 / QKV outputs (the k = 1 in_layers convolution and the QKV projection at the benchmark's batch): waves 1 x 4,
//                             the WEIGHT operand never touches LDS — each wave loads its MFMA fragments from a fragment-major image built at load time, one K tile ahead;
//                             LDS is a two-slot ring of activation tiles, one raw barrier per K tile. Bit-identical to gemm_f16_vh_kernel. Measured against it in the benchmark
//                             (profiles/gemm_wreg_same_box_ab.txt): QKV projection 183.0 -> 170.9 us, in_layers 82.2 -> 73.6 us, headline +1.7 %. Adopted for both
//                             classes (option gemm_wreg); a two-tile distance is not instantiated (see the kernel).
//   gemm_f16_conv3_wreg_kernel the same move for the k = 3 convolution (F32 output with or without residual, 128-row tiles): per-tap fragment-major weight images, waves 1 x 4,
//                             weight register sets rotating per tap, LDS = a two-slot ring of activation SLABS (34 KB, 4 workgroups per CU), one raw barrier per 64-channel
//                             chunk. Bit-identical to gemm_f16_conv3_vh_kernel. The dual-B kernel is not ported.
//   gemm_f16_gn_panel_kernel  the k = 1 in_layers convolution of a ResBlock TOGETHER with the GroupNorm that consumes it: 512 threads own one sequence (<= 896 rows) x 64 output
//                             channels, so the f32 output never goes to memory (see the kernel). Not planned by gemm_plan: diffusion.hip launches it where
//                             gemm_gn_panel_takes admits the layout. Bit-identical to gemm_f16_wreg_kernel + gn_reg_kernel<512, 14>.
// gemm_plan picks between them and chooses h; launch_gemm_f16 launches what it says. Round 3 rewrote the kernels around two measurements
// (profiles/r3_gemm_tile_tables.txt, profiles/r3_gemm_epilogue.txt):
//  * tile-height / dispatch-order policies (tables of mixed heights, tallest-first, whole rounds filled exactly) change nothing:
//    a partially filled round runs proportionally faster, the launch is bound by total work, not by rounds;
//  * the 8-10 us "epilogue burst" of every tile was not HBM bandwidth but SIXTEEN SERIALISED memory round trips: a bias / guard /
//    residual load under a runtime `ptr ? load : 0` select is branched around by hipcc and waited for with vmcnt(0) — which also
//    waits for the previous block's stores (one in-order counter). Every epilogue load is now issued up front, unconditionally,
//    and the stores follow back to back.
// Measured and rejected (the sources are in git history): the one-tile kernels of round 2, and the 256-column 8-phase kernel of round 3 (one workgroup per CU, two
// wave groups in strict alternation — 94 vs 78 us on in_layers, 238 vs 204 on the QKV projection, per-phase timeline in profiles/r3_gemm_256col_kernel.txt). A 2-D XCD
// partition through explicit per-XCD tile tables (round 6, profiles/r6_gemm_xcd2d.txt) changed no launch time; the table path left the kernels with its probe.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace tts {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// GEMM_OUT_QKV_SPLIT: the QKV projection of the reference-precision AttentionBlock (option attn_f32): every f32 result x is stored as the
// fp16 pair hi = fp16(x), lo = fp16(x - hi) (hi + lo = x to 2^-22) in outH / outH2 and outVt / outVt2.
// GEMM_OUT_F32_SCALED: out = alpha * acc + bias + resid (split-precision operands whose weights were scaled by 1 / alpha at load).
// GEMM_OUT_F32_STATS / GEMM_OUT_F32_SCALED_STATS (round 6, option latency_mode): the f32 output + the GroupNorm statistics of the stored values, accumulated per
// (sequence, 32-channel group) in fixed point (fx_add) — the GroupNorm that consumes the output needs no reduction pass of its own (diffusion.hip: gn_apply_kernel).
enum { GEMM_OUT_F32 = 0, GEMM_OUT_F16 = 1, GEMM_OUT_QKV = 2, GEMM_OUT_QKV_SPLIT = 3, GEMM_OUT_F32_SCALED = 4, GEMM_OUT_F32_STATS = 5, GEMM_OUT_F32_SCALED_STATS = 6 };
constexpr bool gemm_mode_qkv(int mode) { return mode == GEMM_OUT_QKV || mode == GEMM_OUT_QKV_SPLIT; }
constexpr bool gemm_mode_f32(int mode) { return mode == GEMM_OUT_F32 || mode == GEMM_OUT_F32_SCALED || mode == GEMM_OUT_F32_STATS || mode == GEMM_OUT_F32_SCALED_STATS; }
constexpr bool gemm_mode_scaled(int mode) { return mode == GEMM_OUT_F32_SCALED || mode == GEMM_OUT_F32_SCALED_STATS; }
constexpr bool gemm_mode_stats(int mode) { return mode == GEMM_OUT_F32_STATS || mode == GEMM_OUT_F32_SCALED_STATS; }

struct GemmArgs {
  const __half *A[3];  // per segment base (row 0 of the packed layout)
  int row_off[3];
  int nseg, kseg;      // kseg % 64 == 0
  int lda;             // halves
  const __half *W;     // [N][ldw]; segment seg starts at column w_off[seg] (defaults: ldw = nseg*kseg, w_off = seg*kseg)
  int ldw_, w_off_[3], custom_w; // set custom_w = 1 to use ldw_/w_off_ (e.g. split-precision: hi|lo halves reused)
  const __half *Wf;    // the fragment-major image of W (one segment: gemm_wfrag_index; the k = 3 convolution: gemm_wfrag3_index), or nullptr
  int wreg;            // 1 with Wf: stream the weight through registers where gemm_f16_wreg_kernel / gemm_f16_conv3_wreg_kernel takes the shape
  int M, N;            // multiples of 128 (buffers are padded)
  const float *bias;   // [N] or nullptr
  const int *row_seq;  // [M]: sequence id, <0 for guard/padding rows (output forced to 0); may be null
  // GEMM_OUT_F32
  float *outF; int ldo; const float *resid; // resid may alias outF
  // GEMM_OUT_F16 (n_valid columns written) / GEMM_OUT_QKV
  __half *outH; int ldh;
  __half *outVt; int ldvt; // QKV: V channels transposed [h*64+d][row]
  __half *outH2, *outVt2;  // GEMM_OUT_QKV_SPLIT: the low halves (same leading dimensions)
  float alpha;             // GEMM_OUT_F32_SCALED
  long long *st_out;       // GEMM_OUT_*_STATS: [FX_STRIPES][st_stripe_ll]: per stripe [sequences][32 groups][4] fixed-point {sum hi, sum lo, sum of squares hi, lo}
  int st_stripe_ll;        //                   (fx_add), accumulated into; a workgroup adds to stripe blockIdx % FX_STRIPES, the reader sums the stripes (exact)
  const int *chunk_seq;    //                   [M / 8]: owning sequence of an aligned 8-row chunk (sequences start at multiples of 8 rows), -1 = guard rows only
  int dual_b;              // 1: the two segments are the hi / lo halves of ONE weight over ONE activation operand -> gemm_f16_vh_dualb_kernel (GEMM_OUT_F32_SCALED only)
  int mode;
  // tile walk, set by launch_gemm_f16 from gemm_plan: th = 16-row blocks per tile (0: chosen from the problem size), cn = column tiles per L2 chunk
  int th, cn;
  int ku; // K tiles per barrier pair of gemm_f16_vh_kernel (0 / 1: one; 2, 4: small problems, set by launch_gemm_f16 or a tool)
};


// LDS image of an operand tile: 128-byte rows (64 halves), the eight 16-byte chunks of row r stored at chunk ^ lds_swz(r). A ds_read_b128 is
// served in groups of 16 lanes = 16 CONSECUTIVE rows, eight of them reading chunk c (fq even) and eight chunk c + 1 (fq odd): the two sets differ in
// chunk bit 0, which the swizzle never touches, and inside a set the four rows of one parity have four different values of bits 1-2 — for ANY first
// row. (Round 2 xor-ed all three chunk bits with (row >> 1) & 7: conflict-free only for a first row that is a multiple of 4, i.e. not for the k = 3
// kernel's tap-shifted reads at rows +1 and +2: SQ_LDS_BANK_CONFLICT was 25 % of its LDS-active cycles, profiles/r3_pmc_lds.json.)
__device__ __forceinline__ int lds_swz(int row) { return ((row >> 1) & 3) << 1; }
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 128 + ((chunk ^ lds_swz(row)) << 4); }

// LDS stages are filled by direct global->LDS DMA (global_load_lds_dwordx4): no staging VGPRs, no ds_write pass.
// The LDS image of a DMA is lane-linear (base + lane*16), so the XOR swizzle is applied to the per-lane
// SOURCE address and again on the fragment read.
typedef const void __attribute__((address_space(1))) *gptr_t;
typedef void __attribute__((address_space(3))) *lptr_t;

// A wave of the 2 x 2 layout owns the 16-row blocks wm, wm + 2, wm + 4, wm + 6 of the tile (interleaved: a 7-block tile
// splits 4 / 3) and 64 columns: acc[i][j] = block wm + 2 i, columns wn * 64 + j * 16 ..
__device__ __forceinline__ int vh_blk(int wm, int i) { return wm + 2 * i; }

// low half of the split-precision pair of x: x - fp16(x), exact in f32, then rounded to fp16
__device__ __forceinline__ float split_lo(float x) { return x - __half2float(__float2half_rn(x)); }
__device__ __forceinline__ uint2 pack_half4(float a, float b, float c, float d) {
  const __half2 p0 = __floats2half2_rn(a, b), p1 = __floats2half2_rn(c, d);
  uint2 u;
  u.x = *(const unsigned *)&p0;
  u.y = *(const unsigned *)&p1;
  return u;
}

// Statistics accumulators are striped: one utterance sends ~440 atomics to each (sequence, group) record per GEMM, and same-line atomics are served one after the
// other by that line's L2 channel (~12 ns each: 5 us behind the kernel). 8 stripes and one set of atomics per wave instead of per chunk -> a dozen per line; the consumer adds the stripes (integers: still exact).
static constexpr int FX_STRIPES = 8;
// 128-bit fixed-point accumulation of an f32 partial sum: hi in units of 2^-8 (|p| < 2^55), the exact remainder in units of 2^-60. Integer addition is associative: the
// totals do not depend on the order in which workgroups arrive, and a per-chunk partial is computed by one wave in a fixed lane tree -> the statistics are reproducible
// run to run and independent of what else is in the batch.
__device__ __forceinline__ void fx_add(long long *dst, float p) {
  const float h = rintf(p * 256.0f);
  const float rem = p - h * (1.0f / 256.0f); // exact: |rem| <= 2^-9, or 0 when ulp(p) >= 2^-8
  atomicAdd((unsigned long long *)dst, (unsigned long long)(long long)h);
  atomicAdd((unsigned long long *)dst + 1, (unsigned long long)(long long)rintf(rem * 4503599627370496.0f)); // 2^52
}
__device__ __forceinline__ void fx_split(float p, long long &hi, long long &lo) {
  const float h = rintf(p * 256.0f);
  hi = (long long)h;
  lo = (long long)rintf((p - h * (1.0f / 256.0f)) * 4503599627370496.0f);
}
__host__ __device__ __forceinline__ double fx_value(long long hi, long long lo) { return (double)hi * (1.0 / 256.0) + (double)lo * (1.0 / 1152921504606846976.0); }
template <int CTRL> __device__ __forceinline__ float gemm_dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
// sum over the lanes that differ in bits 0-2 and 4-5 (the 8 rows of a half block x the 4 column quads of a swapped-order 16x16 accumulator): lanes 0 and 8 of the wave end
// up with the totals of rows 0-7 / 8-15 of the block. Fixed tree.
__device__ __forceinline__ float red_half_block(float x) {
  x += gemm_dpp<0xB1>(x);  // quad_perm [1,0,3,2]: lane ^ 1
  x += gemm_dpp<0x4E>(x);  // quad_perm [2,3,0,1]: lane ^ 2
  x += gemm_dpp<0x141>(x); // row_half_mirror: quads are uniform now, 7 - l swaps the two quads of a half row: lane ^ 4
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// Epilogues. For F32/F16 outputs the MFMA operands are swapped (A-operand = weight rows, B-operand =
// activation rows), so a lane's 4 accumulator registers are 4 CONSECUTIVE output columns of one row:
// residual loads and stores are 16 bytes per lane instead of 4. The V columns of the QKV mode keep the natural order
// (a lane holds 4 consecutive rows of one column) because V is stored transposed.
// EVERY load (bias, guard flags, residual) is issued before the first store, inside at most one wave-uniform branch per
// operand kind: a load under a per-element `ptr ? .. : ..` select costs a vmcnt(0) round trip per element AND drains the stores
// issued before it (see the header of this file).
enum { EPI_NO_RESID = 0, EPI_RESID_IN_ACC = 1, EPI_RESID_LOAD = 2 };
template <int MODE, int MI, int RESID>
__device__ __forceinline__ void gemm_epilogue_vh(const GemmArgs &g, floatx4 (&acc)[MI > 0 ? MI : 1][4], int m0, int n0, int wm, int wn, int fr, int fq) {
  constexpr int MA = MI > 0 ? MI : 1;
  if (MI == 0) return;
  if (gemm_mode_qkv(MODE)) {
    // col = h*192 + {q 0..63 | k 64..127 | v 128..191}; a wave's 64-column span is entirely q, k or v.
    const int c0 = n0 + wn * 64, h = c0 / 192, w0 = c0 - h * 192;
    if (w0 >= 128) { // V, natural operand order: lane = 4 consecutive rows of one column -> 8-byte transposed store
      // unconditional loads + selects (a null pointer reads a valid dummy address and the value is dropped): ONE round trip
      const bool hb = g.bias != nullptr, hs = g.row_seq != nullptr;
      const float *bp = hb ? g.bias : (const float *)g.W;   // W holds >= 128 N bytes
      const int *sp = hs ? g.row_seq : (const int *)g.A[0]; // A holds >= 128 M bytes
      float bv[4];
      int4 sq[MA];
#pragma unroll
      for (int j = 0; j < 4; j++) bv[j] = bp[c0 + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < MI; i++) sq[i] = *(const int4 *)(sp + m0 + vh_blk(wm, i) * 16 + fq * 4);
#pragma unroll
      for (int j = 0; j < 4; j++) bv[j] = hb ? bv[j] : 0.f;
#pragma unroll
      for (int i = 0; i < MI; i++) sq[i] = hs ? sq[i] : make_int4(0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < MI; i++) {
        const int rbase = m0 + vh_blk(wm, i) * 16 + fq * 4;
        const bool gd[4] = {sq[i].x < 0, sq[i].y < 0, sq[i].z < 0, sq[i].w < 0};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; r++) v[r] = gd[r] ? 0.f : acc[i][j][r] + bv[j];
          *(uint2 *)(g.outVt + (size_t)(h * 64 + j * 16 + fr) * g.ldvt + rbase) = pack_half4(v[0], v[1], v[2], v[3]);
          if (MODE == GEMM_OUT_QKV_SPLIT)
            *(uint2 *)(g.outVt2 + (size_t)(h * 64 + j * 16 + fr) * g.ldvt + rbase) = pack_half4(split_lo(v[0]), split_lo(v[1]), split_lo(v[2]), split_lo(v[3]));
        }
      }
      return;
    }
  }
  // swapped operand order: acc[i][j][r] = C[m0 + blk(i)*16 + fr][n0 + wn*64 + j*16 + fq*4 + r]
  const int col0 = n0 + wn * 64 + fq * 4;
  const bool hb = g.bias != nullptr, hs = g.row_seq != nullptr;
  const float *bp = hb ? g.bias : (const float *)g.W;   // see above: unconditional loads, values selected afterwards
  const int *sp = hs ? g.row_seq : (const int *)g.A[0];
  float4 b4[4];
  int sq[MA];
  float4 rr[2][4]; // RESID == EPI_RESID_LOAD: residual of a pair of blocks
  auto load_pair = [&](int p) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int i = min(2 * p + q, MI - 1); // odd MI: the last pair re-reads its first block (never used)
      const float *rp = g.resid + (size_t)(m0 + vh_blk(wm, i) * 16 + fr) * g.ldo + col0;
#pragma unroll
      for (int j = 0; j < 4; j++) rr[q][j] = *(const float4 *)(rp + j * 16);
    }
  };
  if (RESID == EPI_RESID_LOAD) load_pair(0); // the HBM reads first, bias and guards (L2 hits) behind them: one round trip
#pragma unroll
  for (int j = 0; j < 4; j++) b4[j] = *(const float4 *)(bp + col0 + j * 16);
#pragma unroll
  for (int i = 0; i < MI; i++) sq[i] = sp[m0 + vh_blk(wm, i) * 16 + fr];
#pragma unroll
  for (int j = 0; j < 4; j++) b4[j] = hb ? b4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < MI; i++) sq[i] = hs ? sq[i] : 0;
  auto finish = [&](int i, int j) { // bias, guard
    if (gemm_mode_scaled(MODE)) acc[i][j] *= g.alpha;
    float4 v = make_float4(acc[i][j][0] + b4[j].x, acc[i][j][1] + b4[j].y, acc[i][j][2] + b4[j].z, acc[i][j][3] + b4[j].w);
    if (sq[i] < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);
    return v;
  };
  if (gemm_mode_f32(MODE)) {
    // GroupNorm statistics of the stored values (GEMM_OUT_*_STATS): a lane's partial sums over its 2 x 4 values of a (block, 32-column group), reduced over the 8 rows of
    // each half block after the stores
    float ssum[MA][2], ssq[MA][2];
    auto stat_add = [&](int i, int j, const float4 &v) {
      const float a = (v.x + v.y) + (v.z + v.w), b = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
      if (j & 1) { ssum[i][j >> 1] += a; ssq[i][j >> 1] += b; }
      else { ssum[i][j >> 1] = a; ssq[i][j >> 1] = b; }
    };
    auto stat_flush = [&]() {
      // Every 8-row chunk's partial is converted to fixed point on its own (lanes 0 and 8 of the wave) — the unit whose value does not depend on the tiling — and
      // the integers of a lane's chunks that belong to one sequence are added up before the atomics: 4 atomics per lane and group instead of 4 per chunk.
      const int lane = fq * 16 + fr;
      int cs[MA];
#pragma unroll
      for (int i = 0; i < MI; i++) cs[i] = g.chunk_seq[((m0 + vh_blk(wm, i) * 16) >> 3) + (fr >> 3)];
#pragma unroll
      for (int jp = 0; jp < 2; jp++) {
        long long tot[4] = {0, 0, 0, 0};
        int tseq = -1;
        auto flush = [&]() {
          if (tseq >= 0) {
            long long *dst = g.st_out + (size_t)(blockIdx.x % FX_STRIPES) * g.st_stripe_ll + (size_t)(tseq * 32 + ((n0 + wn * 64) >> 5) + jp) * 4;
#pragma unroll
            for (int k = 0; k < 4; k++) atomicAdd((unsigned long long *)dst + k, (unsigned long long)tot[k]);
          }
        };
#pragma unroll
        for (int i = 0; i < MI; i++) { // lane 0 adds up the upper halves (rows 0-7) of the wave's blocks, lane 8 the lower ones
          const float sv = red_half_block(ssum[i][jp]), qv = red_half_block(ssq[i][jp]);
          if ((lane & 0x37) == 0 && cs[i] >= 0) {
            long long f[4];
            fx_split(sv, f[0], f[1]);
            fx_split(qv, f[2], f[3]);
            if (cs[i] != tseq) { flush(); tseq = cs[i]; tot[0] = tot[1] = tot[2] = tot[3] = 0; }
#pragma unroll
            for (int k = 0; k < 4; k++) tot[k] += f[k];
          }
        }
        if ((lane & 0x37) == 0) flush();
      }
    };
    if (RESID == EPI_RESID_LOAD) {
      // residual read here (k = 3 kernel): blocks in pairs, the next pair's 8 loads are in flight while this pair is stored
      constexpr int NP = (MI + 1) / 2;
#pragma unroll
      for (int p = 0; p < NP; p++) {
        float4 v[2][4];
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const int i = 2 * p + q;
          if (i < MI) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
              // same f32 adds in the same order as before: (acc + bias) + resid
              if (gemm_mode_scaled(MODE)) acc[i][j] *= g.alpha;
              float4 t = make_float4(acc[i][j][0] + b4[j].x, acc[i][j][1] + b4[j].y, acc[i][j][2] + b4[j].z, acc[i][j][3] + b4[j].w);
              t.x += rr[q][j].x; t.y += rr[q][j].y; t.z += rr[q][j].z; t.w += rr[q][j].w;
              if (sq[i] < 0) t = make_float4(0.f, 0.f, 0.f, 0.f);
              v[q][j] = t;
              if (gemm_mode_stats(MODE)) stat_add(i, j, t);
            }
          }
        }
        if (p + 1 < NP) load_pair(p + 1);
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const int i = 2 * p + q;
          if (i < MI) {
            float *op = g.outF + (size_t)(m0 + vh_blk(wm, i) * 16 + fr) * g.ldo + col0;
#pragma unroll
            for (int j = 0; j < 4; j++) *(float4 *)(op + j * 16) = v[q][j];
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < MI; i++) {
        float *op = g.outF + (size_t)(m0 + vh_blk(wm, i) * 16 + fr) * g.ldo + col0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float4 v = finish(i, j);
          *(float4 *)(op + j * 16) = v;
          if (gemm_mode_stats(MODE)) stat_add(i, j, v);
        }
      }
    }
    if (gemm_mode_stats(MODE)) stat_flush();
  } else if (MODE == GEMM_OUT_F16) {
#pragma unroll
    for (int i = 0; i < MI; i++) {
      __half *op = g.outH + (size_t)(m0 + vh_blk(wm, i) * 16 + fr) * g.ldh + col0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float4 v = finish(i, j);
        *(uint2 *)(op + j * 16) = pack_half4(v.x, v.y, v.z, v.w);
      }
    }
  } else { // Q or K columns of the QKV projection
    const int c0 = n0 + wn * 64, h = c0 / 192, w0 = c0 - h * 192;
#pragma unroll
    for (int i = 0; i < MI; i++) {
      __half *op = g.outH + (size_t)(m0 + vh_blk(wm, i) * 16 + fr) * g.ldh + h * 128 + w0 + fq * 4;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float4 v = finish(i, j);
        *(uint2 *)(op + j * 16) = pack_half4(v.x, v.y, v.z, v.w);
        if (MODE == GEMM_OUT_QKV_SPLIT)
          *(uint2 *)(g.outH2 + (op - g.outH) + j * 16) = pack_half4(split_lo(v.x), split_lo(v.y), split_lo(v.z), split_lo(v.w));
      }
    }
  }
}

// Pieces every kernel shares.
// Offset (halves) of a lane's 16 bytes of the 8-row DMA piece `piece` of an operand tile: 8 lanes per row, the chunk swizzled by the LDS row. The source row is
// first + min(row, clamp): the k = 3 and the register-streamed kernel clamp rows past their operand into it (duplicates that are never multiplied / stored).
__device__ __forceinline__ int gemm_dma_off(int piece, int lane, int first, int clamp, int ld) {
  const int row = piece * 8 + (lane >> 3);
  return (first + min(row, clamp)) * ld + ((lane & 7) ^ lds_swz(row)) * 8;
}
static constexpr int GEMM_NO_CLAMP = 0x7fffffff;
// Accumulators START from the residual (F32 outputs, swapped operand order: acc[i][j] = 4 consecutive columns of one row): the
// residual read is issued with the first operand tile and hides behind it, instead of being a dependent HBM round trip in front
// of the stores when the K loop is over. The sum is the same set of f32 adds in a different order.
// GEMM_OUT_F32_SCALED (out = alpha acc + bias + resid, alpha a power of two): the accumulators start from resid / alpha — exact, and scaled back
// exactly by the epilogue.
// NB 16-column blocks from column c0, the lane holds columns 4 fq .. of each; row_of(i) = the lane's row of block i.
template <int MODE, int MI, int NB, class ROW>
__device__ __forceinline__ void gemm_acc_start(const GemmArgs &g, floatx4 (&acc)[MI > 0 ? MI : 1][NB], bool resid_first, int c0, int fq, ROW row_of) {
  if (resid_first) {
    const float rs = gemm_mode_scaled(MODE) ? 1.0f / g.alpha : 1.0f;
#pragma unroll
    for (int i = 0; i < MI; i++) {
      const int row = row_of(i);
#pragma unroll
      for (int j = 0; j < NB; j++) {
        const float4 rr = *(const float4 *)(g.resid + (size_t)row * g.ldo + c0 + j * 16 + fq * 4);
        acc[i][j] = (floatx4){rr.x * rs, rr.y * rs, rr.z * rs, rr.w * rs};
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
      for (int j = 0; j < NB; j++) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
  }
}
// The body of a 2 x 2 kernel is instantiated per number of 16-row blocks of the calling WAVE (0..4): the waves of a workgroup may run different
// instantiations; all of them issue the same DMA pieces and pass the same barriers. f(std::integral_constant<int, blocks of this wave>)
template <class F> __device__ __forceinline__ void gemm_for_my_mi(int nblk, int wave, F f) {
  const int my_mi = (nblk - (wave >> 1) + 1) >> 1;
  if (my_mi == 4) f(std::integral_constant<int, 4>{});
  else if (my_mi == 3) f(std::integral_constant<int, 3>{});
  else if (my_mi == 2) f(std::integral_constant<int, 2>{});
  else if (my_mi == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 0>{}); // 1-block tile: this wave only moves operands
}

// Any segment structure (k = 1 convolutions, projections, channel concats, split-precision operands): one 32 KB LDS stage filled by
// LDS-DMA, 4 workgroups per CU overlap each other's load / compute phases.
// Two barriers per K tile. KU (round 6): K tiles per barrier pair. KU = 2 stages two 64-deep tiles side by side (64 KB, 2 workgroups per CU) and multiplies them between ONE pair of barriers: a
// small problem (one utterance: at most two workgroups per CU) pays a DMA round trip + two barriers per pair instead of per tile. Same products in the same order:
// bit-identical to KU = 1.
template <int MODE, int MI, int KU = 1>
__device__ __forceinline__ void gemm_vh_body(const GemmArgs &g, int m0, int n0, int nblk, int lane, int wave) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[]; // named here: an LDS pointer passed in would become a generic pointer
  char *smem = smem_dyn;
  constexpr int MA = MI > 0 ? MI : 1;
  const int wm = wave >> 1, wn = wave & 1;
  const int my_pa = (2 * nblk - wave + 3) >> 2; // 8-row DMA pieces wave, wave + 4, .. of the A tile moved by this wave
  const int tiles_per_seg = g.kseg >> 6;
  const int ldw = g.custom_w ? g.ldw_ : g.nseg * g.kseg;
  int aoff[4], boff[4];
#pragma unroll
  for (int i = 0; i < 4; i++) aoff[i] = gemm_dma_off(wave + 4 * i, lane, m0, GEMM_NO_CLAMP, g.lda);
#pragma unroll
  for (int i = 0; i < 4; i++) boff[i] = gemm_dma_off(wave * 4 + i, lane, n0, GEMM_NO_CLAMP, ldw);
  const int fr = lane & 15, fq = lane >> 4;
  const bool resid_first = gemm_mode_f32(MODE) && g.resid != nullptr;
  floatx4 acc[MA][4];
  gemm_acc_start<MODE, MI, 4>(g, acc, resid_first, n0 + wn * 64, fq, [&](int i) { return m0 + vh_blk(wm, i) * 16 + fr; });
  char *sa = smem, *sb = smem + 16384;
  // operand order (see gemm_epilogue_vh): natural only for the V columns of a QKV projection (wave-uniform)
  const bool natural = gemm_mode_qkv(MODE) && (((n0 + wn * 64) % 192) >= 128);
  // the K loop is instantiated once per operand order so the choice costs nothing inside it
  auto kloop = [&](auto nat) {
    constexpr bool NAT = decltype(nat)::value;
    // segment loop outside, K tiles inside: the segment's base pointers are fetched from the kernel arguments once
    for (int seg = 0; seg < g.nseg; seg++) {
      const __half *aseg = g.A[seg] + (ptrdiff_t)g.row_off[seg] * g.lda;
      const __half *wseg = g.W + (g.custom_w ? g.w_off_[seg] : seg * g.kseg);
      for (int kt = 0; kt < tiles_per_seg; kt += KU) { // kseg % (64 KU) == 0 (checked by the launcher)
#pragma unroll
        for (int u = 0; u < KU; u++) {
          const __half *abase = aseg + ((kt + u) << 6), *wbase = wseg + ((kt + u) << 6);
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (i < my_pa) __builtin_amdgcn_global_load_lds((gptr_t)(abase + aoff[i]), (lptr_t)(sa + u * 32768 + (wave + 4 * i) * 1024), 16, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; i++)
            __builtin_amdgcn_global_load_lds((gptr_t)(wbase + boff[i]), (lptr_t)(sb + u * 32768 + (wave * 4 + i) * 1024), 16, 0, 0);
        }
        __syncthreads(); // waits vmcnt(0) for the DMA, then barrier
#pragma unroll
        for (int ks = 0; ks < 2 * KU; ks++) {
          const char *sau = sa + (ks >> 1) * 32768, *sbu = sb + (ks >> 1) * 32768;
          half8 af[MA], bf[4];
#pragma unroll
          for (int i = 0; i < MI; i++) af[i] = *(const half8 *)(sau + lds_off(vh_blk(wm, i) * 16 + fr, (ks & 1) * 4 + fq));
          if (MI > 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) bf[i] = *(const half8 *)(sbu + lds_off(wn * 64 + i * 16 + fr, (ks & 1) * 4 + fq));
          }
#pragma unroll
          for (int i = 0; i < MI; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
              if (NAT) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
              else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
      }
    }
  };
  if (gemm_mode_qkv(MODE) && natural) kloop(std::true_type{});
  else kloop(std::false_type{});
  if (resid_first) gemm_epilogue_vh<MODE, MI, EPI_RESID_IN_ACC>(g, acc, m0, n0, wm, wn, fr, fq);
  else gemm_epilogue_vh<MODE, MI, EPI_NO_RESID>(g, acc, m0, n0, wm, wn, fr, fq);
}

// Split-precision WEIGHT, one activation operand (round 5: proj_out of the default AttentionBlock, out = A (W_hi + W_lo)^T): the two weight tiles of a K
// tile are staged side by side (16 KB A + 2 x 16 KB B = 48 KB, 3 workgroups per CU) and every A fragment read from LDS feeds both products — against two
// K segments through gemm_vh_body: 48 instead of 64 KB of DMA, 24 instead of 32 KB of fragment reads and 2 instead of 4 barriers per 64 MFMAs.
// g.W = [N][ldw_] with the hi half at column w_off_[0] and the lo half at w_off_[1] (custom_w); g.nseg == 2, g.A[0] == g.A[1], equal row offsets.
// Kept apart from gemm_vh_body: one body templated on the number of weight images cost 5 (KU 1) / 8 (KU 2) VGPRs in gemm_f16_vh_dualb_kernel<4, *>, and gemm_acc_start
// here 2 in the same two instantiations (profiles/gemm_refactor_isa.txt).
static constexpr int GEMM_DUALB_LDS = 49152;
template <int MODE, int MI, int KU = 1>
__device__ __forceinline__ void gemm_vh_dualb_body(const GemmArgs &g, int m0, int n0, int nblk, int lane, int wave) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  char *smem = smem_dyn;
  constexpr int MA = MI > 0 ? MI : 1;
  const int wm = wave >> 1, wn = wave & 1;
  const int my_pa = (2 * nblk - wave + 3) >> 2;
  const int ntiles = g.kseg >> 6, ldw = g.ldw_;
  int aoff[4], boff[4];
#pragma unroll
  for (int i = 0; i < 4; i++) aoff[i] = gemm_dma_off(wave + 4 * i, lane, m0, GEMM_NO_CLAMP, g.lda);
#pragma unroll
  for (int i = 0; i < 4; i++) boff[i] = gemm_dma_off(wave * 4 + i, lane, n0, GEMM_NO_CLAMP, ldw);
  const int fr = lane & 15, fq = lane >> 4;
  const bool resid_first = gemm_mode_f32(MODE) && g.resid != nullptr;
  floatx4 acc[MA][4];
  if (resid_first) {
    const float rs = gemm_mode_scaled(MODE) ? 1.0f / g.alpha : 1.0f;
#pragma unroll
    for (int i = 0; i < MI; i++) {
      const int row = m0 + vh_blk(wm, i) * 16 + fr;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float4 rr = *(const float4 *)(g.resid + (size_t)row * g.ldo + n0 + wn * 64 + j * 16 + fq * 4);
        acc[i][j] = (floatx4){rr.x * rs, rr.y * rs, rr.z * rs, rr.w * rs};
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
  }
  char *sa = smem, *sb0 = smem + 16384, *sb1 = smem + 32768;
  const __half *aseg = g.A[0] + (ptrdiff_t)g.row_off[0] * g.lda;
  const __half *w0 = g.W + g.w_off_[0], *w1 = g.W + g.w_off_[1];
  for (int kt = 0; kt < ntiles; kt += KU) { // KU K tiles per barrier pair (see gemm_vh_body): 48 KB of LDS each
#pragma unroll
    for (int u = 0; u < KU; u++) {
      const __half *abase = aseg + ((kt + u) << 6), *b0 = w0 + ((kt + u) << 6), *b1 = w1 + ((kt + u) << 6);
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (i < my_pa) __builtin_amdgcn_global_load_lds((gptr_t)(abase + aoff[i]), (lptr_t)(sa + u * GEMM_DUALB_LDS + (wave + 4 * i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; i++) __builtin_amdgcn_global_load_lds((gptr_t)(b0 + boff[i]), (lptr_t)(sb0 + u * GEMM_DUALB_LDS + (wave * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; i++) __builtin_amdgcn_global_load_lds((gptr_t)(b1 + boff[i]), (lptr_t)(sb1 + u * GEMM_DUALB_LDS + (wave * 4 + i) * 1024), 16, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2 * KU; ks++) {
      const int uo = (ks >> 1) * GEMM_DUALB_LDS, kk = ks & 1;
      half8 af[MA], bf[4], bl[4];
#pragma unroll
      for (int i = 0; i < MI; i++) af[i] = *(const half8 *)(sa + uo + lds_off(vh_blk(wm, i) * 16 + fr, kk * 4 + fq));
      if (MI > 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) bf[i] = *(const half8 *)(sb0 + uo + lds_off(wn * 64 + i * 16 + fr, kk * 4 + fq));
#pragma unroll
        for (int i = 0; i < 4; i++) bl[i] = *(const half8 *)(sb1 + uo + lds_off(wn * 64 + i * 16 + fr, kk * 4 + fq));
      }
#pragma unroll
      for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[j], af[i], acc[i][j], 0, 0, 0); // the small term first
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
  }
  if (resid_first) gemm_epilogue_vh<MODE, MI, EPI_RESID_IN_ACC>(g, acc, m0, n0, wm, wn, fr, fq);
  else gemm_epilogue_vh<MODE, MI, EPI_NO_RESID>(g, acc, m0, n0, wm, wn, fr, fq);
}

// Tile walk, shared by both kernels. L2-aware: workgroup b runs on XCD b % 8 (each XCD has its own 4 MB L2). An XCD owns a
// contiguous range of 16-row blocks, cut into tiles of g.th blocks (the last one shorter), and walks them once per chunk of g.cn
// column tiles, chunk outermost: the chunk's weight rows (cn * 128 * K * 2 B <= ~2.5 MB) stay L2-resident while the activations
// stream through. (With plain m-major order the 6 MB QKV weight thrashed L2: 417 MB fetched per launch for 64 MB of operands.)
__device__ __forceinline__ bool gemm_vh_tile(const GemmArgs &g, int &m0, int &n0, int &nblk) {
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int nb = g.M >> 4, NT = g.N >> 7;
  const int b0 = (int)((long long)nb * xcd >> 3), b1 = (int)((long long)nb * (xcd + 1) >> 3);
  const int mt = (b1 - b0 + g.th - 1) / g.th;
  if (idx >= mt * NT) return false; // grid is padded to 8 * max tiles per XCD
  const int per_chunk = mt * g.cn, chunk = idx / per_chunk, rem = idx - chunk * per_chunk;
  const int t = rem / g.cn, blk0 = b0 + t * g.th;
  m0 = blk0 << 4;
  nblk = min(g.th, b1 - blk0);
  n0 = (chunk * g.cn + rem - t * g.cn) << 7;
  return true;
}

static constexpr int GEMM_VH_LDS = 32768;
template <int MODE, int WGS, int KU = 1>
static __global__ __launch_bounds__(256, WGS) void gemm_f16_vh_kernel(GemmArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6); // scalar: LDS-DMA bases stay in SGPRs
  int m0, n0, nblk;
  if (!gemm_vh_tile(g, m0, n0, nblk)) return;
  gemm_for_my_mi(nblk, wave, [&](auto mi) { gemm_vh_body<MODE, decltype(mi)::value, KU>(g, m0, n0, nblk, lane, wave); });
}

template <int MODE, int KU = 1>
static __global__ __launch_bounds__(256, KU == 1 ? 3 : 1) void gemm_f16_vh_dualb_kernel(GemmArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int m0, n0, nblk;
  if (!gemm_vh_tile(g, m0, n0, nblk)) return;
  gemm_for_my_mi(nblk, wave, [&](auto mi) { gemm_vh_dualb_body<MODE, decltype(mi)::value, KU>(g, m0, n0, nblk, lane, wave); });
}

// Weight operand through REGISTERS (gemm_f16_wreg_kernel; one K segment, 128-row tiles, F32 / QKV outputs). The weight is constant from load time on, so the loader
// stores a second, fragment-major image of it:
//   Wf[n / 16][k / 32][lane = ((k % 32) / 8) * 16 + n % 16][k % 8]
// = the 8 halves lane (fr, fq) of a v_mfma_f32_16x16x32_f16 weight fragment holds, W[n0 + fr][k0 + 8 fq ..] — the same register contents in the swapped and in the
// natural operand order — so one fragment is one fully coalesced 1 KB global_load_dwordx4 per wave and never touches LDS. The four waves lie 1 x 4 along N: wave w owns
// all rows of the tile x columns 32 w .. 32 w + 31, no weight fragment is fetched twice. LDS holds only activation tiles, as a ring of D + 1 slots of 16 KB filled by
// LDS-DMA D K tiles ahead; the weight fragments of those D tiles wait in registers (16 per tile). ONE raw barrier per K tile:
//   wait (counted vmcnt) for tile t  ->  barrier (every wave has also left tile t - 1)  ->  request tile t + D into the slot / registers of tile t - 1  ->  multiply tile t.
// vmcnt is one in-order counter for the DMA pieces and the register loads: a wave issues exactly MI / 2 + 4 of them per K tile (DMA rows past a short tile are clamped,
// not skipped), so "all but the youngest D - 1 tiles" is one immediate. The register loads are inline asm: beside an LDS-DMA in flight hipcc waits vmcnt(0) for every
// ordinary VGPR-destination load; their destinations are named by the wait statement ("+v") so that no consumer is scheduled above it.
// Every accumulator adds the same products in the same K order through the same instruction and operand order as gemm_vh_body: bit-identical outputs.
static inline size_t gemm_wfrag_index(int n, int k, int K) { // index (in halves) of W[n][k] in the fragment-major image
  return ((((size_t)(n >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k >> 3) & 3) * 16 + (n & 15)) << 3) + (k & 7);
}

// wave-uniform base (SGPR pair) + the lane's 32-bit byte offset: no 64-bit address registers
template <int OFF> __device__ __forceinline__ void wreg_load(half8 &d, const __half *base, unsigned voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(d) : "v"(voff), "s"(base), "i"(OFF));
}
template <int N> __device__ __forceinline__ void wreg_wait(half8 &a, half8 &b, half8 &c, half8 &d) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "i"(N) : "memory");
}

// acc[i][j]: 16-row block i of the tile, columns n0 + 32 wave + 16 j ..; only blocks i < nblk are stored
// Kept apart from gemm_epilogue_vh: one epilogue templated on the wave's part of the tile left this kernel at 126 VGPRs and every object built with
// -amdgpu-mfma-vgpr-form unchanged, but cost 4 VGPRs in gemm_f16_vh_kernel<2, 1, 4> (160 -> 164) and 12 in <3, 1, 4> (164 -> 176) as ar.o and vocoder.o compile them
template <int MODE, int MI, bool NAT>
__device__ __forceinline__ void gemm_epilogue_wreg(const GemmArgs &g, floatx4 (&acc)[MI][2], int m0, int n0, int nblk, int wave, int fr, int fq) {
  const int c0 = n0 + wave * 32;
  const bool hb = g.bias != nullptr, hs = g.row_seq != nullptr;
  const float *bp = hb ? g.bias : (const float *)g.W;   // unconditional loads, values selected afterwards (see gemm_epilogue_vh)
  const int *sp = hs ? g.row_seq : (const int *)g.A[0];
  if (NAT) {
    const int h = c0 / 192, w0 = c0 - h * 192;
    { // V, natural operand order: acc[i][j][r] = C[m0 + 16 i + 4 fq + r][c0 + 16 j + fr]
      float bv[2];
      int4 sq[MI];
#pragma unroll
      for (int j = 0; j < 2; j++) bv[j] = bp[c0 + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < MI; i++) sq[i] = *(const int4 *)(sp + m0 + min(i, nblk - 1) * 16 + fq * 4);
#pragma unroll
      for (int j = 0; j < 2; j++) bv[j] = hb ? bv[j] : 0.f;
#pragma unroll
      for (int i = 0; i < MI; i++) sq[i] = hs ? sq[i] : make_int4(0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < MI; i++) {
        if (i < nblk) {
          const int rbase = m0 + i * 16 + fq * 4;
          const bool gd[4] = {sq[i].x < 0, sq[i].y < 0, sq[i].z < 0, sq[i].w < 0};
#pragma unroll
          for (int j = 0; j < 2; j++) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = gd[r] ? 0.f : acc[i][j][r] + bv[j];
            const size_t o = (size_t)(h * 64 + (w0 - 128) + j * 16 + fr) * g.ldvt + rbase;
            *(uint2 *)(g.outVt + o) = pack_half4(v[0], v[1], v[2], v[3]);
            if (MODE == GEMM_OUT_QKV_SPLIT) *(uint2 *)(g.outVt2 + o) = pack_half4(split_lo(v[0]), split_lo(v[1]), split_lo(v[2]), split_lo(v[3]));
          }
        }
      }
      return;
    }
  }
  // swapped operand order: acc[i][j][r] = C[m0 + 16 i + fr][c0 + 16 j + 4 fq + r]
  const int col0 = c0 + fq * 4;
  float4 b4[2];
  int sq[MI];
#pragma unroll
  for (int j = 0; j < 2; j++) b4[j] = *(const float4 *)(bp + col0 + j * 16);
#pragma unroll
  for (int i = 0; i < MI; i++) sq[i] = sp[m0 + min(i, nblk - 1) * 16 + fr];
#pragma unroll
  for (int j = 0; j < 2; j++) b4[j] = hb ? b4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < MI; i++) sq[i] = hs ? sq[i] : 0;
  auto finish = [&](int i, int j) { // bias, guard: the adds of gemm_epilogue_vh
    float4 v = make_float4(acc[i][j][0] + b4[j].x, acc[i][j][1] + b4[j].y, acc[i][j][2] + b4[j].z, acc[i][j][3] + b4[j].w);
    if (sq[i] < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);
    return v;
  };
  if (MODE == GEMM_OUT_F32) {
#pragma unroll
    for (int i = 0; i < MI; i++) {
      if (i < nblk) {
        float *op = g.outF + (size_t)(m0 + i * 16 + fr) * g.ldo + col0;
#pragma unroll
        for (int j = 0; j < 2; j++) *(float4 *)(op + j * 16) = finish(i, j);
      }
    }
  } else { // Q or K columns of the QKV projection
    const int h = c0 / 192, w0 = c0 - h * 192;
#pragma unroll
    for (int i = 0; i < MI; i++) {
      if (i < nblk) {
        __half *op = g.outH + (size_t)(m0 + i * 16 + fr) * g.ldh + h * 128 + w0 + fq * 4;
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const float4 v = finish(i, j);
          *(uint2 *)(op + j * 16) = pack_half4(v.x, v.y, v.z, v.w);
          if (MODE == GEMM_OUT_QKV_SPLIT)
            *(uint2 *)(g.outH2 + (op - g.outH) + j * 16) = pack_half4(split_lo(v.x), split_lo(v.y), split_lo(v.z), split_lo(v.w));
        }
      }
    }
  }
}

// NAT: this wave's columns are V columns of a QKV projection (natural operand order). A template parameter of the whole body, not of the K loop alone: with two K loops in one
// function hipcc spills the weight registers inside both (seen in the ISA)
template <int MODE, int MI, int D, bool NAT>
__device__ __forceinline__ void gemm_wreg_body(const GemmArgs &g, int m0, int n0, int nblk, int lane, int wave) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[]; // ONE LDS object (see gemm_vh_body)
  char *smem = smem_dyn;
  constexpr int S = D + 1;            // ring slots = weight register sets
  constexpr int NPA = MI / 2;         // DMA pieces (8 rows) per wave and K tile
  constexpr int PER = NPA + 4;        // vmcnt events per wave and K tile
  static_assert(D == 1 || D == 2, "prefetch distance");
  const int T = g.kseg >> 6, KS = g.kseg >> 5;
  const int fr = lane & 15, fq = lane >> 4;
  unsigned aoff[NPA]; // byte offsets from a wave-uniform base: the DMA takes the SGPR-base addressing form
#pragma unroll
  for (int i = 0; i < NPA; i++) aoff[i] = (unsigned)(gemm_dma_off(wave + 4 * i, lane, 0, nblk * 16 - 1, g.lda) * 2);
  const char *aseg = (const char *)(g.A[0] + (ptrdiff_t)(g.row_off[0] + m0) * g.lda);
  const __half *wp0 = g.Wf + (size_t)((n0 >> 4) + wave * 2) * KS * 512, *wp1 = wp0 + (size_t)KS * 512; // wave-uniform
  const unsigned wlane = lane * 16;
  const bool resid_first = MODE == GEMM_OUT_F32 && g.resid != nullptr;
  floatx4 acc[MI][2];
  gemm_acc_start<MODE, MI, 2>(g, acc, resid_first, n0 + wave * 32, fq, [&](int i) { return m0 + min(i, nblk - 1) * 16 + fr; });
  half8 w[S][2][2]; // [set][k step][column block]
  auto issue = [&](int t, auto set_c) {
    constexpr int U = decltype(set_c)::value;
    const char *ab = aseg + (t << 7);
#pragma unroll
    for (int i = 0; i < NPA; i++) __builtin_amdgcn_global_load_lds((gptr_t)(ab + aoff[i]), (lptr_t)(smem + U * 16384 + (wave + 4 * i) * 1024), 16, 0, 0);
    const __half *q0 = wp0 + (size_t)t * 1024, *q1 = wp1 + (size_t)t * 1024;
    wreg_load<0>(w[U][0][0], q0, wlane);
    wreg_load<0>(w[U][0][1], q1, wlane);
    wreg_load<1024>(w[U][1][0], q0, wlane);
    wreg_load<1024>(w[U][1][1], q1, wlane);
  };
  auto kloop = [&]() {
    auto step = [&](int t, auto u_c) {
      constexpr int U = decltype(u_c)::value;
      // tile t has landed: everything but the younger tiles already requested (t + 1 .. t + D - 1, where they exist)
      if (D == 2 && t + 1 < T) wreg_wait<PER>(w[U][0][0], w[U][0][1], w[U][1][0], w[U][1][1]);
      else wreg_wait<0>(w[U][0][0], w[U][0][1], w[U][1][0], w[U][1][1]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // this wave's fragment reads of tile t - 1 are complete
      __builtin_amdgcn_s_barrier();
      if (t + D < T) issue(t + D, std::integral_constant<int, (U + D) % S>{});
      const char *sa = smem + U * 16384;
      // activation fragments one at a time, AHEAD fragments ahead of the MFMA pair that consumes them (the register budget has no room for a K step's worth)
      constexpr int AHEAD = 2;
      half8 af[AHEAD + 1];
      auto frag = [&](int x) { return *(const half8 *)(sa + lds_off((x % MI) * 16 + fr, (x / MI) * 4 + fq)); }; // x = ks * MI + i
#pragma unroll
      for (int x = 0; x < AHEAD; x++) af[x] = frag(x);
#pragma unroll
      for (int x = 0; x < 2 * MI; x++) {
        if (x + AHEAD < 2 * MI) af[(x + AHEAD) % (AHEAD + 1)] = frag(x + AHEAD);
        const int ks = x / MI, i = x % MI;
        const half8 a = af[x % (AHEAD + 1)];
#pragma unroll
        for (int j = 0; j < 2; j++) {
          if (NAT) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, w[U][ks][j], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[U][ks][j], a, acc[i][j], 0, 0, 0);
        }
      }
      // keep that order: hipcc's scheduler otherwise sinks every read to its consumers (one fragment register set, the LDS latency exposed 2 MI times per tile)
      __builtin_amdgcn_sched_group_barrier(0x100, AHEAD, 0);
#pragma unroll
      for (int x = 0; x < 2 * MI; x++) {
        if (x + AHEAD < 2 * MI) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
    };
    for (int t0 = 0; t0 < T; t0 += S) {
      step(t0, std::integral_constant<int, 0>{});
      if (t0 + 1 < T) step(t0 + 1, std::integral_constant<int, 1>{});
      if (S == 3 && t0 + 2 < T) step(t0 + 2, std::integral_constant<int, S - 1>{});
    }
  };
  issue(0, std::integral_constant<int, 0>{});
  if (D == 2) issue(1, std::integral_constant<int, 1>{}); // T >= D (checked by the launcher)
  // Retire the residual loads HERE (a use makes hipcc place its wait now): pending at the loop they would force a wait in front of the first MFMA of every tile
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) asm volatile("" : "+v"(acc[i][j]));
  kloop();
  gemm_epilogue_wreg<MODE, MI, NAT>(g, acc, m0, n0, nblk, wave, fr, fq);
}

// D = 1: a two-slot ring, 32 KB, 4 workgroups per CU with 128 registers per wave (126 used, no spill; the loop waits vmcnt(0) once per tile, which is exact at this distance:
// nothing younger is in flight). D = 2 (three slots, 3 workgroups per CU) compiles to a loop that rotates the weight register sets through v_mov copies — copies of
// inline-asm load destinations that may not have landed — and is therefore not instantiated.
static constexpr int GEMM_WREG_D = 1, GEMM_WREG_LDS = (GEMM_WREG_D + 1) * 16384;
template <int MODE, int D = GEMM_WREG_D>
static __global__ __launch_bounds__(256, 4) void gemm_f16_wreg_kernel(GemmArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int m0, n0, nblk;
  if (!gemm_vh_tile(g, m0, n0, nblk)) return;
  if (gemm_mode_qkv(MODE) && ((n0 + wave * 32) % 192) >= 128) { // wave-uniform; every body passes the same barriers
    if (nblk > 4) gemm_wreg_body<MODE, 8, D, true>(g, m0, n0, nblk, lane, wave);
    else gemm_wreg_body<MODE, 4, D, true>(g, m0, n0, nblk, lane, wave);
  } else {
    if (nblk > 4) gemm_wreg_body<MODE, 8, D, false>(g, m0, n0, nblk, lane, wave);
    else gemm_wreg_body<MODE, 4, D, false>(g, m0, n0, nblk, lane, wave);
  }
}
// the shapes gemm_f16_wreg_kernel takes (gemm_plan has chosen th and ku)
static inline bool gemm_takes_wreg(const GemmArgs &g, int th, int ku) {
  return g.wreg > 0 && g.Wf && g.nseg == 1 && !g.custom_w && th == 8 && ku == 1 && (g.kseg >> 6) >= 2 &&
         (g.mode == GEMM_OUT_F32 || g.mode == GEMM_OUT_QKV || g.mode == GEMM_OUT_QKV_SPLIT);
}

// GEMM + the GroupNorm that consumes it, in one launch (gemm_f16_gn_panel_kernel; the k = 1 in_layers convolution of a ResBlock, whose f32 output H has no other
// reader than the GroupNorm in front of the k = 3 convolution). ONE workgroup of 512 threads owns one sequence (at most 896 rows) x 64 output channels = two GroupNorm
// groups: 8 waves x (7 row blocks x 4 column blocks) of 16 x 16 accumulators, 112 VGPRs per lane. It therefore holds every value a group's statistics are made of: H
// never goes to memory and no statistics cross workgroups.
//   K loop   K tiles of 64 = whole 128-byte lines of every activation row (tiles of 32 in a two-slot ring were measured first: every line crossed the L2 -> L1 path twice,
//            108 us per launch). ONE LDS slot of [896][64] halves (112 KB, gemm_dma_off's image) filled by LDS-DMA, and every wave stages exactly the rows it
//            multiplies: wave w moves the 14 pieces of rows 112 w .. 112 w + 111 and its MFMAs read row blocks 7 w .. 7 w + 6, so the activation tile needs NO
//            barrier. The wave's own counted vmcnt orders its fragment reads behind its DMA, and the prefetch distance comes from registers: a wave copies its 14
//            fragments of tile t into registers, and behind the lgkmcnt(0) that retires those reads it requests its pieces of tile t + 1 into the same rows
//            (program order inside one wave) before the 56 MFMAs of tile t are issued. (The first form dealt the pieces round-robin, wave w moving pieces w + 8 i,
//            and walked K behind two workgroup-wide barriers per tile, "tile landed" and "slot free": 96 us per launch against 86.)
//            The weight tile (8 fragments of 1 KB in the fragment-major image) goes through LDS once per workgroup instead of into the registers of all eight
//            waves: wave w moves fragment w into a two-slot ring behind the activation slot (2 x 8 KB; 128 KB of LDS in all), lane-linear, so every wave's
//            fragment reads are conflict-free. That costs ONE raw barrier per K tile, with the wave's 14 activation pieces of tile t + 1 in flight across it, and
//            takes 56 of the 176 KB a K tile moved through the CU's load path: 84.5 us per launch against 86.7 without it (profiles/gemm_gn_panel_rows_ab.txt).
//            Counted vmcnt (the counts are at the step). Rows past the sequence end are clamped to its last row (duplicates that are never normalised or stored;
//            a wave whose rows all lie past the end stages and multiplies nothing else). The fragment reads are inline asm: behind an LDS-DMA in flight hipcc
//            puts a vmcnt(0) in front of every LDS read it knows of.
//            Every accumulator starts at 0 and adds the same products in ascending K through the same instruction and operand order as gemm_wreg_body<.., NAT = false>,
//            then the bias in one f32 add: the bits of gemm_f16_wreg_kernel<GEMM_OUT_F32>'s H.
//   tail     per 32-channel group: acc + bias -> LDS as [row][32] f32 (112 KB: a wave's panel rows are the LDS rows it staged, free once its own K loop is over),
//            one workgroup-wide barrier, then TAIL — the caller's GroupNorm body (diffusion.hip instantiates
//            gn_reg_kernel<512, 14>'s) — reads its float4s from there; TAIL's own barriers lie between those reads and the second group's writes. gnp_panel_f4
//            names the layout: rows of 128 bytes, chunk ^ (row & 7), conflict-free for the 8-lane groups of the writes and for the reads.
struct GemmGnPanelArgs {
  const __half *A; int lda;   // activations [rows][lda] fp16 (row 0 of the packed layout)
  const __half *Wf;           // fragment-major image of W[N][K] (gemm_wfrag_index)
  int N, K;                   // N % 64 == 0, K % 64 == 0
  const float *bias;          // [N] or nullptr
  const int *seq_start, *seq_len; int ns, rows_total; // 1 <= seq_len[s] <= GEMM_GN_PANEL_ROWS
  // the GroupNorm (gn_reg_kernel's arguments)
  float eps; const float *gn_g, *gn_b, *ss; int do_silu, lut; __half *y; const int *seq_step; int ss_step_stride;
};
static constexpr int GEMM_GN_PANEL_ROWS = 896, GEMM_GN_PANEL_LDS = GEMM_GN_PANEL_ROWS * 128; // one K tile of fp16 = one 32-channel group of f32
static constexpr int GEMM_GN_PANEL_WRING = 2 * 8192, GEMM_GN_PANEL_LDS_LAUNCH = GEMM_GN_PANEL_LDS + GEMM_GN_PANEL_WRING; // + two slots of one weight tile [64 columns][64 K]
// byte offset of float4 chunk q (channels 4 q ..) of row t in the f32 panel
__device__ __forceinline__ int gnp_panel_f4(int t, int q) { return t * 128 + ((q ^ (t & 7)) << 4); }
template <int OFF> __device__ __forceinline__ void gnp_lds_read(half8 &d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
// The plan rule: does a ResBlock's in_layers GEMM + GroupNorm pair of this layout go through the panel kernel. option: gemm_gn_fuse; stats: latency_mode statistics are
// in play; debug_sums: a developer build hashes H; has_wf: the fragment-major image exists; max_len / rows: the layout's longest sequence / packed rows.
static inline int gemm_auto_th(int M, int N);
static inline bool gemm_gn_panel_takes(int option, bool stats, bool debug_sums, bool has_wf, int max_len, int rows, int N, int K) {
  return option != 0 && !stats && !debug_sums && has_wf && max_len >= 1 && max_len <= GEMM_GN_PANEL_ROWS && gemm_auto_th(rows, N) == 8 && (N % 64) == 0 && K >= 64 && (K % 64) == 0;
}
static inline int gemm_gn_panel_grid(int ns, int N) { return 8 * ((ns * (N >> 6) + 7) / 8); } // padded to whole rounds of the 8 XCDs

template <class TAIL>
static __global__ __launch_bounds__(512) void gemm_f16_gn_panel_kernel(GemmGnPanelArgs a, TAIL tail) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  char *smem = smem_dyn;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroup b runs on XCD b % 8: an XCD takes a contiguous range of (sequence, panel) items, sequence-major, so the panels of a sequence fetch its activations through one L2
  const int np = a.N >> 6, nitems = a.ns * np, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int i0 = (int)((long long)nitems * xcd >> 3), i1 = (int)((long long)nitems * (xcd + 1) >> 3);
  if (idx >= i1 - i0) return; // grid padding (whole workgroup, before any barrier)
  const int item = i0 + idx, s = item / np, n0 = (item - s * np) << 6;
  const int T = a.seq_len[s], r0 = a.seq_start[s];
  const int KT = a.K >> 6, fr = lane & 15, fq = lane >> 4; // K tiles of 64: whole 128-byte lines of every activation row
  // DMA piece p = 8 rows x 128 bytes (gemm_dma_off's image: chunk ^ lds_swz(row)); this wave moves pieces 14 wave + i, i < 14: rows 112 wave + 8 i + (lane >> 3),
  // exactly the 7 row blocks its own MFMAs read. The swizzle of those rows depends on the lane alone (112 = 14 x 8)
  const int rb = wave * 112 + (lane >> 3), lda2 = a.lda * 2;
  const unsigned coloff = (unsigned)(((lane & 7) ^ lds_swz(lane >> 3)) << 4);
  const char *aseg = (const char *)(a.A + (size_t)r0 * a.lda);
  const size_t wstride = (size_t)(a.K >> 5) * 512; // halves between the images of two 16-column blocks
  // the weight tile of a K tile = 8 fragments of 1 KB in the fragment-major image, [K step][column block]; wave w stages fragment w (K step w >> 2, column block
  // w & 3) for the whole workgroup into a two-slot ring behind the activation slot, lane-linear: every wave reads all 8 with its own lane offset, conflict-free
  const __half *wsrc = a.Wf + (size_t)((n0 >> 4) + (wave & 3)) * wstride + (wave >> 2) * 512 + lane * 8;
  char *wring = smem + GEMM_GN_PANEL_LDS;
  const unsigned wfb = (unsigned)(size_t)(lptr_t)wring + lane * 16;
  // this wave's fragments: row blocks 7 wave .. 7 wave + 6, lane (fr, fq) = row fr, K chunk 4 ks + fq
  const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem + wave * 7 * 2048;
  const unsigned fb0 = lds0 + lds_off(fr, fq), fb1 = lds0 + lds_off(fr, 4 + fq);
  floatx4 acc[7][4];
#pragma unroll
  for (int i = 0; i < 7; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
  auto dma = [&](int t) {
    const char *ab = aseg + (t << 7);
    int rbv = rb;
    asm volatile("" : "+v"(rbv)); // the 14 offsets are recomputed per tile (a handful of VALU operations) instead of living in 14 registers across the loop
#pragma unroll
    for (int i = 0; i < 14; i++) {
      const unsigned off = (unsigned)(min(rbv + 8 * i, T - 1) * lda2) + coloff;
      __builtin_amdgcn_global_load_lds((gptr_t)(ab + off), (lptr_t)(smem + (wave * 14 + i) * 1024), 16, 0, 0);
    }
  };
  auto wdma = [&](int t) { __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + (size_t)t * 1024), (lptr_t)(wring + ((t & 1) << 13) + wave * 1024), 16, 0, 0); };
  // Activations: a wave reads only LDS rows its own DMA wrote, so its own covering vmcnt orders the fragment reads behind the DMA (RAW), and the re-issue of that
  // DMA behind the lgkmcnt(0) that retires the reads is program order inside one wave (WAR): no barrier. Weights: ONE raw barrier per K tile. Every wave waits for
  // its own piece of W(t) in front of it, so behind it all 8 pieces have landed (RAW); and every wave retired its reads of W(t - 1) (lgkmcnt(0), step t - 1) in
  // front of it, so behind it slot (t + 1) & 1 may be refilled (WAR).
  // vmcnt is one in-order counter. Issue order per step: [activation reads] DMA(t + 1) [14], [barrier] W(t + 1) [1]; the prologue issues DMA(0), W(0). At the top
  // of step t the queue holds DMA(t) [14], W(t) [1], oldest first: vmcnt(1) leaves only W(t) pending, the wave's 14 pieces of tile t have landed. In front of the
  // barrier everything younger than W(t) may be pending: the 14 pieces of DMA(t + 1), which cross the barrier in flight; none in the last step. One wait statement
  // per place, in straight-line code.
  auto step = [&](int t, auto last_c) {
    constexpr bool LAST = decltype(last_c)::value;
    asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); // this wave's own pieces of tile t: the only activation rows it reads
    half8 af[2][7], w[2][4];
    gnp_lds_read<0 * 2048>(af[0][0], fb0);
    gnp_lds_read<1 * 2048>(af[0][1], fb0);
    gnp_lds_read<2 * 2048>(af[0][2], fb0);
    gnp_lds_read<3 * 2048>(af[0][3], fb0);
    gnp_lds_read<4 * 2048>(af[0][4], fb0);
    gnp_lds_read<5 * 2048>(af[0][5], fb0);
    gnp_lds_read<6 * 2048>(af[0][6], fb0);
    gnp_lds_read<0 * 2048>(af[1][0], fb1);
    gnp_lds_read<1 * 2048>(af[1][1], fb1);
    gnp_lds_read<2 * 2048>(af[1][2], fb1);
    gnp_lds_read<3 * 2048>(af[1][3], fb1);
    gnp_lds_read<4 * 2048>(af[1][4], fb1);
    gnp_lds_read<5 * 2048>(af[1][5], fb1);
    gnp_lds_read<6 * 2048>(af[1][6], fb1);
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[0][2]), "+v"(af[0][3]), "+v"(af[0][4]), "+v"(af[0][5]), "+v"(af[0][6]), "+v"(af[1][0]), "+v"(af[1][1]),
                   "+v"(af[1][2]), "+v"(af[1][3]), "+v"(af[1][4]), "+v"(af[1][5]), "+v"(af[1][6])
                 :
                 : "memory");
    if (!LAST) dma(t + 1); // the wave holds its fragments of tile t: its rows are free
    if (LAST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's piece of W(t)
    else asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
    __builtin_amdgcn_s_barrier(); // every wave's piece of W(t) has landed, and every wave has read W(t - 1)
    asm volatile("" ::: "memory");
    if (!LAST) wdma(t + 1);
    const unsigned wf = wfb + ((t & 1) << 13);
    gnp_lds_read<0 * 1024>(w[0][0], wf);
    gnp_lds_read<1 * 1024>(w[0][1], wf);
    gnp_lds_read<2 * 1024>(w[0][2], wf);
    gnp_lds_read<3 * 1024>(w[0][3], wf);
    gnp_lds_read<4 * 1024>(w[1][0], wf);
    gnp_lds_read<5 * 1024>(w[1][1], wf);
    gnp_lds_read<6 * 1024>(w[1][2], wf);
    gnp_lds_read<7 * 1024>(w[1][3], wf);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0][0]), "+v"(w[0][1]), "+v"(w[0][2]), "+v"(w[0][3]), "+v"(w[1][0]), "+v"(w[1][1]), "+v"(w[1][2]), "+v"(w[1][3]) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
#pragma unroll
      for (int i = 0; i < 7; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[ks][j], af[ks][i], acc[i][j], 0, 0, 0);
  };
  dma(0);
  wdma(0);
  for (int t = 0; t + 1 < KT; t++) step(t, std::false_type{});
  step(KT - 1, std::true_type{});
  // nothing of this wave is in flight (its last step waited vmcnt(0)), and the panel rows it writes below are the rows it staged and read itself (the weight ring,
  // which other waves may still be reading, lies behind the panel): no barrier in front of the writes. Other waves read them only behind the __syncthreads() that follows.
  const bool hb = a.bias != nullptr;
  const float *bp = hb ? a.bias : (const float *)a.Wf; // unconditional loads, values selected afterwards (see gemm_epilogue_vh)
  float4 b4[4];
#pragma unroll
  for (int j = 0; j < 4; j++) b4[j] = *(const float4 *)(bp + n0 + j * 16 + fq * 4);
#pragma unroll
  for (int j = 0; j < 4; j++) b4[j] = hb ? b4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int gi = 0; gi < 2; gi++) {
    // (gi == 1: the tail's own barriers lie between its panel reads and these writes)
#pragma unroll
    for (int i = 0; i < 7; i++) {
      const int row = (wave * 7 + i) * 16 + fr;
#pragma unroll
      for (int jj = 0; jj < 2; jj++) {
        const int j = gi * 2 + jj;
        *(float4 *)(smem + gnp_panel_f4(row, jj * 4 + fq)) = make_float4(acc[i][j][0] + b4[j].x, acc[i][j][1] + b4[j].y, acc[i][j][2] + b4[j].z, acc[i][j][3] + b4[j].w);
      }
    }
    __syncthreads();
    tail(a, s, T, r0, n0 + gi * 32, smem);
  }
}

// k = 3 convolution as ONE GEMM with a shared activation slab. The three taps are three row-shifted GEMM
// segments over the SAME activation rows (row_off = -1, 0, +1), so per 64-channel chunk the kernel stages the
// 16 nblk + 2 activation rows m0-1 .. once and multiplies them three times, each time against that tap's weight
// tile and read from LDS one row further down. Operand traffic through the CU's load path per chunk:
// 17 + 3 x 16 = 65 DMA pieces instead of 3 x 32 = 96 — the 128^2 tile is bound by exactly that path
// (64 B/clk/CU feeds at most one 32 KB K tile per 512 MFMA cycles).
// The weight tiles alternate between two LDS buffers: tap p+1's tile is requested before tap p's is waited for
// (counted vmcnt + raw barrier), so only the slab load at the start of a chunk is exposed.
// LDS: 17 KB slab + 2 x 16 KB -> 3 workgroups per CU.
static constexpr int CONV3_VH_LDS = (128 + 8) * 128 + 2 * 16384;
template <int MODE, int MI>
__device__ __forceinline__ void gemm_conv3_vh_body(const GemmArgs &g, int m0, int n0, int nblk, int lane, int wave) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  char *smem = smem_dyn;
  constexpr int MA = MI > 0 ? MI : 1;
  const int wm = wave >> 1, wn = wave & 1;
  const int my_pa = (2 * nblk + 1 - wave + 3) >> 2; // slab = 2 nblk + 1 pieces of 8 rows (the last one carries row m0 + 16 nblk)
  const int nchunks = g.kseg >> 6, ldw = 3 * g.kseg, nph = 3 * nchunks;
  const int prow = lane >> 3, pslot = lane & 7;
  const int fr = lane & 15, fq = lane >> 4;
  floatx4 acc[MA][4]; // from zero: the residual is read by the epilogue (EPI_RESID_LOAD)
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
  char *sa = smem, *sb = smem + (128 + 8) * 128;
  const __half *abase = g.A[0] + (ptrdiff_t)(m0 - 1) * g.lda; // slab row s = activation row m0 - 1 + s (the buffer has its guard rows)
  const __half *wbase = g.W + (size_t)n0 * ldw;
  int aoff[5], boff[4]; // kept apart from gemm_dma_off: with it (and gemm_for_my_mi) gemm_f16_conv3_vh_kernel<5> took 168 VGPRs against 166
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const int row = (wave + 4 * i) * 8 + prow;
    aoff[i] = min(row, g.M - m0 + 1) * g.lda + (pslot ^ lds_swz(row)) * 8; // rows past the buffer end are never multiplied: clamp
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int row = (wave * 4 + i) * 8 + prow;
    boff[i] = row * ldw + (pslot ^ lds_swz(row)) * 8;
  }
  auto stageA = [&](int kc) {
    const __half *src = abase + (min(kc, nchunks - 1) << 6);
#pragma unroll
    for (int i = 0; i < 5; i++)
      if (i < my_pa) __builtin_amdgcn_global_load_lds((gptr_t)(src + aoff[i]), (lptr_t)(sa + (wave + 4 * i) * 1024), 16, 0, 0);
  };
  auto stageB = [&](int p) { // phase p = chunk p / 3, tap p % 3 (clamped past the end: uniform vmcnt arithmetic)
    p = min(p, nph - 1);
    const int kc = p / 3, tap = p - kc * 3;
    const __half *src = wbase + tap * g.kseg + (kc << 6);
    char *dst = sb + (p & 1) * 16384;
#pragma unroll
    for (int i = 0; i < 4; i++) __builtin_amdgcn_global_load_lds((gptr_t)(src + boff[i]), (lptr_t)(dst + (wave * 4 + i) * 1024), 16, 0, 0);
  };
  // one phase; TAP = p % 3 is compile-time (the caller unrolls the three taps of a K chunk)
  auto phase = [&](int kc, int p, auto tap_c) {
    constexpr int TAP = decltype(tap_c)::value;
    stageB(p + 1); // its buffer was last read in phase p-1, which every wave has left (trailing barrier)
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); // all but the 4 pieces just issued: B(p) and the slab have landed
    __builtin_amdgcn_s_barrier();
    const char *sbp = sb + (p & 1) * 16384;
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      half8 af[MA], bf[4];
#pragma unroll
      for (int i = 0; i < MI; i++) af[i] = *(const half8 *)(sa + lds_off(vh_blk(wm, i) * 16 + fr + TAP, ks * 4 + fq));
      if (MI > 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) bf[i] = *(const half8 *)(sbp + lds_off(wn * 64 + i * 16 + fr, ks * 4 + fq));
      }
#pragma unroll
      for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier(); // every wave is done reading the slab and B(p)
    if (TAP == 2) stageA(kc + 1);
  };
  stageA(0);
  stageB(0);
  for (int kc = 0; kc < nchunks; kc++) {
    const int p = 3 * kc;
    phase(kc, p, std::integral_constant<int, 0>{});
    phase(kc, p + 1, std::integral_constant<int, 1>{});
    phase(kc, p + 2, std::integral_constant<int, 2>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // trailing (clamped) pieces must land before the LDS is released
  if ((MODE == GEMM_OUT_F32 || MODE == GEMM_OUT_F32_STATS) && g.resid) gemm_epilogue_vh<MODE, MI, EPI_RESID_LOAD>(g, acc, m0, n0, wm, wn, fr, fq);
  else gemm_epilogue_vh<MODE, MI, EPI_NO_RESID>(g, acc, m0, n0, wm, wn, fr, fq);
}

template <int MODE>
static __global__ __launch_bounds__(256, 3) void gemm_f16_conv3_vh_kernel(GemmArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int m0, n0, nblk;
  if (!gemm_vh_tile(g, m0, n0, nblk)) return;
  gemm_for_my_mi(nblk, wave, [&](auto mi) { gemm_conv3_vh_body<MODE, decltype(mi)::value>(g, m0, n0, nblk, lane, wave); });
}

// k = 3 convolution (three row-shifted segments of one activation buffer, tap-major weights): shared-slab kernel
static inline bool gemm_is_conv3(const GemmArgs &g) {
  return g.nseg == 3 && !g.custom_w && g.A[0] == g.A[1] && g.A[1] == g.A[2] && g.row_off[0] == -1 && g.row_off[1] == 0 && g.row_off[2] == 1 &&
         !gemm_mode_qkv(g.mode) && !gemm_mode_scaled(g.mode);
}

// k = 3 convolution with the WEIGHT operand through registers (gemm_f16_conv3_wreg_kernel; GEMM_OUT_F32 with or without residual, 128-row tiles). The move of
// gemm_f16_wreg_kernel applied to the shared-slab kernel: the loader keeps one fragment-major image per tap,
//   Wf3[tap][n / 16][k / 32][lane][k % 8]   (gemm_wfrag3_index: tap * N * K + gemm_wfrag_index(n, k, K)),
// the waves lie 1 x 4 along N (all rows of the tile x 32 columns each, no weight fragment fetched twice) and LDS holds only the activation slab, as a ring of TWO
// slots of 17 KB (34 KB: four workgroups per CU). Per 64-channel chunk a wave requests its 5 slab pieces (17 pieces over four waves; waves 1-3 repeat piece 16, the
// same bytes to the same place, so that every wave counts the same vmcnt events) and 3 x 4 weight fragments, against 17 + 48 pieces staged by the LDS kernel, and
// passes ONE barrier instead of six. The weight registers rotate per PHASE (one tap of one chunk: 4 fragments = 16 VGPRs per set, two sets): a chunk's worth per
// set (48) does not fit beside 64 accumulator registers in the 128 of four workgroups per CU. Order of a chunk kc (slab slot kc & 1):
//   tap 0: wait vmcnt(0) [slab kc and W(kc, 0), nothing younger in flight] -> barrier (slab kc complete in every wave's view; every wave has left slot (kc + 1) & 1)
//          -> request W(kc, 1), THEN slab kc + 1 (vmcnt is one in-order counter: the weights the next phase waits for must be older than the slab) -> multiply
//   tap 1: wait vmcnt(5) [all but the slab pieces: W(kc, 1)] -> request W(kc, 2) -> multiply          (last chunk: the last slab again, into the free slot)
//   tap 2: wait vmcnt(0) [slab kc + 1, requested two phases ago, and W(kc, 2)] -> request W(kc + 1, 0) -> multiply
// Accumulators start from zero and add chunk, tap, K step in the order of gemm_conv3_vh_body, weight fragment first; the epilogue adds bias, then the loaded
// residual, then zeroes guard rows, as gemm_epilogue_vh<.., EPI_RESID_LOAD> does: bit-identical to gemm_f16_conv3_vh_kernel.
static inline size_t gemm_wfrag3_index(int n, int tap, int k, int N, int K) { // index (in halves) of tap `tap` of W[n][tap * K + k] in the per-tap fragment-major images
  return (size_t)tap * N * K + gemm_wfrag_index(n, k, K);
}
static constexpr int CONV3_WREG_SLOT = (128 + 8) * 128, CONV3_WREG_LDS = 2 * CONV3_WREG_SLOT;

// gemm_epilogue_wreg's F32 branch with the residual read here: (acc + bias) + resid, guard rows zeroed; blocks in pairs, the next pair's loads in flight while this
// pair is stored (the order of gemm_epilogue_vh<.., EPI_RESID_LOAD>). resid may alias outF: a lane reads exactly the elements it writes, before it writes them
template <int MI, bool RESID>
__device__ __forceinline__ void gemm_epilogue_conv3_wreg(const GemmArgs &g, floatx4 (&acc)[MI][2], int m0, int n0, int nblk, int wave, int fr, int fq) {
  const int col0 = n0 + wave * 32 + fq * 4;
  const bool hb = g.bias != nullptr, hs = g.row_seq != nullptr;
  const float *bp = hb ? g.bias : (const float *)g.W; // unconditional loads, values selected afterwards (see gemm_epilogue_vh)
  const int *sp = hs ? g.row_seq : (const int *)g.A[0];
  float4 b4[2], rr[2][2];
  int sq[MI];
  auto load_pair = [&](int p) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const float *rp = g.resid + (size_t)(m0 + min(2 * p + q, nblk - 1) * 16 + fr) * g.ldo + col0; // blocks past a short tile re-read its last one (never used)
#pragma unroll
      for (int j = 0; j < 2; j++) rr[q][j] = *(const float4 *)(rp + j * 16);
    }
  };
  if (RESID) load_pair(0);
#pragma unroll
  for (int j = 0; j < 2; j++) b4[j] = *(const float4 *)(bp + col0 + j * 16);
#pragma unroll
  for (int i = 0; i < MI; i++) sq[i] = sp[m0 + min(i, nblk - 1) * 16 + fr];
#pragma unroll
  for (int j = 0; j < 2; j++) b4[j] = hb ? b4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < MI; i++) sq[i] = hs ? sq[i] : 0;
#pragma unroll
  for (int p = 0; p < MI / 2; p++) {
    float4 v[2][2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int i = 2 * p + q;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        float4 t = make_float4(acc[i][j][0] + b4[j].x, acc[i][j][1] + b4[j].y, acc[i][j][2] + b4[j].z, acc[i][j][3] + b4[j].w);
        if (RESID) { t.x += rr[q][j].x; t.y += rr[q][j].y; t.z += rr[q][j].z; t.w += rr[q][j].w; }
        if (sq[i] < 0) t = make_float4(0.f, 0.f, 0.f, 0.f);
        v[q][j] = t;
      }
    }
    if (RESID && p + 1 < MI / 2) load_pair(p + 1);
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int i = 2 * p + q;
      if (i < nblk) {
        float *op = g.outF + (size_t)(m0 + i * 16 + fr) * g.ldo + col0;
#pragma unroll
        for (int j = 0; j < 2; j++) *(float4 *)(op + j * 16) = v[q][j];
      }
    }
  }
}

template <int MI, bool RESID>
__device__ __forceinline__ void gemm_conv3_wreg_body(const GemmArgs &g, int m0, int n0, int nblk, int lane, int wave) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[]; // ONE LDS object (see gemm_vh_body)
  char *smem = smem_dyn;
  constexpr int NP = 2 * MI + 1;     // 8-row pieces of the slab (rows m0 - 1 .. m0 + 16 MI)
  constexpr int NPA = (NP + 3) / 4;  // requested per wave and chunk: vmcnt events of a slab
  const int nchunks = g.kseg >> 6, KS = g.kseg >> 5;
  const int fr = lane & 15, fq = lane >> 4;
  unsigned aoff[NPA]; // byte offsets from a wave-uniform base; rows past a short tile are clamped into it (duplicates that are never stored)
#pragma unroll
  for (int i = 0; i < NPA; i++) aoff[i] = (unsigned)(gemm_dma_off(min(wave + 4 * i, NP - 1), lane, 0, nblk * 16 + 1, g.lda) * 2);
  const char *aseg = (const char *)(g.A[0] + (ptrdiff_t)(m0 - 1) * g.lda); // slab row s = activation row m0 - 1 + s (the buffer has its guard rows)
  const size_t tap_stride = (size_t)g.N * g.kseg;
  const __half *wp = g.Wf + (size_t)((n0 >> 4) + wave * 2) * KS * 512; // tap 0, this wave's first column block (wave-uniform)
  const unsigned wlane = lane * 16;
  floatx4 acc[MI][2]; // from zero: the residual is read by the epilogue
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
  // fragment read addresses: lds_off(16 i + fr + tap, 4 ks + fq) = 2048 i + lds_off(fr + tap, 4 ks + fq) (the swizzle has period 8 rows): one register per (tap, K step),
  // block and slot are immediate offsets. Opaque to hipcc, which otherwise keeps an address per (block, tap, K step) and spills them
  int fbase[3][2];
#pragma unroll
  for (int tap = 0; tap < 3; tap++)
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
      fbase[tap][ks] = lds_off(fr + tap, ks * 4 + fq);
      asm volatile("" : "+v"(fbase[tap][ks]));
    }
  half8 w[2][2][2]; // [set][k step][column block]
  auto issue_w = [&](int kc, int tap, auto set_c) {
    constexpr int U = decltype(set_c)::value;
    const __half *q0 = wp + (size_t)tap * tap_stride + (size_t)min(kc, nchunks - 1) * 1024, *q1 = q0 + (size_t)KS * 512; // past the last chunk: see issue_slab
    wreg_load<0>(w[U][0][0], q0, wlane);
    wreg_load<0>(w[U][0][1], q1, wlane);
    wreg_load<1024>(w[U][1][0], q0, wlane);
    wreg_load<1024>(w[U][1][1], q1, wlane);
  };
  auto issue_slab = [&](int kc, int slot) {
    const char *ab = aseg + (min(kc, nchunks - 1) << 7); // past the last chunk: the last one again, into the free slot (every phase counts the same vmcnt events)
    asm volatile("" : "+s"(ab));
#pragma unroll
    for (int i = 0; i < NPA; i++) {
      unsigned o = aoff[i];
      asm volatile("" : "+v"(o)); // base and offset opaque: scalar base + 32-bit lane offset (hipcc otherwise re-associates them into 64-bit VGPR addresses kept across the loop)
      __builtin_amdgcn_global_load_lds((gptr_t)(ab + o), (lptr_t)(smem + slot * CONV3_WREG_SLOT + min(wave + 4 * i, NP - 1) * 1024), 16, 0, 0);
    }
  };
  // one phase: chunk kc (PAR = kc & 1 names its slab slot), tap TAP. No branch around a wait or a request: a join would copy weight registers (v_mov of a load
  // destination that may not have landed)
  auto phase = [&](int kc, auto par_c, auto tap_c) {
    constexpr int PAR = decltype(par_c)::value, TAP = decltype(tap_c)::value, U = PAR ^ (TAP & 1);
    wreg_wait<TAP == 1 ? NPA : 0>(w[U][0][0], w[U][0][1], w[U][1][0], w[U][1][1]);
    if (TAP == 0) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // this wave's fragment reads of chunk kc - 1 are complete
      __builtin_amdgcn_s_barrier();
    }
    if (TAP < 2) issue_w(kc, TAP + 1, std::integral_constant<int, U ^ 1>{});
    else issue_w(kc + 1, 0, std::integral_constant<int, U ^ 1>{});
    if (TAP == 0) issue_slab(kc + 1, PAR ^ 1);
    const char *sa = smem + PAR * CONV3_WREG_SLOT;
    // activation fragments one at a time, AHEAD fragments ahead of the MFMA pair that consumes them (see gemm_wreg_body)
    constexpr int AHEAD = 2;
    half8 af[AHEAD + 1];
    auto frag = [&](int x) { return *(const half8 *)(sa + fbase[TAP][x / MI] + (x % MI) * 2048); }; // x = ks * MI + i
#pragma unroll
    for (int x = 0; x < AHEAD; x++) af[x] = frag(x);
#pragma unroll
    for (int x = 0; x < 2 * MI; x++) {
      if (x + AHEAD < 2 * MI) af[(x + AHEAD) % (AHEAD + 1)] = frag(x + AHEAD);
      const int ks = x / MI, i = x % MI;
      const half8 a = af[x % (AHEAD + 1)];
#pragma unroll
      for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[U][ks][j], a, acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x100, AHEAD, 0);
#pragma unroll
    for (int x = 0; x < 2 * MI; x++) {
      if (x + AHEAD < 2 * MI) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    }
  };
  auto chunk = [&](int kc, auto par_c) {
    phase(kc, par_c, std::integral_constant<int, 0>{});
    phase(kc, par_c, std::integral_constant<int, 1>{});
    phase(kc, par_c, std::integral_constant<int, 2>{});
  };
  issue_slab(0, 0);
  issue_w(0, 0, std::integral_constant<int, 0>{});
  for (int kc = 0; kc < nchunks; kc += 2) { // two chunks per trip: slab slots and register sets are compile-time
    chunk(kc, std::integral_constant<int, 0>{});
    if (kc + 1 < nchunks) chunk(kc + 1, std::integral_constant<int, 1>{});
  }
  // the last phase's (repeated) weight request lands before its registers are reused; the repeated slab has landed at the last tap 2
  wreg_wait<0>(w[0][0][0], w[0][0][1], w[0][1][0], w[0][1][1]);
  wreg_wait<0>(w[1][0][0], w[1][0][1], w[1][1][0], w[1][1][1]);
  gemm_epilogue_conv3_wreg<MI, RESID>(g, acc, m0, n0, nblk, wave, fr, fq);
}

template <bool RESID>
static __global__ __launch_bounds__(256, 4) void gemm_f16_conv3_wreg_kernel(GemmArgs g) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int m0, n0, nblk;
  if (!gemm_vh_tile(g, m0, n0, nblk)) return;
  if (nblk > 4) gemm_conv3_wreg_body<8, RESID>(g, m0, n0, nblk, lane, wave);
  else gemm_conv3_wreg_body<4, RESID>(g, m0, n0, nblk, lane, wave);
}
// the shapes gemm_f16_conv3_wreg_kernel takes: g.Wf is then the per-tap image (gemm_wfrag3_index). The STATS and F16 modes, shorter tiles and so the small grids stay
// with the LDS-staged kernel
static inline bool gemm_takes_conv3_wreg(const GemmArgs &g, int th) {
  return g.wreg > 0 && g.Wf && gemm_is_conv3(g) && th == 8 && g.mode == GEMM_OUT_F32;
}

// tile height (16-row blocks) launch_gemm_f16 chooses for an M x N problem
static inline int gemm_auto_th(int M, int N) {
  const int maxb = ((M >> 4) + 7) / 8 + 1, NT = N >> 7;
  int th = 2;
  while (th < 8 && 8 * ((maxb + th - 1) / th) * NT > 1024) th *= 2;
  return th;
}

// What launch_gemm_f16 does with a set of arguments: pure host arithmetic, no HIP call (the kernel tests read it to say which kernel ran). th / ku / cn / grid / lds are the
// EFFECTIVE values, those of the instantiation that is launched: the k = 3 and the register-streamed kernel have no KU (1), the dual-B kernel has 1 and 2.
enum { GEMM_KERNEL_VH = 0, GEMM_KERNEL_DUALB = 1, GEMM_KERNEL_CONV3 = 2, GEMM_KERNEL_WREG = 3, GEMM_KERNEL_CONV3_WREG = 4 };
struct GemmPlan {
  hipError_t err; // hipErrorInvalidValue: refused, nothing is launched (the other fields still say what the rules select)
  int kernel;     // GEMM_KERNEL_*
  int th, ku, cn; // 16-row blocks per tile, K tiles per barrier pair, column tiles per L2 chunk
  int grid, lds;  // workgroups, dynamic LDS bytes
};
static inline GemmPlan gemm_plan(const GemmArgs &g) {
  GemmPlan p = {};
  const int NT = g.N >> 7, ktot = g.nseg * g.kseg, nb = g.M >> 4;
  p.err = hipSuccess;
  if (gemm_mode_scaled(g.mode)) { // the accumulators start from resid / alpha and are scaled back by alpha: exact only for a non-zero power of two
    int e;
    if (!(g.alpha != 0.f) || std::fabs(std::frexp(g.alpha, &e)) != 0.5f) p.err = hipErrorInvalidValue;
  }
  if (gemm_mode_stats(g.mode) && (!g.st_out || !g.chunk_seq || g.st_stripe_ll <= 0)) p.err = hipErrorInvalidValue;
  // dual_b names ONE kernel: a caller whose arguments do not describe "hi | lo halves of one weight over one activation operand" gets an error, not another kernel
  if (g.dual_b && !(gemm_mode_scaled(g.mode) && g.nseg == 2 && g.custom_w && g.A[0] == g.A[1] && g.row_off[0] == g.row_off[1])) p.err = hipErrorInvalidValue;
  int ku = (g.ku == 2 || g.ku == 4) && (g.kseg % (64 * g.ku)) == 0 ? g.ku : 1;
  // L2 chunking of the column tiles: pays for wide outputs (N = 3072: 200 us with chunks of 8 column tiles against 232 unchunked and 207-219
  // with chunks of 6) and costs ~3 % when the activations would have to stream twice for a narrow one (N = 1024, K = 3072)
  // -> only chunk when NT > 8; the chunk is the largest divisor of NT whose weight rows fit ~2.5 MB
  p.cn = NT;
  if (NT > 8)
    for (p.cn = NT; p.cn > 1; p.cn--)
      if (NT % p.cn == 0 && (size_t)p.cn * 128 * ktot * 2 <= (size_t)2560 * 1024) break;
  // Tile height: 128 rows unless the problem is small. Mixed heights, exactly filled rounds and tallest-first orders were measured
  // through explicit tile tables (profiles/r3_gemm_tile_tables.txt): no policy beats uniform 128-row
  // tiles at the benchmark's sizes. Small problems (a single utterance: M = 1 792 rows) want more, shorter tiles — halve the height
  // while the grid stays within one round of the ~1024 resident slots.
  const int maxb = (nb + 7) / 8 + 1; // blocks of the largest XCD range (upper bound)
  p.th = g.th > 0 ? g.th : gemm_auto_th(g.M, g.N);
  // One utterance (M = 1 792 rows, N = 1 024: 224 tiles of 64 rows = at most one workgroup per CU): four K tiles per barrier pair at 64-row tiles — a lone
  // workgroup pays its DMA round trip and two barriers per 256 of K instead of per 64 (profiles/r6_small_gemm.txt: k = 1 12.6 -> 11.6 us warm, 22.8 -> 17.9 us
  // with cold weights; the K = 2 048 integrating conv 25.7 / 36.2 -> 20.3 / 27.8). Same products in the same order: bit-identical to every other tiling.
  // (the split-weight proj_out, 48 KB per K tile: two per barrier pair, 21.5 -> 19.1 us warm / 28.3 -> 25.6 cold; the k = 3 kernel has its own pipeline and only takes
  // the 64-row tiles: 27.3 -> 25.5 / 35.6 -> 32.2)
  if (g.th <= 0 && g.ku == 0 && NT <= 8 && 8 * ((maxb + 3) / 4) * NT <= 256 && (g.kseg % 256) == 0) {
    p.th = 4;
    if (!gemm_is_conv3(g)) ku = g.dual_b ? 2 : 4;
  }
  int mt_max = 0; // tiles of the XCD with the most blocks: the grid is padded to 8 times that
  for (int x = 0; x < 8; x++) {
    const int b0 = (int)((long long)nb * x >> 3), b1 = (int)((long long)nb * (x + 1) >> 3);
    mt_max = std::max(mt_max, (b1 - b0 + p.th - 1) / p.th);
  }
  p.grid = 8 * mt_max * NT;
  if (gemm_takes_wreg(g, p.th, ku)) { p.kernel = GEMM_KERNEL_WREG; p.ku = 1; p.lds = GEMM_WREG_LDS; }
  else if (gemm_takes_conv3_wreg(g, p.th)) { p.kernel = GEMM_KERNEL_CONV3_WREG; p.ku = 1; p.lds = CONV3_WREG_LDS; }
  else if (gemm_is_conv3(g)) { p.kernel = GEMM_KERNEL_CONV3; p.ku = 1; p.lds = CONV3_VH_LDS; }
  else if (g.dual_b) { p.kernel = GEMM_KERNEL_DUALB; p.ku = ku == 2 ? 2 : 1; p.lds = p.ku * GEMM_DUALB_LDS; } // a requested KU of 4 has no dual-B instantiation
  else { p.kernel = GEMM_KERNEL_VH; p.ku = ku; p.lds = ku * GEMM_VH_LDS; } // KU > 1: 64 / 128 KB of LDS -> 2 / 1 workgroups per CU
  return p;
}

// One instantiation's launch. More dynamic LDS than the 48 KB a kernel may use by default (the k = 3 kernel, KU 2 / 4, dual-B KU 2) is asked for once per instantiation.
// The threshold names exactly those: dual-B KU 1 (48 KB) and every smaller stage are never raised; a change of an LDS size changes which instantiations get the call.
static_assert(GEMM_DUALB_LDS <= 48 * 1024 && GEMM_VH_LDS <= 48 * 1024 && GEMM_WREG_LDS <= 48 * 1024 && CONV3_WREG_LDS <= 48 * 1024 && CONV3_VH_LDS > 48 * 1024, "which launches raise their dynamic LDS limit");
template <void (*KERN)(GemmArgs)> static inline void gemm_launch(const GemmPlan &p, const GemmArgs &g, hipStream_t s) {
  if (p.lds > 48 * 1024) {
    static bool raised = false;
    if (!raised) { (void)hipFuncSetAttribute((const void *)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds); raised = true; }
  }
  KERN<<<p.grid, 256, p.lds, s>>>(g);
}
// mode -> instantiation, once per kernel. The occupancy bound of a KU > 1 launch is a compile-time promise: WGS
template <int KU> static inline void gemm_launch_vh(const GemmPlan &p, const GemmArgs &g, hipStream_t s) {
  constexpr int WGS = KU == 1 ? 4 : KU == 2 ? 2 : 1;
  switch (g.mode) {
    case GEMM_OUT_F32: return gemm_launch<gemm_f16_vh_kernel<GEMM_OUT_F32, WGS, KU>>(p, g, s);
    case GEMM_OUT_F16: return gemm_launch<gemm_f16_vh_kernel<GEMM_OUT_F16, WGS, KU>>(p, g, s);
    case GEMM_OUT_QKV: return gemm_launch<gemm_f16_vh_kernel<GEMM_OUT_QKV, WGS, KU>>(p, g, s);
    case GEMM_OUT_QKV_SPLIT: return gemm_launch<gemm_f16_vh_kernel<GEMM_OUT_QKV_SPLIT, WGS, KU>>(p, g, s);
    case GEMM_OUT_F32_SCALED: return gemm_launch<gemm_f16_vh_kernel<GEMM_OUT_F32_SCALED, WGS, KU>>(p, g, s);
    case GEMM_OUT_F32_STATS: return gemm_launch<gemm_f16_vh_kernel<GEMM_OUT_F32_STATS, WGS, KU>>(p, g, s);
    default: return gemm_launch<gemm_f16_vh_kernel<GEMM_OUT_F32_SCALED_STATS, WGS, KU>>(p, g, s);
  }
}
template <int KU> static inline void gemm_launch_dualb(const GemmPlan &p, const GemmArgs &g, hipStream_t s) {
  if (g.mode == GEMM_OUT_F32_SCALED) gemm_launch<gemm_f16_vh_dualb_kernel<GEMM_OUT_F32_SCALED, KU>>(p, g, s);
  else gemm_launch<gemm_f16_vh_dualb_kernel<GEMM_OUT_F32_SCALED_STATS, KU>>(p, g, s);
}
static inline void gemm_launch_conv3(const GemmPlan &p, const GemmArgs &g, hipStream_t s) {
  if (g.mode == GEMM_OUT_F32) gemm_launch<gemm_f16_conv3_vh_kernel<GEMM_OUT_F32>>(p, g, s);
  else if (g.mode == GEMM_OUT_F32_STATS) gemm_launch<gemm_f16_conv3_vh_kernel<GEMM_OUT_F32_STATS>>(p, g, s);
  else gemm_launch<gemm_f16_conv3_vh_kernel<GEMM_OUT_F16>>(p, g, s);
}
static inline void gemm_launch_conv3_wreg(const GemmPlan &p, const GemmArgs &g, hipStream_t s) {
  if (g.resid) gemm_launch<gemm_f16_conv3_wreg_kernel<true>>(p, g, s);
  else gemm_launch<gemm_f16_conv3_wreg_kernel<false>>(p, g, s);
}
static inline void gemm_launch_wreg(const GemmPlan &p, const GemmArgs &g, hipStream_t s) {
  if (g.mode == GEMM_OUT_F32) gemm_launch<gemm_f16_wreg_kernel<GEMM_OUT_F32>>(p, g, s);
  else if (g.mode == GEMM_OUT_QKV) gemm_launch<gemm_f16_wreg_kernel<GEMM_OUT_QKV>>(p, g, s);
  else gemm_launch<gemm_f16_wreg_kernel<GEMM_OUT_QKV_SPLIT>>(p, g, s);
}

static inline hipError_t launch_gemm_f16(const GemmArgs &g, hipStream_t s) {
  const GemmPlan p = gemm_plan(g);
  if (p.err != hipSuccess) return p.err;
  GemmArgs gg = g;
  gg.th = p.th;
  gg.cn = p.cn;
  if (p.kernel == GEMM_KERNEL_WREG) gemm_launch_wreg(p, gg, s);
  else if (p.kernel == GEMM_KERNEL_CONV3_WREG) gemm_launch_conv3_wreg(p, gg, s);
  else if (p.kernel == GEMM_KERNEL_CONV3) gemm_launch_conv3(p, gg, s);
  else if (p.kernel == GEMM_KERNEL_DUALB) p.ku == 2 ? gemm_launch_dualb<2>(p, gg, s) : gemm_launch_dualb<1>(p, gg, s);
  else p.ku == 4 ? gemm_launch_vh<4>(p, gg, s) : p.ku == 2 ? gemm_launch_vh<2>(p, gg, s) : gemm_launch_vh<1>(p, gg, s);
  return hipGetLastError();
}

} // namespace tts
