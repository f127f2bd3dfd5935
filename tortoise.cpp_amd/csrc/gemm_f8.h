// The diffusion k = 3 out_layers convolution on the fp8 MFMA of gfx950 (v_mfma_f32_16x16x128_f8f6f4, OCP e4m3 x e4m3 -> f32): option "conv3_fp8" 1.
//
//   out[r][n] = (sum_tap sum_k A8[r + tap - 1][k] * W8[n][tap][k]) * inv_a[r] * inv_w[n] + bias[n] + resid[r][n]
//
// Three pieces, each one launch (or, the weights, one host pass at load time):
//   gemm_f8_pack_weight        W[n][tap][k] f32 -> e4m3 bytes in one fragment-major image per tap + inv_w[n]. One power-of-two scale per output channel
//                              (f8_pow2_scale: max |W[n]| * s_n in [224, 448), e4m3's top binade), so W * s_n uses the format's whole range and 1 / s_n is exact.
//   quant_f8_amax_kernel +     the fp16 operand the GroupNorm left (packed rows, guard rows zero) -> A8 e4m3 + inv_a[row]. The scale is per SEQUENCE: a tap adds rows
//   quant_f8_convert_kernel    r - 1, r, r + 1 into one accumulator, so they must share a scale, and a sequence's neighbours are guard zeros. The maximum is
//                              reduced without atomics and without a clear: F8_AMAX_PARTS work-groups per sequence each write the maximum of their rows (as the bit
//                              pattern of |x|, an order-independent integer maximum) and the convert launch reduces the parts of its chunk's sequence again. Guard
//                              and pad rows are written as zero bytes, their inv_a as 0.
//   gemm_f8_conv3_kernel       the convolution (below).
//
// gemm_f8_conv3_kernel: 128 rows x 128 columns per work-group, four waves 1 x 4 along N (wave w: all rows x columns 32 w .. 32 w + 31), a K chunk = 128 channels =
// ONE MFMA K step = 128 bytes per activation row. It keeps the pipeline of gemm_f16_conv3_wreg_kernel (gemm_f16.h), whose byte geometry is the same (a 64-channel
// fp16 chunk is 128 bytes too), around a different inner product:
//  * Weights never touch LDS. A tap's weight set of a wave is 2 column blocks x 8 VGPRs, loaded as two coalesced 16-byte loads per lane and block from the per-tap
//    image and requested one tap ahead (two register sets rotate per tap).
//  * Activation slab: rows m0 - 1 .. m0 + 134 of one chunk (17 DMA pieces of 8 rows x 128 B; only 130 rows are multiplied), a two-slot LDS ring (2 x 17 KB, three
//    work-groups per CU: see the accumulators) filled by global_load_lds_dwordx4 one chunk ahead. The three taps read the same slab at row offsets 0, 1, 2.
//  * Bank conflicts: the row pitch stays 128 B and the 16-byte chunks of a row are XOR-swizzled on the SOURCE address with lds_swz (gemm_f16.h), not padded. The K
//    ORDER inside the instruction is chosen so that the reads are the ones that swizzle was measured conflict-free for, at any first row: the MFMA sums over (lane
//    quarter fq, byte j of the lane's 32) and both operands index K the same way, so any row-independent assignment of channels to (fq, j) gives the same sum. Lane
//    (fr, fq) takes bytes 16 fq .. 16 fq + 15 of the chunk as its low half and 64 + 16 fq .. as its high half (gemm_f8_kslot): two ds_read_b128 at 16-byte chunks fq
//    and 4 + fq of row fr, exactly the two fragment reads (K step 0 and 1) of the fp16 kernel. 32 consecutive bytes per lane, the instruction's natural order, would
//    read chunks 2 fq and 2 fq + 1, which differ in the bits the swizzle permutes.
//  * One raw barrier per K chunk, counted vmcnt waits (one in-order counter for DMA pieces and register loads; every wave issues 5 + 3 x 4 per chunk):
//      tap 0: wait vmcnt(0) -> barrier -> request W(kc, 1), then slab kc + 1 -> multiply     tap 1: wait vmcnt(5) -> request W(kc, 2) -> multiply
//      tap 2: wait vmcnt(0) -> request W(kc + 1, 0) -> multiply
//  * Accumulators: 8 row blocks x 2 column blocks x 4 f32 = 64 VGPRs with the 16 x 16 x 128 form (the 32 x 32 x 64 form wants 32-row weight blocks: with 32
//    columns per wave in the 1 x 4 layout that is one block and half the issue rate per fragment read). Operands swapped (weight = A operand): a lane holds 4
//    consecutive columns of one row. Beside them 32 weight registers (two sets), 16 for two activation fragments, and the epilogue's scales, bias and residual: at
//    the 128 registers of four work-groups per CU hipcc spilled (19 / 45 VGPRs), so the kernel is bounded to THREE work-groups per CU: 150 / 166 VGPRs, 0 AGPRs,
//    no scratch, 34 816 B of LDS.
//  * Epilogue, one fixed order: t = acc * (inv_a[r] * inv_w[n]) (powers of two: exact), + bias[n], + resid[r][n]; guard rows (row_seq < 0) are stored as 0 like the
//    fp16 kernels do; rows >= rows_total are not stored.
// Resource summary and measurements: profiles/conv3_fp8.txt.
#pragma once
#include "gemm_f16.h"

#include <cstdint>
#include <vector>

namespace tts {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx8 __attribute__((ext_vector_type(8)));

// ---- the one statement of the operand order ----
// Channel kk (0 .. 127) of a K chunk sits in lane quarter fq, byte j (0 .. 31) of the lane's fragment: low half = 16-byte chunk fq, high half = chunk 4 + fq.
static inline int gemm_f8_kslot_fq(int kk) { return (kk >> 4) & 3; }
static inline int gemm_f8_kslot_byte(int kk) { return ((kk >> 6) << 4) | (kk & 15); }
// byte index of tap `tap` of W[n][tap][k] in the per-tap fragment-major images: [tap][n / 16][k / 128][half][lane = fq * 16 + n % 16][16 bytes]
static inline size_t gemm_f8_wfrag_index(int n, int tap, int k, int N, int K) {
  const int kk = k & 127, j = gemm_f8_kslot_byte(kk);
  return ((((size_t)tap * (N >> 4) + (n >> 4)) * (K >> 7) + (k >> 7)) * 2 + (j >> 4)) * 1024 + (size_t)(gemm_f8_kslot_fq(kk) * 16 + (n & 15)) * 16 + (j & 15);
}

// the power of two s with amax * s in [224, 448) (1 for amax = 0 or a non-finite amax); 1 / s is exact
__host__ __device__ inline float f8_pow2_scale(float amax) {
  if (!(amax > 0.f && amax < 3.0e38f)) return 1.f;
  int e;
  const float m = frexpf(amax, &e); // amax = m 2^e, m in [0.5, 1)
  const int x = (m >= 0.875f ? 8 : 9) - e;
  return ldexpf(1.f, x < -120 ? -120 : x > 120 ? 120 : x);
}

// OCP e4m3 (1-4-3, bias 7, largest finite 448, no infinities), round to nearest even, saturating: the host's statement of v_cvt_pk_fp8_f32
static inline uint8_t f8_e4m3_encode(float f) {
  const uint8_t sign = std::signbit(f) ? 0x80 : 0;
  const float a = std::fabs(f);
  if (!(a == a)) return sign | 0x7f;
  if (a >= 448.0f) return sign | 0x7e;
  int e;
  (void)std::frexp(a, &e);
  const int ex = std::max(e - 1, -6);                  // subnormals share the exponent of the smallest normal
  const float q = std::ldexp(1.0f, ex - 3);            // spacing of the binade
  const float r = std::nearbyint(a / q) * q;           // default rounding mode: to nearest even
  if (r < 0.015625f) return sign | (uint8_t)std::lrint(r * 512.0f);
  (void)std::frexp(r, &e);
  return sign | (uint8_t)(((e - 1 + 7) << 3) | ((int)std::lrint(r / std::ldexp(1.0f, e - 4)) - 8));
}

// W [N][3][K] f32 (tap-major rows, as diff_load holds the fp16 weight) -> img [3 N K] bytes (gemm_f8_wfrag_index), inv_w [N]
static inline void gemm_f8_pack_weight(const float *W, int N, int K, uint8_t *img, float *inv_w) {
  for (int n = 0; n < N; n++) {
    float amax = 0.f;
    for (int i = 0; i < 3 * K; i++) amax = std::max(amax, std::fabs(W[(size_t)n * 3 * K + i]));
    const float s = f8_pow2_scale(amax);
    inv_w[n] = 1.0f / s;
    for (int tap = 0; tap < 3; tap++)
      for (int k = 0; k < K; k++) img[gemm_f8_wfrag_index(n, tap, k, N, K)] = f8_e4m3_encode(W[((size_t)n * 3 + tap) * K + k] * s);
  }
}

// ---- activation quantiser ----
static constexpr int F8_AMAX_PARTS = 32;
// grid (F8_AMAX_PARTS, sequences): part[s][p] = max over the 16-byte vectors p * 256 + t, + 256 F8_AMAX_PARTS, .. of sequence s of the bit pattern of |x| (fp16)
static __global__ __launch_bounds__(256) void quant_f8_amax_kernel(const __half *__restrict__ A, int lda, int Cn, const int *__restrict__ seq_start,
                                                                   const int *__restrict__ seq_len, unsigned *__restrict__ part) {
  __shared__ unsigned sh[4];
  const int s = blockIdx.y, r0 = seq_start[s], vec = Cn >> 3, nv = seq_len[s] * vec;
  unsigned lo = 0, hi = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nv; i += F8_AMAX_PARTS * 256) {
    const int r = i / vec, c = i - r * vec;
    const uint4 v = *(const uint4 *)(A + (size_t)(r0 + r) * lda + c * 8);
    const unsigned w[4] = {v.x & 0x7fff7fffu, v.y & 0x7fff7fffu, v.z & 0x7fff7fffu, v.w & 0x7fff7fffu};
#pragma unroll
    for (int q = 0; q < 4; q++) { lo = max(lo, w[q] & 0xffffu); hi = max(hi, w[q] >> 16); }
  }
  unsigned m = max(lo, hi);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[s * F8_AMAX_PARTS + blockIdx.x] = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}
// one work-group per aligned 8-row chunk of the M (multiple of 8) rows: sequences start at multiples of 8 rows, so a chunk has one owner, the sequence of its first
// row (row_seq < 0: guard rows only). A8[row][0 .. Cn) = e4m3(x * s_q), 0 for guard and pad rows; inv_a[row] = 1 / s_q, 0 for guard and pad rows
static __global__ __launch_bounds__(256) void quant_f8_convert_kernel(const __half *__restrict__ A, int lda, int Cn, const int *__restrict__ row_seq,
                                                                      const unsigned *__restrict__ part, uint8_t *__restrict__ A8, int lda8, float *__restrict__ inv_a) {
  __shared__ float sh_scale;
  const int row0 = blockIdx.x * 8, s = row_seq[row0], vec = Cn >> 3;
  if (threadIdx.x < 64) {
    unsigned m = (s >= 0 && threadIdx.x < F8_AMAX_PARTS) ? part[s * F8_AMAX_PARTS + threadIdx.x] : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if (threadIdx.x == 0) sh_scale = f8_pow2_scale(__half2float(__ushort_as_half((unsigned short)m)));
  }
  __syncthreads();
  const float sc = sh_scale;
  for (int i = threadIdx.x; i < 8 * vec; i += 256) {
    const int r = row0 + i / vec, c = i % vec;
    const bool live = s >= 0 && row_seq[r] >= 0;
    uint2 o = make_uint2(0u, 0u);
    if (live) {
      const uint4 v = *(const uint4 *)(A + (size_t)r * lda + c * 8);
      const __half2 *h = (const __half2 *)&v;
      const float2 f0 = __half22float2(h[0]), f1 = __half22float2(h[1]), f2 = __half22float2(h[2]), f3 = __half22float2(h[3]);
      int a = __builtin_amdgcn_cvt_pk_fp8_f32(f0.x * sc, f0.y * sc, 0, false);
      a = __builtin_amdgcn_cvt_pk_fp8_f32(f1.x * sc, f1.y * sc, a, true);
      int b = __builtin_amdgcn_cvt_pk_fp8_f32(f2.x * sc, f2.y * sc, 0, false);
      b = __builtin_amdgcn_cvt_pk_fp8_f32(f3.x * sc, f3.y * sc, b, true);
      o = make_uint2((unsigned)a, (unsigned)b);
    }
    *(uint2 *)(A8 + (size_t)r * lda8 + c * 8) = o;
    if (c == 0) inv_a[r] = live ? 1.0f / sc : 0.f;
  }
}

struct QuantF8Args {
  const __half *A; int lda;   // row 0 of the packed fp16 operand, halves per row (multiple of 8)
  int C, M, ns;               // channels (multiple of 8), rows (multiple of 8), sequences
  const int *seq_start, *seq_len, *row_seq; // device: [ns], [ns], [M]
  unsigned *part;             // device scratch [ns][F8_AMAX_PARTS]
  uint8_t *A8; int lda8;      // bytes per row (multiple of 8, >= C)
  float *inv_a;               // [M]
};
static inline bool quant_f8_ok(const QuantF8Args &q) {
  return q.A && q.A8 && q.inv_a && q.part && q.seq_start && q.seq_len && q.row_seq && q.C >= 8 && !(q.C & 7) && q.M >= 8 && !(q.M & 7) && q.ns >= 1 && q.ns <= 65535 &&
         q.lda >= q.C && !(q.lda & 7) && q.lda8 >= q.C && !(q.lda8 & 7);
}
static inline hipError_t launch_quant_f8_amax(const QuantF8Args &q, hipStream_t s) {
  if (!quant_f8_ok(q)) return hipErrorInvalidValue;
  quant_f8_amax_kernel<<<dim3(F8_AMAX_PARTS, q.ns), 256, 0, s>>>(q.A, q.lda, q.C, q.seq_start, q.seq_len, q.part);
  return hipGetLastError();
}
static inline hipError_t launch_quant_f8_convert(const QuantF8Args &q, hipStream_t s) {
  if (!quant_f8_ok(q)) return hipErrorInvalidValue;
  quant_f8_convert_kernel<<<q.M / 8, 256, 0, s>>>(q.A, q.lda, q.C, q.row_seq, q.part, q.A8, q.lda8, q.inv_a);
  return hipGetLastError();
}

// ---- the convolution ----
struct GemmF8Args {
  const uint8_t *A8; int lda; // row 0 of the e4m3 operand; bytes per row (multiple of 16, >= K); rows -1 .. M are readable (zero halo, as the fp16 operands)
  const uint8_t *Wf;          // the per-tap images (gemm_f8_wfrag_index)
  const float *inv_a, *inv_w; // [M], [N]
  const float *bias;          // [N] or nullptr
  const int *row_seq;         // [M]: < 0 for guard / pad rows (stored as 0), or nullptr
  float *out; int ldo;        // [M][ldo] (ldo multiple of 4, >= N); rows >= rows_total are not written
  const float *resid;         // [M][ldo] or nullptr; may alias out
  int M, rows_total, N, K;    // M, N, K multiples of 128; 1 <= rows_total <= M
};

static constexpr int GEMM_F8_SLOT = (128 + 8) * 128, GEMM_F8_LDS = 2 * GEMM_F8_SLOT;

template <int OFF> __device__ __forceinline__ void f8_wreg_load(intx4 &d, const uint8_t *base, unsigned voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(d) : "v"(voff), "s"(base), "i"(OFF));
}
template <int N> __device__ __forceinline__ void f8_wreg_wait(intx4 &a, intx4 &b, intx4 &c, intx4 &d) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "i"(N) : "memory");
}
__device__ __forceinline__ intx8 f8_join(const intx4 &lo, const intx4 &hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }

template <bool RESID>
static __global__ __launch_bounds__(256, 3) void gemm_f8_conv3_kernel(GemmF8Args g) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  char *smem = smem_dyn;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // Tile walk: work-group b runs on XCD b % 8. An XCD owns a contiguous range of row tiles and walks the column tiles of each innermost: its L2 keeps the 3 N K
  // bytes of the weight images (3 MB at N = K = 1024) while its eighth of the activations streams through once.
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, MT = g.M >> 7, NT = g.N >> 7;
  const int t0 = (MT * xcd) >> 3, t1 = (MT * (xcd + 1)) >> 3;
  if (idx >= (t1 - t0) * NT) return; // the grid is padded to 8 x the largest range
  const int mt = idx / NT, m0 = (t0 + mt) << 7, n0 = (idx - mt * NT) << 7;
  constexpr int MI = 8, NP = 2 * MI + 1, NPA = (NP + 3) / 4; // 8-row DMA pieces of a slab; pieces (= vmcnt events) per wave and chunk
  const int nchunks = g.K >> 7;
  const int fr = lane & 15, fq = lane >> 4;
  unsigned aoff[NPA]; // byte offsets from a wave-uniform base; slab rows past 129 (activation row m0 + 128, the last a tap reads) are clamped to it
#pragma unroll
  for (int i = 0; i < NPA; i++) {
    const int row = min(wave + 4 * i, NP - 1) * 8 + (lane >> 3);
    aoff[i] = (unsigned)(min(row, 16 * MI + 1) * g.lda + (((lane & 7) ^ lds_swz(row)) << 4));
  }
  const uint8_t *aseg = g.A8 + (ptrdiff_t)(m0 - 1) * g.lda; // slab row s = activation row m0 - 1 + s
  const size_t tap_stride = (size_t)g.N * g.K, nb_stride = (size_t)nchunks * 2048;
  const uint8_t *wp = g.Wf + (size_t)((n0 >> 4) + wave * 2) * nb_stride; // tap 0, this wave's first column block (wave-uniform)
  const unsigned wlane = lane * 16;
  floatx4 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
  // fragment read addresses: lds_off(16 i + fr + tap, 4 h + fq) = 2048 i + lds_off(fr + tap, 4 h + fq) (the swizzle has period 8 rows): one register per (tap, half),
  // block and slot are immediate offsets
  int fbase[3][2];
#pragma unroll
  for (int tap = 0; tap < 3; tap++)
#pragma unroll
    for (int h = 0; h < 2; h++) {
      fbase[tap][h] = lds_off(fr + tap, h * 4 + fq);
      asm volatile("" : "+v"(fbase[tap][h]));
    }
  intx4 w[2][2][2]; // [set][half][column block]
  auto issue_w = [&](int kc, int tap, auto set_c) {
    constexpr int U = decltype(set_c)::value;
    const uint8_t *q0 = wp + (size_t)tap * tap_stride + (size_t)min(kc, nchunks - 1) * 2048, *q1 = q0 + nb_stride; // past the last chunk: the last one again
    f8_wreg_load<0>(w[U][0][0], q0, wlane);
    f8_wreg_load<0>(w[U][0][1], q1, wlane);
    f8_wreg_load<1024>(w[U][1][0], q0, wlane);
    f8_wreg_load<1024>(w[U][1][1], q1, wlane);
  };
  auto issue_slab = [&](int kc, int slot) {
    const uint8_t *ab = aseg + (min(kc, nchunks - 1) << 7); // past the last chunk: the last one again, into the free slot (every phase counts the same vmcnt events)
    asm volatile("" : "+s"(ab));
#pragma unroll
    for (int i = 0; i < NPA; i++) {
      unsigned o = aoff[i];
      asm volatile("" : "+v"(o)); // scalar base + 32-bit lane offset
      __builtin_amdgcn_global_load_lds((gptr_t)(ab + o), (lptr_t)(smem + slot * GEMM_F8_SLOT + min(wave + 4 * i, NP - 1) * 1024), 16, 0, 0);
    }
  };
  // one phase: chunk kc (PAR = kc & 1 names its slab slot), tap TAP; no branch around a wait or a request
  auto phase = [&](int kc, auto par_c, auto tap_c) {
    constexpr int PAR = decltype(par_c)::value, TAP = decltype(tap_c)::value, U = PAR ^ (TAP & 1);
    f8_wreg_wait<TAP == 1 ? NPA : 0>(w[U][0][0], w[U][0][1], w[U][1][0], w[U][1][1]);
    if (TAP == 0) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // this wave's fragment reads of chunk kc - 1 are complete
      __builtin_amdgcn_s_barrier();
    }
    if (TAP < 2) issue_w(kc, TAP + 1, std::integral_constant<int, U ^ 1>{});
    else issue_w(kc + 1, 0, std::integral_constant<int, U ^ 1>{});
    if (TAP == 0) issue_slab(kc + 1, PAR ^ 1);
    const char *sa = smem + PAR * GEMM_F8_SLOT;
    const intx8 w0 = f8_join(w[U][0][0], w[U][1][0]), w1 = f8_join(w[U][0][1], w[U][1][1]);
    // activation fragments (two 16-byte reads each) one block ahead of the MFMA pair that consumes them
    intx4 lo[2], hi[2];
    lo[0] = *(const intx4 *)(sa + fbase[TAP][0]);
    hi[0] = *(const intx4 *)(sa + fbase[TAP][1]);
#pragma unroll
    for (int i = 0; i < MI; i++) {
      if (i + 1 < MI) {
        lo[(i + 1) & 1] = *(const intx4 *)(sa + fbase[TAP][0] + (i + 1) * 2048);
        hi[(i + 1) & 1] = *(const intx4 *)(sa + fbase[TAP][1] + (i + 1) * 2048);
      }
      const intx8 a = f8_join(lo[i & 1], hi[i & 1]);
      acc[i][0] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w0, a, acc[i][0], 0, 0, 0, 0, 0, 0);
      acc[i][1] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w1, a, acc[i][1], 0, 0, 0, 0, 0, 0);
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
  f8_wreg_wait<0>(w[0][0][0], w[0][0][1], w[0][1][0], w[0][1][1]);
  f8_wreg_wait<0>(w[1][0][0], w[1][0][1], w[1][1][0], w[1][1][1]);

  // epilogue: every load of a pair of blocks issued before its first store; unconditional loads through stand-in pointers, values selected afterwards (gemm_f16.h)
  const int col0 = n0 + wave * 32 + fq * 4;
  const bool hb = g.bias != nullptr, hs = g.row_seq != nullptr;
  const float *bp = hb ? g.bias : g.inv_w;
  const int *sp = hs ? g.row_seq : (const int *)g.inv_a;
  float4 iw[2], b4[2], rr[2][2];
  float ia[MI];
  int sq[MI];
  auto load_pair = [&](int p) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const float *rp = g.resid + (size_t)(m0 + (2 * p + q) * 16 + fr) * g.ldo + col0;
#pragma unroll
      for (int j = 0; j < 2; j++) rr[q][j] = *(const float4 *)(rp + j * 16);
    }
  };
  if (RESID) load_pair(0);
#pragma unroll
  for (int j = 0; j < 2; j++) { iw[j] = *(const float4 *)(g.inv_w + col0 + j * 16); b4[j] = *(const float4 *)(bp + col0 + j * 16); }
#pragma unroll
  for (int i = 0; i < MI; i++) { ia[i] = g.inv_a[m0 + i * 16 + fr]; sq[i] = sp[m0 + i * 16 + fr]; }
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
        float4 t = make_float4(acc[i][j][0] * (ia[i] * iw[j].x) + b4[j].x, acc[i][j][1] * (ia[i] * iw[j].y) + b4[j].y, acc[i][j][2] * (ia[i] * iw[j].z) + b4[j].z,
                               acc[i][j][3] * (ia[i] * iw[j].w) + b4[j].w);
        if (RESID) { t.x += rr[q][j].x; t.y += rr[q][j].y; t.z += rr[q][j].z; t.w += rr[q][j].w; }
        if (sq[i] < 0) t = make_float4(0.f, 0.f, 0.f, 0.f);
        v[q][j] = t;
      }
    }
    if (RESID && p + 1 < MI / 2) load_pair(p + 1);
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int row = m0 + (2 * p + q) * 16 + fr;
      if (row < g.rows_total) {
        float *op = g.out + (size_t)row * g.ldo + col0;
#pragma unroll
        for (int j = 0; j < 2; j++) *(float4 *)(op + j * 16) = v[q][j];
      }
    }
  }
}

// shapes the kernel is written for: whole 128 x 128 tiles over K chunks of 128
static inline bool gemm_f8_conv3_shape(int M, int N, int K) { return M >= 128 && N >= 128 && K >= 128 && !(M & 127) && !(N & 127) && !(K & 127); }
// Does a ResBlock's k = 3 convolution run on the fp8 path? Used by res_block (diffusion.hip) and by nothing else. Where it says no under conv3_fp8 = 1 the fp16
// path runs unchanged: latency-mode STATS epilogues, layouts whose GEMMs take tiles shorter than 128 rows (gemm_auto_th), the debug-checksum build.
static inline bool gemm_f8_conv3_takes(int conv3_fp8, bool images, bool stats, bool debug_sums, int M, int N, int K) {
  return conv3_fp8 == 1 && images && !stats && !debug_sums && gemm_f8_conv3_shape(M, N, K) && gemm_auto_th(M, N) == 8;
}
static inline int gemm_f8_conv3_grid(int M, int N) {
  const int MT = M >> 7;
  int mt_max = 0;
  for (int x = 0; x < 8; x++) mt_max = std::max(mt_max, ((MT * (x + 1)) >> 3) - ((MT * x) >> 3));
  return 8 * mt_max * (N >> 7);
}
static inline hipError_t launch_gemm_f8_conv3(const GemmF8Args &g, hipStream_t s) {
  if (!gemm_f8_conv3_shape(g.M, g.N, g.K) || !g.A8 || !g.Wf || !g.inv_a || !g.inv_w || !g.out || g.lda < g.K || (g.lda & 15) || g.ldo < g.N || (g.ldo & 3) ||
      g.rows_total < 1 || g.rows_total > g.M || g.M > (1 << 22))
    return hipErrorInvalidValue;
  const int grid = gemm_f8_conv3_grid(g.M, g.N);
  if (g.resid) gemm_f8_conv3_kernel<true><<<grid, 256, GEMM_F8_LDS, s>>>(g);
  else gemm_f8_conv3_kernel<false><<<grid, 256, GEMM_F8_LDS, s>>>(g);
  return hipGetLastError();
}

} // namespace tts
