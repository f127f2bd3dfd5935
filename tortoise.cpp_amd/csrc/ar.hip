// Autoregressive stage (GPT-2, 30 x 1024, 16 heads x 64) on gfx950.
//
// Replaces: autoregressive_model_load (main.cpp:482-897), autoregressive_graph (2545-3040),
// autoregressive_latent_graph (2053-2519) and the autoregressive() driver (5042-5367).
//
// Numerics follow the reference graph: F32 weights and F32 accumulation for every weight matmul,
// QKV activations rounded to fp16 (main.cpp:2789-2790) — so the KV cache is *stored* as fp16
// without changing a bit — F32 softmax, tanh-GELU, LayerNorm eps 1e-5.
//
// Decode is HBM-bound weight streaming: all weights are read exactly once per step for
// up to 16 candidates (split-K GEMV, deterministic two-level reduction, no atomics, so token ids
// are run-to-run reproducible). Layouts are fixed once at load time (the reference re-transposes
// every weight matrix inside every graph execution, main.cpp:2769-2777).
#include "common.h"
#include "gemm_f16.h"
#include <hip/hip_fp16.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "ar_score.h"

namespace tts {

static constexpr int D = 1024, NH = 16, HD = 64, FF = 4096, V = TTS_VOCAB_MEL, VPAD = 8256;

// LayerNorm-GEMV decode kernels: split-precision fp16 MFMA (default: three products per K step, operands carried to 2^-22 relative; f32 accumulation on top, see dec_ln_gemv_kernel) or exact-f32 MFMA
// products (option "dec_f32_mfma" = 1, read by tts_load_ar: it selects the weight packing; ArState::f32_mfma).
// Weight slabs of the decode step are streamed once per step by exactly one workgroup: non-temporal loads keep them from displacing the
// activations / KV rows in L2 (MI355X_MICROARCH.md, row "nt-weights"; measured 1 008 vs 1 036 us per step, profiles/r3_bench_n1.json).
typedef float ntfloat4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ float4 ldw4(const float4 *p) {
  if (!NT) return *p;
  const ntfloat4 v = __builtin_nontemporal_load((const ntfloat4 *)p);
  return make_float4(v[0], v[1], v[2], v[3]);
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float f16_round(float v) { return __half2float(__float2half_rn(v)); }

__device__ __forceinline__ float gelu_tanh(float x, int lut) {
  const float A = 0.044715f, S = 0.79788456080286535587989211986876f;
  if (lut) {
    float xr = f16_round(x);
    return f16_round(0.5f * xr * (1.0f + tanhf(S * xr * (1.0f + A * xr * xr))));
  }
  // tanh u = 1 - 2 / (1 + e^{2u}) on the hardware exp2/rcp (absolute error ~1e-7; libm's tanhf is ~40 instructions and
  // sits in the serial tail of the c_fc decode kernel)
  const float u = S * x * (1.0f + A * x * x);
  const float th = 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * 2.88539008177793f));
  return 0.5f * x * (1.0f + th);
}

// rows of the transformer input: out[r] = tabA[ia[r]] + tabB[ib[r]]  (ib < 0: no second term).
// tables: 0 voice(one row per voice of the batch), 1 text_emb, 2 mel_emb ; 0 text_pos, 1 mel_pos.
struct EmbedTables { const float *a[3]; const float *b[2]; };
__global__ __launch_bounds__(256) void embed_rows_kernel(EmbedTables t, const int4 *__restrict__ desc,
                                                         float *__restrict__ out) {
  const int r = blockIdx.x;
  const int4 d = desc[r]; // {tableA, idxA, tableB (-1 none), idxB}
  const float4 *pa = (const float4 *)(t.a[d.x] + (size_t)d.y * D);
  float4 v = pa[threadIdx.x];
  if (d.z >= 0) {
    const float4 *pb = (const float4 *)(t.b[d.z] + (size_t)d.w * D);
    float4 w = pb[threadIdx.x];
    v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
  }
  ((float4 *)(out + (size_t)r * D))[threadIdx.x] = v;
}

__device__ __forceinline__ float block_sum_256(float v, float *sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// LayerNorm over 1024 (ggml_norm eps 1e-5, then *g + b). One block (256 thr x float4) per row.
__global__ __launch_bounds__(256) void layernorm_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                        const float *__restrict__ b, float *__restrict__ y) {
  __shared__ float sh[4];
  const size_t row = blockIdx.x;
  float4 v = ((const float4 *)(x + row * D))[threadIdx.x];
  float mean = block_sum_256(v.x + v.y + v.z + v.w, sh) * (1.0f / D);
  v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
  float var = block_sum_256(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w, sh) * (1.0f / D);
  float sc = 1.0f / sqrtf(var + 1e-5f);
  float4 gg = ((const float4 *)g)[threadIdx.x], bb = ((const float4 *)b)[threadIdx.x];
  v.x = v.x * sc * gg.x + bb.x; v.y = v.y * sc * gg.y + bb.y;
  v.z = v.z * sc * gg.z + bb.z; v.w = v.w * sc * gg.w + bb.w;
  ((float4 *)(y + row * D))[threadIdx.x] = v;
}

// Split-K GEMV/skinny GEMM: part[ks][rows][N] = X[rows][k-chunk] * W[k-chunk][N].
// W is [K][N] row-major (N contiguous, N % 64 == 0). Block = 64 columns x one K chunk x RT rows;
// thread (cx = tid&15, ky = tid>>4) owns 4 columns and every 16th k of the chunk, so a wave's load
// instruction covers 4 consecutive W rows x 256 B. Reduction over ky: shuffles inside a wave, LDS
// across the 4 waves; the K chunks are summed in order by the epilogue kernel (deterministic).
// PRO = 1: the input is itself a split-K partial buffer and x[r][k] = gelu(sum_s pin[s][r][k] + bin[k]) is
// formed while staging (fuses the c_fc epilogue into the c_proj GEMV); X then points at pin, ldx = its N.
template <int RT, int PRO>
__global__ __launch_bounds__(256) void gemv_kn_kernel(const float *__restrict__ X, int ldx, int rows,
                                                      const float *__restrict__ W, int N, int K, int kspan,
                                                      float *__restrict__ part, int pin_ks, const float *__restrict__ pin_bias,
                                                      int lut) {
  __shared__ float xs[256 * RT];
  __shared__ float red[4 * RT * 64];
  const int tid = threadIdx.x, cx = tid & 15, ky = tid >> 4;
  const int r0 = blockIdx.z * RT;
  float acc[RT][4];
#pragma unroll
  for (int r = 0; r < RT; r++) { acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.f; }
  // the block's K range [blockIdx.y*kspan, +kspan) is staged through LDS in chunks of <= 256
  for (int k0 = blockIdx.y * kspan, kend = k0 + kspan; k0 < kend; k0 += 256) {
    const int kchunk = min(256, kend - k0);
    __syncthreads();
    for (int idx = tid; idx < kchunk * RT; idx += 256) {
      int r = idx / kchunk, k = idx - r * kchunk;
      float xv = 0.f;
      if (r0 + r < rows) {
        xv = X[(size_t)(r0 + r) * ldx + k0 + k];
        if (PRO) {
          for (int sp = 1; sp < pin_ks; sp++) xv += X[((size_t)sp * rows + r0 + r) * ldx + k0 + k];
          xv = gelu_tanh(xv + pin_bias[k0 + k], lut);
        }
      }
      xs[k * RT + r] = xv;
    }
    __syncthreads();
    const float *wp = W + ((size_t)blockIdx.x * K + k0 + ky) * 64 + cx * 4; // strip-major [N/64][K][64]
#pragma unroll 4
    for (int k = ky; k < kchunk; k += 16) {
      const float4 w = *(const float4 *)wp;
      wp += 16 * 64;
#pragma unroll
      for (int r = 0; r < RT; r++) {
        const float xv = xs[k * RT + r];
        acc[r][0] = fmaf(xv, w.x, acc[r][0]); acc[r][1] = fmaf(xv, w.y, acc[r][1]);
        acc[r][2] = fmaf(xv, w.z, acc[r][2]); acc[r][3] = fmaf(xv, w.w, acc[r][3]);
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int r = 0; r < RT; r++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float v = acc[r][j];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (lane < 16) red[(wave * RT + r) * 64 + cx * 4 + j] = v;
    }
  __syncthreads();
  for (int idx = tid; idx < RT * 16; idx += 256) {
    int r = idx >> 4, c4 = idx & 15;
    if (r0 + r < rows) {
      float4 s;
      const float *p0 = &red[(0 * RT + r) * 64 + c4 * 4], *p1 = &red[(1 * RT + r) * 64 + c4 * 4];
      const float *p2 = &red[(2 * RT + r) * 64 + c4 * 4], *p3 = &red[(3 * RT + r) * 64 + c4 * 4];
      s.x = ((p0[0] + p1[0]) + p2[0]) + p3[0]; s.y = ((p0[1] + p1[1]) + p2[1]) + p3[1];
      s.z = ((p0[2] + p1[2]) + p2[2]) + p3[2]; s.w = ((p0[3] + p1[3]) + p2[3]) + p3[3];
      *(float4 *)&part[((size_t)blockIdx.y * rows + r0 + r) * N + blockIdx.x * 64 + c4 * 4] = s;
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Split-precision MFMA path for the multi-row passes (prefill, latent pass): x*W in f32 is evaluated as
// x_hi*W_hi + x_lo*W_hi + x_hi*W_lo with fp16 hi/lo parts (hi = fp16(v), lo = fp16(v - hi): 22 significant
// bits) on the fp16 MFMA GEMM with f32 accumulation — ~16x the f32 FMA rate at ~2^-21 relative accuracy
// (the oracle gate for these passes is 1e-4). Weights are pre-scaled by 64 so the lo parts stay normal.
// ---------------------------------------------------------------------------------------------
static constexpr float W16_SCALE = 64.0f;
// W f32 strip-major [N/64][K][64] -> out fp16 [N][2K] = [hi(0..K-1) | lo(0..K-1)] of 64*W^T (tile transpose through LDS)
__global__ __launch_bounds__(256) void split_weight_kernel(const float *__restrict__ W, int K, int N, __half *__restrict__ out) {
  __shared__ float t[32][33];
  const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) t[r][tx] = W[((size_t)(n0 >> 6) * K + k0 + r) * 64 + (n0 & 63) + tx] * W16_SCALE; // strip-major source
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const float v = t[tx][r];
    const __half hi = __float2half_rn(v);
    const __half lo = __float2half_rn(v - __half2float(hi));
    out[(size_t)(n0 + r) * 2 * K + k0 + tx] = hi;
    out[(size_t)(n0 + r) * 2 * K + K + k0 + tx] = lo;
  }
}

// ---- load-time weight layouts: one index map per layout, shared by the host packers and the device kernels ------------------------------
// Every layout below is a permutation of a weight matrix w [K][N] (N contiguous) plus at most one rounding per element. Each is written once, as a function from an
// output offset to the source element, and applied twice: by the host packers (ArLoader, options load_device_pack = 0 / load_threads = 1 and the A/B slab options) in a loop
// over the output, and by the pk_* kernels (the default: a worker uploads a tensor as it lies in the file and the layouts are produced from that copy; tts_load_ar spent
// 5.9 s in the host loops on one core and still 0.5 s on sixteen). Same arithmetic per element on both sides (f32 multiply by the LayerNorm gain, exact scaling by 64,
// round-to-nearest-even fp16 hi / lo, the double-precision column sums of the folded bias in ascending k): the buffers are equal byte for byte
// (tests/test_ar_gpu.py compares the logits of the loads bit for bit).
struct WAt { size_t k, n; }; // source element w[k][n]
// strip-major: 64-column strips, [N/64][K][64], so that the K-chunk a GEMV workgroup streams is ONE contiguous region and a wave's load instruction covers 1 KB of
// consecutive bytes (the reference re-transposes every matrix in every graph execution; here the layout is chosen once). 64 consecutive offsets are 64 consecutive sources.
__host__ __device__ __forceinline__ WAt strip_major_at(size_t o, int K, int N) {
  const size_t s0 = o / ((size_t)K * 64), rem = o % ((size_t)K * 64);
  return {rem / 64, s0 * 64 + rem % 64};
}
// mfma16 (decode step, K = 1024, f32): slab of workgroup cb (16 columns) = 4 waves x 16 groups x 64 lanes x float4, where lane (m = lane & 15, q = lane >> 4) of wave wv
// holds W[256 wv + 16 g + 4 q + j][16 cb + m], j = 0..3, for group g.
__host__ __device__ __forceinline__ WAt mfma16_at(size_t o) {
  const size_t j = o & 3, lane = (o >> 2) & 63, g = (o >> 8) & 15, wv = (o >> 12) & 3, cb = o >> 14;
  return {wv * 256 + g * 16 + 4 * (lane >> 4) + j, cb * 16 + (lane & 15)};
}
// mfma16h (decode step, K = 1024, the fp16 family): the same slab for the fp16 MFMAs. Lane (m, q) of wave wv holds for K step s (32 k) the 8 values
// k = 256 wv + 32 s + 8 q + e of column 16 cb + m: element i = (((cb 4 + wv) 8 + s) 64 + lane) 8 + e of the K N. Three encodings of that one order:
//   fp16(64 w) at slot i, 16 contiguous bytes per lane and K step (option ar_weights = 1);
//   split precision (the default): 8 fp16 hi at slot hilo, then 8 fp16 lo at hilo + 8 (hi = fp16(64 w), lo = fp16(64 w - hi)): 32 contiguous bytes per lane, 2 KB per
//   wave and step;
//   one e4m3 BYTE per value at slot fp8 (option ar_weights = 2): a lane's K steps 2 t and 2 t + 1 share one 16-byte load, byte ((((cb 4 + wv) 4 + t) 64 + lane) 2 + (s & 1)) 8 + e.
struct Mfma16hAt { size_t k, n, hilo, fp8; };
__host__ __device__ __forceinline__ Mfma16hAt mfma16h_at(size_t i) {
  const size_t e = i & 7, lane = (i >> 3) & 63, s = (i >> 9) & 7, wv = (i >> 12) & 3, cb = i >> 14;
  return {wv * 256 + s * 32 + 8 * (lane >> 4) + e, cb * 16 + (lane & 15), (i >> 3) * 16 + e, ((((cb * 4 + wv) * 4 + (s >> 1)) * 64 + lane) * 2 + (s & 1)) * 8 + e};
}
// cols4 (decode step, K = 1024 KG): slab of workgroup cb (4 columns) = KG x 4 x 256 threads x 4 values (the 4 columns: a float4, 4 fp16 or 4 e4m3 bytes), thread t
// holding k = 1024 i + 4 t + kk.
__host__ __device__ __forceinline__ WAt cols4_at(size_t o, int K) {
  const unsigned c = o & 3, tid = (o >> 2) & 255, kk = (o >> 10) & 3, q = (unsigned)(o >> 12), KG = K / 1024; // q = cb KG + i
  return {(size_t)(q % KG) * 1024 + 4 * tid + kk, (size_t)(q / KG) * 4 + c};
}
// the split-precision pair of 64 w
struct HiLo { __half hi, lo; };
__host__ __device__ __forceinline__ HiLo split_hilo(float w) {
  const float v = W16_SCALE * w;
  const __half hi = __float2half_rn(v);
  return {hi, __float2half_rn(v - __half2float(hi))};
}

__global__ __launch_bounds__(256) void pk_strip_major_kernel(const float *__restrict__ w, int K, int N, float *__restrict__ t) {
  const size_t total = (size_t)K * N;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
    const WAt a = strip_major_at(o, K, N);
    t[o] = w[a.k * N + a.n];
  }
}
__global__ __launch_bounds__(256) void pk_fold_kernel(const float *__restrict__ w, int K, int N, const float *__restrict__ g, float *__restrict__ wf) {
  const size_t total = (size_t)K * N;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) wf[o] = g[o / N] * w[o];
}
// cf[n] = float(double(c[n]) + sum_k double(b[k]) double(w[k][n])), k ascending (a product of two floats is exact in double: fused or not, the same sum)
__global__ __launch_bounds__(256) void pk_fold_bias_kernel(const float *__restrict__ w, int K, int N, const float *__restrict__ b, const float *__restrict__ c,
                                                           float *__restrict__ cf) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double acc = 0.0;
  for (int k0 = 0; k0 < K; k0 += 16) { // 16 independent loads in flight, then the 16 additions in ascending k (a first version waited for every load: 280 us per launch)
    float wv[16];
#pragma unroll
    for (int j = 0; j < 16; j++) wv[j] = k0 + j < K ? w[(size_t)(k0 + j) * N + n] : 0.f;
#pragma unroll
    for (int j = 0; j < 16; j++)
      if (k0 + j < K) acc += (double)b[k0 + j] * (double)wv[j];
  }
  cf[n] = (float)((double)c[n] + acc);
}
// the split-precision mfma16h slab: one thread per weight (K = 1024)
__global__ __launch_bounds__(256) void pk_mfma16h_kernel(const float *__restrict__ w, int N, __half *__restrict__ t) {
  const size_t total = (size_t)1024 * N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const Mfma16hAt a = mfma16h_at(i);
    const HiLo v = split_hilo(w[a.k * N + a.n]);
    t[a.hilo] = v.hi;
    t[a.hilo + 8] = v.lo;
  }
}
__global__ __launch_bounds__(256) void pk_cols4_kernel(const float *__restrict__ w, int K, int N, float *__restrict__ t) {
  const size_t total = (size_t)K * N;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
    const WAt a = cols4_at(o, K);
    t[o] = w[a.k * N + a.n];
  }
}
// nn.Linear [V][D] -> [D][VPAD], zero padded
__global__ __launch_bounds__(256) void pk_transpose_pad_kernel(const float *__restrict__ w, int rowsV, int colsD, int vpad, float *__restrict__ wt) {
  const size_t total = (size_t)colsD * vpad;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
    const size_t k = o / vpad, n = o % vpad;
    wt[o] = n < (size_t)rowsV ? w[n * colsD + k] : 0.f;
  }
}
// max |w| into *out (bits of a non-negative float order like unsigned integers; a NaN ends up above every number and fails the range check loudly)
__global__ __launch_bounds__(256) void pk_absmax_kernel(const float *__restrict__ w, size_t n, unsigned *__restrict__ out) {
  __shared__ unsigned wm[4];
  unsigned m = 0;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (size_t)gridDim.x * 256) m = max(m, __float_as_uint(fabsf(w[o])));
  for (int off = 32; off; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) { // one atomic per workgroup (32 K waves hitting one address took 340 us per launch)
    m = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
    if (m) atomicMax(out, m);
  }
}
// x f32 [rows][K] -> hi, lo fp16 [rows_pad][K] (pad rows zero)
__global__ __launch_bounds__(256) void split_act_kernel(const float *__restrict__ x, int rows, int K, __half *__restrict__ hi,
                                                        __half *__restrict__ lo) {
  const int r = blockIdx.x;
  for (int c = threadIdx.x * 4; c < K; c += 1024) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) v = *(const float4 *)(x + (size_t)r * K + c);
    const __half2 h0 = __floats2half2_rn(v.x, v.y), h1 = __floats2half2_rn(v.z, v.w);
    const float2 f0 = __half22float2(h0), f1 = __half22float2(h1);
    const __half2 l0 = __floats2half2_rn(v.x - f0.x, v.y - f0.y), l1 = __floats2half2_rn(v.z - f1.x, v.w - f1.y);
    uint2 uh, ul;
    uh.x = *(const unsigned *)&h0; uh.y = *(const unsigned *)&h1;
    ul.x = *(const unsigned *)&l0; ul.y = *(const unsigned *)&l1;
    *(uint2 *)(hi + (size_t)r * K + c) = uh;
    *(uint2 *)(lo + (size_t)r * K + c) = ul;
  }
}

enum { EPI_BIAS = 0, EPI_QKV = 1, EPI_GELU = 2, EPI_RESID = 3 };
struct KvDst {          // where EPI_QKV writes K/V as fp16
  __half *k, *v;        // base of this layer's cache: [cand][max_pos][1024]
  int S;                // positions per candidate in this launch (row = cand*S + s)
  int n_past, max_pos;
  int replicate;        // >0: the single candidate's rows are written for `replicate` candidates
};
// out[r][n] = epilogue(sum_s part[s][r][n] + bias[n]); one block per row, columns strided by 256.
template <int MODE>
__global__ __launch_bounds__(256) void epilogue_kernel(const float *__restrict__ part, int ks, int rows, int N,
                                                       int n_valid, const float *__restrict__ bias,
                                                       float *__restrict__ out, int ldo, KvDst kv, int lut, float pscale) {
  const int r = blockIdx.x;
  for (int n = blockIdx.y * 256 + threadIdx.x; n < n_valid; n += 256 * gridDim.y) {
    float v = part[(size_t)r * N + n];
    for (int s = 1; s < ks; s++) v += part[((size_t)s * rows + r) * N + n];
    v = v * pscale + bias[n]; // pscale = 1 (f32 path) or 1/64 (split-precision weights are pre-scaled; exact power of 2)
    if (MODE == EPI_QKV) {
      // the f32 sum is a value of its own, as in the reference (f32 add, then the fp16 conversion): without the empty asm hipcc fuses the FMA and the
      // conversion into v_fma_mixlo_f16, which rounds the exact sum ONCE to fp16 and lands on the other neighbour at about half of the f32 ties
      asm volatile("" : "+v"(v));
      v = f16_round(v);
      out[(size_t)r * ldo + n] = v;
      if (n >= D) {
        const int c = r / kv.S, s = r - c * kv.S, pos = kv.n_past + s;
        __half hv = __float2half_rn(v);
        __half *base = (n < 2 * D) ? kv.k : kv.v;
        const int ch = (n < 2 * D) ? n - D : n - 2 * D;
        if (kv.replicate > 0) {
          for (int cc = 0; cc < kv.replicate; cc++) base[((size_t)cc * kv.max_pos + pos) * D + ch] = hv;
        } else {
          base[((size_t)c * kv.max_pos + pos) * D + ch] = hv;
        }
      }
    } else if (MODE == EPI_GELU) {
      out[(size_t)r * ldo + n] = gelu_tanh(v, lut);
    } else if (MODE == EPI_RESID) {
      out[(size_t)r * ldo + n] += v;
    } else {
      out[(size_t)r * ldo + n] = v;
    }
  }
}

// EPI_QKV of the split-precision path (ks = 1, pscale = 1 / 64) for a packed row space in which every row names its own cache row (ar_session_extend):
// row r's K and V go to cache row row_dst[r] = slot * max_pos + position. The arithmetic is epilogue_kernel<EPI_QKV>'s.
__global__ __launch_bounds__(256) void epilogue_qkv_ragged_kernel(const float *__restrict__ part, const float *__restrict__ bias, float *__restrict__ out,
                                                                  const int *__restrict__ row_dst, __half *__restrict__ kdst, __half *__restrict__ vdst,
                                                                  float pscale) {
  const int r = blockIdx.x;
  const size_t dst = (size_t)row_dst[r] * D;
  for (int n = blockIdx.y * 256 + threadIdx.x; n < 3 * D; n += 256 * gridDim.y) {
    float v = part[(size_t)r * 3 * D + n];
    v = v * pscale + bias[n];
    asm volatile("" : "+v"(v)); // as epilogue_kernel<EPI_QKV>: round to f32, then to fp16
    v = f16_round(v);
    out[(size_t)r * 3 * D + n] = v;
    if (n >= D) {
      __half *base = (n < 2 * D) ? kdst : vdst;
      base[dst + ((n < 2 * D) ? n - D : n - 2 * D)] = __float2half_rn(v);
    }
  }
}

// Causal attention of the multi-row passes (latent pass: 16 candidates x ~200 rows x 16 heads), default (non-LUT) numerics. One workgroup per
// (candidate, head, block of 64 rows): lane = row, and the four waves split the KEYS (wave w takes the groups of 8 keys w, w + 4, ..) so that every SIMD
// holds several waves to hide the LDS latency (one thread per row alone is < 1 wave per SIMD at 3 216 rows). The keys are staged through LDS in chunks of
// 128 (K and V rows of the head, 128 B each: 32 KB per chunk) and walked with wave-uniform LDS addresses (broadcast reads, no bank conflicts): q.k on
// v_dot2_f32_f16 (q is the fp16-rounded query, so the products are exact and the sum is f32), online softmax per group of 8 keys (one rescale of the 64
// accumulators per group), p.V on v_fma_mix_f32 (f32 weight x fp16 V, f32 accumulate). The four partial states (m, l, acc[64]) are merged through LDS.
// Same arithmetic class as attention_kernel below (f32 weights, f32 accumulation; only the summation order and exp2 vs expf differ), which needed one wave
// per (row, head) and re-read every K/V row from L2 per row: 225 us per layer at 3 216 rows.
typedef _Float16 ar_half2 __attribute__((ext_vector_type(2)));
// The workgroup's work, shared by attention_rows_kernel and attention_rows_ragged_kernel: rows s0 .. s0 + 63 of one sequence of S rows that sits n_past keys
// into its cache. q: the sequence's first row in the qkv buffer at the head's columns (row stride 3 * D), kb / vb: key 0 of the sequence's cache at the head's
// columns, o_rows: the sequence's first output row at the head's columns. A row's bits depend on its own query and the keys before it only: the keys are walked
// from absolute position 0 in chunks of 128 and groups of 8 whatever S, n_past and s0 are.
__device__ __forceinline__ void attention_rows_block(const float *__restrict__ q, const __half *__restrict__ kb, const __half *__restrict__ vb,
                                                     float *__restrict__ o_rows, int S, int n_past, int s0) {
  constexpr int CH = 128; // keys per LDS chunk: 32 KB of LDS, three workgroups per CU (the registers allow three waves per SIMD)
  constexpr float L2E = 1.4426950408889634f;
  __shared__ __attribute__((aligned(16))) __half kvs[2 * CH * HD]; // K chunk | V chunk; reused for the merge: acc[wave][32 dims][lane], two passes
  __shared__ float wm[4][64], wl[4][64];
  __half *ks = kvs, *vs = kvs + CH * HD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = s0 + lane;
  const bool live = s < S;
  const int nk = live ? n_past + s + 1 : 0;         // keys this row sees (ggml_diag_mask_inf(n_past))
  const int nk_block = n_past + min(S, s0 + 64);     // keys the block's last row sees
  ar_half2 q2[HD / 2];
  {
    const float *qp = q + (size_t)(live ? s : S - 1) * 3 * D;
#pragma unroll
    for (int i = 0; i < HD / 4; i++) {
      const float4 f = ((const float4 *)qp)[i];
      q2[2 * i] = (ar_half2){(_Float16)f.x, (_Float16)f.y};
      q2[2 * i + 1] = (ar_half2){(_Float16)f.z, (_Float16)f.w};
    }
  }
  float m = -INFINITY, l = 0.f, acc[HD];
#pragma unroll
  for (int d = 0; d < HD; d++) acc[d] = 0.f;
  for (int j0 = 0; j0 < nk_block; j0 += CH) {
    const int nch = min(CH, nk_block - j0), nch8 = (nch + 7) & ~7;
    __syncthreads(); // the previous chunk has been consumed
    // stage K and V rows j0 .. j0 + nch: 8 threads per row, 16 bytes each (a row of the head = 128 contiguous bytes); the rows that fill the last
    // group of 8 are zeroed (their weights are exp2(-inf) = 0, and 0 x stale LDS bits could be 0 x inf)
    for (int r = tid >> 3; r < nch8; r += 32) {
      const size_t g = (size_t)(j0 + r) * D + (tid & 7) * 8;
      uint4 ku = make_uint4(0u, 0u, 0u, 0u), vu = ku;
      if (r < nch) { ku = *(const uint4 *)(kb + g); vu = *(const uint4 *)(vb + g); }
      *(uint4 *)(ks + r * HD + (tid & 7) * 8) = ku;
      *(uint4 *)(vs + r * HD + (tid & 7) * 8) = vu;
    }
    __syncthreads();
    for (int jg = wave * 8; jg < nch; jg += 32) {
      float sc[8];
      float gmax = m;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const ar_half2 *kr = (const ar_half2 *)(ks + (jg + e) * HD);
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int i = 0; i < HD / 2; i += 2) {
          d0 = __builtin_amdgcn_fdot2(q2[i], kr[i], d0, false);
          d1 = __builtin_amdgcn_fdot2(q2[i + 1], kr[i + 1], d1, false);
        }
        const float v = (j0 + jg + e < nk) ? (d0 + d1) * 0.125f : -INFINITY; // 1/sqrt(64)
        sc[e] = v;
        gmax = fmaxf(gmax, v);
      }
      if (gmax == -INFINITY) continue; // nothing visible to this row yet (or a row past S)
      const float resc = __builtin_amdgcn_exp2f((m - gmax) * L2E); // m = -inf -> 0
      l *= resc;
#pragma unroll
      for (int d = 0; d < HD; d++) acc[d] *= resc;
      m = gmax;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const float pw = __builtin_amdgcn_exp2f((sc[e] - gmax) * L2E); // masked key: exp2(-inf) = 0
        l += pw;
        // acc[d] += pw * V[d] with V read as fp16 by the FMA itself (v_fma_mix_f32: no conversion instructions; hipcc emits cvt + packed FMA otherwise)
        const uint4 *vr = (const uint4 *)(vs + (jg + e) * HD);
#pragma unroll
        for (int i = 0; i < HD / 8; i++) {
          const uint4 u = vr[i];
          const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
          for (int k = 0; k < 4; k++) {
            asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,0]" : "+v"(acc[8 * i + 2 * k]) : "v"(pw), "v"(w[k]));
            asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(acc[8 * i + 2 * k + 1]) : "v"(pw), "v"(w[k]));
          }
        }
      }
    }
  }
  // merge the four waves' partial states of every row (fixed order: wave 0 .. 3)
  __syncthreads(); // the last chunk has been consumed: its LDS becomes the exchange buffer
  float *xa = (float *)kvs; // [wave][32 dims][lane]: 32 KB, dims 0-31 then dims 32-63
  wm[wave][lane] = m; wl[wave][lane] = l;
  float o[16]; // this wave finishes dims 16 wave .. 16 wave + 15 of all 64 rows
#pragma unroll
  for (int half = 0; half < 2; half++) {
    if (half) __syncthreads();
#pragma unroll
    for (int d = 0; d < 32; d++) xa[(wave * 32 + d) * 64 + lane] = acc[half * 32 + d];
    __syncthreads();
    if ((wave >> 1) == half) { // waves 0, 1 own dims 0-31, waves 2, 3 dims 32-63
      const float M = fmaxf(fmaxf(wm[0][lane], wm[1][lane]), fmaxf(wm[2][lane], wm[3][lane])); // wave 0 holds key 0 of every live row: finite
      float f[4], tot = 0.f;
#pragma unroll
      for (int w = 0; w < 4; w++) {
        f[w] = __builtin_amdgcn_exp2f((wm[w][lane] - M) * L2E); // a wave that saw no key: exp2(-inf) = 0
        tot = fmaf(f[w], wl[w][lane], tot);
      }
      const float inv = 1.0f / tot;
#pragma unroll
      for (int d = 0; d < 16; d++) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 4; w++) t = fmaf(f[w], xa[(w * 32 + (wave & 1) * 16 + d) * 64 + lane], t);
        o[d] = t * inv;
      }
    }
  }
  if (!live) return;
  float *op = o_rows + (size_t)s * D + wave * 16;
#pragma unroll
  for (int i = 0; i < 4; i++) ((float4 *)op)[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}
__global__ __launch_bounds__(256) void attention_rows_kernel(const float *__restrict__ qkv, const __half *__restrict__ kc,
                                                             const __half *__restrict__ vc, float *__restrict__ out, int S, int n_past,
                                                             int max_pos) {
  const int c = blockIdx.x, h = blockIdx.y;
  attention_rows_block(qkv + (size_t)c * S * 3 * D + h * HD, kc + (size_t)c * max_pos * D + h * HD, vc + (size_t)c * max_pos * D + h * HD,
                       out + (size_t)c * S * D + h * HD, S, n_past, blockIdx.z * 64);
}
// The ragged form (ar_session_extend): sequence i of the launch is items[i] = {first row in the packed row space, S, n_past, cache slot}: its S new rows sit
// n_past keys into slot's cache, whose earlier rows were written by earlier passes. grid (n_items, NH, ceil(longest S / 64)): a block past its own sequence's
// rows leaves before any barrier.
__global__ __launch_bounds__(256) void attention_rows_ragged_kernel(const float *__restrict__ qkv, const __half *__restrict__ kc,
                                                                    const __half *__restrict__ vc, float *__restrict__ out,
                                                                    const int4 *__restrict__ items, int max_pos) {
  const int4 it = items[blockIdx.x];
  const int h = blockIdx.y, s0 = blockIdx.z * 64;
  if (s0 >= it.y) return;
  attention_rows_block(qkv + (size_t)it.x * 3 * D + h * HD, kc + (size_t)it.w * max_pos * D + h * HD, vc + (size_t)it.w * max_pos * D + h * HD,
                       out + (size_t)it.x * D + h * HD, it.y, it.z, s0);
}

// Causal attention for one (row, head): q from the f16-rounded qkv buffer, K/V from an fp16 cache
// [cand][max_pos][1024]. Row r = cand*S + s sees keys 0 .. n_past+s (ggml_diag_mask_inf(n_past)).
// One wave per (row, head). Scores in LDS (<= 1024 keys).
__global__ __launch_bounds__(64) void attention_kernel(const float *__restrict__ qkv, const __half *__restrict__ kc,
                                                       const __half *__restrict__ vc, float *__restrict__ out, int S,
                                                       int n_past, int max_pos, int lut) {
  __shared__ float sc[1024];
  __shared__ float qs[HD];
  const int r = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  const int c = r / S, s = r - c * S;
  const int nk = n_past + s + 1;
  qs[lane] = qkv[(size_t)r * 3 * D + h * HD + lane];
  __syncthreads();
  const __half *kb = kc + (size_t)c * max_pos * D + h * HD;
  float mx = -INFINITY;
  for (int j = lane; j < nk; j += 64) {
    const uint4 *kp = (const uint4 *)(kb + (size_t)j * D);
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      uint4 u = kp[q];
      const __half2 *h2 = (const __half2 *)&u;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float2 f = __half22float2(h2[e]);
        dot = fmaf(qs[q * 8 + e * 2], f.x, dot);
        dot = fmaf(qs[q * 8 + e * 2 + 1], f.y, dot);
      }
    }
    dot *= 0.125f; // 1/sqrt(64)
    sc[j] = dot;
    mx = fmaxf(mx, dot);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.f;
  for (int j = lane; j < nk; j += 64) {
    float e = lut ? f16_round(expf(f16_round(sc[j] - mx))) : expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  __syncthreads();
  const float inv = 1.0f / sum;
  const __half *vb = vc + (size_t)c * max_pos * D + h * HD + lane;
  float acc = 0.f;
  for (int j = 0; j < nk; j++) acc = fmaf(sc[j] * inv, __half2float(vb[(size_t)j * D]), acc);
  out[(size_t)r * D + h * HD + lane] = acc;
}


// ---------------------------------------------------------------------------------------------
// Decode-step kernels (one new position per candidate). The step is captured in a hipGraph: the
// position counters live in device memory so the same graph is replayed for every step.
// ---------------------------------------------------------------------------------------------
struct StepState { int n_past; int pos_id; };
// index of (candidate r, channel k) in the decode step's interleaved residual-stream layout h4 (described in front of the decode kernels)
__host__ __device__ __forceinline__ size_t h4_index(int r, int k) { return ((((size_t)(r >> 4) * 256 + (k >> 2)) * 16 + (r & 15)) << 2) + (k & 3); }

// First kernel of the decode step. `host_step` is the PINNED HOST block [tokens[B] | n_past, pos_id] the host fills before it launches the graph: the kernel
// reads it over PCIe (one ~2 us round trip inside a kernel that has nothing else to wait for) and block 0 leaves the step state in device memory for
// the 150 launches behind it — instead of a host-to-device copy node in front of the graph (a 5 us blit kernel + a launch boundary per step).
__global__ __launch_bounds__(256) void embed_step_kernel(const float *__restrict__ mel_emb, const float *__restrict__ mel_pos,
                                                         const int *__restrict__ host_step, int B, StepState *__restrict__ ss_out,
                                                         float *__restrict__ h4) {
  const int r = blockIdx.x;
  const int tok = host_step[r], n_past = host_step[B], pos_id = host_step[B + 1];
  if (r == 0 && threadIdx.x == 0) { ss_out->n_past = n_past; ss_out->pos_id = pos_id; }
  const float4 a = ((const float4 *)(mel_emb + (size_t)tok * D))[threadIdx.x];
  const float4 b = ((const float4 *)(mel_pos + (size_t)pos_id * D))[threadIdx.x];
  *(float4 *)(h4 + h4_index(r, 4 * threadIdx.x)) = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); // h4 layout, see below
}

// The same kernel for a session step (tts_ar_session_step): every row is at its own step. The pinned host block is [tokens[B] | n_past[Bpad] | pos_id[B]]
// (Bpad = B in whole tiles of 16). Block r's three words have workgroup-uniform addresses: three independent scalar loads issued together, the one PCIe
// round trip of the kernel above. Block r leaves its context length in row_off[r], the array the RO kernels behind it add to the step state's n_past,
// which block 0 sets to 0. The tile padding of row_off (rows B .. Bpad) was zeroed when the session was opened and is never written.
__global__ __launch_bounds__(256) void embed_session_kernel(const float *__restrict__ mel_emb, const float *__restrict__ mel_pos,
                                                            const int *__restrict__ host_step, int B, int Bpad, StepState *__restrict__ ss_out,
                                                            int *__restrict__ row_off, float *__restrict__ h4) {
  const int r = blockIdx.x;
  const int tok = host_step[r], n_past = host_step[B + r], pos_id = host_step[B + Bpad + r];
  // (the empty asm wants all three in SGPRs HERE: left alone, hipcc sinks n_past's load into the branch below, a second dependent round trip for wave 0)
  asm volatile("" ::"s"(tok), "s"(n_past), "s"(pos_id));
  if (threadIdx.x == 0) {
    row_off[r] = n_past;
    if (r == 0) { ss_out->n_past = 0; ss_out->pos_id = 0; }
  }
  const float4 a = ((const float4 *)(mel_emb + (size_t)tok * D))[threadIdx.x];
  const float4 b = ((const float4 *)(mel_pos + (size_t)pos_id * D))[threadIdx.x];
  *(float4 *)(h4 + h4_index(r, 4 * threadIdx.x)) = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// Round 4 — the residual stream of the DECODE step lives in an interleaved layout, `h4`:
//     element (candidate r, channel k)  ->  h4[r / 16][k / 4][r % 16][k % 4]       (16-byte groups of 4 channels, the 16 candidates of a tile adjacent)
// The LayerNorm-GEMV kernels feed the activations to the matrix pipe as the B operand: lane (m = candidate, q) holds 8 consecutive channels, so with the
// natural [r][1024] layout one wave-level load touched 16 rows x 64 B — sixteen half-used cache lines per instruction, twice each. That is the pattern
// cdna_hip_programming.md warns about ("fragment-shaped loads (16 rows x 64 B per instruction) straight to VGPRs ... TA_BUSY 2x") and the per-launch trace
// shows its price: ~3 us until the 64 KB of activations are in, against <1 us for the same 64 KB read as 1 KB-contiguous instructions by
// dec_gemv_resid_kernel (profiles/r4_decode_launch_breakdown.txt). In h4 the same instruction covers 4 x 256 contiguous bytes = 8 full lines, nothing twice;
// the projection kernels' 64 outputs per workgroup (16 candidates x 4 columns) become ONE contiguous 256-byte block. The prompt pass keeps [row][1024].

// ---- decode step: five launches per layer, no split-K partials ---------------------------------------
// Every weight matrix is packed at load for the workgroup that streams it (one contiguous slab per
// workgroup, every wave-level load instruction 1 KB of consecutive bytes) and every launch writes COMPLETE
// outputs, so LayerNorm, bias, GELU, the fp16 rounding of QKV, the KV-cache append and the residual add all
// live in the prologue/epilogue of the kernel that streams the weights:
//   dec_ln_gemv<QKV>  : LN1(h) . c_attn -> q (fp32 of the fp16-rounded value), K/V appended to the fp16 cache
//   attn_decode       : softmax(q.K/8).V over n_past+1 keys
//   dec_gemv_resid<4> : h += att . c_proj + b
//   dec_ln_gemv<GELU> : gelu(LN2(h) . c_fc + b) -> ff
//   dec_gemv_resid<16>: h += ff . c_proj2 + b
// and the head is dec_ln_gemv<LOGITS> (ln_f, lm_head LayerNorm, lm_head linear) straight to the logits.

// K = 1024 GEMV with LayerNorm prologue for 16 candidates x 16 output columns per workgroup. Default: split-precision
// operands on the fp16 MFMA (x = xh + xl split in registers, 64 W = wh + wl packed at load; wh.xh + wl.xh + wh.xl, 24
// MFMAs of 16 cycles per wave); TTS_DEC_F32MFMA=1: the fp32 MFMA (v_mfma_f32_16x16x4_f32, exact f32 products, 64 MFMAs of
// 32 cycles). Wave w covers k in [256w, 256w+256). Operands are fed swapped (A = weights,
// B = activations) so that a lane ends with 4 consecutive output columns of one candidate. The 4 k values of
// one MFMA are k0 + 4q + j for lane quarter q — a lane's activations are then one float4 of the natural
// [row][k] layout; the weights are packed to match (layout mfma16: mfma16_at). LayerNorm is evaluated on the
// register-resident operands: a row's 1024 values live in 4 lanes x 4 waves.
typedef float floatx2 __attribute__((ext_vector_type(2)));
enum { DEC_QKV = 0, DEC_GELU = 1, DEC_LOGITS = 2 };
#ifdef TTS_DEC_TRACE // developer build (tools/dec_bench.hip): phase timestamps (100 MHz wall clock) of every workgroup, one slot per kernel of a layer
__device__ long long tts_dec_trace[6 * 1024 * 8]; // slot: 0 LN1+QKV, 1 attention, 2 attention projection, 3 LN2+FC, 4 MLP projection, 5 head
#define DEC_T(i) do { if (threadIdx.x == 0) tts_dec_trace[((TSLOT) * 1024 + blockIdx.y * gridDim.x + blockIdx.x) * 8 + (i)] = wall_clock64(); } while (0)
#else
#define DEC_T(i)
#endif
struct DecLnArgs {
  const float *h;            // [rows][1024]
  const float *g1, *b1;      // DEC_LOGITS: ln_f (the LayerNorm feeding W is folded into W/bias at load)
  const float *W;            // layout mfma16 of diag(gamma) W
  const __half *Wh;          // SPLIT 1: layout mfma16h, the same matrix x 64 as fp16 hi|lo pairs; SPLIT 2: mfma16h, fp16 hi only (option ar_weights = 1);
                             // SPLIT 3: mfma16h, OCP fp8 e4m3 of W / wscale[column] (option ar_weights = 2)
  const float *bias;         // bias + beta . W
  int rows, n_valid, ldo;    // ldo: row stride of `out` for DEC_QKV (q) and DEC_LOGITS
  int prefill_B;             // DEC_QKV: 0 = decode (row = candidate, position n_past); > 0 = prompt pass (row = position,
                             // K/V replicated into the caches of prefill_B candidates)
  float *out;                // q [rows][ldo] | ff [rows][4096] | logits [rows][ldo]
  __half *kc, *vc;           // layer's caches [cand][max_pos][1024]
  const StepState *ss;
  int max_pos, lut;
  const float *wscale;       // SPLIT 3: per-output-column scale (a power of two) of the fp8 weights
  const int *row_off = nullptr; // RO (multi-prompt decode): per-row context offset added to the step's n_past (ArState::row_off)
};

// sum over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48): gfx950 half/row swap instructions
__device__ __forceinline__ float rows4_sum(float x) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// sred: two [4][16] arrays (one per pass, so each pass costs one barrier). g == nullptr: the affine part has
// been folded into the weights/bias at load (fold_layernorm).
// KSTEP: k of the i-th float4 of a lane = koff + (i >> KSH) * KSTEP + (i & ((1 << KSH) - 1)) * 4
//   fp32-MFMA operand order: KSH = 0, KSTEP = 16;  fp16-MFMA (split) order: KSH = 1, KSTEP = 32
template <int KSH, int KSTEP>
__device__ __forceinline__ void dec_layernorm(float4 (&x)[16], const float *__restrict__ g, const float *__restrict__ b,
                                              int koff, float (*sred)[4][16], int wave, int m) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) s += (x[i].x + x[i].y) + (x[i].z + x[i].w);
  sred[0][wave][m] = rows4_sum(s); // the 4 lanes of a row write the same value
  __syncthreads();
  const float mean = (((sred[0][0][m] + sred[0][1][m]) + sred[0][2][m]) + sred[0][3][m]) * (1.0f / D);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    x[i].x -= mean; x[i].y -= mean; x[i].z -= mean; x[i].w -= mean;
    ss += (x[i].x * x[i].x + x[i].y * x[i].y) + (x[i].z * x[i].z + x[i].w * x[i].w);
  }
  sred[1][wave][m] = rows4_sum(ss);
  __syncthreads();
  const float var = (((sred[1][0][m] + sred[1][1][m]) + sred[1][2][m]) + sred[1][3][m]) * (1.0f / D);
  const float sc = 1.0f / sqrtf(var + 1e-5f);
  if (g) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int k = koff + (i >> KSH) * KSTEP + (i & ((1 << KSH) - 1)) * 4;
      const float4 gg = *(const float4 *)(g + k), bb = *(const float4 *)(b + k);
      x[i].x = x[i].x * sc * gg.x + bb.x; x[i].y = x[i].y * sc * gg.y + bb.y;
      x[i].z = x[i].z * sc * gg.z + bb.z; x[i].w = x[i].w * sc * gg.w + bb.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) { x[i].x *= sc; x[i].y *= sc; x[i].z *= sc; x[i].w *= sc; }
  }
}

// SPLIT: 0 = fp32 MFMA on f32 weights, 1 = split-precision fp16 MFMA (every PRODUCT to 2^-22 relative; the sum adds the f32 accumulation of 256 products per wave:
// measured against float64 <= 0.2 x 2^-22 sum |x||w| on Gaussian columns, 1.1 on a row with one outlier channel; the f32 rounding of sum + bias comes on top,
// tests/test_ar_dec_kernels_gpu.py), 2 = fp16 WEIGHTS (rounded once at load:
// half the bytes streamed; the activations keep their hi + lo split) — the throughput mode of SURVEY 8d, option "ar_weights";
// 3 = OCP fp8 (e4m3) WEIGHTS with a power-of-two scale per output column (a quarter of the bytes): converted to fp16 in
// registers (exact: every e4m3 value is an fp16 value), multiplied on the fp16 MFMA against the hi + lo split activations.
// RO (DEC_QKV decode only): the K/V store position of row r is n_past + a.row_off[r] — a batch of several prompts (tts_ar_begin_multi); false = the
// single-prompt kernel unchanged.
template <int EPI, int SPLIT = 0, bool NTW = false, bool HT = false, bool RO = false> // HT: a.h is in the h4 layout (decode step); otherwise [row][1024] (prompt pass)
__global__ __launch_bounds__(256) void dec_ln_gemv_kernel(DecLnArgs a_in) {
  constexpr int SP = SPLIT ? 1 : 0;
  constexpr int TSLOT = EPI == DEC_QKV ? 0 : EPI == DEC_GELU ? 3 : 5; (void)TSLOT;
  __shared__ float sred[4][4][16];
  __shared__ float4 accs[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
  const int cb = blockIdx.x, row = blockIdx.y * 16 + m;
  DEC_T(0);
  // EVERY kernel argument is fetched in ONE batch of scalar loads at the top (the empty asm pins the values in SGPRs here). Left to itself
  // hipcc fetches an argument right before its first use: the 104-byte argument block spans two cache lines and nothing of a fresh launch is
  // cached, so the QKV variant ran THREE dependent scalar round trips (arguments, the pointer to the step state, n_past) before its first
  // vector load was issued, and every variant fetched `out` / `lut` (the second line) after the reduction — a cold miss at the very end of
  // each of the step's 61 launches of this kernel (seen in the ISA and in the per-launch trace, profiles/r4_decode_launch_breakdown.txt).
  const DecLnArgs &a = a_in;
  // (input-only operands: the values must be in SGPRs HERE, and the pointers keep their global address space — behind a "+s" they would
  //  become generic pointers and every load a flat_load, which also counts on lgkmcnt)
  asm volatile("" ::"s"(a.h), "s"(a.g1), "s"(a.b1), "s"(a.W), "s"(a.Wh), "s"(a.bias), "s"(a.out), "s"(a.kc), "s"(a.vc), "s"(a.ss), "s"(a.wscale));
  asm volatile("" ::"s"(a.rows), "s"(a.n_valid), "s"(a.ldo), "s"(a.prefill_B), "s"(a.max_pos), "s"(a.lut));
  if (RO) asm volatile("" ::"s"(a.row_off));
  // Everything the epilogue reads (bias, the step's n_past) is requested FIRST: loaded after the reduction they were one or two
  // dependent L2 round trips (~0.5 us each) at the end of every launch. n_past goes through the VECTOR memory path (a zero offset the
  // compiler cannot see through): as a scalar load it is a dependent round trip that every later s_waitcnt lgkmcnt(0) waits for; as the
  // first entry of the in-order vmcnt queue it retires before the activations and nothing waits for it until the epilogue.
  const float4 bi = *(const float4 *)(a.bias + cb * 16 + 4 * q);
  float4 wsc = make_float4(1.f, 1.f, 1.f, 1.f);
  if (SPLIT == 3) wsc = *(const float4 *)(a.wscale + cb * 16 + 4 * q);
  int n_past = 0;
  if (EPI == DEC_QKV) {
    unsigned zero = 0;
    asm volatile("" : "+v"(zero));
    const int *np_ptr = a.prefill_B == 0 ? &a.ss->n_past : (const int *)a.bias; // the prompt pass has no step state (ss may be null): read a valid dummy, drop it
    n_past = *(const int *)((const char *)np_ptr + zero);
    n_past = a.prefill_B == 0 ? n_past : 0;
    // the row's own context offset: a vector load issued beside n_past's (same queue position, no extra round trip). The array is padded to whole
    // tiles of 16 rows (zeros), so the rows of the last tile past the batch read inside it; their results are never stored.
    if (RO) n_past += a.row_off[row];
  }
  // activations next (L2 hits), then the weight slab (HBM): vmcnt retires in order, so the LayerNorm runs on
  // the activations while the 16 x 1 KB-per-wave weight loads are still streaming in
  const int koff = wave * 256 + (SPLIT ? 8 : 4) * q;
  float4 x[16];
  {
    if (HT) {
      // h4: the float4 of (candidate m, channels k .. k+3) sits at ((tile * 256 + k / 4) * 16 + m) * 4; a wave-level load = 4 runs of 256 contiguous
      // bytes (the 16 candidates of one channel group), 8 full cache lines. Rows past the batch are padding of the tile (allocated, never stored).
      const float *hp = a.h + (((size_t)blockIdx.y * 256 + (koff >> 2)) * 16 + m) * 4;
#pragma unroll
      for (int i = 0; i < 16; i++) x[i] = *(const float4 *)(hp + (SPLIT ? (i >> 1) * 8 + (i & 1) : i * 4) * 64);
    } else {
      // rows past the batch re-read the last candidate (branch-free); their results are never stored
      const float *hp = a.h + (size_t)min(row, a.rows - 1) * D + koff;
#pragma unroll
      for (int i = 0; i < 16; i++) x[i] = *(const float4 *)(hp + (SPLIT ? (i >> 1) * 32 + (i & 1) * 4 : i * 16));
    }
  }
  float4 w[16]; // SPLIT: step s = (w[2s] = 8 fp16 hi, w[2s+1] = 8 fp16 lo) of 64*W[k = koff + 32 s + e][col]
  {
    if (SPLIT == 2) { // 8 steps x 16 B per lane: half the slab of the split variant
      const float4 *wp = (const float4 *)a.Wh + ((size_t)(cb * 4 + wave) * 8) * 64;
#pragma unroll
      for (int i = 0; i < 8; i++) w[2 * i] = ldw4<NTW>(wp + i * 64 + lane);
    } else if (SPLIT == 3) { // 8 steps x 8 B per lane, two steps per 16-byte load: w[i] = steps 2 i, 2 i + 1
      const float4 *wp = (const float4 *)a.Wh + ((size_t)(cb * 4 + wave) * 4) * 64;
#pragma unroll
      for (int i = 0; i < 4; i++) w[i] = ldw4<NTW>(wp + i * 64 + lane);
    } else {
      const float4 *wp = (SPLIT ? (const float4 *)a.Wh : (const float4 *)a.W) + ((size_t)(cb * 4 + wave) * 16) * 64;
#pragma unroll
      for (int i = 0; i < 16; i++) w[i] = ldw4<NTW>(SPLIT ? wp + ((i >> 1) * 64 + lane) * 2 + (i & 1) : wp + i * 64 + lane);
    }
  }
  // Every request above stays in front of the first use: without this hipcc sinks the 16 weight loads below the LayerNorm's first
  // reduction (they would be issued only after `s_waitcnt vmcnt(0)` on the activations: the HBM round trip of the slab serialised
  // behind the L2 round trip of x instead of overlapping it; seen in the ISA, round 4).
  __builtin_amdgcn_sched_barrier(0);
  DEC_T(1);
  // the (last) LayerNorm's gamma/beta are folded into W/bias; the head's ln_f keeps its own
  if (EPI == DEC_LOGITS) dec_layernorm<SP, SPLIT ? 32 : 16>(x, a.g1, a.b1, koff, sred, wave, m);
  dec_layernorm<SP, SPLIT ? 32 : 16>(x, nullptr, nullptr, koff, sred + (EPI == DEC_LOGITS ? 2 : 0), wave, m);
  DEC_T(2);
  floatx4 acc;
  if (SPLIT) {
    // split precision on the fp16 MFMA: x = xh + xl, 64 W = wh + wl; wh.xh + wl.xh + wh.xl (the dropped wl.xl term is
    // 2^-22 relative to its product; an xl below 2^-14 is an fp16 subnormal and reaches the matrix pipe as one, not as 0: measured),
    // 24 MFMAs of 16 cycles instead of 64 fp32 MFMAs of 32
    floatx4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
#pragma unroll
    for (int s = 0; s < 8; s++) {
      const float xs[8] = {x[2 * s].x, x[2 * s].y, x[2 * s].z, x[2 * s].w, x[2 * s + 1].x, x[2 * s + 1].y, x[2 * s + 1].z, x[2 * s + 1].w};
      half8 xh, xl;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        xh[e] = (_Float16)xs[e];
        xl[e] = (_Float16)(xs[e] - (float)xh[e]);
      }
      half8 wh;
      if (SPLIT == 3) {
        const uint2 u = ((const uint2 *)&w[s >> 1])[s & 1];
        const floatx2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8(u.x, false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8(u.x, true);
        const floatx2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8(u.y, false), f3 = __builtin_amdgcn_cvt_pk_f32_fp8(u.y, true);
        wh[0] = (_Float16)f0[0]; wh[1] = (_Float16)f0[1]; wh[2] = (_Float16)f1[0]; wh[3] = (_Float16)f1[1];
        wh[4] = (_Float16)f2[0]; wh[5] = (_Float16)f2[1]; wh[6] = (_Float16)f3[0]; wh[7] = (_Float16)f3[1];
      } else wh = *(const half8 *)&w[2 * s];
      a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, a0, 0, 0, 0);
      if (SPLIT == 1) {
        const half8 wl = *(const half8 *)&w[2 * s + 1];
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, a1, 0, 0, 0);
      }
      a2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, a2, 0, 0, 0);
    }
    if (SPLIT == 3) { acc = a2 + a0; acc[0] *= wsc.x; acc[1] *= wsc.y; acc[2] *= wsc.z; acc[3] *= wsc.w; }
    else acc = ((a1 + a2) + a0) * (1.0f / 64.0f);
  } else {
    // four independent accumulator chains keep the fp32 MFMA pipe issue-bound instead of latency-bound
    floatx4 ac0 = {0.f, 0.f, 0.f, 0.f}, ac1 = ac0, ac2 = ac0, ac3 = ac0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      ac0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i].x, x[i].x, ac0, 0, 0, 0);
      ac1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i].y, x[i].y, ac1, 0, 0, 0);
      ac2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i].z, x[i].z, ac2, 0, 0, 0);
      ac3 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i].w, x[i].w, ac3, 0, 0, 0);
    }
    acc = (ac0 + ac1) + (ac2 + ac3);
  }
  DEC_T(3);
  accs[wave][lane] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  __syncthreads();
  DEC_T(4);
  if (wave != 0 || row >= a.rows) return;
  const float4 p0 = accs[0][lane], p1 = accs[1][lane], p2 = accs[2][lane], p3 = accs[3][lane];
  const int col = cb * 16 + 4 * q; // lane: candidate `row`, columns col .. col+3
  float4 v;
  v.x = (((p0.x + p1.x) + p2.x) + p3.x) + bi.x; v.y = (((p0.y + p1.y) + p2.y) + p3.y) + bi.y;
  v.z = (((p0.z + p1.z) + p2.z) + p3.z) + bi.z; v.w = (((p0.w + p1.w) + p2.w) + p3.w) + bi.w;
  if (EPI == DEC_QKV) {
    // QKV activations are rounded to fp16 (main.cpp:2789-2790)
    const __half2 h01 = __floats2half2_rn(v.x, v.y), h23 = __floats2half2_rn(v.z, v.w);
    const int sec = col >> 10, cc = col & (D - 1);
    if (sec == 0) {
      const float2 f01 = __half22float2(h01), f23 = __half22float2(h23);
      *(float4 *)(a.out + (size_t)row * a.ldo + cc) = make_float4(f01.x, f01.y, f23.x, f23.y);
    } else {
      uint2 u;
      u.x = *(const unsigned *)&h01;
      u.y = *(const unsigned *)&h23;
      __half *base = (sec == 1 ? a.kc : a.vc) + cc;
      if (a.prefill_B == 0) *(uint2 *)(base + ((size_t)row * a.max_pos + n_past) * D) = u;
      else
        for (int c = 0; c < a.prefill_B; c++) *(uint2 *)(base + ((size_t)c * a.max_pos + row) * D) = u;
    }
  } else if (EPI == DEC_GELU) {
    v.x = gelu_tanh(v.x, a.lut); v.y = gelu_tanh(v.y, a.lut); v.z = gelu_tanh(v.z, a.lut); v.w = gelu_tanh(v.w, a.lut);
    *(float4 *)(a.out + (size_t)row * FF + col) = v;
  } else {
    float *o = a.out + (size_t)row * a.ldo + col;
    if (col + 0 < a.n_valid) o[0] = v.x;
    if (col + 1 < a.n_valid) o[1] = v.y;
    if (col + 2 < a.n_valid) o[2] = v.z;
    if (col + 3 < a.n_valid) o[3] = v.w;
  }
  DEC_T(5);
}

// h[rows][1024] += X[rows][K] . W[K][1024] + bias, K = 1024 * KG. One workgroup owns 4 output columns over the
// whole K (W in layout cols4, cols4_at: 16 KB x KG contiguous per workgroup); thread t holds k = 1024 i + 4 t + kk.
// The 64 per-thread sums (16 candidates x 4 columns) are reduced with a 6-step exchange butterfly that
// leaves output t on lane t, then across the 4 waves through LDS — a fixed summation tree.
// NT threads per workgroup (256 or 512): with 512 the K range of a thread halves and twice as many activation loads
// are in flight per CU — the c_proj of the MLP (K = 4096) reads 256 KB of activations per workgroup and is bound by how
// many of those loads the CU keeps in flight.
// WH: the slab holds fp16 weights (cols4 order, 8 bytes per (k, 4 columns): option ar_weights = 1), converted to f32 in registers.
// WH = 2: OCP fp8 (e4m3) weights, 4 bytes per (k, 4 columns), times the power-of-two wscale[column] after the reduction (option ar_weights = 2).
template <int KG, int NT = 256, int WH = 0, bool NTW = false, bool HT = false> // HT: h is in the h4 layout (decode step)
__global__ __launch_bounds__(NT) void dec_gemv_resid_kernel(const float *__restrict__ X, int rows, const float *__restrict__ W,
                                                            const float *__restrict__ bias, float *__restrict__ h,
                                                            const float *__restrict__ wscale = nullptr) {
  constexpr int K = 1024 * KG, NW = NT / 64, NG = K / (NT * 4); // NG K groups of NT*4 values per workgroup
  constexpr int TSLOT = KG == 1 ? 2 : 4; (void)TSLOT;
  __shared__ float red[NW][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cb = blockIdx.x, row0 = blockIdx.y * 16;
  DEC_T(0);
  // the residual element and the bias this thread adds at the very end (threads 0-63: output 4 * candidate + column) are requested
  // first instead of after the reduction (a dependent L2 round trip at the end of 60 launches per step)
  const int er = min(row0 + ((tid & 63) >> 2), rows - 1), ecol = cb * 4 + (tid & 3);
  // h4: the workgroup's 16 candidates x 4 columns are 64 consecutive floats (thread t < 64 owns float t of the block)
  const size_t hidx = HT ? (((size_t)blockIdx.y * 256 + cb) * 64 + (tid & 63)) : (size_t)er * D + ecol;
  const float h_old = h[hidx], b_old = bias[ecol];
  float s_old = 1.0f;
  if (WH == 2) s_old = wscale[ecol];
  float4 xa0[8]; // candidates 0-7 of K group 0: requested before the weight stream
#pragma unroll
  for (int r = 0; r < 8; r++) xa0[r] = *(const float4 *)(X + (size_t)min(row0 + r, rows - 1) * K + 4 * tid);
  float4 w[NG][4];
  {
    // cols4 order: float4 index ((k / 1024) * 4 + kk) * 256 + (k % 1024) / 4 for k = g * NT * 4 + 4 * tid + kk
    if (WH == 2) {
      const unsigned *wp = (const unsigned *)W + (size_t)cb * KG * 1024 + (tid & 255);
#pragma unroll
      for (int i = 0; i < NG; i++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const unsigned u = wp[((i * (NT / 256) + (tid >> 8)) * 4 + kk) * 256];
          const floatx2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8(u, false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8(u, true);
          w[i][kk] = make_float4(f0[0], f0[1], f1[0], f1[1]);
        }
    } else if (WH == 1) {
      const uint2 *wp = (const uint2 *)W + (size_t)cb * KG * 1024 + (tid & 255);
#pragma unroll
      for (int i = 0; i < NG; i++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const uint2 u = wp[((i * (NT / 256) + (tid >> 8)) * 4 + kk) * 256];
          const float2 f0 = __half22float2(*(const __half2 *)&u.x), f1 = __half22float2(*(const __half2 *)&u.y);
          w[i][kk] = make_float4(f0.x, f0.y, f1.x, f1.y);
        }
    } else {
      const float4 *wp = (const float4 *)W + (size_t)cb * KG * 1024 + (tid & 255);
#pragma unroll
      for (int i = 0; i < NG; i++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) w[i][kk] = ldw4<NTW>(wp + ((i * (NT / 256) + (tid >> 8)) * 4 + kk) * 256);
    }
  }
  // Activations (L2 hits) are fetched 8 candidates at a time, double-buffered against the FMAs; K group i of the
  // weight slab is consumed for all 16 candidates as soon as it has arrived (vmcnt retires in order), so the
  // FMAs of groups 0..NG-2 overlap the rest of the weight stream. Two columns per v_pk_fma_f32.
  floatx2 acc[32];
#pragma unroll
  for (int j = 0; j < 32; j++) acc[j] = (floatx2){0.f, 0.f};
  const float *xbase = X + 4 * tid;
  int rowoff[16];
#pragma unroll
  for (int r = 0; r < 16; r++) rowoff[r] = min(row0 + r, rows - 1) * K; // rows past the batch re-read the last candidate
  float4 xa[8], xb[8];
#pragma unroll
  for (int r = 0; r < 8; r++) { xa[r] = xa0[r]; xb[r] = *(const float4 *)(xbase + rowoff[8 + r]); }
#pragma unroll
  for (int i = 0; i < NG; i++) {
#pragma unroll
    for (int half = 0; half < 2; half++) {
      // half 0 consumes xa (candidates 0-7), half 1 consumes xb (8-15); the other buffer is refilled meanwhile
      float4 (&cur)[8] = half ? xb : xa;
#pragma unroll
      for (int r = 0; r < 8; r++) {
        const float xs[4] = {cur[r].x, cur[r].y, cur[r].z, cur[r].w};
        floatx2 a01 = acc[(half * 8 + r) * 2], a23 = acc[(half * 8 + r) * 2 + 1];
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const floatx2 xx = {xs[kk], xs[kk]};
          a01 = __builtin_elementwise_fma(xx, (floatx2){w[i][kk].x, w[i][kk].y}, a01);
          a23 = __builtin_elementwise_fma(xx, (floatx2){w[i][kk].z, w[i][kk].w}, a23);
        }
        acc[(half * 8 + r) * 2] = a01; acc[(half * 8 + r) * 2 + 1] = a23;
      }
      if (i + 1 < NG) { // refill the buffer just consumed with the next K group
#pragma unroll
        for (int r = 0; r < 8; r++) cur[r] = *(const float4 *)(xbase + rowoff[half * 8 + r] + (i + 1) * (NT * 4));
      }
    }
  }
  float v[64];
#pragma unroll
  for (int j = 0; j < 32; j++) { v[2 * j] = acc[j][0]; v[2 * j + 1] = acc[j][1]; }
  DEC_T(1);
  // exchange butterfly: after the step with lane mask M a lane keeps the half of its values selected by its
  // bit M, summed with the partner lane's copy; 64 values -> 1, output index = lane.
#pragma unroll
  for (int i = 0; i < 32; i++) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 32]), false, false);
    v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < 16; i++) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 16]), false, false);
    v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int step = 2; step < 6; step++) {
    const int mask = 32 >> step, n = 32 >> step;
    const bool up = (lane & mask) != 0;
#pragma unroll
    for (int i = 0; i < n; i++) {
      const float send = up ? v[i] : v[i + n], keep = up ? v[i + n] : v[i];
      v[i] = keep + __shfl_xor(send, mask);
    }
  }
  DEC_T(2);
  red[wave][lane] = v[0]; // output index = lane = 4 * candidate + column
  __syncthreads();
  DEC_T(3);
  if (tid < 64) {
    const int r = row0 + (tid >> 2), col = cb * 4 + (tid & 3);
    if (r < rows) {
      float t = red[0][tid];
#pragma unroll
      for (int w2 = 1; w2 < NW; w2++) t += red[w2][tid];
      h[HT ? hidx : (size_t)r * D + col] = h_old + ((WH == 2 ? t * s_old : t) + b_old);
    }
  }
  DEC_T(4);
}

// max over the four 16-lane rows of a wave (see rows4_sum)
__device__ __forceinline__ float rows4_max(float x) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float x) { // lane i reads x of the lane the DPP control names (full row/bank masks)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
typedef _Float16 dhalf2 __attribute__((ext_vector_type(2)));

// 32 * NR keys starting at j0 for one (candidate, head): 8 lanes per key (16 B of K and of V each: whole 128 B rows per
// 8 lanes), key group kg = tid >> 3 owns keys j0 + kg + 32 r. All K and V rows of the chunk are requested before the
// first use, so the chunk costs one memory round trip. Online softmax state (m, l, acc) is per wave: m is uniform over
// the wave, l and acc are the lane's partial sums over its own keys.
template <int NR>
__device__ __forceinline__ void attn_decode_chunk(const __half *__restrict__ kb, const __half *__restrict__ vb, int j0, int nk, int kg,
                                                  int l8, const float4 &qa, const float4 &qb, float &m, float &l, float (&acc)[8]) {
  constexpr float L2E = 1.4426950408889634f;
  uint4 kq[NR], vq[NR];
#pragma unroll
  for (int r = 0; r < NR; r++) // uniform base + 32-bit byte offset (one candidate's cache is < 4 GB): saddr-form loads
    kq[r] = *(const uint4 *)((const char *)kb + ((unsigned)min(j0 + kg + 32 * r, nk - 1) * (unsigned)(D * 2) + (unsigned)l8 * 16u));
#pragma unroll
  for (int r = 0; r < NR; r++)
    vq[r] = *(const uint4 *)((const char *)vb + ((unsigned)min(j0 + kg + 32 * r, nk - 1) * (unsigned)(D * 2) + (unsigned)l8 * 16u));
  __builtin_amdgcn_sched_barrier(0); // keep every request in front of the first use (the scheduler would sink the V loads)
  // q was rounded to fp16 by the QKV epilogue: the conversion back is exact. The empty asm pins the first use of q
  // behind the requests above (the conversion is common to all chunk sizes and would be hoisted in front of them).
  float4 qc = qa, qd = qb;
  asm volatile("" : "+v"(qc.x), "+v"(qc.y), "+v"(qc.z), "+v"(qc.w), "+v"(qd.x), "+v"(qd.y), "+v"(qd.z), "+v"(qd.w));
  const dhalf2 q2[4] = {{(_Float16)qc.x, (_Float16)qc.y}, {(_Float16)qc.z, (_Float16)qc.w},
                        {(_Float16)qd.x, (_Float16)qd.y}, {(_Float16)qd.z, (_Float16)qd.w}};
  float s[NR], mc = -INFINITY;
#pragma unroll
  for (int r = 0; r < NR; r++) {
    const dhalf2 *k2 = (const dhalf2 *)&kq[r];
    float d = __builtin_amdgcn_fdot2(k2[0], q2[0], 0.f, false);
    d = __builtin_amdgcn_fdot2(k2[1], q2[1], d, false);
    d = __builtin_amdgcn_fdot2(k2[2], q2[2], d, false);
    d = __builtin_amdgcn_fdot2(k2[3], q2[3], d, false);
    d += dpp_f32<0xB1>(d);  // quad_perm [1,0,3,2]
    d += dpp_f32<0x4E>(d);  // quad_perm [2,3,0,1]
    d += dpp_f32<0x141>(d); // row_half_mirror: lane i <-> 7 - i of each 8
    s[r] = (j0 + kg + 32 * r < nk) ? d * 0.125f : -INFINITY;
    mc = fmaxf(mc, s[r]);
  }
  mc = rows4_max(fmaxf(mc, __shfl_xor(mc, 8)));
  const float mn = fmaxf(m, mc);
  const float mu = (mn == -INFINITY) ? 0.f : mn; // a wave without a valid key yet: all weights 0
  const float alpha = __builtin_amdgcn_exp2f((m - mu) * L2E);
  l *= alpha;
#pragma unroll
  for (int e = 0; e < 8; e++) acc[e] *= alpha;
#pragma unroll
  for (int r = 0; r < NR; r++) {
    const float p = __builtin_amdgcn_exp2f((s[r] - mu) * L2E);
    l += p;
    const __half2 *v2 = (const __half2 *)&vq[r];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float2 f = __half22float2(v2[e]);
      acc[2 * e] = fmaf(p, f.x, acc[2 * e]);
      acc[2 * e + 1] = fmaf(p, f.y, acc[2 * e + 1]);
    }
  }
  m = mn;
}

// Decode attention for one (candidate, head), the default (non-LUT) path: softmax(q.K/8) V over n_past+1 keys with the
// hardware exp2 (relative error ~1e-6 on a weight). Up to 288 keys go through one chunk = one memory round trip
// (attn_decode_chunk); the four waves keep separate online-softmax states that are merged once at the end.
// RO: row c sees ss->n_past + row_off[c] + 1 keys (a batch of several prompts, tts_ar_begin_multi); false: row_off is not read.
template <bool RO = false>
__global__ __launch_bounds__(256) void attn_decode_fast_kernel(const float *__restrict__ qbuf, const __half *__restrict__ kc,
                                                               const __half *__restrict__ vc, const StepState *__restrict__ ss,
                                                               int max_pos, float *__restrict__ out, const int *__restrict__ row_off) {
  constexpr float L2E = 1.4426950408889634f;
  constexpr int TSLOT = 1; (void)TSLOT;
  __shared__ float red[4][HD];
  __shared__ float wm[4], wl[4];
  const int c = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l8 = tid & 7, kg = tid >> 3;
  DEC_T(0);
  // all arguments in one batch of scalar loads (see dec_ln_gemv_kernel) and the one dependent fetch this kernel cannot avoid: n_past.
  // (the load of n_past stays IN FRONT of the asm: behind a volatile asm hipcc no longer proves the memory unclobbered and fetches it through
  //  the vector path, which makes the loop bounds divergent)
  // (RO: the row's offset is a second scalar load from a kernel argument, issued beside n_past's: the same single round trip)
  const int nk = ss->n_past + 1 + (RO ? row_off[c] : 0);
  asm volatile("" ::"s"(qbuf), "s"(kc), "s"(vc), "s"(max_pos), "s"(out)); // input-only: the pointers keep their address space
  const __half *kb = kc + (size_t)c * max_pos * D + h * HD;
  const __half *vb = vc + (size_t)c * max_pos * D + h * HD;
  const float4 qa = *(const float4 *)(qbuf + (size_t)c * D + h * HD + l8 * 8), qb = *(const float4 *)(qbuf + (size_t)c * D + h * HD + l8 * 8 + 4);
  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; e++) acc[e] = 0.f;
  for (int j0 = 0; j0 < nk; j0 += 288) {
    const int rem = nk - j0; // workgroup-uniform
    if (rem <= 96) attn_decode_chunk<3>(kb, vb, j0, nk, kg, l8, qa, qb, m, l, acc);
    else if (rem <= 160) attn_decode_chunk<5>(kb, vb, j0, nk, kg, l8, qa, qb, m, l, acc);
    else if (rem <= 224) attn_decode_chunk<7>(kb, vb, j0, nk, kg, l8, qa, qb, m, l, acc);
    else attn_decode_chunk<9>(kb, vb, j0, nk, kg, l8, qa, qb, m, l, acc);
  }
  // sum over the wave's 8 key groups (lane bits 3-5). l: plain reduction. acc: exchange butterfly, 8 values -> the
  // wave total of dim l8 * 8 + (lane >> 3)
  l += __shfl_xor(l, 8);
  l = rows4_sum(l);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i]), __float_as_uint(acc[i + 4]), false, false);
    acc[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < 2; i++) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[i]), __float_as_uint(acc[i + 2]), false, false);
    acc[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  {
    const bool up = (lane & 8) != 0;
    const float send = up ? acc[0] : acc[1], keep = up ? acc[1] : acc[0];
    acc[0] = keep + __shfl_xor(send, 8);
  }
  DEC_T(1);
  red[wave][l8 * 8 + (lane >> 3)] = acc[0];
  if (lane == 0) { wm[wave] = m; wl[wave] = l; }
  __syncthreads();
  DEC_T(2);
  if (tid < HD) {
    const float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3])); // wave 0 always holds key 0: finite
    float tot = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const float sc = __builtin_amdgcn_exp2f((wm[w] - M) * L2E); // exp2(-inf) = 0 for a wave without keys
      tot = fmaf(sc, wl[w], tot);
      o = fmaf(sc, red[w][tid], o);
    }
    out[(size_t)c * D + h * HD + tid] = o / tot;
  }
  DEC_T(3);
}

// Decode attention for one (candidate, head): q is this step's (fp16-rounded) query, K/V of the new position
// are already in the fp16 cache; softmax(q.K/8) V over n_past+1 keys. 4 waves: keys are spread over all 256
// threads for the scores and over 16 groups for PV.
template <bool RO = false> // as attn_decode_fast_kernel
__global__ __launch_bounds__(256) void attn_decode_kernel(const float *__restrict__ qbuf, const __half *__restrict__ kc,
                                                          const __half *__restrict__ vc, const StepState *__restrict__ ss,
                                                          int max_pos, float *__restrict__ out, int lut, const int *__restrict__ row_off) {
  __shared__ float sc[1024];
  __shared__ float qs[HD];
  __shared__ float red[16 * HD];
  __shared__ float wred[8];
  const int c = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nk = ss->n_past + 1 + (RO ? row_off[c] : 0);
  const __half *kb = kc + (size_t)c * max_pos * D + h * HD;
  const __half *vb = vc + (size_t)c * max_pos * D + h * HD;
  if (tid < HD) qs[tid] = qbuf[(size_t)c * D + h * HD + tid];
  // V rows of the first PV batch do not depend on the scores: request them now, they arrive under the score phase
  const int dl = tid & 15, grp = tid >> 4;
  uint2 vv0[8];
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int j = grp + u * 16;
    vv0[u] = (j < nk) ? *(const uint2 *)(vb + (size_t)j * D + dl * 4) : make_uint2(0u, 0u);
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int j = tid; j < nk; j += 256) {
    const uint4 *kp = (const uint4 *)(kb + (size_t)j * D);
    uint4 u[8];
#pragma unroll
    for (int q = 0; q < 8; q++) u[q] = kp[q];
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const __half2 *h2 = (const __half2 *)&u[q];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const float2 f = __half22float2(h2[e]);
        dot = fmaf(qs[q * 8 + e * 2], f.x, dot);
        dot = fmaf(qs[q * 8 + e * 2 + 1], f.y, dot);
      }
    }
    dot *= 0.125f;
    sc[j] = dot;
    mx = fmaxf(mx, dot);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if (lane == 0) wred[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
  float sum = 0.f;
  for (int j = tid; j < nk; j += 256) {
    const float e = lut ? f16_round(expf(f16_round(sc[j] - mx))) : expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) wred[4 + wave] = sum;
  __syncthreads();
  const float inv = 1.0f / (((wred[4] + wred[5]) + wred[6]) + wred[7]);
  // PV: 16 key groups x 16 lanes; a lane owns 4 consecutive dims (8-byte loads), keys j = grp, grp+16, ...
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int j0 = grp; j0 < nk; j0 += 16 * 8) {
    uint2 vv[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int j = j0 + u * 16;
      if (j0 == grp) vv[u] = vv0[u];
      else vv[u] = (j < nk) ? *(const uint2 *)(vb + (size_t)j * D + dl * 4) : make_uint2(0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int j = j0 + u * 16;
      const float p = (j < nk) ? sc[j] * inv : 0.f;
      const float2 f0 = __half22float2(*(const __half2 *)&vv[u].x), f1 = __half22float2(*(const __half2 *)&vv[u].y);
      a0 = fmaf(p, f0.x, a0); a1 = fmaf(p, f0.y, a1); a2 = fmaf(p, f1.x, a2); a3 = fmaf(p, f1.y, a3);
    }
  }
  red[grp * HD + dl * 4 + 0] = a0; red[grp * HD + dl * 4 + 1] = a1;
  red[grp * HD + dl * 4 + 2] = a2; red[grp * HD + dl * 4 + 3] = a3;
  __syncthreads();
  if (tid < HD) {
    float o = 0.f;
#pragma unroll
    for (int g2 = 0; g2 < 16; g2++) o += red[g2 * HD + tid];
    out[(size_t)c * D + h * HD + tid] = o;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// Device top-k prefilter (option "device_topk"): the sampler (process_logits_and_sample, main.cpp:4753-4806) keeps the 50 largest
// penalised logits of 8194. Instead of 16 x 8194 floats per step crossing PCIe, every candidate's row is reduced on the device to the
// logits >= a threshold that keeps TTS_PF_MIN .. TTS_PF_MAX of them, in index order; the host runs the bit-exact float tail over that
// list (host_logic.cpp: sample_one_list, which also states why the list is sufficient and when the full row is fetched instead).
// One workgroup per candidate, 33 logits per thread in registers as order-preserving integer keys; the threshold is found by bisection
// on the key (one ballot-popcount pass over the registers + one barrier per probe, <= 32 probes), then an index-ordered compaction.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pf_key(float v) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0; // -0 and +0 compare equal as floats: one key
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

// PEN (option "ar_penalty_scope" = 1, upstream's full-history repetition penalty): the kernel penalises before it thresholds. hist = the
// candidates' history bitmaps [B][TTS_HIST_WORDS] (bit i: id i was fed since tts_ar_begin*, or is 1 / 8192), toks = the ids this step was fed
// (ArState::h_toks): candidate c's token joins its set here — thread 0 stores the bit, every thread also compares its indices against the token
// itself, so nobody waits for that store — and the set is idempotent under a step fed twice. The stop mask comes first, then
// g < 0 ? g * penalty : g / penalty in plain float arithmetic (what apply_penalty does on the host: correctly rounded multiply and divide, no
// fast-math), and the lists carry the penalised values; the host tail then applies temperature, top-k, top-p and the multinomial only.
// pf_min: the keep window's lower bound (common.h: pf_min_for(top_k)); above TTS_PF_MAX no list is written (n = -1 for every candidate).
template <bool PEN>
__device__ __forceinline__ float pf_value(const float *__restrict__ src, int i, int mask_stop, bool pen, float penalty) {
  float v = src[i];
  if (mask_stop && i == V - 1) v = -1e30f; // TTS_AR_MASK_STOP: the stop token 8193 is never sampled
  if (PEN && pen) v = (v < 0.f) ? v * penalty : v / penalty;
  return v;
}

// Bit j of the result: this thread's logit j (index j * 256 + tid) is penalised: its id is in the row's history set hc, or is the token this step was fed.
__device__ __forceinline__ unsigned long long pf_history_mask(const uint32_t *__restrict__ hc, int tok, int tid) {
  constexpr int NJ = (V + 255) / 256; // 33
  unsigned long long penm = 0ull;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int i = j * 256 + tid;
    if (i < V && (((hc[i >> 5] >> (i & 31)) & 1u) || i == tok)) penm |= 1ull << j;
  }
  return penm;
}

// Bit j: this thread's logit j is the token this step was fed (penalty scope 0 under typical sampling: the one id the host would penalise).
__device__ __forceinline__ unsigned long long pf_token_mask(int tok, int tid) { return (tok & 255) == tid ? 1ull << (tok >> 8) : 0ull; }

// ---------------------------------------------------------------------------------------------
// Locally typical sampling on the device (option "ar_typical_mass"; the definition: host_logic.cpp typical_keep). One workgroup of 256 threads per row, the
// row's 33 penalised logits per thread in registers. With a_i = m - x_i >= 0 (m = the row maximum, exact) the literal's distance d_i = |-ln p_i - H| is
// |a_i - t|, t = sum a_i e_i / Z = H - ln Z, e_i = exp(-a_i), Z = sum e_i: ln Z cancels and ONE scalar orders the row. The body computes Z and sum a e in double
// (block tree sums), p_i = e_i / Z, the distances' bit patterns as ordered 64-bit keys, and bisects on the key for theta = the smallest distance whose
// inclusive mass M(theta) = sum {p_i : d_i <= theta} reaches the mass (M is a fixed tree sum of non-negative terms: monotone in theta; at most 63 probes, and
// the search ends as soon as one distance is left in the interval).
// Error bounds (u = 2^-53, V = 8194, all sums of same-signed terms, worst-case summation (V - 1) u; H <= ln V = 9.02, t <= ln V):
//   literal: Z_L = Z (1 + (V + 1) u) -> ln p_i off by <= 9.2e-13 + u |ln p_i|; p_i relative 1.0e-12; H_L off by <= H (9.1e-13 + 1.0e-12) + 9.2e-13 <= 1.82e-11;
//            d_L off by <= 1.92e-11 + 2 u (a_i + 9.02); a cumulative c_j relative <= 1.0e-12 + (V - 1) u = 1.92e-12.
//   device:  Z', S' relative <= (V + 3) u (device exp: 1 ulp) -> t' off by <= 9.02 * 1.83e-12 = 1.65e-11; d' off by <= 1.65e-11 + 2 u (a_i + 9.02);
//            M' relative <= 1.92e-12 + u.
//   together |d' - d_L| <= 3.6e-11 + 4.4e-16 (a_i + 9.02) < E = TTS_TYP_TOL_D (2^-33 = 1.16e-10) + TTS_TYP_TOL_REL (2^-49 = 1.8e-15) (t + theta) for every element
//   within 2 E of theta (a_i <= t + theta + 2 E), and |M' - c_L| <= 3.9e-12 < TTS_TYP_TOL_M (2^-35 = 2.9e-11): a margin of 3 and 7.
// The set {d' <= theta} is the literal's, and is returned, only when
//   - no other distance lies within 2 E of theta: then the literal orders every member before every non-member and every other member before the elements AT
//     theta; those must share one logit value (equal logits have equal literal distances, and ties survive the literal's cut);
//   - M(theta) >= mass + TTS_TYP_TOL_M and the mass strictly below theta is < mass - TTS_TYP_TOL_M: the literal's cumulative sum crosses the mass at an element AT theta.
// Otherwise nm = -1: the host fetches the row and runs the literal (tts_ar_topk_fallbacks). Every value a branch depends on went through LDS: workgroup-uniform.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double typ_block_sum(double v, double (*red)[4], int &it, int lane, int wave) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) red[it & 1][wave] = v;
  __syncthreads(); // double-buffered: one barrier per reduction
  const double r = (red[it & 1][0] + red[it & 1][1]) + (red[it & 1][2] + red[it & 1][3]);
  it++;
  return r;
}
// two sums behind one barrier (red2: its own double buffer)
__device__ __forceinline__ void typ_block_sum2(double &a, double &b, double (*red2)[4][2], int &it, int lane, int wave) {
#pragma unroll
  for (int o = 32; o; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
  if (lane == 0) { red2[it & 1][wave][0] = a; red2[it & 1][wave][1] = b; }
  __syncthreads();
  a = (red2[it & 1][0][0] + red2[it & 1][1][0]) + (red2[it & 1][2][0] + red2[it & 1][3][0]);
  b = (red2[it & 1][0][1] + red2[it & 1][1][1]) + (red2[it & 1][2][1] + red2[it & 1][3][1]);
  it++;
}
__device__ __forceinline__ float typ_block_max(float v, double (*red)[4], int &it, int lane, int wave) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  if (lane == 0) red[it & 1][wave] = (double)v;
  __syncthreads();
  const float r = fmaxf(fmaxf((float)red[it & 1][0], (float)red[it & 1][1]), fmaxf((float)red[it & 1][2], (float)red[it & 1][3]));
  it++;
  return r;
}
__device__ __forceinline__ float pf_unkey(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); } // pf_key's inverse (-0 comes back as +0)

// key: the row's penalised logits as pf_key keys (index j * 256 + tid; entries past V are not read). memb: bit j = element j is a member. Returns the number of
// members, or -1 (undecided).
__device__ __forceinline__ int typical_members(const unsigned (&key)[(V + 255) / 256], float mass_f, unsigned long long &memb) {
  constexpr int NJ = (V + 255) / 256;
  __shared__ double red[2][4];
  __shared__ double red2[2][4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double mass = (double)mass_f;
  int it = 0, it2 = 0;
  memb = 0ull;
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NJ; j++)
    if (j * 256 + tid < V) mx = fmaxf(mx, pf_unkey(key[j]));
  const double m = (double)typ_block_max(mx, red, it, lane, wave);
  double p[NJ];
  double zs = 0.0, ss = 0.0;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    p[j] = 0.0;
    if (j * 256 + tid < V) {
      const double a = m - (double)pf_unkey(key[j]);
      const double e = exp(-a);
      p[j] = e; zs += e; ss += a * e;
    }
  }
  const double Z = typ_block_sum(zs, red, it, lane, wave), S = typ_block_sum(ss, red, it, lane, wave);
  if (!(Z > 0.0) || !isfinite(Z) || !isfinite(S)) return -1;
  const double t = S / Z;
  long long dk[NJ]; // the distance's bits: ordered as the distances are (d >= 0); past V: above every probe
  double tot = 0.0;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    p[j] = p[j] / Z;
    tot += p[j];
    dk[j] = 0x7fffffffffffffffll;
    if (j * 256 + tid < V) {
      const double d = fabs((m - (double)pf_unkey(key[j])) - t);
      if (isfinite(d)) dk[j] = __double_as_longlong(d);
    }
  }
  long long lo = -1ll, hi = 0x7fefffffffffffffll; // M(lo) < mass <= M(hi); hi: the largest finite distance's pattern
  double n_in = 0.0; // the number of distances in (lo, hi]
#pragma unroll
  for (int j = 0; j < NJ; j++) n_in += dk[j] <= hi ? 1.0 : 0.0;
  typ_block_sum2(tot, n_in, red2, it2, lane, wave);
  if (!(tot >= mass)) return -1; // the mass is never reached: the literal keeps the whole row
  // Every probe also counts the distances in (lo, mid]: once a single distance is left in (lo, hi] it is theta (M is constant between two distances), which
  // ends the search after some 20 probes instead of 63; distances that tie run the bisection to its end.
  while (hi - lo > 1ll && n_in != 1.0) {
    const long long mid = lo + ((hi - lo) >> 1);
    double ms = 0.0, nc = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      ms += dk[j] <= mid ? p[j] : 0.0;
      nc += (dk[j] <= mid && dk[j] > lo) ? 1.0 : 0.0;
    }
    typ_block_sum2(ms, nc, red2, it2, lane, wave);
    if (ms >= mass) { hi = mid; n_in = nc; }
    else { lo = mid; n_in -= nc; }
  }
  if (hi - lo > 1ll) { // one distance in (lo, hi]: its pattern (a non-negative double: fmaxf's order is not needed, the others contribute 0)
    double dv = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; j++)
      if (dk[j] > lo && dk[j] <= hi) dv = __longlong_as_double(dk[j]);
    hi = __double_as_longlong(typ_block_sum(dv, red, it, lane, wave)); // a sum with one non-zero term: exact
  }
  const double theta = __longlong_as_double(hi), E2 = 2.0 * (TTS_TYP_TOL_D + TTS_TYP_TOL_REL * (t + theta));
  double m_le = 0.0, m_lt = 0.0, n_le = 0.0, n_eq = 0.0, n_win = 0.0;
  float xe = -INFINITY;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const double d = __longlong_as_double(dk[j]); // (past V: a NaN pattern, every comparison below is false)
    if (dk[j] <= hi) { m_le += p[j]; n_le += 1.0; memb |= 1ull << j; }
    if (dk[j] < hi) m_lt += p[j];
    if (dk[j] == hi) { n_eq += 1.0; xe = fmaxf(xe, pf_unkey(key[j])); }
    if (d >= theta - E2 && d <= theta + E2) n_win += 1.0;
  }
  m_le = typ_block_sum(m_le, red, it, lane, wave); m_lt = typ_block_sum(m_lt, red, it, lane, wave);
  n_le = typ_block_sum(n_le, red, it, lane, wave); n_eq = typ_block_sum(n_eq, red, it, lane, wave); n_win = typ_block_sum(n_win, red, it, lane, wave);
  xe = typ_block_max(xe, red, it, lane, wave);
  double n_eqx = 0.0;
#pragma unroll
  for (int j = 0; j < NJ; j++)
    if (dk[j] == hi && pf_unkey(key[j]) == xe) n_eqx += 1.0;
  n_eqx = typ_block_sum(n_eqx, red, it, lane, wave);
  const bool ok = m_le >= mass + TTS_TYP_TOL_M && m_lt < mass - TTS_TYP_TOL_M && n_win == n_eq && n_eqx == n_eq;
  return ok ? (int)n_le : -1;
}

// One row's list: threshold search, index-ordered compaction and the values (pf_value). The ONE body of sample_prefilter_kernel<false / true> and of
// sample_prefilter_rows_kernel (a workgroup of 256 threads per row; src = the row's logits, o = its TTS_PF_WORDS words; penm: pf_history_mask, read only
// under PEN). pf_min and penalty are workgroup-uniform.
// TYP (typical sampling, mass > 0 workgroup-uniform): the typical set of the penalised row is decided first (typical_members; undecided: n = -1); search, compaction
// and value write then run over the members only, a non-member counting as masked (key 0). Fewer than pf_min members: the list is the whole set and header word
// 1 says so (TTS_PF_WHOLE: the host tail accepts n < top_k under it).
template <bool PEN, bool TYP = false>
__device__ __forceinline__ void prefilter_row_block(const float *__restrict__ src, int32_t *__restrict__ o, int mask_stop, int pf_min, unsigned long long penm,
                                                    float penalty, float mass = 0.f) {
  constexpr int NJ = (V + 255) / 256; // 33
  __shared__ int red[2][4];
  __shared__ int4 tab[NJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (pf_min > TTS_PF_MAX) { // top-k beyond what a 128-entry list can serve: the host samples the candidate from its full row
    if (tid == 0) o[0] = -1;
    return;
  }
  unsigned key[NJ];
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int i = j * 256 + tid;
    key[j] = i < V ? pf_key(pf_value<PEN>(src, i, mask_stop, (penm >> j) & 1ull, penalty)) : 0u; // padding: key 0 is below every probe (probes are > 0)
  }
  unsigned lo = 0u, hi = 0xffffffffu, t = 0u; // count(lo) > PF_MAX, count(hi) < pf_min
  int n = -1, it = 0;
  bool whole = false;
  if (TYP) {
    unsigned long long memb;
    const int nm = typical_members(key, mass, memb);
    if (nm < 0) {
      if (tid == 0) o[0] = -1;
      return;
    }
#pragma unroll
    for (int j = 0; j < NJ; j++)
      if (!((memb >> j) & 1ull)) key[j] = 0u;
    if (nm < pf_min) { whole = true; n = nm; t = 1u; hi = lo; } // nm < pf_min <= TTS_PF_MAX: every member (a finite value's key is >= 1); no search
  }
  while (hi - lo > 1u) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    int cw = 0;
#pragma unroll
    for (int j = 0; j < NJ; j++) cw += __popcll(__ballot(key[j] >= mid));
    if (lane == 0) red[it & 1][wave] = cw;
    __syncthreads(); // double-buffered: one barrier per probe
    const int cnt = red[it & 1][0] + red[it & 1][1] + red[it & 1][2] + red[it & 1][3];
    it++;
    if (cnt > TTS_PF_MAX) lo = mid;
    else if (cnt < pf_min) hi = mid;
    else { n = cnt; t = mid; break; }
  }
  if (n < 0) { // more than PF_MAX - pf_min + 1 values tie at the pf_min-th place: the host takes the full row
    if (tid == 0) o[0] = -1;
    return;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int cw = __popcll(__ballot(key[j] >= t));
    if (lane == 0) ((int *)&tab[j])[wave] = cw;
  }
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int4 r = tab[j];
    const unsigned long long m = __ballot(key[j] >= t);
    if (key[j] >= t) {
      const int i = j * 256 + tid;
      const int pos = base + (wave > 0 ? r.x : 0) + (wave > 1 ? r.y : 0) + (wave > 2 ? r.z : 0) + __popcll(m & below);
      o[4 + pos] = i;
      o[4 + TTS_PF_MAX + pos] = __float_as_int(pf_value<PEN>(src, i, mask_stop, (penm >> j) & 1ull, penalty));
    }
    base += r.x + r.y + r.z + r.w;
  }
  if (tid == 0) { o[0] = n; o[1] = (TYP && whole) ? TTS_PF_WHOLE : 0; o[2] = 0; o[3] = 0; }
}

template <bool PEN>
__global__ __launch_bounds__(256) void sample_prefilter_kernel(const float *__restrict__ logits, int mask_stop, int pf_min, int32_t *__restrict__ out,
                                                               uint32_t *__restrict__ hist, const int32_t *__restrict__ toks, float penalty) {
  const int c = blockIdx.x, tid = threadIdx.x;
  unsigned long long penm = 0ull; // PEN: bit j = this thread's logit j is penalised
  if (PEN) {
    uint32_t *hc = hist + (size_t)c * TTS_HIST_WORDS;
    const int tok = toks[c]; // 0 <= tok < V (ar_step checks)
    if (tid == 0) hc[tok >> 5] |= 1u << (tok & 31); // one workgroup per candidate, one writer
    penm = pf_history_mask(hc, tok, tid);
  }
  prefilter_row_block<PEN>(logits + (size_t)c * V, out + (size_t)c * TTS_PF_WORDS, mask_stop, pf_min, penm, penalty);
}

// The prefilter under typical sampling (mass > 0), a kernel of its own: sample_prefilter_kernel<false / true> are what they were. The typical set is that of
// the PENALISED row, so the kernel penalises in either scope and its lists hold penalised values: HIST (scope 1) with the history set as sample_prefilter_kernel<true>;
// scope 0 the one id this step was fed, which is the id the host would penalise (the previous sample).
template <bool HIST>
__global__ __launch_bounds__(256) void sample_prefilter_typical_kernel(const float *__restrict__ logits, int mask_stop, int pf_min, int32_t *__restrict__ out,
                                                                       uint32_t *__restrict__ hist, const int32_t *__restrict__ toks, float penalty, float mass) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const int tok = toks[c]; // 0 <= tok < V (ar_step checks)
  unsigned long long penm;
  if (HIST) {
    uint32_t *hc = hist + (size_t)c * TTS_HIST_WORDS;
    if (tid == 0) hc[tok >> 5] |= 1u << (tok & 31); // one workgroup per candidate, one writer
    penm = pf_history_mask(hc, tok, tid);
  } else penm = pf_token_mask(tok, tid);
  prefilter_row_block<true, true>(logits + (size_t)c * V, out + (size_t)c * TTS_PF_WORDS, mask_stop, pf_min, penm, penalty, mass);
}

// The prefilter of a session opened with TTS_AR_ROW_CONTROLS: every row under its own controls, none of them baked into the launch. ctl [rows padded to whole
// tiles] = {pf_min_for(top_k), the penalty's bits, the penalty scope, the typical mass' bits} per row, written outside the graph (ar_session_controls: at admission, for the
// slots the request takes, always); an empty or parked row keeps the entry of its last request and is never sampled. The entry's address is workgroup-uniform and
// its load is issued first, beside the row's first logits loads. pf_min above TTS_PF_MAX writes n = -1 for this row only. Scope 1: the penalised values,
// as sample_prefilter_kernel<true>; scope 0: pf_value<true> with no bit of penm set, which is sample_prefilter_kernel<false>'s value. The fed token joins the
// row's history set whatever the scope, as in the scope-1 graph: an admission resets the rows it takes. The entry's fourth word: the bits of the row's typical
// mass, 0 = off (a workgroup-uniform branch): rows with and without typical sampling and with different masses share the launch.
__global__ __launch_bounds__(256) void sample_prefilter_rows_kernel(const float *__restrict__ logits, int mask_stop, const int4 *__restrict__ ctl,
                                                                    int32_t *__restrict__ out, uint32_t *__restrict__ hist, const int32_t *__restrict__ toks) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const int4 rc = ctl[c];
  uint32_t *hc = hist + (size_t)c * TTS_HIST_WORDS;
  const int tok = toks[c]; // 0 <= tok < V (ar_session_step checks)
  if (tid == 0) hc[tok >> 5] |= 1u << (tok & 31); // one workgroup per row, one writer
  if (rc.w) { // typical sampling: penalised in either scope (sample_prefilter_typical_kernel)
    const unsigned long long pent = rc.z ? pf_history_mask(hc, tok, tid) : pf_token_mask(tok, tid);
    prefilter_row_block<true, true>(logits + (size_t)c * V, out + (size_t)c * TTS_PF_WORDS, mask_stop, rc.x, pent, __int_as_float(rc.y), __int_as_float(rc.w));
    return;
  }
  const unsigned long long penm = rc.z ? pf_history_mask(hc, tok, tid) : 0ull;
  prefilter_row_block<true>(logits + (size_t)c * V, out + (size_t)c * TTS_PF_WORDS, mask_stop, rc.x, penm, __int_as_float(rc.y));
}

// Penalty scope 1, a step that hands back the logits (tts_ar_step): the fed ids join the candidates' history sets here, since no prefilter runs.
__global__ void hist_mark_kernel(const int32_t *__restrict__ toks, int B, uint32_t *__restrict__ hist) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= B) return;
  const int tok = toks[c];
  hist[(size_t)c * TTS_HIST_WORDS + (tok >> 5)] |= 1u << (tok & 31); // one thread per candidate: its own row
}


struct ArLayerDev {
  float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  float *w_attn, *b_attn, *w_proj, *b_proj, *w_fc, *b_fc, *w_fc2, *b_fc2;
  __half *s_attn = nullptr, *s_proj = nullptr, *s_fc = nullptr, *s_fc2 = nullptr; // [N][2K] hi|lo of 64*W^T
  float *d_attn = nullptr, *d_fc = nullptr;   // layout mfma16 of diag(ln gamma) W (decode step, option dec_f32_mfma)
  __half *dh_attn = nullptr, *dh_fc = nullptr; // layout mfma16h, hi | lo, of the same (split-precision variant)
  float *db_attn = nullptr, *db_fc = nullptr; // bias + ln beta . W
  float *d_proj = nullptr, *d_fc2 = nullptr;  // layout cols4 (decode step)
  __half *q_attn = nullptr, *q_fc = nullptr, *q_proj = nullptr, *q_fc2 = nullptr; // fp16-weight decode slabs (option ar_weights = 1 at load)
  // fp8-weight decode slabs (option ar_weights = 2 at load): e4m3 bytes in the same packing orders + one power-of-two scale per output column
  uint8_t *o_attn = nullptr, *o_fc = nullptr, *o_proj = nullptr, *o_fc2 = nullptr;
  float *os_attn = nullptr, *os_fc = nullptr, *os_proj = nullptr, *os_fc2 = nullptr;
};

struct ArState {
  int n_layers = 0;
  std::vector<ArLayerDev> L;
  float *text_emb = nullptr, *text_pos = nullptr, *mel_emb = nullptr, *mel_pos = nullptr;
  float *lnf_g = nullptr, *lnf_b = nullptr, *lmh_g = nullptr, *lmh_b = nullptr;
  float *lm_w = nullptr /*[1024][VPAD] strip-major*/, *lm_b = nullptr /*[VPAD]*/, *d_lm = nullptr /*mfma16, lm_head.0 folded*/, *d_lmb = nullptr;
  __half *dh_lm = nullptr; // mfma16h hi | lo
  __half *q_lm = nullptr;  // mfma16h fp16 (option ar_weights = 1 at load)
  uint8_t *o_lm = nullptr; // mfma16h e4m3 (option ar_weights = 2 at load)
  float *os_lm = nullptr;
  int loaded_wmode = 0;    // the reduced-precision decode slabs this state was loaded with (0 = none, 1 = fp16, 2 = fp8)
  bool f32_mfma = false;   // option "dec_f32_mfma" at load: LayerNorm-GEMVs on v_mfma_f32_16x16x4_f32 (exact f32 products) instead of split fp16
  std::vector<void *> owned;
  // run state
  int B = 0, n_text = 0, P = 0, max_pos = 0; // several prompts (tts_ar_begin_multi): n_text / P of the LONGEST prompt
  bool prefill_done = false; // the prompt's K/V rows are in the decode cache (set by ar_prefill, cleared by ar_begin)
  std::vector<int> tokens;   // the prompts back to back
  // Prompt groups: group g holds candidates [g_c0[g], g_c0[g] + g_n[g]) and the prompt tokens[g_t0[g] .. + g_ntext[g]). One group = the single-prompt
  // path of rounds 1-6 (multi = false); several: the decode step reads every row's context length from row_off (multi = true).
  std::vector<int> g_c0, g_n, g_t0, g_ntext;
  std::vector<int> g_voice;  // group g's row of the voice table `voice` ([n_voices][1024]; the single-voice entry points: one row, all 0)
  bool multi = false;
  // A session (tts_ar_session_*): B slots, each row at its own step. The step's first kernel writes every row's context length into row_off and sets the
  // step state's n_past to 0 (embed_session_kernel); the host block behind h_toks is [tokens[B] | n_past[Bpad] | pos_id[B]].
  bool session = false;
  // A session opened with TTS_AR_ROW_CONTROLS: its step ends with sample_prefilter_rows_kernel, which reads every row's sampler controls from ctl
  // ([tiles * 16] int4 {pf_min_for(top_k), penalty bits, penalty scope, typical mass bits}; reserved at open, written by ar_session_controls outside the graph). Such a step
  // bakes none of step_scope / step_pf_min / step_penalty and has a graph slot of its own, so a uniform session of the same shape keeps its graph.
  bool rows = false;
  DevBuf ctl;
  int sess_captures0 = -1;   // graph_captures when the session's first step had run (tts_ar_session_recaptures)
  DevBuf row_off;            // multi: [tiles * 16] ints, P of the row's group (0 past the batch); the step state's n_past is then the step index
  DevBuf voice, kcache, vcache, lat_k, lat_v;
  // Session audio (tts_ar_session_enable_audio): the latent pass' K/V rows of every slot, kept from one incremental pass (ar_session_extend) to the next:
  // [layer][slot][sa_S][1024] fp16 each, sa_S = 1 + max_text + min(502, max_steps + 10), that is 2 * n_layers * n_slots * sa_S * 2048 bytes in all, about as
  // much again as the session's decode cache (kcache + vcache: max_text + 2 + max_steps + 1 positions per slot). The decode cache's own mel rows cannot
  // serve: they come from the GEMV path, in another summation order.
  DevBuf sa_k, sa_v, sa_tab; // sa_tab: one launch sequence's tables, [items int4[n_slots] | row_dst int[sa_rows]]
  int sa_S = 0;              // 0: the session has no audio
  int sa_rows = 0;           // the most rows one launch sequence packs (the buffers reserved at enable time hold them)
  DevBuf h, xn, qkv, att, ff, part, desc, logits, hn, a_hi, a_lo;
  DevBuf score_ws, score_io; // ar_score_rows: the slab partials; [targets | lse | logp | stop_logp | greedy] of the scored rows
  // decode-step graph
  DevBuf d_toks;
  int32_t *h_toks = nullptr;   // pinned
  float *h_logits = nullptr;   // pinned [B][8194]
  int32_t *h_pf = nullptr;     // pinned [B][TTS_PF_WORDS]: the device prefilter's lists (step_mode != 0), written by the kernel itself
  int step_mode = 0;           // what the step hands to the host: 0 = the logits, 1 = the prefilter's lists, 2 = lists with the stop token masked
  int h_cap_B = 0;             // candidates the pinned buffers were sized for
  // Penalty scope 1 (option "ar_penalty_scope"): per candidate the set of ids fed since ar_begin_groups plus 1 and 8192, [B][TTS_HIST_WORDS]. The host copy is
  // kept by every ar_step whatever the scope (B stores); the device copy is what the scope-1 step graphs read and extend, and is uploaded from the host copy
  // by the first scope-1 step after a begin or after a scope-0 step (which does not touch it).
  std::vector<uint32_t> hist_host;
  DevBuf hist;
  bool hist_dev_valid = false;
  int step_scope = 0, step_pf_min = TTS_PF_MIN; // what the step being enqueued bakes in: the penalty scope, the prefilter's keep bound
  float step_penalty = 2.0f;                    // and, under scope 1 or typical sampling, the penalty
  float step_mass = 0.f;                        // and the typical mass (0: the prefilter kernels of before)
  // one captured step per mode (a caller alternating tts_ar_step / tts_ar_step_sample, or bench's device_topk on/off loop, re-instantiated
  // the ~150-node graph on every switch)
  hipGraph_t graphs[5] = {};         // [3]: the session step (one mode per session; kept across sessions of the same shape); [4]: a rows session's step
  hipGraphExec_t graph_execs[5] = {};
  int graph_captures = 0; // decode-step graphs captured since the model was loaded (tts_ar_graph_captures)
  // everything the captured step bakes into its nodes: the graph of the previous utterance is replayed when nothing moved
  struct GraphSig {
    int B = 0, max_pos = 0, lut = 0, wmode = 0, mode = 0, multi = 0; // multi: 2 = a session step
    int rows = 0;              // a session with per-row controls: scope, pf_min and penalty below are 0, the history sets and the control table are always in p
    int scope = 0, pf_min = 0; // the sampler controls a step bakes in: penalty scope (an extra node / the penalising prefilter), the prefilter's keep bound (modes 1, 2)
    float penalty = 0;         // scope 1 or typical sampling, modes 1 / 2
    float mass = 0;            // the typical mass, modes 1 / 2
    const void *p[14] = {};
    bool operator==(const GraphSig &o) const {
      return B == o.B && max_pos == o.max_pos && lut == o.lut && wmode == o.wmode && mode == o.mode && multi == o.multi && rows == o.rows && scope == o.scope &&
             pf_min == o.pf_min && penalty == o.penalty && mass == o.mass && std::equal(p, p + 14, o.p);
    }
  } graph_sigs[5];
  GraphSig current_sig(int lut, int wmode) const {
    GraphSig g;
    g.B = B; g.max_pos = max_pos; g.lut = lut; g.wmode = wmode; g.mode = step_mode; g.multi = session ? 2 : multi;
    const bool rw = session && rows;
    g.rows = rw;
    g.scope = rw ? 0 : step_scope; g.pf_min = (step_mode && !rw) ? step_pf_min : 0; g.mass = (step_mode && !rw) ? step_mass : 0.f;
    g.penalty = ((step_scope || g.mass > 0.f) && step_mode && !rw) ? step_penalty : 0.f;
    const void *q[14] = {h.p, qkv.p, att.p, ff.p, kcache.p, vcache.p, d_toks.p, logits.p, h_toks, h_logits, h_pf, (multi || session) ? row_off.p : nullptr,
                         (step_scope || rw) ? hist.p : nullptr, rw ? ctl.p : nullptr};
    std::copy(q, q + 14, g.p);
    return g;
  }
  void drop_graph(int m) {
    if (graph_execs[m]) (void)hipGraphExecDestroy(graph_execs[m]);
    if (graphs[m]) (void)hipGraphDestroy(graphs[m]);
    graph_execs[m] = nullptr; graphs[m] = nullptr;
  }
  ~ArState() {
    for (int m = 0; m < 5; m++) drop_graph(m);
    if (h_toks) (void)hipHostFree(h_toks);
    if (h_logits) (void)hipHostFree(h_logits);
    if (h_pf) (void)hipHostFree(h_pf);
    for (void *p : owned) (void)hipFree(p);
  }
};

// ---------------------------------------------------------------------------------------------
// loader
// ---------------------------------------------------------------------------------------------
// ---- OCP fp8 e4m3 (1-4-3, bias 7, largest finite 448, no infinities): round to nearest even, saturating ----
static uint8_t fp8_e4m3_encode(float f) {
  const uint8_t sign = std::signbit(f) ? 0x80 : 0;
  float a = std::fabs(f);
  if (!(a == a)) return sign | 0x7f;
  if (a >= 448.0f) return sign | 0x7e;
  if (a < 0.0009765625f) return sign; // below half of the smallest subnormal (2^-9 / 2): rounds to zero (ties-to-even at exactly 2^-10 -> 0)
  int e;
  (void)std::frexp(a, &e);           // a = m 2^e, m in [0.5, 1)
  int ex = e - 1;                    // a = 1.xxx 2^ex
  if (ex < -6) ex = -6;              // subnormals share the exponent of the smallest normal
  const float q = std::ldexp(1.0f, ex - 3); // spacing of representable values in this binade
  float r = std::nearbyint(a / q) * q;      // default rounding mode: to nearest even
  if (r >= 448.0f) return sign | 0x7e;
  if (r < 0.015625f) return sign | (uint8_t)std::lrint(r / 0.001953125f); // subnormal: mantissa = r / 2^-9
  (void)std::frexp(r, &e);
  ex = e - 1;
  const int mant = (int)std::lrint(r / std::ldexp(1.0f, ex - 3)) - 8;
  return sign | (uint8_t)(((ex + 7) << 3) | mant);
}
extern "C" uint8_t tts_host_fp8_e4m3(float v) { return fp8_e4m3_encode(v); }
// one power-of-two scale per output column, the smallest with max |w| / scale <= 448 (exact scaling: a matrix whose entries are
// e4m3 values times a power of two per column survives the round trip unchanged)
static std::vector<float> fp8_col_scales(const float *w, int K, int N) {
  std::vector<float> sc(N, 1.0f);
  for (int n = 0; n < N; n++) {
    float amax = 0.f;
    for (int k = 0; k < K; k++) amax = std::max(amax, std::fabs(w[(size_t)k * N + n]));
    if (amax > 0.f) {
      int e;
      (void)std::frexp(amax / 448.0f, &e); // amax / 448 = m 2^e, m in [0.5, 1)  ->  2^e >= amax / 448
      sc[n] = std::ldexp(1.0f, amax / 448.0f == std::ldexp(0.5f, e) ? e - 1 : e);
    }
  }
  return sc;
}

// ---- host packers: a loop over the output offsets of a layout (the *_at maps beside the pk_* kernels, where the layouts are described) and one element encoder ----
struct EncF32 { float operator()(float w, size_t) const { return w; } };
struct EncF16 { float scale; __half operator()(float w, size_t) const { return __float2half_rn(scale * w); } };      // scale 1 or 64: exact
struct EncFp8 { const float *sc; uint8_t operator()(float w, size_t n) const { return fp8_e4m3_encode(w / sc[n]); } }; // sc: fp8_col_scales
// t[o] = enc(w[k][n], n) with (k, n) = at(o): every layout and encoding whose value for offset o lies AT o. RUN consecutive offsets have consecutive sources (a row of
// a strip: 64, the columns of cols4: 4), so the map is evaluated once per run
template <class T, int RUN, class At, class Enc> static std::vector<T> pack(const float *w, int K, int N, At at, Enc enc) {
  std::vector<T> t((size_t)K * N);
  for (size_t o = 0; o < t.size(); o += RUN) {
    const auto a = at(o);
    const float *src = &w[a.k * N + a.n];
    for (int j = 0; j < RUN; j++) t[o + j] = enc(src[j], a.n + j);
  }
  return t;
}
static std::vector<float> strip_major(const float *w, int K, int N) {
  return pack<float, 64>(w, K, N, [=](size_t o) { return strip_major_at(o, K, N); }, EncF32{});
}
static std::vector<__half> pack_mfma16h(const float *w, int N) { // the split-precision encoding: hi | lo
  std::vector<__half> t((size_t)1024 * N * 2);
  for (size_t i = 0; i < (size_t)1024 * N; i++) {
    const Mfma16hAt a = mfma16h_at(i);
    const HiLo v = split_hilo(w[a.k * N + a.n]);
    t[a.hilo] = v.hi;
    t[a.hilo + 8] = v.lo;
  }
  return t;
}
static std::vector<uint8_t> pack_mfma16o(const float *w, int N, const std::vector<float> &sc) { // the e4m3 encoding
  std::vector<uint8_t> t((size_t)1024 * N);
  for (size_t i = 0; i < t.size(); i++) {
    const Mfma16hAt a = mfma16h_at(i);
    t[a.fp8] = fp8_e4m3_encode(w[a.k * N + a.n] / sc[a.n]);
  }
  return t;
}

// LayerNorm affine folded into the matrix it feeds: (xhat*g + b) W + c = xhat (diag(g) W) + (b W + c).
static void fold_layernorm(const float *w, int K, int N, const float *g, const float *b, const float *c,
                           std::vector<float> &wf, std::vector<float> &cf) {
  wf.resize((size_t)K * N);
  std::vector<double> acc(N, 0.0);
  for (int k = 0; k < K; k++)
    for (int n = 0; n < N; n++) {
      wf[(size_t)k * N + n] = g[k] * w[(size_t)k * N + n];
      acc[n] += (double)b[k] * (double)w[(size_t)k * N + n];
    }
  cf.resize(N);
  for (int n = 0; n < N; n++) cf[n] = (float)((double)c[n] + acc[n]);
}

namespace {
// The four matrices [K][N] of a layer and where their layouts go: strip-major f32 (multi-row GEMV), the hi | lo copy of the multi-row MFMA passes, and the decode slab
// as f32 / fp16 (option ar_weights = 1) / e4m3 + column scales (ar_weights = 2) — in cols4 order, or for the two matrices a LayerNorm feeds (LAYER_FOLDS) in mfma16 /
// mfma16h order with the LayerNorm folded in (the f32 one only under dec_f32_mfma; their default slab is LayerFold::dh).
struct LayerMat {
  const char *suffix; int K, N;
  float *ArLayerDev::*strip; __half *ArLayerDev::*split;
  float *ArLayerDev::*d; __half *ArLayerDev::*q; uint8_t *ArLayerDev::*o; float *ArLayerDev::*os;
};
const LayerMat LAYER_MATS[4] = {
    {".attn.c_attn.weight", D, 3 * D, &ArLayerDev::w_attn, &ArLayerDev::s_attn, &ArLayerDev::d_attn, &ArLayerDev::q_attn, &ArLayerDev::o_attn, &ArLayerDev::os_attn},
    {".attn.c_proj.weight", D, D, &ArLayerDev::w_proj, &ArLayerDev::s_proj, &ArLayerDev::d_proj, &ArLayerDev::q_proj, &ArLayerDev::o_proj, &ArLayerDev::os_proj},
    {".mlp.c_fc.weight", D, FF, &ArLayerDev::w_fc, &ArLayerDev::s_fc, &ArLayerDev::d_fc, &ArLayerDev::q_fc, &ArLayerDev::o_fc, &ArLayerDev::os_fc},
    {".mlp.c_proj.weight", FF, D, &ArLayerDev::w_fc2, &ArLayerDev::s_fc2, &ArLayerDev::d_fc2, &ArLayerDev::q_fc2, &ArLayerDev::o_fc2, &ArLayerDev::os_fc2}};
// LayerNorm `ln` (gain g, offset b) folded into LAYER_MATS[mat] (bias c): split-precision slab dh, folded bias db
struct LayerFold {
  int mat; const char *ln, *bias;
  float *ArLayerDev::*g, *ArLayerDev::*b, *ArLayerDev::*c;
  __half *ArLayerDev::*dh; float *ArLayerDev::*db;
};
const LayerFold LAYER_FOLDS[2] = {
    {0, ".ln_1", ".attn.c_attn.bias", &ArLayerDev::ln1_g, &ArLayerDev::ln1_b, &ArLayerDev::b_attn, &ArLayerDev::dh_attn, &ArLayerDev::db_attn},
    {2, ".ln_2", ".mlp.c_fc.bias", &ArLayerDev::ln2_g, &ArLayerDev::ln2_b, &ArLayerDev::b_fc, &ArLayerDev::dh_fc, &ArLayerDev::db_fc}};
struct FoldDst { float **d; __half **dh; float **db; __half **q; uint8_t **o; float **os; }; // a layer's (the two tables) or the head's

// Device layouts from the file's tensors. Two ways (equal byte for byte): kernels from uploaded file-order copies (option load_device_pack, default 1, for the default
// decode arithmetic), or the host packers — kept for the reduced-precision slab options and the f32-MFMA variant (they are A/B options) and for load_threads = 1 (the
// serial loader, the reference of the equality test). head(), globals() and layer(i) are independent jobs run on several threads (common.h: run_parallel): `owned` and
// `temps` are touched under `mu`.
struct ArLoader {
  tts_ctx *ctx; ArState *st; const WeightFile &wf; const bool dev_pack;
  const bool pinned;               // load_threads = 1 copies without the pool, as the serial loader always did
  PinnedPool pin{(size_t)18 << 20, 6};
  std::mutex mu;
  std::vector<void *> temps;       // file-order copies and folded matrices: freed once the packing kernels have run
  // temporaries come out of ONE device allocation (a few hundred hipMalloc / hipFree pairs cost 0.1 s): the file's tensors once more + the gain-folded matrices + the head
  char *arena = nullptr; size_t arena_cap = 0; std::atomic<size_t> arena_at{0};
  // ... and so do the layouts that stay (4.4 GB in ~400 pieces: one hipMalloc now, one hipFree in tts_destroy)
  char *keep = nullptr; size_t keep_cap = 0; std::atomic<size_t> keep_at{0};
  unsigned *d_max = nullptr;       // device path: max |w| bits, per layer the four matrices, then the two gain-folded ones
  const std::string hp = "inference_model.transformer.h.";
  ArLoader(tts_ctx *c, ArState *s, const WeightFile &w, bool dp) : ctx(c), st(s), wf(w), dev_pack(dp), pinned(c->load_threads != 1) {}
  ~ArLoader() {
    for (void *q : temps) (void)hipFree(q);
    if (arena) (void)hipFree(arena);
  }
  static int pgrid(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 8192); }

  int reserve() { // device path: the two arenas (without them: one allocation per buffer) and the max |w| slots
    if (!dev_pack) return TTS_OK;
    size_t need = (size_t)st->n_layers * ((size_t)D * 3 * D + (size_t)D * FF) * 4 + (size_t)3 * D * VPAD * 4 + ((size_t)8 << 20);
    for (auto &kv : wf.t) need += (size_t)kv.second.nelem() * 4 + 256;
    if (hipMalloc((void **)&arena, need) == hipSuccess) arena_cap = need;
    else (void)hipGetLastError();
    const size_t per_layer = ((size_t)12 * D * D) * 4 /* strip-major f32 */ + ((size_t)7 * D * D) * 4 /* split-fp16 decode slabs */ + ((size_t)5 * D * D) * 4 /* 4-column slabs */ +
                             ((size_t)12 * D * D) * 4 /* hi | lo copies for the multi-row passes */ + (size_t)(3 * D + FF) * 4 + 64 * 256;
    need = (size_t)st->n_layers * per_layer + (size_t)D * VPAD * 8 + (size_t)VPAD * 4 + ((size_t)1 << 20);
    if (hipMalloc((void **)&keep, need) == hipSuccess) { keep_cap = need; st->owned.push_back(keep); }
    else (void)hipGetLastError();
    const size_t nmax = (size_t)st->n_layers * 6 * 4;
    if (!(d_max = (unsigned *)alloc(nmax, true))) return TTS_ERR_HIP;
    TTS_HIP(ctx, hipMemsetAsync(d_max, 0, nmax, ctx->stream));
    return TTS_OK;
  }
  void *fresh(size_t bytes, bool temp) { // an allocation of its own: the state's, or (temp) the loader's
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); fail(ctx, TTS_ERR_HIP, "hipMalloc of %zu bytes failed while loading the AR model", bytes); return nullptr; }
    std::lock_guard<std::mutex> lk(mu);
    (temp ? temps : st->owned).push_back(q);
    return q;
  }
  void *alloc(size_t bytes, bool temp) { // out of the arena of its kind while there is one with room
    char *base = temp ? arena : keep;
    if (base) {
      const size_t sz = (bytes + 255) & ~(size_t)255, at = (temp ? arena_at : keep_at).fetch_add(sz);
      if (at + sz <= (temp ? arena_cap : keep_cap)) return base + at;
    }
    return fresh(bytes, temp);
  }
  hipError_t h2d(void *dst, const void *src, size_t bytes) { return pinned ? pin.upload(dst, src, bytes, ctx->load_stream) : PinnedPool::copy_now(dst, src, bytes, ctx->load_stream); }
  template <class T> int put(const std::vector<T> &h, T **dst) {
    void *p = fresh(h.size() * sizeof(T), false);
    if (!p) return TTS_ERR_HIP;
    TTS_HIP(ctx, h2d(p, h.data(), h.size() * sizeof(T)));
    *dst = (T *)p;
    return TTS_OK;
  }
  const HostTensor *get(const std::string &name, int64_t ne0, int64_t ne1) {
    auto it = wf.t.find(name);
    if (it == wf.t.end()) { fail(ctx, TTS_ERR_FORMAT, "tensor '%s' missing from AR model file", name.c_str()); return nullptr; }
    const HostTensor &t = it->second;
    if (t.ne[0] != ne0 || t.ne[1] != ne1 || t.nelem() != ne0 * ne1) {
      fail(ctx, TTS_ERR_FORMAT, "tensor '%s' has wrong shape in model file: got [%d, %d], expected [%d, %d]", name.c_str(), (int)t.ne[0], (int)t.ne[1], (int)ne0, (int)ne1);
      return nullptr;
    }
    return &t;
  }
  // the tensor as it lies in the file into a device buffer of its own (temp: one that lives as long as the loader); a payload that read_weight_file left in the file
  // (device path) goes file -> pinned staging -> device
  int to_device(const std::string &name, const HostTensor &t, bool temp, float **dst) {
    const size_t bytes = (size_t)t.nelem() * 4;
    void *q = temp ? alloc(bytes, true) : fresh(bytes, false);
    if (!q) return TTS_ERR_HIP;
    if (t.data.empty() && t.file_off >= 0) {
      std::pair<void *, size_t> b = pinned ? pin.take(bytes) : std::pair<void *, size_t>{nullptr, 0};
      std::vector<float> tmp;
      void *host = b.first;
      if (!host) { tmp.resize((size_t)t.nelem()); host = tmp.data(); }
      const bool ok = wf.read_payload(t, host);
      const hipError_t e = ok ? PinnedPool::copy_now(q, host, bytes, ctx->load_stream) : hipSuccess;
      pin.give(b);
      if (!ok) return fail(ctx, TTS_ERR_IO, "autoregressive_model_load: tensor '%s' truncated", name.c_str());
      TTS_HIP(ctx, e);
    } else TTS_HIP(ctx, h2d(q, t.data.data(), bytes));
    *dst = (float *)q;
    return TTS_OK;
  }
  int f32(const std::string &name, int64_t ne0, int64_t ne1, float **dst, bool temp = false) {
    const HostTensor *t = get(name, ne0, ne1);
    return t ? to_device(name, *t, temp, dst) : (int)TTS_ERR_FORMAT;
  }
  const float *host(const std::string &name) { return wf.t.at(name).data.data(); } // of a tensor that get() has seen

  // The split-precision layouts hold 64 W as fp16 hi | lo (W16_SCALE): a trained GPT-2 never comes near |W| = 937, but a file that does must fail loudly instead of
  // turning into an fp16 infinity inside the MFMA operands (the diffusion stage's proj_out pair picks its scale per tensor instead). Checked per layer for the four
  // matrices of the file, then the two gain-folded ones: on the host path as they are built, on the device path from pk_absmax_kernel's results after the jobs.
  int range_guard(const std::string &name, float m) {
    if (m * W16_SCALE < 60000.0f) return TTS_OK;
    return fail(ctx, TTS_ERR_FORMAT, "tensor '%s': max |w| = %g does not fit the split-precision fp16 layout (|w| < %g)", name.c_str(), m, 60000.0 / W16_SCALE);
  }
  static float host_absmax(const float *w, size_t n) {
    float m = 0.f;
    for (size_t i = 0; i < n; i++) m = std::max(m, std::fabs(w[i]));
    return m;
  }
  std::string guard_name(const std::string &layer, int j) {
    return j < 4 ? layer + LAYER_MATS[j].suffix : layer + LAYER_MATS[LAYER_FOLDS[j - 4].mat].suffix + " (LayerNorm gain folded in)";
  }
  int device_range_guard() {
    if (!dev_pack) return TTS_OK;
    TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float> mx((size_t)st->n_layers * 6); // the bits pk_absmax_kernel ordered as unsigned integers
    TTS_HIP(ctx, hipMemcpy(mx.data(), d_max, mx.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < st->n_layers; i++)
      for (int j = 0; j < 6; j++)
        if (int r = range_guard(guard_name(hp + std::to_string(i), j), mx[(size_t)i * 6 + j])) return r;
    return TTS_OK;
  }

  // LayerNorm (g, b) folded into w [D][N] with bias c — the gain into the matrix, b . w + c as the new bias — and every decode slab of the folded matrix.
  // Host path (w, g, b, c on the host): folded once, then each slab that the options ask for, before the caller folds its next matrix.
  int fold_host(const float *w, int N, const float *g, const float *b, const float *c, const std::string *guard, const FoldDst &dst) {
    std::vector<float> wfold, cfold;
    fold_layernorm(w, D, N, g, b, c, wfold, cfold);
    int r;
    if (guard && (r = range_guard(*guard, host_absmax(wfold.data(), wfold.size())))) return r;
    if (st->f32_mfma && (r = put(pack<float, 1>(wfold.data(), D, N, [](size_t o) { return mfma16_at(o); }, EncF32{}), dst.d))) return r;
    if ((r = put(pack_mfma16h(wfold.data(), N), dst.dh)) || (r = put(cfold, dst.db))) return r;
    if (ctx->ar_weights == 1 && (r = put(pack<__half, 1>(wfold.data(), D, N, [](size_t i) { return mfma16h_at(i); }, EncF16{W16_SCALE}), dst.q))) return r;
    if (ctx->ar_weights == 2) {
      const std::vector<float> sc = fp8_col_scales(wfold.data(), D, N);
      if ((r = put(pack_mfma16o(wfold.data(), N, sc), dst.o)) || (r = put(sc, dst.os))) return r;
    }
    return TTS_OK;
  }
  // Device path (w the file-order copy, g, b, c on the device): the default slab and bias; max |folded w| into *mx when given
  int fold_dev(const float *w, int N, const float *g, const float *b, const float *c, unsigned *mx, const FoldDst &dst) {
    const size_t n = (size_t)D * N;
    float *fold = (float *)alloc(n * 4, true);
    if (!fold || !(*dst.dh = (__half *)alloc(n * 2 * sizeof(__half), false)) || !(*dst.db = (float *)alloc((size_t)N * 4, false))) return TTS_ERR_HIP;
    pk_fold_kernel<<<pgrid(n), 256, 0, ctx->stream>>>(w, D, N, g, fold);
    if (mx) pk_absmax_kernel<<<std::min(pgrid(n), 1024), 256, 0, ctx->stream>>>(fold, n, mx);
    pk_mfma16h_kernel<<<pgrid(n), 256, 0, ctx->stream>>>(fold, N, *dst.dh);
    pk_fold_bias_kernel<<<(N + 255) / 256, 256, 0, ctx->stream>>>(w, D, N, b, c, *dst.db);
    return TTS_OK;
  }

  int globals() {
    int r;
    if ((r = f32("text_embedding.weight", D, 256, &st->text_emb)) || (r = f32("text_pos_embedding.emb.weight", D, 404, &st->text_pos)) ||
        (r = f32("mel_embedding.weight", D, V, &st->mel_emb)) || (r = f32("mel_pos_embedding.emb.weight", D, 608, &st->mel_pos)) ||
        (r = f32("inference_model.transformer.ln_f.weight", D, 1, &st->lnf_g)) || (r = f32("inference_model.transformer.ln_f.bias", D, 1, &st->lnf_b)) ||
        (r = f32("inference_model.lm_head.0.weight", D, 1, &st->lmh_g)) || (r = f32("inference_model.lm_head.0.bias", D, 1, &st->lmh_b))) return r;
    return TTS_OK;
  }
  // One layer = 50 MB of f32 weights re-tiled into the decode slabs, the strip-major copies and (after the jobs) the split-fp16 MFMA layouts; on the host ~0.2 s of one
  // core + the uploads (tts_load_ar 5.9 s on one thread: see DESIGN.md section 5). The two paths differ in who runs the permutations.
  int layer(int i) {
    const std::string p = hp + std::to_string(i);
    ArLayerDev &l = st->L[i];
    int r;
    if ((r = f32(p + ".ln_1.weight", D, 1, &l.ln1_g)) || (r = f32(p + ".ln_1.bias", D, 1, &l.ln1_b)) || (r = f32(p + ".ln_2.weight", D, 1, &l.ln2_g)) ||
        (r = f32(p + ".ln_2.bias", D, 1, &l.ln2_b)) || (r = f32(p + ".attn.c_attn.bias", 3 * D, 1, &l.b_attn)) || (r = f32(p + ".attn.c_proj.bias", D, 1, &l.b_proj)) ||
        (r = f32(p + ".mlp.c_fc.bias", FF, 1, &l.b_fc)) || (r = f32(p + ".mlp.c_proj.bias", D, 1, &l.b_fc2))) return r;
    const HostTensor *t[4];
    for (int j = 0; j < 4; j++)
      if (!(t[j] = get(p + LAYER_MATS[j].suffix, LAYER_MATS[j].N, LAYER_MATS[j].K))) return TTS_ERR_FORMAT;
    const float *w[4]; // the matrices in file order: on the host, or (device path) temporary copies on the device
    for (int j = 0; j < 4; j++) {
      const LayerMat &m = LAYER_MATS[j];
      const size_t n = (size_t)m.K * m.N;
      if (dev_pack) {
        float *raw = nullptr;
        if ((r = to_device(p + m.suffix, *t[j], true, &raw))) return r;
        if (!(l.*m.strip = (float *)alloc(n * 4, false))) return TTS_ERR_HIP;
        pk_strip_major_kernel<<<pgrid(n), 256, 0, ctx->stream>>>(raw, m.K, m.N, l.*m.strip);
        pk_absmax_kernel<<<std::min(pgrid(n), 1024), 256, 0, ctx->stream>>>(raw, n, d_max + (size_t)i * 6 + j);
        w[j] = raw;
      } else {
        w[j] = t[j]->data.data();
        if ((r = put(strip_major(w[j], m.K, m.N), &(l.*m.strip)))) return r;
      }
    }
    if (!dev_pack)
      for (int j = 0; j < 4; j++)
        if ((r = range_guard(guard_name(p, j), host_absmax(w[j], t[j]->data.size())))) return r;
    for (int q = 0; q < 2; q++) {
      const LayerFold &f = LAYER_FOLDS[q];
      const LayerMat &m = LAYER_MATS[f.mat];
      const FoldDst dst{&(l.*m.d), &(l.*f.dh), &(l.*f.db), &(l.*m.q), &(l.*m.o), &(l.*m.os)};
      const std::string guard = guard_name(p, 4 + q);
      if ((r = dev_pack ? fold_dev(w[f.mat], m.N, l.*f.g, l.*f.b, l.*f.c, d_max + (size_t)i * 6 + 4 + q, dst)
                        : fold_host(w[f.mat], m.N, host(p + f.ln + ".weight"), host(p + f.ln + ".bias"), host(p + f.bias), &guard, dst))) return r;
    }
    for (int j = 0; j < 4; j++) { // the two that no LayerNorm feeds: 4-column slabs
      const LayerMat &m = LAYER_MATS[j];
      if (j == LAYER_FOLDS[0].mat || j == LAYER_FOLDS[1].mat) continue;
      const auto at = [&m](size_t o) { return cols4_at(o, m.K); };
      if (dev_pack) {
        if (!(l.*m.d = (float *)alloc((size_t)m.K * m.N * 4, false))) return TTS_ERR_HIP;
        pk_cols4_kernel<<<pgrid((size_t)m.K * m.N), 256, 0, ctx->stream>>>(w[j], m.K, m.N, l.*m.d);
        continue;
      }
      if ((r = put(pack<float, 4>(w[j], m.K, m.N, at, EncF32{}), &(l.*m.d)))) return r;
      if (ctx->ar_weights == 1 && (r = put(pack<__half, 4>(w[j], m.K, m.N, at, EncF16{1.0f}), &(l.*m.q)))) return r;
      if (ctx->ar_weights == 2) {
        const std::vector<float> sc = fp8_col_scales(w[j], m.K, m.N);
        if ((r = put(pack<uint8_t, 4>(w[j], m.K, m.N, at, EncFp8{sc.data()}), &(l.*m.o))) || (r = put(sc, &(l.*m.os)))) return r;
      }
    }
    if (dev_pack) TTS_HIP(ctx, hipGetLastError());
    return TTS_OK;
  }
  // lm_head.1: nn.Linear [8194][1024] -> [1024][VPAD] so that it streams like the Conv1D weights, lm_head.0's LayerNorm folded into its decode slabs
  int head() {
    const std::string w1 = "inference_model.lm_head.1.weight", ln = "inference_model.lm_head.0";
    auto it = wf.t.find(w1), ib = wf.t.find("inference_model.lm_head.1.bias");
    if (it == wf.t.end() || ib == wf.t.end()) return fail(ctx, TTS_ERR_FORMAT, "lm_head.1 missing from model file");
    if (it->second.ne[0] != D || it->second.ne[1] != V || ib->second.nelem() != V)
      return fail(ctx, TTS_ERR_FORMAT, "tensor 'inference_model.lm_head.1.weight' has wrong shape in model file");
    const HostTensor *g0 = get(ln + ".weight", D, 1), *b0 = get(ln + ".bias", D, 1);
    if (!g0 || !b0) return TTS_ERR_FORMAT;
    std::vector<float> bt(VPAD, 0.f);
    std::copy(ib->second.data.begin(), ib->second.data.end(), bt.begin());
    int r;
    if ((r = put(bt, &st->lm_b))) return r;
    const FoldDst dst{&st->d_lm, &st->dh_lm, &st->d_lmb, &st->q_lm, &st->o_lm, &st->os_lm};
    const size_t n = (size_t)D * VPAD;
    if (dev_pack) {
      float *raw = nullptr, *g = nullptr, *b = nullptr, *wt = (float *)alloc(n * 4, true);
      if ((r = to_device(w1, it->second, true, &raw)) || (r = to_device(ln + ".weight", *g0, true, &g)) || (r = to_device(ln + ".bias", *b0, true, &b))) return r;
      if (!wt || !(st->lm_w = (float *)alloc(n * 4, false))) return TTS_ERR_HIP;
      pk_transpose_pad_kernel<<<pgrid(n), 256, 0, ctx->stream>>>(raw, V, D, VPAD, wt);
      pk_strip_major_kernel<<<pgrid(n), 256, 0, ctx->stream>>>(wt, D, VPAD, st->lm_w);
      if ((r = fold_dev(wt, VPAD, g, b, st->lm_b, nullptr, dst))) return r;
      TTS_HIP(ctx, hipGetLastError());
      return TTS_OK;
    }
    std::vector<float> wt(n, 0.f);
    const float *w = it->second.data.data();
    for (int v = 0; v < V; v++)
      for (int k = 0; k < D; k++) wt[(size_t)k * VPAD + v] = w[(size_t)v * D + k];
    if ((r = put(strip_major(wt.data(), D, VPAD), &st->lm_w))) return r;
    return fold_host(wt.data(), VPAD, g0->data.data(), b0->data.data(), bt.data(), nullptr, dst);
  }
  int split_copies() { // hi | lo copies for the multi-row MFMA path, from the strip-major ones
    for (ArLayerDev &l : st->L)
      for (const LayerMat &m : LAYER_MATS) {
        if (!(l.*m.split = (__half *)alloc((size_t)m.N * 2 * m.K * sizeof(__half), false))) return TTS_ERR_HIP;
        split_weight_kernel<<<dim3(m.N / 32, m.K / 32), 256, 0, ctx->stream>>>(l.*m.strip, m.K, m.N, l.*m.split);
      }
    return TTS_OK;
  }
};
} // namespace

void ar_free(ArState *s) { delete s; }

int ar_load(tts_ctx *ctx, const char *path) {
  static const bool timing = getenv("TTS_TIMING") != nullptr; // host-side breakdown on stderr
  const auto t0 = std::chrono::steady_clock::now();
  auto since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
  // (decided before the file is read: with device-side packing the large tensors stay in the file until a worker wants them)
  const bool dev_pack = ctx->load_device_pack != 0 && ctx->load_threads != 1 && ctx->dec_f32_mfma == 0 && ctx->ar_weights == 0;
  WeightFile wf;
  std::string err;
  int rc = read_weight_file(path, wf, err, dev_pack ? (size_t)256 << 10 : (size_t)-1);
  const double t_read = since(t0);
  if (rc != TTS_OK) return fail(ctx, rc, "autoregressive_model_load: %s", err.c_str());
  std::unique_ptr<ArState> st(new ArState());
  ArLoader ld(ctx, st.get(), wf, dev_pack);
  st->f32_mfma = ctx->dec_f32_mfma != 0;
  while (wf.has(ld.hp + std::to_string(st->n_layers) + ".ln_1.weight")) st->n_layers++;
  if (st->n_layers == 0) return fail(ctx, TTS_ERR_FORMAT, "no transformer layers in '%s'", path);
  // every tensor in the file must be known (main.cpp:834-838)
  for (auto &kv : wf.t) {
    const std::string &n = kv.first;
    bool ok = n == "text_embedding.weight" || n == "text_pos_embedding.emb.weight" || n == "mel_embedding.weight" ||
              n == "mel_pos_embedding.emb.weight" || n.rfind("inference_model.", 0) == 0;
    if (!ok) return fail(ctx, TTS_ERR_FORMAT, "unknown tensor '%s' in model file", n.c_str());
  }
  st->L.resize(st->n_layers);
  if ((rc = ld.reserve())) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  if ((rc = run_parallel(ctx, st->n_layers + 2, [&](int i) { return i == 0 ? ld.head() : i == 1 ? ld.globals() : ld.layer(i - 2); }))) return rc; // the head (0.2 s) first
  if ((rc = ld.device_range_guard())) return rc;
  const double t_layers = since(t1);
  if ((rc = ld.split_copies())) return rc;
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st->loaded_wmode = ctx->ar_weights;
  if (ctx->ar) ar_free(ctx->ar);
  ctx->ar = st.release();
  if (timing) fprintf(stderr, "[tts timing] AR load: file %.1f ms, %d layers %.1f, total %.1f\n", t_read, ctx->ar->n_layers, t_layers, since(t0));
  return TTS_OK;
}

// ---- launch helpers -----------------------------------------------------------------------------
static int pick_rt(int rows) { int rt = 1; while (rt < rows && rt < 16) rt <<= 1; return rt; }

// part <- X[rows][K] * W[K][N]; returns ks through *ks_out. pin_ks > 0: X is a partial buffer (see PRO).
static int launch_gemv(tts_ctx *ctx, ArState *st, const float *X, int ldx, int rows, const float *W, int N, int K,
                       int *ks_out, float *part = nullptr, int pin_ks = 0, const float *pin_bias = nullptr) {
  const int rt = pick_rt(rows);
  const int ztiles = (rows + rt - 1) / rt, strips = N / 64;
  int ks = 1;
  while (ks * 2 * strips * ztiles <= 768 && K / (ks * 2) >= 32) ks *= 2;
  const int kchunk = K / ks; // K range per block (staged through LDS in chunks of <= 256)
  if (!part) {
    TTS_HIP(ctx, st->part.reserve((size_t)ks * rows * N * sizeof(float)));
    part = st->part.as<float>();
  }
  dim3 grid(strips, ks, ztiles);
  ProfScope ps(ctx, "ar_gemv", (double)K * N * 4.0 * ztiles); // weight bytes streamed
#define GEMV_LAUNCH(RT_)                                                                                                   \
  if (pin_ks > 0) gemv_kn_kernel<RT_, 1><<<grid, 256, 0, ctx->stream>>>(X, ldx, rows, W, N, K, kchunk, part, pin_ks, pin_bias, ctx->ggml_lut); \
  else gemv_kn_kernel<RT_, 0><<<grid, 256, 0, ctx->stream>>>(X, ldx, rows, W, N, K, kchunk, part, 0, nullptr, 0)
  switch (rt) {
    case 1: GEMV_LAUNCH(1); break;
    case 2: GEMV_LAUNCH(2); break;
    case 4: GEMV_LAUNCH(4); break;
    case 8: GEMV_LAUNCH(8); break;
    default: GEMV_LAUNCH(16); break;
  }
#undef GEMV_LAUNCH
  TTS_HIP(ctx, hipGetLastError());
  *ks_out = ks;
  return TTS_OK;
}

template <int MODE>
static int launch_epilogue(tts_ctx *ctx, ArState *st, int ks, int rows, int N, int n_valid, const float *bias, float *out,
                           int ldo, KvDst kv, float pscale = 1.0f) {
  ProfScope ps(ctx, "ar_epilogue");
  epilogue_kernel<MODE><<<dim3(rows, (n_valid + 255) / 256), 256, 0, ctx->stream>>>(st->part.as<float>(), ks, rows, N, n_valid, bias,
                                                                                    out, ldo, kv, ctx->ggml_lut, pscale);
  TTS_HIP(ctx, hipGetLastError());
  return TTS_OK;
}


// part[rows][N] (scaled by 64) <- split-precision MFMA product of X[rows][K] with the layer's hi|lo weights.
static int launch_mfma_matmul(tts_ctx *ctx, ArState *st, const float *X, int rows, const __half *Wsplit, int N, int K) {
  const int rpad = (rows + 127) & ~127;
  TTS_HIP(ctx, st->a_hi.reserve((size_t)rpad * FF * sizeof(__half)));
  TTS_HIP(ctx, st->a_lo.reserve((size_t)rpad * FF * sizeof(__half)));
  TTS_HIP(ctx, st->part.reserve((size_t)rpad * N * sizeof(float)));
  split_act_kernel<<<rpad, 256, 0, ctx->stream>>>(X, rows, K, st->a_hi.as<__half>(), st->a_lo.as<__half>());
  GemmArgs g{};
  g.A[0] = st->a_hi.as<__half>(); g.A[1] = st->a_lo.as<__half>(); g.A[2] = st->a_hi.as<__half>();
  g.row_off[0] = g.row_off[1] = g.row_off[2] = 0;
  g.nseg = 3; g.kseg = K; g.lda = K; g.W = Wsplit;
  g.custom_w = 1; g.ldw_ = 2 * K; g.w_off_[0] = 0; g.w_off_[1] = 0; g.w_off_[2] = K; // hi*hi + lo*hi + hi*lo
  g.M = rpad; g.N = N; g.bias = nullptr; g.row_seq = nullptr;
  g.mode = GEMM_OUT_F32; g.outF = st->part.as<float>(); g.ldo = N; g.resid = nullptr;
  ProfScope ps(ctx, "ar_mfma_gemm", 2.0 * rows * (double)N * K);
  TTS_HIP(ctx, launch_gemm_f16(g, ctx->stream));
  return TTS_OK;
}

#define CHECK(x) do { int _r = (x); if (_r) return _r; } while (0)
#define DEC_LN_LAUNCH(EPI_, GRID_, HT_)                                                            \
  do {                                                                                             \
    if (st->f32_mfma) dec_ln_gemv_kernel<EPI_, 0, false, HT_><<<GRID_, 256, 0, ctx->stream>>>(a);   \
    else dec_ln_gemv_kernel<EPI_, 1, true, HT_><<<GRID_, 256, 0, ctx->stream>>>(a);                 \
  } while (0)


// Transformer stack over rows = n_cand_rows * S laid out [cand][pos] in st->h.
//   kc/vc: fp16 K/V destination [cand][kv_max_pos][1024] per layer (layer_stride halves apart).
static int run_layers(tts_ctx *ctx, ArState *st, int rows, int S, int n_past, __half *kc, __half *vc,
                      size_t layer_stride, int kv_max_pos, int replicate) {
  float *h = st->h.as<float>(), *xn = st->xn.as<float>(), *qkv = st->qkv.as<float>();
  float *att = st->att.as<float>(), *ff = st->ff.as<float>();
  KvDst nokv{nullptr, nullptr, 1, 0, 0, 0};
  const bool mfma = rows >= 32; // multi-row passes: split-precision MFMA GEMM; tiny row counts: exact f32 GEMV
  const float ps = mfma ? 1.0f / W16_SCALE : 1.0f;
  for (int l = 0; l < st->n_layers; l++) {
    const ArLayerDev &w = st->L[l];
    int ks = 1;
    { ProfScope ps(ctx, "ar_layernorm");
      layernorm_kernel<<<rows, 256, 0, ctx->stream>>>(h, w.ln1_g, w.ln1_b, xn); }
    if (mfma) CHECK(launch_mfma_matmul(ctx, st, xn, rows, w.s_attn, 3 * D, D));
    else CHECK(launch_gemv(ctx, st, xn, D, rows, w.w_attn, 3 * D, D, &ks));
    KvDst kv{kc + l * layer_stride, vc + l * layer_stride, S, n_past, kv_max_pos, replicate};
    CHECK(launch_epilogue<EPI_QKV>(ctx, st, ks, rows, 3 * D, 3 * D, w.b_attn, qkv, 3 * D, kv, ps));
    { ProfScope ps(ctx, "ar_attention");
      if (ctx->ggml_lut) attention_kernel<<<dim3(rows, NH), 64, 0, ctx->stream>>>(qkv, kv.k, kv.v, att, S, n_past, kv_max_pos, 1);
      else attention_rows_kernel<<<dim3(rows / S, NH, (S + 63) / 64), 256, 0, ctx->stream>>>(qkv, kv.k, kv.v, att, S, n_past, kv_max_pos); }
    if (mfma) CHECK(launch_mfma_matmul(ctx, st, att, rows, w.s_proj, D, D));
    else CHECK(launch_gemv(ctx, st, att, D, rows, w.w_proj, D, D, &ks));
    CHECK(launch_epilogue<EPI_RESID>(ctx, st, ks, rows, D, D, w.b_proj, h, D, nokv, ps));
    { ProfScope ps(ctx, "ar_layernorm");
      layernorm_kernel<<<rows, 256, 0, ctx->stream>>>(h, w.ln2_g, w.ln2_b, xn); }
    if (mfma) CHECK(launch_mfma_matmul(ctx, st, xn, rows, w.s_fc, FF, D));
    else CHECK(launch_gemv(ctx, st, xn, D, rows, w.w_fc, FF, D, &ks));
    CHECK(launch_epilogue<EPI_GELU>(ctx, st, ks, rows, FF, FF, w.b_fc, ff, FF, nokv, ps));
    if (mfma) CHECK(launch_mfma_matmul(ctx, st, ff, rows, w.s_fc2, D, FF));
    else CHECK(launch_gemv(ctx, st, ff, FF, rows, w.w_fc2, D, FF, &ks));
    CHECK(launch_epilogue<EPI_RESID>(ctx, st, ks, rows, D, D, w.b_fc2, h, D, nokv, ps));
  }
  TTS_HIP(ctx, hipGetLastError());
  return TTS_OK;
}

static int reserve_rows(tts_ctx *ctx, ArState *st, int rows) {
  TTS_HIP(ctx, st->h.reserve((size_t)rows * D * 4));
  TTS_HIP(ctx, st->xn.reserve((size_t)rows * D * 4));
  TTS_HIP(ctx, st->hn.reserve((size_t)rows * D * 4));
  TTS_HIP(ctx, st->qkv.reserve((size_t)rows * 3 * D * 4));
  TTS_HIP(ctx, st->att.reserve((size_t)rows * D * 4));
  TTS_HIP(ctx, st->ff.reserve((size_t)rows * FF * 4));
  TTS_HIP(ctx, st->desc.reserve((size_t)rows * sizeof(int4)));
  return TTS_OK;
}

// The step's pinned host buffers for B rows. h_toks holds the larger of the two host blocks: [tokens[B] | n_past, pos_id] and a session's
// [tokens[B] | n_past[Bpad] | pos_id[B]].
static int reserve_pinned(tts_ctx *ctx, ArState *st, int B) {
  if (B <= st->h_cap_B) return TTS_OK; // pinned allocations are slow (milliseconds): keep them across utterances
  if (st->h_toks) (void)hipHostFree(st->h_toks);
  if (st->h_logits) (void)hipHostFree(st->h_logits);
  if (st->h_pf) (void)hipHostFree(st->h_pf);
  st->h_toks = nullptr; st->h_logits = nullptr; st->h_pf = nullptr; st->h_cap_B = 0;
  TTS_HIP(ctx, hipHostMalloc((void **)&st->h_toks, ((size_t)3 * B + 16) * 4));
  TTS_HIP(ctx, hipHostMalloc((void **)&st->h_logits, (size_t)B * V * 4));
  TTS_HIP(ctx, hipHostMalloc((void **)&st->h_pf, (size_t)B * TTS_PF_WORDS * 4));
  st->h_cap_B = B;
  return TTS_OK;
}

static int embed(tts_ctx *ctx, ArState *st, const std::vector<int4> &desc) {
  TTS_HIP(ctx, hipMemcpyAsync(st->desc.p, desc.data(), desc.size() * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
  EmbedTables t{{st->voice.as<float>(), st->text_emb, st->mel_emb}, {st->text_pos, st->mel_pos}};
  embed_rows_kernel<<<(int)desc.size(), 256, 0, ctx->stream>>>(t, st->desc.as<int4>(), st->h.as<float>());
  TTS_HIP(ctx, hipGetLastError());
  return TTS_OK;
}

// tts_ar_begin (one prompt, G = 1) and tts_ar_begin_multi (G prompts back to back in text_ids, group g with n_text[g] ids and n_cand[g] candidates).
// tts_ar_begin_multi_voice: `voice` is a table [n_voices][1024] and group g reads row voice_of[g] (voice_of == nullptr: row 0 for every group — the
// single-voice entry points, n_voices = 1). Every argument is checked before anything changes.
int ar_begin_groups(tts_ctx *ctx, const int32_t *text_ids, const int *n_text, int G, const float *voice, int n_voices, const int *voice_of, const int *n_cand,
                    int max_steps) {
  ArState *st = ctx->ar;
  if (!st) return fail(ctx, TTS_ERR_STATE, "AR model not loaded");
  if (G < 1 || !n_text || !n_cand || max_steps < 1 || !text_ids || !voice) return fail(ctx, TTS_ERR_ARG, "tts_ar_begin: bad argument");
  if (n_voices < 1 || n_voices > (1 << 20)) return fail(ctx, TTS_ERR_ARG, "tts_ar_begin: %d voices", n_voices);
  if (voice_of) {
    for (int g = 0; g < G; g++)
      if (voice_of[g] < 0 || voice_of[g] >= n_voices) return fail(ctx, TTS_ERR_ARG, "tts_ar_begin: prompt %d names voice %d of %d", g, voice_of[g], n_voices);
    for (size_t i = 0; i < (size_t)n_voices * D; i++)
      if (!std::isfinite(voice[i])) return fail(ctx, TTS_ERR_ARG, "tts_ar_begin: voice %d holds a non-finite value", (int)(i / D));
  }
  int B = 0, P_max = 0, T = 0;
  for (int g = 0; g < G; g++) {
    if (n_text[g] < 1 || n_cand[g] < 1) return fail(ctx, TTS_ERR_ARG, "tts_ar_begin: bad argument (prompt %d: %d ids, %d candidates)", g, n_text[g], n_cand[g]);
    if (n_text[g] > 404) return fail(ctx, TTS_ERR_LIMIT, "text has %d ids; the model has 404 text positions", n_text[g]);
    if (n_cand[g] > (1 << 24) - B) return fail(ctx, TTS_ERR_LIMIT, "more than 2^24 candidates");
    B += n_cand[g]; T += n_text[g];
    P_max = std::max(P_max, n_text[g] + 2);
  }
  if (max_steps + 2 > 608) return fail(ctx, TTS_ERR_LIMIT, "max_steps %d exceeds the 608 mel positions", max_steps);
  for (int i = 0; i < T; i++)
    if (text_ids[i] < 0 || text_ids[i] >= 256) return fail(ctx, TTS_ERR_ARG, "text id %d out of range", text_ids[i]);
  const int max_pos = P_max + max_steps + 1;
  if (max_pos > 1024) return fail(ctx, TTS_ERR_LIMIT, "context of %d positions exceeds 1024", max_pos);
  st->B = 0; // (a failure below leaves no half-begun state behind)
  st->g_c0.assign(G, 0); st->g_n.assign(n_cand, n_cand + G); st->g_t0.assign(G, 0); st->g_ntext.assign(n_text, n_text + G);
  st->g_voice.assign(G, 0);
  if (voice_of) st->g_voice.assign(voice_of, voice_of + G);
  for (int g = 1; g < G; g++) { st->g_c0[g] = st->g_c0[g - 1] + n_cand[g - 1]; st->g_t0[g] = st->g_t0[g - 1] + n_text[g - 1]; }
  st->multi = G > 1;
  st->session = false;
  st->n_text = P_max - 2; st->P = P_max;
  st->prefill_done = false;
  st->max_pos = max_pos;
  st->tokens.assign(text_ids, text_ids + T);
  TTS_HIP(ctx, st->voice.reserve((size_t)n_voices * D * 4));
  TTS_HIP(ctx, hipMemcpy(st->voice.p, voice, (size_t)n_voices * D * 4, hipMemcpyHostToDevice));
  size_t cache = (size_t)st->n_layers * B * st->max_pos * D * sizeof(__half);
  TTS_HIP(ctx, st->kcache.reserve(cache));
  TTS_HIP(ctx, st->vcache.reserve(cache));
  TTS_HIP(ctx, st->d_toks.reserve((size_t)(B + 2) * 4)); // [tokens | n_past, pos_id]
  TTS_HIP(ctx, st->logits.reserve((size_t)B * V * 4));
  if (st->multi) { // every row's context offset, once per begin (outside the graph: the step state's n_past becomes the step index)
    std::vector<int> off((size_t)(B + 15) / 16 * 16, 0);
    for (int g = 0; g < G; g++)
      for (int c = 0; c < n_cand[g]; c++) off[(size_t)st->g_c0[g] + c] = n_text[g] + 2;
    TTS_HIP(ctx, st->row_off.reserve(off.size() * sizeof(int)));
    TTS_HIP(ctx, hipMemcpy(st->row_off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  CHECK(reserve_pinned(ctx, st, B));
  st->hist_host.assign((size_t)B * TTS_HIST_WORDS, 0u); // a fresh history per begin: ids 1 and 8192 (what the prompt-shaped row of step 0 penalises)
  for (int b = 0; b < B; b++) {
    uint32_t *hb = st->hist_host.data() + (size_t)b * TTS_HIST_WORDS;
    hb[1 >> 5] |= 1u << (1 & 31);
    hb[8192 >> 5] |= 1u << (8192 & 31);
  }
  st->hist_dev_valid = false;
  // the decode-step graph is kept: ar_step re-captures it only if a buffer moved or the batch shape changed (GraphSig)
  // the decode step's h4 layout holds whole tiles of 16 candidates: the padding rows of the last tile are read (never stored), keep them finite
  CHECK(reserve_rows(ctx, st, std::max((B + 15) / 16 * 16, st->P)));
  TTS_HIP(ctx, hipMemsetAsync(st->h.p, 0, st->h.cap, ctx->stream));
  st->B = B;
  return TTS_OK;
}

int ar_begin(tts_ctx *ctx, const int32_t *text_ids, int n_text, const float *voice, int B, int max_steps) {
  return ar_begin_groups(ctx, text_ids, &n_text, 1, voice, 1, nullptr, &B, max_steps);
}

// Prefill (main.cpp:2586-2665): [voice | text_emb+pos | mel_emb(8192)+mel_pos(0)] — identical for all
// candidates, so it is evaluated once and its K/V rows are written into every candidate's cache.
// Several prompts (tts_ar_begin_multi): one such pass per group, its K/V rows written into the caches of the group's candidates only.
// A session's request (tts_ar_session_admit): the same pass over its slot range [c0, c0 + n_cand).
static int prompt_pass(tts_ctx *ctx, ArState *st, int c0, int n_cand, int n_text, const int *tok, int voice_row) {
  const int P = n_text + 2;
  std::vector<int4> desc(P);
  desc[0] = make_int4(0, voice_row, -1, 0); // the group's row of the voice table
  for (int i = 0; i < n_text; i++) desc[1 + i] = make_int4(1, tok[i], 0, i);
  desc[P - 1] = make_int4(2, 8192, 1, 0);
  CHECK(embed(ctx, st, desc));
  const size_t layer_stride = (size_t)st->B * st->max_pos * D, cand0 = (size_t)c0 * st->max_pos * D;
  // The prompt pass runs on the decode-step kernels, tiled over 16 positions (exact f32, weights re-read from L2 per
  // tile): rows are positions of the one shared prompt, the QKV epilogue replicates K/V into every candidate's cache.
  const int tiles = (P + 15) / 16;
  float *h = st->h.as<float>(), *qkv = st->qkv.as<float>(), *att = st->att.as<float>(), *ff = st->ff.as<float>();
  for (int l = 0; l < st->n_layers; l++) {
    const ArLayerDev &w = st->L[l];
    __half *kc = st->kcache.as<__half>() + l * layer_stride + cand0, *vc = st->vcache.as<__half>() + l * layer_stride + cand0;
    { ProfScope ps(ctx, "ar_gemv", 3.0 * D * D * 4.0 * tiles);
      DecLnArgs a{h, nullptr, nullptr, w.d_attn, w.dh_attn, w.db_attn, P, 3 * D, 3 * D, n_cand, qkv, kc, vc, nullptr, st->max_pos, ctx->ggml_lut};
      DEC_LN_LAUNCH(DEC_QKV, dim3(3 * D / 16, tiles), false); }
    { ProfScope ps(ctx, "ar_attention");
      attention_kernel<<<dim3(P, NH), 64, 0, ctx->stream>>>(qkv, kc, vc, att, P, 0, st->max_pos, ctx->ggml_lut); }
    { ProfScope ps(ctx, "ar_gemv", 1.0 * D * D * 4.0 * tiles);
      dec_gemv_resid_kernel<1><<<dim3(D / 4, tiles), 256, 0, ctx->stream>>>(att, P, w.d_proj, w.b_proj, h); }
    { ProfScope ps(ctx, "ar_gemv", 4.0 * D * D * 4.0 * tiles);
      DecLnArgs a{h, nullptr, nullptr, w.d_fc, w.dh_fc, w.db_fc, P, FF, 0, 0, ff, nullptr, nullptr, nullptr, 0, ctx->ggml_lut};
      DEC_LN_LAUNCH(DEC_GELU, dim3(FF / 16, tiles), false); }
    { ProfScope ps(ctx, "ar_gemv", 4.0 * D * D * 4.0 * tiles);
      dec_gemv_resid_kernel<4, 512><<<dim3(D / 4, tiles), 512, 0, ctx->stream>>>(ff, P, w.d_fc2, w.b_fc2, h); }
  }
  // the group's logits go to the row of its first candidate
  { ProfScope ps(ctx, "ar_gemv", (double)D * VPAD * 4.0);
    DecLnArgs a{h + (size_t)(P - 1) * D, st->lnf_g, st->lnf_b, st->d_lm, st->dh_lm, st->d_lmb, 1, V, V, 0, st->logits.as<float>() + (size_t)c0 * V,
                nullptr, nullptr, nullptr, 0, ctx->ggml_lut};
    DEC_LN_LAUNCH(DEC_LOGITS, dim3(VPAD / 16, 1), false); }
  TTS_HIP(ctx, hipGetLastError());
  return TTS_OK;
}

static int prefill_group(tts_ctx *ctx, ArState *st, int g) {
  return prompt_pass(ctx, st, st->g_c0[g], st->g_n[g], st->g_ntext[g], st->tokens.data() + st->g_t0[g], st->g_voice[g]);
}

int ar_prefill(tts_ctx *ctx, float *logits_out) {
  ArState *st = ctx->ar;
  if (!st || st->B == 0) return fail(ctx, TTS_ERR_STATE, "tts_ar_begin not called");
  TTS_HIP(ctx, st->logits.reserve((size_t)st->B * V * 4));
  const int G = (int)st->g_n.size();
  for (int g = 0; g < G; g++) CHECK(prefill_group(ctx, st, g));
  if (logits_out) {
    for (int g = 0; g < G; g++)
      TTS_HIP(ctx, hipMemcpyAsync(logits_out + (size_t)st->g_c0[g] * V, st->logits.as<float>() + (size_t)st->g_c0[g] * V, (size_t)V * 4, hipMemcpyDeviceToHost,
                                  ctx->stream));
    TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int g = 0; g < G; g++)
      for (int c = 1; c < st->g_n[g]; c++) memcpy(logits_out + (size_t)(st->g_c0[g] + c) * V, logits_out + (size_t)st->g_c0[g] * V, (size_t)V * 4);
  } else {
    TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  st->prefill_done = true;
  return TTS_OK;
}

// The decode step's LN1 + QKV launch. RO: several prompts, every row stores its K/V at its own position (a.row_off).
template <bool RO>
static void launch_dec_qkv(tts_ctx *ctx, const ArState *st, int wm, dim3 grid, const DecLnArgs &a) {
  if (wm == 2) dec_ln_gemv_kernel<DEC_QKV, 3, true, true, RO><<<grid, 256, 0, ctx->stream>>>(a);
  else if (wm == 1) dec_ln_gemv_kernel<DEC_QKV, 2, false, true, RO><<<grid, 256, 0, ctx->stream>>>(a);
  else if (st->f32_mfma) dec_ln_gemv_kernel<DEC_QKV, 0, false, true, RO><<<grid, 256, 0, ctx->stream>>>(a);
  else dec_ln_gemv_kernel<DEC_QKV, 1, true, true, RO><<<grid, 256, 0, ctx->stream>>>(a);
}

// One decode step for all candidates, enqueued on the ctx stream (captured once into a hipGraph): five
// launches per layer (see the kernels above) + embed + head; every launch streams its weights exactly once
// per tile of 16 candidates.
static int enqueue_decode_step(tts_ctx *ctx, ArState *st) {
  const int B = st->B, tiles = (B + 15) / 16;
  float *h = st->h.as<float>() /* h4 layout inside the step */, *q = st->qkv.as<float>(), *att = st->att.as<float>(), *ff = st->ff.as<float>();
  const StepState *ss = (const StepState *)(st->d_toks.as<int>() + B);
  const size_t layer_stride = (size_t)B * st->max_pos * D;
  const int wm = ctx->ar_weights; // 1 / 2: fp16 / fp8 weights, a half / a quarter of the bytes per step (throughput modes, not f32-exact); checked by ar_step
  const double wb = wm == 2 ? 1.0 : wm == 1 ? 2.0 : 4.0;
  const bool ro_k = st->multi || st->session; // several prompts: the rows' context offsets (n_past = step index + row_off[row]); a session: the rows' context lengths
  const int *ro = ro_k ? st->row_off.as<int>() : nullptr;
  if (st->session)
    embed_session_kernel<<<B, 256, 0, ctx->stream>>>(st->mel_emb, st->mel_pos, st->h_toks, B, tiles * 16, (StepState *)(st->d_toks.as<int>() + B), st->row_off.as<int>(), h);
  else
    embed_step_kernel<<<B, 256, 0, ctx->stream>>>(st->mel_emb, st->mel_pos, st->h_toks, B, (StepState *)(st->d_toks.as<int>() + B), h);
  for (int l = 0; l < st->n_layers; l++) {
    const ArLayerDev &w = st->L[l];
    __half *kc = st->kcache.as<__half>() + l * layer_stride, *vc = st->vcache.as<__half>() + l * layer_stride;
    { ProfScope ps(ctx, "ar_gemv", 3.0 * D * D * wb * tiles);
      DecLnArgs a{h, nullptr, nullptr, w.d_attn, wm == 2 ? (const __half *)w.o_attn : wm == 1 ? w.q_attn : w.dh_attn, w.db_attn, B, 3 * D, D, 0, q, kc, vc, ss,
                  st->max_pos, ctx->ggml_lut, w.os_attn, ro};
      if (ro_k) launch_dec_qkv<true>(ctx, st, wm, dim3(3 * D / 16, tiles), a);
      else launch_dec_qkv<false>(ctx, st, wm, dim3(3 * D / 16, tiles), a); }
    { ProfScope ps(ctx, "ar_attention");
      if (ctx->ggml_lut) {
        if (ro_k) attn_decode_kernel<true><<<dim3(B, NH), 256, 0, ctx->stream>>>(q, kc, vc, ss, st->max_pos, att, 1, ro);
        else attn_decode_kernel<false><<<dim3(B, NH), 256, 0, ctx->stream>>>(q, kc, vc, ss, st->max_pos, att, 1, nullptr);
      } else {
        if (ro_k) attn_decode_fast_kernel<true><<<dim3(B, NH), 256, 0, ctx->stream>>>(q, kc, vc, ss, st->max_pos, att, ro);
        else attn_decode_fast_kernel<false><<<dim3(B, NH), 256, 0, ctx->stream>>>(q, kc, vc, ss, st->max_pos, att, nullptr);
      } }
    { ProfScope ps(ctx, "ar_gemv", 1.0 * D * D * wb * tiles);
      if (wm == 2) dec_gemv_resid_kernel<1, 256, 2, false, true><<<dim3(D / 4, tiles), 256, 0, ctx->stream>>>(att, B, (const float *)w.o_proj, w.b_proj, h, w.os_proj);
      else if (wm == 1) dec_gemv_resid_kernel<1, 256, 1, false, true><<<dim3(D / 4, tiles), 256, 0, ctx->stream>>>(att, B, (const float *)w.q_proj, w.b_proj, h);
      else dec_gemv_resid_kernel<1, 256, 0, true, true><<<dim3(D / 4, tiles), 256, 0, ctx->stream>>>(att, B, w.d_proj, w.b_proj, h); }
    { ProfScope ps(ctx, "ar_gemv", 4.0 * D * D * wb * tiles);
      DecLnArgs a{h, nullptr, nullptr, w.d_fc, wm == 2 ? (const __half *)w.o_fc : wm == 1 ? w.q_fc : w.dh_fc, w.db_fc, B, FF, 0, 0, ff, nullptr, nullptr, ss, 0,
                  ctx->ggml_lut, w.os_fc};
      if (wm == 2) dec_ln_gemv_kernel<DEC_GELU, 3, true, true><<<dim3(FF / 16, tiles), 256, 0, ctx->stream>>>(a);
      else if (wm == 1) dec_ln_gemv_kernel<DEC_GELU, 2, false, true><<<dim3(FF / 16, tiles), 256, 0, ctx->stream>>>(a);
      else DEC_LN_LAUNCH(DEC_GELU, dim3(FF / 16, tiles), true); }
    { ProfScope ps(ctx, "ar_gemv", 4.0 * D * D * wb * tiles);
      if (wm == 2) dec_gemv_resid_kernel<4, 512, 2, false, true><<<dim3(D / 4, tiles), 512, 0, ctx->stream>>>(ff, B, (const float *)w.o_fc2, w.b_fc2, h, w.os_fc2);
      else if (wm == 1) dec_gemv_resid_kernel<4, 512, 1, false, true><<<dim3(D / 4, tiles), 512, 0, ctx->stream>>>(ff, B, (const float *)w.q_fc2, w.b_fc2, h);
      else dec_gemv_resid_kernel<4, 512, 0, true, true><<<dim3(D / 4, tiles), 512, 0, ctx->stream>>>(ff, B, w.d_fc2, w.b_fc2, h); }
  }
  { ProfScope ps(ctx, "ar_gemv", (double)D * VPAD * wb * tiles);
    DecLnArgs a{h, st->lnf_g, st->lnf_b, st->d_lm, wm == 2 ? (const __half *)st->o_lm : wm == 1 ? st->q_lm : st->dh_lm, st->d_lmb, B, V, V, 0, st->logits.as<float>(),
                nullptr, nullptr, ss, 0, ctx->ggml_lut, st->os_lm};
    if (wm == 2) dec_ln_gemv_kernel<DEC_LOGITS, 3, true, true><<<dim3(VPAD / 16, tiles), 256, 0, ctx->stream>>>(a);
    else if (wm == 1) dec_ln_gemv_kernel<DEC_LOGITS, 2, false, true><<<dim3(VPAD / 16, tiles), 256, 0, ctx->stream>>>(a);
    else DEC_LN_LAUNCH(DEC_LOGITS, dim3(VPAD / 16, tiles), true); }
  const bool rows = st->session && st->rows; // per-row controls: the history sets are kept for every row, the prefilter reads the control table
  if (st->step_mode == 0) {
    if (st->step_scope || rows) hist_mark_kernel<<<(B + 255) / 256, 256, 0, ctx->stream>>>(st->h_toks, B, st->hist.as<uint32_t>()); // the one node scope 1 adds
    TTS_HIP(ctx, hipMemcpyAsync(st->h_logits, st->logits.p, (size_t)B * V * 4, hipMemcpyDeviceToHost, ctx->stream));
  } else { // the sampler's top-k prefilter on the device: 16 KB instead of 524 KB back to the host per step of 16 candidates
    ProfScope ps(ctx, "ar_prefilter", (double)B * V * 4.0);
    // the lists are written straight into pinned host memory (1 KB per candidate over PCIe from the kernel's stores): no copy node behind the graph
    if (rows)
      sample_prefilter_rows_kernel<<<B, 256, 0, ctx->stream>>>(st->logits.as<float>(), st->step_mode == 2, st->ctl.as<int4>(), st->h_pf, st->hist.as<uint32_t>(),
                                                               st->h_toks);
    else if (st->step_mass > 0.f && st->step_scope)
      sample_prefilter_typical_kernel<true><<<B, 256, 0, ctx->stream>>>(st->logits.as<float>(), st->step_mode == 2, st->step_pf_min, st->h_pf, st->hist.as<uint32_t>(),
                                                                         st->h_toks, st->step_penalty, st->step_mass);
    else if (st->step_mass > 0.f)
      sample_prefilter_typical_kernel<false><<<B, 256, 0, ctx->stream>>>(st->logits.as<float>(), st->step_mode == 2, st->step_pf_min, st->h_pf, nullptr, st->h_toks,
                                                                          st->step_penalty, st->step_mass);
    else if (st->step_scope)
      sample_prefilter_kernel<true><<<B, 256, 0, ctx->stream>>>(st->logits.as<float>(), st->step_mode == 2, st->step_pf_min, st->h_pf, st->hist.as<uint32_t>(),
                                                                 st->h_toks, st->step_penalty);
    else
      sample_prefilter_kernel<false><<<B, 256, 0, ctx->stream>>>(st->logits.as<float>(), st->step_mode == 2, st->step_pf_min, st->h_pf, nullptr, nullptr, 1.0f);
  }
  TTS_HIP(ctx, hipGetLastError());
  return TTS_OK;
}

// Runs the step that the state describes: replays graph slot `slot` (captured first when the slot is empty or anything its nodes bake in has moved: GraphSig),
// or launches the kernels eagerly while one of their families is profiled. Slots 0 .. 2: ar_step's modes; 3: the session step; 4: the step of a session with
// per-row controls.
static int launch_step(tts_ctx *ctx, ArState *st, int slot, double step_bytes) {
  static const bool no_graph = getenv("TTS_NO_GRAPH") != nullptr; // e.g. under rocprofv3, which crashes on graph replays here
  // event records are not captured: the step runs eagerly while one of its own kernel families ("ar_*") is profiled
  // ("ar_decode_step" brackets the whole graph replay and keeps the graph)
  bool prof_ar = ctx->prof_on && ctx->prof_filter.empty();
  for (const std::string &f : ctx->prof_filter) prof_ar |= ctx->prof_on && f.rfind("ar_", 0) == 0 && f != "ar_decode_step";
  if (prof_ar || no_graph) return enqueue_decode_step(ctx, st);
  const ArState::GraphSig sig = st->current_sig(ctx->ggml_lut, ctx->ar_weights);
  if (st->graph_execs[slot] && !(sig == st->graph_sigs[slot])) st->drop_graph(slot);
  if (!st->graph_execs[slot]) {
    st->graph_sigs[slot] = sig;
    TTS_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    st->graph_captures++;
    int rc = enqueue_decode_step(ctx, st);
    hipError_t e = hipStreamEndCapture(ctx->stream, &st->graphs[slot]);
    if (rc || e != hipSuccess) { st->drop_graph(slot); if (rc) return rc; TTS_HIP(ctx, e); } // never keep a half-captured graph
    e = hipGraphInstantiate(&st->graph_execs[slot], st->graphs[slot], nullptr, nullptr, 0);
    if (e != hipSuccess) { st->drop_graph(slot); TTS_HIP(ctx, e); }
  }
  ProfScope ps(ctx, "ar_decode_step", step_bytes);
  TTS_HIP(ctx, hipGraphLaunch(st->graph_execs[slot], ctx->stream));
  return TTS_OK;
}

// Decode step i (main.cpp:2667-2693, 5227-5247): mel_emb[tok] + mel_pos[i+2], n_past = P + i.
// mode 0: the logits come back ([B][8194], logits_out may be null: ar_host_logits); mode 1 / 2: the device prefilter's lists come back
// instead (ar_host_lists; 2 = stop token masked first) and the logits stay in HBM (ar_fetch_logits_row). Each mode is its own graph.
int ar_step(tts_ctx *ctx, const int32_t *prev_ids, int step_i, float *logits_out, int mode) {
  ArState *st = ctx->ar;
  if (!st || st->B == 0) return fail(ctx, TTS_ERR_STATE, "tts_ar_begin not called");
  if (mode < 0 || mode > 2 || (mode && logits_out)) return fail(ctx, TTS_ERR_ARG, "ar_step: bad mode");
  st->step_mode = mode;
  if (step_i < 0 || st->P + step_i >= st->max_pos) return fail(ctx, TTS_ERR_LIMIT, "step %d beyond the KV cache", step_i); // (P: the longest prompt's)
  for (int c = 0; c < st->B; c++)
    if (prev_ids[c] < 0 || prev_ids[c] >= V) return fail(ctx, TTS_ERR_ARG, "mel token %d out of range", prev_ids[c]);
  // checked here, not inside enqueue_decode_step: that runs between hipStreamBeginCapture and hipStreamEndCapture
  if (ctx->ar_weights != 0 && ctx->ar_weights != st->loaded_wmode)
    return fail(ctx, TTS_ERR_STATE, "option ar_weights = %d must be set before tts_load_ar (the fp16 / fp8 slabs are packed at load)", ctx->ar_weights);
  // the sampler controls this step bakes into its nodes (GraphSig), and the history sets of penalty scope 1
  st->step_scope = ctx->ar_penalty_scope;
  st->step_pf_min = pf_min_for(ctx->ar_sp.top_k);
  st->step_penalty = ctx->ar_sp.penalty;
  st->step_mass = ctx->ar_sp.typ_mass;
  if (st->step_scope && !st->hist_dev_valid) { // before this step's ids join the host copy: the step's own kernel adds them on the device
    TTS_HIP(ctx, st->hist.reserve(st->hist_host.size() * 4));
    TTS_HIP(ctx, hipMemcpy(st->hist.p, st->hist_host.data(), st->hist_host.size() * 4, hipMemcpyHostToDevice));
  }
  st->hist_dev_valid = st->step_scope != 0;
  for (int c = 0; c < st->B; c++) {
    st->h_toks[c] = prev_ids[c];
    st->hist_host[(size_t)c * TTS_HIST_WORDS + (prev_ids[c] >> 5)] |= 1u << (prev_ids[c] & 31);
  }
  st->h_toks[st->B] = st->multi ? step_i : st->P + step_i; // n_past (several prompts: the kernels add the row's P, ArState::row_off)
  st->h_toks[st->B + 1] = step_i + 2; // mel position id (main.cpp:5244)
  // HBM-bound step: every weight once (f32: 12 d^2 per layer + the padded head) + the fp16 K/V rows read + logits
  const double step_bytes = (ctx->ar_weights == 2 ? 1.0 : ctx->ar_weights == 1 ? 2.0 : 4.0) * ((double)st->n_layers * 12.0 * D * D + (double)D * V) +
                            (double)st->B * st->n_layers * 2.0 * (st->P + step_i + 1) * D * 2.0 + (double)st->B * V * 4.0;
  CHECK(launch_step(ctx, st, mode, step_bytes));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (logits_out) memcpy(logits_out, st->h_logits, (size_t)st->B * V * 4);
  return TTS_OK;
}

// Candidate c's history set as ascending ids (penalty scope 1: what the full-row sampler penalises; the host copy of the bitmap the device kernel reads).
void ar_history_ids(const tts_ctx *ctx, int c, std::vector<int32_t> &out) {
  out.clear();
  const ArState *st = ctx->ar;
  if (!st || c < 0 || c >= st->B) return;
  const uint32_t *hb = st->hist_host.data() + (size_t)c * TTS_HIST_WORDS;
  for (int w = 0; w < TTS_HIST_WORDS; w++)
    for (uint32_t m = hb[w]; m; m &= m - 1) out.push_back(w * 32 + __builtin_ctz(m));
}

// The pinned lists of the last mode 1 / 2 step ([B][TTS_PF_WORDS]).
const int32_t *ar_host_lists(tts_ctx *ctx) { return ctx->ar ? ctx->ar->h_pf : nullptr; }

// One candidate's logits of the last step, from HBM (the sampler's fallback when a list cannot decide). Returns the pinned row or null.
const float *ar_fetch_logits_row(tts_ctx *ctx, int c) {
  ArState *st = ctx->ar;
  if (!st || c < 0 || c >= st->B) return nullptr;
  float *dst = st->h_logits + (size_t)c * V;
  if (hipMemcpyAsync(dst, st->logits.as<float>() + (size_t)c * V, (size_t)V * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return nullptr;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return nullptr;
  if (st->step_mode == 2) dst[V - 1] = -1e30f;
  return dst;
}

// Latent pass (main.cpp:2053-2519, 5280-5352): full causal forward without the decode cache.
// dst[l][c][p][:] = src[l][0][p][:] for p < n_prompt: the prompt rows of the decode cache (identical for every candidate)
// become the first rows of every candidate in the latent pass' K/V buffers. grid (n_prompt, nb, 2 * n_layers).
__global__ __launch_bounds__(256) void copy_prompt_kv_kernel(const __half *__restrict__ ksrc, const __half *__restrict__ vsrc,
                                                             size_t src_layer_stride, __half *__restrict__ kdst, __half *__restrict__ vdst,
                                                             size_t dst_layer_stride, int S, int n_layers) {
  const int p = blockIdx.x, c = blockIdx.y, l = blockIdx.z % n_layers;
  const bool isv = (int)blockIdx.z >= n_layers;
  const __half *src = (isv ? vsrc : ksrc) + l * src_layer_stride + (size_t)p * D;
  __half *dst = (isv ? vdst : kdst) + l * dst_layer_stride + ((size_t)c * S + p) * D;
  ((uint2 *)dst)[threadIdx.x] = ((const uint2 *)src)[threadIdx.x];
}

// Latent pass (main.cpp:2053-2519): the full stack over [voice | text | mel codes at mel positions 0..] without the
// decode cache's position quirk. The 1 + n_text prompt rows are the same for every candidate and do not depend on the
// mel rows (causal mask): their K/V rows are taken from the decode cache (written by the prompt pass), so the stack runs
// over the mel rows only, with n_past = 1 + n_text. Several prompts: one such pass per group, over the group's own prompt (its first
// candidate's cache rows) and n_mel. Several voices: position 0 of those cache rows was embedded from the group's own voice by its prompt pass, so the
// latent pass reads the right voice without naming it.
static int latents_check(tts_ctx *ctx, const ArState *st, int n_text, const int32_t *codes502, int nb, int n_mel) {
  if (nb < 1 || n_mel < 1 || n_mel > 502 || !codes502) return fail(ctx, TTS_ERR_ARG, "tts_ar_latents: bad argument");
  if (1 + n_text + n_mel > 1024) return fail(ctx, TTS_ERR_LIMIT, "latent pass of %d positions exceeds 1024", 1 + n_text + n_mel);
  for (int c = 0; c < nb; c++)
    for (int j = 0; j < n_mel; j++) {
      const int code = codes502[c * 502 + j];
      if (code < 0 || code >= V) return fail(ctx, TTS_ERR_ARG, "mel code %d out of range", code);
    }
  return TTS_OK;
}

// c0: the cache row that holds the prompt's K/V rows (a group's first candidate; a session request's first slot), n_text: that prompt's length.
// The body tts_ar_latents and tts_ar_score_codes share: desc [nb][n_mel] = (2, input id, 1, mel position id) of every row; leaves hn [nb * n_mel][1024] on the
// device, enqueued on the context's stream.
static int latents_body(tts_ctx *ctx, ArState *st, int c0, int n_text, const std::vector<int4> &desc, int nb, int n_mel) {
  const int Sp = 1 + n_text, S = Sp + n_mel, rows = nb * n_mel;
  CHECK(reserve_rows(ctx, st, rows));
  const size_t lat_stride = (size_t)nb * S * D; // per layer: [cand][S][1024]
  TTS_HIP(ctx, st->lat_k.reserve(st->n_layers * lat_stride * sizeof(__half)));
  TTS_HIP(ctx, st->lat_v.reserve(st->n_layers * lat_stride * sizeof(__half)));
  const size_t src0 = (size_t)c0 * st->max_pos * D;
  copy_prompt_kv_kernel<<<dim3(Sp, nb, 2 * st->n_layers), 256, 0, ctx->stream>>>(
      st->kcache.as<__half>() + src0, st->vcache.as<__half>() + src0, (size_t)st->B * st->max_pos * D, st->lat_k.as<__half>(), st->lat_v.as<__half>(),
      lat_stride, S, st->n_layers);
  CHECK(embed(ctx, st, desc));
  CHECK(run_layers(ctx, st, rows, n_mel, Sp, st->lat_k.as<__half>(), st->lat_v.as<__half>(), lat_stride, S, 0));
  float *xn = st->xn.as<float>(), *hn = st->hn.as<float>();
  layernorm_kernel<<<rows, 256, 0, ctx->stream>>>(st->h.as<float>(), st->lnf_g, st->lnf_b, xn);
  layernorm_kernel<<<rows, 256, 0, ctx->stream>>>(xn, st->lmh_g, st->lmh_b, hn);
  TTS_HIP(ctx, hipGetLastError());
  return TTS_OK;
}

static int latents_rows(tts_ctx *ctx, ArState *st, int c0, int n_text, const int32_t *codes502, int nb, int n_mel, float *out) {
  std::vector<int4> desc((size_t)nb * n_mel);
  for (int c = 0; c < nb; c++)
    for (int j = 0; j < n_mel; j++) desc[(size_t)c * n_mel + j] = make_int4(2, codes502[c * 502 + j], 1, j);
  CHECK(latents_body(ctx, st, c0, n_text, desc, nb, n_mel));
  const float *hn = st->hn.as<float>();
  const int n_out = std::min(500, n_mel);
  for (int c = 0; c < nb; c++)
    TTS_HIP(ctx, hipMemcpyAsync(out + (size_t)c * n_out * D, hn + (size_t)c * n_mel * D, (size_t)n_out * D * 4, hipMemcpyDeviceToHost,
                                ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TTS_OK;
}

// tts_ar_score_codes behind tts_ar_begin (one prompt, one voice) and the prompt pass: the latent pass over nb candidates x n_rows rows (input_ids / mel_pos /
// targets [nb][n_rows], the row table of tts_host_ar_score_rows, padded by the caller), then the fused head over hn. out [4][nb * n_rows] on the host:
// lse | logp | stop_logp | greedy (int32 bits), copied once behind one synchronisation. Always the f32 head (lm_w), whatever ar_weights holds.
int ar_score_rows(tts_ctx *ctx, const int32_t *input_ids, const int32_t *mel_pos, const int32_t *targets, int nb, int n_rows, float *out) {
  ArState *st = ctx->ar;
  if (!st || st->B == 0 || st->multi || st->session || !st->prefill_done) return fail(ctx, TTS_ERR_STATE, "ar_score_rows: no single-prompt tts_ar_begin + prompt pass");
  const int rows = nb * n_rows;
  if (!ar_score_shape_ok(rows, D, V, VPAD)) return fail(ctx, TTS_ERR_ARG, "ar_score_rows: %d rows", rows);
  std::vector<int4> desc((size_t)rows);
  for (int r = 0; r < rows; r++) desc[r] = make_int4(2, input_ids[r], 1, mel_pos[r]);
  CHECK(latents_body(ctx, st, st->g_c0[0], st->g_ntext[0], desc, nb, n_rows));
  TTS_HIP(ctx, st->score_ws.reserve(ar_score_ws_floats(rows, V) * 4));
  TTS_HIP(ctx, st->score_io.reserve((size_t)5 * rows * 4));
  int *d_tgt = st->score_io.as<int>();
  float *d_out = st->score_io.as<float>() + rows;
  TTS_HIP(ctx, hipMemcpyAsync(d_tgt, targets, (size_t)rows * 4, hipMemcpyHostToDevice, ctx->stream));
  { ProfScope ps(ctx, "ar_score", 2.0 * rows * (double)D * V);
    const ArScore a{st->hn.as<float>(), st->lm_w, st->lm_b, d_tgt, st->score_ws.as<float>(), rows, D, V, VPAD};
    const ArScoreOut o{d_out, d_out + rows, d_out + 2 * (size_t)rows, (int *)(d_out + 3 * (size_t)rows), nullptr, nullptr};
    TTS_HIP(ctx, ar_score_launch(a, o, ctx->stream)); }
  TTS_HIP(ctx, hipMemcpyAsync(out, d_out, (size_t)4 * rows * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TTS_OK;
}

static int latents_group(tts_ctx *ctx, ArState *st, int g, const int32_t *codes502, int nb, int n_mel, float *out) {
  return latents_rows(ctx, st, st->g_c0[g], st->g_ntext[g], codes502, nb, n_mel, out);
}

// tts_ar_latents. Several prompts: nb must be the whole batch, every candidate is evaluated against its own prompt (out [B][min(500, n_mel)][1024]).
int ar_latents(tts_ctx *ctx, const int32_t *codes502, int nb, int n_mel, float *out) {
  ArState *st = ctx->ar;
  if (!st || st->B == 0) return fail(ctx, TTS_ERR_STATE, "tts_ar_begin not called");
  if (st->multi && nb != st->B) return fail(ctx, TTS_ERR_ARG, "tts_ar_latents: %d candidates, the batch of several prompts has %d", nb, st->B);
  CHECK(latents_check(ctx, st, st->n_text, codes502, nb, n_mel));
  if (!st->prefill_done) CHECK(ar_prefill(ctx, nullptr));
  if (!st->multi) return latents_group(ctx, st, 0, codes502, nb, n_mel, out);
  const size_t n_out = std::min(500, n_mel);
  for (int g = 0; g < (int)st->g_n.size(); g++)
    CHECK(latents_group(ctx, st, g, codes502 + (size_t)st->g_c0[g] * 502, st->g_n[g], n_mel, out + (size_t)st->g_c0[g] * n_out * D));
  return TTS_OK;
}

// The latent pass of group g alone (the driver's per-group n_mel): codes502 / out hold the group's candidates only.
int ar_latents_group(tts_ctx *ctx, int g, const int32_t *codes502, int n_mel, float *out) {
  ArState *st = ctx->ar;
  if (!st || st->B == 0 || g < 0 || g >= (int)st->g_n.size()) return fail(ctx, TTS_ERR_STATE, "tts_ar_begin not called");
  CHECK(latents_check(ctx, st, st->g_ntext[g], codes502, st->g_n[g], n_mel));
  if (!st->prefill_done) CHECK(ar_prefill(ctx, nullptr));
  return latents_group(ctx, st, g, codes502, st->g_n[g], n_mel, out);
}

// tts_hifigan_stream runs latent passes of growing length BETWEEN decode steps. A DevBuf that grows frees and reallocates, and the captured decode step bakes
// h, qkv, att and ff into its nodes (GraphSig): growing inside the loop would be safe and re-capture the ~150-node graph at every growth. Called right after
// ar_begin_groups (which has validated the call; nothing has run on the buffers yet) with the longest pass the call can run, so that nothing moves afterwards.
int ar_stream_reserve(tts_ctx *ctx, int n_mel) {
  ArState *st = ctx->ar;
  if (!st || st->B < 1) return fail(ctx, TTS_ERR_STATE, "tts_ar_begin not called");
  const int n_text = st->n_text;
  CHECK(reserve_rows(ctx, st, std::max({16, n_text + 2, n_mel})));
  TTS_HIP(ctx, hipMemsetAsync(st->h.p, 0, st->h.cap, ctx->stream)); // ar_begin_groups' zeroed padding rows, again: h may have moved
  const size_t lat = (size_t)st->n_layers * (1 + n_text + n_mel) * D * sizeof(__half);
  TTS_HIP(ctx, st->lat_k.reserve(lat));
  TTS_HIP(ctx, st->lat_v.reserve(lat));
  if (n_mel >= 32) { // launch_mfma_matmul's operands
    const size_t rpad = (size_t)(n_mel + 127) & ~(size_t)127;
    TTS_HIP(ctx, st->a_hi.reserve(rpad * FF * sizeof(__half)));
    TTS_HIP(ctx, st->a_lo.reserve(rpad * FF * sizeof(__half)));
    TTS_HIP(ctx, st->part.reserve(rpad * FF * sizeof(float)));
  }
  return TTS_OK;
}
int ar_graph_captures(const tts_ctx *ctx) { return ctx->ar ? ctx->ar->graph_captures : 0; }

// ---------------------------------------------------------------------------------------------
// Sessions (tts_ar_session_*): the device side. The book of slots and requests is the caller's (ar_driver.cpp); here a session is a batch of n_slots rows whose
// caches hold max_text + 2 + max_steps + 1 positions, every row at its own step (ArState::session).
// ---------------------------------------------------------------------------------------------
// A control table entry: what the penalising prefilter reads of one row's sampler controls.
static int4 control_entry(const SamplerParams &sp, int scope) {
  return make_int4(pf_min_for(sp.top_k), (int)__builtin_bit_cast(uint32_t, sp.penalty), scope, (int)__builtin_bit_cast(uint32_t, sp.typ_mass)); // (mass 0.f: all bits 0)
}
static void hist_reset_row(uint32_t *hb) { // what a begin leaves: ids 1 and 8192 (the prompt-shaped penalty row of step 0)
  std::fill(hb, hb + TTS_HIST_WORDS, 0u);
  hb[1 >> 5] |= 1u << (1 & 31);
  hb[8192 >> 5] |= 1u << (8192 & 31);
}

// Every buffer that the decode step, a prompt pass of max_text + 2 rows and a latent pass of max_cand x 502 rows can touch is reserved here: nothing the
// captured step bakes into its nodes (GraphSig) moves while the session is open. The caller has checked the limits.
int ar_session_open(tts_ctx *ctx, int n_slots, int max_cand, int max_text, int max_steps, bool rows) {
  ArState *st = ctx->ar;
  if (!st) return fail(ctx, TTS_ERR_STATE, "AR model not loaded");
  if (ctx->ar_weights != 0 && ctx->ar_weights != st->loaded_wmode)
    return fail(ctx, TTS_ERR_STATE, "option ar_weights = %d must be set before tts_load_ar (the fp16 / fp8 slabs are packed at load)", ctx->ar_weights);
  const int B = n_slots, Bpad = (B + 15) / 16 * 16, P = max_text + 2, max_pos = P + max_steps + 1;
  st->B = 0; // (a failure below leaves no half-open state behind)
  st->session = false;
  st->rows = false;
  st->g_c0.clear(); st->g_n.clear(); st->g_t0.clear(); st->g_ntext.clear(); st->g_voice.clear(); st->tokens.clear();
  st->multi = false;
  st->n_text = max_text; st->P = P; st->max_pos = max_pos;
  st->prefill_done = false;
  TTS_HIP(ctx, st->voice.reserve((size_t)B * D * 4)); // one row per slot: a request's voice sits in the row of its first slot
  const size_t cache = (size_t)st->n_layers * B * max_pos * D * sizeof(__half);
  TTS_HIP(ctx, st->kcache.reserve(cache));
  TTS_HIP(ctx, st->vcache.reserve(cache));
  TTS_HIP(ctx, st->d_toks.reserve((size_t)(B + 2) * 4));
  TTS_HIP(ctx, st->logits.reserve((size_t)B * V * 4));
  TTS_HIP(ctx, st->row_off.reserve((size_t)Bpad * sizeof(int)));
  TTS_HIP(ctx, hipMemsetAsync(st->row_off.p, 0, (size_t)Bpad * sizeof(int), ctx->stream));
  CHECK(reserve_pinned(ctx, st, B));
  st->hist_host.assign((size_t)B * TTS_HIST_WORDS, 0u);
  for (int b = 0; b < B; b++) hist_reset_row(st->hist_host.data() + (size_t)b * TTS_HIST_WORDS);
  TTS_HIP(ctx, st->hist.reserve(st->hist_host.size() * 4));
  TTS_HIP(ctx, hipMemcpy(st->hist.p, st->hist_host.data(), st->hist_host.size() * 4, hipMemcpyHostToDevice));
  st->hist_dev_valid = false; // (a later tts_ar_begin* starts from its own host copy)
  if (rows) { // the control table, padded to whole tiles: every row starts under the session's own controls (a valid entry; every admission writes its own)
    TTS_HIP(ctx, st->ctl.reserve((size_t)Bpad * sizeof(int4)));
    const std::vector<int4> own((size_t)Bpad, control_entry(ctx->ar_sp, ctx->ar_penalty_scope));
    TTS_HIP(ctx, hipMemcpy(st->ctl.p, own.data(), own.size() * sizeof(int4), hipMemcpyHostToDevice));
  }
  const int lat_rows = max_cand * 502, S_max = std::min(1024, 1 + max_text + 502);
  CHECK(reserve_rows(ctx, st, std::max({Bpad, P, lat_rows})));
  TTS_HIP(ctx, hipMemsetAsync(st->h.p, 0, st->h.cap, ctx->stream)); // the tile padding rows of the h4 layout are read (never stored): finite
  const size_t lat = (size_t)st->n_layers * max_cand * S_max * D * sizeof(__half);
  TTS_HIP(ctx, st->lat_k.reserve(lat));
  TTS_HIP(ctx, st->lat_v.reserve(lat));
  const size_t rpad = (size_t)(lat_rows + 127) & ~(size_t)127; // launch_mfma_matmul's operands; launch_gemv's partials (at most 16 K splits of 31 rows)
  TTS_HIP(ctx, st->a_hi.reserve(rpad * FF * sizeof(__half)));
  TTS_HIP(ctx, st->a_lo.reserve(rpad * FF * sizeof(__half)));
  TTS_HIP(ctx, st->part.reserve(std::max(rpad, (size_t)16 * 32) * FF * sizeof(float)));
  // An empty slot sits at position 0 with token 8193: every step stores its K/V row there before the attention reads it, so it never reads
  // uninitialised memory.
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st->sess_captures0 = -1;
  st->session = true;
  st->rows = rows;
  st->sa_S = 0; st->sa_rows = 0; // no audio until tts_ar_session_enable_audio
  st->B = B;
  return TTS_OK;
}

void ar_session_close(tts_ctx *ctx) {
  ArState *st = ctx->ar;
  if (!st || !st->session) return;
  st->session = false;
  st->rows = false;
  st->sa_S = 0; st->sa_rows = 0;
  st->B = 0; // tts_ar_begin* starts over; the session's step graph stays for the next session of the same shape
}

// A request's prompt pass into its slots [c0, c0 + n_cand): its voice goes to row c0 of the voice table, its K/V rows into its slots' caches only, its first
// logits to row c0 (copied to logits_row), and its history sets start over in the host copy and in the device rows. The caller has checked the arguments.
int ar_session_prompt(tts_ctx *ctx, int c0, int n_cand, const int32_t *text_ids, int n_text, const float *voice, float *logits_row) {
  ArState *st = ctx->ar;
  if (!st || !st->session || c0 < 0 || n_cand < 1 || c0 + n_cand > st->B || n_text < 1 || n_text > st->n_text)
    return fail(ctx, TTS_ERR_STATE, "tts_ar_session_admit: no session, or a request outside it");
  TTS_HIP(ctx, hipMemcpy(st->voice.as<float>() + (size_t)c0 * D, voice, (size_t)D * 4, hipMemcpyHostToDevice));
  uint32_t *hb = st->hist_host.data() + (size_t)c0 * TTS_HIST_WORDS;
  for (int b = 0; b < n_cand; b++) hist_reset_row(hb + (size_t)b * TTS_HIST_WORDS);
  TTS_HIP(ctx, hipMemcpy(st->hist.as<uint32_t>() + (size_t)c0 * TTS_HIST_WORDS, hb, (size_t)n_cand * TTS_HIST_WORDS * 4, hipMemcpyHostToDevice));
  const std::vector<int> tok(text_ids, text_ids + n_text);
  CHECK(prompt_pass(ctx, st, c0, n_cand, n_text, tok.data(), c0));
  TTS_HIP(ctx, hipMemcpyAsync(logits_row, st->logits.as<float>() + (size_t)c0 * V, (size_t)V * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TTS_OK;
}

// Rows [c0, c0 + n) of a rows session's control table take a request's controls at its admission: written between two steps, outside the graph, as
// ar_session_prompt resets the history rows.
int ar_session_controls(tts_ctx *ctx, int c0, int n, const SamplerParams &sp, int scope) {
  ArState *st = ctx->ar;
  if (!st || !st->session || !st->rows || c0 < 0 || n < 1 || c0 + n > st->B) return fail(ctx, TTS_ERR_STATE, "ar_session_controls: no session with per-row controls, or rows outside it");
  const std::vector<int4> e((size_t)n, control_entry(sp, scope));
  TTS_HIP(ctx, hipMemcpy(st->ctl.as<int4>() + c0, e.data(), e.size() * sizeof(int4), hipMemcpyHostToDevice));
  return TTS_OK;
}

// One step over all slots: row r is fed toks[r] at mel position pos_id[r] with n_past[r] positions behind it. live[r]: the row belongs to a running request
// (its token joins the row's history set in the host copy; on the device the step's own kernels add it for every row, and an admission resets the rows it
// takes). mode as ar_step's.
int ar_session_step(tts_ctx *ctx, const int32_t *toks, const int32_t *n_past, const int32_t *pos_id, const char *live, int mode) {
  ArState *st = ctx->ar;
  if (!st || !st->session || st->B == 0) return fail(ctx, TTS_ERR_STATE, "tts_ar_session_open not called");
  if (mode < 0 || mode > 2) return fail(ctx, TTS_ERR_ARG, "ar_session_step: bad mode");
  const int B = st->B, Bpad = (B + 15) / 16 * 16;
  for (int r = 0; r < B; r++) {
    if (toks[r] < 0 || toks[r] >= V) return fail(ctx, TTS_ERR_ARG, "mel token %d out of range", toks[r]);
    if (n_past[r] < 0 || n_past[r] >= st->max_pos) return fail(ctx, TTS_ERR_LIMIT, "slot %d: position %d beyond the KV cache", r, n_past[r]);
    if (pos_id[r] < 0 || pos_id[r] >= 608) return fail(ctx, TTS_ERR_LIMIT, "slot %d: mel position %d of 608", r, pos_id[r]);
  }
  st->step_mode = mode;
  st->step_scope = ctx->ar_penalty_scope;
  st->step_pf_min = pf_min_for(ctx->ar_sp.top_k);
  st->step_penalty = ctx->ar_sp.penalty;
  st->step_mass = ctx->ar_sp.typ_mass;
  double kv_rows = 0;
  for (int r = 0; r < B; r++) {
    st->h_toks[r] = toks[r];
    st->h_toks[B + r] = n_past[r];
    st->h_toks[B + Bpad + r] = pos_id[r];
    if (live[r]) st->hist_host[(size_t)r * TTS_HIST_WORDS + (toks[r] >> 5)] |= 1u << (toks[r] & 31);
    kv_rows += n_past[r] + 1;
  }
  for (int r = B; r < Bpad; r++) st->h_toks[B + r] = 0;
  const double step_bytes = (ctx->ar_weights == 2 ? 1.0 : ctx->ar_weights == 1 ? 2.0 : 4.0) * ((double)st->n_layers * 12.0 * D * D + (double)D * V) +
                            kv_rows * st->n_layers * 2.0 * D * 2.0 + (double)B * V * 4.0;
  CHECK(launch_step(ctx, st, st->rows ? 4 : 3, step_bytes));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (st->sess_captures0 < 0) st->sess_captures0 = st->graph_captures;
  return TTS_OK;
}
int ar_session_recaptures(const tts_ctx *ctx) {
  const ArState *st = ctx->ar;
  return (st && st->session && st->sess_captures0 >= 0) ? st->graph_captures - st->sess_captures0 : 0;
}

// The latent pass of a request: nb candidates over the prompt rows of slot c0 (n_text ids) and n_mel codes each; out [nb][min(500, n_mel)][1024].
int ar_session_latents(tts_ctx *ctx, int c0, int n_text, const int32_t *codes502, int nb, int n_mel, float *out) {
  ArState *st = ctx->ar;
  if (!st || !st->session || c0 < 0 || c0 + nb > st->B) return fail(ctx, TTS_ERR_STATE, "tts_ar_session_open not called");
  CHECK(latents_check(ctx, st, n_text, codes502, nb, n_mel));
  return latents_rows(ctx, st, c0, n_text, codes502, nb, n_mel, out);
}

// Rows [c0, c0 + n) of the last step's logits, from HBM.
int ar_session_logits(tts_ctx *ctx, int c0, int n, float *out) {
  ArState *st = ctx->ar;
  if (!st || !st->session || c0 < 0 || n < 1 || c0 + n > st->B) return fail(ctx, TTS_ERR_STATE, "tts_ar_session_open not called");
  TTS_HIP(ctx, hipMemcpy(out, st->logits.as<float>() + (size_t)c0 * V, (size_t)n * V * 4, hipMemcpyDeviceToHost));
  return TTS_OK;
}

// ---- session audio: the ragged, incremental latent pass ----
// Reserves the per-slot latent K/V rows and every buffer a launch sequence of ar_session_extend can grow (the captured step bakes h, qkv, att and ff into its
// nodes: nothing may move once the session steps). Called before the first admission.
int ar_session_audio_enable(tts_ctx *ctx, int max_steps) {
  ArState *st = ctx->ar;
  if (!st || !st->session || st->B < 1) return fail(ctx, TTS_ERR_STATE, "tts_ar_session_open not called");
  const int B = st->B, S_max = 1 + st->n_text + std::min(502, max_steps + 10);
  const size_t kv = (size_t)st->n_layers * B * S_max * D * sizeof(__half);
  TTS_HIP(ctx, st->sa_k.reserve(kv));
  TTS_HIP(ctx, st->sa_v.reserve(kv));
  // every live request may bring its whole utterance to one pass (stride above max_steps, all finishing together); past 4096 rows the pass runs in
  // several launch sequences (a row's bits do not depend on what else is packed beside it)
  const int rows = std::max(512, std::min(4096, B * std::min(500, max_steps + 1)));
  TTS_HIP(ctx, st->sa_tab.reserve((size_t)B * sizeof(int4) + (size_t)rows * sizeof(int)));
  CHECK(reserve_rows(ctx, st, rows));
  TTS_HIP(ctx, hipMemsetAsync(st->h.p, 0, st->h.cap, ctx->stream)); // ar_session_open's zeroed padding rows, again: h may have moved
  const size_t rpad = (size_t)(rows + 127) & ~(size_t)127; // launch_mfma_matmul's operands
  TTS_HIP(ctx, st->a_hi.reserve(rpad * FF * sizeof(__half)));
  TTS_HIP(ctx, st->a_lo.reserve(rpad * FF * sizeof(__half)));
  TTS_HIP(ctx, st->part.reserve(rpad * FF * sizeof(float)));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st->sa_S = S_max;
  st->sa_rows = rows;
  return TTS_OK;
}

// A one-candidate request's prompt rows [0, 1 + n_text), from the decode cache of its slot (its prompt pass has just written them) into the slot's latent K/V.
int ar_session_audio_prompt(tts_ctx *ctx, int c0, int n_text) {
  ArState *st = ctx->ar;
  if (!st || !st->session || !st->sa_S || c0 < 0 || c0 >= st->B || n_text < 1 || n_text > st->n_text)
    return fail(ctx, TTS_ERR_STATE, "tts_ar_session_enable_audio not called");
  const size_t src0 = (size_t)c0 * st->max_pos * D, dst0 = (size_t)c0 * st->sa_S * D;
  copy_prompt_kv_kernel<<<dim3(1 + n_text, 1, 2 * st->n_layers), 256, 0, ctx->stream>>>(
      st->kcache.as<__half>() + src0, st->vcache.as<__half>() + src0, (size_t)st->B * st->max_pos * D, st->sa_k.as<__half>() + dst0, st->sa_v.as<__half>() + dst0,
      (size_t)st->B * st->sa_S * D, st->sa_S, st->n_layers);
  TTS_HIP(ctx, hipGetLastError());
  return TTS_OK;
}

// One launch sequence over the packed new rows of items [0, n): run_layers' loop on the split-precision MFMA path whatever the row count (the GEMMs pad to
// 128 rows themselves), with the two per-row pieces in their ragged forms. out: the items' rows back to back.
static int extend_launch(tts_ctx *ctx, ArState *st, const ArExtendItem *items, int n, float *out) {
  int rows = 0, max_S = 0;
  for (int k = 0; k < n; k++) { rows += items[k].upto - items[k].have; max_S = std::max(max_S, items[k].upto - items[k].have); }
  std::vector<int4> desc((size_t)rows);
  std::vector<int> tab((size_t)4 * st->B + rows);
  int *row_dst = tab.data() + (size_t)4 * st->B;
  for (int k = 0, r = 0; k < n; k++) {
    const ArExtendItem &it = items[k];
    const int n_past = 1 + it.n_text + it.have;
    tab[4 * k] = r; tab[4 * k + 1] = it.upto - it.have; tab[4 * k + 2] = n_past; tab[4 * k + 3] = it.slot;
    for (int j = it.have; j < it.upto; j++, r++) {
      desc[r] = make_int4(2, it.codes502[j], 1, j);
      row_dst[r] = it.slot * st->sa_S + 1 + it.n_text + j;
    }
  }
  TTS_HIP(ctx, hipMemcpyAsync(st->sa_tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  const int4 *d_items = st->sa_tab.as<int4>();
  const int *d_row_dst = st->sa_tab.as<int>() + (size_t)4 * st->B;
  CHECK(embed(ctx, st, desc));
  float *h = st->h.as<float>(), *xn = st->xn.as<float>(), *qkv = st->qkv.as<float>(), *att = st->att.as<float>(), *ff = st->ff.as<float>();
  const KvDst nokv{nullptr, nullptr, 1, 0, 0, 0};
  const float ps = 1.0f / W16_SCALE;
  const size_t layer_stride = (size_t)st->B * st->sa_S * D;
  for (int l = 0; l < st->n_layers; l++) {
    const ArLayerDev &w = st->L[l];
    __half *kc = st->sa_k.as<__half>() + l * layer_stride, *vc = st->sa_v.as<__half>() + l * layer_stride;
    { ProfScope p(ctx, "ar_layernorm");
      layernorm_kernel<<<rows, 256, 0, ctx->stream>>>(h, w.ln1_g, w.ln1_b, xn); }
    CHECK(launch_mfma_matmul(ctx, st, xn, rows, w.s_attn, 3 * D, D));
    { ProfScope p(ctx, "ar_epilogue");
      epilogue_qkv_ragged_kernel<<<dim3(rows, 3 * D / 256), 256, 0, ctx->stream>>>(st->part.as<float>(), w.b_attn, qkv, d_row_dst, kc, vc, ps); }
    { ProfScope p(ctx, "ar_attention");
      attention_rows_ragged_kernel<<<dim3(n, NH, (max_S + 63) / 64), 256, 0, ctx->stream>>>(qkv, kc, vc, att, d_items, st->sa_S); }
    CHECK(launch_mfma_matmul(ctx, st, att, rows, w.s_proj, D, D));
    CHECK(launch_epilogue<EPI_RESID>(ctx, st, 1, rows, D, D, w.b_proj, h, D, nokv, ps));
    { ProfScope p(ctx, "ar_layernorm");
      layernorm_kernel<<<rows, 256, 0, ctx->stream>>>(h, w.ln2_g, w.ln2_b, xn); }
    CHECK(launch_mfma_matmul(ctx, st, xn, rows, w.s_fc, FF, D));
    CHECK(launch_epilogue<EPI_GELU>(ctx, st, 1, rows, FF, FF, w.b_fc, ff, FF, nokv, ps));
    CHECK(launch_mfma_matmul(ctx, st, ff, rows, w.s_fc2, D, FF));
    CHECK(launch_epilogue<EPI_RESID>(ctx, st, 1, rows, D, D, w.b_fc2, h, D, nokv, ps));
  }
  float *hn = st->hn.as<float>();
  layernorm_kernel<<<rows, 256, 0, ctx->stream>>>(h, st->lnf_g, st->lnf_b, xn);
  layernorm_kernel<<<rows, 256, 0, ctx->stream>>>(xn, st->lmh_g, st->lmh_b, hn);
  TTS_HIP(ctx, hipGetLastError());
  for (int k = 0, r = 0; k < n; k++) {
    const int S = items[k].upto - items[k].have;
    TTS_HIP(ctx, hipMemcpyAsync(out + (size_t)r * D, hn + (size_t)r * D, (size_t)S * D * 4, hipMemcpyDeviceToHost, ctx->stream));
    r += S;
  }
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return TTS_OK;
}

// The latent rows [have, upto) of every item (a one-candidate request in slot `slot` whose rows [0, have) went through earlier calls), computed alone
// against the K/V rows those calls left: bit for bit the rows of a full latent pass (tts_ar_latents of 32 rows or more). Every argument is checked first.
int ar_session_extend(tts_ctx *ctx, const ArExtendItem *items, int n_items, float *out) {
  ArState *st = ctx->ar;
  if (!st || !st->session || !st->sa_S) return fail(ctx, TTS_ERR_STATE, "tts_ar_session_enable_audio not called");
  if (ctx->ggml_lut) return fail(ctx, TTS_ERR_STATE, "ar_session_extend: no incremental latent pass under ggml_lut = 1");
  if (!items || n_items < 1 || n_items > st->B || !out) return fail(ctx, TTS_ERR_ARG, "ar_session_extend: bad argument");
  for (int k = 0; k < n_items; k++) {
    const ArExtendItem &it = items[k];
    if (it.slot < 0 || it.slot >= st->B || it.n_text < 1 || it.n_text > st->n_text || it.have < 0 || it.upto <= it.have || it.upto > 500 || !it.codes502)
      return fail(ctx, TTS_ERR_ARG, "ar_session_extend: item %d: slot %d, %d ids, rows [%d, %d)", k, it.slot, it.n_text, it.have, it.upto);
    if (1 + it.n_text + it.upto > st->sa_S)
      return fail(ctx, TTS_ERR_LIMIT, "ar_session_extend: item %d ends at position %d of %d", k, 1 + it.n_text + it.upto, st->sa_S);
    for (int j = it.have; j < it.upto; j++)
      if (it.codes502[j] < 0 || it.codes502[j] >= V) return fail(ctx, TTS_ERR_ARG, "mel code %d out of range", it.codes502[j]);
  }
  for (int k0 = 0; k0 < n_items;) { // launch sequences of at most sa_rows rows (one item has at most 500)
    int k1 = k0, rows = 0;
    while (k1 < n_items && rows + items[k1].upto - items[k1].have <= st->sa_rows) { rows += items[k1].upto - items[k1].have; k1++; }
    CHECK(extend_launch(ctx, st, items + k0, k1 - k0, out));
    out += (size_t)rows * D;
    k0 = k1;
  }
  return TTS_OK;
}

int ar_layers(const tts_ctx *ctx) { return ctx->ar ? ctx->ar->n_layers : 0; }
int ar_batch(const tts_ctx *ctx) { return ctx->ar ? ctx->ar->B : 0; }

// The pinned buffer the decode graph copies the logits into ([B][8194]); valid after ar_step returns.
float *ar_host_logits(tts_ctx *ctx) { return ctx->ar ? ctx->ar->h_logits : nullptr; }

} // namespace tts
