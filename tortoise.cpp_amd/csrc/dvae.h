// The DVAE encoder on MI355X (gfx950): an 80-band mel -> the 8192-entry speech codes the AR model is trained on      tts_load_dvae / tts_dvae_codes / tts_dvae_codes_audio
//
// Included once, as the last line of aligner.h (hifigan.hip's translation unit; its loader and level tables are model_io.h's): get_codebook_indices of upstream tortoise-tts' DiscreteVAE(channels 80,
// positional_dims 1, num_tokens 8192, codebook_dim 512, hidden_dim 512, num_layers 2, num_resnet_blocks 3, kernel_size 3, no normalization). Upstream's source and
// weights are not available offline: the contract is the arithmetic below ("What pins the DVAE"), checked between two float64 spellings
// (tests/dvae_ref.py); unpinned against upstream. f32 throughout: a code is an argmin.
//
//   h = ReLU(Conv1d(80 -> C_0, k, stride s, pad (k - 1) / 2)(mel))                           dvae_stem_kernel (reads the front end's band-major mel [80][T])
//   layer i = 1 .. L - 1:  h = ReLU(Conv1d(C_{i-1} -> C_i, k, stride s, pad (k - 1) / 2)(h))   cls_down_kernel + dvae_relu_kernel (the ReLU is stored: h is the residual stream)
//   blocks x:  h = h + Conv1(ReLU(Conv3(ReLU(Conv3(h)))))                                    hfg_conv_kernel: slope 1, then slope 0 twice, the skip in `resid`
//   z = Conv1d(H -> dim, k 1)(h)                                                             hfg_conv_kernel, slope 1
//   code[t] = argmin_j |E_j|^2 - 2 z[t] . E_j, the lowest index on a tie                     dvae_vq_kernel + dvae_vq_reduce_kernel
//
// Device layout: time-major f32 rows [row][channels]; clip s owns the rows [start_s, start_s + n_s) of a level, the clips packed without gaps. Level 0 is the mel
// (band-major, clip s at 80 x the frames before it: what the audio front end writes), level i the output of strided layer i - 1. No kernel reads or writes a row
// outside the clip it works on and none uses atomics: two runs agree bit for bit, and a clip alone gives the bits of the clip in a batch.
//
// What the kernels can tile (dvae_parse refuses everything else, TTS_ERR_FORMAT): 1 .. 128 mel channels; odd kernel sizes up to 7; stride 1 .. 4; every
// channel count a multiple of 64 up to 4096; codebook dim a multiple of 32 up to 512 (the quantiser keeps 64 rows of it in LDS); tokens a multiple of 32 up to 65536.
#pragma once
#include <array>

namespace tts {

namespace {
constexpr int DVS_ROWS = 16;    // output rows of a dvae_stem_kernel workgroup; a thread owns one output channel of all of them
constexpr int DVR_ROWS = 64;    // rows of a dvae_relu_kernel workgroup
constexpr int DVQ_TM = 64;      // rows of a dvae_vq_kernel workgroup: two 32-row MFMA tiles per wave share every codebook fragment
constexpr int DVQ_SLAB = 256;   // codes of a dvae_vq_kernel workgroup: 8 tiles of 32, tiles w and w + 4 on wave w
constexpr int DVAE_MAX_CIN = 128, DVAE_MAX_K = 7, DVAE_MAX_STRIDE = 4, DVAE_MAX_C = 4096, DVAE_MAX_DIM = 512, DVAE_MAX_TOKENS = 65536, DVAE_MAX_LAYERS = 8;
constexpr int DVAE_MAX_CLIPS = 256, DVAE_MAX_FRAMES = 16384;

struct DvaeStem {
  const float *mel;  // level 0: clip s band-major [cin][T] at float seq_in[s][4]
  float *out;        // [rows_out][cout]
  const float *w;    // [tap][cin][cout]
  const float *bias; // [cout]
  const int *seq_in, *seq_out;
  int cin, cout, taps, stride, pad; // input frame of tap j for output row t: t stride - pad + j
};
inline size_t dvae_stem_lds(int cin, int taps, int stride) { return (size_t)cin * ((DVS_ROWS - 1) * stride + taps) * 4; }

// out[t][c] = ReLU(b[c] + sum_{tap} sum_{band} w[tap][band][c] mel[band][t stride - pad + tap]): one fmaf per product from 0, taps outer, bands ascending, the bias
// added last. The workgroup's window of every band goes through LDS once (frames outside the clip read as zero: the convolution's padding); a thread reads one
// weight per product and the 16 frames of its rows as LDS broadcasts.
__global__ __launch_bounds__(256) void dvae_stem_kernel(const DvaeStem a) {
  extern __shared__ float sx[];
  const int s = blockIdx.y;
  const int T = a.seq_in[HFG_SEQ * s + 1], fo = a.seq_out[HFG_SEQ * s], T1 = a.seq_out[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * DVS_ROWS;
  if (t0 >= T1) return;
  const float *mel = a.mel + (size_t)a.seq_in[HFG_SEQ * s + 4];
  const int win = (DVS_ROWS - 1) * a.stride + a.taps, base = t0 * a.stride - a.pad;
  for (int idx = threadIdx.x; idx < a.cin * win; idx += 256) {
    const int b = idx / win, f = base + idx % win;
    sx[idx] = f >= 0 && f < T ? mel[(size_t)b * T + f] : 0.f;
  }
  __syncthreads();
  const int c = blockIdx.z * 256 + threadIdx.x;
  if (c >= a.cout) return;
  float acc[DVS_ROWS];
#pragma unroll
  for (int r = 0; r < DVS_ROWS; r++) acc[r] = 0.f;
  for (int tap = 0; tap < a.taps; tap++)
    for (int b = 0; b < a.cin; b++) {
      const float wv = a.w[(size_t)(tap * a.cin + b) * a.cout + c];
      const float *xr = sx + b * win + tap;
#pragma unroll
      for (int r = 0; r < DVS_ROWS; r++) acc[r] = __fmaf_rn(wv, xr[r * a.stride], acc[r]);
    }
  const float bv = a.bias[c];
#pragma unroll
  for (int r = 0; r < DVS_ROWS; r++)
    if (t0 + r < T1) a.out[((size_t)fo + t0 + r) * a.cout + c] = fmaxf(acc[r] + bv, 0.f);
}

// x = ReLU(x) on the rows of every clip (behind cls_down_kernel: the stored tensor is the residual stream), C a multiple of 4
__global__ __launch_bounds__(256) void dvae_relu_kernel(float *__restrict__ x, const int *__restrict__ seq, int C) {
  const int s = blockIdx.y;
  const int f0 = seq[HFG_SEQ * s], n = seq[HFG_SEQ * s + 1];
  const int t0 = blockIdx.x * DVR_ROWS;
  if (t0 >= n) return;
  const int rows = min(DVR_ROWS, n - t0), qpr = C / 4;
  float4 *p = (float4 *)(x + ((size_t)f0 + t0) * C);
  for (int idx = threadIdx.x; idx < rows * qpr; idx += 256) {
    const float4 v = p[idx];
    p[idx] = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
  }
}

struct DvaeVq {
  const float *z;  // [R][D]
  const float *E;  // [D][N]: the codebook as upstream stores it, code j in column j
  const float *e2; // [N]: |E_j|^2, summed in double over the channels ascending and rounded once (dvae_code_norms)
  float *pv;       // [slabs][R]: the minimum of a row over the codes of a slab
  int *pi;         // [slabs][R]: its index, the lowest on a tie
  int R, D, N;
};
inline size_t dvae_vq_lds(int D) { return (size_t)DVQ_TM * (D + 1) * 4 + (size_t)4 * DVQ_TM * 8; }
inline int dvae_vq_slabs(int N) { return (N + DVQ_SLAB - 1) / DVQ_SLAB; }

// The quantiser: s_j = fmaf(-2, z . E_j, |E_j|^2) with z . E_j on the f32-input MFMA (one fmaf per channel from 0, channels ascending: bitwise an fmaf chain),
// and the running minimum of every row fused in; the [rows][codes] matrix lives in the accumulators only. One workgroup: 64 rows x one slab of 256 codes. The
// 64 rows of z (all D channels, D + 1 floats per row: the 32 rows of an A fragment at one channel fall on 32 banks) are staged in LDS once; wave w walks the
// slab's 32-code tiles w and w + 4, reading the codebook from global memory in fragment order (32 consecutive codes per half-wave: 128-byte lines every row
// tile shares in L2). A lane keeps the best of its column per row (tiles ascending, a strict "<": the earlier, lower index stays); then the xor tree over the 32
// columns, the four waves through LDS and dvae_vq_reduce_kernel over the slabs all order (value, index) pairs, so the lowest index wins every tie at every
// level. Rows past R are staged as zeros and never written. N and D are multiples of 32.
__global__ __launch_bounds__(256) void dvae_vq_kernel(const DvaeVq a) {
  extern __shared__ float sx[];
  const int r0 = blockIdx.x * DVQ_TM, c0 = blockIdx.y * DVQ_SLAB;
  const int ld = a.D + 1, rows = min(DVQ_TM, a.R - r0), qpr = a.D / 4;
  for (int idx = threadIdx.x; idx < DVQ_TM * qpr; idx += 256) {
    const int r = idx / qpr, q = (idx % qpr) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) v = *(const float4 *)(a.z + ((size_t)r0 + r) * a.D + q);
    float *d = sx + r * ld + q;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  float best[2][16];
  int bi[2][16];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) { best[m][r] = INFINITY; bi[m][r] = 0x7fffffff; }
  const int cend = min(c0 + DVQ_SLAB, a.N);
  const float *xr = sx + lr * ld + lk;
  for (int j0 = c0 + wave * 32; j0 < cend; j0 += 128) {
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const float *er = a.E + (size_t)lk * a.N + j0 + lr;
    for (int k0 = 0; k0 < a.D; k0 += 32) // D is a multiple of 32
#pragma unroll 8
      for (int k = k0; k < k0 + 32; k += 2) { // lane half lk holds channel k + lk of both operands
        const float b = er[(size_t)k * a.N];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[k], b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[32 * ld + k], b, acc1, 0, 0, 0);
      }
    const int col = j0 + lr;
    const float ev = a.e2[col];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float s0 = __fmaf_rn(-2.0f, acc0[r], ev), s1 = __fmaf_rn(-2.0f, acc1[r], ev);
      if (s0 < best[0][r]) { best[0][r] = s0; bi[0][r] = col; }
      if (s1 < best[1][r]) { best[1][r] = s1; bi[1][r] = col; }
    }
  }
  float *rv = sx + DVQ_TM * ld; // [wave][row] behind the staged rows
  int *ri = (int *)(rv + 4 * DVQ_TM);
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      float v = best[m][r];
      int i = bi[m][r];
#pragma unroll
      for (int d = 16; d; d >>= 1) { // the 32 columns of a lane half: the C/D map keeps the row on (register, lane half)
        const float ov = __shfl_xor(v, d);
        const int oi = __shfl_xor(i, d);
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
      }
      if (lr == 0) {
        const int row = m * 32 + 8 * (r >> 2) + 4 * lk + (r & 3);
        rv[wave * DVQ_TM + row] = v; ri[wave * DVQ_TM + row] = i;
      }
    }
  __syncthreads();
  if ((int)threadIdx.x < rows) {
    float v = rv[threadIdx.x];
    int i = ri[threadIdx.x];
    for (int w = 1; w < 4; w++) {
      const float ov = rv[w * DVQ_TM + threadIdx.x];
      const int oi = ri[w * DVQ_TM + threadIdx.x];
      if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    const size_t o = (size_t)blockIdx.y * a.R + r0 + threadIdx.x;
    a.pv[o] = v; a.pi[o] = i;
  }
}

// codes[r] = the index of the minimum over the slabs, slabs ascending, the lowest index on a tie; best (null or [R]) receives the minimum itself. A row whose
// every distance is NaN has no minimum: code 0.
__global__ __launch_bounds__(256) void dvae_vq_reduce_kernel(const float *__restrict__ pv, const int *__restrict__ pi, int R, int slabs, int N,
                                                             int *__restrict__ codes, float *__restrict__ best) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float v = pv[r];
  int i = pi[r];
  for (int s = 1; s < slabs; s++) {
    const float ov = pv[(size_t)s * R + r];
    const int oi = pi[(size_t)s * R + r];
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  codes[r] = i >= 0 && i < N ? i : 0;
  if (best) best[r] = v;
}

// ---- the launches, stated once for dvae_run and for the test harness (testlib/dvae_harness.hip) ----
void dvae_launch_stem(const DvaeStem &a, int max_out, int B, hipStream_t st) {
  const dim3 grid((unsigned)((max_out + DVS_ROWS - 1) / DVS_ROWS), (unsigned)B, (unsigned)((a.cout + 255) / 256));
  dvae_stem_kernel<<<grid, 256, dvae_stem_lds(a.cin, a.taps, a.stride), st>>>(a);
}
void dvae_launch_relu(float *x, const int *d_seq, int C, int max_n, int B, hipStream_t st) {
  dvae_relu_kernel<<<dim3((unsigned)((max_n + DVR_ROWS - 1) / DVR_ROWS), (unsigned)B), 256, 0, st>>>(x, d_seq, C);
}
// a strided layer behind the stem: cls_down_kernel with the convolution's padding, then the ReLU into the stored tensor
void dvae_launch_down(const ClsDown &a, const int *d_seq_out, int max_out, int B, hipStream_t st) {
  cls_launch_down(a, max_out, B, st);
  dvae_launch_relu(a.out, d_seq_out, a.cout, max_out, B, st);
}
// cls_launch_conv with the input activation: slope 1 = none, slope 0 = a ReLU in hfg_conv_kernel's input stage
void dvae_launch_conv(const float *in, float *out, const float *resid, const float *w, const float *bias, const int *d_seq, int cin, int cout, int taps, float slope,
                      int max_n, int B, hipStream_t st) {
  HfgConv a{};
  a.in = in; a.out = out; a.resid = resid; a.w = w; a.bias = bias; a.cbias = nullptr; a.seq = d_seq;
  a.cin = cin; a.cout = cout; a.taps = taps; a.dil = 1; a.lo = -(taps - 1) / 2; a.phases = 1; a.pad_t = 0; a.rate = 1; a.slope = slope; a.acc_mode = 0;
  const int nt = cout % 64 == 0 ? 2 : 1;
  const dim3 grid((unsigned)((max_n + HFG_TM - 1) / HFG_TM), (unsigned)B, (unsigned)(cout / (32 * nt)));
  const size_t lds = (size_t)(HFG_TM + taps - 1) * 33 * 4;
  if (nt == 2) hfg_conv_kernel<2><<<grid, 256, lds, st>>>(a);
  else hfg_conv_kernel<1><<<grid, 256, lds, st>>>(a);
}
// best: null or [R]
hipError_t dvae_launch_vq(const DvaeVq &a, int *codes, float *best, hipStream_t st) {
  static bool raised = false; // more than 64 KB of dynamic LDS at the full codebook dim
  if (!raised) {
    const hipError_t e = hipFuncSetAttribute((const void *)dvae_vq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dvae_vq_lds(DVAE_MAX_DIM));
    if (e != hipSuccess) return e;
    raised = true;
  }
  const int slabs = dvae_vq_slabs(a.N);
  dvae_vq_kernel<<<dim3((unsigned)((a.R + DVQ_TM - 1) / DVQ_TM), (unsigned)slabs), 256, dvae_vq_lds(a.D), st>>>(a);
  dvae_vq_reduce_kernel<<<(unsigned)((a.R + 255) / 256), 256, 0, st>>>(a.pv, a.pi, a.R, slabs, a.N, codes, best);
  return hipSuccess;
}
// |E_j|^2 of a codebook [D][N]: double, channels ascending, rounded once
void dvae_code_norms(const float *E, int D, int N, float *e2) {
  std::vector<double> acc((size_t)N, 0.0);
  for (int k = 0; k < D; k++)
    for (int j = 0; j < N; j++) { const double v = E[(size_t)k * N + j]; acc[j] += v * v; }
  for (int j = 0; j < N; j++) e2[j] = (float)acc[j];
}
inline int dvae_conv_rows(int n, int stride) { return (n - 1) / stride + 1; } // odd k, pad (k - 1) / 2
bool dvae_channels_ok(int c) { return c >= 64 && c <= DVAE_MAX_C && c % 64 == 0; }
// The tables of dvae_begin (and of the test harness): level 0 = the mel frames, level i the output of strided layer i - 1; the clips packed without gaps;
// level 0 carries the first float of the clip's band-major mel [cin][frames]
template <class T>
LevelTable dvae_levels(const T *frames, int B, int L, int stride, int cin) {
  return level_table(frames, B, L + 1, [stride](int64_t v, int) { return dvae_conv_rows((int)v, stride); }, 1, 0, false, cin);
}
} // namespace

// The model as the loader's host half leaves it (no device call): the configuration from the tensor names and shapes, every tensor repacked for the kernels.
struct DvaeHostConv : HostLayer { int cin = 0, cout = 0, k = 0; }; // w: [tap][cin][cout]
struct DvaeHost {
  int L = 0, blocks = 0, cin = 0, H = 0, dim = 0, N = 0, stride = 2;
  std::vector<DvaeHostConv> down;              // the strided layers; down[0] is the stem
  std::vector<std::array<DvaeHostConv, 3>> res; // net.0, net.2, net.4
  DvaeHostConv head;                           // the final k = 1 convolution
  std::vector<float> E, e2;                    // [dim][N], [N]
};

int dvae_parse(tts_ctx *ctx, const WeightFile &wf, const char *path, DvaeHost &h) {
  const std::string P = "dvae.", EN = P + "encoder.";
  if (!wf.has(EN + "0.0.weight")) return fail(ctx, TTS_ERR_FORMAT, "'%s' is not a DVAE model file", path);
  ModelReader rd{wf, ctx, "DVAE"};
  // Conv1d [cout][cin][k] -> [k][cin][cout]; the sizes are the tensor's own, checked here in the DVAE's words; rd.conv reports a tensor that is missing
  auto conv = [&](const std::string &p, int want_cin, DvaeHostConv &c) -> int {
    if (const HostTensor *w = rd.peek(p + ".weight")) {
      if (w->n_dims != 3 || w->ne[0] < 1 || w->ne[1] < 1 || w->ne[2] < 1 || w->ne[0] > DVAE_MAX_K || w->ne[1] > DVAE_MAX_C || w->ne[2] > DVAE_MAX_C)
        return fail(ctx, TTS_ERR_FORMAT, "tensor '%s.weight' has wrong shape in DVAE model file: got [%d, %d, %d] (%d dims), expected [cout][cin][k <= %d]", p.c_str(),
                    (int)w->ne[0], (int)w->ne[1], (int)w->ne[2], w->n_dims, DVAE_MAX_K);
      c.k = (int)w->ne[0]; c.cin = (int)w->ne[1]; c.cout = (int)w->ne[2];
      if (c.k % 2 == 0) return fail(ctx, TTS_ERR_FORMAT, "DVAE model file: '%s.weight' has %d taps (an odd kernel size, padding (k - 1) / 2)", p.c_str(), c.k);
      if (want_cin && c.cin != want_cin)
        return fail(ctx, TTS_ERR_FORMAT, "tensor '%s.weight' has wrong shape in DVAE model file: %d input channels, the layer before it writes %d", p.c_str(), c.cin, want_cin);
      const HostTensor *b = rd.peek(p + ".bias", 1);
      if (b && b->ne[0] != c.cout)
        return fail(ctx, TTS_ERR_FORMAT, "tensor '%s.bias' has wrong shape in DVAE model file: got %d values, expected %d", p.c_str(), (int)b->ne[0], c.cout);
    }
    return rd.conv(p, c.cout, c.cin, c.k, c);
  };
  while (wf.has(EN + std::to_string(h.L) + ".0.weight")) h.L++;
  if (h.L > DVAE_MAX_LAYERS) return fail(ctx, TTS_ERR_FORMAT, "DVAE model file: %d strided layers (at most %d)", h.L, DVAE_MAX_LAYERS);
  while (wf.has(EN + std::to_string(h.L + h.blocks) + ".net.0.weight")) h.blocks++;
  if (h.blocks > 64) return fail(ctx, TTS_ERR_FORMAT, "DVAE model file: %d ResBlocks (at most 64)", h.blocks);
  int rc;
  h.down.resize(h.L);
  for (int i = 0; i < h.L; i++) {
    if ((rc = conv(EN + std::to_string(i) + ".0", i ? h.down[i - 1].cout : 0, h.down[i]))) return rc;
    if (!dvae_channels_ok(h.down[i].cout))
      return fail(ctx, TTS_ERR_FORMAT, "DVAE model file: %d channels behind strided layer %d (a multiple of 64, 64 .. %d)", h.down[i].cout, i, DVAE_MAX_C);
  }
  h.cin = h.down[0].cin;
  if (h.cin > DVAE_MAX_CIN) return fail(ctx, TTS_ERR_FORMAT, "DVAE model file: %d mel channels (1 .. %d)", h.cin, DVAE_MAX_CIN);
  h.H = h.down[h.L - 1].cout;
  h.res.resize(h.blocks);
  for (int j = 0; j < h.blocks; j++) {
    const std::string p = EN + std::to_string(h.L + j) + ".net.";
    for (int q = 0; q < 3; q++) {
      if ((rc = conv(p + std::to_string(2 * q), h.H, h.res[j][q]))) return rc;
      if (h.res[j][q].cout != h.H)
        return fail(ctx, TTS_ERR_FORMAT, "tensor '%s%d.weight' has wrong shape in DVAE model file: %d output channels, the residual stream has %d", p.c_str(), 2 * q,
                    h.res[j][q].cout, h.H);
    }
  }
  if ((rc = conv(EN + std::to_string(h.L + h.blocks), h.H, h.head))) return rc;
  h.dim = h.head.cout;
  if (h.head.k != 1 || h.dim % 32 || h.dim > DVAE_MAX_DIM)
    return fail(ctx, TTS_ERR_FORMAT, "DVAE model file: the last convolution has %d taps and %d output channels (k 1; the codebook dim a multiple of 32, 32 .. %d)",
                h.head.k, h.dim, DVAE_MAX_DIM);
  {
    if (!rd.has(P + "codebook.embed")) return fail(ctx, TTS_ERR_FORMAT, "tensor 'dvae.codebook.embed' missing from DVAE model file");
    const HostTensor &t = *rd.peek(P + "codebook.embed");
    if (t.n_dims != 2 || t.ne[1] != h.dim || (int64_t)t.data.size() != t.nelem())
      return fail(ctx, TTS_ERR_FORMAT, "tensor 'dvae.codebook.embed' has wrong shape in DVAE model file: got [%d, %d] (%d dims), expected [%d][tokens]", (int)t.ne[1],
                  (int)t.ne[0], t.n_dims, h.dim);
    h.N = (int)t.ne[0];
    if (t.ne[0] < 32 || t.ne[0] % 32 || t.ne[0] > DVAE_MAX_TOKENS)
      return fail(ctx, TTS_ERR_FORMAT, "DVAE model file: %lld tokens (a multiple of 32, 32 .. %d)", (long long)t.ne[0], DVAE_MAX_TOKENS);
    for (float v : t.data)
      if (!std::isfinite(v)) return fail(ctx, TTS_ERR_FORMAT, "tensor 'dvae.codebook.embed' holds a non-finite value");
    h.E = t.data;
    h.e2.resize((size_t)h.N);
    dvae_code_norms(h.E.data(), h.dim, h.N, h.e2.data());
    rd.known++;
  }
  if (const HostTensor *t = rd.peek(P + "config")) { // what no shape holds: {stride}, an integer
    if (t->n_dims != 1 || t->ne[0] != 1 || t->data.size() != 1 || t->data[0] != (float)(int)t->data[0])
      return fail(ctx, TTS_ERR_FORMAT, "tensor 'dvae.config' has wrong shape in DVAE model file: {stride}, one integer");
    h.stride = (int)t->data[0];
    rd.known++;
  }
  if (h.stride < 1 || h.stride > DVAE_MAX_STRIDE) return fail(ctx, TTS_ERR_FORMAT, "DVAE model file: stride %d (1 .. %d)", h.stride, DVAE_MAX_STRIDE);
  return rd.finish(path);
}

struct DvaeConv : HfgLayer { int cin = 0, cout = 0, k = 0; };
struct DvaeState {
  int L = 0, blocks = 0, cin = 0, H = 0, dim = 0, N = 0, stride = 2;
  std::vector<DvaeConv> down;
  std::vector<std::array<DvaeConv, 3>> res;
  DvaeConv head;
  float *E = nullptr, *e2 = nullptr;
  DevWeights dev;
  DevBuf mel, tab, a, b, h, z, pv, pi, codes;
  LevelTable lt; // the layout dvae_begin made, for dvae_run (and the source of its asynchronous upload)
};
void dvae_free(DvaeState *s) { delete s; }

// The file is parsed before the device is asked for: a host-only context reports a broken file as TTS_ERR_FORMAT and a good one as TTS_ERR_HIP.
int dvae_load(tts_ctx *ctx, const char *path) {
  if (!path) return fail(ctx, TTS_ERR_ARG, "tts_load_dvae: bad argument");
  WeightFile wf;
  std::string err;
  int rc = read_weight_file(path, wf, err);
  if (rc != TTS_OK) return fail(ctx, rc, "dvae_load: %s", err.c_str());
  std::unique_ptr<DvaeHost> h(new DvaeHost());
  if ((rc = dvae_parse(ctx, wf, path, *h))) return rc;
  if (ctx->device < 0) return fail(ctx, TTS_ERR_HIP, "host-only context: no HIP device, no CPU fallback");
  (void)hipSetDevice(ctx->device);
  std::unique_ptr<DvaeState> st(new DvaeState());
  st->L = h->L; st->blocks = h->blocks; st->cin = h->cin; st->H = h->H; st->dim = h->dim; st->N = h->N; st->stride = h->stride;
  auto layer = [&](const DvaeHostConv &s, DvaeConv &d) -> int {
    d.cin = s.cin; d.cout = s.cout; d.k = s.k;
    return st->dev.up(ctx, s, d);
  };
  st->down.resize(h->L); st->res.resize(h->blocks);
  for (int i = 0; i < h->L; i++)
    if ((rc = layer(h->down[i], st->down[i]))) return rc;
  for (int j = 0; j < h->blocks; j++)
    for (int q = 0; q < 3; q++)
      if ((rc = layer(h->res[j][q], st->res[j][q]))) return rc;
  if ((rc = layer(h->head, st->head)) || (rc = st->dev.up(ctx, h->E, &st->E)) || (rc = st->dev.up(ctx, h->e2, &st->e2))) return rc;
  if (ctx->dvae) dvae_free(ctx->dvae);
  ctx->dvae = st.release();
  return TTS_OK;
}

int dvae_tokens(const tts_ctx *ctx) { return ctx && ctx->dvae ? ctx->dvae->N : 0; }
int dvae_dim(const tts_ctx *ctx) { return ctx && ctx->dvae ? ctx->dvae->dim : 0; }

// tts_dvae_codes in two halves, as cvvp_voice_begin / cvvp_voice_run: every check and the layout, then (once the mel buffer is filled: an upload in dvae_codes, the
// audio front end's kernels in tts_dvae_codes_audio) one launch sequence for the whole ragged batch and one download. Nothing of it depends on the batch: a clip's
// codes and z are the same bits alone or in any batch. The stage owns its buffers and touches no AR or diffusion state, so it is legal while sessions are open.
int dvae_begin(tts_ctx *ctx, const char *fn, const int32_t *frames, int n_clips, int code_stride, float **d_mel) {
  DvaeState *st = ctx->dvae;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_dvae not called");
  if (!frames || n_clips < 1 || code_stride < 1 || !d_mel) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", fn);
  if (n_clips > DVAE_MAX_CLIPS) return fail(ctx, TTS_ERR_LIMIT, "%s: %d clips (at most %d per call)", fn, n_clips, DVAE_MAX_CLIPS);
  const int B = n_clips, L = st->L;
  for (int s = 0; s < B; s++) {
    if (frames[s] < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %d mel frames (at least 1 expected)", fn, s, frames[s]);
    if (frames[s] > DVAE_MAX_FRAMES) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %d mel frames, at most %d", fn, s, frames[s], DVAE_MAX_FRAMES);
    int n = frames[s];
    for (int l = 0; l < L; l++) n = dvae_conv_rows(n, st->stride);
    if (n > code_stride) return fail(ctx, TTS_ERR_ARG, "%s: clip %d has %d codes, code_stride is %d", fn, s, n, code_stride);
  }
  LevelTable lt = dvae_levels(frames, B, L, st->stride, st->cin);
  const std::vector<int64_t> &total = lt.rows;
  const int64_t R = total[L], moff = (int64_t)st->cin * total[0];
  size_t act = (size_t)R * st->H; // a and b: the strided layers before the last write them in turn, then the ResBlocks' two intermediate tensors
  for (int i = 0; i + 1 < L; i++) act = std::max(act, (size_t)total[i + 1] * st->down[i].cout);
  const int slabs = dvae_vq_slabs(st->N);
  TTS_HIP(ctx, st->mel.reserve((size_t)moff * 4));
  TTS_HIP(ctx, st->tab.reserve(lt.tab.size() * 4));
  TTS_HIP(ctx, st->a.reserve(act * 4));
  TTS_HIP(ctx, st->b.reserve(act * 4));
  TTS_HIP(ctx, st->h.reserve((size_t)R * st->H * 4));
  TTS_HIP(ctx, st->z.reserve((size_t)R * st->dim * 4));
  TTS_HIP(ctx, st->pv.reserve((size_t)slabs * R * 4));
  TTS_HIP(ctx, st->pi.reserve((size_t)slabs * R * 4));
  TTS_HIP(ctx, st->codes.reserve((size_t)R * 4));
  st->lt = std::move(lt); // outlives this call: the copy is asynchronous
  TTS_HIP(ctx, hipMemcpyAsync(st->tab.p, st->lt.tab.data(), st->lt.tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  *d_mel = st->mel.as<float>();
  return TTS_OK;
}

// codes_out [B][code_stride], z_out null or [B][code_stride][dim]: the first n_codes_out[s] entries of a clip are written, the rest is left alone.
int dvae_run(tts_ctx *ctx, int32_t *codes_out, int32_t *n_codes_out, int code_stride, float *z_out) {
  DvaeState *st = ctx->dvae;
  const int B = st->lt.B, L = st->L, D = st->dim;
  const std::vector<int> &max_n = st->lt.max_n;
  const std::vector<int64_t> &total = st->lt.rows;
  const int64_t R = total[L];
  hipStream_t sm = ctx->stream;
  const int *d_tab = st->tab.as<int>();
  auto seq = [&](int l) { return d_tab + (size_t)l * B * HFG_SEQ; };
  float *a = st->a.as<float>(), *b = st->b.as<float>(), *h = st->h.as<float>(), *z = st->z.as<float>();
  // the strided layers write a, b, a, .. and the last one h
  auto dst = [&](int i) { return i == L - 1 ? h : (i % 2 ? b : a); };
  {
    const DvaeConv &c = st->down[0];
    DvaeStem p{};
    p.mel = st->mel.as<float>(); p.out = dst(0); p.w = c.w; p.bias = c.b; p.seq_in = seq(0); p.seq_out = seq(1);
    p.cin = c.cin; p.cout = c.cout; p.taps = c.k; p.stride = st->stride; p.pad = (c.k - 1) / 2;
    ProfScope ps(ctx, "dvae_conv", 2.0 * (double)total[1] * c.k * c.cin * c.cout);
    dvae_launch_stem(p, max_n[1], B, sm);
  }
  for (int i = 1; i < L; i++) {
    const DvaeConv &c = st->down[i];
    ClsDown d{};
    d.in = dst(i - 1); d.out = dst(i); d.w = c.w; d.bias = c.b; d.seq_in = seq(i); d.seq_out = seq(i + 1);
    d.cin = c.cin; d.cout = c.cout; d.taps = c.k; d.stride = st->stride; d.pad = (c.k - 1) / 2;
    ProfScope ps(ctx, "dvae_conv", 2.0 * (double)total[i + 1] * c.k * c.cin * c.cout);
    dvae_launch_down(d, seq(i + 1), max_n[i + 1], B, sm);
  }
  auto conv = [&](const float *in, float *out, const float *resid, const DvaeConv &c, float slope) {
    ProfScope ps(ctx, "dvae_conv", 2.0 * (double)R * c.k * c.cin * c.cout);
    dvae_launch_conv(in, out, resid, c.w, c.b, seq(L), c.cin, c.cout, c.k, slope, max_n[L], B, sm);
  };
  for (const auto &r : st->res) {
    conv(h, a, nullptr, r[0], 1.0f); // no activation on a block's input
    conv(a, b, nullptr, r[1], 0.0f);
    conv(b, h, h, r[2], 0.0f);       // the skip in the epilogue: an element is read and written by the same thread
  }
  conv(h, z, nullptr, st->head, 1.0f);
  {
    DvaeVq q{};
    q.z = z; q.E = st->E; q.e2 = st->e2; q.pv = st->pv.as<float>(); q.pi = st->pi.as<int>(); q.R = (int)R; q.D = D; q.N = st->N;
    ProfScope ps(ctx, "dvae_vq", 2.0 * (double)R * D * st->N);
    TTS_HIP(ctx, dvae_launch_vq(q, st->codes.as<int>(), nullptr, sm));
  }
  TTS_HIP(ctx, hipGetLastError());
  std::vector<int32_t> codes((size_t)R);
  std::vector<float> zh(z_out ? (size_t)R * D : 0);
  TTS_HIP(ctx, hipMemcpyAsync(codes.data(), st->codes.p, codes.size() * 4, hipMemcpyDeviceToHost, sm));
  if (z_out) TTS_HIP(ctx, hipMemcpyAsync(zh.data(), z, zh.size() * 4, hipMemcpyDeviceToHost, sm));
  TTS_HIP(ctx, hipStreamSynchronize(sm));
  for (int s = 0; s < B; s++) {
    const size_t f0 = (size_t)st->lt.rec(L, s)[0];
    const int n = st->lt.rec(L, s)[1];
    n_codes_out[s] = n;
    memcpy(codes_out + (size_t)s * code_stride, &codes[f0], (size_t)n * 4);
    if (z_out) memcpy(z_out + (size_t)s * code_stride * D, &zh[f0 * D], (size_t)n * D * 4);
  }
  return TTS_OK;
}

int dvae_codes(tts_ctx *ctx, const float *mel, const int32_t *frames, int n_clips, int32_t *codes_out, int32_t *n_codes_out, int code_stride, float *z_out) {
  const char *fn = "tts_dvae_codes";
  DvaeState *st = ctx->dvae;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_dvae not called");
  if (!mel || !frames || !codes_out || !n_codes_out || n_clips < 1 || code_stride < 1) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", fn);
  if (n_clips > DVAE_MAX_CLIPS) return fail(ctx, TTS_ERR_LIMIT, "%s: %d clips (at most %d per call)", fn, n_clips, DVAE_MAX_CLIPS);
  int64_t total = 0;
  for (int s = 0; s < n_clips; s++) {
    if (frames[s] < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %d mel frames (at least 1 expected)", fn, s, frames[s]);
    if (frames[s] > DVAE_MAX_FRAMES) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %d mel frames, at most %d", fn, s, frames[s], DVAE_MAX_FRAMES);
    total += (int64_t)st->cin * frames[s];
  }
  for (int64_t i = 0; i < total; i++)
    if (!std::isfinite(mel[i])) return fail(ctx, TTS_ERR_ARG, "%s: the mel holds a non-finite value (float %lld)", fn, (long long)i);
  float *d_mel = nullptr;
  const int rc = dvae_begin(ctx, fn, frames, n_clips, code_stride, &d_mel);
  if (rc) return rc;
  TTS_HIP(ctx, hipMemcpyAsync(d_mel, mel, (size_t)total * 4, hipMemcpyHostToDevice, ctx->stream));
  return dvae_run(ctx, codes_out, n_codes_out, code_stride, z_out);
}

// what tts_dvae_codes_audio needs to know before the front end runs: the loaded model's mel channels (80 for every model the front end can feed), or 0
int dvae_mel_channels(const tts_ctx *ctx) { return ctx && ctx->dvae ? ctx->dvae->cin : 0; }

} // namespace tts
