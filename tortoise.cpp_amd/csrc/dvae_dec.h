// The DVAE decoder on MI355X (gfx950): speech codes -> the 80-band mel, and the reconstruction error of a recording's codes
//   tts_load_dvae_decoder / tts_dvae_decode / tts_dvae_reconstruct / tts_dvae_reconstruct_audio
//
// Included once, behind dvae.h (hifigan.hip's translation unit): DiscreteVAE.decode of upstream tortoise-tts with use_transposed_convs=False and no
// normalisation. Upstream's source and weights are not available offline: the contract is the arithmetic below ("What pins the DVAE decoder"),
// checked against a float64 statement (tests/dvae_dec_ref.py); unpinned against upstream. f32 throughout.
//
//   e = E[:, code[t]];  h = Conv1d(dim -> H, k 1)(e)                                        dvae_embed_kernel (the gather is the MFMA's A operand: e is never stored)
//   blocks x:  h = h + Conv1(ReLU(Conv3(ReLU(Conv3(h)))))                                   hfg_conv_kernel, as the encoder
//   layer i = 0 .. L - 1:  h = ReLU(Conv1d(C_i -> C_{i+1}, k, pad (k - 1) / 2)(nearest_upsample(h, s)))   dvae_up_kernel (the s-times-longer tensor is never stored)
//   mel = Conv1d(C_L -> channels, k 1)(h)                                                   dvae_head_kernel (writes band-major [channels][T'], what dvae_stem_kernel reads)
//   L1 = mean |mel - recon|, MSE = mean (mel - recon)^2 over min(T, T') frames              dvae_err_kernel + dvae_err_reduce_kernel (double, fixed order)
//
// THE FOLD. Output row t = s q + p (phase p) and tap j read the up-sampled row t - pad + j, which is input row q + floor((p - pad + j) / s), or zero outside
// [0, s n): exactly when q + floor(..) is outside [0, n). So per phase the k taps fall on ne_p <= (k - 1) / s + 2 input rows, offsets dlo_p .. dlo_p + ne_p - 1,
// and taps that share a row share their operand: the loader sums their weights (in double, rounded once) into one [cin][cout] slot per (phase, offset). k 3 / s 2
// multiplies 4 slots for 2 output rows where the up-sampled convolution multiplies 6; k 7 / s 4: 10 for 28. Stride 1 is the plain convolution, nothing summed.
//
// Device layout and rules: dvae.h's. Time-major f32 rows [row][channels]; level l holds n s^l rows per clip, the clips packed without gaps; no kernel reads or
// writes a row outside the clip it works on, none uses atomics: two runs agree bit for bit and a clip alone gives the bits of the clip in a batch. The sizes
// dvae_dec_parse accepts are dvae.h's: channel counts multiples of 64 up to 4096, odd kernel sizes up to 7, stride 1 .. 4, 1 .. 128 mel channels, codebook dim a
// multiple of 32 up to 512, tokens a multiple of 32 up to 65536.
#pragma once

namespace tts {

namespace {
constexpr int DVD_ROWS = 128;  // rows of a workgroup of all three MFMA kernels: 4 waves x one 32-row tile (codes; input rows; frames)
constexpr int DVD_ERR_T = 64;  // frames of a dvae_err_kernel tile

struct DvdEmbed {
  const int *codes;  // [R]
  const float *Et;   // [N][D]: the codebook transposed by the loader, a code's row contiguous
  const float *w;    // [D][H]
  const float *bias; // [H]
  float *out;        // [R][H]
  int R, D, H, N;
};

// h[t][c] = b[c] + sum_k E[k][code[t]] w[k][c] on the f32-input MFMA. One wave: 32 codes x 32 NT output channels; lane (row lr, half lk) reads its code's codebook
// row straight into the A operand, a float4 per 8 channels (half 0: channels k0 .. k0 + 3, half 1: k0 + 4 .. k0 + 7), so MFMA j of a step adds channels k0 + j and
// k0 + 4 + j: a fixed order, steps ascending. The weights are read in fragment order as hfg_conv_kernel reads them. No LDS, no barrier. The rows are independent
// of their clips: the launch tiles all R rows of the batch. A code outside 0 .. N - 1 is refused on the host; the clamp keeps the read inside the codebook whatever arrives.
template <int NT>
__global__ __launch_bounds__(256) void dvae_embed_kernel(const DvdEmbed a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int r0 = blockIdx.x * DVD_ROWS + wave * 32, n0 = blockIdx.y * 32 * NT;
  if (r0 >= a.R) return;
  const int code = min(max(a.codes[min(r0 + lr, a.R - 1)], 0), a.N - 1);
  const float *er = a.Et + (size_t)code * a.D + 4 * lk;
  const float *wr = a.w + (size_t)(4 * lk) * a.H + n0 + lr;
  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; n++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[n][r] = 0.f;
  for (int k0 = 0; k0 < a.D; k0 += 8) { // D is a multiple of 32
    const float4 e = *(const float4 *)(er + k0);
    const float ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int n = 0; n < NT; n++) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(ev[j], wr[(size_t)(k0 + j) * a.H + n * 32], acc[n], 0, 0, 0);
  }
#pragma unroll
  for (int n = 0; n < NT; n++) {
    const int col = n0 + n * 32 + lr;
    const float bv = a.bias[col];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int t = r0 + 8 * (r >> 2) + 4 * lk + (r & 3);
      if (t < a.R) a.out[(size_t)t * a.H + col] = acc[n][r] + bv;
    }
  }
}

struct DvdUp {
  const float *in;   // [rows_in][cin]
  float *out;        // [rows_in * S][cout]; never `in`
  const float *w;    // [slot][cin][cout]: the folded weights, phase by phase, offsets ascending
  const float *bias; // [cout]
  const int *seq_in, *seq_out;
  int cin, cout;
  int dmin, nd;               // the input rows any phase reads for input row q: q + dmin .. q + dmin + nd - 1
  int dlo[4], ne[4], slot[4]; // of phase p: its first offset, its offsets, its first weight slot
};
inline size_t dvae_up_lds(int nd) { return (size_t)(DVD_ROWS + nd - 1) * 33 * 4; }

// One workgroup: 128 input rows of one clip -> their 128 S output rows x 64 output channels. Wave w owns input rows 32 w .. 32 w + 31 and ALL S phases of them:
// S x 2 accumulator tiles (S = 4: 128 registers), so the window of input rows (128 + nd - 1 rows, 32 channels at a time, 33-float rows as hfg_conv_kernel's) is
// staged through LDS once per channel chunk and serves every tap of every phase. Per output element: chunks ascending, offsets ascending, channel pairs
// ascending on the MFMA (lane half lk holds channel c0 + k + lk); then the bias, then the ReLU. Rows outside the clip are staged as zeros: the convolution's
// padding, which the fold keeps on whole input rows. A wave whose 32 rows lie past the clip's end stages and waits but multiplies nothing.
template <int S>
__global__ __launch_bounds__(256) void dvae_up_kernel(const DvdUp a) {
  extern __shared__ float sx[];
  const int s = blockIdx.y;
  const int fi = a.seq_in[HFG_SEQ * s], n = a.seq_in[HFG_SEQ * s + 1], fo = a.seq_out[HFG_SEQ * s];
  const int q0 = blockIdx.x * DVD_ROWS;
  if (q0 >= n) return;
  const int n0 = blockIdx.z * 64, win = DVD_ROWS + a.nd - 1;
  const float *in = a.in + (size_t)fi * a.cin;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const bool live = q0 + wave * 32 < n;
  f32x16 acc[S][2];
#pragma unroll
  for (int p = 0; p < S; p++)
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[p][m][r] = 0.f;
  for (int c0 = 0; c0 < a.cin; c0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < win * 8; idx += 256) {
      const int r = idx >> 3, q = (idx & 7) * 4, t = q0 + a.dmin + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t >= 0 && t < n) v = *(const float4 *)(in + (size_t)t * a.cin + c0 + q);
      float *d = sx + r * 33 + q;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    if (live)
      for (int d = 0; d < a.nd; d++) {
        const float *xr = sx + (wave * 32 + lr + d) * 33 + lk;
#pragma unroll
        for (int p = 0; p < S; p++) {
          const int e = a.dmin + d - a.dlo[p];
          if (e < 0 || e >= a.ne[p]) continue; // uniform: phase p has no tap on this input row
          const float *wr = a.w + ((size_t)(a.slot[p] + e) * a.cin + c0 + lk) * a.cout + n0 + lr;
#pragma unroll 4
          for (int k = 0; k < 32; k += 2) {
            const float av = xr[k];
            acc[p][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wr[(size_t)k * a.cout], acc[p][0], 0, 0, 0);
            acc[p][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wr[(size_t)k * a.cout + 32], acc[p][1], 0, 0, 0);
          }
        }
      }
  }
  if (!live) return;
#pragma unroll
  for (int p = 0; p < S; p++)
#pragma unroll
    for (int m = 0; m < 2; m++) {
      const int col = n0 + m * 32 + lr;
      const float bv = a.bias[col];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int q = q0 + wave * 32 + 8 * (r >> 2) + 4 * lk + (r & 3);
        if (q < n) a.out[((size_t)fo + (size_t)q * S + p) * a.cout + col] = fmaxf(acc[p][m][r] + bv, 0.f);
      }
    }
}

struct DvdHead {
  const float *in;   // [rows][cin]
  const float *w;    // [cin][coutp]: the bands padded with zeros to a multiple of 32
  const float *bias; // [coutp]
  float *mel;        // clip s band-major [cout][T] at float cout x (the clip's first row)
  const int *seq;
  int cin, cout, coutp;
};

// mel[band][t] = b[band] + sum_c w[c][band] h[t][c], the product TRANSPOSED: the 32 bands of a tile are the MFMA's rows (A = the weights, fragment order), the
// wave's 32 frames its columns (B = the activations, a float4 of the lane's own row per 8 channels, dvae_embed_kernel's channel order), so a C/D register holds 32
// consecutive frames of one band and the band-major store is one 128-byte line. One wave: 32 frames x 32 bands; blockIdx.z walks the band tiles. No LDS.
__global__ __launch_bounds__(256) void dvae_head_kernel(const DvdHead a) {
  const int s = blockIdx.y;
  const int f0 = a.seq[HFG_SEQ * s], T = a.seq[HFG_SEQ * s + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lk = lane >> 5;
  const int t0 = blockIdx.x * DVD_ROWS + wave * 32, m0 = blockIdx.z * 32;
  if (t0 >= T) return;
  const float *xr = a.in + ((size_t)f0 + min(t0 + lr, T - 1)) * a.cin + 4 * lk;
  const float *wr = a.w + (size_t)(4 * lk) * a.coutp + m0 + lr;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  for (int k0 = 0; k0 < a.cin; k0 += 8) { // cin is a multiple of 64
    const float4 x = *(const float4 *)(xr + k0);
    const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[(size_t)(k0 + j) * a.coutp], xv[j], acc, 0, 0, 0);
  }
  float *mel = a.mel + (size_t)f0 * a.cout;
  const int t = t0 + lr;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int band = m0 + 8 * (r >> 2) + 4 * lk + (r & 3);
    if (band < a.cout && t < T) mel[(size_t)band * T + t] = acc[r] + a.bias[band];
  }
}

// part[s][tile] = (sum |mel - rec|, sum (mel - rec)^2) over all bands of the tile's 64 frames, the first min(T, T') frames of clip s: the difference in f32 (both
// are f32 values), |d| and d d (exact in double) added in double. A thread adds its elements in ascending order, then a fixed tree over the 256 threads.
__global__ __launch_bounds__(256) void dvae_err_kernel(const float *__restrict__ mel, const float *__restrict__ rec, const int *__restrict__ seq_mel,
                                                       const int *__restrict__ seq_rec, int bands, int max_tiles, double2 *__restrict__ part) {
  __shared__ double2 red[256];
  const int s = blockIdx.y;
  const int T = seq_mel[HFG_SEQ * s + 1], Tr = seq_rec[HFG_SEQ * s + 1], m = min(T, Tr);
  const int t0 = blockIdx.x * DVD_ERR_T;
  if (t0 >= m) return;
  const float *x = mel + (size_t)seq_mel[HFG_SEQ * s + 4], *y = rec + (size_t)seq_rec[HFG_SEQ * s] * bands;
  double l1 = 0.0, l2 = 0.0;
  for (int idx = threadIdx.x; idx < bands * DVD_ERR_T; idx += 256) {
    const int b = idx / DVD_ERR_T, t = t0 + idx % DVD_ERR_T;
    if (t < m) {
      const float d = x[(size_t)b * T + t] - y[(size_t)b * Tr + t];
      l1 += (double)fabsf(d); l2 += (double)d * (double)d;
    }
  }
  red[threadIdx.x] = make_double2(l1, l2);
  __syncthreads();
  for (int w = 128; w; w >>= 1) {
    if ((int)threadIdx.x < w) { red[threadIdx.x].x += red[threadIdx.x + w].x; red[threadIdx.x].y += red[threadIdx.x + w].y; }
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)s * max_tiles + blockIdx.x] = red[0];
}
// out[s] = (mean |d|, mean d^2): the tiles of clip s ascending, in double; one thread per clip
__global__ __launch_bounds__(64) void dvae_err_reduce_kernel(const double2 *__restrict__ part, const int *__restrict__ seq_mel, const int *__restrict__ seq_rec,
                                                             int bands, int max_tiles, int B, double2 *__restrict__ out) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= B) return;
  const int m = min(seq_mel[HFG_SEQ * s + 1], seq_rec[HFG_SEQ * s + 1]), tiles = (m + DVD_ERR_T - 1) / DVD_ERR_T;
  double l1 = 0.0, l2 = 0.0;
  for (int i = 0; i < tiles; i++) { const double2 v = part[(size_t)s * max_tiles + i]; l1 += v.x; l2 += v.y; }
  const double cnt = (double)m * (double)bands;
  out[s] = make_double2(l1 / cnt, l2 / cnt);
}

// ---- the launches ----
void dvae_launch_embed(const DvdEmbed &a, hipStream_t st) {
  const unsigned gx = (unsigned)((a.R + DVD_ROWS - 1) / DVD_ROWS);
  if (a.H % 128 == 0) dvae_embed_kernel<4><<<dim3(gx, (unsigned)(a.H / 128)), 256, 0, st>>>(a);
  else dvae_embed_kernel<2><<<dim3(gx, (unsigned)(a.H / 64)), 256, 0, st>>>(a);
}
void dvae_launch_up(const DvdUp &a, int stride, int max_in, int B, hipStream_t st) {
  const dim3 grid((unsigned)((max_in + DVD_ROWS - 1) / DVD_ROWS), (unsigned)B, (unsigned)(a.cout / 64));
  const size_t lds = dvae_up_lds(a.nd);
  switch (stride) {
    case 1: dvae_up_kernel<1><<<grid, 256, lds, st>>>(a); break;
    case 2: dvae_up_kernel<2><<<grid, 256, lds, st>>>(a); break;
    case 3: dvae_up_kernel<3><<<grid, 256, lds, st>>>(a); break;
    default: dvae_up_kernel<4><<<grid, 256, lds, st>>>(a); break;
  }
}
void dvae_launch_head(const DvdHead &a, int max_t, int B, hipStream_t st) {
  dvae_head_kernel<<<dim3((unsigned)((max_t + DVD_ROWS - 1) / DVD_ROWS), (unsigned)B, (unsigned)(a.coutp / 32)), 256, 0, st>>>(a);
}
inline int dvd_floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
} // namespace

// The model as the loader's host half leaves it (no device call)
struct DvdHostUp : DvaeHostConv { // w: the folded slots [slot][cin][cout]
  int dmin = 0, nd = 0, dlo[4] = {0, 0, 0, 0}, ne[4] = {0, 0, 0, 0}, slot[4] = {0, 0, 0, 0}, slots = 0;
};
struct DvaeDecHost {
  int L = 0, blocks = 0, H = 0, dim = 0, N = 0, stride = 2, channels = 0, coutp = 0;
  DvaeHostConv in;                              // dim -> H, k 1
  std::vector<std::array<DvaeHostConv, 3>> res; // net.0, net.2, net.4
  std::vector<DvdHostUp> up;
  DvaeHostConv head;                            // C_L -> channels, k 1, the bands padded to coutp
  std::vector<float> Et;                        // [N][dim]
};

// w [k][cin][cout] -> the slots of every phase (THE FOLD above): the taps of a slot summed in double, taps ascending, and rounded once
void dvae_dec_fold(DvdHostUp &u, int stride) {
  const int pad = (u.k - 1) / 2;
  const size_t per = (size_t)u.cin * u.cout;
  std::vector<float> folded;
  std::vector<double> sum(per);
  u.dmin = dvd_floordiv(-pad, stride);
  u.nd = dvd_floordiv(stride - 1 - pad + u.k - 1, stride) - u.dmin + 1;
  u.slots = 0;
  for (int p = 0; p < stride; p++) {
    u.dlo[p] = dvd_floordiv(p - pad, stride);
    u.ne[p] = dvd_floordiv(p - pad + u.k - 1, stride) - u.dlo[p] + 1;
    u.slot[p] = u.slots;
    for (int e = 0; e < u.ne[p]; e++) {
      std::fill(sum.begin(), sum.end(), 0.0);
      for (int j = 0; j < u.k; j++)
        if (dvd_floordiv(p - pad + j, stride) == u.dlo[p] + e)
          for (size_t i = 0; i < per; i++) sum[i] += (double)u.w[(size_t)j * per + i];
      for (size_t i = 0; i < per; i++) folded.push_back((float)sum[i]);
    }
    u.slots += u.ne[p];
  }
  u.w.swap(folded);
}

int dvae_dec_parse(tts_ctx *ctx, const WeightFile &wf, const char *path, DvaeDecHost &h) {
  const std::string P = "dvae.", DN = P + "decoder.";
  if (!wf.has(DN + "0.weight")) return fail(ctx, TTS_ERR_FORMAT, "'%s' is not a DVAE decoder model file", path);
  ModelReader rd{wf, ctx, "DVAE decoder"};
  // Conv1d [cout][cin][k] -> [k][cin][coutp]: the sizes are the tensor's own (dvae_parse's reader)
  auto conv = [&](const std::string &p, int want_cin, DvaeHostConv &c, bool pad_out = false) -> int {
    if (const HostTensor *w = rd.peek(p + ".weight")) {
      if (w->n_dims != 3 || w->ne[0] < 1 || w->ne[1] < 1 || w->ne[2] < 1 || w->ne[0] > DVAE_MAX_K || w->ne[1] > DVAE_MAX_C || w->ne[2] > DVAE_MAX_C)
        return fail(ctx, TTS_ERR_FORMAT, "tensor '%s.weight' has wrong shape in DVAE decoder model file: got [%d, %d, %d] (%d dims), expected [cout][cin][k <= %d]",
                    p.c_str(), (int)w->ne[0], (int)w->ne[1], (int)w->ne[2], w->n_dims, DVAE_MAX_K);
      c.k = (int)w->ne[0]; c.cin = (int)w->ne[1]; c.cout = (int)w->ne[2];
      if (c.k % 2 == 0) return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: '%s.weight' has %d taps (an odd kernel size, padding (k - 1) / 2)", p.c_str(), c.k);
      if (want_cin && c.cin != want_cin)
        return fail(ctx, TTS_ERR_FORMAT, "tensor '%s.weight' has wrong shape in DVAE decoder model file: %d input channels, the layer before it writes %d", p.c_str(),
                    c.cin, want_cin);
      const HostTensor *b = rd.peek(p + ".bias", 1);
      if (b && b->ne[0] != c.cout)
        return fail(ctx, TTS_ERR_FORMAT, "tensor '%s.bias' has wrong shape in DVAE decoder model file: got %d values, expected %d", p.c_str(), (int)b->ne[0], c.cout);
    }
    return rd.conv(p, c.cout, c.cin, c.k, c, pad_out ? (c.cout + 31) / 32 * 32 : 0);
  };
  while (wf.has(DN + std::to_string(1 + h.blocks) + ".net.0.weight")) h.blocks++;
  if (h.blocks > 64) return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: %d ResBlocks (at most 64)", h.blocks);
  const int first = 1 + h.blocks;
  while (wf.has(DN + std::to_string(first + h.L) + ".0.conv.weight")) h.L++;
  if (wf.has(DN + std::to_string(first + h.L) + ".0.weight"))
    return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: '%s%d.0.weight' is a transposed convolution (use_transposed_convs=True); only the nearest up-sample + "
                "Conv1d decoder is supported", DN.c_str(), first + h.L);
  if (h.L < 1 || h.L > DVAE_MAX_LAYERS) return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: %d up-sampling layers (1 .. %d)", h.L, DVAE_MAX_LAYERS);
  int rc;
  if ((rc = conv(DN + "0", 0, h.in))) return rc;
  h.dim = h.in.cin; h.H = h.in.cout;
  if (h.in.k != 1 || h.dim % 32 || h.dim > DVAE_MAX_DIM)
    return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: the first convolution has %d taps and %d input channels (k 1; the codebook dim a multiple of 32, 32 .. %d)",
                h.in.k, h.dim, DVAE_MAX_DIM);
  if (!dvae_channels_ok(h.H)) return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: %d channels behind the first convolution (a multiple of 64, 64 .. %d)", h.H, DVAE_MAX_C);
  h.res.resize(h.blocks);
  for (int j = 0; j < h.blocks; j++) {
    const std::string p = DN + std::to_string(1 + j) + ".net.";
    for (int q = 0; q < 3; q++) {
      if ((rc = conv(p + std::to_string(2 * q), h.H, h.res[j][q]))) return rc;
      if (h.res[j][q].cout != h.H)
        return fail(ctx, TTS_ERR_FORMAT, "tensor '%s%d.weight' has wrong shape in DVAE decoder model file: %d output channels, the residual stream has %d", p.c_str(),
                    2 * q, h.res[j][q].cout, h.H);
    }
  }
  h.up.resize(h.L);
  for (int i = 0; i < h.L; i++) {
    if ((rc = conv(DN + std::to_string(first + i) + ".0.conv", i ? h.up[i - 1].cout : h.H, h.up[i]))) return rc;
    if (!dvae_channels_ok(h.up[i].cout))
      return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: %d channels behind up-sampling layer %d (a multiple of 64, 64 .. %d)", h.up[i].cout, i, DVAE_MAX_C);
  }
  if ((rc = conv(DN + std::to_string(first + h.L), h.up[h.L - 1].cout, h.head, true))) return rc;
  h.channels = h.head.cout; h.coutp = (h.channels + 31) / 32 * 32;
  if (h.head.k != 1 || h.channels > DVAE_MAX_CIN)
    return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: the last convolution has %d taps and %d output channels (k 1; 1 .. %d mel channels)", h.head.k, h.channels,
                DVAE_MAX_CIN);
  {
    if (!rd.has(P + "codebook.embed")) return fail(ctx, TTS_ERR_FORMAT, "tensor 'dvae.codebook.embed' missing from DVAE decoder model file");
    const HostTensor &t = *rd.peek(P + "codebook.embed");
    if (t.n_dims != 2 || t.ne[1] != h.dim || (int64_t)t.data.size() != t.nelem())
      return fail(ctx, TTS_ERR_FORMAT, "tensor 'dvae.codebook.embed' has wrong shape in DVAE decoder model file: got [%d, %d] (%d dims), expected [%d][tokens]",
                  (int)t.ne[1], (int)t.ne[0], t.n_dims, h.dim);
    if (t.ne[0] < 32 || t.ne[0] % 32 || t.ne[0] > DVAE_MAX_TOKENS)
      return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: %lld tokens (a multiple of 32, 32 .. %d)", (long long)t.ne[0], DVAE_MAX_TOKENS);
    h.N = (int)t.ne[0];
    for (float v : t.data)
      if (!std::isfinite(v)) return fail(ctx, TTS_ERR_FORMAT, "tensor 'dvae.codebook.embed' holds a non-finite value");
    h.Et.resize(t.data.size());
    for (int k = 0; k < h.dim; k++)
      for (int j = 0; j < h.N; j++) h.Et[(size_t)j * h.dim + k] = t.data[(size_t)k * h.N + j];
    rd.known++;
  }
  if (const HostTensor *t = rd.peek(P + "config")) { // what no shape holds: {the up-sampling factor}, an integer
    if (t->n_dims != 1 || t->ne[0] != 1 || t->data.size() != 1 || t->data[0] != (float)(int)t->data[0])
      return fail(ctx, TTS_ERR_FORMAT, "tensor 'dvae.config' has wrong shape in DVAE decoder model file: {stride}, one integer");
    h.stride = (int)t->data[0];
    rd.known++;
  }
  if (h.stride < 1 || h.stride > DVAE_MAX_STRIDE) return fail(ctx, TTS_ERR_FORMAT, "DVAE decoder model file: stride %d (1 .. %d)", h.stride, DVAE_MAX_STRIDE);
  if ((rc = rd.finish(path))) return rc;
  for (DvdHostUp &u : h.up) dvae_dec_fold(u, h.stride);
  return TTS_OK;
}

struct DvdUpLayer : DvaeConv { DvdHostUp geo; }; // geo: the fold's tables (its weight vector left empty)
struct DvaeDecState {
  int L = 0, blocks = 0, H = 0, dim = 0, N = 0, stride = 2, channels = 0, coutp = 0;
  DvaeConv in, head;
  std::vector<std::array<DvaeConv, 3>> res;
  std::vector<DvdUpLayer> up;
  float *Et = nullptr;
  DevWeights dev;
  DevBuf in_buf, a, b, h, mel, part, err;
  LevelTable lt;            // level l: n s^l rows per clip
  std::vector<int> staging; // the tables | the codes: the source of dvae_dec_begin's asynchronous upload
  int64_t frames_of(int64_t n) const { for (int l = 0; l < L; l++) n *= stride; return n; }
};
void dvae_dec_free(DvaeDecState *s) { delete s; }

int dvae_dec_load(tts_ctx *ctx, const char *path) {
  if (!path) return fail(ctx, TTS_ERR_ARG, "tts_load_dvae_decoder: bad argument");
  WeightFile wf;
  std::string err;
  int rc = read_weight_file(path, wf, err);
  if (rc != TTS_OK) return fail(ctx, rc, "dvae_dec_load: %s", err.c_str());
  std::unique_ptr<DvaeDecHost> h(new DvaeDecHost());
  if ((rc = dvae_dec_parse(ctx, wf, path, *h))) return rc;
  if (ctx->device < 0) return fail(ctx, TTS_ERR_HIP, "host-only context: no HIP device, no CPU fallback");
  (void)hipSetDevice(ctx->device);
  std::unique_ptr<DvaeDecState> st(new DvaeDecState());
  st->L = h->L; st->blocks = h->blocks; st->H = h->H; st->dim = h->dim; st->N = h->N; st->stride = h->stride; st->channels = h->channels; st->coutp = h->coutp;
  auto layer = [&](const DvaeHostConv &s, DvaeConv &d) -> int {
    d.cin = s.cin; d.cout = s.cout; d.k = s.k;
    return st->dev.up(ctx, s, d);
  };
  st->res.resize(h->blocks); st->up.resize(h->L);
  if ((rc = layer(h->in, st->in))) return rc;
  for (int j = 0; j < h->blocks; j++)
    for (int q = 0; q < 3; q++)
      if ((rc = layer(h->res[j][q], st->res[j][q]))) return rc;
  for (int i = 0; i < h->L; i++) {
    if ((rc = layer(h->up[i], st->up[i]))) return rc;
    st->up[i].geo = h->up[i];
    st->up[i].geo.w.clear(); st->up[i].geo.b.clear();
  }
  if ((rc = layer(h->head, st->head)) || (rc = st->dev.up(ctx, h->Et, &st->Et))) return rc;
  if (ctx->dvae_dec) dvae_dec_free(ctx->dvae_dec);
  ctx->dvae_dec = st.release();
  return TTS_OK;
}

int dvae_dec_channels(const tts_ctx *ctx) { return ctx && ctx->dvae_dec ? ctx->dvae_dec->channels : 0; }
int dvae_dec_frames(const tts_ctx *ctx, int n_codes) {
  if (n_codes < 1) return TTS_ERR_ARG;
  if (!ctx || !ctx->dvae_dec) return 0;
  const int64_t f = ctx->dvae_dec->frames_of(n_codes);
  return f > INT32_MAX ? TTS_ERR_LIMIT : (int)f;
}

namespace {
// Every check of the decoder's side, no device call: the clips' code counts against the limits the encoder calls state
int dvae_dec_check(tts_ctx *ctx, const char *fn, const int32_t *n_codes, int B) {
  const DvaeDecState *st = ctx->dvae_dec;
  if (B > DVAE_MAX_CLIPS) return fail(ctx, TTS_ERR_LIMIT, "%s: %d clips (at most %d per call)", fn, B, DVAE_MAX_CLIPS);
  for (int s = 0; s < B; s++) {
    if (n_codes[s] < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %d codes (at least 1 expected)", fn, s, n_codes[s]);
    if (st->frames_of(n_codes[s]) > DVAE_MAX_FRAMES)
      return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %d codes decode to %lld mel frames, at most %d", fn, s, n_codes[s], (long long)st->frames_of(n_codes[s]), DVAE_MAX_FRAMES);
  }
  return TTS_OK;
}

// The layout and the buffers of a checked batch; the tables (and `codes`, when the host has them: [B][code_stride]) go up in one asynchronous copy.
// *d_codes: where the packed codes [R] are expected, unless the caller has them on the device already.
int dvae_dec_begin(tts_ctx *ctx, const int32_t *n_codes, int B, const int32_t *codes, int code_stride, const int **d_codes) {
  DvaeDecState *st = ctx->dvae_dec;
  const int L = st->L;
  LevelTable lt = level_table(n_codes, B, L + 1, [st](int64_t v, int) { return v * st->stride; }, 1, 0, false);
  const int64_t R = lt.rows[0];
  size_t act = (size_t)R * st->H;
  for (int i = 0; i < L; i++) act = std::max(act, (size_t)lt.rows[i + 1] * st->up[i].cout);
  const int max_tiles = (lt.max_n[L] + DVD_ERR_T - 1) / DVD_ERR_T;
  st->staging.assign(lt.tab.begin(), lt.tab.end());
  if (codes)
    for (int s = 0; s < B; s++) st->staging.insert(st->staging.end(), codes + (size_t)s * code_stride, codes + (size_t)s * code_stride + n_codes[s]);
  TTS_HIP(ctx, st->in_buf.reserve(st->staging.size() * 4));
  TTS_HIP(ctx, st->a.reserve(act * 4));
  TTS_HIP(ctx, st->b.reserve(act * 4));
  TTS_HIP(ctx, st->h.reserve((size_t)R * st->H * 4));
  TTS_HIP(ctx, st->mel.reserve((size_t)lt.rows[L] * st->channels * 4));
  TTS_HIP(ctx, st->part.reserve((size_t)B * max_tiles * sizeof(double2)));
  TTS_HIP(ctx, st->err.reserve((size_t)B * sizeof(double2)));
  TTS_HIP(ctx, hipMemcpyAsync(st->in_buf.p, st->staging.data(), st->staging.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (d_codes) *d_codes = st->in_buf.as<int>() + lt.tab.size();
  st->lt = std::move(lt);
  return TTS_OK;
}

// One launch sequence for the whole ragged batch: codes [R] on the device -> st->mel
int dvae_dec_launch(tts_ctx *ctx, const int *d_codes) {
  DvaeDecState *st = ctx->dvae_dec;
  const int B = st->lt.B, L = st->L;
  const std::vector<int> &max_n = st->lt.max_n;
  const std::vector<int64_t> &total = st->lt.rows;
  const int64_t R = total[0];
  hipStream_t sm = ctx->stream;
  const int *d_tab = st->in_buf.as<int>();
  auto seq = [&](int l) { return d_tab + (size_t)l * B * HFG_SEQ; };
  float *a = st->a.as<float>(), *b = st->b.as<float>(), *h = st->h.as<float>();
  {
    DvdEmbed p{};
    p.codes = d_codes; p.Et = st->Et; p.w = st->in.w; p.bias = st->in.b; p.out = h; p.R = (int)R; p.D = st->dim; p.H = st->H; p.N = st->N;
    ProfScope ps(ctx, "dvae_dec_embed", 2.0 * (double)R * st->dim * st->H);
    dvae_launch_embed(p, sm);
  }
  auto conv = [&](const float *in, float *out, const float *resid, const DvaeConv &c, float slope) {
    ProfScope ps(ctx, "dvae_dec_res", 2.0 * (double)R * c.k * c.cin * c.cout);
    dvae_launch_conv(in, out, resid, c.w, c.b, seq(0), c.cin, c.cout, c.k, slope, max_n[0], B, sm);
  };
  for (const auto &r : st->res) {
    conv(h, a, nullptr, r[0], 1.0f);
    conv(a, b, nullptr, r[1], 0.0f);
    conv(b, h, h, r[2], 0.0f);
  }
  const float *x = h;
  for (int i = 0; i < L; i++) {
    const DvdUpLayer &c = st->up[i];
    DvdUp u{};
    u.in = x; u.out = x == a ? b : a; u.w = c.w; u.bias = c.b; u.seq_in = seq(i); u.seq_out = seq(i + 1); u.cin = c.cin; u.cout = c.cout;
    u.dmin = c.geo.dmin; u.nd = c.geo.nd;
    for (int p = 0; p < 4; p++) { u.dlo[p] = c.geo.dlo[p]; u.ne[p] = c.geo.ne[p]; u.slot[p] = c.geo.slot[p]; }
    ProfScope ps(ctx, "dvae_dec_up", 2.0 * (double)total[i] * c.geo.slots * c.cin * c.cout); // the multiplications made: the folded slots
    dvae_launch_up(u, st->stride, max_n[i], B, sm);
    x = u.out;
  }
  {
    DvdHead p{};
    p.in = x; p.w = st->head.w; p.bias = st->head.b; p.mel = st->mel.as<float>(); p.seq = seq(L); p.cin = st->head.cin; p.cout = st->channels; p.coutp = st->coutp;
    ProfScope ps(ctx, "dvae_dec_head", 2.0 * (double)total[L] * p.cin * p.coutp);
    dvae_launch_head(p, max_n[L], B, sm);
  }
  TTS_HIP(ctx, hipGetLastError());
  return TTS_OK;
}
} // namespace

// mel_out: the clips back to back, clip s band-major [channels][frames_out[s]]; cap: the floats it holds
int dvae_decode(tts_ctx *ctx, const int32_t *codes, const int32_t *n_codes, int n_clips, int code_stride, float *mel_out, int32_t *frames_out, int64_t cap) {
  const char *fn = "tts_dvae_decode";
  DvaeDecState *st = ctx->dvae_dec;
  if (!st) return fail(ctx, TTS_ERR_STATE, "tts_load_dvae_decoder not called");
  if (!codes || !n_codes || !mel_out || !frames_out || n_clips < 1 || code_stride < 1) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", fn);
  int rc = dvae_dec_check(ctx, fn, n_codes, n_clips);
  if (rc) return rc;
  int64_t floats = 0;
  for (int s = 0; s < n_clips; s++) {
    if (n_codes[s] > code_stride) return fail(ctx, TTS_ERR_ARG, "%s: clip %d has %d codes, code_stride is %d", fn, s, n_codes[s], code_stride);
    for (int i = 0; i < n_codes[s]; i++) {
      const int c = codes[(size_t)s * code_stride + i];
      if (c < 0 || c >= st->N) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: code %d at position %d (0 .. %d)", fn, s, c, i, st->N - 1);
    }
    floats += st->frames_of(n_codes[s]) * st->channels;
  }
  if (floats > cap) return fail(ctx, TTS_ERR_ARG, "%s: the mel takes %lld floats, mel_out holds %lld", fn, (long long)floats, (long long)cap);
  const int *d_codes = nullptr;
  if ((rc = dvae_dec_begin(ctx, n_codes, n_clips, codes, code_stride, &d_codes)) || (rc = dvae_dec_launch(ctx, d_codes))) return rc;
  std::vector<float> mel((size_t)floats);
  TTS_HIP(ctx, hipMemcpyAsync(mel.data(), st->mel.p, mel.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(mel_out, mel.data(), mel.size() * 4);
  for (int s = 0; s < n_clips; s++) frames_out[s] = (int32_t)st->frames_of(n_codes[s]);
  return TTS_OK;
}

// tts_dvae_reconstruct in two halves, as dvae_begin / dvae_run: every check of both models and both layouts, then (once the encoder's mel buffer is filled) the
// encoder's launches, the decoder's on the codes where the quantiser left them, the error reduction, and one download.
// cap: the floats mel_out holds, -1 without a mel_out
int dvae_recon_begin(tts_ctx *ctx, const char *fn, const int32_t *frames, int n_clips, int64_t cap, float **d_mel) {
  DvaeState *en = ctx->dvae;
  DvaeDecState *de = ctx->dvae_dec;
  if (!en) return fail(ctx, TTS_ERR_STATE, "tts_load_dvae not called");
  if (!de) return fail(ctx, TTS_ERR_STATE, "tts_load_dvae_decoder not called");
  if (en->N != de->N || en->cin != de->channels)
    return fail(ctx, TTS_ERR_STATE, "%s: the encoder (%d mel channels, %d tokens) and the decoder (%d, %d) are not two halves of one model", fn, en->cin, en->N,
                de->channels, de->N);
  if (!frames || n_clips < 1) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", fn);
  if (n_clips > DVAE_MAX_CLIPS) return fail(ctx, TTS_ERR_LIMIT, "%s: %d clips (at most %d per call)", fn, n_clips, DVAE_MAX_CLIPS);
  std::vector<int32_t> nc((size_t)n_clips);
  for (int s = 0; s < n_clips; s++) {
    if (frames[s] < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %d mel frames (at least 1 expected)", fn, s, frames[s]);
    if (frames[s] > DVAE_MAX_FRAMES) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %d mel frames, at most %d", fn, s, frames[s], DVAE_MAX_FRAMES);
    int n = frames[s];
    for (int l = 0; l < en->L; l++) n = dvae_conv_rows(n, en->stride);
    nc[s] = n;
  }
  int rc = dvae_dec_check(ctx, fn, nc.data(), n_clips);
  if (rc) return rc;
  int64_t floats = 0;
  for (int s = 0; s < n_clips; s++) floats += de->frames_of(nc[s]) * de->channels;
  if (cap >= 0 && floats > cap) return fail(ctx, TTS_ERR_ARG, "%s: the mel takes %lld floats, mel_out holds %lld", fn, (long long)floats, (long long)cap);
  if ((rc = dvae_begin(ctx, fn, frames, n_clips, INT32_MAX, d_mel))) return rc;
  return dvae_dec_begin(ctx, nc.data(), n_clips, nullptr, 0, nullptr);
}

// l1_out, mse_out [B]; n_codes_out null or [B]; mel_out null or the clips' reconstructions back to back (clip s band-major [channels][codes s^L])
int dvae_recon_run(tts_ctx *ctx, float *l1_out, float *mse_out, int32_t *n_codes_out, float *mel_out) {
  DvaeState *en = ctx->dvae;
  DvaeDecState *de = ctx->dvae_dec;
  const int B = de->lt.B, L = de->L;
  const int64_t floats = de->lt.rows[L] * de->channels;
  int rc = dvae_encode(ctx);
  if (rc || (rc = dvae_dec_launch(ctx, en->codes.as<int>()))) return rc;
  hipStream_t sm = ctx->stream;
  const int max_tiles = (de->lt.max_n[L] + DVD_ERR_T - 1) / DVD_ERR_T;
  const int *seq_mel = en->tab.as<int>(), *seq_rec = de->in_buf.as<int>() + (size_t)L * B * HFG_SEQ;
  {
    ProfScope ps(ctx, "dvae_dec_err", 8.0 * (double)floats);
    dvae_err_kernel<<<dim3((unsigned)max_tiles, (unsigned)B), 256, 0, sm>>>(en->mel.as<float>(), de->mel.as<float>(), seq_mel, seq_rec, de->channels, max_tiles,
                                                                          de->part.as<double2>());
    dvae_err_reduce_kernel<<<(unsigned)((B + 63) / 64), 64, 0, sm>>>(de->part.as<double2>(), seq_mel, seq_rec, de->channels, max_tiles, B, de->err.as<double2>());
  }
  TTS_HIP(ctx, hipGetLastError());
  std::vector<double2> err((size_t)B);
  std::vector<float> mel(mel_out ? (size_t)floats : 0);
  TTS_HIP(ctx, hipMemcpyAsync(err.data(), de->err.p, err.size() * sizeof(double2), hipMemcpyDeviceToHost, sm));
  if (mel_out) TTS_HIP(ctx, hipMemcpyAsync(mel.data(), de->mel.p, mel.size() * 4, hipMemcpyDeviceToHost, sm));
  TTS_HIP(ctx, hipStreamSynchronize(sm));
  for (int s = 0; s < B; s++) {
    l1_out[s] = (float)err[s].x; mse_out[s] = (float)err[s].y;
    if (n_codes_out) n_codes_out[s] = de->lt.rec(0, s)[1];
  }
  if (mel_out) memcpy(mel_out, mel.data(), mel.size() * 4);
  return TTS_OK;
}

int dvae_reconstruct(tts_ctx *ctx, const float *mel, const int32_t *frames, int n_clips, float *l1_out, float *mse_out, float *mel_out) {
  const char *fn = "tts_dvae_reconstruct";
  if (!ctx->dvae) return fail(ctx, TTS_ERR_STATE, "tts_load_dvae not called");
  if (!ctx->dvae_dec) return fail(ctx, TTS_ERR_STATE, "tts_load_dvae_decoder not called");
  if (!mel || !frames || !l1_out || !mse_out || n_clips < 1) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", fn);
  if (n_clips > DVAE_MAX_CLIPS) return fail(ctx, TTS_ERR_LIMIT, "%s: %d clips (at most %d per call)", fn, n_clips, DVAE_MAX_CLIPS);
  int64_t total = 0;
  for (int s = 0; s < n_clips; s++) {
    if (frames[s] < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %d mel frames (at least 1 expected)", fn, s, frames[s]);
    if (frames[s] > DVAE_MAX_FRAMES) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %d mel frames, at most %d", fn, s, frames[s], DVAE_MAX_FRAMES);
    total += (int64_t)ctx->dvae->cin * frames[s];
  }
  for (int64_t i = 0; i < total; i++)
    if (!std::isfinite(mel[i])) return fail(ctx, TTS_ERR_ARG, "%s: the mel holds a non-finite value (float %lld)", fn, (long long)i);
  float *d_mel = nullptr;
  const int rc = dvae_recon_begin(ctx, fn, frames, n_clips, -1, &d_mel);
  if (rc) return rc;
  TTS_HIP(ctx, hipMemcpyAsync(d_mel, mel, (size_t)total * 4, hipMemcpyHostToDevice, ctx->stream));
  return dvae_recon_run(ctx, l1_out, mse_out, nullptr, mel_out);
}

} // namespace tts
