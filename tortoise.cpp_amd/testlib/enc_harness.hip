// Test-only harness around the eleven kernels of csrc/extras.hip and csrc/cvvp.hip (both included whole and unchanged): the CLVP / CVVP encoder layers, the voice
// encoder, the diffusion conditioning encoder and CVVP's stem. Host arrays in, host arrays out, one launch per call on a stream of its own, with the grid, block and
// template arguments of the product's launch site, each restated beside a comment that quotes the line it copies (tests/test_enc_harness_cpu.py looks every quoted
// line up in the two sources). Built as libtts_enc_test.so next to the product library (together with csrc/host_logic.cpp, which the host halves call); it is not
// part of the product (tests/test_enc_kernels_gpu.py and tests/test_enc_harness_cpu.py are the only users).
//
// THE MEMORY CONTRACT. The kernels check no bounds; they rely on the packed layout their callers build:
//   sequences   sequence s = rows [start[s], start[s] + len[s]) of a row-major matrix of `rows` rows; in order, no overlap, len >= 1.
//   attention   reads q | k | v of the sequence's own rows only; a thread past the sequence's end reads the sequence's row 0 and writes nothing.
//   im2col      taps outside the clip are zeros, not reads; output rows at or past out_len[s] are not written.
// The GPU is shared: a case is validated completely BEFORE any HIP call (every address the chosen kernel reads or writes, from the kernel's own index expressions)
// and everything else is refused; every device buffer is margin | payload | margin in one allocation, and the output is copied back whole, margins included.
#include "../csrc/extras.hip"
#include "../csrc/cvvp.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_ENC_TEST_MARGIN = 4096, TTS_ENC_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum {
  TTS_ENC_TEST_EMBED = 0, TTS_ENC_TEST_RMSNORM = 1, TTS_ENC_TEST_ATTN = 2, TTS_ENC_TEST_GEGLU = 3, TTS_ENC_TEST_POOL = 4, TTS_ENC_TEST_MEL_ROWS = 5,
  TTS_ENC_TEST_GROUPNORM = 6, TTS_ENC_TEST_IM2COL3 = 7, TTS_ENC_TEST_IM2COL5 = 8, TTS_ENC_TEST_ROWNORM = 9, TTS_ENC_TEST_ROWMEAN = 10
};
enum { TTS_ENC_TEST_ATTN_ROT64 = 0, TTS_ENC_TEST_ATTN_PLAIN64 = 1, TTS_ENC_TEST_ATTN_BIAS128 = 2 }; // clvp_attn_kernel<true,64,false>, <false,64,false>, <false,128,true>
// caps, sized by the case matrix of tests/enc_cases.py: a set of 8 sequences, 1100 rows (the set of 8), 3072 columns (kpad of the second conditioning convolution)
enum { TTS_ENC_TEST_MAX_SEQ = 8, TTS_ENC_TEST_MAX_ROWS = 1100, TTS_ENC_TEST_MAX_COLS = 3072, TTS_ENC_TEST_MAX_VOCAB = 512 };

// One case. Host pointers only. `out` holds TTS_ENC_TEST_MARGIN bytes, the payload, TTS_ENC_TEST_MARGIN bytes. Row-major everywhere.
//   EMBED      in f32 [vocab][dim], tok [rows]                                       -> out f32 [rows][dim]
//   RMSNORM    in f32 [rows][dim], p0 = g [dim]                                      -> out f16 [rows][dim]
//   ATTN       in f16 [rows][3 dim] (dim = inner: q | k | v, head h at columns h DH), start / len [nseq], variant, p0 = bias_tab [dim / 128][128] (BIAS128 only)
//                                                                                    -> out f16 [rows][dim]
//   GEGLU      in f32 [rows][2 dim] (dim = ff)                                       -> out f16 [rows][dim]
//   POOL       in f32 [rows][dim], start / len, p0 = w, p1 = b [dim]                 -> out f32 [nseq][dim]
//   MEL_ROWS   in f32 mel, in_count floats: clip s = [80][len[s]] at mel_off[s]; start / len: the output rows        -> out f16 [rows][128]
//   GROUPNORM  in f32 [rows][dim] (dim = D: 512, 1024 or 2048), start / len, p0 = g, p1 = b [dim]                    -> out f16 [rows][dim]
//   IM2COL3    variant 1 (channel-major): in f32 mel, in_count floats: clip s = [dim][len[s]] at mel_off[s]; variant 0: in f32 [rows][dim], start / len;
//              dim = cin; out_start / out_len [nseq] with out_len = (len - 1) / 2 + 1                                -> out f16 [out_rows][kpad]
//   IM2COL5    in f32 mel as IM2COL3's variant 1; out_start / out_len                                               -> out f16 [out_rows][kpad]
//   ROWNORM    in f32 [rows][dim], p0 = w, p1 = b [dim]                              -> out f16 [rows][dim]
//   ROWMEAN    in f32 [rows][dim], start / len                                       -> out f32 [nseq][dim]
// poison: the margins of `in` hold 0xFF bytes (NaN in both formats) instead of zeros.
struct tts_enc_case {
  int op, variant, nseq, rows, dim, kpad, vocab, out_rows, poison;
  long long in_count;
  const int *start, *len, *out_start, *out_len, *tok;
  const long long *mel_off;
  const void *in;
  const float *p0, *p1;
  void *out;
};

int tts_enc_test_margin(void) { return TTS_ENC_TEST_MARGIN; }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_ENC_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_ENC_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_ENC_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_ENC_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

struct Plan {
  size_t in_bytes = 0, out_bytes = 0;
  int maxlen = 0, max_out = 0;
  bool seqs = false, outs = false, moff = false; // which index arrays the kernel reads
};

// sequences in order and without overlap inside `rows` rows, len >= 1: x[(start[s] + t) * ld + c], t < len[s]
bool layout_ok(const int *start, const int *len, int nseq, int rows, int *maxlen) {
  if (!start || !len) return false;
  long long end = 0;
  for (int s = 0; s < nseq; s++) {
    if (len[s] < 1 || start[s] < end || (long long)start[s] + len[s] > rows) return false;
    end = (long long)start[s] + len[s];
    *maxlen = std::max(*maxlen, len[s]);
  }
  return true;
}

// 0 for a case that may run; hipErrorInvalidValue for a refused one
int valid(const tts_enc_case &c, Plan &pl) {
  const int bad = (int)hipErrorInvalidValue;
  if (c.op < TTS_ENC_TEST_EMBED || c.op > TTS_ENC_TEST_ROWMEAN) return bad;
  if (!c.in || !c.out) return bad;
  if (c.rows < 1 || c.rows > TTS_ENC_TEST_MAX_ROWS) return bad;
  if (c.dim < 1 || c.dim > TTS_ENC_TEST_MAX_COLS) return bad;
  if (c.poison != 0 && c.poison != 1) return bad;
  const size_t rows = (size_t)c.rows, dim = (size_t)c.dim;
  const bool by_seq = c.op == TTS_ENC_TEST_ATTN || c.op == TTS_ENC_TEST_POOL || c.op == TTS_ENC_TEST_MEL_ROWS || c.op == TTS_ENC_TEST_GROUPNORM ||
                      c.op == TTS_ENC_TEST_IM2COL3 || c.op == TTS_ENC_TEST_IM2COL5 || c.op == TTS_ENC_TEST_ROWMEAN;
  if (by_seq && (c.nseq < 1 || c.nseq > TTS_ENC_TEST_MAX_SEQ)) return bad; // seq_start[blockIdx], blockIdx < nseq
  const bool mel_in = c.op == TTS_ENC_TEST_MEL_ROWS || c.op == TTS_ENC_TEST_IM2COL5 || (c.op == TTS_ENC_TEST_IM2COL3 && c.variant == 1);
  switch (c.op) {
    case TTS_ENC_TEST_EMBED: // emb[tok[r] * dim + c], c < dim; x[r * dim + c]
      if (!c.tok || c.vocab < 1 || c.vocab > TTS_ENC_TEST_MAX_VOCAB || c.dim % 128 || c.dim > 1024) return bad;
      for (int r = 0; r < c.rows; r++)
        if (c.tok[r] < 0 || c.tok[r] >= c.vocab) return bad;
      pl.in_bytes = (size_t)c.vocab * dim * 4; pl.out_bytes = rows * dim * 4;
      break;
    case TTS_ENC_TEST_RMSNORM: // x, y [blockIdx.x * dim + c], g[c]; the product's dims: multiples of 128 up to 1024 (clvp_load)
      if (!c.p0 || c.dim % 128 || c.dim > 1024) return bad;
      pl.in_bytes = rows * dim * 4; pl.out_bytes = rows * dim * 2;
      break;
    case TTS_ENC_TEST_ROWNORM: // as RMSNORM, w[c] and b[c]
      if (!c.p0 || !c.p1 || c.dim % 128 || c.dim > 1024) return bad;
      pl.in_bytes = rows * dim * 4; pl.out_bytes = rows * dim * 2;
      break;
    case TTS_ENC_TEST_GEGLU: // u[blockIdx.x * 2 ff + c] and [.. + ff + c], y[blockIdx.x * ff + c]; ff a multiple of 128 (clvp_load)
      if (c.dim % 128 || c.dim > 1536) return bad;
      pl.in_bytes = rows * 2 * dim * 4; pl.out_bytes = rows * dim * 2;
      break;
    case TTS_ENC_TEST_ATTN: { // qkv[(r0 + t) * 3 inner + {0, 1, 2} inner + h DH + d], t < n, h < inner / DH, d < DH; out[(r0 + qi) * inner + h DH + d], qi < n
      if (c.variant < TTS_ENC_TEST_ATTN_ROT64 || c.variant > TTS_ENC_TEST_ATTN_BIAS128) return bad;
      const int DH = c.variant == TTS_ENC_TEST_ATTN_BIAS128 ? 128 : 64;
      if (c.dim % DH || c.dim > 2048) return bad;
      if ((c.variant == TTS_ENC_TEST_ATTN_BIAS128) != (c.p0 != nullptr)) return bad; // bias_tab[h * 128 + i], i < 128
      if (!layout_ok(c.start, c.len, c.nseq, c.rows, &pl.maxlen)) return bad;
      pl.in_bytes = rows * 3 * dim * 2; pl.out_bytes = rows * dim * 2; pl.seqs = true;
      break;
    }
    case TTS_ENC_TEST_POOL: // x[(r0 + r) * dim + c]; acc[4]: dim <= 1024; pooled[s * dim + c]
      if (!c.p0 || !c.p1 || c.dim % 128 || c.dim > 1024) return bad;
      if (!layout_ok(c.start, c.len, c.nseq, c.rows, &pl.maxlen)) return bad;
      pl.in_bytes = rows * dim * 4; pl.out_bytes = (size_t)c.nseq * dim * 4; pl.seqs = true;
      break;
    case TTS_ENC_TEST_ROWMEAN: // x[start * dim + c + r * dim], c < dim, r < n; pooled[s * dim + c]
      if (c.dim % 128 || c.dim > 1024) return bad;
      if (!layout_ok(c.start, c.len, c.nseq, c.rows, &pl.maxlen)) return bad;
      pl.in_bytes = rows * dim * 4; pl.out_bytes = (size_t)c.nseq * dim * 4; pl.seqs = true;
      break;
    case TTS_ENC_TEST_GROUPNORM: // x, y[(r0 + t) * D + c], c < D, t < T; g[c], b[c]
      if (!c.p0 || !c.p1 || (c.dim != 512 && c.dim != 1024 && c.dim != 2048)) return bad;
      if (!layout_ok(c.start, c.len, c.nseq, c.rows, &pl.maxlen)) return bad;
      pl.in_bytes = rows * dim * 4; pl.out_bytes = rows * dim * 2; pl.seqs = true;
      break;
    case TTS_ENC_TEST_MEL_ROWS: // mel[mel_off[s] + c * T + t], c < 80, t < T; a16[(start[s] + t) * 128 + c], c < 128
      if (c.dim != 80) return bad;
      if (!layout_ok(c.start, c.len, c.nseq, c.rows, &pl.maxlen)) return bad;
      pl.out_bytes = rows * 128 * 2; pl.seqs = true;
      break;
    case TTS_ENC_TEST_IM2COL3:
    case TTS_ENC_TEST_IM2COL5: { // a16[(out_start[s] + t) * kpad + k], t < out_len[s], k < kpad; the input at tap * cin + c, tap < taps, 0 <= ti < Tin only
      const int taps = c.op == TTS_ENC_TEST_IM2COL3 ? 3 : 5;
      if (c.op == TTS_ENC_TEST_IM2COL3 && c.variant != 0 && c.variant != 1) return bad;
      if (c.kpad < taps * c.dim || c.kpad > TTS_ENC_TEST_MAX_COLS || c.kpad % 64) return bad; // the K of a GEMM: the product pads it to a multiple of 64
      if (c.out_rows < 1 || c.out_rows > TTS_ENC_TEST_MAX_ROWS) return bad;
      if (!c.len) return bad;
      if (!layout_ok(c.out_start, c.out_len, c.nseq, c.out_rows, &pl.max_out)) return bad;
      if (mel_in) {
        for (int s = 0; s < c.nseq; s++)
          if (c.len[s] < 1) return bad;
      } else {
        int ml = 0;
        if (!layout_ok(c.start, c.len, c.nseq, c.rows, &ml)) return bad;
        pl.in_bytes = rows * dim * 4;
      }
      for (int s = 0; s < c.nseq; s++) // the convolution's output length: stride 2, `same` padding (cvvp_voice_begin, diff_cond_enc_begin)
        if (c.out_len[s] != (c.len[s] - 1) / 2 + 1) return bad;
      pl.out_bytes = (size_t)c.out_rows * c.kpad * 2; pl.seqs = true; pl.outs = true;
      break;
    }
  }
  if (mel_in) { // clip s = in[mel_off[s] .. + dim * len[s]) inside in_count floats
    if (!c.mel_off || c.in_count < 1 || c.in_count > (long long)TTS_ENC_TEST_MAX_ROWS * TTS_ENC_TEST_MAX_COLS) return bad;
    for (int s = 0; s < c.nseq; s++)
      if (c.mel_off[s] < 0 || c.mel_off[s] + (long long)c.dim * c.len[s] > c.in_count) return bad;
    pl.in_bytes = (size_t)c.in_count * 4; pl.moff = true;
  }
  return 0;
}

} // namespace

extern "C" {

// 0 for a case tts_enc_test_run would launch (host only: no HIP call)
int tts_enc_test_validate(const tts_enc_case *c) {
  Plan pl;
  return c ? valid(*c, pl) : (int)hipErrorInvalidValue;
}
// bytes of the payload of `out` for a valid case, or minus the refusal's status
long long tts_enc_test_out_bytes(const tts_enc_case *c) {
  Plan pl;
  const int rc = c ? valid(*c, pl) : (int)hipErrorInvalidValue;
  return rc ? -(long long)rc : (long long)pl.out_bytes;
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_enc_test_run(const tts_enc_case *cp) {
  Plan pl;
  if (!cp) return (int)hipErrorInvalidValue;
  const int rc = valid(*cp, pl);
  if (rc) return rc;
  const tts_enc_case &c = *cp;
  Dev in, out, p0, p1, start, len, ostart, olen, moff, tok;
  const int in_fill = c.poison ? 0xFF : 0;
  HT(in.alloc(pl.in_bytes, in_fill)); HT(in.put(c.in));
  HT(out.alloc(pl.out_bytes, TTS_ENC_TEST_SENTINEL));
  const size_t ncol = c.op == TTS_ENC_TEST_ATTN ? (size_t)(c.dim / 128) * 128 : (size_t)c.dim; // bias_tab [heads][128]; everything else [dim]
  if (c.p0) { HT(p0.alloc(ncol * 4, 0)); HT(p0.put(c.p0)); }
  if (c.p1) { HT(p1.alloc(ncol * 4, 0)); HT(p1.put(c.p1)); }
  if (pl.seqs) {
    HT(len.alloc((size_t)c.nseq * 4, 0)); HT(len.put(c.len));
    if (c.start) { HT(start.alloc((size_t)c.nseq * 4, 0)); HT(start.put(c.start)); }
  }
  if (pl.outs) {
    HT(ostart.alloc((size_t)c.nseq * 4, 0)); HT(ostart.put(c.out_start));
    HT(olen.alloc((size_t)c.nseq * 4, 0)); HT(olen.put(c.out_len));
  }
  if (pl.moff) { HT(moff.alloc((size_t)c.nseq * 8, 0)); HT(moff.put(c.mel_off)); }
  if (c.op == TTS_ENC_TEST_EMBED) { HT(tok.alloc((size_t)c.rows * 4, 0)); HT(tok.put(c.tok)); }
  const float *x = (const float *)in.data(), *g = (const float *)p0.data(), *b = (const float *)p1.data();
  const __half *qkv = (const __half *)in.data();
  const int *d_start = (const int *)start.data(), *d_len = (const int *)len.data(), *d_ostart = (const int *)ostart.data(), *d_olen = (const int *)olen.data();
  const long long *d_moff = (const long long *)moff.data();
  float *of = (float *)out.data();
  __half *oh = (__half *)out.data();
  const int rows = c.rows, nseq = c.nseq, d = c.dim, maxlen = pl.maxlen;
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    switch (c.op) {
      case TTS_ENC_TEST_EMBED:
        // enc_embed: clvp_embed_kernel<<<rows, 256, 0, ctx->stream>>>(emb, d_tok, dim, x);
        clvp_embed_kernel<<<rows, 256, 0, s>>>(x, (const int *)tok.data(), d, of);
        break;
      case TTS_ENC_TEST_RMSNORM:
        // enc_run_layers: clvp_rmsnorm_kernel<<<rows, 256, 0, ctx->stream>>>(x, l.g_attn, d, y);
        clvp_rmsnorm_kernel<<<rows, 256, 0, s>>>(x, g, d, oh);
        break;
      case TTS_ENC_TEST_ATTN:
        if (c.variant == TTS_ENC_TEST_ATTN_ROT64)
          // enc_run_layers: clvp_attn_kernel<true, 64, false><<<dim3(w.nseq, in / CLVP_DH, (w.maxlen + 255) / 256), 256, 0, ctx->stream>>>(qkv, w.d_start, w.d_len, in, att, nullptr);
          clvp_attn_kernel<true, 64, false><<<dim3(nseq, d / CLVP_DH, (maxlen + 255) / 256), 256, 0, s>>>(qkv, d_start, d_len, d, oh, nullptr);
        else if (c.variant == TTS_ENC_TEST_ATTN_PLAIN64)
          // attn_block_run: clvp_attn_kernel<false, 64, false><<<dim3(w.nseq, D / CLVP_DH, (w.maxlen + 255) / 256), 256, 0, ctx->stream>>>(w.qkv, w.d_start, w.d_len, D, w.att, nullptr);
          clvp_attn_kernel<false, 64, false><<<dim3(nseq, d / CLVP_DH, (maxlen + 255) / 256), 256, 0, s>>>(qkv, d_start, d_len, d, oh, nullptr);
        else
          // diff_cond_enc_run: clvp_attn_kernel<false, 128, true><<<dim3(n_clips, 16, (max2 + 255) / 256), 256, 0, ctx->stream>>>(qkv, d_start, d_len, D, att, b.bias_tab);
          // (16 = D / 128 heads at the product's D = 2048)
          clvp_attn_kernel<false, 128, true><<<dim3(nseq, d / 128, (maxlen + 255) / 256), 256, 0, s>>>(qkv, d_start, d_len, d, oh, g);
        break;
      case TTS_ENC_TEST_GEGLU:
        // enc_run_layers: clvp_geglu_kernel<<<rows, 256, 0, ctx->stream>>>(u, ff, y);
        clvp_geglu_kernel<<<rows, 256, 0, s>>>(x, d, oh);
        break;
      case TTS_ENC_TEST_POOL:
        // clvp_encode: clvp_pool_kernel<<<nseq, 256, 0, ctx->stream>>>(x, d_start, d_len, st->norm_w[e], st->norm_b[e], d, st->pooled.as<float>());
        clvp_pool_kernel<<<nseq, 256, 0, s>>>(x, d_start, d_len, g, b, d, of);
        break;
      case TTS_ENC_TEST_MEL_ROWS:
        // voice_enc_run: venc_mel_rows_kernel<<<dim3(maxlen, n_clips), 128, 0, ctx->stream>>>(st->mel.as<float>(), d_start, d_len, d_moff, a16);
        venc_mel_rows_kernel<<<dim3(maxlen, nseq), 128, 0, s>>>(x, d_start, d_len, d_moff, oh);
        break;
      case TTS_ENC_TEST_GROUPNORM:
        // attn_block_run: if (D == 512) venc_groupnorm_kernel<512><<<dim3(32, w.nseq), 256, 0, ctx->stream>>>(w.x, w.d_start, w.d_len, b.g, b.b, w.y);
        if (d == 512) venc_groupnorm_kernel<512><<<dim3(32, nseq), 256, 0, s>>>(x, d_start, d_len, g, b, oh);
        // attn_block_run: else if (D == 1024) venc_groupnorm_kernel<1024><<<dim3(32, w.nseq), 256, 0, ctx->stream>>>(w.x, w.d_start, w.d_len, b.g, b.b, w.y);
        else if (d == 1024) venc_groupnorm_kernel<1024><<<dim3(32, nseq), 256, 0, s>>>(x, d_start, d_len, g, b, oh);
        // diff_cond_enc_run: venc_groupnorm_kernel<2048><<<dim3(32, n_clips), 256, 0, ctx->stream>>>(x, d_start, d_len, b.g, b.b, y);
        else venc_groupnorm_kernel<2048><<<dim3(32, nseq), 256, 0, s>>>(x, d_start, d_len, g, b, oh);
        break;
      case TTS_ENC_TEST_IM2COL3:
        if (c.variant == 1)
          // diff_cond_enc_run: dcond_im2col_kernel<true><<<dim3(max1, n_clips), 256, 0, ctx->stream>>>(st->mel.as<float>(), d_moff, dm, dm + n_clips, dm + 2 * n_clips, dm + 3 * n_clips, 100, 320, a16);
          // (in_start is not read by the channel-major form: the product passes its unused meta block, the harness a null pointer)
          dcond_im2col_kernel<true><<<dim3(pl.max_out, nseq), 256, 0, s>>>(x, d_moff, nullptr, d_len, d_ostart, d_olen, d, c.kpad, oh);
        else
          // im2col3_rows: dcond_im2col_kernel<false><<<dim3(max_out, nseq), 256, 0, ctx->stream>>>(x, nullptr, in_start, in_len, out_start, out_len, cin, kpad, a16);
          dcond_im2col_kernel<false><<<dim3(pl.max_out, nseq), 256, 0, s>>>(x, nullptr, d_start, d_len, d_ostart, d_olen, d, c.kpad, oh);
        break;
      case TTS_ENC_TEST_IM2COL5:
        // cvvp_voice_run: cvvp_im2col5_kernel<<<dim3(max1, n_clips), 256, 0, ctx->stream>>>(st->mel.as<float>(), d_moff, dm, dm + n_clips, dm + 2 * n_clips, 80, k0, a16);
        cvvp_im2col5_kernel<<<dim3(pl.max_out, nseq), 256, 0, s>>>(x, d_moff, d_len, d_ostart, d_olen, d, c.kpad, oh);
        break;
      case TTS_ENC_TEST_ROWNORM:
        // cvvp_collapse: cvvp_rownorm_kernel<<<rows, 256, 0, ctx->stream>>>(w.x, sd.norm_w, sd.norm_b, d, w.y);
        cvvp_rownorm_kernel<<<rows, 256, 0, s>>>(x, g, b, d, oh);
        break;
      default:
        // cvvp_collapse: cvvp_rowmean_kernel<<<dim3(nseq, (d + 255) / 256), 256, 0, ctx->stream>>>(w.x, d_start, d_len, d, st->pooled.as<float>());
        cvvp_rowmean_kernel<<<dim3(nseq, (d + 255) / 256), 256, 0, s>>>(x, d_start, d_len, d, of);
        break;
    }
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
