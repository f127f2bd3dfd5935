// Test-only harness around the AR stage's two decode GEMV kernels and the weight layouts they read (csrc/ar.hip, included whole and unchanged):
//   tts_dec_test_pack      one weight matrix through the product's host packers or its pk_* kernels -> the slab bytes, the folded bias, the fp8 column scales
//   tts_dec_test_ln_gemv   one launch of dec_ln_gemv_kernel<EPI, SPLIT, NTW, HT, RO> on such a slab
//   tts_dec_test_resid     one launch of dec_gemv_resid_kernel<KG, NT, WH, NTW, HT>
// Host arrays in, host arrays out, one launch on a stream of its own, with the grid and block size of the product's launch site. Built as libtts_dec_test.so
// next to the product library (together with csrc/host_logic.cpp, which ar.hip's host half calls); it is not part of the product
// (tests/test_ar_dec_kernels_gpu.py and tests/test_ar_dec_harness_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (the instantiation is one the product launches, shapes, strides, every row's K/V
// position, the slab's range, every pointer the chosen kernel reads or writes), and every device buffer carries a canary margin in front and behind, inside
// the same allocation. Output buffers are copied back margin | payload | margin; the margins of input buffers are checked here (TTS_DEC_TEST_ERR_CANARY).
#include "../csrc/ar.hip"

#include <cstdint>
#include <cstring>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_DEC_TEST_MARGIN = 4096, TTS_DEC_TEST_SENTINEL = 0xCB, TTS_DEC_TEST_FILL_IN = 0x5A }; // 0x5A: the margins of input buffers
enum { TTS_DEC_TEST_ERR_CANARY = -2 };
enum { TTS_DEC_TEST_MAX_ROWS = 64, TTS_DEC_TEST_MAX_SLOTS = 64 };
enum { TTS_DEC_LAYOUT_STRIP = 0, TTS_DEC_LAYOUT_MFMA16 = 1, TTS_DEC_LAYOUT_MFMA16H = 2, TTS_DEC_LAYOUT_COLS4 = 3, TTS_DEC_LAYOUT_SPLITW = 4 };
enum { TTS_DEC_ENC_F32 = 0, TTS_DEC_ENC_SPLIT = 1, TTS_DEC_ENC_F16 = 2, TTS_DEC_ENC_E4M3 = 3 };

// One matrix W [K][N] f32 (transpose != 0, device only: W is nn.Linear's [vrows][K] and becomes [K][N] zero padded through pk_transpose_pad_kernel).
// g != null: LayerNorm (g, b) and the bias c are folded in (fold_layernorm / pk_fold_kernel + pk_fold_bias_kernel). where: 0 host packers (no HIP call), 1 pk_* kernels.
// Every output is optional and guarded (margin | payload | margin): slab (slab_bytes of payload), fold [K][N] f32 (the matrix the slab was built from),
// bias [N] (g != null), scales [N] (host, every encoding: fp8_col_scales of the folded matrix), absmax [1] (device: pk_absmax_kernel's word as a float).
struct tts_dec_pack_case {
  int K, N, layout, enc, where, transpose, vrows;
  const float *W, *g, *b, *c;
  size_t slab_bytes;
  void *slab;
  float *fold, *bias, *scales, *absmax;
};

// One launch of dec_ln_gemv_kernel. h [rows][1024] f32 (ht: the harness builds the h4 buffer of whole tiles with h4_index, every padding row NaN).
// slab: the layout the instantiation reads (split 0: mfma16 f32, 1: mfma16h hi|lo, 2: mfma16h fp16, 3: mfma16h e4m3 + wscale [N]). bias [N] (folded).
// epi 0 (QKV, N = 3072): out = q [rows][ldo]; kc / vc [n_slots][max_pos][1024] f16 come back whole (pre-filled with the sentinel); prefill_B = 0: decode form,
// row r stores at slot r, position n_past + row_off[r] (ro; row_off [tiles * 16], the padding zero); prefill_B > 0: prompt form, row = position.
// epi 1 (GELU, N = 4096): out = ff [rows][4096]. epi 2 (LOGITS): g1 / b1 [1024], out [rows][ldo], columns < n_valid.
struct tts_dec_ln_case {
  int epi, split, ntw, ht, ro;
  int rows, N, n_valid, ldo, prefill_B, n_past, max_pos, n_slots, lut;
  const float *h, *g1, *b1;
  const void *slab;
  size_t slab_bytes;
  const float *bias, *wscale;
  const int *row_off;
  float *out;        // guarded, rows * ldo (QKV, LOGITS) or rows * 4096 (GELU) floats
  uint16_t *kc, *vc; // guarded, QKV only
};

// One launch of dec_gemv_resid_kernel<kg, kg == 1 ? 256 : 512, wh, ntw, ht>: h += X [rows][1024 kg] . W + bias. slab: cols4 as f32 (wh 0), fp16 (1), e4m3 (2, wscale [1024]).
// h_in [rows][1024]; h_out: the device buffer as it lies, guarded: [rows][1024], or (ht) the h4 buffer of whole tiles whose padding rows went in as NaN.
struct tts_dec_resid_case {
  int kg, wh, ntw, ht, rows;
  const float *X;
  const void *slab;
  size_t slab_bytes;
  const float *bias, *wscale, *h_in;
  float *h_out;
};

int tts_dec_test_margin(void) { return TTS_DEC_TEST_MARGIN; }
// the index of (row, channel) in the h4 layout, for the CPU test of the reference's restatement
size_t tts_dec_test_h4_index(int r, int k) { return h4_index(r, k); }
uint8_t tts_dec_test_fp8(float v) { return tts_host_fp8_e4m3(v); }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  int fill = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int f) {
    bytes = payload; fill = f;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_DEC_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, f, payload + 2 * TTS_DEC_TEST_MARGIN);
  }
  hipError_t in(size_t payload, const void *h) { // an input buffer
    hipError_t e = alloc(payload, TTS_DEC_TEST_FILL_IN);
    return e != hipSuccess ? e : hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice);
  }
  char *data() const { return p + TTS_DEC_TEST_MARGIN; }
  template <class T> T *as() const { return p ? (T *)data() : nullptr; }
  hipError_t get_all(void *h) const { return h ? hipMemcpy(h, p, bytes + 2 * TTS_DEC_TEST_MARGIN, hipMemcpyDeviceToHost) : hipSuccess; }
  bool margins_intact() const { // of a buffer the launch must not write
    if (!p) return true;
    std::vector<unsigned char> m(2 * TTS_DEC_TEST_MARGIN);
    if (hipMemcpy(m.data(), p, TTS_DEC_TEST_MARGIN, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (hipMemcpy(m.data() + TTS_DEC_TEST_MARGIN, p + TTS_DEC_TEST_MARGIN + bytes, TTS_DEC_TEST_MARGIN, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (unsigned char b : m)
      if (b != (unsigned char)fill) return false;
    return true;
  }
};

// a host result into a guarded host buffer
void put_guarded(void *dst, const void *src, size_t bytes) {
  if (!dst) return;
  memset(dst, TTS_DEC_TEST_SENTINEL, bytes + 2 * TTS_DEC_TEST_MARGIN);
  memcpy((char *)dst + TTS_DEC_TEST_MARGIN, src, bytes);
}

size_t slab_bytes_of(int K, int N, int layout, int enc) {
  const size_t n = (size_t)K * N;
  if (layout == TTS_DEC_LAYOUT_SPLITW) return n * 4;
  return enc == TTS_DEC_ENC_F32 || enc == TTS_DEC_ENC_SPLIT ? n * 4 : enc == TTS_DEC_ENC_F16 ? n * 2 : n;
}

bool pack_valid(const tts_dec_pack_case &c) {
  if (!c.W || c.K < 1 || c.N < 1 || (size_t)c.K * c.N > (size_t)4096 * 8256) return false;
  if (c.where != 0 && c.where != 1) return false;
  if ((c.g != nullptr) != (c.b != nullptr) || (c.g != nullptr) != (c.c != nullptr)) return false; // a fold needs all three
  if (c.bias && !c.g) return false;
  if (c.transpose && (c.where != 1 || c.vrows < 1 || c.vrows > c.N)) return false; // the host path takes [K][N]
  if (c.absmax && c.where != 1) return false;
  if (c.fold && c.where == 1 && !c.g && !c.transpose) return false; // the device path gives back a matrix it built, not its input
  if (c.slab && c.slab_bytes != slab_bytes_of(c.K, c.N, c.layout, c.enc)) return false;
  switch (c.layout) {
    case TTS_DEC_LAYOUT_STRIP: if (c.enc != TTS_DEC_ENC_F32 || c.N % 64) return false; break;
    case TTS_DEC_LAYOUT_MFMA16: if (c.enc != TTS_DEC_ENC_F32 || c.K != 1024 || c.N % 16 || c.where != 0) return false; break; // the loader builds it on the host only
    case TTS_DEC_LAYOUT_MFMA16H:
      if (c.K != 1024 || c.N % 16) return false;
      if (c.enc != TTS_DEC_ENC_SPLIT && c.enc != TTS_DEC_ENC_F16 && c.enc != TTS_DEC_ENC_E4M3) return false;
      if (c.where == 1 && c.enc != TTS_DEC_ENC_SPLIT) return false;
      break;
    case TTS_DEC_LAYOUT_COLS4:
      if ((c.K != 1024 && c.K != 4096) || c.N % 4) return false;
      if (c.enc != TTS_DEC_ENC_F32 && c.enc != TTS_DEC_ENC_F16 && c.enc != TTS_DEC_ENC_E4M3) return false;
      if (c.where == 1 && c.enc != TTS_DEC_ENC_F32) return false;
      break;
    case TTS_DEC_LAYOUT_SPLITW: if (c.enc != TTS_DEC_ENC_SPLIT || c.where != 1 || c.K % 32 || c.N % 64) return false; break; // split_weight_kernel reads strip-major
    default: return false;
  }
  return true;
}

bool pow2_positive(float s) {
  if (!(s > 0.f) || !std::isfinite(s)) return false;
  int e;
  return std::frexp(s, &e) == 0.5f;
}

// the product's instantiations of dec_ln_gemv_kernel (prompt_pass, launch_dec_qkv, enqueue_decode_step): 22
bool ln_combo(int epi, int split, int ntw, int ht, int ro) {
  if (epi < DEC_QKV || epi > DEC_LOGITS || split < 0 || split > 3 || (ntw | ht | ro) & ~1) return false;
  if (ntw != (split == 1 || split == 3)) return false; // the non-temporal form goes with SPLIT 1 and 3 at every site
  if (!ht) return split <= 1 && !ro;                   // prompt pass: f32 MFMA or split precision
  return !ro || epi == DEC_QKV;
}

bool ln_valid(const tts_dec_ln_case &c) {
  if (!ln_combo(c.epi, c.split, c.ntw, c.ht, c.ro)) return false;
  if (c.rows < 1 || c.rows > TTS_DEC_TEST_MAX_ROWS || c.N < 16 || c.N % 16 || c.N > VPAD) return false;
  if ((c.lut != 0 && c.lut != 1) || !c.h || !c.slab || !c.bias || !c.out) return false;
  if (c.slab_bytes != (size_t)D * c.N * (c.split <= 1 ? 4 : c.split == 2 ? 2 : 1)) return false;
  if (c.n_valid < 1 || c.n_valid > c.N) return false;
  const int tiles = (c.rows + 15) / 16;
  if (c.epi == DEC_QKV) {
    if (c.N != 3 * D || c.n_valid != c.N || c.ldo < D || c.ldo % 4 || c.ldo > 4 * D) return false;
    if (!c.kc || !c.vc || c.max_pos < 1 || c.max_pos > 1024 || c.n_slots < 1 || c.n_slots > TTS_DEC_TEST_MAX_SLOTS) return false;
    if (c.prefill_B < 0) return false;
    if (c.prefill_B > 0) { // prompt form: row = position, replicated into prefill_B slots
      if (c.ht || c.ro || c.prefill_B > c.n_slots || c.rows > c.max_pos) return false;
    } else {
      if (!c.ht || c.rows > c.n_slots) return false; // the product launches the decode form on h4 only
      if (c.ro && !c.row_off) return false;
      for (int r = 0; r < tiles * 16; r++) {
        const long long off = c.ro ? c.row_off[r] : 0;
        if (r >= c.rows) { if (off != 0) return false; continue; } // padded with zeros to whole tiles, as the session does
        const long long pos = (long long)c.n_past + off;
        if (pos < 0 || pos >= c.max_pos) return false;
      }
    }
  } else if (c.epi == DEC_GELU) {
    if (c.N != FF || c.n_valid != c.N || c.prefill_B != 0) return false;
  } else {
    if (!c.g1 || !c.b1 || c.ldo < c.n_valid || c.ldo > 2 * VPAD || c.prefill_B != 0) return false;
  }
  if (c.split == 1 || c.split == 2) { // the loader's range guard, on what the slab holds: 64 |w| < 60000 and finite
    const uint16_t *s = (const uint16_t *)c.slab;
    const size_t n = c.slab_bytes / 2;
    for (size_t i = 0; i < n; i++) {
      __half hv; memcpy(&hv, s + i, 2);
      const float v = __half2float(hv);
      if (!(std::fabs(v) < 60000.0f)) return false;
    }
  }
  if (c.split == 3) {
    if (!c.wscale) return false;
    for (int n = 0; n < c.N; n++)
      if (!pow2_positive(c.wscale[n])) return false;
  }
  return true;
}

// the product's instantiations of dec_gemv_resid_kernel: 8
bool resid_valid(const tts_dec_resid_case &c) {
  if ((c.kg != 1 && c.kg != 4) || c.wh < 0 || c.wh > 2 || (c.ntw | c.ht) & ~1) return false;
  if (c.ntw != (c.ht && c.wh == 0)) return false;
  if (!c.ht && c.wh != 0) return false;
  if (c.rows < 1 || c.rows > TTS_DEC_TEST_MAX_ROWS || !c.X || !c.slab || !c.bias || !c.h_in || !c.h_out) return false;
  if (c.slab_bytes != (size_t)c.kg * 1024 * D * (c.wh == 0 ? 4 : c.wh == 1 ? 2 : 1)) return false;
  if (c.wh == 2) {
    if (!c.wscale) return false;
    for (int n = 0; n < D; n++)
      if (!pow2_positive(c.wscale[n])) return false;
  }
  return true;
}

#define HT_(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int pack_host(const tts_dec_pack_case &c) {
  const int K = c.K, N = c.N;
  std::vector<float> wfold, cfold;
  const float *w = c.W;
  if (c.g) { fold_layernorm(c.W, K, N, c.g, c.b, c.c, wfold, cfold); w = wfold.data(); }
  put_guarded(c.fold, w, (size_t)K * N * 4);
  if (c.g) put_guarded(c.bias, cfold.data(), (size_t)N * 4);
  const std::vector<float> sc = fp8_col_scales(w, K, N);
  put_guarded(c.scales, sc.data(), (size_t)N * 4);
  if (!c.slab) return 0;
  const auto c4 = [K](size_t o) { return cols4_at(o, K); };
  const auto m16h = [](size_t i) { return mfma16h_at(i); };
  if (c.layout == TTS_DEC_LAYOUT_STRIP) put_guarded(c.slab, strip_major(w, K, N).data(), c.slab_bytes);
  else if (c.layout == TTS_DEC_LAYOUT_MFMA16) put_guarded(c.slab, pack<float, 1>(w, K, N, [](size_t o) { return mfma16_at(o); }, EncF32{}).data(), c.slab_bytes);
  else if (c.layout == TTS_DEC_LAYOUT_MFMA16H) {
    if (c.enc == TTS_DEC_ENC_SPLIT) put_guarded(c.slab, pack_mfma16h(w, N).data(), c.slab_bytes);
    else if (c.enc == TTS_DEC_ENC_F16) put_guarded(c.slab, pack<__half, 1>(w, K, N, m16h, EncF16{W16_SCALE}).data(), c.slab_bytes);
    else put_guarded(c.slab, pack_mfma16o(w, N, sc).data(), c.slab_bytes);
  } else {
    if (c.enc == TTS_DEC_ENC_F32) put_guarded(c.slab, pack<float, 4>(w, K, N, c4, EncF32{}).data(), c.slab_bytes);
    else if (c.enc == TTS_DEC_ENC_F16) put_guarded(c.slab, pack<__half, 4>(w, K, N, c4, EncF16{1.0f}).data(), c.slab_bytes);
    else put_guarded(c.slab, pack<uint8_t, 4>(w, K, N, c4, EncFp8{sc.data()}).data(), c.slab_bytes);
  }
  return 0;
}

int pack_device(const tts_dec_pack_case &c) {
  const int K = c.K, N = c.N;
  const size_t n = (size_t)K * N;
  Dev raw, wt, g, b, cc, fold, bias, mx, strip, slab;
  HT_(raw.in(c.transpose ? (size_t)c.vrows * K * 4 : n * 4, c.W));
  if (c.transpose) HT_(wt.alloc(n * 4, TTS_DEC_TEST_SENTINEL));
  if (c.g) {
    HT_(g.in((size_t)K * 4, c.g)); HT_(b.in((size_t)K * 4, c.b)); HT_(cc.in((size_t)N * 4, c.c));
    HT_(fold.alloc(n * 4, TTS_DEC_TEST_SENTINEL)); HT_(bias.alloc((size_t)N * 4, TTS_DEC_TEST_SENTINEL));
  }
  HT_(mx.alloc(4, TTS_DEC_TEST_SENTINEL)); HT_(hipMemset(mx.data(), 0, 4));
  if (c.layout == TTS_DEC_LAYOUT_SPLITW) HT_(strip.alloc(n * 4, TTS_DEC_TEST_SENTINEL));
  if (c.slab) HT_(slab.alloc(c.slab_bytes, TTS_DEC_TEST_SENTINEL));
  hipStream_t s;
  HT_(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  const int pg = ArLoader::pgrid(n);
  const float *w = raw.as<float>();
  if (e == hipSuccess) {
    if (c.transpose) { pk_transpose_pad_kernel<<<pg, 256, 0, s>>>(w, c.vrows, K, N, wt.as<float>()); w = wt.as<float>(); }
    const float *wf = w;
    if (c.g) {
      pk_fold_kernel<<<pg, 256, 0, s>>>(w, K, N, g.as<float>(), fold.as<float>());
      pk_fold_bias_kernel<<<(N + 255) / 256, 256, 0, s>>>(w, K, N, b.as<float>(), cc.as<float>(), bias.as<float>());
      wf = fold.as<float>();
    }
    pk_absmax_kernel<<<std::min(pg, 1024), 256, 0, s>>>(wf, n, mx.as<unsigned>());
    if (c.slab) {
      if (c.layout == TTS_DEC_LAYOUT_STRIP) pk_strip_major_kernel<<<pg, 256, 0, s>>>(wf, K, N, slab.as<float>());
      else if (c.layout == TTS_DEC_LAYOUT_MFMA16H) pk_mfma16h_kernel<<<pg, 256, 0, s>>>(wf, N, slab.as<__half>());
      else if (c.layout == TTS_DEC_LAYOUT_COLS4) pk_cols4_kernel<<<pg, 256, 0, s>>>(wf, K, N, slab.as<float>());
      else {
        pk_strip_major_kernel<<<pg, 256, 0, s>>>(wf, K, N, strip.as<float>());
        split_weight_kernel<<<dim3(N / 32, K / 32), 256, 0, s>>>(strip.as<float>(), K, N, slab.as<__half>());
      }
    }
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  if (e != hipSuccess || es != hipSuccess) return (int)(e != hipSuccess ? e : es);
  HT_(slab.get_all(c.slab)); HT_(mx.get_all(c.absmax));
  if (c.g) { HT_(fold.get_all(c.fold)); HT_(bias.get_all(c.bias)); }
  else HT_(wt.get_all(c.fold)); // no fold: the transposed, padded matrix
  const bool ok = raw.margins_intact() && g.margins_intact() && b.margins_intact() && cc.margins_intact() && strip.margins_intact() &&
                  (!c.transpose || wt.margins_intact());
  return ok ? 0 : (int)TTS_DEC_TEST_ERR_CANARY;
}

template <int EPI, int SPLIT, bool NTW, bool HT, bool RO> void ln_launch(dim3 grid, hipStream_t s, const DecLnArgs &a) {
  dec_ln_gemv_kernel<EPI, SPLIT, NTW, HT, RO><<<grid, 256, 0, s>>>(a);
}
template <int EPI> void ln_dispatch(const tts_dec_ln_case &c, dim3 grid, hipStream_t s, const DecLnArgs &a) {
  if (!c.ht) {
    if (c.split == 0) ln_launch<EPI, 0, false, false, false>(grid, s, a);
    else ln_launch<EPI, 1, true, false, false>(grid, s, a);
    return;
  }
  if (EPI == DEC_QKV && c.ro) {
    switch (c.split) {
      case 0: ln_launch<DEC_QKV, 0, false, true, true>(grid, s, a); break;
      case 1: ln_launch<DEC_QKV, 1, true, true, true>(grid, s, a); break;
      case 2: ln_launch<DEC_QKV, 2, false, true, true>(grid, s, a); break;
      default: ln_launch<DEC_QKV, 3, true, true, true>(grid, s, a); break;
    }
    return;
  }
  switch (c.split) {
    case 0: ln_launch<EPI, 0, false, true, false>(grid, s, a); break;
    case 1: ln_launch<EPI, 1, true, true, false>(grid, s, a); break;
    case 2: ln_launch<EPI, 2, false, true, false>(grid, s, a); break;
    default: ln_launch<EPI, 3, true, true, false>(grid, s, a); break;
  }
}

} // namespace

extern "C" {

// 0 for a case the run entry would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_dec_test_pack_validate(const tts_dec_pack_case *c) { return c && pack_valid(*c) ? 0 : (int)hipErrorInvalidValue; }
int tts_dec_test_ln_gemv_validate(const tts_dec_ln_case *c) { return c && ln_valid(*c) ? 0 : (int)hipErrorInvalidValue; }
int tts_dec_test_resid_validate(const tts_dec_resid_case *c) { return c && resid_valid(*c) ? 0 : (int)hipErrorInvalidValue; }

int tts_dec_test_pack(const tts_dec_pack_case *c) {
  if (!c || !pack_valid(*c)) return (int)hipErrorInvalidValue;
  return c->where == 0 ? pack_host(*c) : pack_device(*c);
}

int tts_dec_test_ln_gemv(const tts_dec_ln_case *cp) {
  if (!cp || !ln_valid(*cp)) return (int)hipErrorInvalidValue;
  const tts_dec_ln_case &c = *cp;
  const int tiles = (c.rows + 15) / 16;
  const size_t out_elems = (size_t)c.rows * (c.epi == DEC_GELU ? FF : c.ldo);
  const size_t cache_bytes = c.epi == DEC_QKV ? (size_t)c.n_slots * c.max_pos * D * 2 : 0;
  std::vector<float> h4;
  if (c.ht) { // whole tiles, every padding row NaN
    h4.assign((size_t)tiles * 16 * D, std::nanf(""));
    for (int r = 0; r < c.rows; r++)
      for (int k = 0; k < D; k++) h4[h4_index(r, k)] = c.h[(size_t)r * D + k];
  }
  Dev h, g1, b1, slab, bias, wsc, ro, ss, out, kc, vc;
  if (c.ht) HT_(h.in(h4.size() * 4, h4.data())); else HT_(h.in((size_t)c.rows * D * 4, c.h));
  if (c.epi == DEC_LOGITS) { HT_(g1.in((size_t)D * 4, c.g1)); HT_(b1.in((size_t)D * 4, c.b1)); }
  HT_(slab.in(c.slab_bytes, c.slab));
  HT_(bias.in((size_t)c.N * 4, c.bias));
  if (c.split == 3) HT_(wsc.in((size_t)c.N * 4, c.wscale));
  if (c.ro) HT_(ro.in((size_t)tiles * 16 * 4, c.row_off));
  const StepState hs{c.n_past, 0};
  HT_(ss.in(sizeof hs, &hs));
  HT_(out.alloc(out_elems * 4, TTS_DEC_TEST_SENTINEL));
  if (cache_bytes) { HT_(kc.alloc(cache_bytes, TTS_DEC_TEST_SENTINEL)); HT_(vc.alloc(cache_bytes, TTS_DEC_TEST_SENTINEL)); }
  DecLnArgs a{h.as<float>(), g1.as<float>(), b1.as<float>(), c.split == 0 ? slab.as<float>() : nullptr, c.split ? slab.as<__half>() : nullptr, bias.as<float>(),
              c.rows, c.n_valid, c.ldo, c.prefill_B, out.as<float>(), kc.as<__half>(), vc.as<__half>(),
              c.prefill_B > 0 ? nullptr : ss.as<StepState>(), c.max_pos, c.lut, wsc.as<float>(), ro.as<int>()}; // the prompt pass has no step state
  const dim3 grid(c.N / 16, tiles);
  hipStream_t s;
  HT_(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    if (c.epi == DEC_QKV) ln_dispatch<DEC_QKV>(c, grid, s, a);
    else if (c.epi == DEC_GELU) ln_dispatch<DEC_GELU>(c, grid, s, a);
    else ln_dispatch<DEC_LOGITS>(c, grid, s, a);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  if (e != hipSuccess || es != hipSuccess) return (int)(e != hipSuccess ? e : es);
  HT_(out.get_all(c.out));
  if (cache_bytes) { HT_(kc.get_all(c.kc)); HT_(vc.get_all(c.vc)); }
  const bool ok = h.margins_intact() && g1.margins_intact() && b1.margins_intact() && slab.margins_intact() && bias.margins_intact() && wsc.margins_intact() &&
                  ro.margins_intact() && ss.margins_intact();
  return ok ? 0 : (int)TTS_DEC_TEST_ERR_CANARY;
}

int tts_dec_test_resid(const tts_dec_resid_case *cp) {
  if (!cp || !resid_valid(*cp)) return (int)hipErrorInvalidValue;
  const tts_dec_resid_case &c = *cp;
  const int tiles = (c.rows + 15) / 16, K = 1024 * c.kg;
  std::vector<float> h4;
  if (c.ht) {
    h4.assign((size_t)tiles * 16 * D, std::nanf(""));
    for (int r = 0; r < c.rows; r++)
      for (int k = 0; k < D; k++) h4[h4_index(r, k)] = c.h_in[(size_t)r * D + k];
  }
  Dev X, slab, bias, wsc, h;
  HT_(X.in((size_t)c.rows * K * 4, c.X));
  HT_(slab.in(c.slab_bytes, c.slab));
  HT_(bias.in((size_t)D * 4, c.bias));
  if (c.wh == 2) HT_(wsc.in((size_t)D * 4, c.wscale));
  HT_(h.alloc(c.ht ? h4.size() * 4 : (size_t)c.rows * D * 4, TTS_DEC_TEST_SENTINEL)); // in and out: its margins keep the sentinel
  HT_(hipMemcpy(h.data(), c.ht ? h4.data() : c.h_in, h.bytes, hipMemcpyHostToDevice));
  const float *dX = X.as<float>(), *dW = slab.as<float>(), *db = bias.as<float>(), *dsc = wsc.as<float>();
  float *dh = h.as<float>();
  const dim3 grid(D / 4, tiles);
  hipStream_t s;
  HT_(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) {
    const int key = c.kg * 100 + c.wh * 10 + c.ht; // (ntw follows from ht and wh: resid_valid)
    switch (key) {
      case 100: dec_gemv_resid_kernel<1><<<grid, 256, 0, s>>>(dX, c.rows, dW, db, dh); break;
      case 400: dec_gemv_resid_kernel<4, 512><<<grid, 512, 0, s>>>(dX, c.rows, dW, db, dh); break;
      case 101: dec_gemv_resid_kernel<1, 256, 0, true, true><<<grid, 256, 0, s>>>(dX, c.rows, dW, db, dh); break;
      case 111: dec_gemv_resid_kernel<1, 256, 1, false, true><<<grid, 256, 0, s>>>(dX, c.rows, dW, db, dh); break;
      case 121: dec_gemv_resid_kernel<1, 256, 2, false, true><<<grid, 256, 0, s>>>(dX, c.rows, dW, db, dh, dsc); break;
      case 401: dec_gemv_resid_kernel<4, 512, 0, true, true><<<grid, 512, 0, s>>>(dX, c.rows, dW, db, dh); break;
      case 411: dec_gemv_resid_kernel<4, 512, 1, false, true><<<grid, 512, 0, s>>>(dX, c.rows, dW, db, dh); break;
      default: dec_gemv_resid_kernel<4, 512, 2, false, true><<<grid, 512, 0, s>>>(dX, c.rows, dW, db, dh, dsc); break;
    }
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  if (e != hipSuccess || es != hipSuccess) return (int)(e != hipSuccess ? e : es);
  HT_(h.get_all(c.h_out));
  const bool ok = X.margins_intact() && slab.margins_intact() && bias.margins_intact() && wsc.margins_intact();
  return ok ? 0 : (int)TTS_DEC_TEST_ERR_CANARY;
}

} // extern "C"
