// Test-only harness around launch_gemm_f16 (csrc/gemm_f16.h, included unchanged): host arrays in, host arrays out, one launch on a stream of its own.
// Built as libtts_gemm_test.so next to the product library; links nothing from it and is not part of it (tests/test_gemm_kernels_gpu.py and tests/test_gemm_wreg_k3_*.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE anything is launched (shapes, every pointer the chosen mode reads or writes, leading dimensions,
// the rows -1 and M the k = 3 kernel reads, the ">= 128 N / 128 M bytes" the epilogue's dummy loads need), and every device buffer carries a canary margin in
// front and behind, inside the same allocation, that is copied back with the payload.
#include "../csrc/gemm_f16.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tts;

extern "C" {

enum { TTS_GEMM_TEST_MARGIN = 4096, TTS_GEMM_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with

// Plain mirror of GemmArgs. Host pointers only. Activation buffers hold M + 2 rows of lda halves: rows -1 .. M of the packed layout (the product allocates its
// operands the same way); segment seg reads buffer a_sel[seg]. Output buffers hold TTS_GEMM_TEST_MARGIN bytes, the payload, TTS_GEMM_TEST_MARGIN bytes:
//   outF [M][ldo] f32, outH / outH2 [M][ldh] f16, outVt / outVt2 [N / 192 * 64][ldvt] f16, st [FX_STRIPES][st_stripe_ll] int64.
// The harness pre-fills them with the sentinel byte (st: zeros; outF: the residual when resid_aliases_out), launches `launches` times and copies all of it back.
struct tts_gemm_case {
  int M, N, nseg, kseg;
  int row_off[3], a_sel[3];
  int mode, th, ku, wreg, dual_b, custom_w, ldw, w_off[3];
  float alpha;
  int has_bias, has_resid, resid_aliases_out, has_row_seq, has_chunk_seq, has_st;
  int lda, ldo, ldh, ldvt, nseq, st_stripe_ll, launches;
  const uint16_t *A0, *A1, *W;
  const float *bias, *resid; // resid [M][ldo]
  const int *row_seq, *chunk_seq;
  float *outF;
  uint16_t *outH, *outH2, *outVt, *outVt2;
  long long *st;
};

int tts_gemm_test_margin(void) { return TTS_GEMM_TEST_MARGIN; }
int tts_gemm_test_auto_th(int M, int N) { return gemm_auto_th(M, N); }
long long tts_gemm_test_wfrag3_index(int n, int tap, int k, int N, int K) { return (long long)gemm_wfrag3_index(n, tap, k, N, K); } // where the loader puts tap `tap` of W[n][tap * K + k]

} // extern "C"

namespace {

char g_last[160] = "none";

GemmArgs host_args(const tts_gemm_case &c) { // the fields the dispatcher reads; pointers are placeholders that only carry the aliasing structure
  static const __half dummy[2] = {};
  GemmArgs g;
  memset(&g, 0, sizeof g);
  for (int s = 0; s < 3; s++) {
    g.A[s] = dummy + (c.a_sel[s] ? 1 : 0);
    g.row_off[s] = c.row_off[s];
    g.w_off_[s] = c.w_off[s];
  }
  g.nseg = c.nseg; g.kseg = c.kseg; g.lda = c.lda; g.custom_w = c.custom_w; g.ldw_ = c.ldw;
  g.wreg = c.wreg; g.M = c.M; g.N = c.N; g.ldo = c.ldo; g.ldh = c.ldh; g.ldvt = c.ldvt; g.alpha = c.alpha;
  g.st_stripe_ll = c.st_stripe_ll; g.dual_b = c.dual_b; g.mode = c.mode; g.th = c.th; g.ku = c.ku;
  return g;
}

// What launch_gemm_f16 does with these arguments, in the words of its own plan (g.Wf must be set where an image exists).
void describe(const GemmArgs &g, char *buf, int cap) {
  static const char *const names[] = {"vh", "dualb", "conv3", "wreg", "conv3w"};
  const GemmPlan p = gemm_plan(g);
  snprintf(buf, cap, "%s mode=%d th=%d ku=%d cn=%d", names[p.kernel], g.mode, p.th, p.ku, p.cn);
}

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_GEMM_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_GEMM_TEST_MARGIN);
  }
  char *data() const { return p + TTS_GEMM_TEST_MARGIN; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_GEMM_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

// the k = 3 convolution as the product describes it: three taps of ONE buffer, tap-major weight (gemm_is_conv3 reads the same from GemmArgs)
bool conv3_shape(const tts_gemm_case &c) {
  return c.nseg == 3 && !c.custom_w && !c.a_sel[0] && !c.a_sel[1] && !c.a_sel[2] && c.row_off[0] == -1 && c.row_off[1] == 0 && c.row_off[2] == 1;
}

bool valid(const tts_gemm_case &c, bool run) { // run: the output buffers are needed too (a plan names none)
  if (c.M < 16 || c.M > 131072 || (c.M & 15) || c.N < 128 || c.N > 4096 || (c.N & 127)) return false;
  if (c.nseg < 1 || c.nseg > 3 || c.kseg < 64 || c.kseg > 4096 || (c.kseg & 63)) return false;
  if (c.mode < GEMM_OUT_F32 || c.mode > GEMM_OUT_F32_SCALED_STATS || c.th < 0 || c.th > 8) return false;
  if (!(c.ku == 0 || c.ku == 1 || c.ku == 2 || c.ku == 4) || c.launches < 1 || c.launches > 2) return false;
  // operands: 16-byte DMA pieces, rows -1 .. M present, >= 128 bytes per row (the epilogue reads row_seq's stand-in from A, the bias's from W)
  if (c.lda < c.kseg || c.lda < 64 || (c.lda & 7) || !c.A0 || !c.W) return false;
  for (int s = 0; s < c.nseg; s++) {
    if (c.row_off[s] < -1 || c.row_off[s] > 1) return false;
    if (c.a_sel[s] != 0 && c.a_sel[s] != 1) return false;
    if (c.a_sel[s] == 1 && !c.A1) return false;
  }
  const int ldw = c.custom_w ? c.ldw : c.nseg * c.kseg;
  if (ldw < 64 || (ldw & 7)) return false;
  for (int s = 0; s < c.nseg; s++) {
    const int off = c.custom_w ? c.w_off[s] : s * c.kseg;
    if (off < 0 || (off & 7) || off + c.kseg > ldw) return false;
  }
  if (c.has_bias && !c.bias) return false;
  if (c.has_row_seq && !c.row_seq) return false;
  if (c.has_resid && (!gemm_mode_f32(c.mode) || (!c.resid_aliases_out && !c.resid))) return false;
  if (c.resid_aliases_out && !(c.has_resid && c.resid)) return false; // the aliased output starts from the host's residual
  if (gemm_mode_f32(c.mode)) {
    if ((run && !c.outF) || c.ldo < c.N || (c.ldo & 3)) return false;
  } else if (c.mode == GEMM_OUT_F16) {
    if ((run && !c.outH) || c.ldh < c.N || (c.ldh & 3)) return false;
  } else { // Q | K rows of 128 per head, V transposed: whole heads only
    if (c.N % 384) return false;
    if ((run && (!c.outH || !c.outVt)) || c.ldh < c.N / 192 * 128 || (c.ldh & 3) || c.ldvt < c.M || (c.ldvt & 3)) return false;
    if (run && c.mode == GEMM_OUT_QKV_SPLIT && (!c.outH2 || !c.outVt2)) return false;
  }
  if (gemm_mode_stats(c.mode) && (c.has_st || c.has_chunk_seq)) {
    // a (sequence, group) record is indexed seq * 32 + column / 32: at most 32 groups
    if (c.N > 1024 || c.nseq < 1) return false;
    if (c.has_st && ((run && !c.st) || (c.st_stripe_ll > 0 && c.st_stripe_ll < c.nseq * 32 * 4))) return false;
    if (c.has_chunk_seq) {
      if (!c.chunk_seq) return false;
      for (int i = 0; i < c.M / 8; i++)
        if (c.chunk_seq[i] < -1 || c.chunk_seq[i] >= c.nseq) return false;
    }
  }
  return true;
}

} // namespace

extern "C" {

// the kernel / th / ku / cn the launcher selects for a case, without running it (host only: gemm_plan)
static int plan_case(const tts_gemm_case *c, char *buf, int cap, bool images) {
  if (!c || !buf || cap <= 0 || !valid(*c, false)) return (int)hipErrorInvalidValue;
  GemmArgs g = host_args(*c);
  static const __half wf_placeholder[1] = {};
  if (c->wreg && ((c->nseg == 1 && !c->custom_w) || (images && conv3_shape(*c)))) g.Wf = wf_placeholder;
  describe(g, buf, cap);
  return 0;
}
int tts_gemm_test_plan(const tts_gemm_case *c, char *buf, int cap) { return plan_case(c, buf, cap, false); }
// the plan of tts_gemm_test_run_images: a case with wreg set also has the per-tap image of a k = 3 weight
int tts_gemm_test_plan_images(const tts_gemm_case *c, char *buf, int cap) { return plan_case(c, buf, cap, true); }

int tts_gemm_test_last_kernel(char *buf, int cap) {
  if (!buf || cap <= 0) return (int)hipErrorInvalidValue;
  snprintf(buf, cap, "%s", g_last);
  return 0;
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

static int run_case(const tts_gemm_case *cp, bool images) {
  if (!cp || !valid(*cp, true)) return (int)hipErrorInvalidValue;
  const tts_gemm_case &c = *cp;
  const int ldw = c.custom_w ? c.ldw : c.nseg * c.kseg;
  const size_t a_bytes = (size_t)(c.M + 2) * c.lda * 2, w_bytes = (size_t)c.N * ldw * 2;
  const size_t f_bytes = (size_t)c.M * c.ldo * 4, h_bytes = (size_t)c.M * c.ldh * 2, vt_bytes = (size_t)(c.N / 192 * 64) * c.ldvt * 2;
  const size_t st_bytes = (size_t)FX_STRIPES * (c.st_stripe_ll > 0 ? c.st_stripe_ll : 0) * 8;
  Dev a0, a1, w, wf, bias, resid, rseq, cseq, outF, outH, outH2, outVt, outVt2, st;
  GemmArgs g = host_args(c);
  HT(a0.alloc(a_bytes, 0)); HT(a0.put(c.A0));
  if (c.A1) { HT(a1.alloc(a_bytes, 0)); HT(a1.put(c.A1)); }
  HT(w.alloc(w_bytes, 0)); HT(w.put(c.W));
  for (int s = 0; s < 3; s++) g.A[s] = (const __half *)((c.a_sel[s] && s < c.nseg ? a1 : a0).data()) + c.lda; // row 0 = second row of the buffer
  g.W = (const __half *)w.data();
  if (c.wreg && c.nseg == 1 && !c.custom_w) {
    std::vector<uint16_t> img((size_t)c.N * c.kseg);
    for (int n = 0; n < c.N; n++)
      for (int k = 0; k < c.kseg; k++) img[gemm_wfrag_index(n, k, c.kseg)] = c.W[(size_t)n * c.kseg + k];
    HT(wf.alloc(w_bytes, 0)); HT(wf.put(img.data()));
    g.Wf = (const __half *)wf.data();
  } else if (images && c.wreg && conv3_shape(c)) { // one fragment-major image per tap, as the loader builds them
    std::vector<uint16_t> img((size_t)c.N * 3 * c.kseg);
    for (int n = 0; n < c.N; n++)
      for (int tap = 0; tap < 3; tap++)
        for (int k = 0; k < c.kseg; k++) img[gemm_wfrag3_index(n, tap, k, c.N, c.kseg)] = c.W[((size_t)n * 3 + tap) * c.kseg + k];
    HT(wf.alloc(w_bytes, 0)); HT(wf.put(img.data()));
    g.Wf = (const __half *)wf.data();
  }
  if (c.has_bias) { HT(bias.alloc((size_t)c.N * 4, 0)); HT(bias.put(c.bias)); g.bias = (const float *)bias.data(); }
  if (c.has_row_seq) { HT(rseq.alloc((size_t)c.M * 4, 0xFF)); HT(rseq.put(c.row_seq)); g.row_seq = (const int *)rseq.data(); }
  if (gemm_mode_f32(c.mode)) {
    HT(outF.alloc(f_bytes, TTS_GEMM_TEST_SENTINEL));
    g.outF = (float *)outF.data();
    if (c.has_resid && c.resid_aliases_out) { HT(outF.put(c.resid)); g.resid = g.outF; }
    else if (c.has_resid) { HT(resid.alloc(f_bytes, 0)); HT(resid.put(c.resid)); g.resid = (const float *)resid.data(); }
  } else {
    HT(outH.alloc(h_bytes, TTS_GEMM_TEST_SENTINEL));
    g.outH = (__half *)outH.data();
    if (gemm_mode_qkv(c.mode)) { HT(outVt.alloc(vt_bytes, TTS_GEMM_TEST_SENTINEL)); g.outVt = (__half *)outVt.data(); }
    if (c.mode == GEMM_OUT_QKV_SPLIT) {
      HT(outH2.alloc(h_bytes, TTS_GEMM_TEST_SENTINEL)); HT(outVt2.alloc(vt_bytes, TTS_GEMM_TEST_SENTINEL));
      g.outH2 = (__half *)outH2.data(); g.outVt2 = (__half *)outVt2.data();
    }
  }
  if (gemm_mode_stats(c.mode)) {
    if (c.has_st && st_bytes) {
      HT(st.alloc(st_bytes, TTS_GEMM_TEST_SENTINEL)); HT(hipMemset(st.data(), 0, st_bytes));
      g.st_out = (long long *)st.data();
    }
    if (c.has_chunk_seq) { HT(cseq.alloc((size_t)c.M / 8 * 4, 0xFF)); HT(cseq.put(c.chunk_seq)); g.chunk_seq = (const int *)cseq.data(); }
  }
  describe(g, g_last, sizeof g_last);
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  for (int l = 0; l < c.launches && e == hipSuccess; l++) e = launch_gemm_f16(g, s);
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  // outputs come back also after a refusal: the caller checks that nothing was written
  if (outF.p) HT(outF.get_all(c.outF));
  if (outH.p) HT(outH.get_all(c.outH));
  if (outH2.p) HT(outH2.get_all(c.outH2));
  if (outVt.p) HT(outVt.get_all(c.outVt));
  if (outVt2.p) HT(outVt2.get_all(c.outVt2));
  if (st.p) HT(st.get_all(c.st));
  return (int)(e != hipSuccess ? e : es);
}

int tts_gemm_test_run(const tts_gemm_case *cp) { return run_case(cp, false); }
// tts_gemm_test_run that also builds the per-tap image of a k = 3 weight when the case sets wreg (tts_gemm_test_run keeps such a case on the LDS-staged kernel)
int tts_gemm_test_run_images(const tts_gemm_case *cp) { return run_case(cp, true); }

} // extern "C"
