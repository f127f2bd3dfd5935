// Test-only harness around csrc/gemm_f8.h (included unchanged): the weight packer, the activation quantiser and the fp8 k = 3 convolution, host arrays in, host
// arrays out, ONE launch at a time on a stream of its own. Built as libtts_gemm_f8_test.so next to the product library; links nothing from it and is not part of it
// (tests/test_gemm_f8_kernels_gpu.py, tests/test_conv3_fp8_cpu.py and tools/conv3_fp8_bench.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE anything is launched (shapes, leading dimensions, the packed layout the quantiser relies on, every
// pointer), and the convolution's output carries a canary margin in front and behind, inside the same allocation, that is copied back with the payload.
#include "../csrc/gemm_f8.h"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;

namespace {

enum { MARGIN = 4096, SENTINEL = 0xCB };

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * MARGIN);
  }
  char *data() const { return p + MARGIN; }
  hipError_t put(const void *h, size_t n, size_t off = 0) { return hipMemcpy(data() + off, h, n, hipMemcpyHostToDevice); }
  hipError_t get(void *h, size_t n) const { return hipMemcpy(h, data(), n, hipMemcpyDeviceToHost); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * MARGIN, hipMemcpyDeviceToHost); }
};

// the packed layout of diffusion.hip: starts at multiples of 8, at least one guard row in front of and behind every sequence, inside M rows (a multiple of 8)
bool layout_ok(int M, int ns, const int *start, const int *len) {
  if (M < 8 || (M & 7) || M > (1 << 20) || ns < 1 || ns > 4096 || !start || !len) return false;
  int prev_end = 0; // first row the next sequence may NOT use is prev_end (its guard)
  for (int s = 0; s < ns; s++) {
    if (len[s] < 1 || (start[s] & 7) || start[s] < 8 || start[s] <= prev_end || start[s] + len[s] >= M) return false;
    prev_end = start[s] + len[s];
  }
  return true;
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int run_on_stream(hipError_t (*f)(void *, hipStream_t), void *arg) {
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills ran on the null stream
  if (e == hipSuccess) e = f(arg, s);
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  return (int)(e != hipSuccess ? e : es);
}

} // namespace

extern "C" {

int tts_f8_test_margin(void) { return MARGIN; }
long long tts_f8_test_wfrag_index(int n, int tap, int k, int N, int K) { return (long long)gemm_f8_wfrag_index(n, tap, k, N, K); }
float tts_f8_test_scale(float amax) { return f8_pow2_scale(amax); }
int tts_f8_test_takes(int conv3_fp8, int images, int stats, int debug_sums, int M, int N, int K) { return gemm_f8_conv3_takes(conv3_fp8, images != 0, stats != 0, debug_sums != 0, M, N, K); }

// the loader's packer (host only): W [N][3][K] f32 -> img [3 N K] bytes, inv_w [N]
int tts_f8_test_pack(const float *W, int N, int K, uint8_t *img, float *inv_w) {
  if (!W || !img || !inv_w || N < 16 || (N & 15) || K < 128 || (K & 127) || N > 4096 || K > 4096) return (int)hipErrorInvalidValue;
  gemm_f8_pack_weight(W, N, K, img, inv_w);
  return 0;
}

// the quantiser: A [M][C] fp16 (rows 0 .. M - 1 of the packed layout, guard rows as the caller left them) -> A8 [M][C] bytes, inv_a [M]; the amax launch, then
// the convert launch
int tts_f8_test_quant(const uint16_t *A, int M, int Cn, int ns, const int *start, const int *len, uint8_t *A8, float *inv_a) {
  if (!A || !A8 || !inv_a || Cn < 8 || (Cn & 7) || Cn > 4096 || !layout_ok(M, ns, start, len)) return (int)hipErrorInvalidValue;
  std::vector<int> rs(M, -1);
  for (int s = 0; s < ns; s++)
    for (int t = 0; t < len[s]; t++) rs[start[s] + t] = s;
  Dev a, a8, ia, part, dst, dln, drs;
  const size_t ab = (size_t)M * Cn * 2;
  HT(a.alloc(ab, 0)); HT(a.put(A, ab));
  HT(a8.alloc((size_t)M * Cn, SENTINEL)); HT(ia.alloc((size_t)M * 4, SENTINEL)); HT(part.alloc((size_t)ns * F8_AMAX_PARTS * 4, SENTINEL));
  HT(dst.alloc((size_t)ns * 4, 0)); HT(dst.put(start, (size_t)ns * 4));
  HT(dln.alloc((size_t)ns * 4, 0)); HT(dln.put(len, (size_t)ns * 4));
  HT(drs.alloc((size_t)M * 4, 0xFF)); HT(drs.put(rs.data(), (size_t)M * 4));
  QuantF8Args q{};
  q.A = (const __half *)a.data(); q.lda = Cn; q.C = Cn; q.M = M; q.ns = ns;
  q.seq_start = (const int *)dst.data(); q.seq_len = (const int *)dln.data(); q.row_seq = (const int *)drs.data();
  q.part = (unsigned *)part.data(); q.A8 = (uint8_t *)a8.data(); q.lda8 = Cn; q.inv_a = (float *)ia.data();
  int rc = run_on_stream([](void *p, hipStream_t s) { return launch_quant_f8_amax(*(const QuantF8Args *)p, s); }, &q);
  if (rc) return rc;
  rc = run_on_stream([](void *p, hipStream_t s) { return launch_quant_f8_convert(*(const QuantF8Args *)p, s); }, &q);
  if (rc) return rc;
  HT(a8.get(A8, (size_t)M * Cn)); HT(ia.get(inv_a, (size_t)M * 4));
  return 0;
}

// the convolution on caller-supplied bytes and scales. A8 holds M + 2 rows of K bytes (rows -1 .. M of the packed layout), Wimg the per-tap images, out
// MARGIN + M * N * 4 + MARGIN bytes: pre-filled with the sentinel (with the residual when resid_aliases_out), one launch, all of it copied back
struct tts_f8_conv3_case {
  int M, rows_total, N, K, resid_aliases_out;
  const uint8_t *A8, *Wimg;
  const float *inv_a, *inv_w, *bias, *resid; // bias, resid: may be null; resid [M][N]
  const int *row_seq;                        // may be null
  float *out;
};
int tts_f8_test_conv3(const tts_f8_conv3_case *cp) {
  if (!cp) return (int)hipErrorInvalidValue;
  const tts_f8_conv3_case &c = *cp;
  if (!gemm_f8_conv3_shape(c.M, c.N, c.K) || c.M > 65536 || c.N > 4096 || c.K > 4096 || c.rows_total < 1 || c.rows_total > c.M || !c.A8 || !c.Wimg || !c.inv_a ||
      !c.inv_w || !c.out || (c.resid_aliases_out && !c.resid))
    return (int)hipErrorInvalidValue;
  Dev a, w, ia, iw, bias, resid, rseq, out;
  const size_t ab = (size_t)(c.M + 2) * c.K, fb = (size_t)c.M * c.N * 4;
  HT(a.alloc(ab, 0)); HT(a.put(c.A8, ab));
  HT(w.alloc((size_t)3 * c.N * c.K, 0)); HT(w.put(c.Wimg, (size_t)3 * c.N * c.K));
  HT(ia.alloc((size_t)c.M * 4, 0)); HT(ia.put(c.inv_a, (size_t)c.M * 4));
  HT(iw.alloc((size_t)c.N * 4, 0)); HT(iw.put(c.inv_w, (size_t)c.N * 4));
  HT(out.alloc(fb, SENTINEL));
  GemmF8Args g{};
  g.A8 = (const uint8_t *)a.data() + c.K; g.lda = c.K; g.Wf = (const uint8_t *)w.data(); // row 0 = second row of the buffer
  g.inv_a = (const float *)ia.data(); g.inv_w = (const float *)iw.data();
  if (c.bias) { HT(bias.alloc((size_t)c.N * 4, 0)); HT(bias.put(c.bias, (size_t)c.N * 4)); g.bias = (const float *)bias.data(); }
  if (c.row_seq) { HT(rseq.alloc((size_t)c.M * 4, 0xFF)); HT(rseq.put(c.row_seq, (size_t)c.M * 4)); g.row_seq = (const int *)rseq.data(); }
  g.out = (float *)out.data(); g.ldo = c.N;
  if (c.resid && c.resid_aliases_out) { HT(out.put(c.resid, fb)); g.resid = g.out; }
  else if (c.resid) { HT(resid.alloc(fb, 0)); HT(resid.put(c.resid, fb)); g.resid = (const float *)resid.data(); }
  g.M = c.M; g.rows_total = c.rows_total; g.N = c.N; g.K = c.K;
  const int rc = run_on_stream([](void *p, hipStream_t s) { return launch_gemm_f8_conv3(*(const GemmF8Args *)p, s); }, &g);
  HT(out.get_all(c.out)); // the output comes back also after a refusal: the caller checks that nothing was written
  return rc;
}

} // extern "C"
