// Test-only harness around the AR scoring kernels (csrc/ar_score.h, which csrc/ar.hip includes; ar.hip is included here whole and unchanged): host arrays in,
// host arrays out, one launch of the kernel pair per call on a stream of its own, through ar_score_launch, the function the engine itself calls. Built as
// libtts_score_test.so next to the product library (together with csrc/host_logic.cpp, which ar.hip's host half calls); it is not part of the product
// (tests/test_ar_score_kernels_gpu.py and tests/test_ar_score_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (the shape the kernel tiles, every target), and every device buffer carries a canary
// margin in front and behind, inside the same allocation, that is copied back with the payload; the margins of the input buffers hold NaNs.
#include "../csrc/ar.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_SCORE_TEST_MARGIN = 4096, TTS_SCORE_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { POISON = 0xFF }; // the margins of every INPUT buffer: a float read outside the payload is a NaN and shows in the output
// caps, sized by the case matrix of tests/ar_score_cases.py (the full-size head: 1024 x 8256; 130 rows)
enum { TTS_SCORE_TEST_MAX_ROWS = 1 << 12, TTS_SCORE_TEST_MAX_FLOATS = 1 << 24 };

// One case. Host pointers only. hn [R][K]; w [K][NPAD] row-major (the harness lays it out strip-major as the loader does: strip_major); b [NPAD]; tgt [R].
// Every output holds TTS_SCORE_TEST_MARGIN bytes, [R] values, TTS_SCORE_TEST_MARGIN bytes; the payload starts as the sentinel.
struct tts_score_case {
  int R, K, N, NPAD;
  const float *hn, *w, *b;
  const int *tgt;
  void *lse, *logp, *stop_logp, *greedy, *tgt_logit, *stop_logit;
};

int tts_score_test_margin(void) { return TTS_SCORE_TEST_MARGIN; }
int tts_score_test_tile(void) { return ARS_TM; }
int tts_score_test_slab(void) { return ARS_SLAB; }
int tts_score_test_lds(int K) { return K >= 1 && K <= ARS_MAX_K ? (int)ar_score_lds(K) : -1; }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_SCORE_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_SCORE_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_SCORE_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_SCORE_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

// hn[(r0 + r) K + k], r0 + r < R; w strip ((v / 64) K + k) 64 + v % 64 of a 32-column tile that starts below N: below NPAD whole; b[v], v < N; tgt[r] < N so that
// exactly one lane stores the row's target logit; the workspace is sized by ar_score_ws_floats; LDS ar_score_lds(K) <= 160 KB
bool valid(const tts_score_case &c) {
  if (!c.hn || !c.w || !c.b || !c.tgt || !c.lse || !c.logp || !c.stop_logp || !c.greedy || !c.tgt_logit || !c.stop_logit) return false;
  if (c.R < 1 || c.R > TTS_SCORE_TEST_MAX_ROWS) return false;
  if (!ar_score_shape_ok(c.R, c.K, c.N, c.NPAD)) return false;
  if ((int64_t)c.K * c.NPAD > TTS_SCORE_TEST_MAX_FLOATS || c.NPAD - c.N >= 256) return false;
  if (ar_score_lds(c.K) > (size_t)160 * 1024) return false;
  for (int r = 0; r < c.R; r++)
    if (c.tgt[r] < 0 || c.tgt[r] >= c.N) return false;
  return true;
}

} // namespace

extern "C" {

// 0 for a case tts_score_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_score_test_validate(const tts_score_case *c) { return c && valid(*c) ? 0 : (int)hipErrorInvalidValue; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_score_test_run(const tts_score_case *cp) {
  if (!cp || !valid(*cp)) return (int)hipErrorInvalidValue;
  const tts_score_case &c = *cp;
  const size_t R = (size_t)c.R;
  const std::vector<float> ws = strip_major(c.w, c.K, c.NPAD);
  Dev hn, w, b, tgt, work, out[6];
  HT(hn.alloc(R * c.K * 4, POISON)); HT(hn.put(c.hn));
  HT(w.alloc(ws.size() * 4, POISON)); HT(w.put(ws.data()));
  HT(b.alloc((size_t)c.NPAD * 4, POISON)); HT(b.put(c.b));
  HT(tgt.alloc(R * 4, POISON)); HT(tgt.put(c.tgt));
  HT(work.alloc(ar_score_ws_floats(c.R, c.N) * 4, TTS_SCORE_TEST_SENTINEL));
  for (Dev &o : out) HT(o.alloc(R * 4, TTS_SCORE_TEST_SENTINEL));
  HT(hipDeviceSynchronize()); // the fills above ran on the null stream
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  const ArScore a{(const float *)hn.data(), (const float *)w.data(), (const float *)b.data(), (const int *)tgt.data(), (float *)work.data(), c.R, c.K, c.N, c.NPAD};
  const ArScoreOut o{(float *)out[0].data(), (float *)out[1].data(), (float *)out[2].data(), (int *)out[3].data(), (float *)out[4].data(), (float *)out[5].data()};
  const hipError_t e = ar_score_launch(a, o, s);
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  void *host[6] = {c.lse, c.logp, c.stop_logp, c.greedy, c.tgt_logit, c.stop_logit};
  for (int i = 0; i < 6; i++) HT(out[i].get_all(host[i]));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
