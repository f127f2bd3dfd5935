// Test-only harness around the add-on attention on the fp16 MFMA (csrc/addon_attn_h.h, through csrc/hifigan.hip included whole and unchanged): host arrays in,
// host arrays out; one call runs ONE cls_launch_attn_h, the launcher classifier_run and aligner_run call, on a stream of its own. No kernel and no asm of its
// own. Built as libtts_attn_h_test.so next to the product library; not part of the product (tests/test_addon_attn_kernels_gpu.py is the only user).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call, and every device buffer carries a canary margin in front and behind, inside the same
// allocation, that is copied back with the output.
#include "../csrc/hifigan.hip"

#include <cstdint>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_ATTN_H_MARGIN = 4096, TTS_ATTN_H_SENTINEL = 0xCB };
// caps, sized by the cases of tests/test_addon_attn_kernels_gpu.py
enum { TTS_ATTN_H_MAX_CLIPS = 4, TTS_ATTN_H_MAX_ROWS = 1024, TTS_ATTN_H_MAX_E = 1024 };

// n, start: [ns] rows and first row of every clip (start a multiple of 8, in order, no overlap, inside `rows`); qkv [rows][3 E] = q | k | v;
// out: margin | f32 [rows][E] | margin, the payload starts as the sentinel
struct tts_attn_h_case {
  int ns, rows, E, heads, split;
  const int *n, *start;
  const float *qkv;
  void *out;
};

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_ATTN_H_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_ATTN_H_MARGIN);
  }
  char *data() const { return p ? p + TTS_ATTN_H_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
};

// the HFG_SEQ table of the case, or false: every row the kernel reads or writes lies inside a clip, every clip inside `rows`; the launcher checks the head dimension
bool valid(const tts_attn_h_case &c, std::vector<int> &seq, int &max_n) {
  if (!c.out || !c.qkv || !c.n || !c.start || c.split < 0 || c.split > 1) return false;
  if (c.ns < 1 || c.ns > TTS_ATTN_H_MAX_CLIPS || c.rows < 8 || c.rows % 8 || c.rows > TTS_ATTN_H_MAX_ROWS) return false;
  if (c.heads < 1 || c.E < c.heads || c.E % c.heads || c.E % 4 || c.E > TTS_ATTN_H_MAX_E) return false;
  seq.assign((size_t)HFG_SEQ * c.ns, 0);
  int64_t next = 0;
  max_n = 0;
  for (int s = 0; s < c.ns; s++) {
    if (c.n[s] < 1 || c.start[s] % 8 || c.start[s] < next) return false;
    next = (int64_t)c.start[s] + (c.n[s] + 7) / 8 * 8;
    if (next > c.rows) return false;
    seq[(size_t)HFG_SEQ * s] = c.start[s]; seq[(size_t)HFG_SEQ * s + 1] = c.n[s];
    max_n = std::max(max_n, c.n[s]);
  }
  return true;
}

} // namespace

extern "C" {

int tts_attn_h_test_margin(void) { return TTS_ATTN_H_MARGIN; }
int tts_attn_h_test_query_tile(void) { return AAH_TQ; }
int tts_attn_h_test_key_tile(void) { return AAH_TK; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// 0, a HIP error, or -1: the launcher refused the head dimension (nothing was launched; the output keeps its fill)
int tts_attn_h_test_run(const tts_attn_h_case *cp) {
  std::vector<int> seq;
  int max_n = 0;
  if (!cp || !valid(*cp, seq, max_n)) return (int)hipErrorInvalidValue;
  const tts_attn_h_case &c = *cp;
  Dev in, out, dseq;
  const size_t out_bytes = (size_t)c.rows * c.E * 4;
  HT(in.alloc(out_bytes * 3, 0)); HT(in.put(c.qkv));
  HT(dseq.alloc(seq.size() * 4, 0)); HT(dseq.put(seq.data()));
  HT(out.alloc(out_bytes, TTS_ATTN_H_SENTINEL));
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  bool launched = true;
  if (e == hipSuccess) {
    launched = cls_launch_attn_h((const float *)in.data(), (float *)out.data(), (const int *)dseq.data(), c.E, c.heads, max_n, c.ns, c.split != 0, s);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(hipMemcpy(c.out, out.p, out_bytes + 2 * TTS_ATTN_H_MARGIN, hipMemcpyDeviceToHost));
  return e != hipSuccess ? (int)e : es != hipSuccess ? (int)es : launched ? 0 : -1;
}

} // extern "C"
