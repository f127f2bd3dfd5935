// Test-only harness around the aligner's fp16 Linear (csrc/w2v_linear_h.h, through csrc/hifigan.hip included whole and unchanged): host arrays in, host arrays
// out; one call packs the caller's f32 weight on the device (hfg_pack_launch with pt = 1, as DevWeights::pack does) and runs ONE w2v_linear_h_launch, the launcher
// aligner_run calls, on a stream of its own. Built as libtts_w2v_h_test.so next to the product library; not part of the product
// (tests/test_w2v_linear_h_gpu.py is the only user).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call, and every device buffer carries a canary margin in front and behind, inside the same
// allocation, that is copied back with the output.
#include "../csrc/hifigan.hip"

#include <cstdint>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_W2V_H_MARGIN = 4096, TTS_W2V_H_SENTINEL = 0xCB };
// caps, sized by the cases of tests/test_w2v_linear_h_gpu.py
enum { TTS_W2V_H_MAX_CLIPS = 4, TTS_W2V_H_MAX_ROWS = 1024, TTS_W2V_H_MAX_CH = 1024 };

// n, start: [ns] rows and first row of every clip (start a multiple of 8, in order, no overlap, inside `rows`); in [rows][cin]; w [cin][cout]; bias [cout];
// epi 0 bias, 1 bias + GELU, 2 bias + residual: resid [rows][cout], or alias = 1: the residual is the output buffer, which starts as out0 [rows][cout];
// out: margin | f32 [rows][cout] | margin, the payload starts as the sentinel (as out0 with alias)
struct tts_w2v_h_case {
  int ns, rows, cin, cout, epi, alias, split;
  const int *n, *start;
  const float *in, *w, *bias, *resid, *out0;
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
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_W2V_H_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_W2V_H_MARGIN);
  }
  char *data() const { return p ? p + TTS_W2V_H_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
};

// the HFG_SEQ table of the case, or false: every address the pack kernels and the Linear read or write is checked here or by the launcher itself
bool valid(const tts_w2v_h_case &c, std::vector<int> &seq, int &max_n) {
  if (!c.out || !c.in || !c.w || !c.bias || !c.n || !c.start || c.split < 0 || c.split > 1 || c.alias < 0 || c.alias > 1) return false;
  if (c.ns < 1 || c.ns > TTS_W2V_H_MAX_CLIPS || c.rows < 8 || c.rows % 8 || c.rows > TTS_W2V_H_MAX_ROWS) return false;
  if (c.cin < 16 || c.cin % 16 || c.cin > TTS_W2V_H_MAX_CH || c.cout < 32 || c.cout % 32 || c.cout > TTS_W2V_H_MAX_CH) return false; // what the packer tiles
  if (c.epi == W2V_EPI_RESID ? !(c.alias ? c.out0 : c.resid) : c.alias) return false;
  for (size_t i = 0, n = (size_t)c.cin * c.cout; i < n; i++)
    if (!std::isfinite(c.w[i])) return false; // DevWeights::pack refuses it
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

int tts_w2v_h_test_margin(void) { return TTS_W2V_H_MARGIN; }
int tts_w2v_h_test_scale_exp(void) { return HFG_H_EXP; }
int tts_w2v_h_test_row_tile(void) { return W2V_H_TM; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// 0, a HIP error, or -1: the launcher refused the shape (nothing was launched; the output keeps its fill)
int tts_w2v_h_test_run(const tts_w2v_h_case *cp) {
  std::vector<int> seq;
  int max_n = 0;
  if (!cp || !valid(*cp, seq, max_n)) return (int)hipErrorInvalidValue;
  const tts_w2v_h_case &c = *cp;
  Dev in, out, w, pk, bias, resid, dseq;
  const size_t nw = (size_t)c.cin * c.cout, out_bytes = (size_t)c.rows * c.cout * 4;
  HT(in.alloc((size_t)c.rows * c.cin * 4, 0)); HT(in.put(c.in));
  HT(w.alloc(nw * 4, 0)); HT(w.put(c.w));
  HT(pk.alloc(nw * 4 + (size_t)c.cout * 8, 0)); // hi | lo | scales, as DevWeights::pack lays them out
  HT(bias.alloc((size_t)c.cout * 4, 0)); HT(bias.put(c.bias));
  HT(dseq.alloc(seq.size() * 4, 0)); HT(dseq.put(seq.data()));
  if (c.epi == W2V_EPI_RESID && !c.alias) { HT(resid.alloc(out_bytes, 0)); HT(resid.put(c.resid)); }
  HT(out.alloc(out_bytes, TTS_W2V_H_SENTINEL));
  if (c.alias) HT(out.put(c.out0));
  float *dy = (float *)out.data();
  _Float16 *wh = (_Float16 *)pk.data(), *wl = wh + nw;
  float *ws = (float *)(wl + nw);
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  bool launched = true;
  if (e == hipSuccess) {
    hfg_pack_launch(s, (const float *)w.data(), 1, c.cin, c.cout, wh, wl, ws);
    const W2vLinearH a{(const float *)in.data(), dy, c.alias ? dy : (const float *)resid.data(), (const float *)bias.data(), (const int *)dseq.data(), c.cin, c.cout};
    launched = w2v_linear_h_launch(s, a, wh, wl, ws, c.split != 0, c.epi, max_n, c.ns);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(hipMemcpy(c.out, out.p, out_bytes + 2 * TTS_W2V_H_MARGIN, hipMemcpyDeviceToHost));
  return e != hipSuccess ? (int)e : es != hipSuccess ? (int)es : launched ? 0 : -1;
}

} // extern "C"
