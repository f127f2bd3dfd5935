// Test-only harness around the strided add-on convolution on the fp16 MFMA (csrc/cls_down_h.h, through csrc/hifigan.hip included whole and unchanged): host arrays
// in, host arrays out; one call packs the caller's f32 weight on the device (hfg_pack_launch with pt = taps, as DevWeights::pack does) and runs ONE
// cls_launch_down_h, the launcher classifier_run and aligner_run call, on a stream of its own. No kernel and no asm of its own. Built as libtts_down_h_test.so
// next to the product library; not part of the product (tests/test_down_h_kernels_gpu.py is the only user).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call, and every device buffer carries a canary margin in front and behind, inside the same
// allocation, that is copied back with the output.
#include "../csrc/hifigan.hip"

#include <cstdint>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_DOWN_H_MARGIN = 4096, TTS_DOWN_H_SENTINEL = 0xCB };
// caps, sized by the cases of tests/test_down_h_kernels_gpu.py
enum { TTS_DOWN_H_MAX_CLIPS = 4, TTS_DOWN_H_MAX_ROWS = 2048, TTS_DOWN_H_MAX_CH = 1024 };

// n, start: [ns] input rows and first input row of every clip; n_out, start_out: the same for the output (a start a multiple of 8, in order, no overlap, inside
// rows / rows_out); in_ [rows][cin]; w [taps][cin][cout]; bias [cout]; out: margin | f32 [rows_out][cout] | margin, the payload starts as the sentinel
struct tts_down_h_case {
  int ns, rows, rows_out, cin, cout, taps, stride, pad, split;
  const int *n, *start, *n_out, *start_out;
  const float *in, *w, *bias;
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
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_DOWN_H_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_DOWN_H_MARGIN);
  }
  char *data() const { return p ? p + TTS_DOWN_H_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
};

// one level's HFG_SEQ records, or false: every clip inside `rows`
bool table(int ns, const int *n, const int *start, int rows, std::vector<int> &seq, int &max_n) {
  if (!n || !start || rows < 8 || rows % 8 || rows > TTS_DOWN_H_MAX_ROWS) return false;
  seq.assign((size_t)HFG_SEQ * ns, 0);
  int64_t next = 0;
  max_n = 0;
  for (int s = 0; s < ns; s++) {
    if (n[s] < 1 || start[s] % 8 || start[s] < next) return false;
    next = (int64_t)start[s] + (n[s] + 7) / 8 * 8;
    if (next > rows) return false;
    seq[(size_t)HFG_SEQ * s] = start[s]; seq[(size_t)HFG_SEQ * s + 1] = n[s];
    max_n = std::max(max_n, n[s]);
  }
  return true;
}

// the two tables of the case, or false: every row the kernel reads lies inside a clip of `in` (it predicates on the clip's rows), every row it writes inside a clip
// of `out`; the pack kernels read whole [taps][cin][cout] and write cin / 16 x cout / 32 fragments; the launcher checks what the kernel tiles
bool valid(const tts_down_h_case &c, std::vector<int> &seq_in, std::vector<int> &seq_out, int &max_out) {
  if (!c.out || !c.in || !c.w || !c.bias || c.split < 0 || c.split > 1 || c.ns < 1 || c.ns > TTS_DOWN_H_MAX_CLIPS) return false;
  if (c.cin < 32 || c.cin % 32 || c.cin > TTS_DOWN_H_MAX_CH || c.cout < 32 || c.cout % 32 || c.cout > TTS_DOWN_H_MAX_CH) return false;
  if (c.taps < 1 || c.taps > 16 || c.stride < 1 || c.stride > 8 || c.pad < 0 || c.pad > 16) return false;
  for (size_t i = 0, n = (size_t)c.taps * c.cin * c.cout; i < n; i++)
    if (!std::isfinite(c.w[i])) return false; // DevWeights::pack refuses it
  int max_in;
  return table(c.ns, c.n, c.start, c.rows, seq_in, max_in) && table(c.ns, c.n_out, c.start_out, c.rows_out, seq_out, max_out);
}

} // namespace

extern "C" {

int tts_down_h_test_margin(void) { return TTS_DOWN_H_MARGIN; }
int tts_down_h_test_row_tile(void) { return CDH_TM; }
int tts_down_h_test_scale_exp(void) { return HFG_H_EXP; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// 0, a HIP error, or -1: the launcher refused the shape (nothing was launched; the output keeps its fill)
int tts_down_h_test_run(const tts_down_h_case *cp) {
  std::vector<int> seq_in, seq_out;
  int max_out = 0;
  if (!cp || !valid(*cp, seq_in, seq_out, max_out)) return (int)hipErrorInvalidValue;
  const tts_down_h_case &c = *cp;
  Dev in, out, w, pk, bias, dsi, dso;
  const size_t nw = (size_t)c.taps * c.cin * c.cout, out_bytes = (size_t)c.rows_out * c.cout * 4;
  HT(in.alloc((size_t)c.rows * c.cin * 4, 0)); HT(in.put(c.in));
  HT(w.alloc(nw * 4, 0)); HT(w.put(c.w));
  HT(pk.alloc(nw * 4 + (size_t)c.cout * 8, 0)); // hi | lo | scales, as DevWeights::pack lays them out
  HT(bias.alloc((size_t)c.cout * 4, 0)); HT(bias.put(c.bias));
  HT(dsi.alloc(seq_in.size() * 4, 0)); HT(dsi.put(seq_in.data()));
  HT(dso.alloc(seq_out.size() * 4, 0)); HT(dso.put(seq_out.data()));
  HT(out.alloc(out_bytes, TTS_DOWN_H_SENTINEL));
  _Float16 *wh = (_Float16 *)pk.data(), *wl = wh + nw;
  float *ws = (float *)(wl + nw);
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  bool launched = true;
  if (e == hipSuccess) {
    hfg_pack_launch(s, (const float *)w.data(), c.taps, c.cin, c.cout, wh, wl, ws);
    ClsDown d{}; // as classifier_run and aligner_run fill it
    d.in = (const float *)in.data(); d.out = (float *)out.data(); d.w = (const float *)w.data(); d.bias = (const float *)bias.data();
    d.seq_in = (const int *)dsi.data(); d.seq_out = (const int *)dso.data();
    d.cin = c.cin; d.cout = c.cout; d.taps = c.taps; d.stride = c.stride; d.pad = c.pad;
    launched = cls_launch_down_h(d, wh, wl, ws, c.split != 0, max_out, c.ns, s);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(hipMemcpy(c.out, out.p, out_bytes + 2 * TTS_DOWN_H_MARGIN, hipMemcpyDeviceToHost));
  return e != hipSuccess ? (int)e : es != hipSuccess ? (int)es : launched ? 0 : -1;
}

} // extern "C"
