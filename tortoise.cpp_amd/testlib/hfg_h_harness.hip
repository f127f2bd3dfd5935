// Test-only harness around the fp16 convolutions of the HiFi-GAN decoder (csrc/hfg_conv_h.h, through csrc/hifigan.hip included whole and unchanged): host arrays in,
// host arrays out; one call packs the caller's f32 weight on the device (hfg_pack_launch, as DevWeights::pack does) and runs ONE hfg_conv_h_launch on a stream of its
// own. Built as libtts_hfg_h_test.so next to the product library; not part of the product (tests/test_hfg_h_kernels_gpu.py is the only user).
//
// The case is hfg_harness.hip's tts_hfg_case, field for field (tests/hfg_cases.py builds it), with kind = 0. The GPU is shared: a case is validated completely BEFORE
// any HIP call, and every device buffer carries a canary margin in front and behind, inside the same allocation, that is copied back with the output.
#include "../csrc/hifigan.hip"

#include <cstdint>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_HFG_H_MARGIN = 4096, TTS_HFG_H_SENTINEL = 0xCB, TTS_HFG_H_CAND = 6 };
// caps, sized by the cases of tests/test_hfg_h_kernels_gpu.py
enum { TTS_HFG_H_MAX_CAND = 3, TTS_HFG_H_MAX_FRAMES = 48, TTS_HFG_H_MAX_ROWS = 48 * 256, TTS_HFG_H_MAX_CH = 1024, TTS_HFG_H_MAX_VOICES = 3 };

struct tts_hfg_case { // testlib/hfg_harness.hip
  int kind, ns, frames, n_voices;
  int cin, cout, taps, dil, phases, rate, acc_mode, alias;
  float slope;
  const int *cand, *start;
  const float *in, *w, *bias, *cbias, *resid, *out0;
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
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_HFG_H_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_HFG_H_MARGIN);
  }
  char *data() const { return p ? p + TTS_HFG_H_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
};

// hifigan_run's candidate table for the case, or false: every address the pack kernels and the convolution read or write is checked here
bool valid(const tts_hfg_case &c, int split, std::vector<int> &seq, int &maxW) {
  if (c.kind != 0 || split < 0 || split > 1 || !c.out || !c.in || !c.w || !c.bias || !c.cand) return false;
  if (c.ns < 1 || c.ns > TTS_HFG_H_MAX_CAND || c.n_voices < 1 || c.n_voices > TTS_HFG_H_MAX_VOICES) return false;
  if (c.frames < 8 || c.frames % 8 || c.frames > TTS_HFG_H_MAX_FRAMES) return false;
  // staging reads float4 in[t * cin + c0 + q] for whole 32-channel chunks; a K step is 16 channels, a column tile 32 (two per workgroup where 64 divides cout)
  if (c.cin < 32 || c.cin % 32 || c.cin > TTS_HFG_H_MAX_CH || c.cout < 32 || c.cout % 32 || c.cout > TTS_HFG_H_MAX_CH) return false;
  if (c.taps < 1 || c.taps > 11 || c.dil < 1 || c.dil > 5) return false;
  if ((c.phases != 1 && c.phases != 2 && c.phases != 8) || (c.phases > 1 && c.taps != 2)) return false;
  if (hfg_conv_h_lds(split != 0, c.taps, c.dil) > 65536) return false; // LDS row (wave * 64 + lr + 32 + tap * dil) < 256 + (taps - 1) dil
  if (c.rate < 1 || c.rate > 512 || (int64_t)c.frames * c.rate * c.phases > TTS_HFG_H_MAX_ROWS) return false;
  if (c.acc_mode < 0 || c.acc_mode > 2 || c.alias < 0 || c.alias > 1 || ((c.acc_mode || c.alias == 1) && !c.out0) || !(c.slope == c.slope)) return false;
  for (size_t i = 0, n = (size_t)c.phases * c.taps * c.cin * c.cout; i < n; i++)
    if (!std::isfinite(c.w[i])) return false; // DevWeights::pack refuses it
  seq.assign((size_t)HFG_SEQ * c.ns, 0);
  int64_t fpad = 0, lat_rows = 0, kept = 0;
  maxW = 0;
  for (int s = 0; s < c.ns; s++) {
    const int *q = c.cand + TTS_HFG_H_CAND * s;
    const int W = q[0], voice = q[1];
    if (W < 1 || W > c.frames || voice < 0 || voice >= c.n_voices) return false; // rows [start, start + W) x rate; cbias[voice * cout + col]
    int64_t start = fpad;
    if (c.start) {
      start = c.start[s];
      if (start % 8 || start < fpad) return false;
    }
    if (start + (W + 7) / 8 * 8 > c.frames) return false;
    int *r = &seq[(size_t)HFG_SEQ * s];
    r[0] = (int)start; r[1] = W; r[2] = voice; r[3] = q[2]; r[4] = (int)lat_rows; r[5] = (int)kept; r[6] = q[3]; r[7] = q[4]; r[8] = q[5];
    lat_rows += q[2]; kept += q[5]; fpad = start + (W + 7) / 8 * 8;
    maxW = std::max(maxW, W);
  }
  return true;
}

} // namespace

extern "C" {

int tts_hfg_h_test_margin(void) { return TTS_HFG_H_MARGIN; }
int tts_hfg_h_test_scale_exp(void) { return HFG_H_EXP; }

// 0 for a case tts_hfg_h_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_hfg_h_test_validate(const tts_hfg_case *c, int split) {
  std::vector<int> seq;
  int m;
  return c && valid(*c, split, seq, m) ? 0 : (int)hipErrorInvalidValue;
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// split 0: hfg_precision 1 (fp16 operands), 1: hfg_precision 2 (hi + lo pairs). `out`: margin | f32 [frames * rate * phases][cout] | margin.
int tts_hfg_h_test_run(const tts_hfg_case *cp, int split) {
  std::vector<int> seq;
  int maxW = 0;
  if (!cp || !valid(*cp, split, seq, maxW)) return (int)hipErrorInvalidValue;
  const tts_hfg_case &c = *cp;
  Dev in, out, w, pk, bias, cbias, resid, dseq;
  const size_t nw = (size_t)c.phases * c.taps * c.cin * c.cout, out_bytes = (size_t)c.frames * c.rate * c.phases * c.cout * 4;
  HT(in.alloc((size_t)c.frames * c.rate * c.cin * 4, 0)); HT(in.put(c.in));
  HT(w.alloc(nw * 4, 0)); HT(w.put(c.w));
  HT(pk.alloc(nw * 4 + (size_t)c.cout * 8, 0)); // hi | lo | scales, as DevWeights::pack lays them out
  HT(bias.alloc((size_t)c.cout * 4, 0)); HT(bias.put(c.bias));
  HT(dseq.alloc(seq.size() * 4, 0)); HT(dseq.put(seq.data()));
  if (c.cbias) { HT(cbias.alloc((size_t)c.n_voices * c.cout * 4, 0)); HT(cbias.put(c.cbias)); }
  if (c.resid && c.alias == 0) { HT(resid.alloc(out_bytes, 0)); HT(resid.put(c.resid)); }
  HT(out.alloc(out_bytes, TTS_HFG_H_SENTINEL));
  if (c.out0) HT(out.put(c.out0));
  float *dy = (float *)out.data();
  _Float16 *wh = (_Float16 *)pk.data(), *wl = wh + nw;
  float *ws = (float *)(wl + nw);
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    hfg_pack_launch(s, (const float *)w.data(), c.phases * c.taps, c.cin, c.cout, wh, wl, ws);
    HfgConv a{}; // as hifigan_run's `conv` fills it
    a.in = (const float *)in.data(); a.out = dy; a.resid = c.alias == 1 ? dy : (const float *)resid.data(); a.w = (const float *)w.data();
    a.bias = (const float *)bias.data(); a.cbias = (const float *)cbias.data(); a.seq = (const int *)dseq.data();
    a.cin = c.cin; a.cout = c.cout; a.taps = c.taps; a.dil = c.dil; a.lo = -c.dil * (c.taps - 1) / 2; a.phases = c.phases; a.pad_t = c.phases / 2; a.rate = c.rate;
    a.slope = c.slope; a.acc_mode = c.acc_mode;
    hfg_conv_h_launch(s, a, wh, wl, ws, split != 0, (size_t)maxW * c.rate, c.ns);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(hipMemcpy(c.out, out.p, out_bytes + 2 * TTS_HFG_H_MARGIN, hipMemcpyDeviceToHost));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
