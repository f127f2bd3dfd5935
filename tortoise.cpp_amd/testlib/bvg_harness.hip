// Test-only harness around the BigVGAN vocoder's kernels (csrc/bigvgan.h, which csrc/hifigan.hip includes as its last line; hifigan.hip is included here whole
// and unchanged): host arrays in, host arrays out, one launch per call on a stream of its own. bigvgan_run launches its kernels inline, so the grid and block
// expressions are restated here, spelled as in bigvgan.h (tests/test_bvg_harness_cpu.py compares them). Built as libtts_bvg_test.so next to the product library
// (together with csrc/host_logic.cpp, which the host half calls); it is not part of the product (tests/test_bvg_kernels_gpu.py and
// tests/test_bvg_harness_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (the candidate table, every address the chosen kernel reads or writes), and every device
// buffer carries a canary margin in front and behind, inside the same allocation, that is copied back with the payload.
#include "../csrc/hifigan.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_BVG_TEST_MARGIN = 4096, TTS_BVG_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_BVG_TEST_ACT = 0, TTS_BVG_TEST_MEL = 1, TTS_BVG_TEST_POST = 2 };
// caps, sized by the case matrix of tests/bvg_cases.py: three candidates on 48 frames, 128 channels, 12 288 rows in a buffer
enum { TTS_BVG_TEST_MAX_CAND = 3, TTS_BVG_TEST_MAX_FRAMES = 48, TTS_BVG_TEST_MAX_ROWS = 48 * 256, TTS_BVG_TEST_MAX_CH = 128, TTS_BVG_TEST_MAX_RATE = 1024 };

// One case. Host pointers only. `out` holds TTS_BVG_TEST_MARGIN bytes, the payload, TTS_BVG_TEST_MARGIN bytes; the payload starts as the sentinel.
//   T        [ns] frames of every candidate. The HFG_SEQ table is built from it by bigvgan_run's rule: start = the running sum of ceil8(T), frames before =
//            the running sum of T.
//   start    null, or [ns] start frames that replace the running sum (validated: multiples of 8, in order, no overlap, inside `frames`)
//   frames   frames of every row buffer (a multiple of 8, at least the end of the last candidate)
//   ACT      in [frames*rate][C], alpha [C], inv_beta [C]; out f32 [frames*rate][C]
//   MEL      in = mel, candidates back to back, [100][T] each; out f32 [frames][128]
//   POST     in = x [frames*256][C], w [7][C], bias [1], alpha [C], inv_beta [C]; out f32 [sum T * 256]
struct tts_bvg_case {
  int kind, ns, frames, C, rate;
  const int *T, *start;
  const float *in, *w, *bias, *alpha, *inv_beta;
  void *out;
};

int tts_bvg_test_margin(void) { return TTS_BVG_TEST_MARGIN; }
int tts_bvg_test_run_rows(void) { return BVG_RUN; }                // rows one thread of bvg_act_kernel walks
int tts_bvg_test_block_rows(void) { return BVG_ACT_RUNS * BVG_RUN; } // rows of one of its workgroups

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_BVG_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_BVG_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_BVG_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_BVG_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

int ceil8(int v) { return (v + 7) / 8 * 8; }

bool valid(const tts_bvg_case &c, std::vector<int> &seq, int &maxT, int64_t &total) {
  if (c.kind < TTS_BVG_TEST_ACT || c.kind > TTS_BVG_TEST_POST) return false;
  if (!c.out || !c.in || !c.T) return false;
  // every kernel indexes seq with blockIdx.y < ns
  if (c.ns < 1 || c.ns > TTS_BVG_TEST_MAX_CAND) return false;
  if (c.frames < 8 || c.frames % 8 || c.frames > TTS_BVG_TEST_MAX_FRAMES) return false;
  seq.assign((size_t)HFG_SEQ * c.ns, 0);
  int64_t fpad = 0;
  maxT = 0; total = 0;
  for (int s = 0; s < c.ns; s++) {
    const int T = c.T[s];
    if (T < 1 || T > c.frames) return false; // rows [start * R, (start + T) * R): at least one, inside the buffer
    int64_t start = fpad;
    if (c.start) {
      start = c.start[s];
      if (start % 8 || start < fpad) return false; // no layout bigvgan_run builds; an overlap lets two workgroups write the same rows
    }
    if (start + ceil8(T) > c.frames) return false;
    int *q = &seq[(size_t)HFG_SEQ * s];
    q[0] = (int)start; q[1] = T; q[5] = (int)total; q[8] = T; // bigvgan_run's record
    total += T; fpad = start + ceil8(T); maxT = std::max(maxT, T);
  }
  if (c.kind == TTS_BVG_TEST_MEL) return true; // reads mel[before * 100 + ch * T + t], writes out[(f0 + t) * 128 + ch], t < T: inside by the table
  // alpha[c], inv_beta[c] for c < C; rows of C floats, channel blockIdx.z * 32 + lane % 32 (ACT) or c0 + lane % 32 (POST): whole groups of 32
  if (!c.alpha || !c.inv_beta) return false;
  if (c.C < 32 || c.C % 32 || c.C > TTS_BVG_TEST_MAX_CH) return false;
  if (c.kind == TTS_BVG_TEST_POST) return c.w && c.bias && (int64_t)c.frames * 256 <= TTS_BVG_TEST_MAX_ROWS; // w[tap * C + c], b[0]; x rows f0 * 256 + t, t < T * 256
  // rows (f0 * rate + t) of in / out, t < T * rate
  if (c.rate < 1 || c.rate > TTS_BVG_TEST_MAX_RATE || (int64_t)c.frames * c.rate > TTS_BVG_TEST_MAX_ROWS) return false;
  return true;
}

} // namespace

extern "C" {

// 0 for a case tts_bvg_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_bvg_test_validate(const tts_bvg_case *c) {
  std::vector<int> seq;
  int a;
  int64_t t;
  return c && valid(*c, seq, a, t) ? 0 : (int)hipErrorInvalidValue;
}

// the HFG_SEQ table the harness builds for a case (host only), [ns][9] into `out`; hipErrorInvalidValue for a refused case
int tts_bvg_test_table(const tts_bvg_case *c, int *out) {
  std::vector<int> seq;
  int a;
  int64_t t;
  if (!c || !out || !valid(*c, seq, a, t)) return (int)hipErrorInvalidValue;
  memcpy(out, seq.data(), seq.size() * sizeof(int));
  return 0;
}

// The loader's host half on a model file (no HIP call): its status, and for TTS_OK out[0] = C0, out[1] = stages, out[2 .. 7] = strides, out[8 .. 14] = the padded
// channel counts after conv_pre and after every stage. err (cap bytes) receives the message of a refusal.
int tts_bvg_test_parse(const char *path, int *out15, char *err, int cap) {
  tts_ctx ctx;
  WeightFile wf;
  std::string e;
  std::unique_ptr<BvgHost> h(new BvgHost());
  int rc = read_weight_file(path, wf, e);
  if (rc != TTS_OK) fail(&ctx, rc, "bigvgan_load: %s", e.c_str());
  else rc = bigvgan_parse(&ctx, wf, path, *h);
  if (err && cap > 0) { strncpy(err, ctx.err.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
  if (rc == TTS_OK && out15) {
    out15[0] = h->c0; out15[1] = h->n_stages;
    for (int i = 0; i < BVG_MAX_STAGES; i++) out15[2 + i] = h->up[i];
    for (int i = 0; i <= BVG_MAX_STAGES; i++) out15[8 + i] = h->ch[i];
  }
  return rc;
}

// One packed tensor of the parsed model (host only), for the tests of the repack and the padding: which = 0 conv_pre.w, 1 ups[i].w, 2 c1[i][j][n].w,
// 3 c2[i][j][n].w, 4 act[i][j][n].alpha, 5 act[i][j][n].inv_beta, 6 conv_post.w, 7 ups[i].b. Returns the element count (copies at most cap floats), or a TTS status.
long long tts_bvg_test_packed(const char *path, int which, int i, int j, int n, float *out, long long cap) {
  tts_ctx ctx;
  WeightFile wf;
  std::string e;
  std::unique_ptr<BvgHost> h(new BvgHost());
  int rc = read_weight_file(path, wf, e);
  if (rc == TTS_OK) rc = bigvgan_parse(&ctx, wf, path, *h);
  if (rc != TTS_OK) return rc;
  if (i < 0 || i >= h->n_stages || j < 0 || j > 2 || n < 0 || n > (which == 4 || which == 5 ? 5 : 2)) return TTS_ERR_ARG;
  const std::vector<float> *v = which == 0 ? &h->pre.w : which == 1 ? &h->ups[i].w : which == 2 ? &h->c1[i][j][n].w : which == 3 ? &h->c2[i][j][n].w :
                                which == 4 ? &h->act[i][j][n].w : which == 5 ? &h->act[i][j][n].b : which == 6 ? &h->post.w : which == 7 ? &h->ups[i].b : nullptr;
  if (!v) return TTS_ERR_ARG;
  if (out) memcpy(out, v->data(), (size_t)std::min<long long>(cap, (long long)v->size()) * 4);
  return (long long)v->size();
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_bvg_test_run(const tts_bvg_case *cp) {
  std::vector<int> seq;
  int maxT = 0;
  int64_t total = 0;
  if (!cp || !valid(*cp, seq, maxT, total)) return (int)hipErrorInvalidValue;
  const tts_bvg_case &c = *cp;
  Dev in, out, w, bias, al, ib, dseq;
  const int B = c.ns, C = c.C, rate = c.rate;
  size_t in_bytes = 0, out_bytes = 0;
  switch (c.kind) {
    case TTS_BVG_TEST_ACT: in_bytes = out_bytes = (size_t)c.frames * rate * C * 4; break;
    case TTS_BVG_TEST_MEL: in_bytes = (size_t)total * BVG_MEL * 4; out_bytes = (size_t)c.frames * BVG_MEL_PAD * 4; break;
    default: in_bytes = (size_t)c.frames * 256 * C * 4; out_bytes = (size_t)total * 256 * 4; break;
  }
  HT(in.alloc(in_bytes, 0)); HT(in.put(c.in));
  HT(dseq.alloc(seq.size() * 4, 0)); HT(dseq.put(seq.data()));
  if (c.kind != TTS_BVG_TEST_MEL) { HT(al.alloc((size_t)C * 4, 0)); HT(al.put(c.alpha)); HT(ib.alloc((size_t)C * 4, 0)); HT(ib.put(c.inv_beta)); }
  if (c.kind == TTS_BVG_TEST_POST) { HT(w.alloc((size_t)7 * C * 4, 0)); HT(w.put(c.w)); HT(bias.alloc(4, 0)); HT(bias.put(c.bias)); }
  HT(out.alloc(out_bytes, TTS_BVG_TEST_SENTINEL));
  const float *din = (const float *)in.data();
  const int *d_seq = (const int *)dseq.data();
  float *dy = (float *)out.data();
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    switch (c.kind) {
      case TTS_BVG_TEST_ACT: {
        const dim3 grid((unsigned)(((size_t)maxT * rate + BVG_ACT_RUNS * BVG_RUN - 1) / (BVG_ACT_RUNS * BVG_RUN)), (unsigned)B, (unsigned)(C / 32));
        bvg_act_kernel<<<grid, 256, 0, s>>>(din, dy, (const float *)al.data(), (const float *)ib.data(), d_seq, C, rate);
        break;
      }
      case TTS_BVG_TEST_MEL:
        bvg_mel_kernel<<<dim3(maxT, B), 128, 0, s>>>(din, d_seq, dy);
        break;
      default:
        bvg_post_kernel<<<dim3(maxT, B), 256, 0, s>>>(din, (const float *)w.data(), (const float *)bias.data(), (const float *)al.data(), (const float *)ib.data(), d_seq, dy, C);
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
