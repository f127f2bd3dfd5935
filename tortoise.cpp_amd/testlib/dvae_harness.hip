// Test-only harness around the DVAE encoder's kernels (csrc/dvae.h, which csrc/hifigan.hip includes through bigvgan.h, classifier.h and aligner.h; hifigan.hip is
// included here whole and unchanged): host arrays in, host arrays out, one launch (the strided layer: cls_down_kernel and its ReLU; the quantiser: its kernel
// and the slab reduce) per call on a stream of its own, through the dvae_launch_* functions dvae_run itself calls. Built as libtts_dvae_test.so next to the
// product library (together with csrc/host_logic.cpp, which the host half calls); it is not part of the product (tests/test_dvae_kernels_gpu.py and
// tests/test_dvae_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (the clip tables, every address the chosen kernel reads or writes), and every device
// buffer carries a canary margin in front and behind, inside the same allocation, that is copied back with the payload; the margins of the input buffers hold NaNs.
#include "../csrc/hifigan.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_DVAE_TEST_MARGIN = 4096, TTS_DVAE_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { POISON = 0xFF }; // the margins of every INPUT buffer: a float read outside the payload is a NaN and shows in the output
enum { TTS_DVAE_TEST_STEM = 0, TTS_DVAE_TEST_DOWN = 1, TTS_DVAE_TEST_VQ = 2 };
// caps, sized by the case matrix of tests/dvae_ref.py (the full-size quantiser case: 65 rows x 512 channels against 512 x 8192)
enum { TTS_DVAE_TEST_MAX_CLIPS = 4, TTS_DVAE_TEST_MAX_ROWS = 1 << 12, TTS_DVAE_TEST_MAX_FLOATS = 1 << 23 };

// One case. Host pointers only. `out` (and `out2`) hold TTS_DVAE_TEST_MARGIN bytes, the payload, TTS_DVAE_TEST_MARGIN bytes; the payload starts as the sentinel.
//   n      [ns] frames (STEM) or rows (DOWN) of every clip; the HFG_SEQ tables are built from it by dvae_levels, which dvae_begin calls: first row = the running sum of the rows,
//          first mel float = cin x the running sum of the frames; the output rows of a clip are (n - 1) / stride + 1. VQ: unused (ns = 1).
//   STEM   in = the mels back to back, clip s band-major [cin][n[s]]; w [taps][cin][cout], bias [cout]; out f32 [rows_out][cout]
//   DOWN   in [rows][cin]; w [taps][cin][cout], bias [cout]; out f32 [rows_out][cout] = ReLU(Conv1d(stride, pad (taps - 1) / 2))
//   VQ     in = z [rows][cin] (cin = dim), w = E [dim][cout] (cout = tokens), bias = |E_j|^2 [tokens] or null (then dvae_code_norms makes it); out int32 [rows]
//          codes; out2 f32 [rows] the minimum itself
struct tts_dvae_case {
  int kind, ns, rows, cin, cout, taps, stride, rows_out;
  const int *n;
  const float *in, *w, *bias;
  void *out, *out2;
};

int tts_dvae_test_margin(void) { return TTS_DVAE_TEST_MARGIN; }
int tts_dvae_test_stem_tile(void) { return DVS_ROWS; }
int tts_dvae_test_down_tile(void) { return CLS_DTM; }
int tts_dvae_test_vq_tile(void) { return DVQ_TM; }
int tts_dvae_test_vq_slab(void) { return DVQ_SLAB; }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_DVAE_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_DVAE_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_DVAE_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_DVAE_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

struct Plan { std::vector<int> seq, seq_out; int max_out = 0; int64_t in_floats = 0; };

bool valid(const tts_dvae_case &c, Plan &p) {
  if (c.kind < TTS_DVAE_TEST_STEM || c.kind > TTS_DVAE_TEST_VQ) return false;
  if (!c.out || !c.in || !c.w) return false;
  if (c.kind == TTS_DVAE_TEST_VQ) { // z[(r0 + r) D + q], r0 + r < rows; E[k N + j], j < N (N a multiple of 32); pv / pi [slab][rows]; LDS 64 (D + 1) floats + 2 KB
    if (!c.out2 || c.ns != 1) return false;
    if (c.rows < 1 || c.rows > TTS_DVAE_TEST_MAX_ROWS) return false;
    if (c.cin < 32 || c.cin % 32 || c.cin > DVAE_MAX_DIM) return false;
    if (c.cout < 32 || c.cout % 32 || c.cout > DVAE_MAX_TOKENS) return false;
    return (int64_t)c.cin * c.cout <= TTS_DVAE_TEST_MAX_FLOATS;
  }
  if (!c.bias || !c.n) return false;
  if (c.ns < 1 || c.ns > TTS_DVAE_TEST_MAX_CLIPS) return false; // every kernel indexes the tables with blockIdx.y < ns
  if (c.taps < 1 || c.taps > DVAE_MAX_K || c.taps % 2 == 0 || c.stride < 1 || c.stride > DVAE_MAX_STRIDE) return false;
  if (!dvae_channels_ok(c.cout)) return false;
  if (c.kind == TTS_DVAE_TEST_STEM ? (c.cin < 1 || c.cin > DVAE_MAX_CIN) : !dvae_channels_ok(c.cin)) return false; // DOWN: float4 loads of 32-channel chunks
  for (int s = 0; s < c.ns; s++)
    if (c.n[s] < 1 || c.n[s] > TTS_DVAE_TEST_MAX_ROWS) return false;
  const LevelTable t = dvae_levels(c.n, c.ns, 1, c.stride, c.cin); // the function dvae_begin calls, for one strided layer
  p.seq.assign(t.rec(0, 0), t.rec(0, 0) + (size_t)HFG_SEQ * c.ns); p.seq_out.assign(t.rec(1, 0), t.rec(1, 0) + (size_t)HFG_SEQ * c.ns);
  p.max_out = t.max_n[1];
  const int64_t ri = t.rows[0], ro = t.rows[1];
  if (ri != c.rows || ro != c.rows_out) return false; // the buffers hold exactly the clips
  p.in_floats = ri * c.cin;
  return p.in_floats <= TTS_DVAE_TEST_MAX_FLOATS && ro * c.cout <= TTS_DVAE_TEST_MAX_FLOATS;
}

} // namespace

extern "C" {

// 0 for a case tts_dvae_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_dvae_test_validate(const tts_dvae_case *c) {
  Plan p;
  return c && valid(*c, p) ? 0 : (int)hipErrorInvalidValue;
}

// dvae_begin's tables for clips of n[s] mel frames of cin channels behind L strided layers (host only): tab [L + 1][ns][9], rows / max_n [L + 1]
int tts_dvae_test_levels(const int *n, int ns, int L, int stride, int cin, int *tab, long long *rows, int *max_n) {
  if (!n || !tab || !rows || !max_n || ns < 1 || L < 0 || stride < 1 || cin < 1) return (int)hipErrorInvalidValue;
  const LevelTable t = dvae_levels(n, ns, L, stride, cin);
  memcpy(tab, t.tab.data(), t.tab.size() * sizeof(int));
  for (int l = 0; l <= L; l++) { rows[l] = t.rows[l]; max_n[l] = t.max_n[l]; }
  return 0;
}

// The loader's host half on a model file (no HIP call): its status, and for TTS_OK out[0 .. 6] = strided layers, ResBlocks, mel channels, hidden channels,
// codebook dim, tokens, stride. err (cap bytes) receives the message of a refusal.
int tts_dvae_test_parse(const char *path, int *out7, char *err, int cap) {
  tts_ctx ctx;
  WeightFile wf;
  std::string e;
  std::unique_ptr<DvaeHost> h(new DvaeHost());
  int rc = read_weight_file(path, wf, e);
  if (rc != TTS_OK) fail(&ctx, rc, "dvae_load: %s", e.c_str());
  else rc = dvae_parse(&ctx, wf, path, *h);
  if (err && cap > 0) { strncpy(err, ctx.err.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
  if (rc == TTS_OK && out7) {
    const int v[7] = {h->L, h->blocks, h->cin, h->H, h->dim, h->N, h->stride};
    memcpy(out7, v, sizeof v);
  }
  return rc;
}

// One packed tensor of the parsed model (host only), for the tests of the repack: which = 0 down[i].w, 1 res[i / 3][i % 3].w, 2 head.w, 3 E, 4 |E_j|^2.
// Returns the element count (copies at most cap floats), or a TTS status.
long long tts_dvae_test_packed(const char *path, int which, int i, float *out, long long cap) {
  tts_ctx ctx;
  WeightFile wf;
  std::string e;
  std::unique_ptr<DvaeHost> h(new DvaeHost());
  int rc = read_weight_file(path, wf, e);
  if (rc == TTS_OK) rc = dvae_parse(&ctx, wf, path, *h);
  if (rc != TTS_OK) return rc;
  const std::vector<float> *v = nullptr;
  if (which == 0 && i >= 0 && i < h->L) v = &h->down[i].w;
  else if (which == 1 && i >= 0 && i < 3 * h->blocks) v = &h->res[i / 3][i % 3].w;
  else if (which == 2) v = &h->head.w;
  else if (which == 3) v = &h->E;
  else if (which == 4) v = &h->e2;
  if (!v) return TTS_ERR_ARG;
  if (out) memcpy(out, v->data(), (size_t)std::min<long long>(cap, (long long)v->size()) * 4);
  return (long long)v->size();
}

// |E_j|^2 as the loader makes it (host only)
int tts_dvae_test_code_norms(const float *E, int dim, int tokens, float *e2) {
  if (!E || !e2 || dim < 1 || tokens < 1) return (int)hipErrorInvalidValue;
  dvae_code_norms(E, dim, tokens, e2);
  return 0;
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_dvae_test_run(const tts_dvae_case *cp) {
  Plan p;
  if (!cp || !valid(*cp, p)) return (int)hipErrorInvalidValue;
  const tts_dvae_case &c = *cp;
  Dev in, out, out2, w, bias, dseq, dseq_out, pv, pi;
  hipStream_t s;
  hipError_t e = hipSuccess;
  if (c.kind == TTS_DVAE_TEST_VQ) {
    const int R = c.rows, D = c.cin, N = c.cout, slabs = dvae_vq_slabs(N);
    std::vector<float> e2((size_t)N);
    if (c.bias) memcpy(e2.data(), c.bias, (size_t)N * 4);
    else dvae_code_norms(c.w, D, N, e2.data());
    HT(in.alloc((size_t)R * D * 4, POISON)); HT(in.put(c.in));
    HT(w.alloc((size_t)D * N * 4, POISON)); HT(w.put(c.w));
    HT(bias.alloc((size_t)N * 4, POISON)); HT(bias.put(e2.data()));
    HT(pv.alloc((size_t)slabs * R * 4, TTS_DVAE_TEST_SENTINEL)); HT(pi.alloc((size_t)slabs * R * 4, TTS_DVAE_TEST_SENTINEL));
    HT(out.alloc((size_t)R * 4, TTS_DVAE_TEST_SENTINEL)); HT(out2.alloc((size_t)R * 4, TTS_DVAE_TEST_SENTINEL));
    HT(hipDeviceSynchronize()); // the fills above ran on the null stream
    HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    DvaeVq q{};
    q.z = (const float *)in.data(); q.E = (const float *)w.data(); q.e2 = (const float *)bias.data(); q.pv = (float *)pv.data(); q.pi = (int *)pi.data();
    q.R = R; q.D = D; q.N = N;
    e = dvae_launch_vq(q, (int *)out.data(), (float *)out2.data(), s);
  } else {
    const int B = c.ns;
    HT(dseq.alloc(p.seq.size() * 4, 0)); HT(dseq.put(p.seq.data()));
    HT(dseq_out.alloc(p.seq_out.size() * 4, 0)); HT(dseq_out.put(p.seq_out.data()));
    HT(in.alloc((size_t)p.in_floats * 4, POISON)); HT(in.put(c.in));
    HT(w.alloc((size_t)c.taps * c.cin * c.cout * 4, POISON)); HT(w.put(c.w));
    HT(bias.alloc((size_t)c.cout * 4, POISON)); HT(bias.put(c.bias));
    HT(out.alloc((size_t)c.rows_out * c.cout * 4, TTS_DVAE_TEST_SENTINEL));
    HT(hipDeviceSynchronize());
    HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (c.kind == TTS_DVAE_TEST_STEM) {
      DvaeStem a{};
      a.mel = (const float *)in.data(); a.out = (float *)out.data(); a.w = (const float *)w.data(); a.bias = (const float *)bias.data();
      a.seq_in = (const int *)dseq.data(); a.seq_out = (const int *)dseq_out.data();
      a.cin = c.cin; a.cout = c.cout; a.taps = c.taps; a.stride = c.stride; a.pad = (c.taps - 1) / 2;
      dvae_launch_stem(a, p.max_out, B, s);
    } else {
      ClsDown d{};
      d.in = (const float *)in.data(); d.out = (float *)out.data(); d.w = (const float *)w.data(); d.bias = (const float *)bias.data();
      d.seq_in = (const int *)dseq.data(); d.seq_out = (const int *)dseq_out.data();
      d.cin = c.cin; d.cout = c.cout; d.taps = c.taps; d.stride = c.stride; d.pad = (c.taps - 1) / 2;
      dvae_launch_down(d, d.seq_out, p.max_out, B, s);
    }
  }
  if (e == hipSuccess) e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  if (c.kind == TTS_DVAE_TEST_VQ) HT(out2.get_all(c.out2));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
