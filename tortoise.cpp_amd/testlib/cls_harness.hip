// Test-only harness around the classifier's kernels (csrc/classifier.h, which csrc/hifigan.hip includes through the last line of csrc/bigvgan.h; hifigan.hip is included here whole and
// unchanged): host arrays in, host arrays out, one launch (the GroupNorm trio: its three) per call on a stream of its own, through the cls_launch_* functions
// classifier_run itself calls. Built as libtts_cls_test.so next to the product library (together with csrc/host_logic.cpp, which the host half calls); it is not
// part of the product (tests/test_cls_kernels_gpu.py and tests/test_cls_harness_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (the clip tables, every address the chosen kernel reads or writes), and every device
// buffer carries a canary margin in front and behind, inside the same allocation, that is copied back with the payload.
#include "../csrc/hifigan.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_CLS_TEST_MARGIN = 4096, TTS_CLS_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_CLS_TEST_STEM = 0, TTS_CLS_TEST_GN = 1, TTS_CLS_TEST_DOWN = 2, TTS_CLS_TEST_ATTN = 3, TTS_CLS_TEST_HEAD = 4 };
// caps, sized by the case matrix of tests/cls_cases.py
enum { TTS_CLS_TEST_MAX_CLIPS = 4, TTS_CLS_TEST_MAX_ROWS = 4096, TTS_CLS_TEST_MAX_FLOATS = 1 << 21 };

// One case. Host pointers only. `out` holds TTS_CLS_TEST_MARGIN bytes, the payload, TTS_CLS_TEST_MARGIN bytes; the payload starts as the sentinel.
//   n        [ns] rows of every clip. The HFG_SEQ table is built from it by cls_levels, which classifier_run calls: first row = the running sum of ceil8(n),
//            first GroupNorm tile = the running sum of ceil(n / tile), first sample = the first row.
//   start    null, or [ns] first rows that replace the running sum (validated: multiples of 8, in order, no overlap, inside `rows`)
//   rows     rows of the input buffer (a multiple of 8)
//   STEM     in = samples [rows], clip s at start[s]; w [C][3], bias [C]; out f32 [rows][C]
//   GN       in [rows][C], gamma [C], beta [C]; out f32 [rows][C]; stat null or f64 [ns][G][2] = {mean, 1 / sqrt(var + eps)}
//   DOWN     in [rows][C], w [taps][C][C2], bias [C2]; out f32 [rows_out][C2], clip s at start_out[s] (null: the running sum) with (n - 1) / stride + 1 rows
//   ATTN     in = qkv [rows][3 C] (C = E; q | k | v, head h at columns h * C / heads of each); out f32 [rows][C]
//   HEAD     in = x [rows][C], w [2][C], bias [2]; out f32 [ns][3]
struct tts_cls_case {
  int kind, ns, rows, C, C2, taps, stride, heads, rows_out;
  const int *n, *start, *start_out;
  const float *in, *w, *bias, *gamma, *beta;
  void *out;
  double *stat;
};

int tts_cls_test_margin(void) { return TTS_CLS_TEST_MARGIN; }
int tts_cls_test_gn_tile(void) { return CLS_GN_TILE; }
int tts_cls_test_down_tile(void) { return CLS_DTM; }
int tts_cls_test_stem_tile(void) { return CLS_STEM_ROWS; }
int tts_cls_test_groups(int C) { return C >= 1 ? cls_groups(C) : 0; }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_CLS_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_CLS_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_CLS_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_CLS_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

int ceil8(int v) { return (v + 7) / 8 * 8; }

// the table of `n` rows per clip inside a buffer of `rows` rows: level 0 of cls_levels, the function classifier_run calls, with `start` in the place of its
// first rows; false: a layout classifier_run never builds
bool table(const int *n, const int *start, int ns, int rows, std::vector<int> &seq, int &max_n, int &tiles) {
  for (int s = 0; s < ns; s++)
    if (n[s] < 1 || n[s] > rows) return false;
  LevelTable t = cls_levels(n, ns, 0, 1);
  int64_t next = 0;
  for (int s = 0; s < ns; s++) {
    int *q = &t.tab[(size_t)HFG_SEQ * s];
    if (start) {
      if (start[s] % 8 || start[s] < next) return false; // an overlap lets two workgroups write the same rows
      q[0] = q[4] = start[s];
    }
    next = (int64_t)q[0] + ceil8(n[s]);
    if (next > rows) return false;
  }
  seq.swap(t.tab); max_n = t.max_n[0]; tiles = (int)t.tiles[0];
  return true;
}

struct Plan { std::vector<int> seq, seq_out, n_out; int max_n = 0, tiles = 0, max_out = 0, tiles_out = 0; };

bool valid(const tts_cls_case &c, Plan &p) {
  if (c.kind < TTS_CLS_TEST_STEM || c.kind > TTS_CLS_TEST_HEAD) return false;
  if (!c.out || !c.in || !c.n) return false;
  if (c.ns < 1 || c.ns > TTS_CLS_TEST_MAX_CLIPS) return false; // every kernel indexes the table with blockIdx.y (HEAD: blockIdx.x) < ns
  if (c.rows < 8 || c.rows % 8 || c.rows > TTS_CLS_TEST_MAX_ROWS) return false;
  if (!cls_pow2_channels(c.C) || (int64_t)c.rows * c.C > TTS_CLS_TEST_MAX_FLOATS) return false; // float4 columns, C / 4 threads per row, 1024 / C rows per pass
  if (!table(c.n, c.start, c.ns, c.rows, p.seq, p.max_n, p.tiles)) return false;
  switch (c.kind) {
    case TTS_CLS_TEST_STEM: return c.w && c.bias;                       // w[c * 3 + k], b[c]; x[first sample + i], 0 <= i < n
    case TTS_CLS_TEST_GN: return c.gamma && c.beta;                     // gamma, beta as float4 at 4 q < C; part[(first tile + tile) * G + g], stat[s * G + g]
    case TTS_CLS_TEST_HEAD: return c.w && c.bias;                       // x[first row * C + c], w[c], w[C + c]
    case TTS_CLS_TEST_DOWN: {
      if (!c.w || !c.bias) return false;
      if (c.C2 < 64 || c.C2 % 64 || c.C2 > 2 * CLS_MAX_C) return false; // column group blockIdx.z * 64 + 32 (wave >> 1) + lane % 32
      if (c.taps < 1 || c.taps > 11 || c.taps % 2 == 0 || c.stride < 2 || c.stride > 6) return false;
      if (cls_down_lds(c.taps, c.stride) > 64 * 1024) return false;
      if (c.rows_out < 8 || c.rows_out % 8 || c.rows_out > TTS_CLS_TEST_MAX_ROWS || (int64_t)c.rows_out * c.C2 > TTS_CLS_TEST_MAX_FLOATS) return false;
      const LevelTable two = cls_levels(c.n, c.ns, 1, c.stride); // the Downsample's output rows, as classifier_run counts them
      p.n_out.resize(c.ns);
      for (int s = 0; s < c.ns; s++) p.n_out[s] = two.rec(1, s)[1];
      return table(p.n_out.data(), c.start_out, c.ns, c.rows_out, p.seq_out, p.max_out, p.tiles_out);
    }
    default: // ATTN: qkv[(first row + t) * 3 C + {0, C, 2 C} + h * DH + d], out[(first row + t) * C + h * DH + d], t < n, h < heads, d < DH = 64 or 128
      if (c.heads < 1 || c.C % c.heads || (c.C / c.heads != 64 && c.C / c.heads != 128)) return false;
      return (int64_t)c.rows * 3 * c.C <= TTS_CLS_TEST_MAX_FLOATS;
  }
}

} // namespace

extern "C" {

// 0 for a case tts_cls_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_cls_test_validate(const tts_cls_case *c) {
  Plan p;
  return c && valid(*c, p) ? 0 : (int)hipErrorInvalidValue;
}

// the HFG_SEQ tables the harness builds for a case (host only): [ns][9] of the input into `in_tab`, of the output (DOWN; else untouched) into `out_tab`
int tts_cls_test_table(const tts_cls_case *c, int *in_tab, int *out_tab) {
  Plan p;
  if (!c || !in_tab || !valid(*c, p)) return (int)hipErrorInvalidValue;
  memcpy(in_tab, p.seq.data(), p.seq.size() * sizeof(int));
  if (out_tab && !p.seq_out.empty()) memcpy(out_tab, p.seq_out.data(), p.seq_out.size() * sizeof(int));
  return 0;
}

// classifier_run's tables for clips of n[s] samples at 24 kHz (host only): tab [depth + 1][ns][9], rows / tiles / max_n [depth + 1]
int tts_cls_test_levels(const int *n, int ns, int depth, int F, int *tab, long long *rows, long long *tiles, int *max_n) {
  if (!n || !tab || !rows || !tiles || !max_n || ns < 1 || depth < 0 || F < 1) return (int)hipErrorInvalidValue;
  const LevelTable t = cls_levels(n, ns, depth, F);
  memcpy(tab, t.tab.data(), t.tab.size() * sizeof(int));
  for (int l = 0; l <= depth; l++) { rows[l] = t.rows[l]; tiles[l] = t.tiles[l]; max_n[l] = t.max_n[l]; }
  return 0;
}

// The loader's host half on a model file (no HIP call): its status, and for TTS_OK out[0 .. 7] = base channels, depth, kernel size, embedding dimension,
// ResBlocks per level, attention blocks, downsample factor, heads. err (cap bytes) receives the message of a refusal.
int tts_cls_test_parse(const char *path, int *out8, char *err, int cap) {
  tts_ctx ctx;
  WeightFile wf;
  std::string e;
  std::unique_ptr<ClsHost> h(new ClsHost());
  int rc = read_weight_file(path, wf, e);
  if (rc != TTS_OK) fail(&ctx, rc, "classifier_load: %s", e.c_str());
  else rc = classifier_parse(&ctx, wf, path, *h);
  if (err && cap > 0) { strncpy(err, ctx.err.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
  if (rc == TTS_OK && out8) {
    const int v[8] = {h->b0, h->depth, h->K, h->E, h->rb, h->n_attn, h->F, h->H};
    memcpy(out8, v, sizeof v);
  }
  return rc;
}

// One packed tensor of the parsed model (host only), for the tests of the repack: which = 0 stem.w, 1 res[i].ca.w, 2 res[i].cb.w, 3 down[i].w, 4 fin.w,
// 5 attn[i].qkv.w, 6 attn[i].qkv.b, 7 head.w, 8 attn[i].proj.w. Returns the element count (copies at most cap floats), or a TTS status.
long long tts_cls_test_packed(const char *path, int which, int i, float *out, long long cap) {
  tts_ctx ctx;
  WeightFile wf;
  std::string e;
  std::unique_ptr<ClsHost> h(new ClsHost());
  int rc = read_weight_file(path, wf, e);
  if (rc == TTS_OK) rc = classifier_parse(&ctx, wf, path, *h);
  if (rc != TTS_OK) return rc;
  const std::vector<float> *v = nullptr;
  if (which == 0) v = &h->stem.w;
  else if ((which == 1 || which == 2) && i >= 0 && i < (int)h->res.size()) v = which == 1 ? &h->res[i].ca.w : &h->res[i].cb.w;
  else if (which == 3 && i >= 0 && i < (int)h->down.size()) v = &h->down[i].w;
  else if (which == 4) v = &h->fin.w;
  else if ((which == 5 || which == 6 || which == 8) && i >= 0 && i < (int)h->attn.size()) v = which == 5 ? &h->attn[i].qkv.w : which == 6 ? &h->attn[i].qkv.b : &h->attn[i].proj.w;
  else if (which == 7) v = &h->head.w;
  if (!v) return TTS_ERR_ARG;
  if (out) memcpy(out, v->data(), (size_t)std::min<long long>(cap, (long long)v->size()) * 4);
  return (long long)v->size();
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_cls_test_run(const tts_cls_case *cp) {
  Plan p;
  if (!cp || !valid(*cp, p)) return (int)hipErrorInvalidValue;
  const tts_cls_case &c = *cp;
  const int B = c.ns, C = c.C, G = cls_groups(C);
  Dev in, out, w, bias, gam, bet, dseq, dseq_out, part, stat;
  size_t in_bytes = (size_t)c.rows * C * 4, out_bytes = in_bytes;
  if (c.kind == TTS_CLS_TEST_STEM) in_bytes = (size_t)c.rows * 4;
  if (c.kind == TTS_CLS_TEST_ATTN) in_bytes = (size_t)c.rows * 3 * C * 4;
  if (c.kind == TTS_CLS_TEST_DOWN) out_bytes = (size_t)c.rows_out * c.C2 * 4;
  if (c.kind == TTS_CLS_TEST_HEAD) out_bytes = (size_t)B * 3 * 4;
  HT(dseq.alloc(p.seq.size() * 4, 0)); HT(dseq.put(p.seq.data()));
  const int *d_seq = (const int *)dseq.data();
  hipStream_t s;
  HT(in.alloc(in_bytes, 0)); HT(in.put(c.in));
  HT(out.alloc(out_bytes, TTS_CLS_TEST_SENTINEL));
  const float *din = (const float *)in.data();
  float *dy = (float *)out.data();
  hipError_t e = hipSuccess;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  switch (c.kind) {
    case TTS_CLS_TEST_STEM: {
      HT(w.alloc((size_t)C * 3 * 4, 0)); HT(w.put(c.w)); HT(bias.alloc((size_t)C * 4, 0)); HT(bias.put(c.bias));
      HT(hipDeviceSynchronize()); // the fills above ran on the null stream
      cls_launch_stem(din, (const float *)w.data(), (const float *)bias.data(), d_seq, C, p.max_n, B, dy, s);
      break;
    }
    case TTS_CLS_TEST_GN: {
      HT(gam.alloc((size_t)C * 4, 0)); HT(gam.put(c.gamma)); HT(bet.alloc((size_t)C * 4, 0)); HT(bet.put(c.beta));
      HT(part.alloc((size_t)p.tiles * G * sizeof(double2), TTS_CLS_TEST_SENTINEL)); HT(stat.alloc((size_t)B * G * sizeof(double2), TTS_CLS_TEST_SENTINEL));
      HT(hipDeviceSynchronize());
      cls_launch_gn_silu(din, dy, (const float *)gam.data(), (const float *)bet.data(), d_seq, C, p.max_n, B, (double2 *)part.data(), (double2 *)stat.data(), s);
      break;
    }
    case TTS_CLS_TEST_DOWN: {
      HT(w.alloc((size_t)c.taps * C * c.C2 * 4, 0)); HT(w.put(c.w)); HT(bias.alloc((size_t)c.C2 * 4, 0)); HT(bias.put(c.bias));
      HT(dseq_out.alloc(p.seq_out.size() * 4, 0)); HT(dseq_out.put(p.seq_out.data()));
      HT(hipDeviceSynchronize());
      ClsDown a{};
      a.in = din; a.out = dy; a.w = (const float *)w.data(); a.bias = (const float *)bias.data(); a.seq_in = d_seq; a.seq_out = (const int *)dseq_out.data();
      a.cin = C; a.cout = c.C2; a.taps = c.taps; a.stride = c.stride; a.pad = (c.taps - 1) / 2;
      cls_launch_down(a, p.max_out, B, s);
      break;
    }
    case TTS_CLS_TEST_HEAD: {
      HT(w.alloc((size_t)2 * C * 4, 0)); HT(w.put(c.w)); HT(bias.alloc(2 * 4, 0)); HT(bias.put(c.bias));
      HT(hipDeviceSynchronize());
      cls_head_kernel<<<B, 64, 0, s>>>(din, d_seq, (const float *)w.data(), (const float *)bias.data(), C, dy);
      break;
    }
    default:
      HT(hipDeviceSynchronize());
      cls_launch_attn(din, dy, d_seq, C, c.heads, p.max_n, B, s);
      break;
  }
  if (e == hipSuccess) e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  if (c.kind == TTS_CLS_TEST_GN && c.stat) HT(hipMemcpy(c.stat, stat.data(), (size_t)B * G * sizeof(double2), hipMemcpyDeviceToHost));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
