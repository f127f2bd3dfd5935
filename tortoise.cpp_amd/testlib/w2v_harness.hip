// Test-only harness around the aligner's new kernels (csrc/aligner.h, which csrc/hifigan.hip includes through bigvgan.h and classifier.h; hifigan.hip is included
// here whole and unchanged): host arrays in, host arrays out, one launch (the clip statistics: their two) per call on a stream of its own, through the
// w2v_launch_* functions aligner_run itself calls. Built as libtts_w2v_test.so next to the product library (together with csrc/host_logic.cpp, which the host
// half calls); it is not part of the product (tests/test_w2v_kernels_gpu.py and tests/test_w2v_harness_cpu.py are the only users).
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

enum { TTS_W2V_TEST_MARGIN = 4096, TTS_W2V_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_W2V_TEST_STATS = 0, TTS_W2V_TEST_STEM = 1, TTS_W2V_TEST_LN = 2, TTS_W2V_TEST_POS = 3, TTS_W2V_TEST_HEAD = 4 };
// caps, sized by the case matrix of tests/w2v_cases.py
enum { TTS_W2V_TEST_MAX_CLIPS = 4, TTS_W2V_TEST_MAX_ROWS = 1 << 15, TTS_W2V_TEST_MAX_FLOATS = 1 << 21 };

// One case. Host pointers only. `out` (and `out2`) hold TTS_W2V_TEST_MARGIN bytes, the payload, TTS_W2V_TEST_MARGIN bytes; the payload starts as the sentinel.
//   n        [ns] rows (STATS, STEM: samples) of every clip. The HFG_SEQ table is built from it by w2v_levels, which aligner_run calls: first row = the running
//            sum of ceil8(n), first statistics tile = the running sum of ceil(n / tile), first sample = the first row.
//   start    null, or [ns] first rows that replace the running sum (validated: multiples of 8, in order, no overlap, inside `rows`)
//   rows     rows of the input buffer (a multiple of 8)
//   STATS    in = samples [rows]; out f64 [ns][2] = {mean, 1 / sqrt(unbiased var + 1e-7)}
//   STEM     in = samples [rows], stat f64 [ns][2], w [C][taps], bias [C]; out f32 [rows_out][C], clip s at start_out[s] (null: the running sum) with
//            (n - taps) / stride + 1 rows
//   LN       in [rows][C], gamma [C], beta [C]; mode 0: LayerNorm, 1: LayerNorm + GELU, 2: w2v_gelu_kernel alone (gamma, beta unused); out f32 [rows][C]
//   POS      in [rows][C] (C = D), w [D / C2][taps][C2][C2] (C2 = channels of a group), bias [D]; out f32 [rows][D]
//   HEAD     in [rows][C] (C = D), w [D][C2] (C2 = V), bias [V]; out2 int32 [rows] ids; out f32 [rows][V] logits when mode = 1 (else out is left alone)
struct tts_w2v_case {
  int kind, ns, rows, C, C2, taps, stride, mode, rows_out;
  const int *n, *start, *start_out;
  const float *in, *w, *bias, *gamma, *beta;
  const double *stat;
  void *out, *out2;
};

int tts_w2v_test_margin(void) { return TTS_W2V_TEST_MARGIN; }
int tts_w2v_test_stat_tile(void) { return W2V_ST_TILE; }
int tts_w2v_test_stem_tile(void) { return W2V_STEM_ROWS; }
int tts_w2v_test_pos_tile(void) { return W2V_PTM; }
int tts_w2v_test_head_tile(void) { return W2V_HEAD_ROWS; }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_W2V_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_W2V_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_W2V_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_W2V_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

int ceil8(int v) { return (v + 7) / 8 * 8; }

// the table of `n` rows per clip inside a buffer of `rows` rows: level 0 of w2v_levels, the function aligner_run calls, with `start` in the place of its
// first rows; false: a layout aligner_run never builds
bool table(const int *n, const int *start, int ns, int rows, std::vector<int> &seq, int &max_n, int &tiles) {
  for (int s = 0; s < ns; s++)
    if (n[s] < 1 || n[s] > rows) return false;
  LevelTable t = w2v_levels(n, ns, 0, nullptr, nullptr);
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

bool valid(const tts_w2v_case &c, Plan &p) {
  if (c.kind < TTS_W2V_TEST_STATS || c.kind > TTS_W2V_TEST_HEAD) return false;
  if (!c.out || !c.in || !c.n) return false;
  if (c.ns < 1 || c.ns > TTS_W2V_TEST_MAX_CLIPS) return false; // every kernel indexes the table with blockIdx.y (the finish kernel: blockIdx.x) < ns
  if (c.rows < 8 || c.rows % 8 || c.rows > TTS_W2V_TEST_MAX_ROWS) return false;
  if (!table(c.n, c.start, c.ns, c.rows, p.seq, p.max_n, p.tiles)) return false;
  if (c.kind == TTS_W2V_TEST_STATS) return true; // x[first sample + i], i < n; part[first tile + tile]; stat[s]
  if (!w2v_channels_ok(c.C)) return false;        // lane + 64 i < C, i < 16; float4 columns
  switch (c.kind) {
    case TTS_W2V_TEST_STEM: {
      if (!c.w || !c.bias || !c.stat) return false;
      if (c.taps < 1 || c.taps > 64 || c.stride < 1 || c.stride > 8) return false; // the window: (64 - 1) stride + taps floats of LDS
      if (c.rows_out < 8 || c.rows_out % 8 || c.rows_out > TTS_W2V_TEST_MAX_ROWS || (int64_t)c.rows_out * c.C > TTS_W2V_TEST_MAX_FLOATS) return false;
      p.n_out.resize(c.ns);
      for (int s = 0; s < c.ns; s++) {
        if (c.n[s] < c.taps) return false; // sample (T - 1) stride + taps - 1 < n
        p.n_out[s] = w2v_conv_frames(c.n[s], c.taps, c.stride); // as aligner_run counts them
      }
      return table(p.n_out.data(), c.start_out, c.ns, c.rows_out, p.seq_out, p.max_out, p.tiles_out);
    }
    case TTS_W2V_TEST_LN:
      if (c.mode < 0 || c.mode > 2 || (c.mode < 2 && (!c.gamma || !c.beta))) return false;
      return (int64_t)c.rows * c.C <= TTS_W2V_TEST_MAX_FLOATS;
    case TTS_W2V_TEST_POS: // in[(first row + t) D + g cg + q], t in [0, n); w[((g K + tap) cg + ci) cg + co]; LDS (63 + K) (cg + 1) floats
      if (!c.w || !c.bias) return false;
      if (c.C2 < 64 || c.C2 % 64 || c.C % c.C2 || c.taps < 1 || c.taps > 256 || w2v_pos_lds(c.C2, c.taps) > 64 * 1024) return false;
      return (int64_t)c.rows * c.C <= TTS_W2V_TEST_MAX_FLOATS && (int64_t)c.taps * c.C2 * c.C <= TTS_W2V_TEST_MAX_FLOATS;
    default: // HEAD: x[(first row + t) D + d] staged 8 rows at a time (8 D floats of LDS), w[d V + c], ids[first row + t], logits[(first row + t) V + c]
      if (!c.w || !c.bias || !c.out2) return false;
      if (c.C2 < 1 || c.C2 > W2V_MAX_V || c.mode < 0 || c.mode > 1) return false;
      return (int64_t)c.rows * c.C <= TTS_W2V_TEST_MAX_FLOATS && (int64_t)c.rows * c.C2 <= TTS_W2V_TEST_MAX_FLOATS;
  }
}

} // namespace

extern "C" {

// 0 for a case tts_w2v_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_w2v_test_validate(const tts_w2v_case *c) {
  Plan p;
  return c && valid(*c, p) ? 0 : (int)hipErrorInvalidValue;
}

// the HFG_SEQ tables the harness builds for a case (host only): [ns][9] of the input into `in_tab`, of the output (STEM; else untouched) into `out_tab`
int tts_w2v_test_table(const tts_w2v_case *c, int *in_tab, int *out_tab) {
  Plan p;
  if (!c || !in_tab || !valid(*c, p)) return (int)hipErrorInvalidValue;
  memcpy(in_tab, p.seq.data(), p.seq.size() * sizeof(int));
  if (out_tab && !p.seq_out.empty()) memcpy(out_tab, p.seq_out.data(), p.seq_out.size() * sizeof(int));
  return 0;
}

// aligner_run's tables for clips of n[s] samples at 16 kHz behind N convolutions of k[i] taps and stride s[i] (host only): tab [N + 1][ns][9],
// rows / max_n [N + 1], tiles [0] = the statistics tiles of level 0
int tts_w2v_test_levels(const int *n, int ns, int N, const int *k, const int *s, int *tab, long long *rows, long long *tiles, int *max_n) {
  if (!n || !tab || !rows || !tiles || !max_n || ns < 1 || N < 0 || (N && (!k || !s))) return (int)hipErrorInvalidValue;
  const LevelTable t = w2v_levels(n, ns, N, k, s);
  memcpy(tab, t.tab.data(), t.tab.size() * sizeof(int));
  for (int l = 0; l <= N; l++) { rows[l] = t.rows[l]; max_n[l] = t.max_n[l]; }
  tiles[0] = t.tiles[0];
  return 0;
}

// The loader's host half on a model file (no HIP call): its status, and for TTS_OK out[0 .. 9] = N, C, D, K, channels of a group, depth, feed-forward width,
// V, heads, blank id. err (cap bytes) receives the message of a refusal.
int tts_w2v_test_parse(const char *path, int *out10, char *err, int cap) {
  tts_ctx ctx;
  WeightFile wf;
  std::string e;
  std::unique_ptr<W2vHost> h(new W2vHost());
  int rc = read_weight_file(path, wf, e);
  if (rc != TTS_OK) fail(&ctx, rc, "aligner_load: %s", e.c_str());
  else rc = aligner_parse(&ctx, wf, path, *h);
  if (err && cap > 0) { strncpy(err, ctx.err.c_str(), (size_t)cap - 1); err[cap - 1] = 0; }
  if (rc == TTS_OK && out10) {
    const int v[10] = {h->N, h->C, h->D, h->K, h->cg, h->depth, h->FF, h->V, h->H, h->blank};
    memcpy(out10, v, sizeof v);
  }
  return rc;
}

// One packed tensor of the parsed model (host only), for the tests of the repack: which = 0 conv[i].w, 1 proj.w, 2 pos.w, 3 layers[i].qkv.w,
// 4 layers[i].qkv.b, 5 layers[i].out.w, 6 layers[i].w1.w, 7 layers[i].w2.w, 8 head.w. Returns the element count (copies at most cap floats), or a TTS status.
long long tts_w2v_test_packed(const char *path, int which, int i, float *out, long long cap) {
  tts_ctx ctx;
  WeightFile wf;
  std::string e;
  std::unique_ptr<W2vHost> h(new W2vHost());
  int rc = read_weight_file(path, wf, e);
  if (rc == TTS_OK) rc = aligner_parse(&ctx, wf, path, *h);
  if (rc != TTS_OK) return rc;
  const std::vector<float> *v = nullptr;
  const bool li = i >= 0 && i < (int)h->layers.size();
  if (which == 0 && i >= 0 && i < h->N) v = &h->conv[i].w;
  else if (which == 1) v = &h->proj.w;
  else if (which == 2) v = &h->pos.w;
  else if (which == 3 && li) v = &h->layers[i].qkv.w;
  else if (which == 4 && li) v = &h->layers[i].qkv.b;
  else if (which == 5 && li) v = &h->layers[i].out.w;
  else if (which == 6 && li) v = &h->layers[i].w1.w;
  else if (which == 7 && li) v = &h->layers[i].w2.w;
  else if (which == 8) v = &h->head.w;
  if (!v) return TTS_ERR_ARG;
  if (out) memcpy(out, v->data(), (size_t)std::min<long long>(cap, (long long)v->size()) * 4);
  return (long long)v->size();
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_w2v_test_run(const tts_w2v_case *cp) {
  Plan p;
  if (!cp || !valid(*cp, p)) return (int)hipErrorInvalidValue;
  const tts_w2v_case &c = *cp;
  const int B = c.ns, C = c.C;
  const bool samples = c.kind == TTS_W2V_TEST_STATS || c.kind == TTS_W2V_TEST_STEM;
  Dev in, out, out2, w, bias, gam, bet, dseq, dseq_out, part, stat;
  const size_t in_bytes = samples ? (size_t)c.rows * 4 : (size_t)c.rows * C * 4;
  size_t out_bytes = in_bytes;
  if (c.kind == TTS_W2V_TEST_STATS) out_bytes = (size_t)B * sizeof(double2);
  if (c.kind == TTS_W2V_TEST_STEM) out_bytes = (size_t)c.rows_out * C * 4;
  if (c.kind == TTS_W2V_TEST_HEAD) out_bytes = (size_t)c.rows * c.C2 * 4;
  HT(dseq.alloc(p.seq.size() * 4, 0)); HT(dseq.put(p.seq.data()));
  const int *d_seq = (const int *)dseq.data();
  hipStream_t s;
  HT(in.alloc(in_bytes, 0)); HT(in.put(c.in));
  HT(out.alloc(out_bytes, TTS_W2V_TEST_SENTINEL));
  const float *din = (const float *)in.data();
  float *dy = (float *)out.data();
  hipError_t e = hipSuccess;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  switch (c.kind) {
    case TTS_W2V_TEST_STATS: {
      HT(part.alloc((size_t)p.tiles * sizeof(double2), TTS_W2V_TEST_SENTINEL));
      HT(hipDeviceSynchronize()); // the fills above ran on the null stream
      w2v_launch_stats(din, d_seq, p.max_n, B, (double2 *)part.data(), (double2 *)out.data(), s);
      break;
    }
    case TTS_W2V_TEST_STEM: {
      HT(w.alloc((size_t)C * c.taps * 4, 0)); HT(w.put(c.w)); HT(bias.alloc((size_t)C * 4, 0)); HT(bias.put(c.bias));
      HT(stat.alloc((size_t)B * sizeof(double2), 0)); HT(stat.put(c.stat));
      HT(dseq_out.alloc(p.seq_out.size() * 4, 0)); HT(dseq_out.put(p.seq_out.data()));
      HT(hipDeviceSynchronize());
      w2v_launch_stem(din, (const double2 *)stat.data(), (const float *)w.data(), (const float *)bias.data(), d_seq, (const int *)dseq_out.data(), C, c.taps, c.stride,
                      p.max_out, B, dy, s);
      break;
    }
    case TTS_W2V_TEST_LN: {
      if (c.mode == 2) { // the GELU alone works in place: the clips' rows are copied into the output buffer first, the rows of no clip keep the sentinel
        for (int q = 0; q < B; q++) {
          const size_t o = (size_t)p.seq[(size_t)HFG_SEQ * q] * C * 4;
          HT(hipMemcpy(out.data() + o, in.data() + o, (size_t)c.n[q] * C * 4, hipMemcpyDeviceToDevice));
        }
        HT(hipDeviceSynchronize());
        w2v_launch_gelu(dy, d_seq, C, p.max_n, B, s);
        break;
      }
      HT(gam.alloc((size_t)C * 4, 0)); HT(gam.put(c.gamma)); HT(bet.alloc((size_t)C * 4, 0)); HT(bet.put(c.beta));
      HT(hipDeviceSynchronize());
      w2v_launch_ln(din, dy, (const float *)gam.data(), (const float *)bet.data(), d_seq, C, c.mode, p.max_n, B, s);
      break;
    }
    case TTS_W2V_TEST_POS: {
      HT(w.alloc((size_t)c.taps * c.C2 * C * 4, 0)); HT(w.put(c.w)); HT(bias.alloc((size_t)C * 4, 0)); HT(bias.put(c.bias));
      HT(hipDeviceSynchronize());
      W2vPos a{};
      a.in = din; a.out = dy; a.w = (const float *)w.data(); a.bias = (const float *)bias.data(); a.seq = d_seq; a.D = C; a.cg = c.C2; a.K = c.taps;
      w2v_launch_pos(a, p.max_n, B, s);
      break;
    }
    default: {
      HT(w.alloc((size_t)C * c.C2 * 4, 0)); HT(w.put(c.w)); HT(bias.alloc((size_t)c.C2 * 4, 0)); HT(bias.put(c.bias));
      HT(out2.alloc((size_t)c.rows * 4, TTS_W2V_TEST_SENTINEL));
      HT(hipDeviceSynchronize());
      w2v_launch_head(din, (const float *)w.data(), (const float *)bias.data(), d_seq, C, c.C2, p.max_n, B, (int *)out2.data(), c.mode ? dy : nullptr, s);
      break;
    }
  }
  if (e == hipSuccess) e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  if (c.kind == TTS_W2V_TEST_HEAD) HT(out2.get_all(c.out2));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
