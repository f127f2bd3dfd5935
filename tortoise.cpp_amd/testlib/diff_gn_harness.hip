// Test-only harness around the diffusion stage's GroupNorm kernels and the three row kernels that share their layout (csrc/diffusion.hip, included whole and
// unchanged): host arrays in, host arrays out, one launch on a stream of its own (STATS_APPLY_F32: the two launches of the latent conditioner's code_norm), with
// the grid, block size and dynamic LDS of the product's launch site (gn_fused, gn_stats, gn, diffusion_latent_conditioner).
// Built as libtts_gn_test.so next to the product library (together with csrc/host_logic.cpp, which diffusion.hip's host half calls); it is not part of the
// product (tests/test_gn_kernels_gpu.py and tests/test_gn_harness_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (the packed layout, every index into a table, every pointer the chosen kernel reads or
// writes), and every device buffer carries a canary margin in front and behind, inside the same allocation, that is copied back with the payload.
#include "../csrc/diffusion.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_GN_TEST_MARGIN = 4096, TTS_GN_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_GN_TEST_REG512 = 0, TTS_GN_TEST_REG1024 = 1, TTS_GN_TEST_FUSED = 2, TTS_GN_TEST_AUTO = 3, TTS_GN_TEST_STATS = 4, TTS_GN_TEST_STATS_APPLY_F32 = 5,
       TTS_GN_TEST_APPLY = 6, TTS_GN_TEST_TO_F16 = 7, TTS_GN_TEST_GATHER_F16 = 8, TTS_GN_TEST_GATHER_F32 = 9 };
enum { TTS_GN_TEST_MAX_SEQ = 64, TTS_GN_TEST_MAX_ROWS = 8192, TTS_GN_TEST_MAX_TABLE = 64, TTS_GN_TEST_MAX_STRIDE = 1 << 16, TTS_GN_TEST_MAX_TOUCH = 1 << 22 };

// One case. Host pointers only. `out` holds TTS_GN_TEST_MARGIN bytes, the payload, TTS_GN_TEST_MARGIN bytes.
//   layout   ns sequences; sequence s on rows [start[s], start[s] + len[s]) of the rows_total rows the launch covers. x and the output are [x_rows][1024]; the
//            launch covers their rows [row0, row0 + rows_total) and start[] is relative to row0 (row0 = 0, x_rows = rows_total: the whole layout; otherwise one
//            part of a GroupNorm partition, Layout::gn_parts). row_seq / chunk_seq are derived here by the rule of Layout::build.
//   REG512, REG1024, FUSED, AUTO   x f32, g, b [1024], ss (optional) [n_steps rows of 2048, ss_step_stride floats apart], seq_step (optional) [ns],
//            do_silu, lut (silu_dev's mode 0 / 1 / 2), eps, pf0 / pf1 (optional weight-touch buffers of pf*_bytes, pf*_lines lines of 128 bytes touched; the
//            one-pass kernel takes none); out fp16 [x_rows][1024]. AUTO: the class Layout::gn_class names for the longest sequence; *picked receives it.
//   STATS    x, eps; out float2 [ns][32].
//   STATS_APPLY_F32   x, g, b, ss = the voice table [n_steps][2048], seq_voice (optional) [ns], eps; out f32 [rows_total][1024]
//   APPLY    as REG512 plus st [FX_STRIPES][ns * 32 * 4] fixed-point statistics; rows_total % 4 == 0, <= LAT_MAX_ROWS
//   TO_F16   x; out fp16 [rows_total][1024].  GATHER_F16 / GATHER_F32   x [x_rows][1024], src_row [rows_total] (-1: zero row); out [rows_total][1024]
struct tts_gn_case {
  int kind, ns, rows_total, row0, x_rows;
  int do_silu, lut, n_steps, ss_step_stride;
  int pf0_lines, pf1_lines;
  float eps;
  long long pf0_bytes, pf1_bytes;
  const int *start, *len, *seq_step, *seq_voice, *src_row;
  const float *x, *g, *b, *ss;
  const long long *st;
  const char *pf0, *pf1;
  void *out;
  int *picked; // optional: receives the kernel class launched (AUTO: what Layout::gn_class named)
};

int tts_gn_test_margin(void) { return TTS_GN_TEST_MARGIN; }
int tts_gn_test_class(int tmax) { return Layout::gn_class(tmax); } // the dispatch thresholds of gn_fused(), read from the product

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_GN_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_GN_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_GN_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_GN_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

bool is_gn(int k) { return k == TTS_GN_TEST_REG512 || k == TTS_GN_TEST_REG1024 || k == TTS_GN_TEST_FUSED || k == TTS_GN_TEST_AUTO || k == TTS_GN_TEST_APPLY; }
bool is_gather(int k) { return k == TTS_GN_TEST_GATHER_F16 || k == TTS_GN_TEST_GATHER_F32; }

bool valid(const tts_gn_case &c) {
  if (c.kind < TTS_GN_TEST_REG512 || c.kind > TTS_GN_TEST_GATHER_F32) return false;
  if (!c.x || !c.out) return false;
  const int mult = c.kind == TTS_GN_TEST_APPLY ? 4 : 8;
  if (c.rows_total < mult || c.rows_total % mult || c.rows_total > TTS_GN_TEST_MAX_ROWS) return false;
  if (c.kind == TTS_GN_TEST_APPLY && c.rows_total > LAT_MAX_ROWS) return false;
  if (is_gather(c.kind)) {
    if (!c.src_row || c.x_rows < 1 || c.x_rows > TTS_GN_TEST_MAX_ROWS || c.row0 != 0) return false;
    for (int r = 0; r < c.rows_total; r++)
      if (c.src_row[r] < -1 || c.src_row[r] >= c.x_rows) return false;
    return true;
  }
  // the packed layout
  if (c.ns < 1 || c.ns > TTS_GN_TEST_MAX_SEQ || !c.start || !c.len) return false;
  if (c.row0 < 0 || c.row0 % 8 || c.x_rows > TTS_GN_TEST_MAX_ROWS || c.x_rows % mult || c.row0 > c.x_rows || c.rows_total > c.x_rows - c.row0) return false;
  const bool part_ok = c.kind <= TTS_GN_TEST_AUTO; // only gn_fused() launches parts
  if (!part_ok && (c.row0 != 0 || c.x_rows != c.rows_total)) return false;
  long long prev_end = 0; // first row a sequence may start on
  for (int s = 0; s < c.ns; s++) {
    const long long st = c.start[s], ln = c.len[s];
    if (st < prev_end || st % 8 || ln < 1 || st + ln + 1 > c.rows_total) return false; // in order, aligned, and a guard row follows inside the launch
    prev_end = st + ln + 1;
  }
  const int cap[3] = {14 * 512 / 8, 18 * 1024 / 8, TTS_GN_TEST_MAX_ROWS}; // rows a class holds: NJ * NT / 8
  if (c.kind <= TTS_GN_TEST_FUSED)
    for (int s = 0; s < c.ns; s++)
      if (c.len[s] > cap[c.kind]) return false;
  if (c.kind == TTS_GN_TEST_STATS || c.kind == TTS_GN_TEST_TO_F16) return true;
  if (!c.g || !c.b) return false;
  if (c.kind == TTS_GN_TEST_STATS_APPLY_F32) {
    if (!c.ss || c.n_steps < 1 || c.n_steps > TTS_GN_TEST_MAX_TABLE) return false;
    if (c.seq_voice)
      for (int s = 0; s < c.ns; s++)
        if (c.seq_voice[s] < 0 || c.seq_voice[s] >= c.n_steps) return false;
    return true;
  }
  if (!is_gn(c.kind)) return false;
  if (c.lut < 0 || c.lut > 2 || (c.do_silu != 0 && c.do_silu != 1)) return false;
  if (c.seq_step && !c.ss) return false;
  if (c.ss) {
    if (c.n_steps < 1 || c.n_steps > TTS_GN_TEST_MAX_TABLE || c.ss_step_stride < 0 || c.ss_step_stride > TTS_GN_TEST_MAX_STRIDE) return false;
    if (!c.seq_step && c.n_steps != 1) return false;
    if (c.seq_step)
      for (int s = 0; s < c.ns; s++)
        if (c.seq_step[s] < 0 || c.seq_step[s] >= c.n_steps) return false;
  }
  if (c.pf0_lines < 0 || c.pf1_lines < 0 || c.pf0_bytes < 0 || c.pf1_bytes < 0 || c.pf0_bytes > TTS_GN_TEST_MAX_TOUCH || c.pf1_bytes > TTS_GN_TEST_MAX_TOUCH) return false;
  if ((c.pf0_lines && !c.pf0) || (c.pf1_lines && !c.pf1)) return false;
  if ((long long)c.pf0_lines * 128 > c.pf0_bytes || (long long)c.pf1_lines * 128 > c.pf1_bytes) return false;
  if (c.kind == TTS_GN_TEST_APPLY && !c.st) return false;
  return true;
}

} // namespace

extern "C" {

// 0 for a case tts_gn_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_gn_test_validate(const tts_gn_case *c) { return c && valid(*c) ? 0 : (int)hipErrorInvalidValue; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_gn_test_run(const tts_gn_case *cp) {
  if (!cp || !valid(*cp)) return (int)hipErrorInvalidValue;
  const tts_gn_case &c = *cp;
  const int rows = c.rows_total;
  const bool gather = is_gather(c.kind);
  const int xr = gather ? c.x_rows : (c.kind <= TTS_GN_TEST_AUTO ? c.x_rows : rows);
  Dev x, out, start, len, rseq, cseq, g, b, ss, step, st, pf0, pf1, stats, src;
  HT(x.alloc((size_t)xr * C * 4, 0)); HT(x.put(c.x));
  size_t out_bytes;
  switch (c.kind) {
    case TTS_GN_TEST_STATS: out_bytes = (size_t)c.ns * 32 * 8; break;
    case TTS_GN_TEST_STATS_APPLY_F32: case TTS_GN_TEST_GATHER_F32: out_bytes = (size_t)rows * C * 4; break;
    case TTS_GN_TEST_GATHER_F16: case TTS_GN_TEST_TO_F16: case TTS_GN_TEST_APPLY: out_bytes = (size_t)rows * C * 2; break;
    default: out_bytes = (size_t)xr * C * 2; break;
  }
  HT(out.alloc(out_bytes, TTS_GN_TEST_SENTINEL));
  int tmax = 0;
  if (gather) {
    HT(src.alloc((size_t)rows * 4, 0)); HT(src.put(c.src_row));
  } else {
    HT(start.alloc((size_t)c.ns * 4, 0)); HT(start.put(c.start));
    HT(len.alloc((size_t)c.ns * 4, 0)); HT(len.put(c.len));
    std::vector<int> rs(rows, -1), cs((rows + 7) / 8, -1); // Layout::build
    for (int s = 0; s < c.ns; s++) {
      tmax = std::max(tmax, c.len[s]);
      for (int t = 0; t < c.len[s]; t++) { rs[c.start[s] + t] = s; cs[(c.start[s] + t) >> 3] = s; }
    }
    HT(rseq.alloc(rs.size() * 4, 0)); HT(rseq.put(rs.data()));
    HT(cseq.alloc(cs.size() * 4, 0)); HT(cseq.put(cs.data()));
  }
  if (c.g) { HT(g.alloc((size_t)C * 4, 0)); HT(g.put(c.g)); HT(b.alloc((size_t)C * 4, 0)); HT(b.put(c.b)); }
  if (c.ss && (is_gn(c.kind) || c.kind == TTS_GN_TEST_STATS_APPLY_F32)) {
    const size_t stride = c.kind == TTS_GN_TEST_STATS_APPLY_F32 ? 2 * C : (size_t)c.ss_step_stride;
    HT(ss.alloc(((size_t)(c.n_steps - 1) * stride + 2 * C) * 4, 0)); HT(ss.put(c.ss));
    const int *idx = c.kind == TTS_GN_TEST_STATS_APPLY_F32 ? c.seq_voice : c.seq_step;
    if (idx) { HT(step.alloc((size_t)c.ns * 4, 0)); HT(step.put(idx)); }
  }
  if (is_gn(c.kind)) {
    if (c.pf0 && c.pf0_bytes) { HT(pf0.alloc((size_t)c.pf0_bytes, 0)); HT(pf0.put(c.pf0)); }
    if (c.pf1 && c.pf1_bytes) { HT(pf1.alloc((size_t)c.pf1_bytes, 0)); HT(pf1.put(c.pf1)); }
  }
  const int stripe_ll = c.ns * 32 * 4;
  if (c.kind == TTS_GN_TEST_APPLY) { HT(st.alloc((size_t)FX_STRIPES * stripe_ll * 8, 0)); HT(st.put(c.st)); }
  if (c.kind == TTS_GN_TEST_STATS_APPLY_F32) HT(stats.alloc((size_t)c.ns * 32 * 8, TTS_GN_TEST_SENTINEL));

  const float *dx = (const float *)x.data() + (size_t)c.row0 * C;
  const int *d_start = (const int *)start.data(), *d_len = (const int *)len.data(), *d_step = (const int *)step.data();
  const float *dg = (const float *)g.data(), *db = (const float *)b.data(), *dss = (const float *)ss.data();
  __half *y16 = (__half *)out.data() + (size_t)(c.kind <= TTS_GN_TEST_AUTO ? c.row0 : 0) * C;
  const int l0 = pf0.p ? c.pf0_lines : 0, l1 = pf1.p ? c.pf1_lines : 0;
  int kind = c.kind;
  if (kind == TTS_GN_TEST_AUTO) kind = Layout::gn_class(tmax); // as gn_fused()
  if (c.picked) *c.picked = kind;
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
#define GN_ARGS dx, d_start, d_len, rows, c.ns, c.eps, dg, db, dss, c.do_silu, c.lut, y16, (const char *)pf0.data(), l0, (const char *)pf1.data(), l1, d_step, c.ss_step_stride
    switch (kind) {
      case TTS_GN_TEST_REG512: gn_reg_kernel<512, 14><<<dim3(32, c.ns), 512, 0, s>>>(GN_ARGS); break;
      case TTS_GN_TEST_REG1024: gn_reg_kernel<1024, 18><<<dim3(32, c.ns), 1024, 0, s>>>(GN_ARGS); break;
      case TTS_GN_TEST_FUSED:
        gn_fused_kernel<0><<<dim3(32, c.ns), 256, 0, s>>>(dx, d_start, d_len, rows, c.ns, c.eps, dg, db, dss, c.do_silu, c.lut, y16, d_step, c.ss_step_stride);
        break;
      case TTS_GN_TEST_STATS: gn_stats_kernel<<<dim3(32, c.ns), 256, 0, s>>>(dx, d_start, d_len, c.eps, (float2 *)out.data()); break;
      case TTS_GN_TEST_STATS_APPLY_F32:
        gn_stats_kernel<<<dim3(32, c.ns), 256, 0, s>>>(dx, d_start, d_len, c.eps, (float2 *)stats.data());
        e = hipGetLastError();
        if (e == hipSuccess)
          gn_apply_f32_kernel<<<rows, 256, 0, s>>>(dx, (const int *)rseq.data(), (const float2 *)stats.data(), dg, db, dss, d_step, (float *)out.data());
        break;
      case TTS_GN_TEST_APPLY:
        gn_apply_kernel<<<rows / 4, 256, 0, s>>>(dx, (const int *)cseq.data(), d_start, d_len, (const long long *)st.data(), stripe_ll, c.eps, dg, db, dss, c.do_silu,
                                                 c.lut, y16, (const char *)pf0.data(), l0, (const char *)pf1.data(), l1, d_step, c.ss_step_stride);
        break;
      case TTS_GN_TEST_TO_F16: to_f16_kernel<<<rows, 256, 0, s>>>(dx, (const int *)rseq.data(), y16); break;
      case TTS_GN_TEST_GATHER_F16: gather_f16_kernel<<<rows, 256, 0, s>>>(dx, (const int *)src.data(), y16); break;
      default: gather_f32_kernel<<<rows, 256, 0, s>>>(dx, (const int *)src.data(), (float *)out.data()); break;
    }
#undef GN_ARGS
    if (e == hipSuccess) e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
