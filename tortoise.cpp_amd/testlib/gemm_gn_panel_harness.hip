// Test-only harness around gemm_f16_gn_panel_kernel (csrc/gemm_f16.h + csrc/diffusion.hip, included whole and unchanged): one case = one packed layout, fp16
// activations and a weight; it runs (a) the pair the engine ran before — launch_gemm_f16 (F32 output, register-streamed weight: gemm_f16_wreg_kernel) followed by
// gn_reg_kernel<512, 14> with gn_fused()'s launch shape — and (b) the panel kernel through the product's launch_gemm_gn_panel, on the same device operands, and
// returns both fp16 outputs with their canary margins. It also exposes the plan rule (gemm_gn_panel_takes), which is host arithmetic.
// Built as libtts_gnp_test.so next to the product library (with csrc/host_logic.cpp, which diffusion.hip's host half calls); not part of the product
// (tests/test_gemm_gn_panel_gpu.py and tests/test_gemm_gn_panel_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call, and every output buffer carries a margin in front and behind, inside the same allocation,
// that is copied back with the payload.
#include "../csrc/diffusion.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_GNP_TEST_MARGIN = 4096, TTS_GNP_TEST_SENTINEL = 0xCB, TTS_GNP_TEST_MAX_SEQ = 64, TTS_GNP_TEST_MAX_ROWS = 8192, TTS_GNP_TEST_MAX_TABLE = 64,
       TTS_GNP_TEST_MAX_STRIDE = 1 << 16 };

// One case. Host pointers only.
//   layout  ns sequences on rows [start[s], start[s] + len[s]) of `rows` packed rows (rows % 128 == 0; in order, 8-aligned, a guard row behind each)
//   A       fp16 [rows][K]            W  fp16 [Nw][K], Nw = N rounded up to 128 (the pair's GEMM multiplies all Nw rows, the panel kernel the first N)
//   bias    f32 [Nw] or null          g, b  f32 [1024]        ss  null or n_steps rows of 2048 floats, ss_step_stride floats apart; seq_step null or [ns]
//   out_pair, out_fused   margin | fp16 [rows][1024] | margin, both pre-filled with the sentinel byte. The pair's GroupNorm normalises all 1024 channels of an H
//           whose columns >= Nw are zero; the panel kernel writes channels < N only.
struct tts_gnp_case {
  int ns, rows, N, K;
  int do_silu, lut, n_steps, ss_step_stride;
  float eps;
  const int *start, *len, *seq_step;
  const uint16_t *A, *W;
  const float *bias, *g, *b, *ss;
  void *out_pair, *out_fused;
};

int tts_gnp_test_margin(void) { return TTS_GNP_TEST_MARGIN; }
int tts_gnp_test_takes(int option, int stats, int debug_sums, int has_wf, int max_len, int rows, int N, int K) {
  return gemm_gn_panel_takes(option, stats != 0, debug_sums != 0, has_wf != 0, max_len, rows, N, K) ? 1 : 0;
}
int tts_gnp_test_grid(int ns, int N) { return gemm_gn_panel_grid(ns, N); }
int tts_gnp_test_lds(void) { return GEMM_GN_PANEL_LDS; }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_GNP_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_GNP_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_GNP_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_GNP_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

int nw_of(int N) { return (N + 127) / 128 * 128; }

bool valid(const tts_gnp_case &c) {
  if (!c.A || !c.W || !c.g || !c.b || !c.out_pair || !c.out_fused || !c.start || !c.len) return false;
  if (c.rows < 128 || c.rows % 128 || c.rows > TTS_GNP_TEST_MAX_ROWS) return false;
  if (c.N < 64 || c.N % 64 || c.N > C || c.K < 128 || c.K % 64 || c.K > 2048) return false; // the register-streamed GEMM of the pair needs two K tiles of 64
  if (c.ns < 1 || c.ns > TTS_GNP_TEST_MAX_SEQ) return false;
  long long prev_end = 0;
  for (int s = 0; s < c.ns; s++) {
    const long long st = c.start[s], ln = c.len[s];
    if (st < prev_end || st % 8 || ln < 1 || ln > GEMM_GN_PANEL_ROWS || st + ln + 1 > c.rows) return false;
    prev_end = st + ln + 1;
  }
  if (c.lut < 0 || c.lut > 2 || (c.do_silu != 0 && c.do_silu != 1)) return false;
  if (c.seq_step && !c.ss) return false;
  if (c.ss) {
    if (c.n_steps < 1 || c.n_steps > TTS_GNP_TEST_MAX_TABLE || c.ss_step_stride < 0 || c.ss_step_stride > TTS_GNP_TEST_MAX_STRIDE) return false;
    if (!c.seq_step && c.n_steps != 1) return false;
    if (c.seq_step)
      for (int s = 0; s < c.ns; s++)
        if (c.seq_step[s] < 0 || c.seq_step[s] >= c.n_steps) return false;
  }
  return true;
}

} // namespace

extern "C" {

int tts_gnp_test_validate(const tts_gnp_case *c) { return c && valid(*c) ? 0 : (int)hipErrorInvalidValue; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_gnp_test_run(const tts_gnp_case *cp) {
  if (!cp || !valid(*cp)) return (int)hipErrorInvalidValue;
  const tts_gnp_case &c = *cp;
  const int rows = c.rows, Nw = nw_of(c.N), K = c.K;
  // the pair's plan, before anything is allocated: it must be the register-streamed kernel
  GemmArgs g{};
  for (int i = 0; i < 3; i++) { g.A[i] = nullptr; g.row_off[i] = 0; }
  g.nseg = 1; g.kseg = K; g.lda = K; g.M = rows; g.N = Nw; g.mode = GEMM_OUT_F32; g.ldo = C; g.wreg = 1; g.th = 8;
  g.Wf = (const __half *)c.W; // (any non-null value: the plan only asks whether an image exists)
  if (gemm_plan(g).err != hipSuccess || gemm_plan(g).kernel != GEMM_KERNEL_WREG) return (int)hipErrorInvalidValue;

  std::vector<uint16_t> wf((size_t)Nw * K);
  for (int n = 0; n < Nw; n++)
    for (int k = 0; k < K; k++) wf[gemm_wfrag_index(n, k, K)] = c.W[(size_t)n * K + k];
  std::vector<int> rs(rows, -1); // Layout::build
  for (int s = 0; s < c.ns; s++)
    for (int t = 0; t < c.len[s]; t++) rs[c.start[s] + t] = s;

  Dev A, W, Wf, bias, gg, bb, ss, step, start, len, rseq, H, yp, yf;
  HT(A.alloc((size_t)rows * K * 2, 0)); HT(A.put(c.A));
  HT(W.alloc((size_t)Nw * K * 2, 0)); HT(W.put(c.W));
  HT(Wf.alloc((size_t)Nw * K * 2, 0)); HT(Wf.put(wf.data()));
  if (c.bias) { HT(bias.alloc((size_t)Nw * 4, 0)); HT(bias.put(c.bias)); }
  HT(gg.alloc((size_t)C * 4, 0)); HT(gg.put(c.g));
  HT(bb.alloc((size_t)C * 4, 0)); HT(bb.put(c.b));
  if (c.ss) {
    HT(ss.alloc(((size_t)(c.n_steps - 1) * c.ss_step_stride + 2 * C) * 4, 0)); HT(ss.put(c.ss));
    if (c.seq_step) { HT(step.alloc((size_t)c.ns * 4, 0)); HT(step.put(c.seq_step)); }
  }
  HT(start.alloc((size_t)c.ns * 4, 0)); HT(start.put(c.start));
  HT(len.alloc((size_t)c.ns * 4, 0)); HT(len.put(c.len));
  HT(rseq.alloc((size_t)rows * 4, 0)); HT(rseq.put(rs.data()));
  HT(H.alloc((size_t)rows * C * 4, 0));
  HT(yp.alloc((size_t)rows * C * 2, TTS_GNP_TEST_SENTINEL));
  HT(yf.alloc((size_t)rows * C * 2, TTS_GNP_TEST_SENTINEL));

  for (int i = 0; i < 3; i++) g.A[i] = (const __half *)A.data();
  g.W = (const __half *)W.data(); g.Wf = (const __half *)Wf.data(); g.bias = (const float *)bias.data();
  g.row_seq = (const int *)rseq.data(); g.outF = (float *)H.data(); g.resid = nullptr;
  const int *d_start = (const int *)start.data(), *d_len = (const int *)len.data(), *d_step = (const int *)step.data();
  GemmGnPanelArgs a{};
  a.A = (const __half *)A.data(); a.lda = K; a.Wf = (const __half *)Wf.data(); a.N = c.N; a.K = K; a.bias = (const float *)bias.data();
  a.seq_start = d_start; a.seq_len = d_len; a.ns = c.ns; a.rows_total = rows;
  a.eps = c.eps; a.gn_g = (const float *)gg.data(); a.gn_b = (const float *)bb.data(); a.ss = (const float *)ss.data(); a.do_silu = c.do_silu; a.lut = c.lut;
  a.y = (__half *)yf.data(); a.seq_step = d_step; a.ss_step_stride = c.ss_step_stride;

  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) e = launch_gemm_f16(g, s);
  if (e == hipSuccess) {
    gn_reg_kernel<512, 14><<<dim3(32, c.ns), 512, 0, s>>>((const float *)H.data(), d_start, d_len, rows, c.ns, c.eps, a.gn_g, a.gn_b, a.ss, c.do_silu, c.lut,
                                                          (__half *)yp.data(), nullptr, 0, nullptr, 0, d_step, c.ss_step_stride);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = launch_gemm_gn_panel(a, s);
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  if (e != hipSuccess || es != hipSuccess) return (int)(e != hipSuccess ? e : es); // after a failed launch nothing more is asked of the device
  HT(yp.get_all(c.out_pair));
  HT(yf.get_all(c.out_fused));
  return 0;
}

} // extern "C"
