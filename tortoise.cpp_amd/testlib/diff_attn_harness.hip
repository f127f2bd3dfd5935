// Test-only harness around the diffusion stage's AttentionBlock core (csrc/diffusion.hip, included whole and unchanged): diff_attn_kernel<2,2> (the default, 128
// queries per workgroup), diff_attn_kernel<2,1> (option attn_q64, 64 queries per workgroup) and diff_attn_f32_kernel (options attn_f32 / lc_attn_f32, split
// precision). Host arrays in, host arrays out, one launch on a non-blocking stream of its own, with the grid, block size, dynamic LDS and nq of the product's
// launch site (attention_block) and, for the split-precision kernel, the hipFuncSetAttribute call the loader makes (more than 64 KB of dynamic LDS).
// Built as libtts_dattn_test.so next to the product library (together with csrc/host_logic.cpp, which diffusion.hip's host half calls); it is not part of the
// product (tests/test_dattn_kernels_gpu.py and tests/test_dattn_harness_cpu.py are the only users).
//
// THE MEMORY CONTRACT. The kernels check no bounds; they rely on the packed layout (Layout::build) and on the slack of the work buffers (Work::reserve):
//   reads   Q rows start + q0 .. start + q0 + 127 of every workgroup with q0 < len (q0 a multiple of 128, or of 64 with 64-query workgroups), whole 64-key K and
//           V^T tiles up to row start + 64 ceil(len / 64) - 1: both reach past the sequence, into its guard row, the next sequences and the 128 slack rows.
//   layout  sequences in order, start % 8 == 0, first start >= 8, len >= 1, a guard row behind every sequence, rows % 128 == 0.
//   sizes   qk (qk_lo) [(rows + 128)][2048] halves, vt (vt_lo) [1024][ldvt] with ldvt = rows + 128, out (out_lo) [(rows + 2)][1024], bias_tab [16][128] f32;
//           the kernel's out pointer is one row (1024 halves) into the output allocation, as Work::ATT16() is.
//   values  ROWS OUTSIDE A SEQUENCE HOLD FINITE VALUES. A key past the sequence's end gets weight 0, not a skipped product: the matrix pipe would turn 0 x Inf
//           or 0 x NaN into NaN. Any finite value there (the product keeps zeros, the tests put +-60000) leaves the output bits alone.
// The GPU is shared: a case is validated completely BEFORE any HIP call and everything else is refused; every device buffer carries a canary margin in front
// and behind, inside the same allocation, and the output buffers are copied back whole, margins included.
#include "../csrc/diffusion.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_DATTN_TEST_MARGIN = 4096, TTS_DATTN_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_DATTN_TEST_F16_Q128 = 0, TTS_DATTN_TEST_F16_Q64 = 1, TTS_DATTN_TEST_F32 = 2 };
enum { TTS_DATTN_TEST_MAX_SEQ = 8, TTS_DATTN_TEST_MAX_ROWS = 4096 };

// One case. Host pointers only.
//   layout   ns sequences; sequence s on rows [start[s], start[s] + len[s]) of a layout of `rows` rows.
//   qk       [qk_rows][2048] halves, qk_rows = rows + 128: row r, head h: Q on columns h * 128 .. + 63, K on h * 128 + 64 .. + 127. The caller supplies the WHOLE
//            image: guard rows, slack rows and other sequences' rows are case inputs.
//   vt       [1024][ldvt] halves, ldvt = rows + 128: V^T[h * 64 + d][row].
//   qk_lo, vt_lo, out_lo   the low halves of the split pairs: F32 only (ignored otherwise).
//   bias_tab [16][128] f32: head h, (key > query ? 64 : 0) + min(|key - query|, 63).
//   out, out_lo   TTS_DATTN_TEST_MARGIN bytes, [out_rows][1024] halves, TTS_DATTN_TEST_MARGIN bytes; out_rows = rows + 2 and layout row r is buffer row r + 1.
struct tts_dattn_case {
  int kind, ns, rows, ldvt, qk_rows, out_rows;
  const int *start, *len;
  const void *qk, *qk_lo, *vt, *vt_lo;
  const float *bias_tab;
  void *out, *out_lo;
  int *launch; // optional [4]: receives grid, block, dynamic LDS bytes, nq
};

int tts_dattn_test_margin(void) { return TTS_DATTN_TEST_MARGIN; }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_DATTN_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_DATTN_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_DATTN_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_DATTN_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

int queries_per_wg(int kind) { return kind == TTS_DATTN_TEST_F16_Q64 ? 64 : 128; }

bool valid(const tts_dattn_case &c) {
  if (c.kind < TTS_DATTN_TEST_F16_Q128 || c.kind > TTS_DATTN_TEST_F32) return false;
  if (!c.qk || !c.vt || !c.bias_tab || !c.out || !c.start || !c.len) return false;
  if (c.kind == TTS_DATTN_TEST_F32 && (!c.qk_lo || !c.vt_lo || !c.out_lo)) return false;
  if (c.ns < 1 || c.ns > TTS_DATTN_TEST_MAX_SEQ) return false;
  if (c.rows < 128 || c.rows % 128 || c.rows > TTS_DATTN_TEST_MAX_ROWS) return false; // Layout::build pads to 128
  if (c.qk_rows != c.rows + 128 || c.ldvt != c.rows + 128 || c.out_rows != c.rows + 2) return false; // Work::reserve
  const int qw = queries_per_wg(c.kind);
  long long prev_end = 8; // first row a sequence may start on: Layout::build starts at 8
  for (int s = 0; s < c.ns; s++) {
    const long long st = c.start[s], ln = c.len[s];
    if (st < prev_end || st % 8 || ln < 1 || st + ln + 1 > c.rows) return false; // in order, aligned, and a guard row follows inside the layout
    prev_end = st + ln + 1;
    // what the kernels read (implied by the rules above; stated on its own because it is what keeps the launch inside its buffers)
    if (st + (ln + qw - 1) / qw * qw > c.qk_rows) return false;                       // Q rows of the last workgroup
    if (st + (ln + 63) / 64 * 64 > c.qk_rows || st + (ln + 63) / 64 * 64 > c.ldvt) return false; // the last K and V^T tile
  }
  return true;
}

} // namespace

extern "C" {

// 0 for a case tts_dattn_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_dattn_test_validate(const tts_dattn_case *c) { return c && valid(*c) ? 0 : (int)hipErrorInvalidValue; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_dattn_test_run(const tts_dattn_case *cp) {
  if (!cp || !valid(*cp)) return (int)hipErrorInvalidValue;
  const tts_dattn_case &c = *cp;
  const bool f32 = c.kind == TTS_DATTN_TEST_F32;
  const size_t qk_bytes = (size_t)c.qk_rows * 2048 * 2, vt_bytes = (size_t)C * c.ldvt * 2, out_bytes = (size_t)c.out_rows * C * 2;
  int max_len = 0;
  for (int s = 0; s < c.ns; s++) max_len = std::max(max_len, c.len[s]);
  // as attention_block(): nq from the layout's longest sequence, one workgroup per (query block, head, sequence)
  const int qw = queries_per_wg(c.kind), nq = (max_len + qw - 1) / qw, grid = nq * NHEAD * c.ns;
  const int lds = f32 ? (int)ATT32_LDS : att_lds<2>();
  if (c.launch) { c.launch[0] = grid; c.launch[1] = 256; c.launch[2] = lds; c.launch[3] = nq; }
  Dev qk, qk_lo, vt, vt_lo, out, out_lo, start, len, tab;
  HT(qk.alloc(qk_bytes, 0)); HT(qk.put(c.qk));
  HT(vt.alloc(vt_bytes, 0)); HT(vt.put(c.vt));
  HT(out.alloc(out_bytes, TTS_DATTN_TEST_SENTINEL));
  if (f32) {
    HT(qk_lo.alloc(qk_bytes, 0)); HT(qk_lo.put(c.qk_lo));
    HT(vt_lo.alloc(vt_bytes, 0)); HT(vt_lo.put(c.vt_lo));
    HT(out_lo.alloc(out_bytes, TTS_DATTN_TEST_SENTINEL));
  }
  HT(start.alloc((size_t)c.ns * 4, 0)); HT(start.put(c.start));
  HT(len.alloc((size_t)c.ns * 4, 0)); HT(len.put(c.len));
  HT(tab.alloc((size_t)NHEAD * 128 * 4, 0)); HT(tab.put(c.bias_tab));
  if (f32) HT(hipFuncSetAttribute((const void *)diff_attn_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ATT32_LDS)); // as the loader: > 64 KB of dynamic LDS
  const __half *dqk = (const __half *)qk.data(), *dvt = (const __half *)vt.data();
  const int *d_start = (const int *)start.data(), *d_len = (const int *)len.data();
  const float *dtab = (const float *)tab.data();
  __half *dout = (__half *)out.data() + C; // as Work::ATT16(): one halo row in front
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    switch (c.kind) {
      case TTS_DATTN_TEST_F16_Q128: diff_attn_kernel<2, 2><<<grid, 256, lds, s>>>(dqk, dvt, c.ldvt, d_start, d_len, dtab, dout, nq); break;
      case TTS_DATTN_TEST_F16_Q64: diff_attn_kernel<2, 1><<<grid, 256, lds, s>>>(dqk, dvt, c.ldvt, d_start, d_len, dtab, dout, nq); break;
      default:
        diff_attn_f32_kernel<<<grid, 256, lds, s>>>(dqk, (const __half *)qk_lo.data(), dvt, (const __half *)vt_lo.data(), c.ldvt, d_start, d_len, dtab, dout,
                                                    (__half *)out_lo.data() + C, nq);
        break;
    }
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  if (f32) HT(out_lo.get_all(c.out_lo));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
