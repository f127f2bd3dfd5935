// Test-only harness around the AR stage's attention kernels and its QKV epilogues (csrc/ar.hip, included whole and unchanged, as tools/dec_bench.hip does):
// host arrays in, host arrays out, one launch on a stream of its own, with the grid and block size of the product's launch site.
// Built as libtts_ar_test.so next to the product library (together with csrc/host_logic.cpp, which ar.hip's host half calls); it is not part of the product
// (tests/test_ar_attn_kernels_gpu.py and tests/test_ar_attn_harness_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (positions, key counts, ragged items, every pointer the chosen kernel reads or
// writes), and every device buffer carries a canary margin in front and behind, inside the same allocation, that is copied back with the payload.
#include "../csrc/ar.hip"

#include <cstdint>
#include <cstring>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_AR_TEST_MARGIN = 4096, TTS_AR_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_AR_TEST_ATTENTION = 0, TTS_AR_TEST_ROWS = 1, TTS_AR_TEST_RAGGED = 2, TTS_AR_TEST_DECODE_FAST = 3, TTS_AR_TEST_DECODE = 4, TTS_AR_TEST_EPILOGUE = 5 };
enum { TTS_AR_TEST_MAX_CAND = 32, TTS_AR_TEST_MAX_ITEMS = 64, TTS_AR_TEST_MAX_ROWS = 4096 };

// One launch. Host pointers only. Every output buffer holds TTS_AR_TEST_MARGIN bytes, the payload, TTS_AR_TEST_MARGIN bytes.
//   ATTENTION, ROWS: q = qkv [n_cand * S][3072] f32 (the kernels read columns 0 .. 1023), kc / vc [n_cand][max_pos][1024] f16, out [n_cand * S][1024] f32
//   RAGGED:          q = qkv [n_rows][3072], items [n_items] = {first row, S, n_past, slot}, kc / vc [n_cand slots][max_pos][1024], out [n_rows][1024]
//   DECODE_FAST, DECODE: q [n_cand][1024] f32, StepState{n_past, 0} is written to device memory here, ro != 0: row_off [n_cand]; out [n_cand][1024]
//   EPILOGUE: part [n_rows][3072] f32, bias [3072], pscale, row_dst [n_rows] (distinct cache rows of n_cand slots of max_pos). epilogue_qkv_ragged_kernel
//             writes out [n_rows][3072] f32 and kout / vout [n_cand][max_pos][1024] f16; epilogue_kernel<EPI_QKV> (ks = 1, one candidate of n_rows
//             positions from n_past = 0) writes out2 [n_rows][3072] and kout2 / vout2 [n_rows][1024] from the same device copies of part and bias.
struct tts_ar_case {
  int kernel, lut, ro;
  int n_cand, S, n_past, max_pos;
  int n_items, n_rows;
  float pscale;
  const float *q;
  const uint16_t *kc, *vc;
  const int *items, *row_off, *row_dst;
  const float *part, *bias;
  float *out, *out2;
  uint16_t *kout, *vout, *kout2, *vout2;
};

int tts_ar_test_margin(void) { return TTS_AR_TEST_MARGIN; }

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_AR_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_AR_TEST_MARGIN);
  }
  char *data() const { return p + TTS_AR_TEST_MARGIN; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_AR_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

// rows of q and out the case names
int case_rows(const tts_ar_case &c) {
  switch (c.kernel) {
    case TTS_AR_TEST_ATTENTION: case TTS_AR_TEST_ROWS: return c.n_cand * c.S;
    case TTS_AR_TEST_RAGGED: case TTS_AR_TEST_EPILOGUE: return c.n_rows;
    default: return c.n_cand;
  }
}

bool valid(const tts_ar_case &c) {
  if (c.kernel < TTS_AR_TEST_ATTENTION || c.kernel > TTS_AR_TEST_EPILOGUE) return false;
  if (c.n_cand < 1 || c.n_cand > TTS_AR_TEST_MAX_CAND || c.max_pos < 1 || c.max_pos > 1024) return false; // attention_kernel / attn_decode_kernel: sc[1024]
  if ((c.lut != 0 && c.lut != 1) || (c.ro != 0 && c.ro != 1)) return false;
  if (c.kernel == TTS_AR_TEST_EPILOGUE) {
    if (c.n_rows < 1 || c.n_rows > TTS_AR_TEST_MAX_ROWS || !c.part || !c.bias || !c.row_dst) return false;
    if (!c.out || !c.out2 || !c.kout || !c.vout || !c.kout2 || !c.vout2) return false;
    if (!(c.pscale > 0.f) || !(c.pscale <= 1.f)) return false;
    const int cache_rows = c.n_cand * c.max_pos;
    for (int r = 0; r < c.n_rows; r++) {
      if (c.row_dst[r] < 0 || c.row_dst[r] >= cache_rows) return false;
      for (int r2 = 0; r2 < r; r2++)
        if (c.row_dst[r2] == c.row_dst[r]) return false; // two rows writing one cache row: a race
    }
    return true;
  }
  if (!c.q || !c.kc || !c.vc || !c.out) return false;
  if (c.kernel == TTS_AR_TEST_ATTENTION || c.kernel == TTS_AR_TEST_ROWS) {
    if (c.S < 1 || c.n_past < 0 || c.n_past > c.max_pos || c.S > c.max_pos - c.n_past) return false;
    if (c.lut && c.kernel == TTS_AR_TEST_ROWS) return false; // the rows kernels have no LUT form
    return true;
  }
  if (c.kernel == TTS_AR_TEST_RAGGED) {
    if (c.lut || !c.items || c.n_items < 1 || c.n_items > TTS_AR_TEST_MAX_ITEMS || c.n_rows < 1 || c.n_rows > TTS_AR_TEST_MAX_ROWS) return false;
    for (int i = 0; i < c.n_items; i++) {
      const int first = c.items[4 * i], S = c.items[4 * i + 1], n_past = c.items[4 * i + 2], slot = c.items[4 * i + 3];
      if (slot < 0 || slot >= c.n_cand || S < 1 || n_past < 0 || n_past > c.max_pos || S > c.max_pos - n_past) return false;
      if (first < 0 || first > c.n_rows || S > c.n_rows - first) return false;
      for (int i2 = 0; i2 < i; i2++) { // items do not overlap in the packed row space
        const int f2 = c.items[4 * i2], S2 = c.items[4 * i2 + 1];
        if (first < f2 + S2 && f2 < first + S) return false;
      }
    }
    return true;
  }
  // decode: every row's key count n_past + 1 + row_off[c] in [1, max_pos] (0 keys: attn_decode_chunk's clamp min(.., nk - 1) would read row -1)
  if (c.n_past < 0 || c.n_past >= c.max_pos) return false;
  if (c.lut && c.kernel == TTS_AR_TEST_DECODE_FAST) return false;
  if (c.ro) {
    if (!c.row_off) return false;
    for (int i = 0; i < c.n_cand; i++) {
      const long long nk = (long long)c.n_past + 1 + c.row_off[i];
      if (nk < 1 || nk > c.max_pos) return false;
    }
  }
  return true;
}

} // namespace

extern "C" {

// 0 for a case tts_ar_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_ar_test_validate(const tts_ar_case *c) { return c && valid(*c) ? 0 : (int)hipErrorInvalidValue; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_ar_test_run(const tts_ar_case *cp) {
  if (!cp || !valid(*cp)) return (int)hipErrorInvalidValue;
  const tts_ar_case &c = *cp;
  const int rows = case_rows(c);
  const size_t cache_bytes = (size_t)c.n_cand * c.max_pos * D * 2;
  hipStream_t s;
  if (c.kernel == TTS_AR_TEST_EPILOGUE) {
    Dev part, bias, rdst, out, out2, kout, vout, kout2, vout2;
    HT(part.alloc((size_t)rows * 3 * D * 4, 0)); HT(part.put(c.part));
    HT(bias.alloc((size_t)3 * D * 4, 0)); HT(bias.put(c.bias));
    HT(rdst.alloc((size_t)rows * 4, 0)); HT(rdst.put(c.row_dst));
    HT(out.alloc((size_t)rows * 3 * D * 4, TTS_AR_TEST_SENTINEL)); HT(out2.alloc((size_t)rows * 3 * D * 4, TTS_AR_TEST_SENTINEL));
    HT(kout.alloc(cache_bytes, TTS_AR_TEST_SENTINEL)); HT(vout.alloc(cache_bytes, TTS_AR_TEST_SENTINEL));
    HT(kout2.alloc((size_t)rows * D * 2, TTS_AR_TEST_SENTINEL)); HT(vout2.alloc((size_t)rows * D * 2, TTS_AR_TEST_SENTINEL));
    HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
    if (e == hipSuccess) {
      epilogue_qkv_ragged_kernel<<<dim3(rows, 3 * D / 256), 256, 0, s>>>((const float *)part.data(), (const float *)bias.data(), (float *)out.data(),
                                                                         (const int *)rdst.data(), (__half *)kout.data(), (__half *)vout.data(), c.pscale);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      KvDst kv{(__half *)kout2.data(), (__half *)vout2.data(), rows, 0, rows, 0};
      epilogue_kernel<EPI_QKV><<<dim3(rows, (3 * D + 255) / 256), 256, 0, s>>>((const float *)part.data(), 1, rows, 3 * D, 3 * D, (const float *)bias.data(),
                                                                                (float *)out2.data(), 3 * D, kv, 0, c.pscale);
      e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    HT(out.get_all(c.out)); HT(out2.get_all(c.out2));
    HT(kout.get_all(c.kout)); HT(vout.get_all(c.vout)); HT(kout2.get_all(c.kout2)); HT(vout2.get_all(c.vout2));
    return (int)(e != hipSuccess ? e : es);
  }
  const bool decode = c.kernel == TTS_AR_TEST_DECODE_FAST || c.kernel == TTS_AR_TEST_DECODE;
  Dev q, kc, vc, out, items, ro, ss;
  HT(q.alloc((size_t)rows * (decode ? D : 3 * D) * 4, 0)); HT(q.put(c.q));
  HT(kc.alloc(cache_bytes, 0)); HT(kc.put(c.kc));
  HT(vc.alloc(cache_bytes, 0)); HT(vc.put(c.vc));
  HT(out.alloc((size_t)rows * D * 4, TTS_AR_TEST_SENTINEL));
  int max_S = 0;
  if (c.kernel == TTS_AR_TEST_RAGGED) {
    HT(items.alloc((size_t)c.n_items * 16, 0)); HT(items.put(c.items));
    for (int i = 0; i < c.n_items; i++) max_S = std::max(max_S, c.items[4 * i + 1]);
  }
  if (decode) {
    const StepState hs{c.n_past, 0};
    HT(ss.alloc(sizeof hs, 0)); HT(ss.put(&hs));
    if (c.ro) { HT(ro.alloc((size_t)c.n_cand * 4, 0)); HT(ro.put(c.row_off)); }
  }
  const float *dq = (const float *)q.data();
  const __half *dk = (const __half *)kc.data(), *dv = (const __half *)vc.data();
  float *dout = (float *)out.data();
  const StepState *dss = (const StepState *)ss.data();
  const int *dro = (const int *)ro.data();
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    switch (c.kernel) {
      case TTS_AR_TEST_ATTENTION:
        attention_kernel<<<dim3(rows, NH), 64, 0, s>>>(dq, dk, dv, dout, c.S, c.n_past, c.max_pos, c.lut);
        break;
      case TTS_AR_TEST_ROWS:
        attention_rows_kernel<<<dim3(rows / c.S, NH, (c.S + 63) / 64), 256, 0, s>>>(dq, dk, dv, dout, c.S, c.n_past, c.max_pos);
        break;
      case TTS_AR_TEST_RAGGED:
        attention_rows_ragged_kernel<<<dim3(c.n_items, NH, (max_S + 63) / 64), 256, 0, s>>>(dq, dk, dv, dout, (const int4 *)items.data(), c.max_pos);
        break;
      case TTS_AR_TEST_DECODE_FAST:
        if (c.ro) attn_decode_fast_kernel<true><<<dim3(c.n_cand, NH), 256, 0, s>>>(dq, dk, dv, dss, c.max_pos, dout, dro);
        else attn_decode_fast_kernel<false><<<dim3(c.n_cand, NH), 256, 0, s>>>(dq, dk, dv, dss, c.max_pos, dout, nullptr);
        break;
      default:
        if (c.ro) attn_decode_kernel<true><<<dim3(c.n_cand, NH), 256, 0, s>>>(dq, dk, dv, dss, c.max_pos, dout, c.lut, dro);
        else attn_decode_kernel<false><<<dim3(c.n_cand, NH), 256, 0, s>>>(dq, dk, dv, dss, c.max_pos, dout, c.lut, nullptr);
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
