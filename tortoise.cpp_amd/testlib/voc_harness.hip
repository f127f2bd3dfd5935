// Test-only harness around the UnivNet vocoder's kernels (csrc/vocoder.hip, included whole and unchanged): host arrays in, host arrays out, one launch per call on
// a stream of its own. voc_run launches its kernels inline, so the six grid / block expressions are restated here, each beside the line of voc_run it copies.
// Built as libtts_voc_test.so next to the product library (together with csrc/host_logic.cpp, which vocoder.hip's host half calls); it is not part of the
// product (tests/test_voc_kernels_gpu.py and tests/test_voc_harness_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (the packed layout, every index into row_seq / seq_start / seq_len, every address the
// chosen kernel reads or writes), and every device buffer carries a canary margin in front and behind, inside the same allocation, that is copied back with the
// payload.
#include "../csrc/vocoder.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_VOC_TEST_MARGIN = 4096, TTS_VOC_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_VOC_TEST_CONV = 0, TTS_VOC_TEST_CONVT = 1, TTS_VOC_TEST_LVC_GATE = 2, TTS_VOC_TEST_LVC_MFMA = 3, TTS_VOC_TEST_DCONV = 4, TTS_VOC_TEST_POST = 5,
       TTS_VOC_TEST_MEL_ROWS = 6, TTS_VOC_TEST_NOISE_ROWS = 7, TTS_VOC_TEST_COND_F16 = 8, TTS_VOC_TEST_PHILOX = 9 };
enum { TTS_VOC_TEST_MAX_SEQ = 16, TTS_VOC_TEST_MAX_ROWS = 256, TTS_VOC_TEST_MAX_HOP = 256, TTS_VOC_TEST_MAX_CIN = 128, TTS_VOC_TEST_MAX_K = 7,
       TTS_VOC_TEST_MAX_DIL = 64, TTS_VOC_TEST_MAX_N = 1 << 22 };

// One case. Host pointers only. `out` holds TTS_VOC_TEST_MARGIN bytes, the payload, TTS_VOC_TEST_MARGIN bytes.
//   layout   ns sequences; sequence s on frames [start[s], start[s] + len[s]) of `rows` frames, as voc_run lays them out (len >= 11 = one mel frame + 10 pad
//            frames, start % 8 == 0, the first sequence not before row 8, a guard row behind every sequence, rows % 8 == 0). row_seq / row_t / out_off are
//            derived here by the rule of voc_run. An audio-rate tensor at `hop` samples per frame is [rows * hop][channels].
//   CONV        conv_direct_kernel: x [rows*hop][Cin], w [K][Cin][Cout], bias [Cout], resid (optional) [rows*hop][Cout]; out f32 [rows*hop][Cout]
//   CONVT       convt_kernel: x [rows*hop][32] (hop = hop_in), w [2s][32][32], bias [32]; out f32 [rows*hop*s][32]
//   LVC_GATE / LVC_MFMA   x = the dilated conv's output [rows*hop][32], kern [rows][24576], kb [rows][256], xio = the tensor the gate is added to
//            [rows*hop][32]; out f32 [rows*hop][32] = xio after the launch (the output buffer starts as xio, not as the sentinel)
//   DCONV       voc_dconv_mfma_kernel: x [rows*hop][32], w [3][32][32], bias [32]; out f32 [rows*hop][32]
//   POST        conv_post_kernel: x [rows*256][32], w [7][32], bias [1]; out f32 [sum(len*256 - 6)], sequence after sequence
//   MEL_ROWS    x = mel [100][len - 10] per sequence, concatenated; out f32 [rows][100]
//   NOISE_ROWS  x = noise [64][len] per sequence, concatenated; out f32 [rows][64]
//   COND_F16    x [rows][64]; out fp16 [rows][64]
//   PHILOX      n, seed, stream; out f32 [n]
struct tts_voc_case {
  int kind, ns, rows;
  int hop, s, dil, layer;
  int Cin, Cout, K, pad, pre_leaky, post_leaky, reflect;
  unsigned int stream;
  unsigned long long seed;
  long long n;
  const int *start, *len;
  const float *x, *w, *bias, *resid, *kern, *kb, *xio;
  void *out;
};

int tts_voc_test_margin(void) { return TTS_VOC_TEST_MARGIN; }
int tts_voc_test_lvc_col(int tap, int i, int ch) { return lvc_col(tap, i, ch); } // the predicted kernel's order, read from the product

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_VOC_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_VOC_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_VOC_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_VOC_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

bool pow2(int v) { return v >= 1 && (v & (v - 1)) == 0; }
bool flag(int v) { return v == 0 || v == 1; }

bool valid(const tts_voc_case &c) {
  if (c.kind < TTS_VOC_TEST_CONV || c.kind > TTS_VOC_TEST_PHILOX) return false;
  if (!c.out) return false;
  if (c.kind == TTS_VOC_TEST_PHILOX) return c.n >= 1 && c.n <= TTS_VOC_TEST_MAX_N;
  if (!c.x) return false;
  // the packed layout, as voc_run builds it. Every kernel indexes row_seq with a frame of [0, rows) and seq_start / seq_len with a value of row_seq
  if (c.ns < 1 || c.ns > TTS_VOC_TEST_MAX_SEQ || !c.start || !c.len) return false;
  if (c.rows < 8 || c.rows % 8 || c.rows > TTS_VOC_TEST_MAX_ROWS) return false;
  long long prev_end = 8; // first row a sequence may start on: row 0 is never live (lvc_*: pos - 1 >= 0)
  for (int s = 0; s < c.ns; s++) {
    const long long st = c.start[s], ln = c.len[s];
    // in order, aligned, at least T = 1 mel frame + 10 pad frames, and a guard row follows inside the layout (so the last row is never live: lvc_*: pos + 1 < P)
    if (st < prev_end || st % 8 || ln < 11 || st + ln + 1 > c.rows) return false;
    prev_end = st + ln + 1;
  }
  switch (c.kind) {
    case TTS_VOC_TEST_CONV:
      // reads x[lo + q] with 0 <= q < n only (the bounds check under test), w[k][ci][co], bias[co], resid / y at p < P
      if (!c.w || !c.bias) return false;
      if (c.Cout != 32 && c.Cout != 64) return false; // 256 / Cout positions per block, every thread one (position, channel)
      if (c.Cin < 1 || c.Cin > TTS_VOC_TEST_MAX_CIN || c.K < 1 || c.K > TTS_VOC_TEST_MAX_K) return false;
      if (!pow2(c.hop) || c.hop > TTS_VOC_TEST_MAX_HOP) return false;
      if (c.dil < 1 || c.dil > TTS_VOC_TEST_MAX_DIL || c.pad < 0 || c.pad > TTS_VOC_TEST_MAX_DIL * TTS_VOC_TEST_MAX_K) return false;
      return flag(c.pre_leaky) && flag(c.post_leaky) && flag(c.reflect);
    case TTS_VOC_TEST_CONVT:
      // shifts for divisions: hop_in and s powers of two; reads x[lo_in + t] with 0 <= t < n_in, w[k < 2s]
      if (!c.w || !c.bias) return false;
      if (!pow2(c.hop) || !pow2(c.s) || c.s < 2 || c.hop * c.s > TTS_VOC_TEST_MAX_HOP) return false;
      return true;
    case TTS_VOC_TEST_LVC_GATE:
      // chunk = min(64, hop), hop / 64 chunks per frame: hop < 64 or whole chunks. The window reads row_seq[(row*hop + s0 - 1 + j) / hop], j < chunk + 2: frames
      // row - 1 .. row + 1 of a live row, inside [0, rows) because rows 0 and rows - 1 are guards; y only where that frame is of the same sequence
      if (!c.kern || !c.kb || !c.xio) return false;
      if (!pow2(c.hop) || c.hop > TTS_VOC_TEST_MAX_HOP) return false;
      return c.layer >= 0 && c.layer < 4;
    case TTS_VOC_TEST_LVC_MFMA:
      // no bounds check: reads y[pos - 1 .. pos + 1] for every pos of a live frame: >= 0 and < rows * hop because rows 0 and rows - 1 are guards
      if (!c.kern || !c.kb || !c.xio) return false;
      if (c.hop < 64 || c.hop % 64 || c.hop > TTS_VOC_TEST_MAX_HOP) return false; // a wave walks hop / 64 tiles
      return c.layer >= 0 && c.layer < 4;
    case TTS_VOC_TEST_DCONV:
      // q clamped to [0, P - 1]; P = rows * hop is a multiple of 512, so every tile of a block below P is whole
      if (!c.w || !c.bias) return false;
      if (c.hop != 64 && c.hop != 256) return false; // voc_run passes hop_shift 6 or 8
      return c.dil >= 1 && c.dil < c.hop;             // a tap that leaves the sequence must land in the guard frame
    case TTS_VOC_TEST_POST:
      // reads x[(start*256 + j + k)] for j < len*256 - 6, k < 7: inside the sequence
      return c.w && c.bias;
    default: return true; // MEL_ROWS, NOISE_ROWS (offsets derived here from len), COND_F16
  }
}

} // namespace

extern "C" {

// 0 for a case tts_voc_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_voc_test_validate(const tts_voc_case *c) { return c && valid(*c) ? 0 : (int)hipErrorInvalidValue; }

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_voc_test_run(const tts_voc_case *cp) {
  if (!cp || !valid(*cp)) return (int)hipErrorInvalidValue;
  const tts_voc_case &c = *cp;
  Dev x, out, w, bias, resid, kern, kb, rseq, rt, start, len, offs;
  const int R = c.rows, B = c.ns;
  const int64_t P = (int64_t)R * c.hop;
  size_t out_bytes = 0;
  int max_len = 0;
  if (c.kind != TTS_VOC_TEST_PHILOX) {
    std::vector<int> rs(R, -1), rtv(R, 0); // voc_run
    std::vector<int64_t> mel_off(B), nz_off(B), out_off(B);
    int64_t mel_total = 0, nz_total = 0, out_total = 0;
    for (int s = 0; s < B; s++) {
      for (int t = 0; t < c.len[s]; t++) { rs[c.start[s] + t] = s; rtv[c.start[s] + t] = t; }
      max_len = std::max(max_len, c.len[s]);
      mel_off[s] = mel_total; mel_total += (int64_t)100 * (c.len[s] - 10);
      nz_off[s] = nz_total; nz_total += (int64_t)64 * c.len[s];
      out_off[s] = out_total; out_total += (int64_t)c.len[s] * 256 - 6;
    }
    HT(rseq.alloc((size_t)R * 4, 0)); HT(rseq.put(rs.data()));
    HT(rt.alloc((size_t)R * 4, 0)); HT(rt.put(rtv.data()));
    HT(start.alloc((size_t)B * 4, 0)); HT(start.put(c.start));
    HT(len.alloc((size_t)B * 4, 0)); HT(len.put(c.len));
    size_t x_bytes = 0, w_bytes = 0, b_bytes = 0;
    switch (c.kind) {
      case TTS_VOC_TEST_CONV:
        x_bytes = (size_t)P * c.Cin * 4; w_bytes = (size_t)c.K * c.Cin * c.Cout * 4; b_bytes = (size_t)c.Cout * 4; out_bytes = (size_t)P * c.Cout * 4; break;
      case TTS_VOC_TEST_CONVT:
        x_bytes = (size_t)P * 32 * 4; w_bytes = (size_t)2 * c.s * 32 * 32 * 4; b_bytes = 32 * 4; out_bytes = (size_t)P * c.s * 32 * 4; break;
      case TTS_VOC_TEST_LVC_GATE: case TTS_VOC_TEST_LVC_MFMA: x_bytes = out_bytes = (size_t)P * 32 * 4; break;
      case TTS_VOC_TEST_DCONV: x_bytes = out_bytes = (size_t)P * 32 * 4; w_bytes = 3 * 32 * 32 * 4; b_bytes = 32 * 4; break;
      case TTS_VOC_TEST_POST: x_bytes = (size_t)R * 256 * 32 * 4; w_bytes = 7 * 32 * 4; b_bytes = 4; out_bytes = (size_t)out_total * 4; break;
      case TTS_VOC_TEST_MEL_ROWS: x_bytes = (size_t)mel_total * 4; out_bytes = (size_t)R * 100 * 4; break;
      case TTS_VOC_TEST_NOISE_ROWS: x_bytes = (size_t)nz_total * 4; out_bytes = (size_t)R * 64 * 4; break;
      default: x_bytes = (size_t)R * 64 * 4; out_bytes = (size_t)R * 64 * 2; break;
    }
    HT(x.alloc(x_bytes, 0)); HT(x.put(c.x));
    if (w_bytes) { HT(w.alloc(w_bytes, 0)); HT(w.put(c.w)); HT(bias.alloc(b_bytes, 0)); HT(bias.put(c.bias)); }
    if (c.kind == TTS_VOC_TEST_CONV && c.resid) { HT(resid.alloc(out_bytes, 0)); HT(resid.put(c.resid)); }
    if (c.kind == TTS_VOC_TEST_LVC_GATE || c.kind == TTS_VOC_TEST_LVC_MFMA) {
      HT(kern.alloc((size_t)R * 24576 * 4, 0)); HT(kern.put(c.kern));
      HT(kb.alloc((size_t)R * 256 * 4, 0)); HT(kb.put(c.kb));
    }
    if (c.kind == TTS_VOC_TEST_POST || c.kind == TTS_VOC_TEST_MEL_ROWS || c.kind == TTS_VOC_TEST_NOISE_ROWS) {
      const std::vector<int64_t> &o = c.kind == TTS_VOC_TEST_POST ? out_off : c.kind == TTS_VOC_TEST_MEL_ROWS ? mel_off : nz_off;
      HT(offs.alloc((size_t)B * 8, 0)); HT(offs.put(o.data()));
    }
  } else {
    out_bytes = (size_t)c.n * 4;
  }
  HT(out.alloc(out_bytes, TTS_VOC_TEST_SENTINEL));
  if (c.kind == TTS_VOC_TEST_LVC_GATE || c.kind == TTS_VOC_TEST_LVC_MFMA) HT(out.put(c.xio));

  const float *dx = (const float *)x.data(), *dw = (const float *)w.data(), *db = (const float *)bias.data();
  const int *d_rs = (const int *)rseq.data(), *d_rt = (const int *)rt.data(), *d_st = (const int *)start.data(), *d_ln = (const int *)len.data();
  const int64_t *d_off = (const int64_t *)offs.data();
  float *dy = (float *)out.data();
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    switch (c.kind) {
      case TTS_VOC_TEST_CONV: { // conv(), vocoder.hip:495-499
        ConvArgs a{dx, dw, db, dy, (const float *)resid.data(), d_rs, d_st, d_ln, (int)P, c.Cin, c.Cout, c.K, c.dil, c.pad, c.hop, c.pre_leaky, c.post_leaky, c.reflect};
        const int per = 256 / c.Cout;
        conv_direct_kernel<<<(int)((P + per - 1) / per), 256, 0, s>>>(a);
        break;
      }
      case TTS_VOC_TEST_CONVT: { // voc_run, vocoder.hip:604
        const int64_t Pout = P * c.s;
        convt_kernel<<<(int)((Pout + 7) / 8), 256, 0, s>>>(dx, dw, db, d_rs, d_st, d_ln, c.hop, c.s, Pout, dy);
        break;
      }
      case TTS_VOC_TEST_LVC_GATE: { // voc_run, vocoder.hip:641-642
        dim3 grid(std::max(1, c.hop / 64), R);
        lvc_gate_kernel<<<grid, 256, 0, s>>>(dx, (const float *)kern.data(), (const float *)kb.data(), d_rs, c.hop, c.layer, dy);
        break;
      }
      case TTS_VOC_TEST_LVC_MFMA: // voc_run, vocoder.hip:635
        lvc_mfma_kernel<<<R, 256, 0, s>>>(dx, (const float *)kern.data(), (const float *)kb.data(), d_rs, c.hop, c.layer, dy);
        break;
      case TTS_VOC_TEST_DCONV: // voc_run, vocoder.hip:633
        voc_dconv_mfma_kernel<<<(int)((P + 255) / 256), 256, 0, s>>>(dx, dw, db, d_rs, c.hop == 64 ? 6 : 8, c.dil, P, dy);
        break;
      case TTS_VOC_TEST_POST: { // voc_run, vocoder.hip:647-650
        dim3 grid((int)(((int64_t)max_len * 256 + 255) / 256), B);
        conv_post_kernel<<<grid, 256, 0, s>>>(dx, dw, db, d_st, d_ln, d_off, dy);
        break;
      }
      case TTS_VOC_TEST_MEL_ROWS: voc_mel_rows_kernel<<<R, 128, 0, s>>>(dx, d_off, d_rs, d_rt, d_ln, dy); break;     // vocoder.hip:590
      case TTS_VOC_TEST_NOISE_ROWS: voc_noise_rows_kernel<<<R, 64, 0, s>>>(dx, d_off, d_rs, d_rt, d_ln, dy); break;  // vocoder.hip:591
      case TTS_VOC_TEST_COND_F16: voc_cond_f16_kernel<<<R, 64, 0, s>>>(dx, d_rs, (__half *)out.data()); break;        // vocoder.hip:617
      default: voc_philox_kernel<<<(int)((c.n + 255) / 256), 256, 0, s>>>(dy, c.n, c.seed, c.stream); break;        // vocoder.hip:587
    }
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
