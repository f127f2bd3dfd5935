// Test-only harness around the HiFi-GAN decoder's kernels (csrc/hifigan.hip, included whole and unchanged): host arrays in, host arrays out, one launch per call on
// a stream of its own. hifigan_run launches its kernels inline (the convolutions through its `conv` lambda), so the grid, block and LDS-size expressions and the
// derived fields of HfgConv are restated here, each beside the line of hifigan.hip it copies. Built as libtts_hfg_test.so next to the product library (together with
// csrc/host_logic.cpp, which hifigan.hip's host half calls); it is not part of the product (tests/test_hfg_kernels_gpu.py and tests/test_hfg_harness_cpu.py are the
// only users).
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

enum { TTS_HFG_TEST_MARGIN = 4096, TTS_HFG_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_HFG_TEST_CONV = 0, TTS_HFG_TEST_CONV_SMALL = 1, TTS_HFG_TEST_INTERP = 2, TTS_HFG_TEST_COND = 3, TTS_HFG_TEST_POST = 4 };
// caps, sized by the case matrix of tests/hfg_cases.py: layout C has 3 candidates on 48 frames; the longest level is layout C at conv_post's 256 rows per frame;
// conv_pre reads 1024 channels; the ResBlocks reach 11 taps and dilation 5; three voices
enum { TTS_HFG_TEST_MAX_CAND = 3, TTS_HFG_TEST_MAX_FRAMES = 48, TTS_HFG_TEST_MAX_ROWS = 48 * 256, TTS_HFG_TEST_MAX_CH = 1024, TTS_HFG_TEST_MAX_TAPS = 11,
       TTS_HFG_TEST_MAX_DIL = 5, TTS_HFG_TEST_MAX_RATE = 256, TTS_HFG_TEST_MAX_VOICES = 3, TTS_HFG_TEST_LDS = 65536 };
enum { TTS_HFG_TEST_CAND = 6 }; // ints per candidate of `cand`

// One case. Host pointers only. `out` holds TTS_HFG_TEST_MARGIN bytes, the payload, TTS_HFG_TEST_MARGIN bytes.
//   cand     [ns][6] = {W (frames evaluated: T, or a chunk's window), voice, L, w0, keep0, keep_n}. The 9-int HFG_SEQ table is built from it by hifigan_run's rule:
//            start = the running sum of ceil8(W), first latent row = the running sum of L, output frames before = the running sum of keep_n.
//   start    null, or [ns] start frames that replace the running sum (validated: multiples of 8, in order, no overlap, inside `frames`)
//   frames   frames of every activation buffer (a multiple of 8, at least the end of the last candidate)
//   CONV / CONV_SMALL   in [frames*rate][cin], w [phases][taps][cin][cout], bias [cout], cbias null or [n_voices][cout], resid null or [frames*rate*phases][cout],
//            out0 the tensor `out` starts from (needed for acc_mode 1, 2 and alias 1; otherwise the output starts as the sentinel);
//            alias 0: none, 1: resid == out (the element is read and written by the same thread; `resid` is ignored and `out0` is what is read),
//            2: in == out, which hifigan_run never does and the kernels cannot take: always refused;  out f32 [frames*rate*phases][cout]
//   INTERP   in = latents [sum L][1024]; out f32 [frames][1024]
//   COND     w [512][1024], bias [512], in = g [n_voices][1024]; out f32 [n_voices][512]
//   POST     in = x [frames*256][32], w [7][32], bias [1]; out f32 [sum keep_n * 256]
struct tts_hfg_case {
  int kind, ns, frames, n_voices;
  int cin, cout, taps, dil, phases, rate, acc_mode, alias;
  float slope;
  const int *cand, *start;
  const float *in, *w, *bias, *cbias, *resid, *out0;
  void *out;
};

int tts_hfg_test_margin(void) { return TTS_HFG_TEST_MARGIN; }
int tts_hfg_test_seq_ints(void) { return HFG_SEQ; }            // the width of the product's candidate record
int tts_hfg_test_frames(int L) { return tts_diffusion_frames(L); } // T of an utterance of L latent rows, read from the product
// dynamic LDS of a convolution launch: hifigan.hip:408 (the 256-row tile) and hifigan.hip:403 (the small-M tile)
long long tts_hfg_test_lds_bytes(int kind, int taps, int dil) {
  return (long long)((kind == TTS_HFG_TEST_CONV_SMALL ? HFG_TS : HFG_TM) + (long long)(taps - 1) * dil) * 33 * 4;
}

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_HFG_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_HFG_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_HFG_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_HFG_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

int ceil8(int v) { return (v + 7) / 8 * 8; }
bool is_conv(int k) { return k == TTS_HFG_TEST_CONV || k == TTS_HFG_TEST_CONV_SMALL; }
int nt_of(int cout) { return cout >= 64 ? 2 : 1; } // hifigan.hip:406

// the product's table by hifigan_run's rule (the two lines are cited below), or false. maxW / maxKeep size the grids as hifigan_run's do.
bool table(const tts_hfg_case &c, std::vector<int> &seq, int &maxW, int &maxKeep, int64_t &lat_rows, int64_t &kept) {
  // every kernel indexes seq with blockIdx.y < ns
  if (c.ns < 1 || c.ns > TTS_HFG_TEST_MAX_CAND || !c.cand) return false;
  // the buffers are frames * rows-per-frame long: every f0 + t below is measured against `frames`
  if (c.frames < 8 || c.frames % 8 || c.frames > TTS_HFG_TEST_MAX_FRAMES) return false;
  seq.assign((size_t)HFG_SEQ * c.ns, 0);
  int64_t fpad = 0;
  maxW = maxKeep = 0; lat_rows = kept = 0;
  for (int s = 0; s < c.ns; s++) {
    const int *q = c.cand + TTS_HFG_TEST_CAND * s;
    const int W = q[0], voice = q[1], L = q[2], w0 = q[3], keep0 = q[4], keep_n = q[5];
    // rows [start * R, (start + W) * R) of in / out / resid / x: W >= 1, inside the buffer
    if (W < 1 || W > c.frames) return false;
    int64_t start = fpad;
    if (c.start) {
      start = c.start[s];
      // a start that is no multiple of 8 frames breaks the float4 alignment of no row, but it is no layout hifigan_run builds; one before the previous candidate's
      // padded end overlaps its rows: two workgroups would write the same output rows
      if (start % 8 || start < fpad) return false;
    }
    if (start + ceil8(W) > c.frames) return false; // the last row of the candidate, and its padding rows, lie inside every activation buffer
    // cbias[voice * cout + col], read by the convolutions' epilogue
    if (voice < 0 || voice >= c.n_voices) return false;
    // hfg_interp_kernel reads latent rows [first, first + L): L >= 1 (a0 = min(.., L - 1) must not be negative), at most the product's HFG_MAX_ROWS
    if (L < 1 || L > HFG_MAX_ROWS) return false;
    if (w0 < 0) return false;
    // INTERP: the window lies inside the utterance, as hifigan_run clips it (the kernel clamps its source rows, so this protects the meaning, not an address)
    if (c.kind == TTS_HFG_TEST_INTERP && (int64_t)w0 + W > tts_diffusion_frames(L)) return false;
    // hfg_post_kernel reads x rows around (keep0 * 256 + j) and writes audio[before * 256 + j] for j < keep_n * 256: the kept frames lie inside the window
    if (keep0 < 0 || keep_n < 1 || (int64_t)keep0 + keep_n > W) return false;
    int *r = &seq[(size_t)HFG_SEQ * s]; // hifigan.hip:363
    r[0] = (int)start; r[1] = W; r[2] = voice; r[3] = L; r[4] = (int)lat_rows; r[5] = (int)kept; r[6] = w0; r[7] = keep0; r[8] = keep_n;
    lat_rows += L; kept += keep_n; fpad = start + ceil8(W); // hifigan.hip:364
    maxW = std::max(maxW, W); maxKeep = std::max(maxKeep, keep_n);
  }
  return true;
}

bool valid(const tts_hfg_case &c, std::vector<int> &seq, int &maxW, int &maxKeep, int64_t &lat_rows, int64_t &kept) {
  if (c.kind < TTS_HFG_TEST_CONV || c.kind > TTS_HFG_TEST_POST) return false;
  if (!c.out || !c.in) return false; // the copy back; the first operand of every kernel
  // cond[v * 512 + co], g[v * 1024 + c]; cbias rows
  if (c.n_voices < 1 || c.n_voices > TTS_HFG_TEST_MAX_VOICES) return false;
  if (c.kind == TTS_HFG_TEST_COND) return c.w && c.bias; // w[co * 1024 + c], b[co]: fixed sizes
  if (!table(c, seq, maxW, maxKeep, lat_rows, kept)) return false;
  if (c.kind == TTS_HFG_TEST_INTERP) return true; // z[(f0 + t) * 1024 + c], t < W: inside `frames` by the table
  if (!c.w || !c.bias) return false;              // w[..], bias[col] / b[0]
  if (c.kind == TTS_HFG_TEST_POST) return (int64_t)c.frames * 256 <= TTS_HFG_TEST_MAX_ROWS; // x rows f0 * 256 + ti, 0 <= ti < W * 256: the kernel's own check
  // ---- the two convolution kernels
  // staging reads float4 in[t * cin + c0 + q], q < 32, for c0 = 0, 32, .. < cin: a cin that is no multiple of 32 reads past the row (and past the buffer on the last)
  if (c.cin < 32 || c.cin % 32 || c.cin > TTS_HFG_TEST_MAX_CH) return false;
  if (c.cout < 32 || c.cout > TTS_HFG_TEST_MAX_CH) return false;
  if (c.kind == TTS_HFG_TEST_CONV) {
    // columns n0 + n * 32 + lr of w, bias, cbias, out with n0 = z * 32 nt: cout must be whole groups of 32 nt
    if (c.cout % (32 * nt_of(c.cout))) return false;
  } else {
    // columns n0 + lr with n0 = z * 128 + wave * 32: cout must be whole groups of 128 (hifigan.hip:401)
    if (c.cout % 128) return false;
  }
  // w[(tap * cin + ..) * cout + ..], tap < taps; the LDS row (lr + tap * dil) * 33 < win * 33 needs taps >= 1, dil >= 1
  if (c.taps < 1 || c.dil < 1) return false;
  // phase < phases selects w + phase * taps * cin * cout and output row t * phases + phase; the 2-tap form of the transposed convolution is the only one the
  // kernel's lo = (phase + pad_t) / phases - 1 describes
  if (c.phases != 1 && c.phases != 2 && c.phases != 8) return false;
  if (c.phases > 1 && c.taps != 2) return false;
  // sx[win * 33] floats of dynamic LDS: 64 KB per workgroup
  if (tts_hfg_test_lds_bytes(c.kind, c.taps, c.dil) > TTS_HFG_TEST_LDS) return false;
  if (c.taps > TTS_HFG_TEST_MAX_TAPS || c.dil > TTS_HFG_TEST_MAX_DIL) return false; // the caps of the case matrix
  // rows f0 * rate + t of `in`, (f0 * rate + t) * phases + phase of out / resid
  if (c.rate < 1 || c.rate > TTS_HFG_TEST_MAX_RATE || (int64_t)c.frames * c.rate * c.phases > TTS_HFG_TEST_MAX_ROWS) return false;
  if (c.acc_mode < 0 || c.acc_mode > 2) return false;
  // in == out: a workgroup would stage rows that another one has already overwritten; out[o] of acc_mode 1, 2 and of resid == out needs a defined tensor
  if (c.alias < 0 || c.alias > 1) return false;
  if ((c.acc_mode || c.alias == 1) && !c.out0) return false;
  if (!(c.slope == c.slope)) return false;
  return true;
}

} // namespace

extern "C" {

// 0 for a case tts_hfg_test_run would launch, hipErrorInvalidValue otherwise (host only: no HIP call)
int tts_hfg_test_validate(const tts_hfg_case *c) {
  std::vector<int> seq;
  int a, b;
  int64_t l, k;
  return c && valid(*c, seq, a, b, l, k) ? 0 : (int)hipErrorInvalidValue;
}

// the HFG_SEQ table the harness builds for a case (host only), [ns][9] into `seq`; hipErrorInvalidValue for a refused case
int tts_hfg_test_table(const tts_hfg_case *c, int *out) {
  std::vector<int> seq;
  int a, b;
  int64_t l, k;
  if (!c || !out || c->kind == TTS_HFG_TEST_COND || !valid(*c, seq, a, b, l, k)) return (int)hipErrorInvalidValue;
  memcpy(out, seq.data(), seq.size() * sizeof(int));
  return 0;
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_hfg_test_run(const tts_hfg_case *cp) {
  std::vector<int> seq;
  int maxW = 0, maxKeep = 0;
  int64_t lat_rows = 0, kept = 0;
  if (!cp || !valid(*cp, seq, maxW, maxKeep, lat_rows, kept)) return (int)hipErrorInvalidValue;
  const tts_hfg_case &c = *cp;
  Dev in, out, w, bias, cbias, resid, dseq;
  const int B = c.ns;
  size_t in_bytes = 0, w_bytes = 0, b_bytes = 0, out_bytes = 0;
  switch (c.kind) {
    case TTS_HFG_TEST_CONV: case TTS_HFG_TEST_CONV_SMALL:
      in_bytes = (size_t)c.frames * c.rate * c.cin * 4; w_bytes = (size_t)c.phases * c.taps * c.cin * c.cout * 4; b_bytes = (size_t)c.cout * 4;
      out_bytes = (size_t)c.frames * c.rate * c.phases * c.cout * 4; break;
    case TTS_HFG_TEST_INTERP: in_bytes = (size_t)lat_rows * HFG_LAT * 4; out_bytes = (size_t)c.frames * HFG_LAT * 4; break;
    case TTS_HFG_TEST_COND: in_bytes = (size_t)c.n_voices * HFG_LAT * 4; w_bytes = (size_t)HFG_C0 * HFG_LAT * 4; b_bytes = HFG_C0 * 4; out_bytes = (size_t)c.n_voices * HFG_C0 * 4; break;
    default: in_bytes = (size_t)c.frames * 256 * 32 * 4; w_bytes = 7 * 32 * 4; b_bytes = 4; out_bytes = (size_t)kept * 256 * 4; break;
  }
  HT(in.alloc(in_bytes, 0)); HT(in.put(c.in));
  if (w_bytes) { HT(w.alloc(w_bytes, 0)); HT(w.put(c.w)); HT(bias.alloc(b_bytes, 0)); HT(bias.put(c.bias)); }
  if (c.kind != TTS_HFG_TEST_COND) { HT(dseq.alloc(seq.size() * 4, 0)); HT(dseq.put(seq.data())); }
  const bool conv = is_conv(c.kind);
  if (conv && c.cbias) { HT(cbias.alloc((size_t)c.n_voices * c.cout * 4, 0)); HT(cbias.put(c.cbias)); }
  if (conv && c.resid && c.alias == 0) { HT(resid.alloc(out_bytes, 0)); HT(resid.put(c.resid)); }
  HT(out.alloc(out_bytes, TTS_HFG_TEST_SENTINEL));
  if (conv && c.out0) HT(out.put(c.out0)); // acc_mode 1, 2 and resid == out read what the buffer holds

  const float *din = (const float *)in.data(), *dw = (const float *)w.data(), *db = (const float *)bias.data();
  const int *d_seq = (const int *)dseq.data();
  float *dy = (float *)out.data();
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    switch (c.kind) {
      case TTS_HFG_TEST_CONV: case TTS_HFG_TEST_CONV_SMALL: {
        const int cin = c.cin, cout = c.cout, taps = c.taps, dil = c.dil, phases = c.phases, rate = c.rate;
        HfgConv a{};
        a.in = din; a.out = dy; a.resid = c.alias == 1 ? dy : (const float *)resid.data(); a.w = dw; a.bias = db; a.cbias = (const float *)cbias.data(); a.seq = d_seq; // hifigan.hip:397
        a.cin = cin; a.cout = cout; a.taps = taps; a.dil = dil; a.lo = -dil * (taps - 1) / 2; a.phases = phases; a.pad_t = phases / 2; a.rate = rate; // hifigan.hip:398
        a.slope = c.slope; a.acc_mode = c.acc_mode; // hifigan.hip:399
        if (c.kind == TTS_HFG_TEST_CONV_SMALL) { // hifigan.hip:401-403 (the `cout % 128 == 0` rule is in valid(); the row threshold is the caller's choice of kind)
          const dim3 grid((unsigned)(((size_t)maxW * rate + HFG_TS - 1) / HFG_TS), (unsigned)B, (unsigned)(cout / 128 * phases));
          hfg_conv_small_kernel<<<grid, 256, (size_t)(HFG_TS + (taps - 1) * dil) * 33 * 4, s>>>(a);
        } else { // hifigan.hip:406-410
          const int nt = cout >= 64 ? 2 : 1;
          const dim3 grid((unsigned)(((size_t)maxW * rate + HFG_TM - 1) / HFG_TM), (unsigned)B, (unsigned)(cout / (32 * nt) * phases));
          const size_t lds = (size_t)(HFG_TM + (taps - 1) * dil) * 33 * 4;
          if (nt == 2) hfg_conv_kernel<2><<<grid, 256, lds, s>>>(a);
          else hfg_conv_kernel<1><<<grid, 256, lds, s>>>(a);
        }
        break;
      }
      case TTS_HFG_TEST_INTERP: // hifigan.hip:389
        hfg_interp_kernel<<<dim3(maxW, B), 256, 0, s>>>(din, d_seq, dy);
        break;
      case TTS_HFG_TEST_COND: // hifigan.hip:390
        hfg_cond_kernel<<<dim3(HFG_C0 / 4, c.n_voices), 256, 0, s>>>(dw, db, din, dy);
        break;
      default: // hifigan.hip:429
        hfg_post_kernel<<<dim3(maxKeep, B), 256, 0, s>>>(din, dw, db, d_seq, dy);
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
