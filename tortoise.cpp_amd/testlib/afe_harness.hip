// Test-only harness around the audio front-end's kernels (csrc/audio_frontend.hip: its kernels, without the host half, which needs the engine): host arrays in,
// host arrays out, one launch per call on a stream of its own. The grid and block expressions of afe_front are restated here, each beside the line it copies.
// Built as libtts_afe_test.so next to the product library (together with csrc/host_logic.cpp, which holds the tables the kernels read); it is not part of the
// product (tests/test_afe_kernels_gpu.py and tests/test_afe_harness_cpu.py are the only users).
//
// The GPU is shared: a case is validated completely BEFORE any HIP call (every address the chosen kernel reads or writes), and every device buffer carries a
// canary margin in front and behind, inside the same allocation, that is copied back with the payload.
#define TTS_AFE_KERNELS_ONLY
#include "../csrc/audio_frontend.hip"

#include <cstdint>
#include <cstring>
#include <vector>

using namespace tts;
hipEvent_t tts::prof_event(tts_ctx *) { return nullptr; } // profiling is off in this harness

extern "C" {

enum { TTS_AFE_TEST_MARGIN = 4096, TTS_AFE_TEST_SENTINEL = 0xCB }; // margin bytes on either side of every buffer; the byte every output buffer is pre-filled with
enum { TTS_AFE_TEST_RESAMPLE = 0, TTS_AFE_TEST_MEL80 = 1, TTS_AFE_TEST_MEL100 = 2, TTS_AFE_TEST_NONFINITE = 3 };
// caps, sized by the case matrix of tests/afe_cases.py: three ragged clips; the longest input is upstream's 132 300-sample window plus a crop margin
enum { TTS_AFE_TEST_MAX_CLIPS = 3, TTS_AFE_TEST_MAX_SAMPLES = 1 << 18 };

// One case. Host pointers only. `out` holds TTS_AFE_TEST_MARGIN bytes, the payload, TTS_AFE_TEST_MARGIN bytes.
//   in       the clips' samples, one after the other; in_len [n_clips]
//   RESAMPLE   orig_rate -> new_rate; out f32: ceil(n len / o) samples per clip, one after the other. Equal rates: no launch, a device copy (as afe_front does)
//   MEL80/100  start [n_clips], win [n_clips]: the virtual signal of AfeMelClip; norms null or [80] (MEL80 only); out f32 [bands][win / 256 + 1] per clip
//   NONFINITE  out: one uint32
struct tts_afe_case {
  int kind, n_clips, orig_rate, new_rate;
  const long long *in_len, *start, *win;
  const float *in, *norms;
  void *out;
};

int tts_afe_test_margin(void) { return TTS_AFE_TEST_MARGIN; }
int tts_afe_test_fpw(void) { return AFE_FPW; }         // frames per workgroup of afe_mel_kernel
int tts_afe_test_block(void) { return 256; }           // outputs per workgroup of afe_resample_kernel
// {o, n, width, taps} of a rate pair; the status of afe_resample_geometry (TTS_ERR_LIMIT for a table above the product's cap)
int tts_afe_test_geometry(int orig_rate, int new_rate, int *out4) {
  AfeResampleGeom g{};
  const int rc = afe_resample_geometry(orig_rate, new_rate, &g);
  if (out4) { out4[0] = g.o; out4[1] = g.n; out4[2] = g.width; out4[3] = g.taps; }
  return rc;
}
int tts_afe_test_table(int orig_rate, int new_rate, float *tab) { // [n][taps]
  AfeResampleGeom g{};
  const int rc = afe_resample_geometry(orig_rate, new_rate, &g);
  if (rc || !tab) return rc ? rc : TTS_ERR_ARG;
  afe_resample_table(g, tab);
  return TTS_OK;
}
void tts_afe_test_fft_tables(float *t2048) { afe_fft_tables(t2048, t2048 + 512, t2048 + 1024); } // tw_re[512] | tw_im[512] | win[1024]
// span [bands][3] and the weights (at most cap floats are written); returns the weight count
int tts_afe_test_filterbank(int bands, int *span, float *w, int cap) {
  std::vector<int> s;
  std::vector<float> v;
  const int rc = afe_filterbank(bands, s, v);
  if (rc) return rc;
  if (span) memcpy(span, s.data(), s.size() * sizeof(int));
  if (w) memcpy(w, v.data(), std::min<size_t>(v.size(), (size_t)std::max(cap, 0)) * sizeof(float));
  return (int)v.size();
}

} // extern "C"

namespace {

struct Dev { // one device allocation: margin | payload | margin
  char *p = nullptr;
  size_t bytes = 0;
  ~Dev() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t payload, int fill) {
    bytes = payload;
    hipError_t e = hipMalloc((void **)&p, payload + 2 * TTS_AFE_TEST_MARGIN);
    if (e != hipSuccess) { p = nullptr; return e; }
    return hipMemset(p, fill, payload + 2 * TTS_AFE_TEST_MARGIN);
  }
  char *data() const { return p ? p + TTS_AFE_TEST_MARGIN : nullptr; }
  hipError_t put(const void *h) { return hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice); }
  hipError_t get_all(void *h) const { return hipMemcpy(h, p, bytes + 2 * TTS_AFE_TEST_MARGIN, hipMemcpyDeviceToHost); }
};

struct Plan {
  AfeResampleGeom g{};
  std::vector<AfeResClip> res;
  std::vector<AfeMelClip> mel;
  long long total_in = 0, total_out = 0, max_out = 0; // floats (NONFINITE: total_out = 1 word)
  int max_frames = 0, bands = 0;
};

// 0 for a case that may run; hipErrorInvalidValue for a refused one; TTS_ERR_LIMIT for a rate pair whose table the product refuses
int valid(const tts_afe_case &c, Plan &pl) {
  const int bad = (int)hipErrorInvalidValue;
  if (c.kind < TTS_AFE_TEST_RESAMPLE || c.kind > TTS_AFE_TEST_NONFINITE) return bad;
  if (!c.in || !c.out || !c.in_len) return bad; // the first operand of every kernel; the copy back
  if (c.n_clips < 1 || c.n_clips > TTS_AFE_TEST_MAX_CLIPS) return bad; // clips[blockIdx.y], blockIdx.y < n_clips
  for (int s = 0; s < c.n_clips; s++) {
    // xs[i], 0 <= i < in_len, of a buffer of total_in floats
    if (c.in_len[s] < 1 || c.in_len[s] > TTS_AFE_TEST_MAX_SAMPLES) return bad;
  }
  const bool mel = c.kind == TTS_AFE_TEST_MEL80 || c.kind == TTS_AFE_TEST_MEL100;
  if (c.kind == TTS_AFE_TEST_RESAMPLE) {
    if (c.orig_rate < 1 || c.new_rate < 1) return bad;
    const int rc = afe_resample_geometry(c.orig_rate, c.new_rate, &pl.g); // tab[p * taps + k], p < n, k < taps: the table the harness uploads has n * taps entries
    if (rc) return rc == TTS_ERR_LIMIT ? rc : bad;
  }
  if (mel) {
    if (!c.start || !c.win) return bad;
    if (c.norms && c.kind != TTS_AFE_TEST_MEL80) return bad; // the product divides the 80-band side only
    pl.bands = c.kind == TTS_AFE_TEST_MEL80 ? 80 : 100;
  }
  for (int s = 0; s < c.n_clips; s++) {
    const long long n = c.in_len[s];
    if (c.kind == TTS_AFE_TEST_RESAMPLE) {
      const long long out = afe_resample_len(pl.g, n); // y[out_off + j], j < out_len
      if (out < 1 || out > 4LL * TTS_AFE_TEST_MAX_SAMPLES) return bad;
      pl.res.push_back(AfeResClip{pl.total_in, n, pl.total_out, out});
      pl.total_out += out; pl.max_out = std::max(pl.max_out, out);
    } else if (mel) {
      const long long st = c.start[s], w = c.win[s];
      // reflect: j = -j needs 512 <= win - 1 (j < win after one fold), j = 2 (win - 1) - j >= 0 needs the last frame's end (frames - 1) * 256 + 511 <= 2 (win - 1),
      // which win >= 513 gives; xs[j] is read for j < n - start only: start inside the clip
      if (w < 513 || w > TTS_AFE_TEST_MAX_SAMPLES || st < 0 || st >= n) return bad;
      const int frames = (int)(w / 256) + 1;
      pl.mel.push_back(AfeMelClip{pl.total_in, n, st, w, pl.total_out, frames, 0}); // mel[mel_off + b * frames + f], b < bands, f < frames
      pl.total_out += (long long)pl.bands * frames; pl.max_frames = std::max(pl.max_frames, frames);
    }
    pl.total_in += n;
  }
  if (c.kind == TTS_AFE_TEST_NONFINITE) pl.total_out = 1;
  return 0;
}

} // namespace

extern "C" {

// 0 for a case tts_afe_test_run would launch (host only: no HIP call)
int tts_afe_test_validate(const tts_afe_case *c) {
  Plan pl;
  return c ? valid(*c, pl) : (int)hipErrorInvalidValue;
}
// floats of the payload of `out` for a valid case, or the refusal's status (negative or hipErrorInvalidValue, as tts_afe_test_validate)
long long tts_afe_test_out_floats(const tts_afe_case *c) {
  Plan pl;
  const int rc = c ? valid(*c, pl) : (int)hipErrorInvalidValue;
  return rc ? -(long long)(rc < 0 ? -rc : rc) : pl.total_out;
}

#define HT(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

int tts_afe_test_run(const tts_afe_case *cp) {
  Plan pl;
  if (!cp) return (int)hipErrorInvalidValue;
  const int rc = valid(*cp, pl);
  if (rc) return rc;
  const tts_afe_case &c = *cp;
  Dev in, out, tab, meta, fft, span, fbw, norms;
  HT(in.alloc((size_t)pl.total_in * 4, 0)); HT(in.put(c.in));
  HT(out.alloc((size_t)pl.total_out * 4, TTS_AFE_TEST_SENTINEL));
  const bool mel = !pl.mel.empty();
  const bool copy = c.kind == TTS_AFE_TEST_RESAMPLE && c.orig_rate == c.new_rate;
  if (c.kind == TTS_AFE_TEST_RESAMPLE && !copy) {
    std::vector<float> h((size_t)pl.g.n * pl.g.taps);
    afe_resample_table(pl.g, h.data());
    HT(tab.alloc(h.size() * 4, 0)); HT(tab.put(h.data()));
    HT(meta.alloc(pl.res.size() * sizeof(AfeResClip), 0)); HT(meta.put(pl.res.data()));
  }
  if (mel) {
    std::vector<float> t(2048), w;
    std::vector<int> sp;
    afe_fft_tables(t.data(), t.data() + 512, t.data() + 1024);
    afe_filterbank(pl.bands, sp, w);
    HT(fft.alloc(t.size() * 4, 0)); HT(fft.put(t.data()));
    HT(span.alloc(sp.size() * 4, 0)); HT(span.put(sp.data()));
    HT(fbw.alloc(w.size() * 4, 0)); HT(fbw.put(w.data()));
    HT(meta.alloc(pl.mel.size() * sizeof(AfeMelClip), 0)); HT(meta.put(pl.mel.data()));
    if (c.norms) { HT(norms.alloc(80 * 4, 0)); HT(norms.put(c.norms)); }
  }
  if (c.kind == TTS_AFE_TEST_NONFINITE) HT(hipMemset(out.data(), 0, 4)); // the product zeroes the count before the launch
  const float *din = (const float *)in.data();
  float *dy = (float *)out.data();
  hipStream_t s;
  HT(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipDeviceSynchronize(); // the fills above ran on the null stream
  if (e == hipSuccess) {
    const int nc = c.n_clips;
    const float *f = (const float *)fft.data();
    const float log_floor = (float)std::log(1e-5); // afe_front's constant
    switch (c.kind) {
      case TTS_AFE_TEST_RESAMPLE:
        if (copy) e = hipMemcpyAsync(dy, din, (size_t)pl.total_in * 4, hipMemcpyDeviceToDevice, s); // afe_front: equal rates pass through
        else // afe_front's 22.05 k -> 24 k launch (one table, all clips); its per-clip launch is this one with n_clips = 1
          afe_resample_kernel<<<dim3((unsigned)((pl.max_out + 255) / 256), nc), 256, 0, s>>>(din, (const float *)tab.data(), (const AfeResClip *)meta.data(), pl.g.o, pl.g.n,
                                                                                             pl.g.width, pl.g.taps, dy);
        break;
      case TTS_AFE_TEST_MEL80:
        afe_mel_kernel<80, 2><<<dim3((pl.max_frames + AFE_FPW - 1) / AFE_FPW, nc), 256, 0, s>>>(din, (const AfeMelClip *)meta.data(), f, f + 512, f + 1024, (const int *)span.data(),
                                                                                               (const float *)fbw.data(), (const float *)norms.data(), log_floor, dy);
        break;
      case TTS_AFE_TEST_MEL100:
        afe_mel_kernel<100, 1><<<dim3((pl.max_frames + AFE_FPW - 1) / AFE_FPW, nc), 256, 0, s>>>(din, (const AfeMelClip *)meta.data(), f, f + 512, f + 1024, (const int *)span.data(),
                                                                                                (const float *)fbw.data(), nullptr, log_floor, dy);
        break;
      default:
        afe_nonfinite_kernel<<<(unsigned)std::min<long long>((pl.total_in + 255) / 256, 1024), 256, 0, s>>>(din, pl.total_in, (unsigned int *)dy);
        break;
    }
    if (e == hipSuccess) e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
  HT(out.get_all(c.out));
  return (int)(e != hipSuccess ? e : es);
}

} // extern "C"
