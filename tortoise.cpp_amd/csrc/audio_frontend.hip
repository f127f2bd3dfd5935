// Audio front-end of the two voice-conditioning encoders on MI355X (gfx950): clips -> both voice latents without a host round trip for the samples.
//   tts_voice_from_audio / tts_audio_mel (include/tortoise_mi355x.h)
// Upstream tortoise-tts' load_audio + get_conditioning_latents (restated from memory): torchaudio.functional.resample with its defaults to
// 22 050 Hz, from there again to 24 000 Hz; a 132 300-sample window -> 80-band HTK power log-mel -> tts_voice_latent's encoder; the first 102 400 samples at
// 24 kHz -> 100-band Slaney magnitude log-mel -> tts_diffusion_conditioning_latent's encoder. The mel definitions are those of tts_host_mel_voice80 and
// tts_host_mel_diffusion100 (host_logic.cpp), the yardstick the kernels are held against.
//
// All f32, no fast-math. Every table (resampler taps, twiddles, Hann window, filterbank) is evaluated in double on the host and rounded once
// (host_logic.cpp: afe_*). Every sum has one fixed order that depends on the output element alone: a result never depends on the grid, on the other clips
// of the call or on an earlier call. These run once per voice: written for clarity, sized from the compiler's resource summary (profiles/voice_from_audio.txt).
#include "common.h"
#include <cmath>

namespace tts {

namespace {
constexpr int AFE_NFFT = 1024, AFE_HOP = 256, AFE_BINS = 513;
// Frames per workgroup of afe_mel_kernel. LDS per workgroup = FPW x (2 x 1024 + 516) floats + 1024 floats of twiddles = 45 120 B at 4 (the compiler's resource
// summary: 34 VGPRs, no scratch, 3 waves per SIMD): three workgroups of 256 threads per CU (160 KB), and a 401-frame clip still fills 101 workgroups. 8 frames
// would leave one workgroup per CU beside its neighbour's 86 KB and halve that grid.
constexpr int AFE_FPW = 4;

// One clip of a resampler launch: x[in_off .. + in_len) -> y[out_off .. + out_len)
struct AfeResClip { long long in_off, in_len, out_off, out_len; };
// One clip of a mel launch. The frames are taken from a VIRTUAL signal of `win` samples: v[j] = x[src_off + start + j] while start + j < n, else 0 (the zero
// padding behind a short clip); reflect padding of 512 on both sides of v; frames = win / 256 + 1, written [BANDS][frames] at mel_off.
struct AfeMelClip { long long src_off, n, start, win, mel_off; int frames, pad_; };

// y[j] = sum_k tab[j % n][k] * xpad[(j / n) * o + k], xpad = x behind `width` zeros and before zeros; k ascending, one fmaf per tap
__global__ __launch_bounds__(256) void afe_resample_kernel(const float *__restrict__ x, const float *__restrict__ tab, const AfeResClip *__restrict__ clips, int o,
                                                           int n, int width, int taps, float *__restrict__ y) {
  const AfeResClip c = clips[blockIdx.y];
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= c.out_len) return;
  const long long blk = j / n;
  const int p = (int)(j - blk * n);
  const float *t = tab + (size_t)p * taps;
  const long long i0 = blk * o - width; // the sample under tap 0
  const float *xs = x + c.in_off;
  float acc = 0.f;
  for (int k = 0; k < taps; k++) {
    const long long i = i0 + k;
    const float v = (i >= 0 && i < c.in_len) ? xs[i] : 0.f;
    acc = __fmaf_rn(t[k], v, acc);
  }
  y[c.out_off + j] = acc;
}

// count += the number of non-finite values of x[0 .. n)
__global__ __launch_bounds__(256) void afe_nonfinite_kernel(const float *__restrict__ x, long long n, unsigned int *__restrict__ count) {
  unsigned int bad = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) bad += isfinite(x[i]) ? 0u : 1u;
  for (int d = 32; d; d >>= 1) bad += __shfl_xor(bad, d);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, bad);
}

// STFT (n_fft 1024, hop 256, periodic Hann, centre, reflect) + mel filterbank + log of AFE_FPW frames of one clip. POWER 2: |X|^2 (AR side), 1: |X|.
// Per frame: the windowed samples enter LDS in bit-reversed order, ten radix-2 decimation-in-time stages (512 butterflies each, twiddle w[k * 1024 / len] from
// the table) leave X[0 .. 1023] in place; bins 0 .. 512 -> spec; band b = sum over its non-zero span, bins ascending, one fmaf per bin;
// out = (m > 1e-5 ? logf(m) : log_floor) / norm[b], log_floor = (float)log(1e-5) from the host (so that silence is the same constant in every cell).
template <int BANDS, int POWER>
__global__ __launch_bounds__(256) void afe_mel_kernel(const float *__restrict__ x, const AfeMelClip *__restrict__ clips, const float *__restrict__ tw_re,
                                                      const float *__restrict__ tw_im, const float *__restrict__ win, const int *__restrict__ span,
                                                      const float *__restrict__ fbw, const float *__restrict__ norms, float log_floor, float *__restrict__ mel) {
  __shared__ float s_re[AFE_FPW][AFE_NFFT], s_im[AFE_FPW][AFE_NFFT], s_spec[AFE_FPW][516];
  __shared__ float s_twr[512], s_twi[512];
  const AfeMelClip c = clips[blockIdx.y];
  const int f0 = blockIdx.x * AFE_FPW;
  if (f0 >= c.frames) return;
  const int nf = min(AFE_FPW, c.frames - f0);
  const int tid = threadIdx.x;
  for (int k = tid; k < 512; k += 256) { s_twr[k] = tw_re[k]; s_twi[k] = tw_im[k]; }
  const float *xs = x + c.src_off + c.start;
  const long long avail = c.n - c.start; // samples of the virtual signal that exist; the rest of `win` is zero padding
  for (int e = tid; e < nf * AFE_NFFT; e += 256) {
    const int f = e >> 10, i = e & 1023;
    long long j = (long long)(f0 + f) * AFE_HOP + i - AFE_NFFT / 2;
    if (j < 0) j = -j;
    if (j >= c.win) j = 2 * (c.win - 1) - j;
    const float v = j < avail ? xs[j] : 0.f;
    s_re[f][__brev((unsigned)i) >> 22] = v * win[i];
    s_im[f][i] = 0.f;
  }
  __syncthreads();
  for (int len = 2; len <= AFE_NFFT; len <<= 1) {
    const int half = len >> 1, step = AFE_NFFT / len;
    for (int e = tid; e < nf * 512; e += 256) {
      const int f = e >> 9, b = e & 511;
      const int k = b & (half - 1), lo = ((b - k) << 1) + k, hi = lo + half;
      const float wr = s_twr[k * step], wi = s_twi[k * step];
      const float ar = s_re[f][hi], ai = s_im[f][hi], ur = s_re[f][lo], ui = s_im[f][lo];
      const float vr = __fmaf_rn(ar, wr, -(ai * wi)), vi = __fmaf_rn(ar, wi, ai * wr);
      s_re[f][lo] = ur + vr; s_im[f][lo] = ui + vi;
      s_re[f][hi] = ur - vr; s_im[f][hi] = ui - vi;
    }
    __syncthreads();
  }
  for (int e = tid; e < nf * AFE_BINS; e += 256) {
    const int f = e / AFE_BINS, k = e - f * AFE_BINS;
    const float re = s_re[f][k], im = s_im[f][k];
    const float p = __fmaf_rn(re, re, im * im);
    s_spec[f][k] = POWER == 2 ? p : sqrtf(p);
  }
  __syncthreads();
  for (int e = tid; e < nf * BANDS; e += 256) {
    const int b = e / nf, f = e - b * nf; // neighbouring threads: neighbouring frames of one band (the output's fast axis)
    const int k0 = span[3 * b], cnt = span[3 * b + 1];
    const float *w = fbw + span[3 * b + 2];
    float m = 0.f;
    for (int k = 0; k < cnt; k++) m = __fmaf_rn(w[k], s_spec[f][k0 + k], m);
    const float lg = m > 1e-5f ? logf(m) : log_floor;
    mel[c.mel_off + (long long)b * c.frames + f0 + f] = norms ? lg / norms[b] : lg;
  }
}
} // namespace

#ifndef TTS_AFE_KERNELS_ONLY
// ------------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------------
struct AfeTable { AfeResampleGeom g; DevBuf tab; };
struct AfeState {
  std::map<std::pair<int, int>, std::unique_ptr<AfeTable>> tables; // one per reduced rate pair
  DevBuf fft, span[2], fbw[2], norms; // fft: tw_re[512] | tw_im[512] | win[1024]; [0] 80 bands, [1] 100 bands
  DevBuf audio, a22, a24, meta, count, mel;
  std::vector<AfeResClip> cls_meta_h; // outlives the call: the copy is asynchronous
  DevBuf cls_meta; // afe_resample_to_24k's clip records: the classifier's calls share nothing but the tap tables with the voice calls
  std::vector<AfeResClip> w2v_meta_h;
  DevBuf w2v_meta; // afe_resample_to_16k's clip records (the aligner's calls)
  bool ready = false;
};
void afe_free(AfeState *s) { delete s; }

namespace {
struct AfeClipPlan {
  int64_t src_off, n_src, off22, n22, off24, n24; // n22: samples at 22 050 Hz (= the source when its rate is 22 050); n24: those computed at 24 kHz
  int rate;
  AfeMelClip m80, m100;
};
struct AfePlan {
  std::vector<AfeClipPlan> clips;
  int64_t total_src = 0, total22 = 0, total24 = 0;
  std::vector<int32_t> frames80, frames100;
};

int afe_table(tts_ctx *ctx, AfeState *st, int orig, int target, AfeTable **out) {
  AfeResampleGeom g;
  const int rc = afe_resample_geometry(orig, target, &g);
  if (rc) return rc;
  auto key = std::make_pair(g.o, g.n);
  auto it = st->tables.find(key);
  if (it == st->tables.end()) {
    std::unique_ptr<AfeTable> t(new AfeTable());
    t->g = g;
    std::vector<float> h((size_t)g.n * g.taps);
    afe_resample_table(g, h.data());
    TTS_HIP(ctx, t->tab.reserve(h.size() * 4));
    TTS_HIP(ctx, hipMemcpy(t->tab.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    it = st->tables.emplace(key, std::move(t)).first;
  }
  *out = it->second.get();
  return TTS_OK;
}

int afe_init(tts_ctx *ctx) {
  if (!ctx->afe) ctx->afe = new AfeState();
  AfeState *st = ctx->afe;
  if (st->ready) return TTS_OK;
  std::vector<float> t(2048);
  afe_fft_tables(t.data(), t.data() + 512, t.data() + 1024);
  TTS_HIP(ctx, st->fft.reserve(t.size() * 4));
  TTS_HIP(ctx, hipMemcpy(st->fft.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
  for (int i = 0; i < 2; i++) {
    std::vector<int> span;
    std::vector<float> w;
    afe_filterbank(i ? 100 : 80, span, w);
    TTS_HIP(ctx, st->span[i].reserve(span.size() * 4));
    TTS_HIP(ctx, st->fbw[i].reserve(w.size() * 4));
    TTS_HIP(ctx, hipMemcpy(st->span[i].p, span.data(), span.size() * 4, hipMemcpyHostToDevice));
    TTS_HIP(ctx, hipMemcpy(st->fbw[i].p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  }
  TTS_HIP(ctx, st->norms.reserve(80 * 4));
  TTS_HIP(ctx, st->count.reserve(4));
  st->ready = true;
  return TTS_OK;
}

// Every check that needs no device, and the layout of the call: where each clip's samples lie at the three rates and what its two mel launches read.
int afe_plan(tts_ctx *ctx, const char *fn, const int64_t *n_samples, const int32_t *rates, int n_clips, const tts_voice_audio_opts *opts, bool want80,
             bool want100, AfePlan &pl) {
  if (opts && opts->struct_size < sizeof(tts_voice_audio_opts)) return fail(ctx, TTS_ERR_ARG, "%s: struct_size %u, version 8 declares %zu bytes (set it to sizeof(tts_voice_audio_opts))", fn, opts->struct_size, sizeof(tts_voice_audio_opts));
  const bool full = opts && opts->full_clips;
  if (opts && (opts->full_clips != 0 && opts->full_clips != 1)) return fail(ctx, TTS_ERR_ARG, "%s: full_clips %d: 0 or 1", fn, opts->full_clips);
  const int64_t crop = opts ? opts->crop_offset : 0;
  if (crop < 0) return fail(ctx, TTS_ERR_ARG, "%s: crop_offset %lld: at least 0", fn, (long long)crop);
  if (n_clips < 1 || n_clips > 4096) return fail(ctx, TTS_ERR_ARG, "%s: %d clips (1 .. 4096 expected)", fn, n_clips);
  AfeResampleGeom g24;
  afe_resample_geometry(22050, 24000, &g24);
  long long mel80 = 0, mel100 = 0;
  for (int s = 0; s < n_clips; s++) {
    AfeClipPlan c{};
    c.n_src = n_samples[s]; c.rate = rates[s];
    if (c.rate < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: sample rate %d", fn, s, c.rate);
    if (c.n_src < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %lld samples", fn, s, (long long)c.n_src);
    if (c.n_src > (1 << 26)) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %lld samples, at most 2^26", fn, s, (long long)c.n_src);
    AfeResampleGeom g;
    const int rc = afe_resample_geometry(c.rate, 22050, &g);
    if (rc == TTS_ERR_LIMIT) return fail(ctx, rc, "%s: clip %d: %d Hz -> 22050 Hz takes a tap table of %d x %d entries, at most %lld", fn, s, c.rate, g.n, g.taps, (long long)AFE_MAX_TABLE);
    c.n22 = c.rate == 22050 ? c.n_src : afe_resample_len(g, c.n_src);
    if (c.n22 > (1 << 26)) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %lld samples at 22050 Hz, at most 2^26", fn, s, (long long)c.n22);
    c.n24 = afe_resample_len(g24, c.n22);
    if (!full) c.n24 = std::min<int64_t>(c.n24, AFE_WIN100); // the diffusion side reads the first 102 400 samples only
    if (full && ((want80 && c.n22 <= 512) || (want100 && c.n24 <= 512)))
      return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %lld samples at 22050 Hz: reflect padding needs more than 512 (full_clips)", fn, s, (long long)c.n22);
    c.src_off = pl.total_src; c.off22 = pl.total22; c.off24 = pl.total24;
    pl.total_src += c.n_src; pl.total22 += c.n22; pl.total24 += c.n24;
    // AR side: the window, or the whole clip
    const int64_t w80 = full ? c.n22 : AFE_WIN80, w100 = full ? c.n24 : AFE_WIN100;
    c.m80 = AfeMelClip{c.off22, c.n22, c.n22 > w80 ? std::min(crop, c.n22 - w80) : 0, w80, mel80, (int)(w80 / AFE_HOP) + 1, 0};
    c.m100 = AfeMelClip{c.off24, c.n24, 0, w100, mel100, (int)(w100 / AFE_HOP) + 1, 0};
    if (c.m80.frames > 16384) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %d mel frames, at most 16384", fn, s, c.m80.frames);
    mel80 += 80LL * c.m80.frames; mel100 += 100LL * c.m100.frames;
    pl.frames80.push_back(c.m80.frames); pl.frames100.push_back(c.m100.frames);
    pl.clips.push_back(c);
  }
  return TTS_OK;
}

// Upload, the finite count, the resamplers and the mel launches, all on ctx->stream; then the one host read: the count. d_mel80 / d_mel100 null: that side is skipped.
int afe_front(tts_ctx *ctx, const char *fn, const float *audio, const AfePlan &pl, const tts_voice_audio_opts *opts, float *d_mel80, float *d_mel100) {
  AfeState *st = ctx->afe;
  const int nc = (int)pl.clips.size();
  std::vector<AfeTable *> tabs(nc, nullptr);
  AfeTable *t24 = nullptr;
  for (int s = 0; s < nc; s++)
    if (pl.clips[s].rate != 22050) { const int rc = afe_table(ctx, st, pl.clips[s].rate, 22050, &tabs[s]); if (rc) return rc; }
  if (d_mel100) { const int rc = afe_table(ctx, st, 22050, 24000, &t24); if (rc) return rc; }
  TTS_HIP(ctx, st->audio.reserve((size_t)pl.total_src * 4));
  TTS_HIP(ctx, st->a22.reserve((size_t)pl.total22 * 4));
  if (d_mel100) TTS_HIP(ctx, st->a24.reserve((size_t)pl.total24 * 4));
  // meta: [nc] source -> 22.05 k | [nc] 22.05 k -> 24 k (AfeResClip), then [nc] 80-band | [nc] 100-band (AfeMelClip)
  const size_t res_bytes = (size_t)2 * nc * sizeof(AfeResClip), mel_bytes = (size_t)2 * nc * sizeof(AfeMelClip);
  TTS_HIP(ctx, st->meta.reserve(res_bytes + mel_bytes));
  std::vector<AfeResClip> rc_h(2 * nc);
  std::vector<AfeMelClip> mc_h(2 * nc);
  for (int s = 0; s < nc; s++) {
    const AfeClipPlan &c = pl.clips[s];
    rc_h[s] = AfeResClip{c.src_off, c.n_src, c.off22, c.n22};
    rc_h[nc + s] = AfeResClip{c.off22, c.n22, c.off24, c.n24};
    mc_h[s] = c.m80; mc_h[nc + s] = c.m100;
  }
  AfeResClip *d_res = st->meta.as<AfeResClip>();
  AfeMelClip *d_mc = (AfeMelClip *)(st->meta.as<char>() + res_bytes);
  hipStream_t sm = ctx->stream;
  TTS_HIP(ctx, hipMemcpyAsync(d_res, rc_h.data(), res_bytes, hipMemcpyHostToDevice, sm));
  TTS_HIP(ctx, hipMemcpyAsync(d_mc, mc_h.data(), mel_bytes, hipMemcpyHostToDevice, sm));
  TTS_HIP(ctx, hipMemcpyAsync(st->audio.p, audio, (size_t)pl.total_src * 4, hipMemcpyHostToDevice, sm));
  TTS_HIP(ctx, hipMemsetAsync(st->count.p, 0, 4, sm));
  const float *norms = nullptr;
  if (opts && opts->mel_norms80 && d_mel80) {
    TTS_HIP(ctx, hipMemcpyAsync(st->norms.p, opts->mel_norms80, 80 * 4, hipMemcpyHostToDevice, sm));
    norms = st->norms.as<float>();
  }
  const float *src = st->audio.as<float>();
  float *a22 = st->a22.as<float>(), *a24 = st->a24.as<float>();
  {
    ProfScope ps(ctx, "afe_finite", (double)pl.total_src);
    afe_nonfinite_kernel<<<(unsigned)std::min<int64_t>((pl.total_src + 255) / 256, 1024), 256, 0, sm>>>(src, pl.total_src, st->count.as<unsigned int>());
  }
  int max80 = 0, max100 = 0;
  int64_t max24 = 0;
  for (int s = 0; s < nc; s++) {
    const AfeClipPlan &c = pl.clips[s];
    max80 = std::max(max80, c.m80.frames); max100 = std::max(max100, c.m100.frames); max24 = std::max(max24, c.n24);
    if (!tabs[s]) { // already at 22 050 Hz: the samples pass through bit for bit
      TTS_HIP(ctx, hipMemcpyAsync(a22 + c.off22, src + c.src_off, (size_t)c.n_src * 4, hipMemcpyDeviceToDevice, sm));
      continue;
    }
    const AfeResampleGeom &g = tabs[s]->g;
    ProfScope ps(ctx, "afe_resample", 2.0 * c.n22 * g.taps);
    afe_resample_kernel<<<dim3((unsigned)((c.n22 + 255) / 256), 1), 256, 0, sm>>>(src, tabs[s]->tab.as<float>(), d_res + s, g.o, g.n, g.width, g.taps, a22);
  }
  const float *fft = st->fft.as<float>();
  const float log_floor = (float)std::log(1e-5);
  if (d_mel80) {
    ProfScope ps(ctx, "afe_mel", 0);
    afe_mel_kernel<80, 2><<<dim3((max80 + AFE_FPW - 1) / AFE_FPW, nc), 256, 0, sm>>>(a22, d_mc, fft, fft + 512, fft + 1024, st->span[0].as<int>(), st->fbw[0].as<float>(), norms, log_floor, d_mel80);
  }
  if (d_mel100) {
    const AfeResampleGeom &g = t24->g;
    {
      ProfScope ps(ctx, "afe_resample", 2.0 * pl.total24 * g.taps);
      afe_resample_kernel<<<dim3((unsigned)((max24 + 255) / 256), nc), 256, 0, sm>>>(a22, t24->tab.as<float>(), d_res + nc, g.o, g.n, g.width, g.taps, a24);
    }
    ProfScope ps(ctx, "afe_mel", 0);
    afe_mel_kernel<100, 1><<<dim3((max100 + AFE_FPW - 1) / AFE_FPW, nc), 256, 0, sm>>>(a24, d_mc + nc, fft, fft + 512, fft + 1024, st->span[1].as<int>(), st->fbw[1].as<float>(), nullptr, log_floor, d_mel100);
  }
  TTS_HIP(ctx, hipGetLastError());
  unsigned int bad = 0;
  TTS_HIP(ctx, hipMemcpyAsync(&bad, st->count.p, 4, hipMemcpyDeviceToHost, sm));
  TTS_HIP(ctx, hipStreamSynchronize(sm));
  if (bad) return fail(ctx, TTS_ERR_ARG, "%s: the audio holds %u non-finite samples", fn, bad);
  return TTS_OK;
}
} // namespace

int afe_voice_from_audio(tts_ctx *ctx, const float *audio, const int64_t *n_samples, const int32_t *sample_rate, int n_clips, const tts_voice_audio_opts *opts,
                         float *out1024, float *out2048) {
  const char *fn = "tts_voice_from_audio";
  if (!audio || !n_samples || !sample_rate || (!out1024 && !out2048)) return fail(ctx, TTS_ERR_ARG, "%s: bad arguments", fn);
  if (out1024 && !ctx->venc) return fail(ctx, TTS_ERR_STATE, "tts_load_voice_encoder not called");
  if (out2048 && !ctx->dcond) return fail(ctx, TTS_ERR_STATE, "tts_load_diffusion_conditioning_encoder not called");
  AfePlan pl;
  int rc = afe_plan(ctx, fn, n_samples, sample_rate, n_clips, opts, out1024 != nullptr, out2048 != nullptr, pl);
  if (rc) return rc;
  if ((rc = afe_init(ctx))) return rc;
  float *d80 = nullptr, *d100 = nullptr;
  if (out1024 && (rc = voice_enc_begin(ctx, pl.frames80.data(), n_clips, &d80))) return rc;
  if (out2048 && (rc = diff_cond_enc_begin(ctx, pl.frames100.data(), n_clips, &d100))) return rc;
  if ((rc = afe_front(ctx, fn, audio, pl, opts, d80, d100))) return rc;
  // the outputs are written only when both sides have succeeded
  std::vector<float> o1(1024), o2(2048);
  if (out1024 && (rc = voice_enc_run(ctx, o1.data()))) return rc;
  if (out2048 && (rc = diff_cond_enc_run(ctx, o2.data()))) return rc;
  if (out1024) memcpy(out1024, o1.data(), 1024 * 4);
  if (out2048) memcpy(out2048, o2.data(), 2048 * 4);
  return TTS_OK;
}

// tts_cvvp_voice_audio: the AR side's mel (the window, crop_offset, mel_norms80) written straight into the CVVP stem's input buffer; no host copy of the mel
int afe_cvvp_voice_audio(tts_ctx *ctx, const float *audio, const int64_t *n_samples, const int32_t *sample_rate, int n_clips, const tts_voice_audio_opts *opts,
                         float *latents_out) {
  const char *fn = "tts_cvvp_voice_audio";
  if (!audio || !n_samples || !sample_rate || !latents_out) return fail(ctx, TTS_ERR_ARG, "%s: bad arguments", fn);
  if (!ctx->cvvp) return fail(ctx, TTS_ERR_STATE, "tts_load_cvvp not called");
  AfePlan pl;
  int rc = afe_plan(ctx, fn, n_samples, sample_rate, n_clips, opts, true, false, pl);
  if (rc) return rc;
  if (opts && opts->full_clips) return fail(ctx, TTS_ERR_ARG, "%s: full_clips 1: CVVP scores the windowed clip, as upstream does; whole clips are not supported", fn);
  if ((rc = afe_init(ctx))) return rc;
  float *d80 = nullptr;
  if ((rc = cvvp_voice_begin(ctx, pl.frames80.data(), n_clips, &d80))) return rc;
  if ((rc = afe_front(ctx, fn, audio, pl, opts, d80, nullptr))) return rc;
  return cvvp_voice_run(ctx, latents_out);
}

// tts_dvae_codes_audio: the AR side's mel of the WHOLE clip (full_clips 1 whatever opts says: the codes are the recording's; mel_norms80 from opts) written
// straight into the DVAE stem's input buffer; no host copy of the mel. The bits of tts_dvae_codes on tts_audio_mel(bands 80, full_clips 1) of every clip.
int afe_dvae_codes_audio(tts_ctx *ctx, const float *audio, const int64_t *n_samples, const int32_t *sample_rate, int n_clips, const tts_voice_audio_opts *opts,
                         int32_t *codes_out, int32_t *n_codes_out, int code_stride, float *z_out) {
  const char *fn = "tts_dvae_codes_audio";
  if (!ctx->dvae) return fail(ctx, TTS_ERR_STATE, "tts_load_dvae not called");
  if (!audio || !n_samples || !sample_rate || !codes_out || !n_codes_out || n_clips < 1 || code_stride < 1) return fail(ctx, TTS_ERR_ARG, "%s: bad argument", fn);
  if (dvae_mel_channels(ctx) != 80) return fail(ctx, TTS_ERR_STATE, "%s: the loaded DVAE reads %d mel channels, the audio front end makes 80", fn, dvae_mel_channels(ctx));
  if (opts && opts->struct_size < sizeof(tts_voice_audio_opts))
    return fail(ctx, TTS_ERR_ARG, "%s: struct_size %u, version 8 declares %zu bytes (set it to sizeof(tts_voice_audio_opts))", fn, opts->struct_size, sizeof(tts_voice_audio_opts));
  tts_voice_audio_opts full{};
  full.struct_size = sizeof(tts_voice_audio_opts);
  if (opts) full = *opts;
  full.full_clips = 1; full.crop_offset = 0;
  AfePlan pl;
  int rc = afe_plan(ctx, fn, n_samples, sample_rate, n_clips, &full, true, false, pl);
  if (rc) return rc;
  float *d80 = nullptr;
  if ((rc = dvae_begin(ctx, fn, pl.frames80.data(), n_clips, code_stride, &d80))) return rc; // every check of the DVAE side before any device work
  if ((rc = afe_init(ctx))) return rc;
  if ((rc = afe_front(ctx, fn, audio, pl, &full, d80, nullptr))) return rc;
  return dvae_run(ctx, codes_out, n_codes_out, code_stride, z_out);
}

int afe_audio_mel(tts_ctx *ctx, const float *audio, int64_t n, int sample_rate, int bands, const tts_voice_audio_opts *opts, float *mel_out, int64_t cap) {
  const char *fn = "tts_audio_mel";
  if (!audio || (bands != 80 && bands != 100)) return fail(ctx, TTS_ERR_ARG, "%s: bad arguments (bands: 80 or 100)", fn);
  AfePlan pl;
  const int32_t rate = sample_rate;
  int rc = afe_plan(ctx, fn, &n, &rate, 1, opts, bands == 80, bands == 100, pl);
  if (rc) return rc;
  const int frames = bands == 80 ? pl.frames80[0] : pl.frames100[0];
  if (!mel_out) return frames;
  if (cap < (int64_t)bands * frames) return fail(ctx, TTS_ERR_ARG, "%s: mel_out holds %lld floats, %lld needed", fn, (long long)cap, (long long)bands * frames);
  if ((rc = afe_init(ctx))) return rc;
  AfeState *st = ctx->afe;
  TTS_HIP(ctx, st->mel.reserve((size_t)bands * frames * 4));
  float *d = st->mel.as<float>();
  if ((rc = afe_front(ctx, fn, audio, pl, opts, bands == 80 ? d : nullptr, bands == 100 ? d : nullptr))) return rc;
  TTS_HIP(ctx, hipMemcpyAsync(mel_out, d, (size_t)bands * frames * 4, hipMemcpyDeviceToHost, ctx->stream));
  TTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return frames;
}
// The classifier's input stage (classifier.h): every clip through afe_resample_kernel with the tap table of its rate -> 24 000 Hz, ONE stage as upstream's
// load_audio (the voice calls above go through 22 050 Hz, as upstream's conditioning path does). Only the first out_len samples of a clip are computed. The
// tables are the front end's (one per reduced rate pair, made at first use); the clip records have a buffer of their own. Launches only: the caller synchronises.
static int afe_resample_clips(tts_ctx *ctx, const float *d_src, float *d_dst, const ClsResampleClip *clips, int n_clips, int to_rate, const char *who,
                              std::vector<AfeResClip> AfeState::*meta_h, DevBuf AfeState::*meta_d) {
  if (!ctx->afe) ctx->afe = new AfeState();
  AfeState *st = ctx->afe;
  std::vector<AfeResClip> &h = st->*meta_h;
  DevBuf &meta = st->*meta_d;
  h.resize(n_clips);
  std::vector<AfeTable *> tabs(n_clips, nullptr);
  for (int s = 0; s < n_clips; s++) {
    const int rc = afe_table(ctx, st, clips[s].rate, to_rate, &tabs[s]);
    if (rc) return fail(ctx, rc, "%s: no tap table for %d Hz -> %d Hz", who, clips[s].rate, to_rate);
    h[s] = AfeResClip{clips[s].in_off, clips[s].in_len, clips[s].out_off, clips[s].out_len};
  }
  TTS_HIP(ctx, meta.reserve(h.size() * sizeof(AfeResClip)));
  TTS_HIP(ctx, hipMemcpyAsync(meta.p, h.data(), h.size() * sizeof(AfeResClip), hipMemcpyHostToDevice, ctx->stream));
  for (int s = 0; s < n_clips; s++) {
    const AfeResampleGeom &g = tabs[s]->g;
    ProfScope ps(ctx, "afe_resample", 2.0 * clips[s].out_len * g.taps);
    afe_resample_kernel<<<dim3((unsigned)((clips[s].out_len + 255) / 256), 1), 256, 0, ctx->stream>>>(d_src, tabs[s]->tab.as<float>(), meta.as<AfeResClip>() + s,
                                                                                                    g.o, g.n, g.width, g.taps, d_dst);
  }
  return TTS_OK;
}
int afe_resample_to_24k(tts_ctx *ctx, const float *d_src, float *d_dst, const ClsResampleClip *clips, int n_clips) {
  return afe_resample_clips(ctx, d_src, d_dst, clips, n_clips, 24000, "tts_classify_audio", &AfeState::cls_meta_h, &AfeState::cls_meta);
}
// The aligner's input stage (aligner.h): the same kernel and tables, to 16 000 Hz, one stage; clip records of its own.
int afe_resample_to_16k(tts_ctx *ctx, const float *d_src, float *d_dst, const ClsResampleClip *clips, int n_clips) {
  return afe_resample_clips(ctx, d_src, d_dst, clips, n_clips, 16000, "tts_aligner_ids", &AfeState::w2v_meta_h, &AfeState::w2v_meta);
}
#endif // TTS_AFE_KERNELS_ONLY

} // namespace tts
