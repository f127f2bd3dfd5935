// C ABI of libtortoise_mi355x.so (see include/tortoise_mi355x.h for the reference call sites).
#include "common.h"
#include <sched.h>
#include <cctype>
#include <cstddef>
#include <cmath>
#include <algorithm>
#include <chrono>
#include <fstream>
#include <new>

using namespace tts;

hipEvent_t tts::prof_event(tts_ctx *c) {
  if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

// No exception crosses the C ABI: allocation failures and anything unexpected become a status + tts_last_error text.
template <class F>
static int guarded(tts_ctx *c, F body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return fail(c, TTS_ERR_LIMIT, "out of host memory");
  } catch (const std::exception &e) {
    return fail(c, TTS_ERR_STATE, "internal error: %s", e.what());
  } catch (...) {
    return fail(c, TTS_ERR_STATE, "internal error");
  }
}

extern "C" {

tts_ctx *tts_create(int device) {
  if (device == -1) { // host-only context: tokenizer / RNG / sampler; every device stage fails loudly
    tts_ctx *c = new tts_ctx();
    c->device = -1;
    c->seed_value = (uint32_t)std::chrono::duration_cast<std::chrono::milliseconds>(
                        std::chrono::system_clock::now().time_since_epoch()).count();
    c->generator.seed(c->seed_value);
    return c;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return nullptr; // no CPU fallback
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  tts_ctx *c = new tts_ctx();
  c->device = device;
  if (hipStreamCreate(&c->stream) != hipSuccess || hipStreamCreateWithFlags(&c->load_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
      hipEventCreate(&c->ev1) != hipSuccess) {
    delete c;
    return nullptr;
  }
  // the reference seeds with wall-clock ms unless --seed is given (main.cpp:39-47)
  c->seed_value = (uint32_t)std::chrono::duration_cast<std::chrono::milliseconds>(
                      std::chrono::system_clock::now().time_since_epoch()).count();
  c->generator.seed(c->seed_value);
  return c;
}

// NUMA node of the context's GPU and that node's CPU list (sysfs); -1 / "" when unknown
static int device_numa(const tts_ctx *c, std::string &cpulist) {
  cpulist.clear();
  if (!c || c->device < 0) return -1;
  char bus[64] = {};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, c->device) != hipSuccess) return -1;
  for (char *p = bus; *p; p++) *p = (char)tolower(*p);
  FILE *f = fopen((std::string("/sys/bus/pci/devices/") + bus + "/numa_node").c_str(), "r");
  int node = -1;
  if (f) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
  if (node < 0) return -1;
  f = fopen(("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist").c_str(), "r");
  if (f) {
    char buf[1024] = {};
    if (fgets(buf, sizeof buf, f)) { cpulist = buf; while (!cpulist.empty() && isspace((unsigned char)cpulist.back())) cpulist.pop_back(); }
    fclose(f);
  }
  return node;
}
int tts_device_numa_node(const tts_ctx *c, char *out, int cap) {
  std::string cl;
  const int node = device_numa(c, cl);
  if (out && cap > 0) snprintf(out, (size_t)cap, "%s", cl.c_str());
  return node;
}
int tts_pin_to_device_numa_node(tts_ctx *c) {
  std::string cl;
  if (device_numa(c, cl) < 0 || cl.empty()) return 0;
  cpu_set_t set;
  CPU_ZERO(&set);
  int n = 0;
  for (size_t i = 0; i < cl.size();) { // "a-b,c,d-e"
    char *end = nullptr;
    const long a = strtol(cl.c_str() + i, &end, 10);
    long b = a;
    if (*end == '-') b = strtol(end + 1, &end, 10);
    for (long k = a; k <= b && k < CPU_SETSIZE; k++) { CPU_SET((int)k, &set); n++; }
    i = (size_t)(end - cl.c_str());
    if (i < cl.size() && cl[i] == ',') i++;
    else if (i < cl.size() && !isdigit((unsigned char)cl[i])) break;
  }
  if (n == 0 || sched_setaffinity(0, sizeof set, &set) != 0) return 0;
  if (c->sampler_pool) { sampler_pool_free(c->sampler_pool); c->sampler_pool = nullptr; } // its threads are re-created (inside the mask) at the next use
  return n;
}

void tts_destroy(tts_ctx *c) {
  if (!c) return;
  if (c->sampler_pool) sampler_pool_free(c->sampler_pool);
  if (c->device < 0) { delete c->tok; delete c; return; }
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->session) ar_drv_close(c);
  diff_session_close(c);
  if (c->ar) ar_free(c->ar);
  if (c->diff) diff_free(c->diff);
  if (c->voc) voc_free(c->voc);
  if (c->clvp) clvp_free(c->clvp);
  if (c->cvvp) cvvp_free(c->cvvp);
  if (c->venc) voice_enc_free(c->venc);
  if (c->dcond) diff_cond_enc_free(c->dcond);
  if (c->hifigan) hifigan_free(c->hifigan);
  if (c->bigvgan) bigvgan_free(c->bigvgan);
  if (c->classifier) classifier_free(c->classifier);
  if (c->aligner) aligner_free(c->aligner);
  if (c->dvae) dvae_free(c->dvae);
  if (c->rlg) random_voice_free(c->rlg);
  if (c->afe) afe_free(c->afe);
  if (c->fp16_counts) (void)hipFree(c->fp16_counts);
  delete c->tok;
  for (auto &kv : c->prof)
    for (auto &pr : kv.second.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->load_stream) (void)hipStreamDestroy(c->load_stream);
  delete c;
}

int tts_version(void) { return TTS_API_VERSION; }

const char *tts_last_error(const tts_ctx *c) { return c ? c->err.c_str() : "no context (no HIP device?)"; }

// The autoregressive sampler's six controls: the ONE statement of what each accepts, for tts_set_option and for a request descriptor (tts_ar_session_admit_ex,
// tts_host_ar_request_check). Returns the refusal's text, or null for a value that is fine.
static const char *const kArControlKeys[6] = {"ar_temperature", "ar_top_k", "ar_top_p", "ar_repetition_penalty", "ar_penalty_scope", "ar_typical_mass"};
static int ar_control_index(const std::string &k) {
  for (int i = 0; i < 6; i++)
    if (k == kArControlKeys[i]) return i;
  return -1;
}
static const char *ar_control_error(int which, double value) {
  static_assert(TTS_VOCAB_MEL == 8194, "the text below names the vocabulary size");
  switch (which) {
  case 0: return (!std::isfinite(value) || !(value > 0) || !std::isfinite((float)value) || !((float)value > 0)) ? "ar_temperature: a finite value > 0" : nullptr;
  case 1: return (!(value >= 1 && value <= TTS_VOCAB_MEL) || value != std::floor(value)) ? "ar_top_k: an integer in 1 .. 8194" : nullptr;
  case 2: return (!(value > 0 && value <= 1) || !((float)value > 0)) ? "ar_top_p: a value in (0, 1]" : nullptr;
  case 3: return (!std::isfinite(value) || !(value >= 1) || !std::isfinite((float)value)) ? "ar_repetition_penalty: a finite value >= 1" : nullptr;
  case 4: return (value != 0 && value != 1) ? "ar_penalty_scope: 0 (the ids of the last input) or 1 (every id fed since tts_ar_begin)" : nullptr;
  case 5: return (value != 0 && (!(value > 0 && value < 1) || !((float)value > 0 && (float)value < 1))) ? "ar_typical_mass: 0 (off) or a value in (0, 1)" : nullptr;
  }
  return "unknown sampler control";
}
static void ar_control_store(int which, double value, SamplerParams &sp, int &scope) { // a value ar_control_error has passed
  switch (which) {
  case 0: sp.temp = (float)value; break;
  case 1: sp.top_k = (int)value; break;
  case 2: sp.top_p = (float)value; break;
  case 3: sp.penalty = (float)value; break;
  case 4: scope = (int)value; break;
  case 5: sp.typ_mass = (float)value; break;
  }
}

int tts_set_option(tts_ctx *c, const char *key, double value) {
  if (!c || !key) return TTS_ERR_ARG;
  std::string k(key);
  if (k == "gn_eps") c->gn_eps = (float)value;
  else if (k == "ggml_lut") c->ggml_lut = value != 0;
  else if (k.rfind("prof_only:", 0) == 0) { // value 1: add the family to the list of profiled families; 0: back to "all"
    if (value != 0) c->prof_filter.push_back(k.substr(10));
    else c->prof_filter.clear();
  }
  else if (k == "device_topk") c->device_topk = value != 0; // 1 default: see tts_ar_step_sample
  else if (k == "sampler_threads") { // worker threads for the per-candidate sampler scans (0 = run them on the caller)
    if (c->sampler_pool) { sampler_pool_free(c->sampler_pool); c->sampler_pool = nullptr; }
    c->sampler_threads = value < 0 ? -1 : (int)value;
  }
  else if (k == "share_uncond") c->share_uncond = value != 0;
  else if (k == "prof_stride") c->prof_stride = value < 1 ? 1 : (int)value;
  else if (k == "diff_graph") c->diff_graph = value != 0;
  else if (k == "dec_f32_mfma") c->dec_f32_mfma = value != 0;
  else if (k == "attn_f32") c->attn_f32 = value != 0;
  else if (k == "attn_proj_f16") c->attn_proj_f16 = value != 0;
  else if (k == "proj_dual_b") c->proj_dual_b = value != 0;
  else if (k == "gemm_wreg") c->gemm_wreg = value == 1 ? tts_ctx::GEMM_WREG_ALL : value == 2 ? 1 : value == 3 ? 2 : value == 4 ? 4 : 0; // 0 the LDS-staged kernels, 1 every class that has a register-streamed kernel, 2 / 3 / 4 in_layers / QKV / k = 3 out_layers only (A/B)
  else if (k == "gemm_gn_fuse") c->gemm_gn_fuse = value != 0;
  else if (k == "lc_attn_f32") c->lc_attn_f32 = value != 0;
  else if (k == "latency_mode") c->latency_mode = value != 0;
  else if (k == "fp16_check") c->fp16_check = value != 0;
  else if (k == "rng_fast_normal") c->rng_fast_normal = value != 0;
  else if (k == "noise_pipeline") c->noise_pipeline = value != 0;
  else if (k == "load_device_pack") c->load_device_pack = value != 0;
  else if (k == "load_threads") c->load_threads = value < 0 ? 0 : value > 64 ? 64 : (int)value;
  else if (k == "attn_q64") c->attn_q64 = value < 0 ? 0 : value > 2 ? 2 : (int)value; // 0 never, 1 always, 2 auto (grids of at most one 128-query workgroup per CU)
  else if (k == "hoist_integrator") c->hoist_integrator = value < 0 ? 0 : (int)value; // 0 off, 1 on for small layouts, n > 1: on for layouts of at most n packed rows (A/B)
  else if (k == "attn_f32_drop") c->attn_f32_drop = (int)value & 7;
  else if (k == "ar_weights") {
    if (value != 0 && value != 1 && value != 2) return fail(c, TTS_ERR_ARG, "ar_weights: 0 (f32), 1 (fp16) or 2 (fp8 e4m3)");
    c->ar_weights = (int)value;
  }
  else if (k == "diff_sampler") { // additions within version 8: the sampler of tts_diffusion / tts_diffusion_multi_voice (diff_control_error: the one statement of
                                  // what the three accept, shared with a diffusion session's request descriptor)
    if (const char *e = diff_control_error(0, value)) return fail(c, TTS_ERR_ARG, "%s", e);
    c->diff_sampler = (int)value;
  }
  else if (k == "ddim_eta") {
    if (const char *e = diff_control_error(1, value)) return fail(c, TTS_ERR_ARG, "%s", e);
    c->ddim_eta = value;
  }
  else if (k == "cond_free_k") {
    if (const char *e = diff_control_error(2, value)) return fail(c, TTS_ERR_ARG, "%s", e);
    c->cond_free_k = (float)value;
  }
  else if (k == "diff_temperature") {
    if (const char *e = diff_control_error(3, value)) return fail(c, TTS_ERR_ARG, "%s", e);
    c->diff_temperature = value;
  }
  else if (k == "cond_free") {
    if (const char *e = diff_control_error(4, value)) return fail(c, TTS_ERR_ARG, "%s", e);
    c->cond_free = (int)value;
  }
  // additions within version 8: the autoregressive sampler's controls (read by tts_sample, tts_ar_step_sample and the tts_autoregressive* drivers)
  // (and, per request, by tts_ar_session_admit_ex: ar_control_error is the one statement of what each of them accepts)
  else if (ar_control_index(k) >= 0) {
    const int which = ar_control_index(k);
    if (const char *e = ar_control_error(which, value)) return fail(c, TTS_ERR_ARG, "%s", e);
    ar_control_store(which, value, c->ar_sp, c->ar_penalty_scope);
  }
  else if (k == "hfg_small_m") { // addition within version 8: tile selection of tts_hifigan_chunk, same bits either way
    if (!(value >= 0 && value <= (1 << 24)) || value != std::floor(value)) return fail(c, TTS_ERR_ARG, "hfg_small_m: a row count in 0 .. 2^24 (0 = never)");
    c->hfg_small_m = (int)value;
  }
  else if (k == "prof_eager_every") c->prof_eager_every = value < 1 ? 1 : (int)value;
  else if (k == "stream_cus") {
    // Partition of the chip between two contexts of one process (INTEGRATION.md "two-context pipeline"): value n > 0 re-creates this
    // context's stream on the n lowest CUs of every XCD, n < 0 on all BUT those, 0 on the whole chip again. The AR stage is a chain of
    // 151 short dependent kernels per decode step that uses a fraction of the chip and cannot be interleaved with another stream's
    // 1000-workgroup kernels (measured: its kernels then wait for the running GEMM to drain, 228 ms -> 1-1.9 s; stream priority
    // changes nothing); on its own CUs it runs undisturbed while the other context's diffusion stage has the rest.
    // hipExtStreamCreateWithCUMask on gfx950: bit i = XCD i % 8, CU slot i / 8 (tools/cu_mask_probe.hip); an XCD with no bit set is
    // unrestricted, so every XCD keeps at least one CU. Only before any model is loaded / graph captured on the old stream.
    if (c->device < 0) return fail(c, TTS_ERR_HIP, "host-only context: no stream");
    if (c->ar || c->diff || c->voc || c->clvp || c->cvvp || c->venc || c->dcond || c->hifigan) return fail(c, TTS_ERR_STATE, "stream_cus must be set before the models are loaded");
    (void)hipSetDevice(c->device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return fail(c, TTS_ERR_HIP, "hipGetDeviceProperties failed");
    const int xcds = 8, per_xcd = prop.multiProcessorCount / xcds, n = (int)(value < 0 ? -value : value);
    if (prop.multiProcessorCount % xcds || per_xcd > 32 || n >= per_xcd) return fail(c, TTS_ERR_ARG, "stream_cus %d: the device has %d CUs per XCD", (int)value, per_xcd);
    hipStream_t s = nullptr;
    if (n == 0) {
      if (hipStreamCreate(&s) != hipSuccess) return fail(c, TTS_ERR_HIP, "hipStreamCreate failed");
    } else {
      uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int slot = 0; slot < per_xcd; slot++)
        if ((slot < n) == (value > 0))
          for (int x = 0; x < xcds; x++) { const int bit = slot * xcds + x; mask[bit >> 5] |= 1u << (bit & 31); }
      if (hipExtStreamCreateWithCUMask(&s, (uint32_t)((per_xcd * xcds + 31) / 32), mask) != hipSuccess)
        return fail(c, TTS_ERR_HIP, "hipExtStreamCreateWithCUMask failed");
    }
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
    c->stream = s;
    c->stream_cus = (int)value;
  }
  else if (k == "rng_shard_offset") { if (value < 0) return fail(c, TTS_ERR_ARG, "rng_shard_offset < 0"); c->rng_shard_offset = (int)value; }
  else if (k == "rng_shard_total") { if (value < 0) return fail(c, TTS_ERR_ARG, "rng_shard_total < 0"); c->rng_shard_total = (int)value; }
  else return fail(c, TTS_ERR_ARG, "unknown option '%s'", key);
  return TTS_OK;
}

#define NEED_CTX(c)                                                                              \
  do {                                                                                         \
    if (!(c)) return TTS_ERR_ARG;                                                              \
    if ((c)->device < 0) return fail((c), TTS_ERR_HIP, "host-only context: no HIP device, no CPU fallback"); \
    (void)hipSetDevice((c)->device);                                                           \
  } while (0)

// While a session is open (tts_ar_session_open) the AR state is the session's: the single-call entry points refuse.
#define NO_SESSION(c, name)                                                                                          \
  do {                                                                                                               \
    if ((c)->session) return fail((c), TTS_ERR_STATE, "%s: a session is open (tts_ar_session_close first)", name); \
  } while (0)

int tts_load_ar(tts_ctx *c, const char *path) { NEED_CTX(c); NO_SESSION(c, "tts_load_ar"); return guarded(c, [&] { return ar_load(c, path); }); }
// While a diffusion session is open (tts_diff_session_open) its admissions own the diffusion run state: the single-call entry points refuse.
#define NO_DIFF_SESSION(c, name)                                                                                                \
  do {                                                                                                                        \
    if ((c)->diff_session) return fail((c), TTS_ERR_STATE, "%s: a diffusion session is open (tts_diff_session_close first)", name); \
  } while (0)
int tts_load_diffusion(tts_ctx *c, const char *path) { NEED_CTX(c); NO_DIFF_SESSION(c, "tts_load_diffusion"); return guarded(c, [&] { return diff_load(c, path); }); }
int tts_load_vocoder(tts_ctx *c, const char *path) { NEED_CTX(c); return guarded(c, [&] { return voc_load(c, path); }); }
int tts_load_diffusion_conditioning_encoder(tts_ctx *c, const char *path) { NEED_CTX(c); return guarded(c, [&] { return diff_cond_enc_load(c, path); }); }
int tts_diffusion_conditioning_latent(tts_ctx *c, const float *mel, const int32_t *frames, int n_clips, float *out2048) {
  NEED_CTX(c);
  return guarded(c, [&] { return diff_cond_enc_latent(c, mel, frames, n_clips, out2048); });
}
int tts_set_diffusion_conditioning_latent(tts_ctx *c, const float *latent2048) { NEED_CTX(c); return guarded(c, [&] { return diff_set_cond_latent(c, latent2048); }); }
int tts_load_voice_encoder(tts_ctx *c, const char *path) { NEED_CTX(c); return guarded(c, [&] { return voice_enc_load(c, path); }); }
int tts_voice_latent(tts_ctx *c, const float *mel, const int32_t *frames, int n_clips, float *out1024) {
  NEED_CTX(c);
  return guarded(c, [&] { return voice_enc_latent(c, mel, frames, n_clips, out1024); });
}
int tts_voice_audio_opts_init(tts_voice_audio_opts *o) {
  if (!o || o->struct_size < sizeof(tts_voice_audio_opts)) return TTS_ERR_ARG;
  o->mel_norms80 = nullptr; o->crop_offset = 0; o->full_clips = 0;
  return TTS_OK;
}
// Legal while a session is open: the front-end and the two encoders own their buffers and touch no AR or diffusion state.
int tts_voice_from_audio(tts_ctx *c, const float *audio, const int64_t *n_samples, const int32_t *sample_rate, int n_clips, const tts_voice_audio_opts *opts,
                         float *out1024, float *out2048) {
  NEED_CTX(c);
  return guarded(c, [&] { return afe_voice_from_audio(c, audio, n_samples, sample_rate, n_clips, opts, out1024, out2048); });
}
int tts_audio_mel(tts_ctx *c, const float *audio, int64_t n, int sample_rate, int bands, const tts_voice_audio_opts *opts, float *mel_out, int64_t cap) {
  NEED_CTX(c);
  return guarded(c, [&] { return afe_audio_mel(c, audio, n, sample_rate, bands, opts, mel_out, cap); });
}
int tts_load_clvp(tts_ctx *c, const char *path) { NEED_CTX(c); return guarded(c, [&] { return clvp_load(c, path); }); }
int tts_clvp_score(tts_ctx *c, const int32_t *text_ids, int n_text, const int32_t *codes, const int32_t *code_len, int n_candidates,
                   int code_stride, float *scores_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return clvp_score(c, text_ids, n_text, codes, code_len, n_candidates, code_stride, scores_out); });
}
// CVVP: the second re-ranker (cvvp.hip). Legal while a session is open, as tts_voice_from_audio is: it owns its buffers and touches no AR or diffusion state.
int tts_load_cvvp(tts_ctx *c, const char *path) { NEED_CTX(c); return guarded(c, [&] { return cvvp_load(c, path); }); }
int tts_cvvp_latent_dim(const tts_ctx *c) { return c ? cvvp_latent_dim(c) : TTS_ERR_ARG; }
int tts_cvvp_rows(int mel_frames) { // the two strided convolutions of the stem: k 5 / stride 2 / padding 2, then k 3 / stride 2 / padding 1
  if (mel_frames < 1) return TTS_ERR_ARG;
  const int t1 = (mel_frames - 1) / 2 + 1;
  return (t1 - 1) / 2 + 1;
}
int tts_cvvp_voice(tts_ctx *c, const float *mel80, const int32_t *frames, int n_clips, float *latents_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return cvvp_voice(c, mel80, frames, n_clips, latents_out); });
}
int tts_cvvp_voice_audio(tts_ctx *c, const float *audio, const int64_t *n_samples, const int32_t *sample_rate, int n_clips, const tts_voice_audio_opts *opts,
                         float *latents_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return afe_cvvp_voice_audio(c, audio, n_samples, sample_rate, n_clips, opts, latents_out); });
}
int tts_cvvp_score(tts_ctx *c, const float *voice_latents, int n_clips, const int32_t *codes, const int32_t *code_len, int n_candidates, int code_stride,
                   float *scores_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return cvvp_score(c, voice_latents, n_clips, codes, code_len, n_candidates, code_stride, scores_out); });
}
int tts_load_hifigan(tts_ctx *c, const char *path) { NEED_CTX(c); return guarded(c, [&] { return hifigan_load(c, path); }); }
int tts_hifigan_samples(int latent_rows) { return 256 * tts_diffusion_frames(latent_rows); }
int tts_hifigan_decode(tts_ctx *c, const float *latents, const int32_t *rows, int n_candidates, const float *voices, int n_voices,
                       const int32_t *voice_of_candidate, float *audio_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return hifigan_decode(c, latents, rows, n_candidates, voices, n_voices, voice_of_candidate, audio_out); });
}
int tts_hifigan_chunk(tts_ctx *c, const float *latents, const int32_t *rows, int n_candidates, const float *voices, int n_voices,
                      const int32_t *voice_of_candidate, const int32_t *frame0, const int32_t *n_frames, float *audio_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return hifigan_chunk(c, latents, rows, n_candidates, voices, n_voices, voice_of_candidate, frame0, n_frames, audio_out); });
}
int tts_hifigan_stream_recaptures(const tts_ctx *c) { return c ? c->stream_recaptures : -1; }
// BigVGAN: the second vocoder (bigvgan.h). Legal while a session is open: it owns its buffers and touches no AR or diffusion state.
int tts_load_bigvgan(tts_ctx *c, const char *path) { NEED_CTX(c); return guarded(c, [&] { return bigvgan_load(c, path); }); }
int tts_bigvgan_samples(int mel_frames) { return 256 * mel_frames; }
int tts_bigvgan(tts_ctx *c, const float *mel, const int32_t *frames, int n_candidates, float *audio_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return bigvgan_run(c, mel, frames, n_candidates, audio_out); });
}
int tts_bigvgan_config(tts_ctx *c, int32_t *out8) { NEED_CTX(c); return bigvgan_config(c, out8); }
// tortoise-detect (classifier.h). The loader parses the file before it asks for the device, so a host-only context still tells a broken file (TTS_ERR_FORMAT) from a
// good one (TTS_ERR_HIP). tts_classify_audio is legal while a session is open: it owns its buffers and touches no AR or diffusion state.
int tts_load_classifier(tts_ctx *c, const char *path) {
  if (!c) return TTS_ERR_ARG;
  return guarded(c, [&] { return classifier_load(c, path); });
}
int tts_classifier_positions(int n_samples_24k) { // upstream's configuration: five downsamples by 4 of the cropped clip
  if (n_samples_24k < 1) return TTS_ERR_ARG;
  int n = n_samples_24k < TTS_CLS_MAX_SAMPLES ? n_samples_24k : TTS_CLS_MAX_SAMPLES;
  for (int l = 0; l < 5; l++) n = (n - 1) / 4 + 1;
  return n;
}
int tts_classify_audio(tts_ctx *c, const float *audio, const int64_t *n_samples, const int32_t *sample_rate, int n_clips, float *prob_out, float *logits_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return classifier_run(c, audio, n_samples, sample_rate, n_clips, prob_out, logits_out, afe_resample_to_24k); });
}
// The wav2vec2 CTC aligner (aligner.h) and what rests on it: tts_align_audio and tts_redact_audio are tts_aligner_ids of one clip followed by the host rules of
// host_logic.cpp (ctc_align, redact_spans). Every argument is checked, and the text parsed, before any device work; an output is written only on success.
int tts_load_aligner(tts_ctx *c, const char *path) {
  if (!c) return TTS_ERR_ARG;
  return guarded(c, [&] { return aligner_load(c, path); });
}
int tts_aligner_frames(int n_samples_16k) { // upstream's configuration: k = 10, 3, 3, 3, 3, 2, 2 and s = 5, 2, 2, 2, 2, 2, 2, no padding
  static const int k[7] = {10, 3, 3, 3, 3, 2, 2}, s[7] = {5, 2, 2, 2, 2, 2, 2};
  if (n_samples_16k < 1) return TTS_ERR_ARG;
  int n = n_samples_16k;
  for (int i = 0; i < 7; i++) {
    if (n < k[i]) return TTS_ERR_ARG;
    n = (n - k[i]) / s[i] + 1;
  }
  return n;
}
int tts_aligner_clip_frames(tts_ctx *c, int64_t n_samples, int sample_rate) { NEED_CTX(c); return aligner_clip_frames(c, n_samples, sample_rate); }
int tts_aligner_vocab(tts_ctx *c, int32_t *vocab_out, int cap, int32_t *blank_out) { NEED_CTX(c); return aligner_vocab(c, vocab_out, cap, blank_out); }
int tts_aligner_ids(tts_ctx *c, const float *audio, const int64_t *n_samples, const int32_t *sample_rate, int n_clips, int32_t *ids_out, int32_t *n_frames_out,
                    int frame_stride, float *logits_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return aligner_run(c, audio, n_samples, sample_rate, n_clips, ids_out, n_frames_out, frame_stride, logits_out, afe_resample_to_16k); });
}
// offsets of the characters of `text` (code points, brackets not interpreted) in the caller's clip
static int align_clip(tts_ctx *c, const char *fn, const float *audio, int64_t n, int rate, const std::vector<int32_t> &text, std::vector<int64_t> &al) {
  const int frames = aligner_clip_frames(c, n, rate);
  if (frames < 0) return frames;
  std::vector<int32_t> ids((size_t)frames), vocab;
  int32_t got = 0, blank = 0, rate32 = rate;
  int rc = aligner_run(c, audio, &n, &rate32, 1, ids.data(), &got, frames, nullptr, afe_resample_to_16k);
  if (rc) return rc;
  vocab.resize((size_t)aligner_vocab(c, nullptr, 0, &blank));
  aligner_vocab(c, vocab.data(), (int)vocab.size(), nullptr);
  std::string err;
  rc = ctc_align(ids.data(), got, vocab.data(), (int)vocab.size(), blank, text, n, al, err);
  return rc < 0 ? fail(c, rc, "%s: %s", fn, err.c_str()) : rc;
}
int tts_align_audio(tts_ctx *c, const float *audio, int64_t n_samples, int sample_rate, const char *text, int64_t *offsets_out, int cap) {
  NEED_CTX(c);
  return guarded(c, [&]() -> int {
    if (!c->aligner) return fail(c, TTS_ERR_STATE, "tts_load_aligner not called");
    std::vector<int32_t> t;
    if (!audio || !text || !offsets_out || cap < 0) return fail(c, TTS_ERR_ARG, "tts_align_audio: bad argument");
    if (utf8_decode(text, t) < 0) return fail(c, TTS_ERR_ARG, "tts_align_audio: the text is not UTF-8");
    if ((int64_t)t.size() > cap) return fail(c, TTS_ERR_ARG, "tts_align_audio: room for %d of %d offsets", cap, (int)t.size());
    std::vector<int64_t> al;
    const int rc = align_clip(c, "tts_align_audio", audio, n_samples, sample_rate, t, al);
    if (rc < 0) return rc;
    for (size_t i = 0; i < al.size(); i++) offsets_out[i] = al[i];
    return rc;
  });
}
int64_t tts_redact_audio(tts_ctx *c, const float *audio, int64_t n_samples, int sample_rate, const char *text, float *out, int64_t cap) {
  NEED_CTX(c);
  return guarded(c, [&]() -> int {
    const char *fn = "tts_redact_audio";
    if (!c->aligner) return fail(c, TTS_ERR_STATE, "tts_load_aligner not called");
    if (!audio || !text || !out || n_samples < 1) return fail(c, TTS_ERR_ARG, "%s: bad argument", fn);
    if (n_samples > (1 << 26)) return fail(c, TTS_ERR_LIMIT, "%s: %lld samples, at most 2^26", fn, (long long)n_samples);
    std::vector<int32_t> t, clean, iv;
    std::string err;
    if (utf8_decode(text, t) < 0) return fail(c, TTS_ERR_ARG, "%s: the text is not UTF-8", fn);
    const int n_iv = redact_spans(t, clean, iv, err);
    if (n_iv < 0) return fail(c, n_iv, "%s: %s", fn, err.c_str());
    if (clean.size() == t.size()) { // no bracket: the clip unchanged, as upstream returns it before the model runs
      if (cap < n_samples) return fail(c, TTS_ERR_ARG, "%s: room for %lld of %lld samples", fn, (long long)cap, (long long)n_samples);
      for (int64_t i = 0; i < n_samples; i++)
        if (!std::isfinite(audio[i])) return fail(c, TTS_ERR_ARG, "%s: the audio holds a non-finite sample (element %lld)", fn, (long long)i);
      memmove(out, audio, (size_t)n_samples * 4);
      return (int)n_samples;
    }
    if (clean.empty()) return 0; // every character is bracketed: nothing is kept
    std::vector<int64_t> al;
    const int rc = align_clip(c, fn, audio, n_samples, sample_rate, clean, al);
    if (rc < 0) return rc;
    int64_t total = 0;
    for (int i = 0; i < n_iv; i++) total += std::max<int64_t>(0, al[iv[2 * i + 1]] - al[iv[2 * i]]);
    if (total > cap) return fail(c, TTS_ERR_ARG, "%s: room for %lld of %lld samples", fn, (long long)cap, (long long)total);
    int64_t at = 0;
    for (int i = 0; i < n_iv; i++) { // clip[align[first] : align[last]]: the last character's own duration is cut, as upstream cuts it
      const int64_t a = al[iv[2 * i]], b = al[iv[2 * i + 1]];
      if (b > a) { memmove(out + at, audio + a, (size_t)(b - a) * 4); at += b - a; }
    }
    return (int)total;
  });
}
// Random voices (random_voice.h). The loader parses its files before it asks for the device, as tts_load_classifier does. tts_random_voice is legal while a
// session is open, as tts_voice_from_audio is: it owns its buffers, touches no AR or diffusion state and never draws from the context's std::mt19937.
int tts_load_random_voice(tts_ctx *c, const char *auto_path, const char *diff_path) {
  if (!c) return TTS_ERR_ARG;
  return guarded(c, [&] { return random_voice_load(c, auto_path, diff_path); });
}
int tts_random_voice_dim(const tts_ctx *c, int side) { return random_voice_dim(c, side); }
int tts_random_voice(tts_ctx *c, const uint64_t *seeds, int n, const float *z_auto, const float *z_diff, float *out_auto, float *out_diff) {
  NEED_CTX(c);
  return guarded(c, [&] { return random_voice_run(c, seeds, n, z_auto, z_diff, out_auto, out_diff); });
}
int tts_random_voice_noise(tts_ctx *c, uint64_t seed, int side, float *out, int cap) {
  NEED_CTX(c);
  return guarded(c, [&] { return random_voice_noise(c, seed, side, out, cap); });
}
// The DVAE encoder (dvae.h): audio -> speech codes. The loader parses the file before it asks for the device, as tts_load_classifier does. The two code calls are
// legal while a session is open: the stage owns its buffers and touches no AR or diffusion state.
int tts_load_dvae(tts_ctx *c, const char *path) {
  if (!c) return TTS_ERR_ARG;
  return guarded(c, [&] { return dvae_load(c, path); });
}
int tts_dvae_rows(int mel_frames) { return tts_cvvp_rows(mel_frames); } // upstream's configuration: two convolutions k 3 / stride 2 / padding 1
int tts_dvae_tokens(const tts_ctx *c) { return dvae_tokens(c); }
int tts_dvae_dim(const tts_ctx *c) { return dvae_dim(c); }
int tts_dvae_codes(tts_ctx *c, const float *mel80, const int32_t *frames, int n_clips, int32_t *codes_out, int32_t *n_codes_out, int code_stride, float *z_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return dvae_codes(c, mel80, frames, n_clips, codes_out, n_codes_out, code_stride, z_out); });
}
int tts_dvae_codes_audio(tts_ctx *c, const float *audio, const int64_t *n_samples, const int32_t *sample_rate, int n_clips, const tts_voice_audio_opts *opts,
                         int32_t *codes_out, int32_t *n_codes_out, int code_stride, float *z_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return afe_dvae_codes_audio(c, audio, n_samples, sample_rate, n_clips, opts, codes_out, n_codes_out, code_stride, z_out); });
}
// tts_ar_begin (one candidate), tts_ar_prefill, tts_host_pad_codes, tts_ar_latents, tts_host_trimmed_rows as one call: the latents of GIVEN codes (a recording's,
// from tts_dvae_codes) under a text and a voice. No sampling: the context's generator is never touched.
int tts_ar_latents_for_codes(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice1024, const int32_t *codes, int n_codes, int32_t *rows_out,
                             float *latents_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_latents_for_codes");
  return guarded(c, [&]() -> int {
    const char *fn = "tts_ar_latents_for_codes";
    if (!text_ids || n_text < 1 || !voice1024 || !codes || n_codes < 1 || !rows_out || !latents_out) return fail(c, TTS_ERR_ARG, "%s: bad argument", fn);
    if (n_codes > 500) return fail(c, TTS_ERR_LIMIT, "%s: %d codes, at most 500 (chunk longer recordings)", fn, n_codes);
    for (int i = 0; i < n_codes; i++)
      if (codes[i] < 0 || codes[i] >= 8192) return fail(c, TTS_ERR_ARG, "%s: code %d at position %d (0 .. 8191: a speech code, not a start or stop token)", fn, codes[i], i);
    int rc = ar_begin(c, text_ids, n_text, voice1024, 1, 1);
    if (rc) return rc;
    std::vector<float> logits(TTS_VOCAB_MEL), lat((size_t)500 * 1024);
    if ((rc = ar_prefill(c, logits.data()))) return rc;
    std::vector<int> padded(codes, codes + n_codes);
    pad_codes(padded);
    if (padded.size() != 502) return fail(c, TTS_ERR_LIMIT, "%s: %d codes pad to %d, not 502", fn, n_codes, (int)padded.size());
    std::vector<int32_t> c502(padded.begin(), padded.end());
    if ((rc = ar_latents(c, c502.data(), 1, 502, lat.data()))) return rc;
    const int rows = trimmed_latent_rows(c502.data());
    if (rows < 0 || rows > 500) return fail(c, TTS_ERR_LIMIT, "%s: %d latent rows", fn, rows);
    memcpy(latents_out, lat.data(), (size_t)rows * 1024 * 4);
    *rows_out = rows;
    return TTS_OK;
  });
}
// Teacher-forced scores of GIVEN codes under a text and a voice: tts_ar_begin (one candidate) + the prompt pass + the latent pass over the row table of
// tts_host_ar_score_rows + the fused head (ar_score.h). Every check runs before any device work; no sampling: the context's generator is never touched.
int tts_ar_score_codes(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice1024, const int32_t *codes, const int32_t *n_codes, int n_cand,
                       int code_stride, int positions, float *logp_out, float *stop_logp_out, int32_t *greedy_out, float *lse_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_score_codes");
  return guarded(c, [&]() -> int {
    const char *fn = "tts_ar_score_codes";
    if (!c->ar) return fail(c, TTS_ERR_STATE, "%s: AR model not loaded", fn);
    if (!text_ids || n_text < 1 || !voice1024 || !codes || !n_codes || n_cand < 1 || code_stride < 1 || !logp_out) return fail(c, TTS_ERR_ARG, "%s: bad argument", fn);
    if (positions != TTS_SCORE_POS_DECODE && positions != TTS_SCORE_POS_TRAIN) return fail(c, TTS_ERR_ARG, "%s: positions %d (0 decode, 1 train)", fn, positions);
    if (n_cand > 64) return fail(c, TTS_ERR_LIMIT, "%s: %d candidates, at most 64", fn, n_cand);
    int n_max = 0;
    for (int b = 0; b < n_cand; b++) {
      if (n_codes[b] < 1 || n_codes[b] > code_stride) return fail(c, TTS_ERR_ARG, "%s: candidate %d has %d codes (1 .. code_stride %d)", fn, b, n_codes[b], code_stride);
      if (n_codes[b] > 500) return fail(c, TTS_ERR_LIMIT, "%s: candidate %d has %d codes, at most 500 (chunk longer recordings)", fn, b, n_codes[b]);
      for (int i = 0; i < n_codes[b]; i++) {
        const int v = codes[(size_t)b * code_stride + i];
        if (v < 0 || v >= 8192) return fail(c, TTS_ERR_ARG, "%s: candidate %d: code %d at position %d (0 .. 8191: a speech code, not a start or stop token)", fn, b, v, i);
      }
      n_max = std::max(n_max, n_codes[b]);
    }
    if (1 + n_text + n_max + 1 > 1024) return fail(c, TTS_ERR_LIMIT, "%s: %d text ids and %d codes exceed the 1024 positions", fn, n_text, n_max);
    // the uniform pass: n_max + 1 rows per candidate, shorter candidates continued with code 83 (causal: no scored row sees the padding)
    const int n_rows = n_max + 1;
    std::vector<int32_t> ids((size_t)n_cand * n_rows), pos(ids.size()), tgt(ids.size()), padded((size_t)n_max);
    for (int b = 0; b < n_cand; b++) {
      std::copy(codes + (size_t)b * code_stride, codes + (size_t)b * code_stride + n_codes[b], padded.begin());
      std::fill(padded.begin() + n_codes[b], padded.end(), 83);
      const size_t o = (size_t)b * n_rows;
      int rc = ar_score_row_table(padded.data(), n_max, positions, &ids[o], &pos[o], &tgt[o]);
      if (rc) return fail(c, rc, "%s: row table", fn);
      tgt[o + n_codes[b]] = 8193; // the candidate's own last row predicts the stop token
    }
    int rc = ar_begin(c, text_ids, n_text, voice1024, 1, 1);
    if (rc) return rc;
    if ((rc = ar_prefill(c, nullptr))) return rc;
    std::vector<float> out((size_t)4 * n_cand * n_rows);
    if ((rc = ar_score_rows(c, ids.data(), pos.data(), tgt.data(), n_cand, n_rows, out.data()))) return rc;
    const size_t R = (size_t)n_cand * n_rows, os = (size_t)code_stride + 1;
    for (int b = 0; b < n_cand; b++)
      for (int j = 0; j <= n_codes[b]; j++) {
        const size_t r = (size_t)b * n_rows + j;
        if (lse_out) lse_out[b * os + j] = out[r];
        logp_out[b * os + j] = out[R + r];
        if (stop_logp_out) stop_logp_out[b * os + j] = out[2 * R + r];
        if (greedy_out) memcpy(&greedy_out[b * os + j], &out[3 * R + r], 4);
      }
    return TTS_OK;
  });
}
int tts_host_stream_final_rows(const int32_t *codes, int k) { return (k < 0 || (k > 0 && !codes)) ? TTS_ERR_ARG : stream_final_rows(codes, k); }
int tts_ar_layers(const tts_ctx *c) { return c ? ar_layers(c) : 0; }
int tts_diffusion_layers(const tts_ctx *c) { return c ? diff_layers(c) : 0; }

void tts_seed(tts_ctx *c, uint32_t seed) {
  if (!c) return;
  c->seed_value = seed;
  c->generator.seed(seed);
  c->distribution.reset();
  c->normal_distribution.reset();
}
int tts_rng_load_state(tts_ctx *c, const char *path) {
  if (!c) return TTS_ERR_ARG;
  std::ifstream fin(path);
  if (!fin) return fail(c, TTS_ERR_IO, "cannot open '%s'", path);
  fin >> c->generator;
  c->distribution.reset();
  c->normal_distribution.reset();
  return fin ? TTS_OK : fail(c, TTS_ERR_FORMAT, "bad RNG state file '%s'", path);
}
int tts_rng_save_state(tts_ctx *c, const char *path) {
  if (!c || !path) return TTS_ERR_ARG;
  std::ofstream fout(path);
  if (!fout) return fail(c, TTS_ERR_IO, "cannot open '%s' for writing", path);
  fout << c->generator;
  return fout ? TTS_OK : fail(c, TTS_ERR_IO, "cannot write '%s'", path);
}
float tts_rng_uniform(tts_ctx *c) { return c ? c->distribution(c->generator) : 0.f; }
void tts_rng_normal(tts_ctx *c, float *out, int64_t n) { // sample_normal_noise, main.cpp:4695-4701
  if (!c || !out || n <= 0) return;
  rng_normal_fill(c, out, n);
}

int tts_tokenizer_load(tts_ctx *c, const char *path) {
  if (!c || !path) return TTS_ERR_ARG;
  return guarded(c, [&] {
    std::unique_ptr<Tokenizer> t(new Tokenizer());
    if (!t->load(path)) return fail(c, TTS_ERR_IO, "Failed to open %s (missing, truncated or malformed)", path);
    delete c->tok;
    c->tok = t.release();
    return (int)c->tok->vocab.size();
  });
}
int tts_tokenize(tts_ctx *c, const char *message, int32_t *out, int cap) {
  if (!c || !c->tok) return c ? fail(c, TTS_ERR_STATE, "tokenizer not loaded") : TTS_ERR_ARG;
  if (!message || !out || cap < 0) return fail(c, TTS_ERR_ARG, "tts_tokenize: bad argument");
  return guarded(c, [&] {
    std::vector<int> ids = c->tok->encode(message);
    for (int i = 0; i < (int)ids.size() && i < cap; i++) out[i] = ids[i];
    return (int)ids.size();
  });
}

int tts_ar_begin(tts_ctx *c, const int32_t *ids, int n, const float *voice, int B, int max_steps) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_begin");
  return guarded(c, [&] { return ar_begin(c, ids, n, voice, B, max_steps); });
}
int tts_ar_prefill(tts_ctx *c, float *logits) { NEED_CTX(c); NO_SESSION(c, "tts_ar_prefill"); return guarded(c, [&] { return ar_prefill(c, logits); }); }
int tts_ar_step(tts_ctx *c, const int32_t *prev, int i, float *logits) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_step");
  return guarded(c, [&] { return ar_step(c, prev, i, logits, 0); });
}
int tts_ar_step_sample(tts_ctx *c, const int32_t *prev, int i, unsigned flags, int32_t *samples_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_step_sample");
  if (!prev || !samples_out) return TTS_ERR_ARG;
  return guarded(c, [&] { return ar_drv_step_sample(c, prev, i, flags, samples_out); });
}
int tts_ar_topk_fallbacks(const tts_ctx *c) { return c ? c->topk_fallbacks : -1; }
int tts_diffusion_time_mlp_retries(const tts_ctx *c) { return c ? c->time_mlp_retries : -1; }
int tts_diffusion_fp16_check(tts_ctx *c, int64_t counts[2]) {
  if (!c || !counts) return TTS_ERR_ARG;
  return guarded(c, [&] { return tts::diff_fp16_check(c, counts); });
}
int tts_host_sample_row(const float *row, const int32_t *ids, int ids_per_cand, float uniform) {
  if (!row || !ids || ids_per_cand < 1) return -1;
  return sample_one_row(row, ids, ids_per_cand, uniform);
}
static bool sampler_params_ok(const float *row, const int32_t *ids, int n_ids, float temperature, int top_k, float top_p, float penalty) {
  if (!row || n_ids < 0 || (n_ids > 0 && !ids)) return false;
  for (int i = 0; i < n_ids; i++)
    if (ids[i] < 0 || ids[i] >= TTS_VOCAB_MEL) return false;
  return std::isfinite(temperature) && temperature > 0 && top_k >= 1 && top_k <= TTS_VOCAB_MEL && top_p > 0 && top_p <= 1 && std::isfinite(penalty) && penalty >= 1;
}
int tts_host_sample_row_ex(const float *row, const int32_t *ids, int n_ids, float uniform, float temperature, int top_k, float top_p, float penalty, int mode) {
  if (!sampler_params_ok(row, ids, n_ids, temperature, top_k, top_p, penalty) || (mode != 0 && mode != 1)) return -2;
  SamplerParams sp; sp.temp = temperature; sp.top_k = top_k; sp.top_p = top_p; sp.penalty = penalty;
  return sample_one_row_ex(row, ids, n_ids, uniform, sp, mode == 1);
}
int tts_host_sample_prefiltered_ex(const float *row, const int32_t *ids, int n_ids, float uniform, float temperature, int top_k, float top_p, float penalty, int keep,
                                   int already_penalised) {
  if (!sampler_params_ok(row, ids, n_ids, temperature, top_k, top_p, penalty) || keep < 1 || keep > TTS_PF_MAX) return -2;
  SamplerParams sp; sp.temp = temperature; sp.top_k = top_k; sp.top_p = top_p; sp.penalty = penalty;
  std::vector<int32_t> list(TTS_PF_WORDS);
  std::vector<float> pen; // already_penalised: what sample_prefilter_kernel<true> thresholds, the penalised row
  if (already_penalised) {
    pen.assign(row, row + TTS_VOCAB_MEL);
    for (int i = 0; i < n_ids; i++) { const float g = row[ids[i]]; pen[ids[i]] = g < 0 ? g * penalty : g / penalty; }
    row = pen.data();
  }
  if (host_prefilter_row(row, keep, list.data()) < 0) return -1;
  return sample_one_from_list_ex(list.data(), ids, n_ids, uniform, sp, already_penalised != 0);
}
int tts_host_typical_keep(const float *row, double mass, uint8_t *keep_out) {
  if (!row || !keep_out || mass == 0 || ar_control_error(5, mass)) return -2;
  return typical_keep(row, (double)(float)mass, (char *)keep_out);
}
int tts_host_sample_row_typical(const float *row, const int32_t *ids, int n_ids, float uniform, float temperature, int top_k, float top_p, float penalty, double mass,
                                int mode) {
  if (!sampler_params_ok(row, ids, n_ids, temperature, top_k, top_p, penalty) || (mode != 0 && mode != 1) || ar_control_error(5, mass)) return -2;
  SamplerParams sp; sp.temp = temperature; sp.top_k = top_k; sp.top_p = top_p; sp.penalty = penalty; sp.typ_mass = (float)mass;
  return sample_one_row_ex(row, ids, n_ids, uniform, sp, mode == 1);
}
int tts_host_sample_prefiltered_typical(const float *row, const int32_t *ids, int n_ids, float uniform, float temperature, int top_k, float top_p, float penalty,
                                        double mass, int keep) {
  if (ar_control_error(5, mass)) return -2;
  if (mass == 0) return tts_host_sample_prefiltered_ex(row, ids, n_ids, uniform, temperature, top_k, top_p, penalty, keep, 1);
  if (!sampler_params_ok(row, ids, n_ids, temperature, top_k, top_p, penalty) || keep < 1 || keep > TTS_PF_MAX) return -2;
  SamplerParams sp; sp.temp = temperature; sp.top_k = top_k; sp.top_p = top_p; sp.penalty = penalty; sp.typ_mass = (float)mass;
  std::vector<int32_t> list(TTS_PF_WORDS);
  std::vector<float> pen(row, row + TTS_VOCAB_MEL); // what the typical body sees in either scope: the penalised row
  for (int i = 0; i < n_ids; i++) { const float g = row[ids[i]]; pen[ids[i]] = g < 0 ? g * penalty : g / penalty; }
  if (host_prefilter_row_typical(pen.data(), (double)sp.typ_mass, keep, list.data()) < 0) return -1;
  return sample_one_from_list_ex(list.data(), ids, n_ids, uniform, sp, true);
}
int tts_host_sample_prefiltered(const float *row, const int32_t *ids, int ids_per_cand, float uniform, int keep) {
  if (!row || !ids || ids_per_cand < 1 || keep < 1 || keep > TTS_PF_MAX) return -2;
  std::vector<int32_t> list(TTS_PF_WORDS);
  if (host_prefilter_row(row, keep, list.data()) < 0) return -1;
  return sample_one_from_list(list.data(), ids, ids_per_cand, uniform);
}
int tts_ar_latents(tts_ctx *c, const int32_t *codes, int nb, int n_mel, float *out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_latents");
  return guarded(c, [&] { return ar_latents(c, codes, nb, n_mel, out); });
}
int tts_sample(tts_ctx *c, const float *logits, const int32_t *ids, int ids_per_cand, int B, int32_t *out) {
  if (!c || !logits || !ids || !out || B < 1 || ids_per_cand < 1) return TTS_ERR_ARG;
  for (int i = 0; i < B * ids_per_cand; i++)
    if (ids[i] < 0 || ids[i] >= TTS_VOCAB_MEL) return fail(c, TTS_ERR_ARG, "penalty id out of range");
  if (int rc = shard_check(c, B)) return rc;
  return guarded(c, [&] { sample_candidates(c, c->generator, c->ar_sp, logits, ids, ids_per_cand, B, out); return (int)TTS_OK; });
}

// The decode loop behind the calls below: ar_driver.cpp.
int tts_autoregressive(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice, int B, int max_steps,
                       unsigned flags, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_autoregressive");
  return guarded(c, [&] {
    return ar_drv_autoregressive(c, text_ids, &n_text, 1, voice, 1, nullptr, &B, max_steps, flags, codes_out, rows_out, latents_out, steps_out);
  });
}

int tts_hifigan_stream(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice, int max_steps, unsigned flags, int stride_codes, tts_audio_cb cb,
                       void *user, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_hifigan_stream");
  if (stride_codes < 1 || !cb) return fail(c, TTS_ERR_ARG, "tts_hifigan_stream: bad argument (stride_codes %d: >= 1, a callback)", stride_codes);
  if (!c->ar) return fail(c, TTS_ERR_STATE, "AR model not loaded");
  if (!c->hifigan) return fail(c, TTS_ERR_STATE, "tts_load_hifigan not called");
  if (voice)
    for (int i = 0; i < TTS_DMODEL; i++)
      if (!std::isfinite(voice[i])) return fail(c, TTS_ERR_ARG, "tts_hifigan_stream: the voice holds a non-finite value");
  return guarded(c, [&] {
    const int B = 1;
    return ar_drv_autoregressive(c, text_ids, &n_text, 1, voice, 1, nullptr, &B, max_steps, flags, codes_out, rows_out, latents_out, steps_out, stride_codes, cb, user);
  });
}

int tts_autoregressive_multi(tts_ctx *c, const int32_t *text_ids, const int32_t *n_text, int n_prompts, const float *voice, const int32_t *n_cand, int max_steps,
                             unsigned flags, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_autoregressive_multi");
  if (n_prompts < 1 || !n_text || !n_cand) return fail(c, TTS_ERR_ARG, "tts_autoregressive_multi: bad argument");
  return guarded(c, [&] {
    return ar_drv_autoregressive(c, text_ids, n_text, n_prompts, voice, 1, nullptr, n_cand, max_steps, flags, codes_out, rows_out, latents_out, steps_out);
  });
}

int tts_ar_begin_multi(tts_ctx *c, const int32_t *text_ids, const int32_t *n_text, int n_prompts, const float *voice, const int32_t *n_cand, int max_steps) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_begin_multi");
  if (n_prompts < 1 || !n_text || !n_cand) return fail(c, TTS_ERR_ARG, "tts_ar_begin_multi: bad argument");
  return guarded(c, [&] { return ar_begin_groups(c, text_ids, n_text, n_prompts, voice, 1, nullptr, n_cand, max_steps); });
}

// Several voices in one batch (API version 8): the voice table and the groups' rows of it are checked by ar_begin_groups before any device work.
int tts_ar_begin_multi_voice(tts_ctx *c, const int32_t *text_ids, const int32_t *n_text, int n_prompts, const float *voices, int n_voices,
                             const int32_t *voice_of_prompt, const int32_t *n_cand, int max_steps) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_begin_multi_voice");
  if (n_prompts < 1 || !n_text || !n_cand || !voices || !voice_of_prompt || n_voices < 1) return fail(c, TTS_ERR_ARG, "tts_ar_begin_multi_voice: bad argument");
  return guarded(c, [&] { return ar_begin_groups(c, text_ids, n_text, n_prompts, voices, n_voices, voice_of_prompt, n_cand, max_steps); });
}

int tts_autoregressive_multi_voice(tts_ctx *c, const int32_t *text_ids, const int32_t *n_text, int n_prompts, const float *voices, int n_voices,
                                   const int32_t *voice_of_prompt, const int32_t *n_cand, int max_steps, unsigned flags, int32_t *codes_out, int32_t *rows_out,
                                   float *latents_out, int32_t *steps_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_autoregressive_multi_voice");
  if (n_prompts < 1 || !n_text || !n_cand || !voices || !voice_of_prompt || n_voices < 1)
    return fail(c, TTS_ERR_ARG, "tts_autoregressive_multi_voice: bad argument");
  return guarded(c, [&] {
    return ar_drv_autoregressive(c, text_ids, n_text, n_prompts, voices, n_voices, voice_of_prompt, n_cand, max_steps, flags, codes_out, rows_out, latents_out,
                               steps_out);
  });
}

int tts_split_turns(tts_ctx *c, const char *message, int n_voices, int max_ids, int32_t *starts_out, int32_t *lens_out, int32_t *voice_out, int cap) {
  if (!c) return TTS_ERR_ARG;
  if (!c->tok) return fail(c, TTS_ERR_STATE, "tokenizer not loaded");
  if (!message || n_voices < 1 || max_ids < 3 || max_ids > 404 || cap < 0 || (cap > 0 && (!starts_out || !lens_out || !voice_out)))
    return fail(c, TTS_ERR_ARG, "tts_split_turns: bad argument (n_voices %d: >= 1, max_ids %d: 3 .. 404)", n_voices, max_ids);
  return guarded(c, [&] {
    std::vector<TurnChunk> ch;
    long bad = 0;
    if (!split_turns(*c->tok, message, n_voices, max_ids, ch, &bad)) return fail(c, TTS_ERR_ARG, "tts_split_turns: a turn names voice %ld of %d", bad, n_voices);
    for (int k = 0; k < (int)ch.size() && k < cap; k++) { starts_out[k] = ch[k].start; lens_out[k] = ch[k].len; voice_out[k] = ch[k].voice; }
    return (int)ch.size();
  });
}

int tts_split_text(tts_ctx *c, const char *message, int max_ids, int32_t *starts_out, int32_t *lens_out, int cap) {
  if (!c) return TTS_ERR_ARG;
  if (!c->tok) return fail(c, TTS_ERR_STATE, "tokenizer not loaded");
  if (!message || max_ids < 3 || max_ids > 404 || cap < 0 || (cap > 0 && (!starts_out || !lens_out)))
    return fail(c, TTS_ERR_ARG, "tts_split_text: bad argument (max_ids %d: 3 .. 404)", max_ids);
  return guarded(c, [&] {
    const std::vector<std::pair<int, int>> ch = split_text(*c->tok, message, max_ids);
    for (int k = 0; k < (int)ch.size() && k < cap; k++) { starts_out[k] = ch[k].first; lens_out[k] = ch[k].second; }
    return (int)ch.size();
  });
}

int tts_ar_set_stop_schedule(tts_ctx *c, const int32_t *stop_at, int n_candidates) {
  if (!c || n_candidates < 0) return TTS_ERR_ARG;
  return guarded(c, [&]() -> int { // (vector::assign may throw: nothing crosses the C ABI)
    if (!stop_at || n_candidates == 0) { c->stop_schedule.clear(); return TTS_OK; }
    for (int b = 0; b < n_candidates; b++)
      if (stop_at[b] < 1) return fail(c, TTS_ERR_ARG, "tts_ar_set_stop_schedule: candidate %d would stop before its first code", b);
    c->stop_schedule.assign(stop_at, stop_at + n_candidates);
    return TTS_OK;
  });
}

int tts_ar_stop_status(tts_ctx *c, int32_t *stopped_out, int n_candidates) {
  if (!c || !stopped_out || n_candidates < 1) return TTS_ERR_ARG;
  if ((int)c->ar_stopped.size() != n_candidates) return fail(c, TTS_ERR_STATE, "tts_ar_stop_status: the last tts_autoregressive call had %d candidates", (int)c->ar_stopped.size());
  std::copy(c->ar_stopped.begin(), c->ar_stopped.end(), stopped_out);
  return TTS_OK;
}

// ---- in-flight batching (include/tortoise_mi355x.h: tts_ar_session_*) ----
int tts_host_session_first_fit(const uint8_t *busy, int n_slots, int n_cand) {
  if (!busy || n_slots < 1 || n_cand < 1) return -1;
  return session_first_fit(busy, n_slots, n_cand);
}

#define NEED_SESSION(c, name)                                                                       \
  do {                                                                                              \
    if (!(c)->session) return fail((c), TTS_ERR_STATE, "%s: tts_ar_session_open not called", name); \
  } while (0)

int tts_ar_session_close(tts_ctx *c) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_close");
  ar_drv_close(c);
  return TTS_OK;
}

int tts_ar_session_open(tts_ctx *c, int n_slots, int max_cand, int max_text, int max_steps, unsigned flags) {
  NEED_CTX(c);
  if (!c->ar) return fail(c, TTS_ERR_STATE, "AR model not loaded");
  if (n_slots < 1 || max_cand < 1 || max_cand > n_slots || max_text < 1 || max_steps < 1 ||
      (flags & ~(unsigned)(TTS_AR_MASK_STOP | TTS_AR_RETIRE | TTS_AR_ROW_CONTROLS)))
    return fail(c, TTS_ERR_ARG, "tts_ar_session_open: bad argument (n_slots %d: >= 1, max_cand %d: 1 .. n_slots, max_text %d, max_steps %d: >= 1, flags %u)", n_slots,
                max_cand, max_text, max_steps, flags);
  if (n_slots > 4096) return fail(c, TTS_ERR_LIMIT, "tts_ar_session_open: %d slots, at most 4096", n_slots);
  if (max_text > 404) return fail(c, TTS_ERR_LIMIT, "text of %d ids; the model has 404 text positions", max_text);
  if (max_steps > 500) return fail(c, TTS_ERR_LIMIT, "max_steps %d exceeds the 500 codes apply_padding accepts", max_steps);
  if (max_text + 2 + max_steps + 1 > 1024) return fail(c, TTS_ERR_LIMIT, "context of %d positions exceeds 1024", max_text + 2 + max_steps + 1);
  return guarded(c, [&] { return ar_drv_open(c, n_slots, max_cand, max_text, max_steps, flags); });
}

int tts_ar_session_room(const tts_ctx *c) {
  if (!c) return TTS_ERR_ARG;
  if (c->device < 0) return TTS_ERR_HIP;
  if (!c->session) return TTS_ERR_STATE;
  return ar_drv_room(c);
}

int tts_ar_session_recaptures(const tts_ctx *c) {
  if (!c) return TTS_ERR_ARG;
  if (c->device < 0) return TTS_ERR_HIP;
  if (!c->session) return TTS_ERR_STATE;
  return ar_session_recaptures(c);
}

// What a request descriptor must satisfy in a session of max_cand candidates and max_steps steps, before any device work: the status, and in `why` the text.
// On TTS_OK sp / scope hold the request's controls as the sampler will read them.
// The struct's growth rule: the size a header before "typical_mass" declared, or one that covers every field this library knows.
static const size_t kArRequestSize0 = offsetof(tts_ar_request, typical_mass);
static bool request_size_ok(uint32_t n) { return n == kArRequestSize0 || n >= sizeof(tts_ar_request); }
// pinned_mass: what a descriptor of the older size runs under (the session's).
static int request_check(const tts_ar_request *req, int max_cand, int max_steps, double pinned_mass, SamplerParams &sp, int &scope, std::string &why) {
  char buf[200];
  if (!req) { why = "null request"; return TTS_ERR_ARG; }
  if (!request_size_ok(req->struct_size)) {
    snprintf(buf, sizeof buf, "struct_size %u, version 8 declares %zu bytes (%zu before typical_mass was appended; set it to sizeof(tts_ar_request))", req->struct_size,
             sizeof(tts_ar_request), kArRequestSize0);
    why = buf;
    return TTS_ERR_ARG;
  }
  if (req->n_cand < 1) { snprintf(buf, sizeof buf, "bad argument (%d candidates)", req->n_cand); why = buf; return TTS_ERR_ARG; }
  if (req->n_cand > max_cand) { snprintf(buf, sizeof buf, "%d candidates, the session was opened for %d", req->n_cand, max_cand); why = buf; return TTS_ERR_LIMIT; }
  if (req->stop_at)
    for (int b = 0; b < req->n_cand; b++)
      if (req->stop_at[b] < 1) { snprintf(buf, sizeof buf, "candidate %d would stop before its first code", b); why = buf; return TTS_ERR_ARG; }
  if (req->max_steps < 0) { snprintf(buf, sizeof buf, "max_steps %d: 0 (the session's) or 1 .. %d", req->max_steps, max_steps); why = buf; return TTS_ERR_ARG; }
  if (req->max_steps > max_steps) { snprintf(buf, sizeof buf, "max_steps %d, the session was opened for %d", req->max_steps, max_steps); why = buf; return TTS_ERR_LIMIT; }
  const double v[6] = {req->temperature, req->top_k, req->top_p, req->repetition_penalty, req->penalty_scope,
                       req->struct_size >= sizeof(tts_ar_request) ? req->typical_mass : pinned_mass};
  for (int k = 0; k < 6; k++) {
    if (const char *e = ar_control_error(k, v[k])) { why = e; return TTS_ERR_ARG; }
    ar_control_store(k, v[k], sp, scope);
  }
  return TTS_OK;
}

int tts_host_ar_request_check(const tts_ar_request *req, int max_cand, int max_steps) {
  if (max_cand < 1 || max_steps < 1) return TTS_ERR_ARG;
  SamplerParams sp;
  int scope = 0;
  std::string why;
  return request_check(req, max_cand, max_steps, 0.0, sp, scope, why);
}

int tts_ar_request_init(tts_ctx *c, tts_ar_request *req) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_request_init");
  if (!req) return fail(c, TTS_ERR_ARG, "tts_ar_request_init: null request");
  if (!request_size_ok(req->struct_size))
    return fail(c, TTS_ERR_ARG, "tts_ar_request_init: struct_size %u, version 8 declares %zu bytes (set it to sizeof(tts_ar_request) first)", req->struct_size,
                sizeof(tts_ar_request));
  req->n_cand = 1; req->seed = 0; req->max_steps = 0; req->stop_at = nullptr;
  tts_ar_request d;
  ar_drv_defaults(c, &d);
  req->temperature = d.temperature; req->top_k = d.top_k; req->top_p = d.top_p; req->repetition_penalty = d.repetition_penalty; req->penalty_scope = d.penalty_scope;
  if (req->struct_size >= sizeof(tts_ar_request)) req->typical_mass = d.typical_mass; // an older caller's struct ends before the field
  return TTS_OK;
}

// ---- the session's entry points (state and host rules: ar_driver.cpp; device work: ar.hip) ----
int tts_ar_session_admit(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice, int n_cand, uint32_t seed, const int32_t *stop_at) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_admit");
  return guarded(c, [&] { return ar_drv_admit(c, "tts_ar_session_admit", text_ids, n_text, voice, n_cand, seed, stop_at, nullptr, 0, 0); });
}
int tts_ar_session_admit_ex(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice, const tts_ar_request *req) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_admit_ex");
  SamplerParams sp;
  int scope = 0, max_cand = 0, max_steps = 0;
  ar_drv_limits(c, max_cand, max_steps);
  std::string why;
  tts_ar_request pinned;
  ar_drv_defaults(c, &pinned);
  if (int rc = request_check(req, max_cand, max_steps, pinned.typical_mass, sp, scope, why)) return fail(c, rc, "tts_ar_session_admit_ex: %s", why.c_str());
  return guarded(c, [&] {
    return ar_drv_admit(c, "tts_ar_session_admit_ex", text_ids, n_text, voice, req->n_cand, req->seed, req->stop_at, &sp, scope, req->max_steps);
  });
}
int tts_ar_session_step(tts_ctx *c) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_step");
  return guarded(c, [&] { return ar_drv_step(c); });
}
int tts_ar_session_finished(tts_ctx *c, int32_t *ids_out, int cap) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_finished");
  if (cap < 0 || (cap > 0 && !ids_out)) return fail(c, TTS_ERR_ARG, "tts_ar_session_finished: bad argument");
  return ar_drv_finished(c, ids_out, cap);
}
int tts_ar_session_collect(tts_ctx *c, int request, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out, int32_t *stopped_out) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_collect");
  if (!codes_out || !rows_out) return fail(c, TTS_ERR_ARG, "tts_ar_session_collect: null output");
  return guarded(c, [&] { return ar_drv_collect(c, request, codes_out, rows_out, latents_out, steps_out, stopped_out); });
}
int tts_ar_session_logits(tts_ctx *c, int request, float *logits_out) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_logits");
  if (!logits_out) return fail(c, TTS_ERR_ARG, "tts_ar_session_logits: null output");
  return guarded(c, [&] { return ar_drv_logits(c, request, logits_out); });
}
int tts_ar_session_cancel(tts_ctx *c, int request) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_cancel");
  return guarded(c, [&] { return ar_drv_cancel(c, request); });
}
int tts_ar_session_enable_audio(tts_ctx *c, int stride_steps) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_enable_audio");
  if (stride_steps < 1) return fail(c, TTS_ERR_ARG, "tts_ar_session_enable_audio: stride_steps %d: >= 1", stride_steps);
  if (!c->hifigan) return fail(c, TTS_ERR_STATE, "tts_ar_session_enable_audio: tts_load_hifigan not called");
  return guarded(c, [&] { return ar_drv_enable_audio(c, stride_steps); });
}
int tts_ar_session_audio(tts_ctx *c, int request, float *out, int cap_samples, int32_t *is_last) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_audio");
  return guarded(c, [&] { return ar_drv_audio(c, request, out, cap_samples, is_last); });
}

// ---- diffusion session: the entry points (state and device work: diffusion.hip; descriptor checks: host_logic.cpp) ----
#define NEED_DIFF_SESSION(c, name)                                                                          \
  do {                                                                                                      \
    if (!(c)->diff_session) return fail((c), TTS_ERR_STATE, "%s: tts_diff_session_open not called", name); \
  } while (0)
int tts_diff_session_open(tts_ctx *c, int max_packed_rows, int max_requests) {
  NEED_CTX(c);
  if (!c->diff) return fail(c, TTS_ERR_STATE, "diffusion model not loaded");
  if (max_packed_rows < 128 || max_requests < 1)
    return fail(c, TTS_ERR_ARG, "tts_diff_session_open: bad argument (max_packed_rows %d: >= 128, max_requests %d: >= 1)", max_packed_rows, max_requests);
  if (max_packed_rows > (1 << 20) || max_requests > 4096)
    return fail(c, TTS_ERR_LIMIT, "tts_diff_session_open: %d rows / %d requests, at most 2^20 / 4096", max_packed_rows, max_requests);
  return guarded(c, [&] { return diff_session_open(c, max_packed_rows, max_requests); });
}
int tts_diff_session_close(tts_ctx *c) {
  NEED_CTX(c);
  NEED_DIFF_SESSION(c, "tts_diff_session_close");
  diff_session_close(c);
  return TTS_OK;
}
int tts_diff_request_init(tts_ctx *c, tts_diff_request *req) {
  NEED_CTX(c);
  NEED_DIFF_SESSION(c, "tts_diff_request_init");
  if (!req) return fail(c, TTS_ERR_ARG, "tts_diff_request_init: null request");
  if (!diff_request_size_ok(req->struct_size))
    return fail(c, TTS_ERR_ARG, "tts_diff_request_init: struct_size %u, version 8 declares %zu bytes (set it to sizeof(tts_diff_request) first)", req->struct_size,
                sizeof(tts_diff_request));
  req->n_cand = 1; req->latents = nullptr; req->rows = nullptr; req->voice_latent2048 = nullptr; req->n_steps = 80; req->noise = nullptr; req->seed = 0;
  diff_session_defaults(c, req);
  return TTS_OK;
}
int tts_diff_session_room(const tts_ctx *c) {
  if (!c) return TTS_ERR_ARG;
  if (c->device < 0) return TTS_ERR_HIP;
  if (!c->diff_session) return TTS_ERR_STATE;
  return diff_session_room(c);
}
int tts_diff_session_captures(const tts_ctx *c) {
  if (!c) return TTS_ERR_ARG;
  if (c->device < 0) return TTS_ERR_HIP;
  if (!c->diff_session) return TTS_ERR_STATE;
  return diff_session_captures(c);
}
int tts_diff_session_admit(tts_ctx *c, const tts_diff_request *req) {
  NEED_CTX(c);
  NEED_DIFF_SESSION(c, "tts_diff_session_admit");
  std::string why; // every check before any device work
  tts_diff_request pinned;
  pinned.struct_size = sizeof pinned;
  diff_session_defaults(c, &pinned);
  if (int rc = diff_request_check(req, diff_session_room(c), pinned.temperature, pinned.cond_free, why)) return fail(c, rc, "tts_diff_session_admit: %s", why.c_str());
  return guarded(c, [&] { return diff_session_admit(c, req); });
}
int tts_diff_session_step(tts_ctx *c) {
  NEED_CTX(c);
  NEED_DIFF_SESSION(c, "tts_diff_session_step");
  return guarded(c, [&] { return diff_session_step(c); });
}
int tts_diff_session_finished(tts_ctx *c, int32_t *ids, int cap) {
  NEED_CTX(c);
  NEED_DIFF_SESSION(c, "tts_diff_session_finished");
  if (cap < 0 || (cap > 0 && !ids)) return fail(c, TTS_ERR_ARG, "tts_diff_session_finished: bad argument");
  return guarded(c, [&] { return diff_session_finished(c, ids, cap); });
}
int tts_diff_session_collect(tts_ctx *c, int request, float *mel_out) {
  NEED_CTX(c);
  NEED_DIFF_SESSION(c, "tts_diff_session_collect");
  if (!mel_out) return fail(c, TTS_ERR_ARG, "tts_diff_session_collect: null output");
  return guarded(c, [&] { return diff_session_collect(c, request, mel_out); });
}
int tts_diff_session_cancel(tts_ctx *c, int request) {
  NEED_CTX(c);
  NEED_DIFF_SESSION(c, "tts_diff_session_cancel");
  return guarded(c, [&] { return diff_session_cancel(c, request); });
}

int tts_diffusion_forward(tts_ctx *c, const float *latents, int L, const float *x_t, int timestep, int cond_free, float *out) {
  NEED_CTX(c);
  NO_DIFF_SESSION(c, "tts_diffusion_forward");
  return guarded(c, [&] { return diff_forward(c, latents, L, x_t, timestep, cond_free, out); });
}
int tts_diffusion(tts_ctx *c, const float *latents, const int32_t *rows, int B, int n_steps, const float *noise,
                  int noise_mode, float *mel_out) {
  NEED_CTX(c);
  // the DEVICE noise streams are keyed by the global candidate id; host / reference noise does not look at the shard options
  NO_DIFF_SESSION(c, "tts_diffusion");
  if (B >= 1 && !noise && noise_mode == TTS_NOISE_DEVICE) if (int rc = shard_check(c, B)) return rc;
  return guarded(c, [&] { return diff_sample(c, latents, rows, B, n_steps, noise, noise_mode, mel_out); });
}
int tts_diffusion_multi_voice(tts_ctx *c, const float *latents, const int32_t *rows, int B, const float *voice_latents, int n_voices,
                              const int32_t *voice_of_candidate, int n_steps, const float *noise, int noise_mode, float *mel_out) {
  NEED_CTX(c);
  NO_DIFF_SESSION(c, "tts_diffusion_multi_voice");
  if (B >= 1 && !noise && noise_mode == TTS_NOISE_DEVICE) if (int rc = shard_check(c, B)) return rc;
  return guarded(c, [&] { return diff_sample_voices(c, latents, rows, B, voice_latents, n_voices, voice_of_candidate, n_steps, noise, noise_mode, mel_out); });
}
int tts_diffusion_last_layout(const tts_ctx *c, int32_t *packed_rows_out, int32_t *sequences_out) {
  if (!c || !packed_rows_out || !sequences_out) return TTS_ERR_ARG;
  if (c->device < 0) return TTS_ERR_HIP;
  if (c->last_diff_rows < 0) return TTS_ERR_STATE;
  *packed_rows_out = c->last_diff_rows; *sequences_out = c->last_diff_seqs;
  return TTS_OK;
}
int tts_vocoder_samples(int T) { return (T + 10) * 256 - 6; }
int tts_vocoder(tts_ctx *c, const float *mel, const int32_t *frames, int B, const float *noise, int noise_mode, float *audio) {
  NEED_CTX(c);
  if (B >= 1 && !noise && noise_mode == TTS_NOISE_DEVICE) if (int rc = shard_check(c, B)) return rc;
  return guarded(c, [&] { return voc_run(c, mel, frames, B, noise, noise_mode, audio); });
}

// Streaming form of the vocoder for first-audio latency: the UnivNet stack is fully convolutional, so the samples of frames
// [frame0, frame0 + n_frames) depend only on mel / noise frames within a bounded halo (conv_pre k7, kernel predictor k5 + 6 x k3 + k3,
// transposed convs, the dilated 1/3/9/27 convs of the 8-sample stage ~ 6 frames, conv_post k7): a window of the sequence with
// VOC_HALO frames on either side reproduces them exactly; windows that touch a sequence end keep the reference's boundary treatment
// (reflect pad / zero pad / the 10 silent frames) because they coincide with it. The halo is tied to the loaded architecture in
// vocoder.hip (voc_receptive_frames: 20 frames for UnivNet c32, static_assert against TTS_VOC_CHUNK_HALO). Cost: every chunk evaluates
// up to 2 x 24 + 10 extra frames (a 100-frame chunk costs ~1.6x its share of the one-shot call).
int tts_vocoder_chunk(tts_ctx *c, const float *mel, int T, const float *noise, int frame0, int n_frames, float *audio_out,
                      int *n_samples_out) {
  NEED_CTX(c);
  if (!mel || !noise || !audio_out || T < 1 || n_frames < 1 || frame0 < 0 || frame0 >= T + 10)
    return fail(c, TTS_ERR_ARG, "tts_vocoder_chunk: bad argument");
  return guarded(c, [&] {
    const int Tm = T + 10, f1 = std::min(Tm, frame0 + n_frames);
    const int halo = voc_halo_frames();
    int w0 = std::max(0, frame0 - halo), w1 = f1 + halo;
    if (w1 >= T) w1 = Tm;                                   // the window reaches the silent pad frames: take the true end
    const int wt = (w1 == Tm ? T : w1) - w0;                // mel frames handed to the vocoder (it appends 10 pad frames itself)
    std::vector<float> wm((size_t)100 * wt), wn((size_t)64 * (wt + 10)), wa((size_t)(wt + 10) * 256);
    for (int ch = 0; ch < 100; ch++) memcpy(&wm[(size_t)ch * wt], mel + (size_t)ch * T + w0, (size_t)wt * 4);
    for (int ch = 0; ch < 64; ch++)
      for (int t = 0; t < wt + 10; t++) wn[(size_t)ch * (wt + 10) + t] = noise[(size_t)ch * Tm + std::min(w0 + t, Tm - 1)];
    const int32_t frames = wt;
    int rc = voc_run(c, wm.data(), &frames, 1, wn.data(), TTS_NOISE_REFERENCE, wa.data());
    if (rc) return rc;
    const int64_t total = (int64_t)Tm * 256 - 6, s0 = (int64_t)frame0 * 256, s1 = std::min<int64_t>((int64_t)f1 * 256, total);
    const int64_t n = std::max<int64_t>(0, s1 - s0);
    memcpy(audio_out, wa.data() + (s0 - (int64_t)w0 * 256), (size_t)n * 4);
    if (n_samples_out) *n_samples_out = (int)n;
    return (int)TTS_OK;
  });
}

static void prof_resolve(tts_ctx *c) {
  (void)hipStreamSynchronize(c->stream);
  for (auto &kv : c->prof) {
    for (auto &pr : kv.second.pending) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { kv.second.ms += ms; kv.second.launches++; }
      c->ev_pool.push_back(pr.first);
      c->ev_pool.push_back(pr.second);
    }
    kv.second.pending.clear();
  }
}
int tts_prof_reset(tts_ctx *c, int enable) {
  if (!c) return TTS_ERR_ARG;
  if (c->device >= 0) prof_resolve(c);
  c->prof.clear();
  c->prof_on = enable != 0;
  return TTS_OK;
}
int tts_prof_get(tts_ctx *c, const char *family, double *ms, int64_t *launches, double *work) {
  if (!c || !family) return TTS_ERR_ARG;
  if (c->device >= 0) prof_resolve(c);
  // a family name also names its sub-families ("diff_gemm" = diff_gemm_qkv + diff_gemm_k3 + ...: the GEMM launches are recorded per shape class)
  double tms = 0, tw = 0;
  int64_t tl = 0;
  const std::string f(family), pre = f + "_";
  for (auto &kv : c->prof)
    if (kv.first == f || kv.first.rfind(pre, 0) == 0) { tms += kv.second.ms; tl += kv.second.launches; tw += kv.second.work; }
  if (ms) *ms = tms;
  if (launches) *launches = tl;
  if (work) *work = tw;
  return TTS_OK;
}

} // extern "C"
