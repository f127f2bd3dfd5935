// C ABI of libtortoise_mi355x.so (see include/tortoise_mi355x.h for the reference call sites).
#include "common.h"
#include <sched.h>
#include <cctype>
#include <cmath>
#include <algorithm>
#include <chrono>
#include <fstream>
#include <new>

namespace tts {
int ar_begin(tts_ctx *, const int32_t *, int, const float *, int, int);
int ar_begin_groups(tts_ctx *, const int32_t *, const int *, int, const float *, int n_voices, const int *voice_of, const int *, int);
int ar_latents_group(tts_ctx *, int, const int32_t *, int, float *);
int ar_stream_reserve(tts_ctx *, int n_mel);
int ar_graph_captures(const tts_ctx *);
int ar_session_open(tts_ctx *, int n_slots, int max_cand, int max_text, int max_steps, bool rows);
int ar_session_controls(tts_ctx *, int c0, int n);
void ar_session_close(tts_ctx *);
int ar_session_prompt(tts_ctx *, int c0, int n_cand, const int32_t *text_ids, int n_text, const float *voice, float *logits_row);
int ar_session_step(tts_ctx *, const int32_t *toks, const int32_t *n_past, const int32_t *pos_id, const char *live, int mode);
int ar_session_recaptures(const tts_ctx *);
int ar_session_latents(tts_ctx *, int c0, int n_text, const int32_t *codes502, int nb, int n_mel, float *out);
int ar_session_logits(tts_ctx *, int c0, int n, float *out);
int ar_session_audio_enable(tts_ctx *, int max_steps);
int ar_session_audio_prompt(tts_ctx *, int c0, int n_text);
int ar_session_extend(tts_ctx *, const ArExtendItem *items, int n_items, float *out);
int ar_prefill(tts_ctx *, float *);
int ar_step(tts_ctx *, const int32_t *, int, float *, int mode);
const int32_t *ar_host_lists(tts_ctx *);
const float *ar_fetch_logits_row(tts_ctx *, int);
void ar_history_ids(const tts_ctx *, int c, std::vector<int32_t> &out);
int ar_batch(const tts_ctx *);
int ar_latents(tts_ctx *, const int32_t *, int, int, float *);
int ar_layers(const tts_ctx *);
float *ar_host_logits(tts_ctx *);
int diff_layers(const tts_ctx *);
int diff_forward(tts_ctx *, const float *, int, const float *, int, int, float *);
int diff_sample(tts_ctx *, const float *, const int32_t *, int, int, const float *, int, float *);
int diff_sample_voices(tts_ctx *, const float *, const int32_t *, int, const float *, int, const int32_t *, int, const float *, int, float *);
int voc_run(tts_ctx *, const float *, const int32_t *, int, const float *, int, float *);
} // namespace tts

// The book of an open session (tts_ar_session_*): which slots are taken, and per request what tts_autoregressive keeps in its locals for one call.
namespace tts {
struct SessionRequest {
  int id = 0, c0 = 0, n_cand = 0, n_text = 0;
  std::mt19937 gen;              // seeded at admission: tts_autoregressive's stream after tts_seed(seed)
  ArStopBook book;               // one group
  std::vector<int32_t> stop_at;  // the request's stop schedule (empty: none)
  std::vector<int32_t> samples;  // the tokens the next step feeds (after ArStopBook::step)
  int i = 0;                     // tts_autoregressive's loop counter: iterations applied so far
  // the request's own sampler controls and step limit (tts_ar_session_admit_ex; tts_ar_session_admit: the session's)
  SamplerParams sp;
  int scope = 0, max_steps = 0;
  int state = 0;                 // 0 running, 1 finished, 2 finished by reaching max_steps in strict mode (collect returns TTS_ERR_LIMIT)
  // Audio (a one-candidate request of a session with tts_ar_session_enable_audio): tts_hifigan_stream's book, HfgStream, per request.
  bool audio = false, audio_done = false; // audio_done: the request has finished and its last frames are in pcm
  int have = 0, emitted = 0;              // latent rows held (frozen once a chunk was decoded from them), frames decoded so far
  std::vector<float> voice, lat, pcm;     // the request's voice [1024]; its latent rows [have][1024]; the samples tts_ar_session_audio has not drained yet
};
struct ArSession {
  int n_slots = 0, max_cand = 0, max_text = 0, max_steps = 0;
  unsigned flags = 0;
  // the options read once at tts_ar_session_open: every session call runs under them (SessionOptions), whatever tts_set_option has stored since
  SamplerParams sp;
  int scope = 0, ar_weights = 0, ggml_lut = 0, device_topk = 1;
  std::vector<uint8_t> busy;
  std::map<int, SessionRequest> reqs;
  std::vector<int> finished; // ids, oldest first
  int next_id = 0;
  int audio_stride = 0;      // tts_ar_session_enable_audio: steps of the session's clock between two audio passes (0: a session without audio)
  long clock = 0;            // steps the session has run
};
} // namespace tts

using namespace tts;

namespace {
struct SessionOptions { // puts the session's options into the context for the length of one call
  tts_ctx *c;
  SamplerParams sp;
  int scope, w, lut, topk;
  SessionOptions(tts_ctx *ctx, const ArSession &s) : c(ctx), sp(ctx->ar_sp), scope(ctx->ar_penalty_scope), w(ctx->ar_weights), lut(ctx->ggml_lut), topk(ctx->device_topk) {
    c->ar_sp = s.sp; c->ar_penalty_scope = s.scope; c->ar_weights = s.ar_weights; c->ggml_lut = s.ggml_lut; c->device_topk = s.device_topk;
  }
  ~SessionOptions() { c->ar_sp = sp; c->ar_penalty_scope = scope; c->ar_weights = w; c->ggml_lut = lut; c->device_topk = topk; }
};
struct SamplerOptions { // inside a SessionOptions: one request's sampler controls around the calls that sample or write its table rows
  tts_ctx *c;
  SamplerParams sp;
  int scope;
  SamplerOptions(tts_ctx *ctx, const SamplerParams &p, int sc) : c(ctx), sp(ctx->ar_sp), scope(ctx->ar_penalty_scope) { c->ar_sp = p; c->ar_penalty_scope = sc; }
  ~SamplerOptions() { c->ar_sp = sp; c->ar_penalty_scope = scope; }
};
bool same_controls(const SamplerParams &a, int sa, const SamplerParams &b, int sb) {
  return a.temp == b.temp && a.top_k == b.top_k && a.top_p == b.top_p && a.penalty == b.penalty && sa == sb;
}
// first fit: the first index of the lowest run of n_cand free slots, or -1
int session_first_fit(const uint8_t *busy, int n_slots, int n_cand) {
  int run = 0;
  for (int i = 0; i < n_slots; i++) {
    run = busy[i] ? 0 : run + 1;
    if (run == n_cand) return i - n_cand + 1;
  }
  return -1;
}
void session_release(ArSession &s, int id) {
  auto it = s.reqs.find(id);
  if (it == s.reqs.end()) return;
  std::fill(s.busy.begin() + it->second.c0, s.busy.begin() + it->second.c0 + it->second.n_cand, (uint8_t)0);
  s.finished.erase(std::remove(s.finished.begin(), s.finished.end(), id), s.finished.end());
  s.reqs.erase(it);
}
// One iteration of tts_autoregressive's loop from the samples on: the stop rule, then the loop's two exits.
void session_advance(ArSession &s, SessionRequest &r) {
  const bool retire = (s.flags & TTS_AR_RETIRE) != 0;
  const bool sched = !r.stop_at.empty() && (s.flags & TTS_AR_MASK_STOP) && retire;
  const bool all_ended = r.book.step(r.samples.data(), r.i, retire, sched ? r.stop_at.data() : nullptr);
  r.i++;
  if (all_ended) r.state = 1;
  else if (r.i >= r.max_steps) r.state = ((s.flags & TTS_AR_MASK_STOP) || retire) ? 1 : 2;
  if (r.state) s.finished.push_back(r.id);
}
} // namespace

// One audio pass of a session: every audio request that has just finished, and with clock_due every running one, brings its new final latent rows to ONE
// incremental latent pass (ar_session_extend) and its new final frames to ONE ragged tts_hifigan_chunk call. stream_emit's rules per request: after k sampled
// codes the rows stream_final_rows(k) are final and the frames below tts_diffusion_frames(rows) - TTS_HFG_HALO_FRAMES with them; a finished request keeps
// trimmed_latent_rows rows and is decoded to its end; a row is frozen once audio has been decoded from it.
static int session_audio_pass(tts_ctx *c, ArSession &s, bool clock_due) {
  struct Due { SessionRequest *r; std::vector<int32_t> codes; int L, upto; bool last; };
  std::vector<Due> due;
  for (auto &kv : s.reqs) {
    SessionRequest &r = kv.second;
    if (!r.audio || r.audio_done || (r.state == 0 && !clock_due)) continue;
    if (r.state == 2) { r.audio_done = true; continue; } // a strict request that found no stop token: an error of its own, nothing more to hear
    Due d{&r, {}, 0, 0, r.state != 0};
    std::vector<int> sq = r.book.seq[0];
    if (d.last) { // what tts_ar_session_collect will return
      if (sq.size() > 500) sq.resize(500);
      pad_codes(sq);
      d.codes.assign(sq.begin(), sq.end());
      d.L = trimmed_latent_rows(d.codes.data());
      d.upto = tts_diffusion_frames(d.L);
      if (d.L < r.have) return fail(c, TTS_ERR_STATE, "tts_ar_session_step: request %d: %d rows were final, the utterance keeps %d", r.id, r.have, d.L);
    } else { // sq.size() codes so far, none of them the stop token (one candidate: the request ends with it)
      d.codes.assign(502, 83);
      d.codes[0] = 8192;
      std::copy(sq.begin(), sq.begin() + std::min<size_t>(sq.size(), 501), d.codes.begin() + 1);
      d.L = stream_final_rows(d.codes.data() + 1, (int)sq.size());
      d.upto = tts_diffusion_frames(d.L) - TTS_HFG_HALO_FRAMES;
      if (d.L <= r.have || d.upto <= r.emitted) continue;
    }
    due.push_back(std::move(d));
  }
  if (due.empty()) return TTS_OK;
  std::vector<ArExtendItem> items;
  size_t new_rows = 0;
  for (Due &d : due)
    if (d.L > d.r->have) { items.push_back(ArExtendItem{d.r->c0, d.r->n_text, d.r->have, d.L, d.codes.data()}); new_rows += (size_t)(d.L - d.r->have); }
  if (!items.empty()) {
    std::vector<float> rows(new_rows * TTS_DMODEL);
    if (int rc = ar_session_extend(c, items.data(), (int)items.size(), rows.data())) return rc;
    size_t off = 0;
    for (Due &d : due) {
      if (d.L <= d.r->have) continue;
      const size_t n = (size_t)(d.L - d.r->have) * TTS_DMODEL;
      d.r->lat.insert(d.r->lat.end(), rows.begin() + off, rows.begin() + off + n);
      d.r->have = d.L;
      off += n;
    }
  }
  std::vector<float> lat, voices, audio;
  std::vector<int32_t> n_rows, voice_of, f0, nf;
  size_t frames = 0;
  for (Due &d : due) {
    if (d.upto <= d.r->emitted) continue; // (a finished request that keeps no row, or whose frames are all out)
    lat.insert(lat.end(), d.r->lat.begin(), d.r->lat.end());
    voices.insert(voices.end(), d.r->voice.begin(), d.r->voice.end());
    voice_of.push_back((int32_t)n_rows.size());
    n_rows.push_back(d.r->have); f0.push_back(d.r->emitted); nf.push_back(d.upto - d.r->emitted);
    frames += (size_t)(d.upto - d.r->emitted);
  }
  if (!n_rows.empty()) {
    audio.resize(frames * 256);
    if (int rc = hifigan_chunk(c, lat.data(), n_rows.data(), (int)n_rows.size(), voices.data(), (int)n_rows.size(), voice_of.data(), f0.data(), nf.data(), audio.data()))
      return rc;
    size_t off = 0;
    for (Due &d : due) {
      if (d.upto <= d.r->emitted) continue;
      const size_t n = (size_t)(d.upto - d.r->emitted) * 256;
      d.r->pcm.insert(d.r->pcm.end(), audio.begin() + off, audio.begin() + off + n);
      d.r->emitted = d.upto;
      off += n;
    }
  }
  for (Due &d : due)
    if (d.last) d.r->audio_done = true;
  return TTS_OK;
}

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
  delete c->session;
  if (c->device < 0) { delete c->tok; delete c; return; }
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  diff_session_close(c);
  if (c->ar) ar_free(c->ar);
  if (c->diff) diff_free(c->diff);
  if (c->voc) voc_free(c->voc);
  if (c->clvp) clvp_free(c->clvp);
  if (c->venc) voice_enc_free(c->venc);
  if (c->dcond) diff_cond_enc_free(c->dcond);
  if (c->hifigan) hifigan_free(c->hifigan);
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

// The autoregressive sampler's five controls: the ONE statement of what each accepts, for tts_set_option and for a request descriptor (tts_ar_session_admit_ex,
// tts_host_ar_request_check). Returns the refusal's text, or null for a value that is fine.
static const char *const kArControlKeys[5] = {"ar_temperature", "ar_top_k", "ar_top_p", "ar_repetition_penalty", "ar_penalty_scope"};
static int ar_control_index(const std::string &k) {
  for (int i = 0; i < 5; i++)
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
    if (c->ar || c->diff || c->voc || c->clvp || c->venc || c->dcond || c->hifigan) return fail(c, TTS_ERR_STATE, "stream_cus must be set before the models are loaded");
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
int tts_load_clvp(tts_ctx *c, const char *path) { NEED_CTX(c); return guarded(c, [&] { return clvp_load(c, path); }); }
int tts_clvp_score(tts_ctx *c, const int32_t *text_ids, int n_text, const int32_t *codes, const int32_t *code_len, int n_candidates,
                   int code_stride, float *scores_out) {
  NEED_CTX(c);
  return guarded(c, [&] { return clvp_score(c, text_ids, n_text, codes, code_len, n_candidates, code_stride, scores_out); });
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
// decode step + sampler in one call: the device prefilter's lists cross PCIe instead of the logits (ar.hip: sample_prefilter_kernel)
static int step_sample(tts_ctx *c, const int32_t *prev, int i, bool mask_stop, int32_t *out, int *fallbacks) {
  if (int rc = ar_step(c, prev, i, nullptr, mask_stop ? 2 : 1)) return rc;
  const int B = ar_batch(c);
  std::vector<int32_t> hist; // penalty scope 1: the lists hold penalised values; only a full-row fallback needs the candidate's history as ids
  const bool scope1 = c->ar_penalty_scope == 1;
  const PenaltyIdsFn ids_of = [&](int b, const int32_t *&p, int &n) {
    if (scope1) { ar_history_ids(c, b, hist); p = hist.data(); n = (int)hist.size(); }
    else { p = prev + b; n = 1; }
  };
  if (sample_candidates_list(c, c->generator, ar_host_lists(c), ids_of, scope1, B, out, [&](int b) { return ar_fetch_logits_row(c, b); }, fallbacks))
    return fail(c, TTS_ERR_HIP, "tts_ar_step_sample: fetching a logits row failed");
  return TTS_OK;
}
int tts_ar_step_sample(tts_ctx *c, const int32_t *prev, int i, unsigned flags, int32_t *samples_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_ar_step_sample");
  if (!prev || !samples_out) return TTS_ERR_ARG;
  return guarded(c, [&] {
    if (ar_batch(c) < 1) return fail(c, TTS_ERR_STATE, "tts_ar_begin not called"); // before the shard check: with no AR state the batch is 0
    if (int rc = shard_check(c, ar_batch(c))) return rc;
    c->topk_fallbacks = 0;
    return step_sample(c, prev, i, (flags & TTS_AR_MASK_STOP) != 0, samples_out, &c->topk_fallbacks);
  });
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
  return guarded(c, [&] { sample_candidates(c, c->generator, logits, ids, ids_per_cand, B, out); return (int)TTS_OK; });
}

// autoregressive(), main.cpp:5042-5367, for G prompt groups in one decode loop (tts_autoregressive: G = 1; tts_autoregressive_multi). Group g's
// prompt is text_ids[t0_g .. + n_text[g]), its candidates [c0_g, c0_g + n_cand[g]) of the batch. voice: [n_voices][1024], group g reads row voice_of[g]
// (tts_autoregressive_multi_voice; voice_of == nullptr: one voice for all). Nothing after ar_begin_groups depends on the voices.
//
// tts_hifigan_stream (one candidate, `hs` non-null): the same loop; after every hs->stride new codes the latent pass runs over the rows that are already
// final and the HiFi-GAN chunk path decodes the frames that became final, which go to the callback while the loop goes on sampling.
struct HfgStream {
  int stride;
  tts_audio_cb cb;
  void *user;
  const float *voice;
  int have = 0, emitted = 0;            // latent rows held (frozen once a chunk was decoded from them), frames handed to the callback
  std::vector<float> lat, pass, audio;  // the utterance's latent rows; one pass' output; one chunk's samples
  std::vector<int32_t> codes;           // the pass' input: 8192, the sampled codes, 83 beyond (never read: n_mel ends before)
};
// Latent rows [hs->have, L) from a pass over the first L rows (the earlier rows are kept as they were when their audio left: what the callback got stays the
// decode of the latents the call returns), then the frames [hs->emitted, upto) of an utterance of L rows so far to the callback.
static int stream_emit(tts_ctx *c, HfgStream *hs, const int32_t *codes502, int L, int upto, int is_last) {
  if (L > hs->have) {
    // The last pass is tts_autoregressive's, length and all. A pass over a prefix runs at least 32 rows (the rows past L read padding and are dropped: causal),
    // so that it takes the multi-row path (ar.hip run_layers: rows >= 32) that every utterance of 31 rows or more ends on — the exact-f32 GEMV path of shorter
    // passes sums in another order, and its split-K factor depends on the row count.
    const int n_mel = is_last ? std::min(502, L + 1) : std::max(L, 32), n_out = std::min(500, n_mel);
    hs->pass.resize((size_t)n_out * TTS_DMODEL);
    if (int rc = ar_latents_group(c, 0, codes502, n_mel, hs->pass.data())) return rc;
    hs->lat.resize((size_t)L * TTS_DMODEL);
    std::copy(hs->pass.begin() + (size_t)hs->have * TTS_DMODEL, hs->pass.begin() + (size_t)L * TTS_DMODEL, hs->lat.begin() + (size_t)hs->have * TTS_DMODEL);
    hs->have = L;
  }
  const int32_t rows = hs->have, f0 = hs->emitted, n = upto - hs->emitted;
  if (n < 1) return TTS_OK;
  hs->audio.resize((size_t)n * 256);
  if (int rc = hifigan_chunk(c, hs->lat.data(), &rows, 1, hs->voice, 1, nullptr, &f0, &n, hs->audio.data())) return rc;
  hs->emitted = upto;
  if (hs->cb(hs->user, hs->audio.data(), n * 256, is_last)) return fail(c, TTS_ERR_STATE, "tts_hifigan_stream: cancelled by the callback");
  return TTS_OK;
}

static int autoregressive_impl(tts_ctx *c, const int32_t *text_ids, const int *n_text, int G, const float *voice, int n_voices, const int *voice_of,
                               const int *n_cand, int max_steps, unsigned flags, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out,
                               HfgStream *hs = nullptr) {
  static const bool timing = getenv("TTS_TIMING") != nullptr; // developer aid: host-side breakdown of the stage on stderr
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_begin = now(), t_sample = 0, t_step = 0;
  if (!codes_out || !rows_out) return fail(c, TTS_ERR_ARG, "tts_autoregressive: null output");
  if (G < 1 || !n_text || !n_cand) return fail(c, TTS_ERR_ARG, "tts_autoregressive: bad argument");
  int B = 0, P_max = 0;
  for (int g = 0; g < G; g++) { B += n_cand[g] > 0 ? n_cand[g] : 0; P_max = std::max(P_max, n_text[g] + 2); }
  if (max_steps > 500) return fail(c, TTS_ERR_LIMIT, "max_steps %d exceeds the 500 codes apply_padding accepts", max_steps);
  // The stop schedule (tts_ar_set_stop_schedule: a bench / test device, not a reference feature) is checked BEFORE any device work, applies only to calls that pass
  // TTS_AR_MASK_STOP | TTS_AR_RETIRE (the combination it is documented for: a strict call is never truncated by a forgotten schedule) and says so on stderr once.
  const bool sched = !c->stop_schedule.empty() && (flags & TTS_AR_MASK_STOP) && (flags & TTS_AR_RETIRE);
  if (!c->stop_schedule.empty() && !sched) {
    static bool warned = false;
    if (!warned) { fprintf(stderr, "tts_autoregressive: a stop schedule is set but the call does not pass TTS_AR_MASK_STOP | TTS_AR_RETIRE: ignored\n"); warned = true; }
  }
  if (sched && (int)c->stop_schedule.size() != B) return fail(c, TTS_ERR_ARG, "tts_autoregressive: the stop schedule holds %d candidates, the call %d", (int)c->stop_schedule.size(), B);
  if (hs) c->stream_recaptures = 0;
  int rc = ar_begin_groups(c, text_ids, n_text, G, voice, n_voices, voice_of, n_cand, max_steps);
  if (rc) return rc;
  // the longest latent pass a streaming call can run (trim_latents keeps at most 9 rows past the codes), reserved once the call is known to be valid and
  // before the decode step's buffers are used
  if (hs && (rc = ar_stream_reserve(c, std::max(32, std::min(502, max_steps + 10))))) return rc;
  int captures0 = -1; // decode-step graphs captured when the loop's first step had run
  const int V = TTS_VOCAB_MEL;
  std::vector<float> logits0((size_t)B * V);
  const double t_after_begin = now();
  if ((rc = ar_prefill(c, logits0.data()))) return rc;
  float *logits = logits0.data(); // after the first step: the pinned buffer the decode graph copies into (no extra host copy)
  const double t_after_prefill = now();
  // mel_transformer_inputs_vector: [1 ... 1, 8192] per candidate at step 0 (5095-5105), afterwards
  // the previous samples (5208-5217). Several prompts: every row is padded to the longest prompt's P with more 1s — the penalty is applied once per
  // DISTINCT id (sample_one / sample_one_list skip repeated ids; the literal form recomputes l[id] from the unpenalised logit), so the padded row
  // penalises exactly what the group's own row does (tests/test_multi_prompt_cpu.py checks it on the sampler).
  const int P = P_max;
  std::vector<int32_t> ids((size_t)P * B, 1);
  for (int b = 0; b < B; b++) ids[(size_t)b * P + P - 1] = 8192;
  int ids_per_cand = P;
  std::vector<int32_t> samples(B);
  // Stop rule (ArStopBook, host_logic.cpp). Reference (strict, always for B == 1): the loop ends only in an iteration where ALL B samples are 8193
  // (main.cpp:5214-5222), a candidate's sequence freezes at its first 8193 (5210-5213); several prompts: that rule per group, and an ended group's rows
  // are fed 8193. TTS_AR_RETIRE (throughput mode): a candidate retires at its first 8193 — from then on its input token is forced to 8193
  // and its samples are ignored — the loop ends when every candidate has retired, and reaching max_steps pads and returns instead of failing.
  // The uniforms are consumed exactly as in strict mode (two per candidate and step, candidate order), so every
  // sequence is the one strict mode would have produced.
  const bool retire = (flags & TTS_AR_RETIRE) != 0;
  if ((rc = shard_check(c, B))) return rc;
  ArStopBook book;
  book.init(n_cand, G);
  std::vector<int32_t> next; // the samples of the coming iteration when the device-top-k step already produced them
  bool have_next = false;
  c->topk_fallbacks = 0;
  // Penalty scope 1 (option "ar_penalty_scope"; HF generate's repetition penalty as upstream tortoise-tts runs it): every id fed since ar_begin_groups plus 1 and
  // 8192. ar_step keeps that set per candidate (the bitmap its penalising prefilter reads); the full-row sampler gets it as an id list. At step 0 nothing has
  // been fed: the set is {1, 8192}, exactly the distinct ids of the prompt-shaped row above.
  const bool scope1 = c->ar_penalty_scope == 1;
  std::vector<std::vector<int32_t>> hist(scope1 ? B : 0);
  std::vector<int32_t> hist_one;
  int i = 0;
  for (;;) {
    double t0 = now();
    if (have_next) { samples = next; have_next = false; }
    else {
      if (flags & TTS_AR_MASK_STOP)
        for (int b = 0; b < B; b++) logits[(size_t)b * V + 8193] = -1e30f;
      if (scope1 && i > 0) {
        for (int b = 0; b < B; b++) ar_history_ids(c, b, hist[b]);
        sample_candidates(c, c->generator, logits, [&](int b, const int32_t *&p, int &n) { p = hist[b].data(); n = (int)hist[b].size(); }, B, samples.data());
      } else
        sample_candidates(c, c->generator, logits, ids.data(), ids_per_cand, B, samples.data());
      t_sample += now() - t0;
    }
    const bool all_ended = book.step(samples.data(), i, retire, sched ? c->stop_schedule.data() : nullptr);
    ids.assign(samples.begin(), samples.end());
    ids_per_cand = 1;
    i++;
    if (all_ended) break;
    if (i >= max_steps) {
      if ((flags & TTS_AR_MASK_STOP) || retire) break;
      return fail(c, TTS_ERR_LIMIT, "no stop token within %d steps", max_steps);
    }
    if (hs && i % hs->stride == 0) { // i codes so far, none of them the stop token (one candidate: the loop ends with it)
      const std::vector<int> &sq = book.seq[0];
      hs->codes.assign(502, 83);
      hs->codes[0] = 8192;
      std::copy(sq.begin(), sq.begin() + std::min<size_t>(sq.size(), 501), hs->codes.begin() + 1);
      const int L = stream_final_rows(hs->codes.data() + 1, (int)sq.size());
      const int upto = tts_diffusion_frames(L) - TTS_HFG_HALO_FRAMES;
      if (L > hs->have && upto > hs->emitted && (rc = stream_emit(c, hs, hs->codes.data(), L, upto, 0))) return rc;
    }
    if (captures0 < 0 && i > 1) captures0 = ar_graph_captures(c);
    t0 = now();
    if (!c->device_topk) {
      if ((rc = ar_step(c, samples.data(), i - 1, nullptr, 0))) return rc;
      logits = ar_host_logits(c);
      t_step += now() - t0;
      continue;
    }
    // device top-k: the step hands back each candidate's ~64..128 largest logits and the sampler runs on those (same uniforms, same ids)
    if ((rc = ar_step(c, samples.data(), i - 1, nullptr, (flags & TTS_AR_MASK_STOP) ? 2 : 1))) return rc;
    t_step += now() - t0;
    t0 = now();
    next.resize(B);
    const PenaltyIdsFn ids_of = [&](int b, const int32_t *&p, int &n) {
      if (scope1) { ar_history_ids(c, b, hist_one); p = hist_one.data(); n = (int)hist_one.size(); }
      else { p = ids.data() + b; n = 1; }
    };
    if (sample_candidates_list(c, c->generator, ar_host_lists(c), ids_of, scope1, B, next.data(), [&](int b) { return ar_fetch_logits_row(c, b); }, &c->topk_fallbacks,
                               book.retired.data()))
      return fail(c, TTS_ERR_HIP, "tts_autoregressive: fetching a logits row failed");
    t_sample += now() - t0;
    have_next = true;
  }
  const double t_after_loop = now();
  if (hs) c->stream_recaptures = captures0 < 0 ? 0 : ar_graph_captures(c) - captures0;
  if (steps_out) *steps_out = i;
  std::vector<std::vector<int>> &seq = book.seq;
  c->ar_stopped.assign(B, 0); // who was cut at max_steps (TTS_AR_RETIRE / TTS_AR_MASK_STOP): tts_ar_stop_status
  for (int b = 0; b < B; b++) c->ar_stopped[b] = (!seq[b].empty() && seq[b].back() == 8193) ? 1 : 0;
  std::vector<int> max_rows(G, 0);
  for (int g = 0; g < G; g++)
    for (int b = book.c0[g]; b < book.c0[g] + n_cand[g]; b++) {
      if (seq[b].size() > 500) seq[b].resize(500); // the reference asserts (main.cpp:4517)
      pad_codes(seq[b]);
      std::copy(seq[b].begin(), seq[b].end(), codes_out + (size_t)b * 502);
      rows_out[b] = trimmed_latent_rows(codes_out + (size_t)b * 502);
      max_rows[g] = std::max(max_rows[g], rows_out[b]);
    }
  if (hs) { // the remaining rows from tts_autoregressive's own pass, the remaining frames with is_last
    if (rows_out[0] < hs->have) return fail(c, TTS_ERR_STATE, "tts_hifigan_stream: %d rows were final, the utterance keeps %d", hs->have, rows_out[0]);
    if ((rc = stream_emit(c, hs, codes_out, rows_out[0], tts_diffusion_frames(rows_out[0]), 1))) return rc;
    if (latents_out) std::copy(hs->lat.begin(), hs->lat.end(), latents_out);
    return TTS_OK;
  }
  if (!latents_out) return TTS_OK;
  // latent pass over the mel prefix that trim_latents keeps (causal: rows beyond it cannot matter), per group over its own prompt and rows
  const double t_before_lat = now();
  size_t off = 0;
  for (int g = 0; g < G; g++) {
    const int n_mel = std::min(502, max_rows[g] + 1);
    const int n_out = std::min(500, n_mel);
    std::vector<float> lat((size_t)n_cand[g] * n_out * TTS_DMODEL);
    if ((rc = ar_latents_group(c, g, codes_out + (size_t)book.c0[g] * 502, n_mel, lat.data()))) return rc;
    for (int k = 0; k < n_cand[g]; k++) {
      const int b = book.c0[g] + k;
      std::copy(lat.begin() + (size_t)k * n_out * TTS_DMODEL, lat.begin() + ((size_t)k * n_out + rows_out[b]) * TTS_DMODEL, latents_out + off);
      off += (size_t)rows_out[b] * TTS_DMODEL;
    }
  }
  if (timing)
    fprintf(stderr, "[tts timing] AR: begin %.1f ms, prefill %.1f, loop %.1f (steps %.1f in %d, sampler %.1f), latents %.1f, total %.1f\n",
            t_after_begin - t_begin, t_after_prefill - t_after_begin, t_after_loop - t_after_prefill, t_step, i - 1, t_sample,
            now() - t_before_lat, now() - t_begin);
  return TTS_OK;
}

int tts_autoregressive(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice, int B, int max_steps,
                       unsigned flags, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_autoregressive");
  return guarded(c, [&] {
    return autoregressive_impl(c, text_ids, &n_text, 1, voice, 1, nullptr, &B, max_steps, flags, codes_out, rows_out, latents_out, steps_out);
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
    HfgStream hs{stride_codes, cb, user, voice};
    const int B = 1;
    return autoregressive_impl(c, text_ids, &n_text, 1, voice, 1, nullptr, &B, max_steps, flags, codes_out, rows_out, latents_out, steps_out, &hs);
  });
}

int tts_autoregressive_multi(tts_ctx *c, const int32_t *text_ids, const int32_t *n_text, int n_prompts, const float *voice, const int32_t *n_cand, int max_steps,
                             unsigned flags, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out) {
  NEED_CTX(c);
  NO_SESSION(c, "tts_autoregressive_multi");
  if (n_prompts < 1 || !n_text || !n_cand) return fail(c, TTS_ERR_ARG, "tts_autoregressive_multi: bad argument");
  return guarded(c, [&] {
    return autoregressive_impl(c, text_ids, n_text, n_prompts, voice, 1, nullptr, n_cand, max_steps, flags, codes_out, rows_out, latents_out, steps_out);
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
    return autoregressive_impl(c, text_ids, n_text, n_prompts, voices, n_voices, voice_of_prompt, n_cand, max_steps, flags, codes_out, rows_out, latents_out,
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
  delete c->session;
  c->session = nullptr;
  ar_session_close(c);
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
  return guarded(c, [&] {
    if (c->session) { delete c->session; c->session = nullptr; ar_session_close(c); }
    std::unique_ptr<ArSession> s(new ArSession());
    s->n_slots = n_slots; s->max_cand = max_cand; s->max_text = max_text; s->max_steps = max_steps; s->flags = flags;
    s->sp = c->ar_sp; s->scope = c->ar_penalty_scope; s->ar_weights = c->ar_weights; s->ggml_lut = c->ggml_lut; s->device_topk = c->device_topk;
    s->busy.assign((size_t)n_slots, 0);
    if (int rc = ar_session_open(c, n_slots, max_cand, max_text, max_steps, (flags & TTS_AR_ROW_CONTROLS) != 0)) return rc;
    c->topk_fallbacks = 0;
    c->session = s.release();
    return (int)TTS_OK;
  });
}

int tts_ar_session_room(const tts_ctx *c) {
  if (!c) return TTS_ERR_ARG;
  if (c->device < 0) return TTS_ERR_HIP;
  if (!c->session) return TTS_ERR_STATE;
  int best = 0, run = 0;
  for (uint8_t b : c->session->busy) { run = b ? 0 : run + 1; best = std::max(best, run); }
  return best;
}

int tts_ar_session_recaptures(const tts_ctx *c) {
  if (!c) return TTS_ERR_ARG;
  if (c->device < 0) return TTS_ERR_HIP;
  if (!c->session) return TTS_ERR_STATE;
  return ar_session_recaptures(c);
}

// What a request descriptor must satisfy in a session of max_cand candidates and max_steps steps, before any device work: the status, and in `why` the text.
// On TTS_OK sp / scope hold the request's controls as the sampler will read them.
static int request_check(const tts_ar_request *req, int max_cand, int max_steps, SamplerParams &sp, int &scope, std::string &why) {
  char buf[160];
  if (!req) { why = "null request"; return TTS_ERR_ARG; }
  if (req->struct_size < sizeof(tts_ar_request)) {
    snprintf(buf, sizeof buf, "struct_size %u, version 8 declares %zu bytes (set it to sizeof(tts_ar_request))", req->struct_size, sizeof(tts_ar_request));
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
  const double v[5] = {req->temperature, req->top_k, req->top_p, req->repetition_penalty, req->penalty_scope};
  for (int k = 0; k < 5; k++) {
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
  return request_check(req, max_cand, max_steps, sp, scope, why);
}

int tts_ar_request_init(tts_ctx *c, tts_ar_request *req) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_request_init");
  if (!req) return fail(c, TTS_ERR_ARG, "tts_ar_request_init: null request");
  if (req->struct_size < sizeof(tts_ar_request))
    return fail(c, TTS_ERR_ARG, "tts_ar_request_init: struct_size %u, version 8 declares %zu bytes (set it to sizeof(tts_ar_request) first)", req->struct_size,
                sizeof(tts_ar_request));
  const ArSession &s = *c->session;
  req->n_cand = 1; req->seed = 0; req->max_steps = 0; req->stop_at = nullptr;
  req->temperature = s.sp.temp; req->top_k = s.sp.top_k; req->top_p = s.sp.top_p; req->repetition_penalty = s.sp.penalty; req->penalty_scope = s.scope;
  return TTS_OK;
}

// tts_ar_session_admit and tts_ar_session_admit_ex (fn: the caller's name in the messages). sp / scope / max_steps: the request's, already checked.
static int session_admit(tts_ctx *c, const char *fn, const int32_t *text_ids, int n_text, const float *voice, int n_cand, uint32_t seed, const int32_t *stop_at,
                         const SamplerParams &sp, int scope, int max_steps) {
  ArSession &s = *c->session;
  // every argument before any device work
  if (!text_ids || !voice || n_text < 1 || n_cand < 1) return fail(c, TTS_ERR_ARG, "%s: bad argument (%d ids, %d candidates)", fn, n_text, n_cand);
  if (n_text > s.max_text) return fail(c, TTS_ERR_LIMIT, "%s: %d ids, the session was opened for %d", fn, n_text, s.max_text);
  if (n_cand > s.max_cand) return fail(c, TTS_ERR_LIMIT, "%s: %d candidates, the session was opened for %d", fn, n_cand, s.max_cand);
  for (int i = 0; i < n_text; i++)
    if (text_ids[i] < 0 || text_ids[i] >= 256) return fail(c, TTS_ERR_ARG, "text id %d out of range", text_ids[i]);
  for (int i = 0; i < TTS_DMODEL; i++)
    if (!std::isfinite(voice[i])) return fail(c, TTS_ERR_ARG, "%s: the voice holds a non-finite value", fn);
  if (stop_at)
    for (int b = 0; b < n_cand; b++)
      if (stop_at[b] < 1) return fail(c, TTS_ERR_ARG, "%s: candidate %d would stop before its first code", fn, b);
  const bool rows = (s.flags & TTS_AR_ROW_CONTROLS) != 0;
  if (!rows && !same_controls(sp, scope, s.sp, s.scope))
    return fail(c, TTS_ERR_STATE, "%s: the request's sampler controls differ from the session's (open the session with TTS_AR_ROW_CONTROLS)", fn);
  const int c0 = session_first_fit(s.busy.data(), s.n_slots, n_cand);
  if (c0 < 0) return fail(c, TTS_ERR_LIMIT, "%s: no run of %d free slots (collect a finished request first)", fn, n_cand);
  return guarded(c, [&] {
    SessionOptions opt(c, s);
    SamplerOptions ropt(c, sp, scope); // the request's controls: its table rows, its first codes
    const int V = TTS_VOCAB_MEL, P = n_text + 2;
    std::vector<float> row((size_t)V);
    if (int rc = ar_session_prompt(c, c0, n_cand, text_ids, n_text, voice, row.data())) return rc;
    if (rows) // every admission writes its rows: whatever the slots' last request left there (finished, cancelled or failed half-way) is gone
      if (int rc = ar_session_controls(c, c0, n_cand)) return rc;
    SessionRequest r;
    r.id = s.next_id; r.c0 = c0; r.n_cand = n_cand; r.n_text = n_text;
    r.sp = sp; r.scope = scope; r.max_steps = max_steps;
    r.gen.seed(seed);
    r.book.init(&n_cand, 1);
    if (stop_at) r.stop_at.assign(stop_at, stop_at + n_cand);
    // tts_autoregressive's iteration 0: every candidate samples from the prompt's logits under the prompt-shaped penalty row [1 ... 1, 8192]
    if (s.flags & TTS_AR_MASK_STOP) row[8193] = -1e30f;
    std::vector<float> logits0((size_t)n_cand * V);
    for (int b = 0; b < n_cand; b++) std::copy(row.begin(), row.end(), logits0.begin() + (size_t)b * V);
    std::vector<int32_t> ids((size_t)P * n_cand, 1);
    for (int b = 0; b < n_cand; b++) ids[(size_t)b * P + P - 1] = 8192;
    r.samples.resize(n_cand);
    sample_candidates(c, r.gen, logits0.data(), ids.data(), P, n_cand, r.samples.data());
    if (s.audio_stride && n_cand == 1) { // the prompt's rows of the latent pass, once, from the decode cache the prompt pass has just written
      if (int rc = ar_session_audio_prompt(c, c0, n_text)) return rc;
      r.audio = true;
      r.voice.assign(voice, voice + TTS_DMODEL);
    }
    std::fill(s.busy.begin() + c0, s.busy.begin() + c0 + n_cand, (uint8_t)1);
    SessionRequest &slot = s.reqs[r.id] = std::move(r);
    s.next_id++;
    session_advance(s, slot);
    if (slot.audio && slot.state != 0) // finished with its first code: no step will see it
      if (int rc = session_audio_pass(c, s, false)) return rc;
    return slot.id;
  });
}

int tts_ar_session_admit(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice, int n_cand, uint32_t seed, const int32_t *stop_at) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_admit");
  const ArSession &s = *c->session;
  return session_admit(c, "tts_ar_session_admit", text_ids, n_text, voice, n_cand, seed, stop_at, s.sp, s.scope, s.max_steps);
}

int tts_ar_session_admit_ex(tts_ctx *c, const int32_t *text_ids, int n_text, const float *voice, const tts_ar_request *req) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_admit_ex");
  const ArSession &s = *c->session;
  SamplerParams sp;
  int scope = 0;
  std::string why;
  if (int rc = request_check(req, s.max_cand, s.max_steps, sp, scope, why)) return fail(c, rc, "tts_ar_session_admit_ex: %s", why.c_str());
  return session_admit(c, "tts_ar_session_admit_ex", text_ids, n_text, voice, req->n_cand, req->seed, req->stop_at, sp, scope,
                       req->max_steps ? req->max_steps : s.max_steps);
}

int tts_ar_session_step(tts_ctx *c) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_step");
  ArSession &s = *c->session;
  return guarded(c, [&] {
    int n_live = 0;
    for (auto &kv : s.reqs) n_live += kv.second.state == 0;
    if (n_live == 0) return 0;
    SessionOptions opt(c, s);
    const int V = TTS_VOCAB_MEL;
    // An empty slot sits at position 0. A finished request's rows are parked at position n_text + 2, the first mel position that its latent pass recomputes
    // anyway: its prompt's K/V rows [0, n_text + 1) stay as the prompt pass wrote them until the request is collected, and the row reads written memory only.
    std::vector<int32_t> toks((size_t)s.n_slots, 8193), n_past((size_t)s.n_slots, 0), pos((size_t)s.n_slots, 0);
    std::vector<char> live((size_t)s.n_slots, 0);
    for (auto &kv : s.reqs) {
      const SessionRequest &r = kv.second;
      for (int b = 0; b < r.n_cand; b++) {
        const int k = r.c0 + b;
        if (r.state == 0) { toks[k] = r.samples[b]; n_past[k] = r.n_text + 2 + (r.i - 1); pos[k] = (r.i - 1) + 2; live[k] = 1; }
        else { n_past[k] = r.n_text + 2; pos[k] = 2; }
      }
    }
    const bool mask = (s.flags & TTS_AR_MASK_STOP) != 0;
    const int mode = s.device_topk ? (mask ? 2 : 1) : 0;
    if (int rc = ar_session_step(c, toks.data(), n_past.data(), pos.data(), live.data(), mode)) return rc;
    std::vector<std::vector<int32_t>> hist;
    std::vector<int32_t> hist_one, next;
    for (auto &kv : s.reqs) {
      SessionRequest &r = kv.second;
      if (r.state != 0) continue;
      SamplerOptions ropt(c, r.sp, r.scope); // the request's own controls: the uniform session's are the session's
      const bool scope1 = r.scope == 1;
      next.assign((size_t)r.n_cand, 0);
      if (mode == 0) { // the full rows, as tts_autoregressive with device_topk = 0
        float *logits = ar_host_logits(c) + (size_t)r.c0 * V;
        if (mask)
          for (int b = 0; b < r.n_cand; b++) logits[(size_t)b * V + 8193] = -1e30f;
        if (scope1) {
          hist.resize((size_t)r.n_cand);
          for (int b = 0; b < r.n_cand; b++) ar_history_ids(c, r.c0 + b, hist[b]);
          sample_candidates(c, r.gen, logits, [&](int b, const int32_t *&p, int &n) { p = hist[b].data(); n = (int)hist[b].size(); }, r.n_cand, next.data());
        } else
          sample_candidates(c, r.gen, logits, r.samples.data(), 1, r.n_cand, next.data());
      } else {
        const PenaltyIdsFn ids_of = [&](int b, const int32_t *&p, int &n) {
          if (scope1) { ar_history_ids(c, r.c0 + b, hist_one); p = hist_one.data(); n = (int)hist_one.size(); }
          else { p = r.samples.data() + b; n = 1; }
        };
        if (sample_candidates_list(c, r.gen, ar_host_lists(c) + (size_t)r.c0 * TTS_PF_WORDS, ids_of, scope1, r.n_cand, next.data(),
                                   [&](int b) { return ar_fetch_logits_row(c, r.c0 + b); }, &c->topk_fallbacks, r.book.retired.data()))
          return fail(c, TTS_ERR_HIP, "tts_ar_session_step: fetching a logits row failed");
      }
      r.samples = next;
      session_advance(s, r);
      n_live -= r.state != 0;
    }
    s.clock++;
    if (s.audio_stride)
      if (int rc = session_audio_pass(c, s, s.clock % s.audio_stride == 0)) return rc;
    return n_live;
  });
}

int tts_ar_session_finished(tts_ctx *c, int32_t *ids_out, int cap) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_finished");
  if (cap < 0 || (cap > 0 && !ids_out)) return fail(c, TTS_ERR_ARG, "tts_ar_session_finished: bad argument");
  const std::vector<int> &f = c->session->finished;
  for (int k = 0; k < (int)f.size() && k < cap; k++) ids_out[k] = f[k];
  return (int)f.size();
}

int tts_ar_session_collect(tts_ctx *c, int request, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out, int32_t *stopped_out) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_collect");
  ArSession &s = *c->session;
  if (!codes_out || !rows_out) return fail(c, TTS_ERR_ARG, "tts_ar_session_collect: null output");
  auto it = s.reqs.find(request);
  if (it == s.reqs.end()) return fail(c, TTS_ERR_ARG, "tts_ar_session_collect: no request %d", request);
  if (it->second.state == 0) return fail(c, TTS_ERR_STATE, "tts_ar_session_collect: request %d is still running", request);
  if (it->second.state == 2) {
    const int limit = it->second.max_steps;
    session_release(s, request);
    return fail(c, TTS_ERR_LIMIT, "no stop token within %d steps", limit);
  }
  return guarded(c, [&] {
    SessionOptions opt(c, s);
    SessionRequest &r = it->second;
    std::vector<std::vector<int>> seq = r.book.seq; // (the request stays collectable if the latent pass fails)
    int max_rows = 0;
    for (int b = 0; b < r.n_cand; b++) {
      if (stopped_out) stopped_out[b] = (!seq[b].empty() && seq[b].back() == 8193) ? 1 : 0;
      if (seq[b].size() > 500) seq[b].resize(500);
      pad_codes(seq[b]);
      std::copy(seq[b].begin(), seq[b].end(), codes_out + (size_t)b * 502);
      rows_out[b] = trimmed_latent_rows(codes_out + (size_t)b * 502);
      max_rows = std::max(max_rows, rows_out[b]);
    }
    if (steps_out) *steps_out = r.i;
    if (latents_out && r.audio && r.audio_done && r.have == rows_out[0]) { // the frozen rows: what the request's audio was decoded from
      std::copy(r.lat.begin(), r.lat.end(), latents_out);
    } else if (latents_out) { // the latent pass over the mel prefix that trim_latents keeps, as tts_autoregressive's
      const int n_mel = std::min(502, max_rows + 1), n_out = std::min(500, n_mel);
      std::vector<float> lat((size_t)r.n_cand * n_out * TTS_DMODEL);
      if (int rc = ar_session_latents(c, r.c0, r.n_text, codes_out, r.n_cand, n_mel, lat.data())) return rc;
      size_t off = 0;
      for (int b = 0; b < r.n_cand; b++) {
        std::copy(lat.begin() + (size_t)b * n_out * TTS_DMODEL, lat.begin() + ((size_t)b * n_out + rows_out[b]) * TTS_DMODEL, latents_out + off);
        off += (size_t)rows_out[b] * TTS_DMODEL;
      }
    }
    session_release(s, request);
    return (int)TTS_OK;
  });
}

int tts_ar_session_logits(tts_ctx *c, int request, float *logits_out) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_logits");
  if (!logits_out) return fail(c, TTS_ERR_ARG, "tts_ar_session_logits: null output");
  auto it = c->session->reqs.find(request);
  if (it == c->session->reqs.end()) return fail(c, TTS_ERR_ARG, "tts_ar_session_logits: no request %d", request);
  return guarded(c, [&] { return ar_session_logits(c, it->second.c0, it->second.n_cand, logits_out); });
}

int tts_ar_session_cancel(tts_ctx *c, int request) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_cancel");
  if (!c->session->reqs.count(request)) return fail(c, TTS_ERR_ARG, "tts_ar_session_cancel: no request %d", request);
  session_release(*c->session, request);
  return TTS_OK;
}

int tts_ar_session_enable_audio(tts_ctx *c, int stride_steps) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_enable_audio");
  ArSession &s = *c->session;
  if (stride_steps < 1) return fail(c, TTS_ERR_ARG, "tts_ar_session_enable_audio: stride_steps %d: >= 1", stride_steps);
  if (!c->hifigan) return fail(c, TTS_ERR_STATE, "tts_ar_session_enable_audio: tts_load_hifigan not called");
  if (s.next_id > 0) return fail(c, TTS_ERR_STATE, "tts_ar_session_enable_audio: the session has admitted a request (call it right after tts_ar_session_open)");
  if (s.ggml_lut) return fail(c, TTS_ERR_STATE, "tts_ar_session_enable_audio: the session runs under ggml_lut = 1, whose latent pass has no incremental form");
  return guarded(c, [&] {
    SessionOptions opt(c, s);
    if (int rc = ar_session_audio_enable(c, s.max_steps)) return rc;
    s.audio_stride = stride_steps;
    return (int)TTS_OK;
  });
}

int tts_ar_session_audio(tts_ctx *c, int request, float *out, int cap_samples, int32_t *is_last) {
  NEED_CTX(c);
  NEED_SESSION(c, "tts_ar_session_audio");
  ArSession &s = *c->session;
  if (!s.audio_stride) return fail(c, TTS_ERR_STATE, "tts_ar_session_audio: tts_ar_session_enable_audio not called");
  auto it = s.reqs.find(request);
  if (it == s.reqs.end()) return fail(c, TTS_ERR_ARG, "tts_ar_session_audio: no request %d", request);
  SessionRequest &r = it->second;
  if (!r.audio) return fail(c, TTS_ERR_ARG, "tts_ar_session_audio: request %d has %d candidates (several candidates are re-ranked and cannot stream)", request, r.n_cand);
  if (cap_samples < 0 || (cap_samples > 0 && !out) || !is_last) return fail(c, TTS_ERR_ARG, "tts_ar_session_audio: bad argument");
  return guarded(c, [&] {
    const size_t n = std::min(r.pcm.size(), (size_t)cap_samples) / 256 * 256; // whole frames
    std::copy(r.pcm.begin(), r.pcm.begin() + n, out);
    r.pcm.erase(r.pcm.begin(), r.pcm.begin() + n);
    *is_last = (r.audio_done && r.pcm.empty()) ? 1 : 0;
    return (int)n;
  });
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
  if (req->struct_size < sizeof(tts_diff_request))
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
  if (int rc = diff_request_check(req, diff_session_room(c), why)) return fail(c, rc, "tts_diff_session_admit: %s", why.c_str());
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
