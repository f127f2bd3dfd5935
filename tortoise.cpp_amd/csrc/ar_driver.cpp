// The AR request driver: autoregressive(), main.cpp:5042-5367, as ONE set of host rules (the sampler call of an iteration, an iteration's bookkeeping, what a
// finished sequence becomes, which audio is due) behind the three front ends: the single calls (tts_autoregressive*, tts_ar_step_sample), tts_hifigan_stream and
// the sessions (tts_ar_session_*). The rules that need no device are in ar_rules.cpp; the device side is ar.hip's; api.cpp checks arguments and forwards.
#include "common.h"
#include <chrono>
#include <cmath>
#include <cstdlib>

namespace tts {

// ---- the sampler call of one iteration ----
// What "the next tokens of candidates [c0, c0 + n) of the AR state's batch" are sampled from and under. Two uniforms of `gen` per candidate in candidate order
// whatever the fields say.
struct SampleCall {
  std::mt19937 &gen;
  SamplerParams sp;
  int scope = 0;
  bool mask_stop = false;        // TTS_AR_MASK_STOP: applied here to full rows; the step has applied it to the lists
  int c0 = 0, n = 0;
  float *rows = nullptr;         // the candidates' full logits rows [n][V], or null: the device prefilter's lists of the last step
  const int32_t *ids = nullptr;  // penalty ids [n][ids_per_cand]: the tokens of the last input, or iteration 0's prompt-shaped row [1 ... 1, 8192] (prompt_row)
  int ids_per_cand = 1;
  bool prompt_row = false;       // scope 1 takes the candidate's history instead of `ids` in every later iteration; at iteration 0 that set is {1, 8192}, the row's ids
  const char *retired = nullptr; // lists only: candidates that are not evaluated (out = 8193)
  int *fallbacks = nullptr;      // lists only: counts the candidates whose list could not decide and whose full row was fetched
  explicit SampleCall(std::mt19937 &g) : gen(g) {}
  SampleCall(std::mt19937 &g, const ArRun &run, int first_slot) // a later iteration of `run`
      : gen(g), sp(run.sp), scope(run.scope), mask_stop(run.mask_stop), c0(first_slot), n((int)run.samples.size()), ids(run.samples.data()),
        retired(run.book.retired.data()) {}
  void prompt(const int32_t *row_ids, int P) { ids = row_ids; ids_per_cand = P; prompt_row = true; } // iteration 0
};
// `out` [n] must not alias s.ids. fn: the caller's name in the message.
static int sample_next(tts_ctx *c, const char *fn, const SampleCall &s, int32_t *out) {
  const int V = TTS_VOCAB_MEL;
  const bool history = s.scope == 1 && !s.prompt_row;
  if (s.rows) {
    if (s.mask_stop)
      for (int b = 0; b < s.n; b++) s.rows[(size_t)b * V + 8193] = -1e30f;
    if (!history) { sample_candidates(c, s.gen, s.sp, s.rows, s.ids, s.ids_per_cand, s.n, out); return TTS_OK; }
    std::vector<std::vector<int32_t>> hist((size_t)s.n); // all of them up front: the sampler pool's threads ask
    for (int b = 0; b < s.n; b++) ar_history_ids(c, s.c0 + b, hist[b]);
    sample_candidates(c, s.gen, s.sp, s.rows, [&](int b, const int32_t *&p, int &k) { p = hist[b].data(); k = (int)hist[b].size(); }, s.n, out);
    return TTS_OK;
  }
  // Under scope 1 the lists hold penalised values (ar_step keeps the history set) and only the serial full-row fallback asks for ids: built on demand.
  // (One reference per closure: a std::function holds it in place, no allocation per request and step.)
  struct { tts_ctx *c; const SampleCall &s; bool history; std::vector<int32_t> hist; } a{c, s, history, {}};
  const PenaltyIdsFn ids_of = [&a](int b, const int32_t *&p, int &k) {
    if (a.history) { ar_history_ids(a.c, a.s.c0 + b, a.hist); p = a.hist.data(); k = (int)a.hist.size(); }
    else { p = a.s.ids + (size_t)b * a.s.ids_per_cand; k = a.s.ids_per_cand; }
  };
  // (typical sampling: the device penalises in either scope before it decides the set, so its lists hold penalised values)
  if (sample_candidates_list(c, s.gen, s.sp, ar_host_lists(c) + (size_t)s.c0 * TTS_PF_WORDS, ids_of, history || s.sp.typ_mass > 0, s.n, out,
                             [&a](int b) { return ar_fetch_logits_row(a.c, a.s.c0 + b); }, s.fallbacks, s.retired))
    return fail(c, TTS_ERR_HIP, "%s: fetching a logits row failed", fn);
  return TTS_OK;
}

// decode step + sampler in one call: the device prefilter's lists cross PCIe instead of the logits (ar.hip: sample_prefilter_kernel)
int ar_drv_step_sample(tts_ctx *c, const int32_t *prev, int i, unsigned flags, int32_t *samples_out) {
  if (ar_batch(c) < 1) return fail(c, TTS_ERR_STATE, "tts_ar_begin not called"); // before the shard check: with no AR state the batch is 0
  if (int rc = shard_check(c, ar_batch(c))) return rc;
  c->topk_fallbacks = 0;
  SampleCall s(c->generator);
  s.sp = c->ar_sp; s.scope = c->ar_penalty_scope; s.mask_stop = (flags & TTS_AR_MASK_STOP) != 0;
  s.n = ar_batch(c); s.ids = prev; s.fallbacks = &c->topk_fallbacks;
  if (int rc = ar_step(c, prev, i, nullptr, s.mask_stop ? 2 : 1)) return rc;
  return sample_next(c, "tts_ar_step_sample", s, samples_out);
}

// The latent pass over the mel prefix that trim_latents keeps (causal: rows beyond it cannot matter) of n candidates whose longest keeps max_rows rows:
// pass(n_mel, lat [n][n_out][1024]) runs it, each candidate's rows_of[b] rows are appended at `out`.
template <class Pass>
static int finish_latents(int n, int max_rows, const int32_t *rows_of, Pass pass, float *&out) {
  const int n_mel = std::min(502, max_rows + 1), n_out = std::min(500, n_mel);
  std::vector<float> lat((size_t)n * n_out * TTS_DMODEL);
  if (int rc = pass(n_mel, lat.data())) return rc;
  for (int b = 0; b < n; b++) {
    out = std::copy(lat.begin() + (size_t)b * n_out * TTS_DMODEL, lat.begin() + ((size_t)b * n_out + rows_of[b]) * TTS_DMODEL, out);
  }
  return TTS_OK;
}

// ---- the single calls: G groups of one ArRun over ar_step ----
// tts_hifigan_stream (one candidate): after every `stride` new codes the latent pass runs over the rows that are already final and the HiFi-GAN chunk path
// decodes the frames that became final, which go to the callback while the loop goes on sampling.
namespace {
struct HfgStream {
  int stride;
  tts_audio_cb cb;
  void *user;
  const float *voice;
  ArStreamBook book;
  std::vector<float> pass, audio; // one pass' output; one chunk's samples
  std::vector<int32_t> codes;     // the pass' input
};
} // namespace
// Latent rows [have, L) from a pass over the first L rows (the earlier rows are kept as they were when their audio left: what the callback got stays the
// decode of the latents the call returns), then the frames [emitted, upto) of an utterance of L rows so far to the callback.
static int stream_emit(tts_ctx *c, HfgStream &hs, int L, int upto, int is_last) {
  ArStreamBook &k = hs.book;
  if (L > k.have) {
    // The last pass is tts_autoregressive's, length and all. A pass over a prefix runs at least 32 rows (the rows past L read padding and are dropped: causal),
    // so that it takes the multi-row path (ar.hip run_layers: rows >= 32) that every utterance of 31 rows or more ends on — the exact-f32 GEMV path of shorter
    // passes sums in another order, and its split-K factor depends on the row count.
    const int n_mel = is_last ? std::min(502, L + 1) : std::max(L, 32), n_out = std::min(500, n_mel);
    hs.pass.resize((size_t)n_out * TTS_DMODEL);
    if (int rc = ar_latents_group(c, 0, hs.codes.data(), n_mel, hs.pass.data())) return rc;
    k.lat.resize((size_t)L * TTS_DMODEL);
    std::copy(hs.pass.begin() + (size_t)k.have * TTS_DMODEL, hs.pass.begin() + (size_t)L * TTS_DMODEL, k.lat.begin() + (size_t)k.have * TTS_DMODEL);
    k.have = L;
  }
  const int32_t rows = k.have, f0 = k.emitted, n = upto - k.emitted;
  if (n < 1) return TTS_OK;
  hs.audio.resize((size_t)n * 256);
  if (int rc = hifigan_chunk(c, k.lat.data(), &rows, 1, hs.voice, 1, nullptr, &f0, &n, hs.audio.data())) return rc;
  k.emitted = upto;
  if (hs.cb(hs.user, hs.audio.data(), n * 256, is_last)) return fail(c, TTS_ERR_STATE, "tts_hifigan_stream: cancelled by the callback");
  return TTS_OK;
}

// G prompt groups in one decode loop (tts_autoregressive: G = 1; tts_autoregressive_multi). Group g's prompt is text_ids[t0_g .. + n_text[g]), its candidates
// [c0_g, c0_g + n_cand[g]) of the batch. voice: [n_voices][1024], group g reads row voice_of[g] (tts_autoregressive_multi_voice; voice_of == nullptr: one voice
// for all). Nothing after ar_begin_groups depends on the voices.
int ar_drv_autoregressive(tts_ctx *c, const int32_t *text_ids, const int *n_text, int G, const float *voice, int n_voices, const int *voice_of, const int *n_cand,
                          int max_steps, unsigned flags, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out, int stride_codes,
                          tts_audio_cb cb, void *user) {
  static const bool timing = getenv("TTS_TIMING") != nullptr; // developer aid: host-side breakdown of the stage on stderr
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_begin = now(), t_sample = 0, t_step = 0;
  if (!codes_out || !rows_out) return fail(c, TTS_ERR_ARG, "tts_autoregressive: null output");
  if (G < 1 || !n_text || !n_cand) return fail(c, TTS_ERR_ARG, "tts_autoregressive: bad argument");
  int B = 0, P = 0; // P: the longest prompt's
  for (int g = 0; g < G; g++) { B += n_cand[g] > 0 ? n_cand[g] : 0; P = std::max(P, n_text[g] + 2); }
  if (max_steps > 500) return fail(c, TTS_ERR_LIMIT, "max_steps %d exceeds the 500 codes apply_padding accepts", max_steps);
  // The stop schedule (tts_ar_set_stop_schedule: a bench / test device, not a reference feature) is checked BEFORE any device work, applies only to calls that pass
  // TTS_AR_MASK_STOP | TTS_AR_RETIRE (the combination it is documented for) and says so on stderr once.
  const bool mask_stop = (flags & TTS_AR_MASK_STOP) != 0;
  const bool sched = !c->stop_schedule.empty() && mask_stop && (flags & TTS_AR_RETIRE);
  if (!c->stop_schedule.empty() && !sched) {
    static bool warned = false;
    if (!warned) { fprintf(stderr, "tts_autoregressive: a stop schedule is set but the call does not pass TTS_AR_MASK_STOP | TTS_AR_RETIRE: ignored\n"); warned = true; }
  }
  if (sched && (int)c->stop_schedule.size() != B) return fail(c, TTS_ERR_ARG, "tts_autoregressive: the stop schedule holds %d candidates, the call %d", (int)c->stop_schedule.size(), B);
  std::unique_ptr<HfgStream> hs;
  if (stride_codes > 0) { hs.reset(new HfgStream{stride_codes, cb, user, voice}); c->stream_recaptures = 0; }
  int rc = ar_begin_groups(c, text_ids, n_text, G, voice, n_voices, voice_of, n_cand, max_steps);
  if (rc) return rc;
  // the longest latent pass a streaming call can run (trim_latents keeps at most 9 rows past the codes), reserved once the call is known to be valid and
  // before the decode step's buffers are used
  if (hs && (rc = ar_stream_reserve(c, std::max(32, std::min(502, max_steps + 10))))) return rc;
  int captures0 = -1; // decode-step graphs captured when the loop's first step had run
  std::vector<float> logits0((size_t)B * TTS_VOCAB_MEL);
  const double t_after_begin = now();
  if ((rc = ar_prefill(c, logits0.data()))) return rc;
  const double t_after_prefill = now();
  // mel_transformer_inputs_vector: [1 ... 1, 8192] per candidate at step 0 (5095-5105), afterwards the previous samples (5208-5217). Several prompts: every
  // row is padded to the longest prompt's P with more 1s — the penalty is applied once per DISTINCT id (sample_one / sample_one_list skip repeated ids; the
  // literal form recomputes l[id] from the unpenalised logit), so the padded row penalises exactly what the group's own row does
  // (tests/test_multi_prompt_cpu.py checks it on the sampler).
  std::vector<int32_t> prompt_ids((size_t)P * B, 1), next((size_t)B);
  for (int b = 0; b < B; b++) prompt_ids[(size_t)b * P + P - 1] = 8192;
  if ((rc = shard_check(c, B))) return rc;
  ArRun run;
  run.init(n_cand, G, c->ar_sp, c->ar_penalty_scope, max_steps, flags, sched ? c->stop_schedule.data() : nullptr);
  c->topk_fallbacks = 0;
  // The uniforms are consumed the same way in every mode (two per candidate and step, candidate order), so every sequence is the one strict mode would produce.
  float *rows = logits0.data(); // iteration 0: the prompt pass' rows; later the pinned buffer the decode graph copies into, or null: the device top-k's lists
  for (;;) {
    double t0 = now();
    SampleCall s(c->generator, run, 0);
    s.rows = rows; s.fallbacks = &c->topk_fallbacks;
    if (run.i == 0) s.prompt(prompt_ids.data(), P);
    if ((rc = sample_next(c, "tts_autoregressive", s, next.data()))) return rc;
    run.samples.swap(next);
    t_sample += now() - t0;
    run.advance();
    if (run.state == 2) return fail(c, TTS_ERR_LIMIT, "no stop token within %d steps", max_steps);
    if (run.state) break;
    if (hs && run.i % hs->stride == 0) {
      std::string why;
      int L = 0, upto = 0;
      if (hs->book.due(run.book.seq[0], false, hs->codes, L, upto, why) == 1 && (rc = stream_emit(c, *hs, L, upto, 0))) return rc;
    }
    if (captures0 < 0 && run.i > 1) captures0 = ar_graph_captures(c);
    t0 = now();
    // device top-k: the step hands back each candidate's ~64..128 largest logits and the sampler runs on those (same uniforms, same ids)
    if ((rc = ar_step(c, run.samples.data(), run.i - 1, nullptr, !c->device_topk ? 0 : mask_stop ? 2 : 1))) return rc;
    rows = c->device_topk ? nullptr : ar_host_logits(c);
    t_step += now() - t0;
  }
  const double t_after_loop = now();
  if (hs) c->stream_recaptures = captures0 < 0 ? 0 : ar_graph_captures(c) - captures0;
  if (steps_out) *steps_out = run.i;
  const ArStopBook &book = run.book;
  c->ar_stopped.assign(B, 0); // who was cut at max_steps (TTS_AR_RETIRE / TTS_AR_MASK_STOP): tts_ar_stop_status
  std::vector<int> max_rows(G, 0);
  for (int g = 0; g < G; g++)
    max_rows[g] = ar_finish_codes(book.seq.data() + book.c0[g], n_cand[g], codes_out + (size_t)book.c0[g] * 502, rows_out + book.c0[g], c->ar_stopped.data() + book.c0[g]);
  if (hs) { // the remaining rows from tts_autoregressive's own pass, the remaining frames with is_last
    std::string why;
    int L = 0, upto = 0;
    if (hs->book.due(book.seq[0], true, hs->codes, L, upto, why) < 0) return fail(c, TTS_ERR_STATE, "tts_hifigan_stream: %s", why.c_str());
    if ((rc = stream_emit(c, *hs, L, upto, 1))) return rc;
    if (latents_out) std::copy(hs->book.lat.begin(), hs->book.lat.end(), latents_out);
    return TTS_OK;
  }
  if (!latents_out) return TTS_OK;
  const double t_before_lat = now();
  for (int g = 0; g < G; g++) // per group over its own prompt and rows
    if ((rc = finish_latents(n_cand[g], max_rows[g], rows_out + book.c0[g],
                             [&](int n_mel, float *lat) { return ar_latents_group(c, g, codes_out + (size_t)book.c0[g] * 502, n_mel, lat); }, latents_out)))
      return rc;
  if (timing)
    fprintf(stderr, "[tts timing] AR: begin %.1f ms, prefill %.1f, loop %.1f (steps %.1f in %d, sampler %.1f), latents %.1f, total %.1f\n",
            t_after_begin - t_begin, t_after_prefill - t_after_begin, t_after_loop - t_after_prefill, t_step, run.i - 1, t_sample,
            now() - t_before_lat, now() - t_begin);
  return TTS_OK;
}

// ---- the sessions: a map of ArRuns (one group each) over ar_session_step ----
struct SessionRequest {
  int id = 0, c0 = 0, n_cand = 0, n_text = 0;
  std::mt19937 gen; // seeded at admission: tts_autoregressive's stream after tts_seed(seed)
  ArRun run;        // state 2: tts_ar_session_collect returns TTS_ERR_LIMIT
  // Audio (a one-candidate request of a session with tts_ar_session_enable_audio)
  bool audio = false, audio_done = false; // audio_done: the request has finished and its last frames are in pcm
  ArStreamBook stream;
  std::vector<float> voice, pcm;          // the request's voice [1024]; the samples tts_ar_session_audio has not drained yet
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
  std::vector<int32_t> toks, n_past, pos, next; // tts_ar_session_step's inputs and one request's samples: kept between steps, no allocation per step
  std::vector<char> live;
};

namespace {
struct SessionOptions { // puts the session's options into the context for the length of one call (ar.hip reads them all over)
  tts_ctx *c;
  SamplerParams sp;
  int scope, w, lut, topk;
  SessionOptions(tts_ctx *ctx, const ArSession &s) : c(ctx), sp(ctx->ar_sp), scope(ctx->ar_penalty_scope), w(ctx->ar_weights), lut(ctx->ggml_lut), topk(ctx->device_topk) {
    c->ar_sp = s.sp; c->ar_penalty_scope = s.scope; c->ar_weights = s.ar_weights; c->ggml_lut = s.ggml_lut; c->device_topk = s.device_topk;
  }
  ~SessionOptions() { c->ar_sp = sp; c->ar_penalty_scope = scope; c->ar_weights = w; c->ggml_lut = lut; c->device_topk = topk; }
};
bool same_controls(const SamplerParams &a, int sa, const SamplerParams &b, int sb) {
  return a.temp == b.temp && a.top_k == b.top_k && a.top_p == b.top_p && a.penalty == b.penalty && a.typ_mass == b.typ_mass && sa == sb;
}
void session_release(ArSession &s, int id) {
  auto it = s.reqs.find(id);
  if (it == s.reqs.end()) return;
  std::fill(s.busy.begin() + it->second.c0, s.busy.begin() + it->second.c0 + it->second.n_cand, (uint8_t)0);
  s.finished.erase(std::remove(s.finished.begin(), s.finished.end(), id), s.finished.end());
  s.reqs.erase(it);
}
void session_advance(ArSession &s, SessionRequest &r) {
  r.run.advance();
  if (r.run.state) s.finished.push_back(r.id);
}
} // namespace

// One audio pass of a session: every audio request that has just finished, and with clock_due every running one, brings its new final latent rows to ONE
// incremental latent pass (ar_session_extend) and its new final frames to ONE ragged tts_hifigan_chunk call (what is due: ArStreamBook::due).
static int session_audio_pass(tts_ctx *c, ArSession &s, bool clock_due) {
  struct Due { SessionRequest *r; std::vector<int32_t> codes; int L, upto; bool last; };
  std::vector<Due> due;
  for (auto &kv : s.reqs) {
    SessionRequest &r = kv.second;
    if (!r.audio || r.audio_done || (r.run.state == 0 && !clock_due)) continue;
    if (r.run.state == 2) { r.audio_done = true; continue; } // a strict request that found no stop token: an error of its own, nothing more to hear
    Due d{&r, {}, 0, 0, r.run.state != 0};
    std::string why;
    const int k = r.stream.due(r.run.book.seq[0], d.last, d.codes, d.L, d.upto, why);
    if (k < 0) return fail(c, k, "tts_ar_session_step: request %d: %s", r.id, why.c_str());
    if (k) due.push_back(std::move(d));
  }
  if (due.empty()) return TTS_OK;
  std::vector<ArExtendItem> items;
  size_t new_rows = 0;
  for (Due &d : due)
    if (d.L > d.r->stream.have) { items.push_back(ArExtendItem{d.r->c0, d.r->n_text, d.r->stream.have, d.L, d.codes.data()}); new_rows += (size_t)(d.L - d.r->stream.have); }
  if (!items.empty()) {
    std::vector<float> rows(new_rows * TTS_DMODEL);
    if (int rc = ar_session_extend(c, items.data(), (int)items.size(), rows.data())) return rc;
    size_t off = 0;
    for (Due &d : due) {
      ArStreamBook &k = d.r->stream;
      if (d.L <= k.have) continue;
      const size_t n = (size_t)(d.L - k.have) * TTS_DMODEL;
      k.lat.insert(k.lat.end(), rows.begin() + off, rows.begin() + off + n);
      k.have = d.L;
      off += n;
    }
  }
  std::vector<float> lat, voices, audio;
  std::vector<int32_t> n_rows, voice_of, f0, nf;
  size_t frames = 0;
  for (Due &d : due) {
    const ArStreamBook &k = d.r->stream;
    if (d.upto <= k.emitted) continue; // (a finished request that keeps no row, or whose frames are all out)
    lat.insert(lat.end(), k.lat.begin(), k.lat.end());
    voices.insert(voices.end(), d.r->voice.begin(), d.r->voice.end());
    voice_of.push_back((int32_t)n_rows.size());
    n_rows.push_back(k.have); f0.push_back(k.emitted); nf.push_back(d.upto - k.emitted);
    frames += (size_t)(d.upto - k.emitted);
  }
  if (!n_rows.empty()) {
    audio.resize(frames * 256);
    if (int rc = hifigan_chunk(c, lat.data(), n_rows.data(), (int)n_rows.size(), voices.data(), (int)n_rows.size(), voice_of.data(), f0.data(), nf.data(), audio.data()))
      return rc;
    size_t off = 0;
    for (Due &d : due) {
      if (d.upto <= d.r->stream.emitted) continue;
      const size_t n = (size_t)(d.upto - d.r->stream.emitted) * 256;
      d.r->pcm.insert(d.r->pcm.end(), audio.begin() + off, audio.begin() + off + n);
      d.r->stream.emitted = d.upto;
      off += n;
    }
  }
  for (Due &d : due)
    if (d.last) d.r->audio_done = true;
  return TTS_OK;
}

void ar_drv_close(tts_ctx *c) {
  delete c->session;
  c->session = nullptr;
  ar_session_close(c);
}

int ar_drv_open(tts_ctx *c, int n_slots, int max_cand, int max_text, int max_steps, unsigned flags) {
  if (c->session) ar_drv_close(c);
  std::unique_ptr<ArSession> s(new ArSession());
  s->n_slots = n_slots; s->max_cand = max_cand; s->max_text = max_text; s->max_steps = max_steps; s->flags = flags;
  s->sp = c->ar_sp; s->scope = c->ar_penalty_scope; s->ar_weights = c->ar_weights; s->ggml_lut = c->ggml_lut; s->device_topk = c->device_topk;
  s->busy.assign((size_t)n_slots, 0);
  if (int rc = ar_session_open(c, n_slots, max_cand, max_text, max_steps, (flags & TTS_AR_ROW_CONTROLS) != 0)) return rc;
  c->topk_fallbacks = 0;
  c->session = s.release();
  return TTS_OK;
}

int ar_drv_room(const tts_ctx *c) {
  int best = 0, run = 0;
  for (uint8_t b : c->session->busy) { run = b ? 0 : run + 1; best = std::max(best, run); }
  return best;
}
void ar_drv_limits(const tts_ctx *c, int &max_cand, int &max_steps) { max_cand = c->session->max_cand; max_steps = c->session->max_steps; }
void ar_drv_defaults(const tts_ctx *c, tts_ar_request *req) {
  const ArSession &s = *c->session;
  req->temperature = s.sp.temp; req->top_k = s.sp.top_k; req->top_p = s.sp.top_p; req->repetition_penalty = s.sp.penalty; req->penalty_scope = s.scope;
  req->typical_mass = s.sp.typ_mass;
}

int ar_drv_admit(tts_ctx *c, const char *fn, const int32_t *text_ids, int n_text, const float *voice, int n_cand, uint32_t seed, const int32_t *stop_at,
                 const SamplerParams *sp_or_null, int scope_of_sp, int max_steps) {
  ArSession &s = *c->session;
  const SamplerParams &sp = sp_or_null ? *sp_or_null : s.sp;
  const int scope = sp_or_null ? scope_of_sp : s.scope;
  if (!max_steps) max_steps = s.max_steps;
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
  SessionOptions opt(c, s);
  const int V = TTS_VOCAB_MEL, P = n_text + 2;
  std::vector<float> logits0((size_t)n_cand * V);
  if (int rc = ar_session_prompt(c, c0, n_cand, text_ids, n_text, voice, logits0.data())) return rc;
  if (rows) // every admission writes its rows: whatever the slots' last request left there (finished, cancelled or failed half-way) is gone
    if (int rc = ar_session_controls(c, c0, n_cand, sp, scope)) return rc;
  SessionRequest r;
  r.id = s.next_id; r.c0 = c0; r.n_cand = n_cand; r.n_text = n_text;
  r.gen.seed(seed);
  r.run.init(&n_cand, 1, sp, scope, max_steps, s.flags, stop_at);
  // iteration 0: every candidate samples from the prompt's logits (one row, the candidates share it) under the prompt-shaped penalty row [1 ... 1, 8192]
  for (int b = 1; b < n_cand; b++) std::copy(logits0.begin(), logits0.begin() + V, logits0.begin() + (size_t)b * V);
  std::vector<int32_t> ids((size_t)P * n_cand, 1);
  for (int b = 0; b < n_cand; b++) ids[(size_t)b * P + P - 1] = 8192;
  SampleCall first(r.gen, r.run, c0);
  first.rows = logits0.data();
  first.prompt(ids.data(), P);
  if (int rc = sample_next(c, fn, first, r.run.samples.data())) return rc;
  if (s.audio_stride && n_cand == 1) { // the prompt's rows of the latent pass, once, from the decode cache the prompt pass has just written
    if (int rc = ar_session_audio_prompt(c, c0, n_text)) return rc;
    r.audio = true;
    r.voice.assign(voice, voice + TTS_DMODEL);
  }
  std::fill(s.busy.begin() + c0, s.busy.begin() + c0 + n_cand, (uint8_t)1);
  SessionRequest &slot = s.reqs[r.id] = std::move(r);
  s.next_id++;
  session_advance(s, slot);
  if (slot.audio && slot.run.state != 0) // finished with its first code: no step will see it
    if (int rc = session_audio_pass(c, s, false)) return rc;
  return slot.id;
}

int ar_drv_step(tts_ctx *c) {
  ArSession &s = *c->session;
  int n_live = 0;
  for (auto &kv : s.reqs) n_live += kv.second.run.state == 0;
  if (n_live == 0) return 0;
  SessionOptions opt(c, s);
  // An empty slot sits at position 0. A finished request's rows are parked at position n_text + 2, the first mel position that its latent pass recomputes
  // anyway: its prompt's K/V rows [0, n_text + 1) stay as the prompt pass wrote them until the request is collected, and the row reads written memory only.
  std::vector<int32_t> &toks = s.toks, &n_past = s.n_past, &pos = s.pos, &next = s.next;
  std::vector<char> &live = s.live;
  toks.assign((size_t)s.n_slots, 8193); n_past.assign((size_t)s.n_slots, 0); pos.assign((size_t)s.n_slots, 0); live.assign((size_t)s.n_slots, 0);
  for (auto &kv : s.reqs) {
    const SessionRequest &r = kv.second;
    for (int b = 0; b < r.n_cand; b++) {
      const int k = r.c0 + b;
      if (r.run.state == 0) { toks[k] = r.run.samples[b]; n_past[k] = r.n_text + 2 + (r.run.i - 1); pos[k] = (r.run.i - 1) + 2; live[k] = 1; }
      else { n_past[k] = r.n_text + 2; pos[k] = 2; }
    }
  }
  const bool mask = (s.flags & TTS_AR_MASK_STOP) != 0;
  const int mode = s.device_topk ? (mask ? 2 : 1) : 0;
  if (int rc = ar_session_step(c, toks.data(), n_past.data(), pos.data(), live.data(), mode)) return rc;
  for (auto &kv : s.reqs) {
    SessionRequest &r = kv.second;
    if (r.run.state != 0) continue;
    next.assign((size_t)r.n_cand, 0);
    // the request's own controls (a uniform session's are the session's); mode 0: the full rows, as tts_autoregressive with device_topk = 0
    SampleCall call(r.gen, r.run, r.c0);
    call.rows = mode == 0 ? ar_host_logits(c) + (size_t)r.c0 * TTS_VOCAB_MEL : nullptr;
    call.fallbacks = &c->topk_fallbacks;
    if (int rc = sample_next(c, "tts_ar_session_step", call, next.data())) return rc;
    r.run.samples.swap(next);
    session_advance(s, r);
    n_live -= r.run.state != 0;
  }
  s.clock++;
  if (s.audio_stride)
    if (int rc = session_audio_pass(c, s, s.clock % s.audio_stride == 0)) return rc;
  return n_live;
}

int ar_drv_finished(tts_ctx *c, int32_t *ids_out, int cap) {
  const std::vector<int> &f = c->session->finished;
  for (int k = 0; k < (int)f.size() && k < cap; k++) ids_out[k] = f[k];
  return (int)f.size();
}

int ar_drv_collect(tts_ctx *c, int request, int32_t *codes_out, int32_t *rows_out, float *latents_out, int32_t *steps_out, int32_t *stopped_out) {
  ArSession &s = *c->session;
  auto it = s.reqs.find(request);
  if (it == s.reqs.end()) return fail(c, TTS_ERR_ARG, "tts_ar_session_collect: no request %d", request);
  SessionRequest &r = it->second;
  if (r.run.state == 0) return fail(c, TTS_ERR_STATE, "tts_ar_session_collect: request %d is still running", request);
  if (r.run.state == 2) {
    const int limit = r.run.max_steps;
    session_release(s, request);
    return fail(c, TTS_ERR_LIMIT, "no stop token within %d steps", limit);
  }
  SessionOptions opt(c, s);
  const int max_rows = ar_finish_codes(r.run.book.seq.data(), r.n_cand, codes_out, rows_out, stopped_out); // (the request stays collectable if the latent pass fails)
  if (steps_out) *steps_out = r.run.i;
  if (latents_out && r.audio && r.audio_done && r.stream.have == rows_out[0]) { // the frozen rows: what the request's audio was decoded from
    std::copy(r.stream.lat.begin(), r.stream.lat.end(), latents_out);
  } else if (latents_out) {
    if (int rc = finish_latents(r.n_cand, max_rows, rows_out, [&](int n_mel, float *lat) { return ar_session_latents(c, r.c0, r.n_text, codes_out, r.n_cand, n_mel, lat); },
                                latents_out))
      return rc;
  }
  session_release(s, request);
  return TTS_OK;
}

int ar_drv_logits(tts_ctx *c, int request, float *logits_out) {
  auto it = c->session->reqs.find(request);
  if (it == c->session->reqs.end()) return fail(c, TTS_ERR_ARG, "tts_ar_session_logits: no request %d", request);
  return ar_session_logits(c, it->second.c0, it->second.n_cand, logits_out);
}

int ar_drv_cancel(tts_ctx *c, int request) {
  if (!c->session->reqs.count(request)) return fail(c, TTS_ERR_ARG, "tts_ar_session_cancel: no request %d", request);
  session_release(*c->session, request);
  return TTS_OK;
}

int ar_drv_enable_audio(tts_ctx *c, int stride_steps) {
  ArSession &s = *c->session;
  if (s.next_id > 0) return fail(c, TTS_ERR_STATE, "tts_ar_session_enable_audio: the session has admitted a request (call it right after tts_ar_session_open)");
  if (s.ggml_lut) return fail(c, TTS_ERR_STATE, "tts_ar_session_enable_audio: the session runs under ggml_lut = 1, whose latent pass has no incremental form");
  SessionOptions opt(c, s);
  if (int rc = ar_session_audio_enable(c, s.max_steps)) return rc;
  s.audio_stride = stride_steps;
  return TTS_OK;
}

int ar_drv_audio(tts_ctx *c, int request, float *out, int cap_samples, int32_t *is_last) {
  ArSession &s = *c->session;
  if (!s.audio_stride) return fail(c, TTS_ERR_STATE, "tts_ar_session_audio: tts_ar_session_enable_audio not called");
  auto it = s.reqs.find(request);
  if (it == s.reqs.end()) return fail(c, TTS_ERR_ARG, "tts_ar_session_audio: no request %d", request);
  SessionRequest &r = it->second;
  if (!r.audio) return fail(c, TTS_ERR_ARG, "tts_ar_session_audio: request %d has %d candidates (several candidates are re-ranked and cannot stream)", request, r.n_cand);
  if (cap_samples < 0 || (cap_samples > 0 && !out) || !is_last) return fail(c, TTS_ERR_ARG, "tts_ar_session_audio: bad argument");
  const size_t n = std::min(r.pcm.size(), (size_t)cap_samples) / 256 * 256; // whole frames
  std::copy(r.pcm.begin(), r.pcm.begin() + n, out);
  r.pcm.erase(r.pcm.begin(), r.pcm.begin() + n);
  *is_last = (r.audio_done && r.pcm.empty()) ? 1 : 0;
  return (int)n;
}

} // namespace tts
