// The AR request driver's rules that need no device (ar_driver.cpp applies them): an iteration's bookkeeping, what a finished sequence becomes, which audio of
// a streaming request is due, where a request fits. tools/ar_driver_rules_check.sh runs them under the sanitizers on the CPU.
#include "common.h"

namespace tts {

void ArRun::init(const int *n_cand, int G, const SamplerParams &p, int penalty_scope, int steps, unsigned flags, const int32_t *stops) {
  book.init(n_cand, G);
  const int B = (int)book.seq.size();
  samples.assign((size_t)B, 0);
  if (stops) stop_at.assign(stops, stops + B);
  else stop_at.clear();
  sp = p; scope = penalty_scope; max_steps = steps;
  mask_stop = (flags & TTS_AR_MASK_STOP) != 0; retire = (flags & TTS_AR_RETIRE) != 0;
  i = 0; state = 0;
}

// Stop rule (ArStopBook, host_logic.cpp). Reference (strict, always for B == 1): the loop ends only in an iteration where ALL B samples are 8193
// (main.cpp:5214-5222), a candidate's sequence freezes at its first 8193 (5210-5213); several prompts: that rule per group, and an ended group's rows
// are fed 8193. TTS_AR_RETIRE (throughput mode): a candidate retires at its first 8193 — from then on its input token is forced to 8193
// and its samples are ignored — the loop ends when every candidate has retired, and reaching max_steps pads and returns instead of failing (so does
// TTS_AR_MASK_STOP). The stop schedule applies only under TTS_AR_MASK_STOP | TTS_AR_RETIRE: a strict run is never truncated by a forgotten schedule.
void ArRun::advance() {
  const bool sched = !stop_at.empty() && mask_stop && retire;
  const bool all_ended = book.step(samples.data(), i, retire, sched ? stop_at.data() : nullptr);
  i++;
  if (all_ended) state = 1;
  else if (i >= max_steps) state = (mask_stop || retire) ? 1 : 2;
}

int ar_finish_codes(const std::vector<int> *seq, int n, int32_t *codes_out, int32_t *rows_out, int32_t *stopped) {
  int max_rows = 0;
  for (int b = 0; b < n; b++) {
    std::vector<int> sq = seq[b];
    if (stopped) stopped[b] = (!sq.empty() && sq.back() == 8193) ? 1 : 0;
    if (sq.size() > 500) sq.resize(500); // the reference asserts (main.cpp:4517)
    pad_codes(sq);
    std::copy(sq.begin(), sq.end(), codes_out + (size_t)b * 502);
    rows_out[b] = trimmed_latent_rows(codes_out + (size_t)b * 502);
    max_rows = std::max(max_rows, rows_out[b]);
  }
  return max_rows;
}

int ArStreamBook::due(const std::vector<int> &seq, bool last, std::vector<int32_t> &codes502, int &L, int &upto, std::string &why) const {
  codes502.assign(502, 83);
  if (last) { // what the call (tts_ar_session_collect) returns
    int32_t rows = 0;
    ar_finish_codes(&seq, 1, codes502.data(), &rows, nullptr);
    L = rows;
    upto = tts_diffusion_frames(L);
    if (L < have) {
      char buf[96];
      snprintf(buf, sizeof buf, "%d rows were final, the utterance keeps %d", have, L);
      why = buf;
      return TTS_ERR_STATE;
    }
    return 1;
  }
  // seq.size() codes so far, none of them the stop token (one candidate: the run ends with it): 8192, the codes, 83 beyond (never read: the pass ends before)
  codes502[0] = 8192;
  std::copy(seq.begin(), seq.begin() + std::min<size_t>(seq.size(), 501), codes502.begin() + 1);
  L = stream_final_rows(codes502.data() + 1, (int)seq.size());
  upto = tts_diffusion_frames(L) - TTS_HFG_HALO_FRAMES;
  return (L > have && upto > emitted) ? 1 : 0;
}

int session_first_fit(const uint8_t *busy, int n_slots, int n_cand) {
  int run = 0;
  for (int i = 0; i < n_slots; i++) {
    run = busy[i] ? 0 : run + 1;
    if (run == n_cand) return i - n_cand + 1;
  }
  return -1;
}

} // namespace tts
