// Host-only check of the AR request driver's pure rules (csrc/ar_rules.cpp: ArRun::advance, ar_finish_codes, ArStreamBook::due) under AddressSanitizer and
// UBSan: tools/ar_driver_rules_check.sh builds this file with ar_rules.cpp and host_logic.cpp into one program and runs it on the CPU. No device is touched.
// Sequences of 0, 1, 499, 500 and 501 codes, with and without a trailing 8193, with trailing 8139s (the literal apply_padding strips) and with runs of 83
// (what trim_latents cuts at).
#include "../tortoise.cpp_amd/csrc/common.h"

using namespace tts;

static int failures = 0;
#define EXPECT(cond)                                                             \
  do {                                                                           \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } \
  } while (0)

static std::vector<int> make_seq(int n, int fill, int tail, int n_tail, bool stop) {
  std::vector<int> s;
  for (int i = 0; i < n; i++) s.push_back(fill < 0 ? (i * 37 + 11) % 8192 : fill);
  for (int i = 0; i < n_tail && i < n; i++) s[n - 1 - i] = tail;
  if (stop && n > 0) s[n - 1] = 8193;
  return s;
}

// what a finished sequence becomes, and that the streaming book never declares more rows final than it keeps
static void check_sequence(const std::vector<int> &seq) {
  int32_t codes[502 + 1], rows = -1, stopped = -1;
  codes[502] = 0x5a5a5a5a; // a canary behind the row
  const int max_rows = ar_finish_codes(&seq, 1, codes, &rows, &stopped);
  EXPECT(codes[502] == 0x5a5a5a5a && codes[0] == 8192 && codes[501] == 8193);
  EXPECT(rows >= 0 && rows <= 500 && max_rows == rows);
  EXPECT(stopped == ((!seq.empty() && seq.back() == 8193) ? 1 : 0));
  const int n_codes = (int)seq.size() - stopped; // the codes in front of the stop token
  ArStreamBook book;
  std::vector<int32_t> c502;
  std::string why;
  int L = 0, upto = 0;
  for (int k = 1; k <= n_codes; k++) { // the loop asks after every code; a stop token ends the run before it asks
    const std::vector<int> prefix(seq.begin(), seq.begin() + k);
    const int due = book.due(prefix, false, c502, L, upto, why);
    EXPECT(due == 0 || due == 1);
    EXPECT(c502.size() == 502 && c502[0] == 8192 && L >= 0 && L <= 500);
    if (due == 1) { EXPECT(L > book.have && upto > book.emitted); book.have = L; book.emitted = upto; }
  }
  const int due = book.due(seq, true, c502, L, upto, why);
  EXPECT(L == rows && upto == tts_diffusion_frames(rows) && std::equal(c502.begin(), c502.end(), codes));
  if (!seq.empty() && seq.back() == 8139) EXPECT(due == 1 || (due == TTS_ERR_STATE && rows < book.have)); // apply_padding strips them: rows already heard may go
  else EXPECT(due == 1 && upto >= book.emitted);
  book.have = rows + 1; // more rows declared final than the utterance keeps: refused with the text the callers prefix
  EXPECT(book.due(seq, true, c502, L, upto, why) == TTS_ERR_STATE && why.find("rows were final, the utterance keeps") != std::string::npos);
}

// the decode loop's bookkeeping over a scripted run of two groups (candidates 0 and 1; candidate 2)
static void check_run(unsigned flags, int max_steps, const int32_t *stops, int want_state, int want_i) {
  const int n_cand[2] = {2, 1};
  ArRun run;
  run.init(n_cand, 2, SamplerParams(), 0, max_steps, flags, stops);
  EXPECT(run.samples.size() == 3 && run.state == 0 && run.i == 0);
  while (run.state == 0 && run.i < 600) {
    for (int b = 0; b < 3; b++) run.samples[b] = (run.i >= 3 + 2 * b) ? 8193 : 100 + run.i; // candidate b samples the stop token from iteration 3 + 2b on
    run.advance();
  }
  EXPECT(run.state == want_state && run.i == want_i);
  for (const std::vector<int> &s : run.book.seq) EXPECT((int)s.size() <= run.i);
}

int main() {
  for (int n : {0, 1, 2, 8, 9, 10, 31, 32, 499, 500, 501})
    for (int stop = 0; stop < 2; stop++) {
      check_sequence(make_seq(n, -1, 0, 0, stop));
      check_sequence(make_seq(n, -1, 8139, 3, stop)); // trailing 8139s (behind them the stop token, if any)
      check_sequence(make_seq(n, -1, 8139, n, false)); // nothing but 8139s
      check_sequence(make_seq(n, -1, 83, 8, stop));    // 8 trailing 83s: the padding completes the run
      check_sequence(make_seq(n, -1, 83, 9, stop));    // a run trim_latents cuts by itself
      check_sequence(make_seq(n, 83, 0, 0, stop));     // nothing but 83s
    }
  const int32_t stops[3] = {2, 9, 4};
  check_run(0, 500, nullptr, 1, 8);                                   // strict: group 0 ends at iteration 5 (both have stopped: 3 and 5), group 1 at 7
  check_run(0, 6, nullptr, 2, 6);                                     // strict, max_steps first: the error state
  check_run(TTS_AR_MASK_STOP, 6, nullptr, 1, 6);                      // ... a cut under either flag
  check_run(TTS_AR_RETIRE, 6, stops, 1, 6);                           // (a schedule without TTS_AR_MASK_STOP is not read)
  check_run(TTS_AR_MASK_STOP | TTS_AR_RETIRE, 500, stops, 1, 6);      // the schedule: candidates stop at 2, 5 (its own sample; the schedule says 9) and 4
  check_run(TTS_AR_MASK_STOP | TTS_AR_RETIRE, 1, nullptr, 1, 1);
  uint8_t busy[6] = {1, 0, 1, 0, 0, 1};
  EXPECT(session_first_fit(busy, 6, 1) == 1 && session_first_fit(busy, 6, 2) == 3 && session_first_fit(busy, 6, 3) == -1);
  printf("ar_driver rules: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
