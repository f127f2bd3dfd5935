// Host-side logic of the drop-in: weight container reader, tokenizer, sampler, diffusion schedule,
// sequence bookkeeping, WAV writer. Reference behaviour is cited per function (file:line in
// /root/reference); tests/test_host_parity.py checks each against the real reference code.
#include "common.h"
#include <unistd.h>
#include <iomanip>
#include <random>
#include <sstream>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <algorithm>
#include <cmath>
#include <fstream>
#include <functional>
#include <limits>
#include <regex>

namespace tts {

int fail(tts_ctx *ctx, int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) {
    static std::mutex mu; // load workers may fail at the same time (common.h: run_parallel)
    std::lock_guard<std::mutex> lk(mu);
    ctx->err = buf;
  }
  return code;
}

// ---------------------------------------------------------------------------------------------
// Reference-order normal noise in bulk. The reference draws every noise value with ONE call of std::normal_distribution<double>::operator()(std::mt19937 &)
// (main.cpp:4695-4701; 81 x 100 T values per utterance in diffusion(), 64 (T + 10) in vocoder()), ~38 ns each on the GPU box's host: 0.27 s for one utterance, more than
// the device needs for the whole sampling loop. libstdc++'s algorithm (bits/random.tcc; restated in oracle/orc_math.cpp and pinned there against the reference's compiled
// lines) is Marsaglia's polar method over generate_canonical<double, 53>:
//     u = (g() + g() * 2^32) / 2^64  (clamped below 1);   x = 2 u1 - 1, y = 2 u2 - 1, r2 = x x + y y, repeat while r2 > 1 or r2 == 0;
//     m = sqrt(-2 log(r2) / r2);   return y m now, x m at the next call;   every returned value v goes through v * stddev + mean.
// Only the generator calls and the accept test are sequential; log / sqrt / divide depend on one accepted pair each. rng_normal_fill runs the sequential part on the
// calling thread (the generator object itself: it ends in the state single draws leave it in) and the per-pair arithmetic on a few threads — the same operations in the
// same order per value, so every float equals the one operator() returns (tests/test_host_parity.py compares the two forms draw for draw, and the fast form against
// the reference's compiled lines). The distribution object's cached second value is read and written through its stream operators (the library's own state interface).
// ---------------------------------------------------------------------------------------------
namespace {
// (the reference's build has no fused multiply-add: contraction is switched off in every function below that multiplies and adds)
inline double canonical53(std::mt19937 &g) {
#pragma clang fp contract(off)
  const double lo = (double)g();
  const double hi = (double)g();
  double ret = (lo + hi * 4294967296.0) / 18446744073709551616.0;
  if (ret >= 1.0) ret = std::nextafter(1.0, 0.0);
  return ret;
}
struct PolarPair { double x, y, r2; };
inline void polar_finish(const PolarPair &p, double &first, double &second) {
#pragma clang fp contract(off)
  const double m = std::sqrt(-2 * std::log(p.r2) / p.r2);
  first = p.y * m;
  second = p.x * m;
}
inline float as_returned(double v) {
#pragma clang fp contract(off)
  return (float)(v * 1.0 + 0.0);
} // operator() ends with ret * stddev + mean (turns -0 into +0, like the original)
bool normal_saved(const std::normal_distribution<double> &d, double &saved) {
  std::ostringstream os;
  os << d; // "mean stddev saved_available [saved]" at max_digits10
  std::istringstream is(os.str());
  double mean = 0, sd = 0;
  int avail = 0;
  is >> mean >> sd >> avail;
  if (avail) is >> saved;
  return avail != 0;
}
void normal_set_saved(std::normal_distribution<double> &d, bool avail, double saved) {
  if (!avail) { d.reset(); return; }
  std::ostringstream os;
  os.precision(std::numeric_limits<double>::max_digits10);
  os << std::scientific << d.mean() << ' ' << d.stddev() << ' ' << 1 << ' ' << saved;
  std::istringstream is(os.str());
  is >> d;
}
} // namespace

void rng_normal_fill(tts_ctx *ctx, float *dst, int64_t n) {
#pragma clang fp contract(off)
  if (n <= 0) return;
  std::normal_distribution<double> &nd = ctx->normal_distribution;
  if (!ctx->rng_fast_normal || n < 4096 || nd.mean() != 0.0 || nd.stddev() != 1.0) {
    for (int64_t i = 0; i < n; i++) dst[i] = nd(ctx->generator);
    return;
  }
  // (nothing has touched the generator yet: if the pair buffer cannot be had, the single-draw form does the whole job)
  std::vector<PolarPair> pp;
  try {
    pp.resize((size_t)(n + 1) / 2);
  } catch (...) {
    for (int64_t i = 0; i < n; i++) dst[i] = nd(ctx->generator);
    return;
  }
  int64_t at = 0;
  double saved = 0;
  if (normal_saved(nd, saved)) dst[at++] = as_returned(saved); // the cached second value of an earlier pair comes first
  const int64_t left = n - at, pairs = (left + 1) / 2;
  std::mt19937 &g = ctx->generator;
  for (int64_t i = 0; i < pairs; i++) { // the sequential part: generator calls and the accept test
    double x, y, r2;
    do {
      x = 2.0 * canonical53(g) - 1.0;
      y = 2.0 * canonical53(g) - 1.0;
      r2 = x * x + y * y;
    } while (r2 > 1.0 || r2 == 0.0);
    pp[(size_t)i] = PolarPair{x, y, r2};
  }
  float *out = dst + at;
  double last_second = 0;
  auto finish = [&](int64_t a, int64_t b) {
#pragma clang loop vectorize(disable) // scalar libm log / sqrt, as in the original
    for (int64_t i = a; i < b; i++) {
      double v0, v1;
      polar_finish(pp[(size_t)i], v0, v1);
      out[2 * i] = as_returned(v0);
      if (2 * i + 1 < left) out[2 * i + 1] = as_returned(v1);
      else last_second = v1; // only the last pair of an odd count gets here (one thread)
    }
  };
  const int nt = (int)std::min<int64_t>(std::min(8u, std::max(1u, std::thread::hardware_concurrency())), pairs / 8192);
  if (nt <= 1) finish(0, pairs);
  else {
    std::vector<std::thread> th;
    int started = 1; // ranges [pairs t / nt, pairs (t + 1) / nt): range 0 is this thread's; a thread that cannot be created leaves its range (and the rest) to this one
    try {
      th.reserve((size_t)nt);
      for (; started < nt; started++) th.emplace_back(finish, pairs * started / nt, pairs * (started + 1) / nt);
    } catch (...) {
    }
    finish(0, pairs / nt);
    if (started < nt) finish(pairs * started / nt, pairs);
    for (auto &t : th) t.join();
  }
  normal_set_saved(nd, (left & 1) != 0, last_second);
}

// ---------------------------------------------------------------------------------------------
// Weight container. Reference loaders: main.cpp:811-888 (AR), 1545-1625 (diffusion), 1932-2012
// (vocoder): u32 magic 'ggml', then {i32 n_dims, i32 name_len, i32 ttype, i32 ne[n_dims], name,
// data} until EOF. Only F32 (ttype 0) occurs in the published files.
// ---------------------------------------------------------------------------------------------
WeightFile::~WeightFile() { if (fd >= 0) close(fd); }
bool WeightFile::read_payload(const HostTensor &ht, void *dst) const {
  if (fd < 0 || ht.file_off < 0) return false;
  char *p = (char *)dst;
  size_t left = (size_t)ht.nelem() * sizeof(float);
  long long off = ht.file_off;
  while (left > 0) {
    const ssize_t g = pread(fd, p, left, (off_t)off);
    if (g <= 0) return false;
    p += g; off += g; left -= (size_t)g;
  }
  return true;
}

int read_weight_file(const char *path, WeightFile &out, std::string &err, size_t lazy_from) {
  // Two passes (round 6): the record headers are walked with seeks, then the tensor payloads (1.6 GB for the AR model) are read by a few threads with pread() —
  // the single fread() pass of rounds 1-5 spent as long zero-filling and copying as the page cache took to deliver.
  FILE *f = fopen(path, "rb");
  if (!f) { err = std::string("failed to open '") + path + "'"; return TTS_ERR_IO; }
  fseeko(f, 0, SEEK_END);
  const long long file_size = ftello(f);
  fseeko(f, 0, SEEK_SET);
  uint32_t magic = 0;
  if (fread(&magic, 4, 1, f) != 1 || magic != 0x67676d6cu) {
    fclose(f);
    err = std::string("invalid model file '") + path + "' (bad magic)";
    return TTS_ERR_FORMAT;
  }
  struct Pending { HostTensor *t; long long off; std::string name; };
  std::vector<Pending> pend;
  for (;;) {
    int32_t hdr[3];
    size_t got = fread(hdr, 4, 3, f);
    if (got == 0) break; // clean EOF
    if (got != 3) { fclose(f); err = "truncated record header"; return TTS_ERR_IO; }
    int n_dims = hdr[0], name_len = hdr[1], ttype = hdr[2];
    if (n_dims < 1 || n_dims > 4 || name_len < 1 || name_len > 1024) {
      fclose(f); err = "corrupt record header"; return TTS_ERR_FORMAT;
    }
    if (ttype != 0) { fclose(f); err = "unsupported tensor type (only F32)"; return TTS_ERR_FORMAT; }
    HostTensor t;
    t.n_dims = n_dims;
    for (int i = 0; i < n_dims; i++) {
      int32_t v;
      if (fread(&v, 4, 1, f) != 1 || v < 1) { fclose(f); err = "corrupt shape"; return TTS_ERR_FORMAT; }
      t.ne[i] = v;
    }
    std::string name(name_len, '\0');
    if (fread(&name[0], 1, name_len, f) != (size_t)name_len) { fclose(f); err = "truncated name"; return TTS_ERR_IO; }
    // a corrupt shape must not turn into a giant allocation (no exception may cross the C ABI)
    unsigned long long want = 4;
    for (int i = 0; i < n_dims; i++) {
      want *= (unsigned long long)t.ne[i];
      if (want > (unsigned long long)file_size) break;
    }
    const long long off = ftello(f);
    if (want > (unsigned long long)(file_size - off)) { fclose(f); err = "tensor '" + name + "' truncated"; return TTS_ERR_IO; }
    if (fseeko(f, (off_t)want, SEEK_CUR) != 0) { fclose(f); err = "tensor '" + name + "' truncated"; return TTS_ERR_IO; }
    t.file_off = off;
    auto ins = out.t.emplace(name, std::move(t)); // a repeated name keeps its first record, as the single-pass reader did
    if (ins.second && want < (unsigned long long)lazy_from) pend.push_back(Pending{&ins.first->second, off, std::move(name)});
    else if (ins.second && out.fd < 0) out.fd = dup(fileno(f));
  }
  const int fd = fileno(f);
  const int n = (int)pend.size();
  int nt = (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  nt = std::min(nt, std::max(1, n));
  std::atomic<int> next{0}, bad{-1}, oom{0};
  auto work = [&]() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n || bad.load() >= 0 || oom.load()) break;
      Pending &p = pend[i];
      try {
        p.t->data.resize((size_t)p.t->nelem());
      } catch (...) { oom.store(1); break; }
      char *dst = (char *)p.t->data.data();
      size_t left = p.t->data.size() * sizeof(float);
      long long off = p.off;
      while (left > 0) {
        const ssize_t g = pread(fd, dst, left, (off_t)off);
        if (g <= 0) { int z = -1; bad.compare_exchange_strong(z, i); break; }
        dst += g; off += g; left -= (size_t)g;
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  fclose(f);
  if (oom.load()) { err = "out of host memory"; return TTS_ERR_LIMIT; }
  if (bad.load() >= 0) { err = "tensor '" + pend[bad.load()].name + "' truncated"; return TTS_ERR_IO; }
  return TTS_OK;
}

// ---------------------------------------------------------------------------------------------
// Tokenizer. The reference scrapes tokenizer.json with a character state machine rather than a
// JSON parser (common.cpp:166-255) and the resulting map — quirks included, e.g. the first key of
// every nested object is swallowed — *is* the vocabulary, so the same machine is restated here.
// ---------------------------------------------------------------------------------------------
static void subst(std::string &s, const char *from, const char *to) {
  const size_t fl = strlen(from), tl = strlen(to);
  for (size_t p = s.find(from); p != std::string::npos; p = s.find(from, p + tl)) s.replace(p, fl, to);
}

bool Tokenizer::load(const char *path) {
  std::ifstream in(path);
  if (!in) return false;
  const std::string js((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  vocab.clear();
  if (js.empty() || js[0] != '{') return true;
  enum { OUTSIDE, IN_KEY, IN_STRVAL } st = OUTSIDE;
  std::string key, val;
  const int n = (int)js.size();
  auto commit = [&]() {
    subst(key, "\\u0120", " ");
    subst(key, "\\u010a", "\n");
    subst(key, "\\\"", "\"");
    try { vocab[key] = std::stoi(val); } catch (...) { /* non-integer value: ignored */ }
    key.clear();
    val.clear();
    st = OUTSIDE;
  };
  for (int i = 1; i < n; ++i) {
    const char ch = js[i];
    if (st == OUTSIDE) {
      if (ch == '"') st = IN_KEY; // everything else between tokens is skipped
      continue;
    }
    std::string &cur = (st == IN_KEY) ? key : val;
    if (ch == '\\' && i + 1 < n) { // escapes are kept verbatim
      cur += ch;
      cur += js[++i];
      continue;
    }
    if (ch != '"') { cur += ch; continue; }
    if (st == IN_STRVAL) { commit(); continue; }
    // closing quote of a key: expect [spaces] ':' [spaces] value. Every scan is bounded: a truncated or malformed file
    // is a load failure (status + last_error), never a read past the buffer.
    ++i;
    while (i < n && js[i] == ' ') ++i;
    ++i;
    while (i < n && js[i] == ' ') ++i;
    if (i >= n) return false;
    if (js[i] == '"') { st = IN_STRVAL; continue; }
    while (i < n && js[i] != ',' && js[i] != '}') val += js[i++];
    if (i >= n) return false; // value runs into the end of the file
    commit();
  }
  return st == OUTSIDE; // a key or string value still open at EOF: truncated file
}

// gpt_split_words + greedy longest match (common.cpp:268-339); main.cpp:6559-6567 wraps the
// result with 255 ... 0 after replacing " " by "[SPACE]".
std::vector<int> Tokenizer::encode(const std::string &message) const {
  std::string text = message;
  subst(text, " ", "[SPACE]");
  static const std::regex word_re(
      R"(\[SPACE\]|\[UNK\]|\[STOP\]|'s|'t|'re|'ve|'m|'ll|'d| ?[[:alpha:]]+| ?[[:digit:]]+| ?[^\s\[\][:alpha:][:digit:]]+|\s+(?!\S)|\s+)");
  std::vector<int> ids{255};
  std::smatch m;
  while (std::regex_search(text, m, word_re)) {
    const std::string word = m.str(0);
    size_t i = 0;
    while (i < word.size()) {
      size_t len = word.size() - i;
      for (; len > 0; --len) {
        auto it = vocab.find(word.substr(i, len));
        if (it != vocab.end()) { ids.push_back(it->second); break; }
      }
      if (len == 0) {
        fprintf(stderr, "gpt_tokenize: unknown token '%s'\n", word.substr(i, 1).c_str());
        len = 1;
      }
      i += len;
    }
    text = m.suffix();
  }
  ids.push_back(0);
  return ids;
}

// ---------------------------------------------------------------------------------------------
// Sampler: process_logits_and_sample (main.cpp:4753-4806) and helpers (4562-4720).
// The reference sorts all 8194 logits three times per candidate; here only the top-k survivors
// are processed, in the same float operation order, so the sampled ids and the RNG consumption
// (two uniforms per candidate, the second used) are identical. Ties among survivors fall back to
// the literal formulation so std::sort's tie order is inherited rather than re-invented.
// ---------------------------------------------------------------------------------------------
static inline float exp_like_reference(float v) { return (float)::exp((double)v); } // exp(float) -> ::exp(double)

static int multinomial_literal(std::vector<float> &l, float sample, double top_p_cut) {
  const int V = (int)l.size();
  const float LOWEST = std::numeric_limits<float>::lowest();
  std::vector<std::pair<float, int>> pairs(V);
  for (int i = 0; i < V; i++) pairs[i] = {l[i], i};
  std::sort(pairs.begin(), pairs.end(),
            [](const std::pair<float, int> &a, const std::pair<float, int> &b) { return a.first < b.first; });
  std::vector<float> sl(V);
  float sum = 0;
  for (int i = 0; i < V; i++) { sl[i] = exp_like_reference(pairs[i].first); sum += sl[i]; }
  for (int i = 0; i < V; i++) sl[i] /= sum;
  for (int i = 1; i < V; i++) sl[i] += sl[i - 1];
  for (int i = 0; i < V - 1; i++)
    if (sl[i] <= top_p_cut) l[pairs[i].second] = LOWEST; // float against double, as the reference's `<= 0.2`
  sum = 0;
  for (int i = 0; i < V; i++) { l[i] = exp_like_reference(l[i]); sum += l[i]; }
  float cum = 0;
  for (int i = 0; i < V; i++) {
    cum += l[i] / sum;
    if (cum >= sample) return i;
  }
  return V - 1;
}

// ---------------------------------------------------------------------------------------------
// Locally typical sampling (option "ar_typical_mass"; Meister et al. 2022, as HF's TypicalLogitsWarper states it and upstream tortoise-tts' typical_sampling /
// typical_mass hands it to generate). THE definition, on the penalised float row x and in double throughout: m = max x; e_i = exp(x_i - m); Z = sum e_i in index
// order; ln p_i = (x_i - m) - ln Z; p_i = exp(ln p_i); H = -sum p_i ln p_i (terms with p_i = 0 skipped); d_i = |-ln p_i - H|; stable ascending sort by d; c_j =
// the cumulative p in that order; j* = the first j with c_j >= mass (V - 1 if none); the members are {i : d_i <= d_(j*)}: ties at the cut survive, the smallest d
// is always kept. Every other statement of the stage (sample_one's engine path, the device body in ar.hip, typical_keep_device_rule) is held to this one.
// ---------------------------------------------------------------------------------------------
int typical_keep(const float *row, double mass, char *keep) {
#pragma clang fp contract(off)
  const int V = TTS_VOCAB_MEL;
  thread_local std::vector<double> lnp, pr, d;
  thread_local std::vector<int> ord;
  lnp.resize(V); pr.resize(V); d.resize(V); ord.resize(V);
  double m = (double)row[0];
  for (int i = 1; i < V; i++) m = std::max(m, (double)row[i]);
  double Z = 0;
  for (int i = 0; i < V; i++) Z += std::exp((double)row[i] - m);
  const double lnZ = std::log(Z);
  double H = 0;
  for (int i = 0; i < V; i++) {
    lnp[i] = ((double)row[i] - m) - lnZ;
    pr[i] = std::exp(lnp[i]);
    if (pr[i] != 0) H -= pr[i] * lnp[i];
  }
  for (int i = 0; i < V; i++) { d[i] = std::fabs(-lnp[i] - H); ord[i] = i; }
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return d[a] < d[b]; });
  double c = 0;
  int js = V - 1;
  for (int j = 0; j < V; j++) {
    c += pr[ord[j]];
    if (c >= mass) { js = j; break; }
  }
  const double cut = d[ord[js]];
  int n = 0;
  for (int i = 0; i < V; i++) { keep[i] = d[i] <= cut; n += keep[i]; }
  return n;
}

// The set as the device body decides it (ar.hip: typical_members; the bounds are derived there and in DESIGN.md "What pins typical sampling"). With a = m - x >= 0
// the distance is d_i = |a_i - t|, t = sum a_i e_i / Z = H - ln Z (ln Z cancels), so one scalar orders the row. theta = the smallest d whose inclusive mass
// M(theta) = sum {p_i : d_i <= theta} reaches `mass`. The set {d <= theta} is the literal's when
//   - no other d lies within 2 E of theta, E = TTS_TYP_TOL_D + TTS_TYP_TOL_REL (t + theta) >= |d - d_literal| (elements AT theta must share one logit value: equal
//     logits have equal literal distances, and ties survive the literal's cut);
//   - M(theta) >= mass + TTS_TYP_TOL_M and the mass strictly below theta is < mass - TTS_TYP_TOL_M (TTS_TYP_TOL_M >= |M - c_literal|).
// Otherwise -1: the caller takes the full row and the literal. The sums here run in another order than the device's; both stay inside the same bounds.
int typical_keep_device_rule(const float *row, double mass, char *keep) {
#pragma clang fp contract(off)
  const int V = TTS_VOCAB_MEL;
  std::vector<double> e(V), d(V);
  std::vector<int> ord(V);
  float mf = row[0];
  for (int i = 1; i < V; i++) mf = std::max(mf, row[i]);
  const double m = (double)mf;
  double Z = 0, S = 0;
  for (int i = 0; i < V; i++) { e[i] = std::exp((double)row[i] - m); Z += e[i]; S += (m - (double)row[i]) * e[i]; }
  if (!(Z > 0) || !std::isfinite(Z) || !std::isfinite(S)) return -1;
  const double t = S / Z;
  for (int i = 0; i < V; i++) { d[i] = std::fabs((m - (double)row[i]) - t); ord[i] = i; }
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return d[a] < d[b]; });
  double below = 0;
  for (int j = 0; j < V;) {
    int k = j;
    double at = 0;
    while (k < V && d[ord[k]] == d[ord[j]]) at += e[ord[k++]] / Z;
    const double incl = below + at;
    if (incl >= mass) {
      const double theta = d[ord[j]], E2 = 2.0 * (TTS_TYP_TOL_D + TTS_TYP_TOL_REL * (t + theta));
      if (!(incl >= mass + TTS_TYP_TOL_M) || !(below < mass - TTS_TYP_TOL_M)) return -1;
      for (int q = j + 1; q < k; q++) if (row[ord[q]] != row[ord[j]]) return -1;
      if (j > 0 && d[ord[j - 1]] >= theta - E2) return -1;
      if (k < V && d[ord[k]] <= theta + E2) return -1;
      for (int i = 0; i < V; i++) keep[i] = d[i] <= theta;
      return k;
    }
    below = incl;
    j = k;
  }
  return -1; // the mass is never reached (the literal then keeps the whole row): left to the literal
}

int host_prefilter_row_typical(const float *row, double mass, int pf_min, int32_t *list) {
  const int V = TTS_VOCAB_MEL;
  std::fill(list, list + TTS_PF_WORDS, 0);
  list[0] = -1;
  if (pf_min > TTS_PF_MAX) return -1;
  std::vector<char> keep(V);
  const int nm = typical_keep_device_rule(row, mass, keep.data());
  if (nm < 0) return -1;
  std::vector<float> masked(row, row + V);
  for (int i = 0; i < V; i++) if (!keep[i]) masked[i] = -std::numeric_limits<float>::infinity();
  if (nm >= pf_min) return host_prefilter_row(masked.data(), pf_min, list); // the members >= the usual threshold
  float *lv = (float *)(list + 4 + TTS_PF_MAX); // fewer than pf_min (<= TTS_PF_MAX) members: the whole set
  int k = 0;
  for (int i = 0; i < V; i++)
    if (keep[i]) { list[4 + k] = i; lv[k] = row[i]; k++; }
  list[0] = nm; list[1] = TTS_PF_WHOLE;
  return nm;
}

struct Surv { float v; int idx; float e; };

// Tail shared by the full-row scan and the device-prefiltered list: `s` = the top-k survivors in INDEX order with their tempered
// values. top-p over the ascending order, final softmax + multinomial in index order. Survivors that tie: their exp terms are equal, so
// every sum below is the same number whichever of them std::sort puts first, and the order matters only where the top-p cut (or the
// exemption of the last element) separates two of them — then the tail returns -1 and the caller takes the literal formulation to inherit
// std::sort's tie order (measured on the 2-layer synthetic model: bit-equal logits among the 50 survivors in about 1 row of 200).
// Also -1 when a softmax sum is not a positive finite number (exp overflows at a small temperature: the literal formulation's NaN
// handling is then the definition).
static int sample_survivors(std::vector<Surv> &s, std::vector<Surv> &asc, float sample, double top_p_cut) {
  const int V = TTS_VOCAB_MEL;
  const float LOWEST = std::numeric_limits<float>::lowest();
  asc = s;
  std::sort(asc.begin(), asc.end(), [](const Surv &a, const Surv &b) { return a.v < b.v; });
  // top-p over the ascending survivors (non-survivors contribute exp(lowest) = +0)
  float sum = 0;
  for (auto &a : asc) { a.e = exp_like_reference(a.v); sum += a.e; }
  if (!(sum > 0) || !std::isfinite(sum)) return -1;
  float cum = 0;
  bool prev_below = false;
  for (size_t i = 0; i < asc.size(); i++) {
    cum += asc[i].e / sum;
    const bool below = cum <= top_p_cut, last = i + 1 == asc.size();
    if (i > 0 && asc[i].v == asc[i - 1].v && (below != prev_below || (last && below))) return -1; // the cut / the exemption falls inside a tie
    prev_below = below;
    if (!last && below)
      for (auto &b : s) if (b.idx == asc[i].idx) b.v = LOWEST; // cut
  }
  // final softmax + multinomial in index order
  sum = 0;
  for (auto &a : s) { a.e = (a.v == LOWEST) ? 0.f : exp_like_reference(a.v); sum += a.e; }
  if (!(sum > 0) || !std::isfinite(sum)) return -1;
  if (!(0.0f < sample)) return 0; // cumulative(=0) >= sample already at index 0
  cum = 0;
  for (auto &a : s) {
    cum += a.e / sum;
    if (cum >= sample) return a.idx;
  }
  return V - 1;
}

static inline float penalised(float g, float penalty) { return (g < 0) ? g * penalty : g / penalty; } // apply_penalty, main.cpp:4562-4570

// The survivors of temp_inplace + top_k_inplace are {i : val(i) / temp >= hmin / temp}, hmin = the k-th largest penalised value (float
// division by a positive temp is monotone, so the k-th largest quotient is the quotient of the k-th largest). That set is an up-set
// {val >= cut}: cut = the smallest float whose quotient still reaches hmin / temp, found by stepping down from hmin. For ordinary values at
// most two adjacent floats share a quotient; where the quotient saturates (overflow to inf, underflow to 0) the class is unbounded: after
// 8 steps the caller gives up (false) and takes the literal formulation / the full row.
static bool topk_cut(float hmin, float temp, float &cut) {
  const float LOWEST = std::numeric_limits<float>::lowest();
  const float kth = hmin / temp;
  cut = hmin;
  for (int tries = 0;; tries++) {
    const float below = std::nextafter(cut, LOWEST);
    if (below == cut) return false;
    if (!(below / temp >= kth)) return true;
    if (tries == 8) return false;
    cut = below;
  }
}

// Above this top-k the full-row sampler goes straight to the literal formulation (the heap scan below is built for a few dozen survivors).
static const int FAST_TOPK_MAX = 512;

// One candidate, given its uniform draw: pure function of its arguments (runs on the sampler pool's threads).
static int sample_one(const float *src, const int32_t *ids, int ids_per_cand, float sample, const SamplerParams &p, bool literal_only = false) {
  const int V = TTS_VOCAB_MEL, TOPK = p.top_k;
  const float LOWEST = std::numeric_limits<float>::lowest();
  const float temp = p.temp;
  thread_local std::vector<Surv> s, asc;
  thread_local std::vector<float> l; // only materialised for the (rare) literal fallback
  thread_local std::vector<float> prow, heap;
  thread_local std::vector<char> tkeep;
  const bool typ = p.typ_mass > 0;
  auto literal = [&]() {
    l.assign(src, src + V);
    for (int j = 0; j < ids_per_cand; j++) {
      const int id = ids[j];
      l[id] = penalised(src[id], p.penalty);
    }
    if (typ) { // the typical stage: after the penalty, before the temperature; a non-member has probability exactly 0 from here on, like top_k_inplace's masked entries
      tkeep.resize(V);
      typical_keep(l.data(), (double)p.typ_mass, tkeep.data());
      for (int i = 0; i < V; i++) if (!tkeep[i]) l[i] = LOWEST;
    }
    for (int i = 0; i < V; i++) l[i] /= temp;
    std::vector<float> tmp(l);
    std::nth_element(tmp.begin(), tmp.begin() + (V - TOPK), tmp.end());
    const float kth = tmp[V - TOPK];
    for (int i = 0; i < V; i++) if (l[i] < kth) l[i] = LOWEST;
    return multinomial_literal(l, sample, p.top_p_cut());
  };
  if (literal_only || TOPK > FAST_TOPK_MAX) return literal();
  if (typ) {
    // The engine's path under typical sampling: the penalised row, the literal's member set (typical_keep: one formulation), non-members masked. At most
    // top-k members: they all survive top-k (a masked entry has probability 0 and changes no sum), so the tail runs over the members; more: the scan below
    // over the masked row.
    prow.assign(src, src + V);
    for (int j = 0; j < ids_per_cand; j++) prow[ids[j]] = penalised(src[ids[j]], p.penalty);
    tkeep.resize(V);
    const int nm = typical_keep(prow.data(), (double)p.typ_mass, tkeep.data());
    for (int i = 0; i < V; i++) if (!tkeep[i]) prow[i] = LOWEST;
    if (nm <= TOPK) {
      s.clear();
      for (int i = 0; i < V; i++) if (tkeep[i]) s.push_back({prow[i] / temp, i, 0.f});
      const int pick = sample_survivors(s, asc, sample, p.top_p_cut());
      return pick < 0 ? literal() : pick;
    }
  }
  // gather -> apply_penalty -> scatter touches at most a few distinct ids under penalty scope 0 (the prompt-shaped
  // [1 ... 1, 8192] at step 0, the previous sample afterwards): keep them as overrides. More than four (scope 1: the
  // whole history): a penalised copy of the row is scanned instead.
  int pid[4]; float pval[4]; int np = 0;
  bool many = false;
  for (int j = 0; j < ids_per_cand; j++) {
    const int id = ids[j];
    bool seen = false;
    for (int q = 0; q < np; q++) seen |= (pid[q] == id);
    if (seen) continue;
    if (np == 4) { many = true; break; }
    pid[np] = id; pval[np] = penalised(src[id], p.penalty); np++;
  }
  const float *row = src;
  if (typ) { row = prow.data(); np = 0; } // penalised and masked above
  else if (many) {
    prow.assign(src, src + V);
    for (int j = 0; j < ids_per_cand; j++) prow[ids[j]] = penalised(src[ids[j]], p.penalty);
    row = prow.data();
    np = 0;
  }
  auto val = [&](int i) { for (int q = 0; q < np; q++) if (pid[q] == i) return pval[q]; return row[i]; };
  // k-th largest penalised logit: min-heap of the k largest seen so far (almost every element fails
  // the single compare against the heap minimum)
  heap.resize(TOPK);
  for (int i = 0; i < TOPK; i++) heap[i] = val(i);
  std::make_heap(heap.begin(), heap.end(), std::greater<float>());
  float hmin = heap[0];
  for (int i = TOPK; i < V; i++) {
    float x = row[i];
    if (x <= hmin) continue;              // (penalised values are <= their source: x * p <= x < 0, x / p <= x otherwise, p >= 1)
    x = val(i);
    if (x <= hmin) continue;
    std::pop_heap(heap.begin(), heap.end(), std::greater<float>());
    heap[TOPK - 1] = x;
    std::push_heap(heap.begin(), heap.end(), std::greater<float>());
    hmin = heap[0];
  }
  // overrides never exceed their source, so the scan above cannot miss them. Threshold on the tempered values: ties (also
  // those created by the division's rounding) survive, as in val_where_below_thresh: exactly the values >= cut (topk_cut).
  float cut;
  if (!topk_cut(hmin, temp, cut)) return literal();
  s.clear();
  for (int i = 0; i < V; i++) {
    if (row[i] < cut) continue;
    const float x = val(i);
    if (x >= cut) s.push_back({x / temp, i, 0.f});
  }
  const int pick = sample_survivors(s, asc, sample, p.top_p_cut());
  return pick < 0 ? literal() : pick; // a tie: inherit std::sort's tie order from the literal formulation
}

// The same candidate from the decode step's device prefilter (ar.hip: sample_prefilter_kernel): `n` (index, value) pairs in index
// order holding EVERY value >= the smallest one listed (thr). already_penalised = false (penalty scope 0): the values are raw logits and
// the penalty is applied here; true (scope 1): the kernel applied it. Returns the id sample_one would return on the full row, or -1 when
// that cannot be guaranteed from the list alone (the caller then fetches the row). For any temperature > 0, top-k and penalty >= 1:
//   - a penalised value never exceeds its source (x * p <= x < 0, x / p <= x otherwise), so in both forms every unlisted id has a
//     penalised value < thr;
//   - hmin = the k-th largest penalised value among the listed ones (n >= k) and cut = the smallest float with cut / temp >= hmin / temp
//     (topk_cut: exact). The list decides iff thr <= cut: then hmin >= thr, the k largest penalised values of the row are all listed and
//     hmin is the row's k-th largest; and every unlisted value is < cut, i.e. its quotient is < hmin / temp: no survivor is missing.
//     thr > cut (the logits between rank k and rank n within an ulp or two of each other) -> -1;
//   - raw lists: more than 4 distinct penalty ids are not looked up here -> -1; a tie among the survivors needs the literal
//     formulation over the full row -> -1.
// Typical sampling (p.typ_mass > 0): the list holds the row's typical MEMBERS >= thr, penalised (already_penalised in either scope), and every non-member is
// masked, so the argument above holds with "unlisted member" for "unlisted id". whole (header word 1 = TTS_PF_WHOLE): the list is the whole typical set; n may
// be below top-k (the set then survives top-k whole) and nothing unlisted can be missing, so thr is not consulted.
static int sample_one_list(int n, const int32_t *idx, const float *lv, const int32_t *ids, int ids_per_cand, float sample, const SamplerParams &p,
                           bool already_penalised, bool whole = false) {
  const int TOPK = p.top_k;
  const float temp = p.temp;
  thread_local std::vector<Surv> s, asc;
  thread_local std::vector<float> pv;
  if (n < TOPK && !whole) return -1;
  int pid[4]; int np = 0;
  if (!already_penalised)
    for (int j = 0; j < ids_per_cand; j++) {
      bool seen = false;
      for (int q = 0; q < np; q++) seen |= (pid[q] == ids[j]);
      if (seen) continue;
      if (np == 4) return -1;
      pid[np++] = ids[j];
    }
  pv.resize(n);
  float thr = lv[0];
  for (int i = 0; i < n; i++) {
    const float g = lv[i];
    thr = std::min(thr, g);
    bool pen = false;
    for (int q = 0; q < np; q++) pen |= (pid[q] == idx[i]);
    pv[i] = pen ? penalised(g, p.penalty) : g;
  }
  if (whole && n <= TOPK) {
    s.clear();
    for (int i = 0; i < n; i++) s.push_back({pv[i] / temp, idx[i], 0.f});
    return sample_survivors(s, asc, sample, p.top_p_cut());
  }
  asc.resize(n); // scratch: the k-th largest penalised value
  for (int i = 0; i < n; i++) asc[i].v = pv[i];
  std::nth_element(asc.begin(), asc.begin() + (TOPK - 1), asc.end(), [](const Surv &a, const Surv &b) { return a.v > b.v; });
  const float hmin = asc[TOPK - 1].v;
  float cut;
  if (!topk_cut(hmin, temp, cut)) return -1;
  if (!whole && !(thr <= cut)) return -1;
  s.clear();
  for (int i = 0; i < n; i++)
    if (pv[i] >= cut) s.push_back({pv[i] / temp, idx[i], 0.f});
  return sample_survivors(s, asc, sample, p.top_p_cut());
}

// Small persistent pool for the per-candidate sampler work (16 independent scans of 8194 logits between two
// decode steps). Workers spin for a short while after each job — the decode loop calls back within ~1 ms — and
// sleep on a condition variable otherwise.
struct SamplerPool {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv;
  // (job generation << 32) | next item. Items are claimed by compare-exchange on the whole word, so a worker that is
  // still leaving job g can neither claim an item of job g+1 nor disturb its counters: its exchange fails as soon as the
  // generation has moved on. `remaining` and `n_items` are published BEFORE the ticket (release) and only read after a
  // ticket load (acquire) that showed the matching generation.
  std::atomic<uint64_t> ticket{0};
  std::atomic<int> remaining{0}, n_items{0};
  std::function<void(int)> fn;
  std::atomic<bool> stop{false};
  explicit SamplerPool(int n) {
    for (int i = 0; i < n; i++) th.emplace_back([this] { loop(); });
  }
  ~SamplerPool() {
    { std::lock_guard<std::mutex> lk(m); stop.store(true); ticket.fetch_add(1ull << 32, std::memory_order_release); }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
  static uint32_t gen_of(uint64_t t) { return (uint32_t)(t >> 32); }
  void drain(uint32_t g) {
    for (;;) {
      uint64_t t = ticket.load(std::memory_order_acquire);
      if (gen_of(t) != g) return;                 // job g is over (or was never ours)
      const int i = (int)(uint32_t)t;
      if (i >= n_items.load(std::memory_order_relaxed)) return;
      if (!ticket.compare_exchange_weak(t, t + 1, std::memory_order_acq_rel)) continue;
      fn(i);                                      // job g cannot complete before this item does: fn is still job g's
      remaining.fetch_sub(1, std::memory_order_release);
    }
  }
  void loop() {
    uint32_t seen = 0;
    for (;;) {
      // spin up to 2 ms for the next job, then block
      auto t0 = std::chrono::steady_clock::now();
      while (gen_of(ticket.load(std::memory_order_acquire)) == seen) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(2000)) {
          std::unique_lock<std::mutex> lk(m);
          cv.wait(lk, [&] { return gen_of(ticket.load(std::memory_order_acquire)) != seen; });
          break;
        }
      }
      seen = gen_of(ticket.load(std::memory_order_acquire));
      if (stop.load()) return;
      drain(seen);
    }
  }
  void run(int n, std::function<void(int)> f) {
    uint32_t g;
    {
      std::lock_guard<std::mutex> lk(m);
      fn = std::move(f);
      n_items.store(n, std::memory_order_relaxed);
      remaining.store(n, std::memory_order_relaxed);
      g = gen_of(ticket.load(std::memory_order_relaxed)) + 1;
      ticket.store((uint64_t)g << 32, std::memory_order_release); // publishes fn / n_items / remaining, next item = 0
    }
    cv.notify_all();
    drain(g);
    while (remaining.load(std::memory_order_acquire) > 0) std::this_thread::yield();
  }
};
void sampler_pool_free(SamplerPool *p) { delete p; }

// The RNG is consumed in candidate order exactly as the reference does; the scans then run in parallel.
// Sharded batch (options "rng_shard_offset" / "rng_shard_total"): this context holds candidates
// [offset, offset + B) of a batch of `total`; the used uniform of (step s, global candidate c) is output 2 (s total + c) + 1
// of the one mt19937 stream, so the draws of the other ranks' candidates are skipped (each uniform is one 32-bit output).
// `gen`: the stream the uniforms come from. The context's own generator is one shard of the declared batch; any other generator (a session request's,
// tts_ar_session_admit) is a whole stream of its own: two uniforms per candidate and step, nothing skipped.
static void draw_uniforms(tts_ctx *ctx, std::mt19937 &gen, int B, std::vector<float> &samples) {
  const bool own = &gen == &ctx->generator;
  const int total = own && ctx->rng_shard_total > 0 ? ctx->rng_shard_total : B, c0 = own ? shard_base(ctx) : 0;
  samples.resize(B);
  if (c0 > 0) gen.discard(2ull * c0);
  std::uniform_real_distribution<float> &dist = ctx->distribution; // holds its bounds only: no state is shared between generators
  for (int c = 0; c < B; c++) {
    float sample = dist(gen); // first draw discarded (main.cpp:4708-4709)
    sample = dist(gen);
    samples[c] = sample;
  }
  if (total - c0 - B > 0) gen.discard(2ull * (total - c0 - B));
}

static void run_on_pool(tts_ctx *ctx, int B, const std::function<void(int)> &one) {
  if (B < 4 || ctx->sampler_threads == 0) { for (int c = 0; c < B; c++) one(c); return; }
  if (!ctx->sampler_pool) {
    const int hw = (int)std::thread::hardware_concurrency();
    const int n = ctx->sampler_threads > 0 ? ctx->sampler_threads : std::max(1, std::min(7, hw - 1));
    ctx->sampler_pool = new SamplerPool(n);
  }
  ctx->sampler_pool->run(B, one);
}

void sample_candidates(tts_ctx *ctx, std::mt19937 &gen, const SamplerParams &sp, const float *logits, const PenaltyIdsFn &ids_of, int B, int32_t *out) {
  const int V = TTS_VOCAB_MEL;
  std::vector<float> samples;
  draw_uniforms(ctx, gen, B, samples);
  run_on_pool(ctx, B, [&](int c) {
    const int32_t *ids = nullptr; int n_ids = 0;
    ids_of(c, ids, n_ids);
    out[c] = sample_one(logits + (size_t)c * V, ids, n_ids, samples[c], sp);
  });
}
void sample_candidates(tts_ctx *ctx, std::mt19937 &gen, const SamplerParams &sp, const float *logits, const int32_t *ids, int ids_per_cand, int B,
                       int32_t *out) {
  sample_candidates(ctx, gen, sp, logits, [&](int c, const int32_t *&p, int &n) { p = ids + (size_t)c * ids_per_cand; n = ids_per_cand; }, B, out);
}

// The decode loop's sampler over the device prefilter's lists (ar.hip: [B][TTS_PF_WORDS] = {n, 0, 0, 0, idx[128], value[128]}), same
// uniforms, same ids. A candidate whose list cannot decide (n < 0: the device found no threshold keeping pf_min..128 values; or
// sample_one_list's -1) is sampled from its full row, fetched through `full_row` (which applies the stop mask itself) and penalised
// here with ids_of(c) in either form.
// `retired` (may be null): candidates whose sequence has ended (TTS_AR_RETIRE). Their uniforms are drawn like everybody's — the stream stays the reference's — but
// nothing is sampled for them (out = 8193): round 5's ragged bench pass spent 27 ms per utterance evaluating lists and fetching full logits rows for candidates whose
// sample the loop then threw away.
int sample_candidates_list(tts_ctx *ctx, std::mt19937 &gen, const SamplerParams &sp, const int32_t *lists, const PenaltyIdsFn &ids_of, bool already_penalised, int B,
                           int32_t *out, const std::function<const float *(int)> &full_row, int *n_fallbacks, const char *retired) {
  std::vector<float> samples;
  draw_uniforms(ctx, gen, B, samples);
  auto one = [&](int c) {
    if (retired && retired[c]) { out[c] = 8193; return; }
    const int32_t *l = lists + (size_t)c * TTS_PF_WORDS;
    const int n = l[0];
    if (n < 1 || n > TTS_PF_MAX) { out[c] = -1; return; }
    const int32_t *ids = nullptr; int n_ids = 0;
    if (!already_penalised) ids_of(c, ids, n_ids);
    out[c] = sample_one_list(n, l + 4, (const float *)(l + 4 + TTS_PF_MAX), ids, n_ids, samples[c], sp, already_penalised, sp.typ_mass > 0 && (l[1] & TTS_PF_WHOLE));
  };
  if (B < 8 || ctx->sampler_threads == 0) { for (int c = 0; c < B; c++) one(c); } // ~2 us per list: the pool's wake-up costs more below 8
  else run_on_pool(ctx, B, one);
  int fb = 0;
  for (int c = 0; c < B; c++) {
    if (out[c] >= 0) continue;
    const float *row = full_row(c);
    if (!row) return -1;
    const int32_t *ids = nullptr; int n_ids = 0;
    ids_of(c, ids, n_ids);
    out[c] = sample_one(row, ids, n_ids, samples[c], sp);
    fb++;
  }
  if (n_fallbacks) *n_fallbacks += fb;
  return 0;
}
int sample_candidates_list(tts_ctx *ctx, std::mt19937 &gen, const SamplerParams &sp, const int32_t *lists, const int32_t *ids, int ids_per_cand, int B, int32_t *out,
                           const std::function<const float *(int)> &full_row, int *n_fallbacks, const char *retired) {
  return sample_candidates_list(ctx, gen, sp, lists, [&](int c, const int32_t *&p, int &n) { p = ids + (size_t)c * ids_per_cand; n = ids_per_cand; }, false, B, out,
                                full_row, n_fallbacks, retired);
}

// Host restatement of the device prefilter for tests (tts_host_sample_prefiltered*): the `keep` largest values and every tie of the
// smallest of them, in index order; n = -1 when that exceeds the list capacity.
int host_prefilter_row(const float *row, int keep, int32_t *list) {
  const int V = TTS_VOCAB_MEL;
  std::vector<float> tmp(row, row + V);
  std::nth_element(tmp.begin(), tmp.begin() + (keep - 1), tmp.end(), std::greater<float>());
  const float thr = tmp[keep - 1];
  int n = 0;
  for (int i = 0; i < V; i++) n += row[i] >= thr;
  std::fill(list, list + TTS_PF_WORDS, 0);
  if (n > TTS_PF_MAX) { list[0] = -1; return -1; }
  list[0] = n;
  float *lv = (float *)(list + 4 + TTS_PF_MAX);
  int k = 0;
  for (int i = 0; i < V; i++)
    if (row[i] >= thr) { list[4 + k] = i; lv[k] = row[i]; k++; }
  return n;
}

int sample_one_row_ex(const float *row, const int32_t *ids, int n_ids, float uniform, const SamplerParams &p, bool literal_only) {
  return sample_one(row, ids, n_ids, uniform, p, literal_only);
}
int sample_one_from_list_ex(const int32_t *list, const int32_t *ids, int n_ids, float uniform, const SamplerParams &p, bool already_penalised) {
  const int n = list[0];
  if (n < 1 || n > TTS_PF_MAX) return -1;
  return sample_one_list(n, list + 4, (const float *)(list + 4 + TTS_PF_MAX), ids, n_ids, uniform, p, already_penalised, p.typ_mass > 0 && (list[1] & TTS_PF_WHOLE));
}
int sample_one_row(const float *row, const int32_t *ids, int ids_per_cand, float uniform) { return sample_one(row, ids, ids_per_cand, uniform, SamplerParams()); }
int sample_one_from_list(const int32_t *list, const int32_t *ids, int ids_per_cand, float uniform) {
  return sample_one_from_list_ex(list, ids, ids_per_cand, uniform, SamplerParams(), false);
}

// apply_padding, main.cpp:4510-4532 (the 8139 is the reference's literal, not 8193)
void pad_codes(std::vector<int> &codes) {
  while (!codes.empty() && codes.back() == 8139) codes.pop_back();
  codes.resize(500, 83);
  codes[497] = 45;
  codes[498] = 45;
  codes[499] = 248;
  codes.push_back(8193);
  codes.insert(codes.begin(), 8192);
}

void ArStopBook::init(const int *n_cand, int G) {
  c0.assign(G, 0); n.assign(n_cand, n_cand + G);
  for (int g = 1; g < G; g++) c0[g] = c0[g - 1] + n[g - 1];
  const int B = G ? c0[G - 1] + n[G - 1] : 0;
  done.assign(B, 0); retired.assign(B, 0); ended.assign(G, 0);
  seq.assign(B, {});
}

// One prompt (G = 1) is the loop of rounds 1-6 exactly: strict mode ends when all B samples of one iteration are 8193, retire mode when every
// candidate has retired.
bool ArStopBook::step(int32_t *samples, int i, bool retire, const int32_t *stop_at) {
  bool all = true;
  for (size_t g = 0; g < n.size(); g++) {
    int stops = 0;
    for (int b = c0[g]; b < c0[g] + n[g]; b++) {
      if (stop_at && i == stop_at[b]) samples[b] = 8193; // tts_ar_set_stop_schedule
      if (retired[b]) { samples[b] = 8193; stops++; continue; }
      if (!(seq[b].size() > 0 && seq[b].back() == 8193)) seq[b].push_back(samples[b]);
      if (samples[b] == 8193) { stops++; done[b] = 1; if (retire) retired[b] = 1; }
    }
    if (stops == n[g] && !ended[g]) {
      ended[g] = 1;
      for (int b = c0[g]; b < c0[g] + n[g]; b++) retired[b] = 1; // the group's rows are fed 8193 from now on
    }
    all = all && ended[g];
  }
  return all;
}

// trim_latents, main.cpp:4873-4915: rows kept until more than 8 consecutive 83s.
int trimmed_latent_rows(const int32_t *codes502) {
  int run = 0;
  for (int c = 0; c < 500; c++) {
    run = (codes502[1 + c] == 83) ? run + 1 : 0;
    if (run > 8) return c;
  }
  return 500;
}

// tts_hifigan_stream: latent row j is a function of the inputs 0 .. j (causal), input 0 is 8192 and input 1 + i the i-th sampled code; pad_codes rewrites from
// the stop token onward, so after k sampled non-stop codes the rows 0 .. k are final. trim_latents cuts at the first run of more than 8 codes 83 and at 500
// rows. A run the sampler itself produced counts, and the padding is 83s too: when the last 8 sampled codes are 83 and the utterance is cut here, the padding
// completes the run and row k is trimmed, so it is not declared final yet.
int stream_final_rows(const int32_t *codes, int k) {
  int run = 0;
  for (int c = 0; c < k && c < 500; c++) {
    run = (codes[c] == 83) ? run + 1 : 0;
    if (run > 8) return c;
  }
  return std::min(std::min(k + 1, k - run + 8), 500);
}

// get_relative_position_buckets, main.cpp:4722-4749 (i = query, c = key)
int rel_bucket(int i, int c) {
  const int dist = std::abs(c - i);
  int b = (i < c) ? 16 : 0;
  if (dist < 8) return b + dist;
  int big = 8 + (int)(::log((double)(float(dist) / 8)) / ::log(64.0 / 8.0) * (16.0 - 8.0));
  return b + std::min(big, 15);
}

// generate_timestep_embedding, main.cpp:5496-5521 (dim 1024, max_period 10000; cos half first)
void timestep_embedding(int t, float *out) {
  for (int i = 0; i < 512; ++i) {
    float freq = ::exp(-::log((double)10000) * static_cast<float>(i) / 512);
    float arg = static_cast<float>(t) * freq;
    out[i] = (float)::cos((double)arg);
    out[512 + i] = (float)::sin((double)arg);
  }
}

// Schedule: main.cpp:5370-5493 + 5641-5716, then the per-step scalars of 5988-6015 in the exact
// types the reference uses (double tables, float at the point of use).
void DiffSchedule::build(int n_steps) {
  n = n_steps;
  timestep_map.resize(n);
  for (int i = 0; i < n; i++) timestep_map[i] = (int)std::lround((double)i * 3999.0 / (n - 1)); // == literal table for n=80
  const int NT = 4000;
  const double scale = 1000.0 / NT, beta_start = scale * 0.0001, beta_end = scale * 0.02;
  std::vector<double> acp4000(NT);
  double prod = 1.0;
  for (int i = 0; i < NT; ++i) {
    double beta = beta_start + i * (float)(beta_end - beta_start) / (NT - 1);
    double alpha = 1.0f - beta;
    prod = (i == 0) ? alpha : prod * alpha;
    acp4000[i] = prod;
  }
  std::vector<double> beta(n), pvar(n), plv(n);
  acp.assign(n, 0.0); prev.assign(n, 0.0);
  float last = 1.0; // float on purpose (main.cpp:5663)
  for (int k = 0; k < n; k++) {
    beta[k] = 1 - (acp4000[timestep_map[k]] / last);
    last = acp4000[timestep_map[k]];
  }
  prod = 1.0;
  for (int k = 0; k < n; k++) {
    double alpha = 1.0f - beta[k];
    prod = (k == 0) ? alpha : prod * alpha;
    acp[k] = prod;
    prev[k] = (k == 0) ? 1.0f : acp[k - 1];
  }
  for (int k = 0; k < n; k++) pvar[k] = beta[k] * (1.0 - prev[k]) / (1.0 - acp[k]);
  plv[0] = std::log(pvar[1]);
  for (int k = 1; k < n; k++) plv[k] = std::log(pvar[k]);
  max_log.resize(n); min_log.resize(n); cfk.resize(n); sqrt_recip.resize(n); sqrt_recipm1.resize(n);
  coef1.resize(n); coef2.resize(n);
  for (int t = 0; t < n; t++) {
    max_log[t] = std::log(beta[t]);
    min_log[t] = plv[t];
    cfk[t] = base_k * (1 - (float)t / float(n));
    sqrt_recip[t] = std::sqrt(1.0f / acp[t]);
    sqrt_recipm1[t] = std::sqrt(1.0f / acp[t] - 1);
    coef1[t] = beta[t] * std::sqrt(prev[t]) / (1.0 - acp[t]);
    coef2[t] = (1.0 - prev[t]) * std::sqrt(1.0 - beta[t]) / (1.0 - acp[t]);
  }
}

// DDIM per-step scalars (Song et al. 2021 eq. 12 / 16, as upstream tortoise-tts' ddim_sample states them) on the respaced schedule of build().
// At t = 0 (prev = 1): sigma = 0, c_x0 = 1, c_eps = 0. For eta <= 1 the argument of the last root is acp (1 - prev)^2 / ((1 - acp) prev) >= 0 at eta = 1 and
// grows as eta falls.
void DiffSchedule::build_ddim(double eta) {
  ddim_sigma.resize(n); ddim_c_x0.resize(n); ddim_c_eps.resize(n);
  c_x0.resize(n); c_eps.resize(n); sigma.resize(n);
  for (int t = 0; t < n; t++) {
    ddim_sigma[t] = eta * std::sqrt((1.0 - prev[t]) / (1.0 - acp[t])) * std::sqrt(1.0 - acp[t] / prev[t]);
    ddim_c_x0[t] = std::sqrt(prev[t]);
    ddim_c_eps[t] = std::sqrt(std::max(0.0, 1.0 - prev[t] - ddim_sigma[t] * ddim_sigma[t]));
    sigma[t] = (float)ddim_sigma[t]; c_x0[t] = (float)ddim_c_x0[t]; c_eps[t] = (float)ddim_c_eps[t];
  }
}

// DPM-Solver++(2M) per-step scalars (Lu et al. 2022, multistep second order on the data prediction) on the respaced schedule of build(). Step t moves from level
// acp[t] (alpha_s, sigma_s, lambda_s) to prev[t] (alpha_n, sigma_n, lambda_n); h = lambda_n - lambda_s, phi = alpha_n (1 - e^-h); the step before it came from level
// acp[t + 1], r = (lambda_s - lambda(acp[t + 1])) / h. Second order: x_n = (sigma_n / sigma_s) x + phi (1 + 1 / 2r) x0 - (phi / 2r) x0_prev. First order (c = 0,
// b = phi) at t = n - 1, which has no history, and at t = 1 and t = 0: the respaced schedule ends at timestep 0 of 4000, where log-SNR jumps by several step
// widths, and a second-order update across that jump extrapolates with r ~ 0.1 (DESIGN.md "What pins the DPM-Solver++ sampler"). At t = 0 sigma_n = 0: (0, 1, 0).
void DiffSchedule::build_dpmpp() {
  dpm_a.assign(n, 0.f); dpm_b.assign(n, 0.f); dpm_c.assign(n, 0.f); dpm_order.assign(n, 1);
  auto lambda = [](double a) { return 0.5 * std::log(a) - 0.5 * std::log(1.0 - a); };
  dpm_b[0] = 1.f;
  for (int t = 1; t < n; t++) {
    const double sigma_s = std::sqrt(1.0 - acp[t]), alpha_n = std::sqrt(prev[t]), sigma_n = std::sqrt(1.0 - prev[t]);
    const double lambda_s = lambda(acp[t]), h = lambda(prev[t]) - lambda_s, phi = alpha_n * -std::expm1(-h);
    dpm_a[t] = (float)(sigma_n / sigma_s);
    if (t >= 2 && t <= n - 2) {
      const double r = (lambda_s - lambda(acp[t + 1])) / h;
      dpm_order[t] = 2;
      dpm_b[t] = (float)(phi * (1.0 + 1.0 / (2.0 * r)));
      dpm_c[t] = (float)(-phi / (2.0 * r));
    } else dpm_b[t] = (float)phi;
  }
}

// Text splitter (tts_split_text; our own rule, stated in include/tortoise_mi355x.h). Chunks are byte ranges of the message; every chunk tokenizes to
// at most max_ids ids. Token counts are those of Tokenizer::encode on the chunk's bytes (255 ... 0 included).
std::vector<std::pair<int, int>> split_text(const Tokenizer &tok, const std::string &msg, int max_ids) {
  auto ws = [&](int i) { return isspace((unsigned char)msg[i]) != 0; };
  auto fits = [&](int a, int b) { // the trimmed piece, as it would be emitted
    while (a < b && ws(a)) a++;
    while (b > a && ws(b - 1)) b--;
    return (int)tok.encode(msg.substr(a, b - a)).size() <= max_ids;
  };
  const int n = (int)msg.size();
  // sentences: [a, b) trimmed, ending after '.', '!' or '?' followed by whitespace or the end of the text
  std::vector<std::pair<int, int>> sent;
  for (int i = 0; i < n;) {
    while (i < n && ws(i)) i++;
    if (i >= n) break;
    int j = i;
    while (j < n && !((msg[j] == '.' || msg[j] == '!' || msg[j] == '?') && (j + 1 == n || ws(j + 1)))) j++;
    j = std::min(n, j + 1);
    int e = j;
    while (e > i && ws(e - 1)) e--;
    sent.push_back({i, e});
    i = j;
  }
  std::vector<std::pair<int, int>> out;
  auto emit = [&](int a, int b) { // trimmed, never empty
    while (a < b && ws(a)) a++;
    while (b > a && ws(b - 1)) b--;
    if (b > a) out.push_back({a, b - a});
  };
  // an over-long sentence [a, b): cut after the last ',', ';', ':' or space whose piece fits, else at the longest fitting prefix (whole UTF-8 characters)
  auto split_long = [&](int a, int b) {
    while (a < b) {
      while (a < b && ws(a)) a++;
      if (a >= b) break;
      if (fits(a, b)) { emit(a, b); break; }
      int best = -1;
      for (int k = a + 1; k < b; k++) { // break points in order; the token count grows with the piece, so stop at the first that does not fit
        const char ch = msg[k - 1];
        if (!(ch == ',' || ch == ';' || ch == ':' || ws(k - 1))) continue;
        if (!fits(a, k)) break;
        best = k;
      }
      if (best < 0) { // hard cut: the longest prefix that fits (bisection over character starts, then checked downwards)
        int lo = a + 1, hi = b; // lo: fits (one character is at most one id, max_ids >= 3), hi: does not
        while (lo < b && ((unsigned char)msg[lo] & 0xC0) == 0x80) lo++;
        auto cstart = [&](int k) { while (k > a && k < b && ((unsigned char)msg[k] & 0xC0) == 0x80) k--; return k; };
        while (hi - lo > 1) {
          const int mid = cstart(lo + (hi - lo) / 2);
          if (mid <= lo) break;
          if (fits(a, mid)) lo = mid; else hi = mid;
        }
        while (lo > a + 1 && !fits(a, lo)) lo = cstart(lo - 1);
        best = lo;
        while (best < b && ((unsigned char)msg[best] & 0xC0) == 0x80) best++; // never split a character
      }
      emit(a, best);
      a = best;
    }
  };
  for (size_t s0 = 0; s0 < sent.size();) {
    const int a = sent[s0].first;
    if (!fits(a, sent[s0].second)) { split_long(a, sent[s0].second); s0++; continue; }
    size_t s1 = s0 + 1; // greedy: whole sentences while the chunk fits
    while (s1 < sent.size() && fits(a, sent[s1].second)) s1++;
    emit(a, sent[s1 - 1].second);
    s0 = s1;
  }
  return out;
}

// Turn splitter (tts_split_turns; the rule is stated in include/tortoise_mi355x.h): turns are the lines of the message, a turn that begins with
// "<decimal index>|" (blanks in front of the digits allowed) speaks with that voice and the prefix is not text, a turn without one keeps the voice of the
// turn before it (the first: voice 0); every turn's text then goes through split_text. Returns false for a voice index >= n_voices (*bad_voice says which).
bool split_turns(const Tokenizer &tok, const std::string &msg, int n_voices, int max_ids, std::vector<TurnChunk> &out, long *bad_voice) {
  const int n = (int)msg.size();
  int voice = 0;
  for (int a = 0; a <= n;) {
    int b = a;
    while (b < n && msg[b] != '\n') b++;
    int p = a;
    while (p < b && (msg[p] == ' ' || msg[p] == '\t')) p++;
    int q = p;
    long idx = 0;
    while (q < b && msg[q] >= '0' && msg[q] <= '9') { idx = std::min(idx * 10 + (msg[q] - '0'), 1000000000L); q++; }
    int text0 = a;
    if (q > p && q < b && msg[q] == '|') {
      if (idx >= n_voices) { if (bad_voice) *bad_voice = idx; return false; }
      voice = (int)idx;
      text0 = q + 1;
    }
    for (const std::pair<int, int> &c : split_text(tok, msg.substr(text0, b - text0), max_ids)) out.push_back({text0 + c.first, c.second, voice});
    a = b + 1;
  }
  return true;
}

} // namespace tts

// ---- host-logic probes: the host-side pieces of the stage drivers, callable without a GPU (tests/test_host_parity.py) ----
extern "C" int tts_host_schedule(int n_steps, int32_t *timestep_map, float *max_log, float *min_log, float *cfk, float *sqrt_recip,
                                 float *sqrt_recipm1, float *coef1, float *coef2) {
  if (n_steps < 2) return TTS_ERR_ARG;
  tts::DiffSchedule s;
  s.build(n_steps);
  for (int t = 0; t < n_steps; t++) {
    timestep_map[t] = s.timestep_map[t];
    max_log[t] = s.max_log[t]; min_log[t] = s.min_log[t]; cfk[t] = s.cfk[t];
    sqrt_recip[t] = s.sqrt_recip[t]; sqrt_recipm1[t] = s.sqrt_recipm1[t];
    coef1[t] = s.coef1[t]; coef2[t] = s.coef2[t];
  }
  return TTS_OK;
}
extern "C" int tts_host_schedule_ddim(int n_steps, double eta, double *acp, double *acp_prev, float *c_x0, float *c_eps, float *sigma) {
  if (n_steps < 2 || !(eta >= 0.0 && eta <= 1.0) || !acp || !acp_prev || !c_x0 || !c_eps || !sigma) return TTS_ERR_ARG; // (a NaN eta fails both comparisons)
  tts::DiffSchedule s;
  s.build(n_steps);
  s.build_ddim(eta);
  for (int t = 0; t < n_steps; t++) {
    acp[t] = s.acp[t]; acp_prev[t] = s.prev[t];
    c_x0[t] = s.c_x0[t]; c_eps[t] = s.c_eps[t]; sigma[t] = s.sigma[t];
  }
  return TTS_OK;
}
extern "C" int tts_host_schedule_dpmpp(int n_steps, float *a, float *b, float *c, int32_t *order) {
  if (n_steps < 2 || !a || !b || !c || !order) return TTS_ERR_ARG;
  tts::DiffSchedule s;
  s.build(n_steps);
  s.build_dpmpp();
  for (int t = 0; t < n_steps; t++) { a[t] = s.dpm_a[t]; b[t] = s.dpm_b[t]; c[t] = s.dpm_c[t]; order[t] = s.dpm_order[t]; }
  return TTS_OK;
}
extern "C" void tts_host_timestep_embedding(int t, float *out1024) { tts::timestep_embedding(t, out1024); }
extern "C" int tts_host_rel_bucket(int query, int key) { return tts::rel_bucket(query, key); }
extern "C" int tts_host_pad_codes(const int32_t *codes, int n, int32_t *out502) {
  if (n < 0 || n > 500) return TTS_ERR_ARG;
  std::vector<int> v(codes, codes + n);
  tts::pad_codes(v);
  if (v.size() != 502) return TTS_ERR_LIMIT;
  std::copy(v.begin(), v.end(), out502);
  return TTS_OK;
}
extern "C" int tts_host_trimmed_rows(const int32_t *codes502) { return tts::trimmed_latent_rows(codes502); }
// The row table of tts_ar_score_codes, stated once: n codes have n + 1 scored rows. Row 0 feeds the start token 8192 at mel position 0 and predicts code 0; row
// j >= 1 feeds code j - 1 and predicts code j, the last one the stop token 8193. Code i sits at mel position i + 2 in TTS_SCORE_POS_DECODE (what the decode
// step saw: ar_step feeds step i's token at position i + 2) and at i + 1 in TTS_SCORE_POS_TRAIN (the latent pass's and upstream forward()'s).
int tts::ar_score_row_table(const int32_t *codes, int n, int positions, int32_t *input_ids, int32_t *mel_pos, int32_t *targets) {
  if (!codes || !input_ids || !mel_pos || !targets || n < 1 || (positions != TTS_SCORE_POS_DECODE && positions != TTS_SCORE_POS_TRAIN)) return TTS_ERR_ARG;
  if (n > 500) return TTS_ERR_LIMIT;
  for (int i = 0; i < n; i++)
    if (codes[i] < 0 || codes[i] >= 8192) return TTS_ERR_ARG;
  const int shift = positions == TTS_SCORE_POS_DECODE ? 2 : 1;
  for (int j = 0; j <= n; j++) {
    input_ids[j] = j == 0 ? 8192 : codes[j - 1];
    mel_pos[j] = j == 0 ? 0 : j - 1 + shift;
    targets[j] = j == n ? 8193 : codes[j];
  }
  return TTS_OK;
}
extern "C" int tts_host_ar_score_rows(const int32_t *codes, int n_codes, int positions, int32_t *input_ids, int32_t *mel_pos, int32_t *targets) {
  return tts::ar_score_row_table(codes, n_codes, positions, input_ids, mel_pos, targets);
}
// The decode loop's stop bookkeeping (tts::ArStopBook, the one tts_autoregressive_multi runs) on scripted samples: samples [max_steps][B] are what the
// sampler returns at each iteration. Outputs as the driver's: codes [B][502] (padded), stopped [B], *steps; inputs [max_steps][B] (may be null): the tokens fed to
// the decode step after each iteration. TTS_ERR_LIMIT when strict mode reaches max_steps.
extern "C" int tts_host_ar_stop_run(const int32_t *n_cand, int G, const int32_t *samples, int max_steps, unsigned flags, const int32_t *stop_at,
                                    int32_t *codes_out, int32_t *stopped_out, int32_t *steps_out, int32_t *inputs_out) {
  if (!n_cand || G < 1 || !samples || max_steps < 1 || max_steps > 500 || !codes_out || !stopped_out || !steps_out) return TTS_ERR_ARG;
  int B = 0;
  for (int g = 0; g < G; g++) { if (n_cand[g] < 1) return TTS_ERR_ARG; B += n_cand[g]; }
  const bool retire = (flags & TTS_AR_RETIRE) != 0, sched = stop_at && (flags & TTS_AR_MASK_STOP) && retire;
  tts::ArStopBook book;
  book.init(n_cand, G);
  std::vector<int32_t> s(B);
  int i = 0;
  for (;;) {
    std::copy(samples + (size_t)i * B, samples + (size_t)(i + 1) * B, s.begin());
    const bool end = book.step(s.data(), i, retire, sched ? stop_at : nullptr);
    if (inputs_out) std::copy(s.begin(), s.end(), inputs_out + (size_t)i * B);
    i++;
    if (end) break;
    if (i >= max_steps) {
      if ((flags & TTS_AR_MASK_STOP) || retire) break;
      *steps_out = i;
      return TTS_ERR_LIMIT;
    }
  }
  *steps_out = i;
  for (int b = 0; b < B; b++) {
    stopped_out[b] = (!book.seq[b].empty() && book.seq[b].back() == 8193) ? 1 : 0;
    std::vector<int> v = book.seq[b];
    if (v.size() > 500) v.resize(500);
    tts::pad_codes(v);
    std::copy(v.begin(), v.end(), codes_out + (size_t)b * 502);
  }
  return TTS_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Mel front-end of the two voice-conditioning encoders (upstream tortoise-tts; the reference has no audio INPUT path at all).
// STFT with a periodic Hann window, centre = true (reflect padding of n_fft / 2), frames = n / hop + 1; triangular mel filterbank with
// Slaney area normalisation on the Slaney ("librosa") or HTK mel scale.
//   TacotronSTFT(1024, 256, 1024, 100, 24000, 0, 12000) -> magnitude, librosa filterbank, log(clamp 1e-5), normalised to [-1, 1] with the
//     constants the vocoder driver de-normalises with (main.cpp:6044-6060)                                   = tts_host_mel_diffusion100 (normalize = 1; upstream feeds the conditioning encoder the UN-normalised log-mel: normalize = 0)
//   torchaudio MelSpectrogram(n_fft 1024, hop 256, power 2, sample_rate 22050, f_max 8000, n_mels 80, norm "slaney", mel_scale "htk"),
//     log(clamp 1e-5), divided by the per-band mel_norms of the upstream data directory (optional here)       = tts_host_mel_voice80
// ------------------------------------------------------------------------------------------------------------------------------
namespace tts {
static void fft_inplace(std::vector<double> &re, std::vector<double> &im) { // radix-2, size = power of two
  const size_t n = re.size();
  for (size_t i = 1, j = 0; i < n; i++) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    const double ang = -2.0 * M_PI / (double)len;
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < len / 2; k++) {
        const double wr = std::cos(ang * (double)k), wi = std::sin(ang * (double)k);
        const double ur = re[i + k], ui = im[i + k];
        const double vr = re[i + k + len / 2] * wr - im[i + k + len / 2] * wi, vi = re[i + k + len / 2] * wi + im[i + k + len / 2] * wr;
        re[i + k] = ur + vr; im[i + k] = ui + vi;
        re[i + k + len / 2] = ur - vr; im[i + k + len / 2] = ui - vi;
      }
  }
}
static double hz_to_mel(double f, bool htk) {
  if (htk) return 2595.0 * std::log10(1.0 + f / 700.0);
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m, bool htk) {
  if (htk) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}
// [n_mels][n_fft / 2 + 1], triangles between n_mels + 2 points equally spaced on the mel scale, each divided by half its width in Hz (Slaney)
static std::vector<double> mel_filterbank(int n_mels, int n_fft, double sr, double f_min, double f_max, bool htk) {
  const int nb = n_fft / 2 + 1;
  std::vector<double> pts(n_mels + 2), fb((size_t)n_mels * nb, 0.0);
  const double m0 = hz_to_mel(f_min, htk), m1 = hz_to_mel(f_max, htk);
  for (int i = 0; i < n_mels + 2; i++) pts[i] = mel_to_hz(m0 + (m1 - m0) * i / (n_mels + 1), htk);
  for (int m = 0; m < n_mels; m++) {
    const double lo = pts[m], ce = pts[m + 1], hi = pts[m + 2], enorm = 2.0 / (hi - lo);
    for (int k = 0; k < nb; k++) {
      const double f = sr * k / n_fft, up = (f - lo) / (ce - lo), down = (hi - f) / (hi - ce);
      fb[(size_t)m * nb + k] = std::max(0.0, std::min(up, down)) * enorm;
    }
  }
  return fb;
}
// mel_out [n_mels][frames]; power 1 = magnitude, 2 = power spectrum; returns the frame count (n / hop + 1), < 0 on bad arguments
static int mel_spectrogram(const float *audio, int64_t n, int n_fft, int hop, int n_mels, double sr, double f_min, double f_max, bool htk, int power,
                           std::vector<double> &mel_out) {
  if (!audio || n <= n_fft / 2 || (n_fft & (n_fft - 1)) || hop < 1 || n_mels < 1) return TTS_ERR_ARG; // reflect padding needs n > n_fft / 2
  const int nb = n_fft / 2 + 1, pad = n_fft / 2, frames = (int)(n / hop) + 1;
  const std::vector<double> fb = mel_filterbank(n_mels, n_fft, sr, f_min, f_max, htk);
  std::vector<double> win(n_fft), re(n_fft), im(n_fft), spec(nb);
  for (int i = 0; i < n_fft; i++) win[i] = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / n_fft); // periodic Hann
  mel_out.assign((size_t)n_mels * frames, 0.0);
  for (int t = 0; t < frames; t++) {
    for (int i = 0; i < n_fft; i++) {
      int64_t j = (int64_t)t * hop + i - pad; // reflect (no edge repeat): -1 -> 1, n -> n - 2
      if (j < 0) j = -j;
      if (j >= n) j = 2 * (n - 1) - j;
      re[i] = (double)audio[j] * win[i]; im[i] = 0.0;
    }
    fft_inplace(re, im);
    for (int k = 0; k < nb; k++) { const double p = re[k] * re[k] + im[k] * im[k]; spec[k] = power == 2 ? p : std::sqrt(p); }
    for (int m = 0; m < n_mels; m++) {
      double a = 0;
      for (int k = 0; k < nb; k++) a += fb[(size_t)m * nb + k] * spec[k];
      mel_out[(size_t)m * frames + t] = a;
    }
  }
  return frames;
}
} // namespace tts
extern "C" int tts_host_mel_frames(int64_t n_samples) { return n_samples < 0 ? TTS_ERR_ARG : (int)(n_samples / 256) + 1; }
// normalize = 0: log(clamp(mel, 1e-5)) as upstream's get_conditioning_latents feeds the contextual_embedder (wav_to_univnet_mel(...,
// do_normalization=False)): the input of tts_diffusion_conditioning_latent. normalize = 1: mapped to [-1, 1] with the constants the vocoder
// driver de-normalises with (normalize_tacotron_mel; the inverse is main.cpp:6044-6060): the scale of the diffusion stage's OUTPUT.
extern "C" int tts_host_mel_diffusion100(const float *audio24k, int64_t n, int normalize, float *mel_out) {
  std::vector<double> mel;
  const int frames = tts::mel_spectrogram(audio24k, n, 1024, 256, 100, 24000.0, 0.0, 12000.0, /*htk=*/false, /*power=*/1, mel);
  if (frames < 0) return frames;
  const double mel_max = 2.3143386840820312, mel_min = -11.512925148010254;
  for (size_t i = 0; i < mel.size(); i++) {
    const double lm = std::log(std::max(mel[i], 1e-5));
    mel_out[i] = (float)(normalize ? 2.0 * ((lm - mel_min) / (mel_max - mel_min)) - 1.0 : lm);
  }
  return frames;
}
extern "C" int tts_host_mel_voice80(const float *audio22k, int64_t n, const float *mel_norms80, float *mel_out) {
  std::vector<double> mel;
  const int frames = tts::mel_spectrogram(audio22k, n, 1024, 256, 80, 22050.0, 0.0, 8000.0, /*htk=*/true, /*power=*/2, mel);
  if (frames < 0) return frames;
  for (int m = 0; m < 80; m++)
    for (int t = 0; t < frames; t++)
      mel_out[(size_t)m * frames + t] = (float)(std::log(std::max(mel[(size_t)m * frames + t], 1e-5)) / (mel_norms80 ? (double)mel_norms80[m] : 1.0));
  return frames;
}

// writeWav, main.cpp:4821-4868
extern "C" int tts_write_wav(const char *path, const float *samples, int64_t n, int sample_rate) {
  FILE *f = fopen(path, "wb");
  if (!f) return TTS_ERR_IO;
  const int32_t channels = 1, bits = 32;
  const int32_t byte_rate = sample_rate * channels * bits / 8, block_align = channels * bits / 8;
  const int32_t data_size = (int32_t)(n * sizeof(float)), file_size = 36 + data_size, fmt_size = 16;
  const int32_t format = 3;
  fwrite("RIFF", 1, 4, f); fwrite(&file_size, 4, 1, f); fwrite("WAVE", 1, 4, f);
  fwrite("fmt ", 1, 4, f); fwrite(&fmt_size, 4, 1, f);
  fwrite(&format, 2, 1, f); fwrite(&channels, 2, 1, f); fwrite(&sample_rate, 4, 1, f);
  fwrite(&byte_rate, 4, 1, f); fwrite(&block_align, 2, 1, f); fwrite(&bits, 2, 1, f);
  fwrite("data", 1, 4, f); fwrite(&data_size, 4, 1, f);
  fwrite(samples, sizeof(float), (size_t)n, f);
  fclose(f);
  return TTS_OK;
}

// mel frames of a latent of L rows (pure host arithmetic; here so that the session's row probe below has it in every library this file is built into)
extern "C" int tts_diffusion_frames(int L) { return L * 4 * 24000 / 22050; }

// ---- diffusion session: the checks and probes that need no device (tts_diff_session_*) ----
namespace tts {
const char *diff_control_error(int which, double value) {
  switch (which) {
  case 0: return (value != 0 && value != 1 && value != 3) ? "diff_sampler: 0 (ancestral DDPM), 1 (DDIM) or 3 (DPM-Solver++(2M))" : nullptr;
  case 1: return !(value >= 0 && value <= 1) ? "ddim_eta: a value in [0, 1]" : nullptr;
  case 2: return (!std::isfinite(value) || value < 0 || !std::isfinite((float)value)) ? "cond_free_k: a finite value >= 0" : nullptr;
  case 3: return (!std::isfinite(value) || value < 0 || !std::isfinite((float)value)) ? "diff_temperature: a finite value >= 0" : nullptr;
  case 4: return (value != 0 && value != 1) ? "cond_free: 1 (guided) or 0 (unguided: the conditioned sequences only)" : nullptr;
  }
  return "unknown diffusion control";
}
int diff_packed_rows(const int *frames, int n) {
  long long r = 8;
  for (int s = 0; s < n; s++) r = (r + frames[s] + 1 + 7) & ~7LL;
  return (int)((r + 127) & ~127LL);
}
// The struct's growth rule (tts_ar_request's): the size a header before "temperature" declared, or one that covers every field this library knows.
bool diff_request_size_ok(uint32_t n) { return n == offsetof(tts_diff_request, temperature) || n >= sizeof(tts_diff_request); }
int diff_request_check(const tts_diff_request *req, int max_packed_rows, double pinned_temperature, int pinned_cond_free, std::string &why) {
  char buf[240];
  if (!req) { why = "null request"; return TTS_ERR_ARG; }
  if (!diff_request_size_ok(req->struct_size)) {
    snprintf(buf, sizeof buf, "struct_size %u, version 8 declares %zu bytes (%zu before temperature and cond_free were appended; set it to sizeof(tts_diff_request))",
             req->struct_size, sizeof(tts_diff_request), offsetof(tts_diff_request, temperature));
    why = buf;
    return TTS_ERR_ARG;
  }
  if (req->n_cand < 1) { snprintf(buf, sizeof buf, "bad argument (%d candidates)", req->n_cand); why = buf; return TTS_ERR_ARG; }
  if (!req->latents || !req->rows) { why = "null latents or rows"; return TTS_ERR_ARG; }
  if (req->n_cand > 4096) { snprintf(buf, sizeof buf, "%d candidates, at most 4096", req->n_cand); why = buf; return TTS_ERR_LIMIT; }
  size_t n_lat = 0;
  for (int c = 0; c < req->n_cand; c++) {
    if (req->rows[c] < 1 || req->rows[c] > 500) { snprintf(buf, sizeof buf, "latent rows %d out of range (1 .. 500)", req->rows[c]); why = buf; return TTS_ERR_ARG; }
    n_lat += (size_t)req->rows[c] * TTS_DMODEL;
  }
  if (req->n_steps < 2) { snprintf(buf, sizeof buf, "n_steps %d: at least 2", req->n_steps); why = buf; return TTS_ERR_ARG; }
  const bool grown = req->struct_size >= sizeof(tts_diff_request); // an older caller's struct ends before the two fields
  const double v[5] = {(double)req->sampler, req->ddim_eta, req->cond_free_k, grown ? req->temperature : pinned_temperature,
                       grown ? (double)req->cond_free : (double)pinned_cond_free};
  for (int k = 0; k < 5; k++)
    if (const char *e = diff_control_error(k, v[k])) { why = e; return TTS_ERR_ARG; }
  for (size_t i = 0; i < n_lat; i++)
    if (!std::isfinite(req->latents[i])) { why = "a latent holds a non-finite value"; return TTS_ERR_ARG; }
  if (req->voice_latent2048)
    for (int i = 0; i < 2 * TTS_DMODEL; i++)
      if (!std::isfinite(req->voice_latent2048[i])) { why = "the voice latent holds a non-finite value"; return TTS_ERR_ARG; }
  const int need = tts_host_diff_packed_rows_ex(req->rows, req->n_cand, (int)v[4]);
  if (need > max_packed_rows) { snprintf(buf, sizeof buf, "the request takes %d packed rows, %d are free", need, max_packed_rows); why = buf; return TTS_ERR_LIMIT; }
  return TTS_OK;
}
} // namespace tts
extern "C" int tts_host_diff_packed_rows(const int32_t *latent_rows, int n_cand) { return tts_host_diff_packed_rows_ex(latent_rows, n_cand, 1); }
extern "C" int tts_host_diff_packed_rows_ex(const int32_t *latent_rows, int n_cand, int cond_free) {
  if (!latent_rows || n_cand < 1 || n_cand > 4096 || (cond_free != 0 && cond_free != 1)) return TTS_ERR_ARG;
  std::vector<int> frames;
  for (int pass = 0; pass < 1 + cond_free; pass++) // the conditioned sequences, then (guided) their unconditioned copies
    for (int c = 0; c < n_cand; c++) {
      if (latent_rows[c] < 1 || latent_rows[c] > 500) return TTS_ERR_ARG;
      frames.push_back(tts_diffusion_frames(latent_rows[c]));
    }
  return tts::diff_packed_rows(frames.data(), (int)frames.size());
}
extern "C" int tts_host_diff_request_check(const tts_diff_request *req, int max_packed_rows) {
  if (max_packed_rows < 1) return TTS_ERR_ARG;
  std::string why;
  return tts::diff_request_check(req, max_packed_rows, 1.0, 1, why);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Audio front-end on the device (csrc/audio_frontend.hip): the tables its kernels read, each evaluated in double here and rounded ONCE to float, and the
// WAV reader. The mel side restates the functions above (mel_filterbank, the periodic Hann window) as tables; the resampler is upstream's
// torchaudio.functional.resample with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).
// ------------------------------------------------------------------------------------------------------------------------------
namespace tts {
static int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }
// o = orig / gcd, n = new / gcd, width = ceil(6 o / base), base = min(o, n) 0.99; the table is [n][2 width + o]
int afe_resample_geometry(int orig_rate, int new_rate, AfeResampleGeom *g) {
  if (orig_rate < 1 || new_rate < 1 || !g) return TTS_ERR_ARG;
  const int64_t d = gcd64(orig_rate, new_rate);
  g->o = (int)(orig_rate / d); g->n = (int)(new_rate / d);
  const double base = std::min(g->o, g->n) * 0.99;
  g->width = (int)std::ceil(6.0 * g->o / base);
  g->taps = 2 * g->width + g->o;
  return (int64_t)g->n * g->taps > AFE_MAX_TABLE ? TTS_ERR_LIMIT : TTS_OK;
}
// tab[p][k] = sinc(pi t) cos^2(pi t / 12) base / o with t = clamp((-p / n + (k - width) / o) base, -6, 6)
void afe_resample_table(const AfeResampleGeom &g, float *tab) {
  const double base = std::min(g.o, g.n) * 0.99, scale = base / g.o;
  for (int p = 0; p < g.n; p++)
    for (int k = 0; k < g.taps; k++) {
      double t = (-(double)p / g.n + (double)(k - g.width) / g.o) * base;
      t = std::max(-6.0, std::min(6.0, t));
      const double win = std::cos(t * M_PI / 6.0 / 2.0), a = t * M_PI;
      tab[(size_t)p * g.taps + k] = (float)((a == 0.0 ? 1.0 : std::sin(a) / a) * win * win * scale);
    }
}
int64_t afe_resample_len(const AfeResampleGeom &g, int64_t n) { return (g.n * n + g.o - 1) / g.o; }
// tw[k] = (cos, -sin)(2 pi k / 1024), k < 512; win[i] = periodic Hann
void afe_fft_tables(float *tw_re, float *tw_im, float *win) {
  for (int k = 0; k < 512; k++) { tw_re[k] = (float)std::cos(-2.0 * M_PI * k / 1024.0); tw_im[k] = (float)std::sin(-2.0 * M_PI * k / 1024.0); }
  for (int i = 0; i < 1024; i++) win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * i / 1024.0));
}
// The filterbank of `bands` (80: HTK scale, 22 050 Hz, 0 .. 8 000 Hz; 100: Slaney scale, 24 000 Hz, 0 .. 12 000 Hz), Slaney-normalised, as its non-zero span per
// band: span[b] = {first bin, bin count, offset into w}. A band whose triangle holds no bin has count 0.
int afe_filterbank(int bands, std::vector<int> &span, std::vector<float> &w) {
  if (bands != 80 && bands != 100) return TTS_ERR_ARG;
  const std::vector<double> fb = bands == 80 ? mel_filterbank(80, 1024, 22050.0, 0.0, 8000.0, true) : mel_filterbank(100, 1024, 24000.0, 0.0, 12000.0, false);
  span.assign((size_t)3 * bands, 0);
  w.clear();
  for (int b = 0; b < bands; b++) {
    int lo = 513, hi = -1;
    for (int k = 0; k < 513; k++)
      if (fb[(size_t)b * 513 + k] != 0.0) { lo = std::min(lo, k); hi = k; }
    span[3 * b] = hi < 0 ? 0 : lo; span[3 * b + 1] = hi < 0 ? 0 : hi - lo + 1; span[3 * b + 2] = (int)w.size();
    for (int k = lo; k <= hi; k++) w.push_back((float)fb[(size_t)b * 513 + k]);
  }
  return TTS_OK;
}
} // namespace tts

// The inverse of tts_write_wav: RIFF/WAVE with PCM16, PCM24 or float32 samples (format 1 or 3, or WAVE_FORMAT_EXTENSIBLE with one of those as its sub-format),
// any channel count (averaged), unknown chunks skipped (a chunk of odd size is followed by a pad byte).
extern "C" int64_t tts_read_wav(const char *path, float *out, int64_t cap, int32_t *sample_rate) {
  if (!path) return TTS_ERR_ARG;
  FILE *f = fopen(path, "rb");
  if (!f) return TTS_ERR_IO;
  struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
  unsigned char h[12];
  if (fread(h, 1, 12, f) != 12) return TTS_ERR_IO;
  if (memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) return TTS_ERR_FORMAT;
  int fmt = 0, channels = 0, bits = 0, rate = 0;
  auto u16 = [](const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); };
  auto u32 = [](const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); };
  for (;;) {
    unsigned char ch[8];
    if (fread(ch, 1, 8, f) != 8) return fmt ? TTS_ERR_IO : TTS_ERR_FORMAT; // the file ends before its data chunk
    const uint32_t size = u32(ch + 4);
    if (!memcmp(ch, "fmt ", 4)) {
      unsigned char b[40] = {};
      if (size < 16) return TTS_ERR_FORMAT;
      const size_t take = std::min<size_t>(size, sizeof b);
      if (fread(b, 1, take, f) != take) return TTS_ERR_IO;
      fmt = (int)u16(b); channels = (int)u16(b + 2); rate = (int)u32(b + 4); bits = (int)u16(b + 14);
      if (fmt == 0xFFFE && take >= 26) fmt = (int)u16(b + 24); // WAVE_FORMAT_EXTENSIBLE: the first two bytes of the sub-format GUID
      if (fseek(f, (long)(size - take + (size & 1)), SEEK_CUR)) return TTS_ERR_IO;
    } else if (!memcmp(ch, "data", 4)) {
      if (!fmt) return TTS_ERR_FORMAT;
      if (channels < 1 || rate < 1 || !((fmt == 1 && (bits == 16 || bits == 24)) || (fmt == 3 && bits == 32))) return TTS_ERR_FORMAT;
      const int bps = bits / 8;
      const int64_t frames = (int64_t)(size / ((uint32_t)bps * channels));
      if (sample_rate) *sample_rate = rate;
      if (!out) { // the count the file can deliver: a data chunk longer than the file is a truncated file
        const long at = ftell(f);
        if (at < 0 || fseek(f, 0, SEEK_END)) return TTS_ERR_IO;
        return ftell(f) - at < frames * bps * channels ? TTS_ERR_IO : frames;
      }
      if (cap < frames) return TTS_ERR_ARG;
      std::vector<unsigned char> row((size_t)bps * channels);
      for (int64_t i = 0; i < frames; i++) {
        if (fread(row.data(), 1, row.size(), f) != row.size()) return TTS_ERR_IO;
        double a = 0;
        for (int c = 0; c < channels; c++) {
          const unsigned char *p = row.data() + (size_t)c * bps;
          if (fmt == 3) { float v; memcpy(&v, p, 4); a += v; }
          else if (bits == 16) a += (int16_t)u16(p) / 32768.0;
          else a += ((int32_t)((uint32_t)p[0] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 24) >> 8) / 8388608.0; // sign-extended from bit 23
        }
        out[i] = (float)(a / channels);
      }
      return frames;
    } else if (fseek(f, (long)(size + (size & 1)), SEEK_CUR)) return TTS_ERR_IO;
  }
}

// ---- alignment and redaction: the host half of the wav2vec2 CTC aligner (aligner.h). The project's statement of upstream tortoise-tts' Wav2VecAlignment rules
// (max_alignment, align, redact), from memory: unpinned against upstream, pinned to the Python restatement of tests/aligner_ref.py. Text is UTF-8 and a
// "character" is one code point; lower() folds 'A' .. 'Z' only. ----
namespace tts {

int utf8_decode(const char *s, std::vector<int32_t> &out) {
  out.clear();
  if (!s) return TTS_ERR_ARG;
  const unsigned char *p = (const unsigned char *)s;
  while (*p) {
    int32_t c = *p++;
    int more = c < 0x80 ? 0 : (c >> 5) == 6 ? 1 : (c >> 4) == 14 ? 2 : (c >> 3) == 30 ? 3 : -1;
    if (more < 0) return TTS_ERR_ARG;
    if (more) c &= 0x3f >> more;
    for (int i = 0; i < more; i++) {
      if ((*p & 0xc0) != 0x80) return TTS_ERR_ARG;
      c = c << 6 | (*p++ & 0x3f);
    }
    out.push_back(c);
  }
  return (int)out.size();
}

void utf8_encode(const std::vector<int32_t> &cp, std::string &out) {
  out.clear();
  for (int32_t c : cp) {
    if (c < 0x80) out += (char)c;
    else if (c < 0x800) { out += (char)(0xc0 | c >> 6); out += (char)(0x80 | (c & 0x3f)); }
    else if (c < 0x10000) { out += (char)(0xe0 | c >> 12); out += (char)(0x80 | (c >> 6 & 0x3f)); out += (char)(0x80 | (c & 0x3f)); }
    else { out += (char)(0xf0 | c >> 18); out += (char)(0x80 | (c >> 12 & 0x3f)); out += (char)(0x80 | (c >> 6 & 0x3f)); out += (char)(0x80 | (c & 0x3f)); }
  }
}

// CTC decode: collapse runs of equal ids, drop the blank and every token without a character (-1), map the rest through the vocabulary
int ctc_decode(const int32_t *ids, int n_frames, const int32_t *vocab, int n_vocab, int blank, std::vector<int32_t> &out, std::string &err) {
  out.clear();
  if (n_frames < 0 || (n_frames && !ids) || !vocab || n_vocab < 1) { err = "ctc_decode: bad argument"; return TTS_ERR_ARG; }
  for (int i = 0; i < n_frames; i++) {
    if (ids[i] < 0 || ids[i] >= n_vocab) { err = "ctc_decode: frame " + std::to_string(i) + " holds id " + std::to_string(ids[i]) + " outside the vocabulary"; return TTS_ERR_ARG; }
    if (i && ids[i] == ids[i - 1]) continue;
    if (ids[i] == blank || vocab[ids[i]] < 0) continue;
    out.push_back(vocab[ids[i]]);
  }
  return (int)out.size();
}

// max_alignment(s1, s2): s1 with every character that s2 cannot account for, in order, replaced by '~'. The recursion
//   s1 empty -> "";  s2 empty -> '~' x len(s1);  s1[0] == s2[0] -> s1[0] + f(s1[1:], s2[1:]);
//   else a = f(s1, s2[1:]), b = '~' + f(s1[1:], s2): a if it has strictly more non-'~' characters than b, else b
// memoised on the two lengths, here as the table of its non-'~' counts filled from the ends, then one walk from the front taking the recursion's choices.
int max_alignment(const std::vector<int32_t> &s1, const std::vector<int32_t> &s2, std::vector<int32_t> &out, std::string &err) {
  out.clear();
  for (int32_t c : s1)
    if (c == '~') { err = "max_alignment: the text holds '~', the mark of an unaligned character"; return TTS_ERR_ARG; }
  const size_t n1 = s1.size(), n2 = s2.size();
  if ((n1 + 1) * (n2 + 1) > ((size_t)1 << 28)) { err = "max_alignment: the strings are too long"; return TTS_ERR_LIMIT; }
  std::vector<int32_t> cnt((n1 + 1) * (n2 + 1), 0); // cnt[i][j]: non-'~' characters of f(s1[i:], s2[j:])
  auto at = [&](size_t i, size_t j) -> int32_t & { return cnt[i * (n2 + 1) + j]; };
  for (size_t i = n1; i-- > 0;)
    for (size_t j = n2; j-- > 0;)
      at(i, j) = s1[i] == s2[j] ? 1 + at(i + 1, j + 1) : std::max(at(i, j + 1), at(i + 1, j));
  size_t i = 0, j = 0;
  while (i < n1) {
    if (j == n2) { out.push_back('~'); i++; }
    else if (s1[i] == s2[j]) { out.push_back(s1[i]); i++; j++; }
    else if (at(i, j + 1) > at(i + 1, j)) j++;
    else { out.push_back('~'); i++; }
  }
  return (int)out.size();
}

// One sample offset per character of `text`, in samples of a clip of n_samples whose frames carry `ids`.
int ctc_align(const int32_t *ids, int n_frames, const int32_t *vocab, int n_vocab, int blank, const std::vector<int32_t> &text, int64_t n_samples,
              std::vector<int64_t> &al, std::string &err) {
  al.clear();
  if (n_frames < 1 || !ids || !vocab || n_vocab < 1 || n_samples < 1) { err = "ctc_align: bad argument"; return TTS_ERR_ARG; }
  if (text.empty()) return 0;
  std::vector<int32_t> low(text), pred, fixed;
  for (int32_t &c : low)
    if (c >= 'A' && c <= 'Z') c += 32;
  int rc = ctc_decode(ids, n_frames, vocab, n_vocab, blank, pred, err);
  if (rc < 0) return rc;
  if ((rc = max_alignment(low, pred, fixed, err)) < 0) return rc;
  // nothing of the text was heard: upstream's rule would place nothing and interpolate every offset between 0 and n_samples; here it is the failure
  if (std::all_of(fixed.begin(), fixed.end(), [](int32_t c) { return c == '~'; })) { err = "the text does not match the audio"; return TTS_ERR_ARG; }
  auto token = [&](int32_t cp) { // the vocabulary id of a character: the first token that carries it, -1 for none
    for (int v = 0; v < n_vocab; v++)
      if (vocab[v] == cp) return v;
    return -1;
  };
  const int64_t step = n_samples / n_frames;
  const size_t n = fixed.size();
  al.assign(n, -1);
  al[0] = 0; // character 0 sits at offset 0
  size_t next = 1;
  while (next < n && fixed[next] == '~') next++; // the '~' passed on the way stay open
  for (int f = 0; f < n_frames && next < n; f++)
    if (ids[f] == token(fixed[next])) {
      al[next++] = (int64_t)f * step;
      while (next < n && fixed[next] == '~') next++;
    }
  if (next < n) { al.clear(); err = "the text does not match the audio"; return TTS_ERR_ARG; }
  // open offsets: linear between the placed neighbour before and the next placed one (n_samples behind the end), integer floor
  for (size_t i = 1; i < n; i++) {
    if (al[i] != -1) continue;
    size_t nf = i + 1;
    while (nf < n && al[nf] == -1) nf++;
    const int64_t hi = nf < n ? al[nf] : n_samples, lo = al[i - 1], gap = hi - lo;
    for (size_t j = i; j < nf; j++) {
      const int64_t num = (int64_t)(j - i + 1) * gap, den = (int64_t)(nf - i + 1);
      al[j] = (num >= 0 ? num / den : -((-num + den - 1) / den)) + lo;
    }
  }
  return (int)n;
}

// The text without its brackets, and the kept intervals {first character, last character} (indices into the bare text) of every non-empty unbracketed
// piece: upstream's non_redacted_intervals.
int redact_spans(const std::vector<int32_t> &text, std::vector<int32_t> &clean, std::vector<int32_t> &iv, std::string &err) {
  clean.clear(); iv.clear();
  bool inside = false;
  int32_t piece0 = 0;
  auto close_piece = [&] {
    if ((int32_t)clean.size() > piece0) { iv.push_back(piece0); iv.push_back((int32_t)clean.size() - 1); }
  };
  for (int32_t c : text) {
    if (c == '[') {
      if (inside) { err = "nested '[' in the text"; return TTS_ERR_ARG; }
      close_piece();
      inside = true;
    } else if (c == ']') {
      if (!inside) { err = "']' without '[' in the text"; return TTS_ERR_ARG; }
      inside = false;
      piece0 = (int32_t)clean.size();
    } else clean.push_back(c);
  }
  if (inside) { err = "'[' without ']' in the text"; return TTS_ERR_ARG; }
  close_piece();
  return (int)iv.size() / 2;
}

static int put_utf8(const std::vector<int32_t> &cp, char *out, int cap) {
  std::string s;
  utf8_encode(cp, s);
  if (!out || cap < (int)s.size() + 1) return TTS_ERR_ARG;
  memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

} // namespace tts

extern "C" int tts_host_ctc_decode(const int32_t *ids, int n_frames, const int32_t *vocab, int n_vocab, int blank, char *out, int cap) {
  std::vector<int32_t> cp;
  std::string err;
  const int rc = tts::ctc_decode(ids, n_frames, vocab, n_vocab, blank, cp, err);
  return rc < 0 ? rc : tts::put_utf8(cp, out, cap);
}
extern "C" int tts_host_max_alignment(const char *s1, const char *s2, char *out, int cap) {
  std::vector<int32_t> a, b, r;
  std::string err;
  if (tts::utf8_decode(s1, a) < 0 || tts::utf8_decode(s2, b) < 0) return TTS_ERR_ARG;
  const int rc = tts::max_alignment(a, b, r, err);
  return rc < 0 ? rc : tts::put_utf8(r, out, cap);
}
extern "C" int tts_host_ctc_align(const int32_t *ids, int n_frames, const int32_t *vocab, int n_vocab, int blank, const char *text, int64_t n_samples,
                                  int64_t *offsets_out, int cap) {
  std::vector<int32_t> t;
  std::vector<int64_t> al;
  std::string err;
  if (tts::utf8_decode(text, t) < 0) return TTS_ERR_ARG;
  const int rc = tts::ctc_align(ids, n_frames, vocab, n_vocab, blank, t, n_samples, al, err);
  if (rc < 0) return rc;
  if (rc > cap || (rc && !offsets_out)) return TTS_ERR_ARG;
  for (int i = 0; i < rc; i++) offsets_out[i] = al[i];
  return rc;
}
extern "C" int tts_host_redact_spans(const char *text, char *clean_out, int cap, int32_t *intervals_out, int cap_intervals) {
  std::vector<int32_t> t, clean, iv;
  std::string err;
  if (tts::utf8_decode(text, t) < 0) return TTS_ERR_ARG;
  const int rc = tts::redact_spans(t, clean, iv, err);
  if (rc < 0) return rc;
  if (rc > cap_intervals || (rc && !intervals_out)) return TTS_ERR_ARG;
  if (tts::put_utf8(clean, clean_out, cap) < 0) return TTS_ERR_ARG;
  for (size_t i = 0; i < iv.size(); i++) intervals_out[i] = iv[i];
  return rc;
}

// ---- random voices (random_voice.h): the load-time fold and the blend of several voices ----
namespace tts {
void rlg_fold(const float *w, const float *b, int dim, int equal, float *w_out, float *b_out) {
  const size_t nw = (size_t)dim * dim;
  if (!equal) {
    if (w_out != w) memcpy(w_out, w, nw * sizeof(float));
    if (b_out != b) memcpy(b_out, b, (size_t)dim * sizeof(float));
    return;
  }
  const double lr_mul_d = 0.1;
  const float lr_mul = (float)lr_mul_d, scale = (float)(lr_mul_d / std::sqrt((double)dim));
  for (size_t i = 0; i < nw; i++) w_out[i] = w[i] * scale;
  for (int i = 0; i < dim; i++) b_out[i] = b[i] * lr_mul;
}
} // namespace tts
extern "C" int tts_host_random_voice_fold(const float *w, const float *b, int dim, int equal, float *w_out, float *b_out) {
  if (!w || !b || !w_out || !b_out || dim < 1 || dim > 65536) return TTS_ERR_ARG;
  tts::rlg_fold(w, b, dim, equal, w_out, b_out);
  return TTS_OK;
}
// upstream's load_voices rule for several named voices (the mean of their latents), generalised to weights: out[i] = sum_v w[v] x[v][i] / sum_v w[v],
// accumulated in double in voice order, rounded once
extern "C" int tts_host_blend_voices(const float *latents, const float *weights, int n, int dim, float *out) {
  if (!latents || !out || n < 1 || dim < 1) return TTS_ERR_ARG;
  double wsum = 0;
  for (int v = 0; v < n; v++) {
    const double wv = weights ? (double)weights[v] : 1.0;
    if (!std::isfinite(wv)) return TTS_ERR_ARG;
    wsum += wv;
  }
  if (!(wsum > 0) || !std::isfinite(wsum)) return TTS_ERR_ARG;
  for (size_t i = 0; i < (size_t)n * dim; i++)
    if (!std::isfinite(latents[i])) return TTS_ERR_ARG;
  for (int i = 0; i < dim; i++) {
    double a = 0;
    for (int v = 0; v < n; v++) a += (weights ? (double)weights[v] : 1.0) * (double)latents[(size_t)v * dim + i];
    out[i] = (float)(a / wsum);
  }
  return TTS_OK;
}
