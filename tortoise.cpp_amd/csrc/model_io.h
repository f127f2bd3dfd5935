// Host scaffolding of the add-on models in hifigan.hip's translation unit (HiFi-GAN, BigVGAN, classifier, aligner, DVAE), stated once:
//   ModelReader   a model file's tensors by name and PyTorch shape, repacked into plain float vectors for the kernels
//   DevWeights    those vectors on the device, owned by the model's state
//   LevelTable    the per-level HFG_SEQ records of a ragged batch of clips
//   ClipIngest    a batch of clips at any sample rate -> checked, uploaded and brought to the model's rate (classifier, aligner)
// Included once, in hifigan.hip behind its kernels (HFG_SEQ is declared there); no kernel lives here.
#pragma once

namespace tts {

struct HostLayer { std::vector<float> w, b; };          // a repacked weight and its bias; a norm's gamma and beta; any pair of vectors
struct HfgLayer { float *w = nullptr, *b = nullptr; }; // the same pair on the device

struct ModelReader {
  const WeightFile &wf;
  tts_ctx *ctx;
  const char *model; // as the messages name it: "HiFi-GAN", "BigVGAN", "classifier", "aligner", "DVAE"
  size_t known = 0;  // tensors accepted so far; a parser that checks a tensor in words of its own counts it here

  bool has(const std::string &name) const { return wf.has(name); }
  // the tensor if the file holds it (with nd dimensions, when nd is given): for reading a configuration off the shapes
  const HostTensor *peek(const std::string &name, int nd = 0) const {
    auto it = wf.t.find(name);
    return it != wf.t.end() && (!nd || it->second.n_dims == nd) ? &it->second : nullptr;
  }
  // PyTorch shape [d0][d1][d2] = container ne {d2, d1, d0}; d2 = 0: [d0][d1]; d1 = 0: a vector of d0. Null after fail().
  const HostTensor *need(const std::string &name, int64_t d0, int64_t d1, int64_t d2) {
    auto it = wf.t.find(name);
    if (it == wf.t.end()) { fail(ctx, TTS_ERR_FORMAT, "tensor '%s' missing from %s model file", name.c_str(), model); return nullptr; }
    const HostTensor &t = it->second;
    const int nd = d2 ? 3 : d1 ? 2 : 1;
    const int64_t want[3] = {nd == 3 ? d2 : nd == 2 ? d1 : d0, nd == 3 ? d1 : nd == 2 ? d0 : 1, nd == 3 ? d0 : 1};
    bool ok = t.n_dims == nd && (int64_t)t.data.size() == t.nelem();
    for (int i = 0; i < nd && ok; i++) ok = t.ne[i] == want[i];
    if (!ok) {
      fail(ctx, TTS_ERR_FORMAT, "tensor '%s' has wrong shape in %s model file: got [%d, %d, %d] (%d dims), expected [%d, %d, %d]", name.c_str(), model,
           (int)t.ne[0], (int)t.ne[1], (int)t.ne[2], t.n_dims, (int)want[0], (int)want[1], (int)want[2]);
      return nullptr;
    }
    known++;
    return &t;
  }
  // <p>.weight [d0][d1][d2] as the file stores it, <p>.bias [d0]
  int raw(const std::string &p, int64_t d0, int64_t d1, int64_t d2, HostLayer &l) {
    const HostTensor *w, *b;
    if (!(w = need(p + ".weight", d0, d1, d2)) || !(b = need(p + ".bias", d0, 0, 0))) return TTS_ERR_FORMAT;
    l.w = w->data; l.b = b->data;
    return TTS_OK;
  }
  // Conv1d [cout][cin][k] -> [k][cinp][coutp], the bias -> [coutp]: zero where a padded channel is an operand or a result (0: no padding)
  int conv(const std::string &p, int cout, int cin, int k, HostLayer &l, int coutp = 0, int cinp = 0) {
    const HostTensor *w, *b;
    if (!(w = need(p + ".weight", cout, cin, k)) || !(b = need(p + ".bias", cout, 0, 0))) return TTS_ERR_FORMAT;
    if (!coutp) coutp = cout;
    if (!cinp) cinp = cin;
    l.w.assign((size_t)k * cinp * coutp, 0.f);
    for (int co = 0; co < cout; co++)
      for (int ci = 0; ci < cin; ci++)
        for (int j = 0; j < k; j++) l.w[((size_t)j * cinp + ci) * coutp + co] = w->data[((size_t)co * cin + ci) * k + j];
    l.b.assign(coutp, 0.f);
    std::copy(b->data.begin(), b->data.end(), l.b.begin());
    return TTS_OK;
  }
  // Linear [cout][cin] -> [cin][cout]
  int linear(const std::string &p, int cout, int cin, HostLayer &l) {
    const HostTensor *w, *b;
    if (!(w = need(p + ".weight", cout, cin, 0)) || !(b = need(p + ".bias", cout, 0, 0))) return TTS_ERR_FORMAT;
    l.w.resize((size_t)cin * cout);
    for (int co = 0; co < cout; co++)
      for (int ci = 0; ci < cin; ci++) l.w[(size_t)ci * cout + co] = w->data[(size_t)co * cin + ci];
    l.b = b->data;
    return TTS_OK;
  }
  // two vectors of c: <p><a> -> l.w, <p><b> -> l.b (a norm: ".weight", ".bias")
  int vec_pair(const std::string &p, const char *a, const char *b, int c, HostLayer &l) {
    const HostTensor *ta, *tb;
    if (!(ta = need(p + a, c, 0, 0)) || !(tb = need(p + b, c, 0, 0))) return TTS_ERR_FORMAT;
    l.w = ta->data; l.b = tb->data;
    return TTS_OK;
  }
  int norm(const std::string &p, int c, HostLayer &l) { return vec_pair(p, ".weight", ".bias", c, l); }
  // every tensor of the file was asked for
  int finish(const char *path) const {
    if (wf.t.size() == known) return TTS_OK;
    return fail(ctx, TTS_ERR_FORMAT, "unknown tensors in %s model file '%s' (%d tensors, %d expected)", model, path, (int)wf.t.size(), (int)known);
  }
};

// The device copies of a model's vectors; freed with the state that holds it.
struct DevWeights {
  std::vector<void *> owned;
  DevWeights() = default;
  DevWeights(const DevWeights &) = delete;
  DevWeights &operator=(const DevWeights &) = delete;
  ~DevWeights() { for (void *p : owned) (void)hipFree(p); }
  int up(tts_ctx *ctx, const std::vector<float> &src, float **dst) {
    void *p = nullptr;
    TTS_HIP(ctx, hipMalloc(&p, src.size() * 4));
    owned.push_back(p);
    TTS_HIP(ctx, hipMemcpy(p, src.data(), src.size() * 4, hipMemcpyHostToDevice));
    *dst = (float *)p;
    return TTS_OK;
  }
  int up(tts_ctx *ctx, const HostLayer &s, HfgLayer &d) { int e = up(ctx, s.w, &d.w); return e ? e : up(ctx, s.b, &d.b); }
};

// The HFG_SEQ records of B clips on L levels, level by level: record (l, s) = {first row, rows, 0, first statistics tile, unit x the clip's first row on
// level 0}; ints 3 and 4 on level 0 only unless `every_level`.
struct LevelTable {
  int B = 0;
  std::vector<int> tab;             // [L][B][HFG_SEQ]
  std::vector<int64_t> rows, tiles; // of a level: the rows with their padding, the statistics tiles
  std::vector<int> max_n;           // of a level: the longest clip
  const int *rec(int l, int s) const { return &tab[((size_t)l * B + s) * HFG_SEQ]; }
};
// n0[s]: rows of clip s on level 0; next(n, l): rows on level l + 1 of a clip with n on level l; a clip's first row is a multiple of `align` (1: the clips are
// packed without gaps); tile: rows of a statistics tile (0: no tiles)
template <class T, class Next>
LevelTable level_table(const T *n0, int B, int L, Next next, int align, int tile, bool every_level, int unit = 1) {
  LevelTable t;
  t.B = B;
  t.tab.assign((size_t)L * B * HFG_SEQ, 0); t.rows.assign(L, 0); t.tiles.assign(L, 0); t.max_n.assign(L, 0);
  for (int s = 0; s < B; s++) {
    const int64_t first0 = t.rows[0];
    int64_t n = n0[s];
    for (int l = 0; l < L; l++) {
      int *q = &t.tab[((size_t)l * B + s) * HFG_SEQ];
      q[0] = (int)t.rows[l]; q[1] = (int)n;
      if (l == 0 || every_level) { q[3] = (int)t.tiles[l]; q[4] = (int)(unit * first0); }
      t.rows[l] += (n + align - 1) / align * align; t.max_n[l] = std::max(t.max_n[l], (int)n);
      if (tile) t.tiles[l] += (n + tile - 1) / tile;
      if (l + 1 < L) n = next(n, l);
    }
  }
  return t;
}

// A batch of clips for a model that reads `rate` Hz: clip s has n_samples[s] samples at rates[s] Hz, back to back in `audio`.
struct ClipIngest {
  std::vector<ClsResampleClip> rs;     // the clips the resampler converts
  std::vector<int64_t> src_off, n_dst; // of a clip: its first sample in `audio`; its samples at `rate` Hz, cropped
  int64_t total_src = 0, total_dst = 0; // samples of all clips: in `audio`; at `rate` Hz with every clip's first sample at a multiple of 8
  std::vector<float> up;               // samples | tables: clip_upload's staging, which outlives the asynchronous copy
};
// Every check of the clips, in the order the callers' callers rely on: per clip its length, its rate, its length at `rate` Hz (at most `crop` samples are
// ever computed; 0: all of them), then per_clip(s, samples at `rate` Hz), the model's own checks; then the total; then the samples themselves.
template <class PerClip>
int clip_ingest(tts_ctx *ctx, const char *fn, const float *audio, const int64_t *n_samples, const int32_t *rates, int B, int rate, int64_t crop, ClipIngest &g,
                PerClip per_clip) {
  g.src_off.resize(B); g.n_dst.resize(B);
  for (int s = 0; s < B; s++) {
    const int64_t n = n_samples[s];
    if (n < 1) return fail(ctx, TTS_ERR_ARG, "%s: clip %d: %lld samples", fn, s, (long long)n);
    if (n > (1 << 26)) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %lld samples, at most 2^26", fn, s, (long long)n);
    AfeResampleGeom geom;
    if (rates[s] < 1 || afe_resample_geometry(rates[s], rate, &geom) != TTS_OK)
      return fail(ctx, TTS_ERR_ARG, "%s: clip %d: sample rate %d is outside the audio front end's range", fn, s, rates[s]);
    g.src_off[s] = g.total_src;
    int64_t nd = rates[s] == rate ? n : afe_resample_len(geom, n);
    if (crop) nd = std::min(nd, crop);
    g.n_dst[s] = nd;
    if (nd > (1 << 26)) return fail(ctx, TTS_ERR_LIMIT, "%s: clip %d: %lld samples at %d kHz, at most 2^26", fn, s, (long long)nd, rate / 1000);
    const int rc = per_clip(s, nd);
    if (rc) return rc;
    if (rates[s] != rate) g.rs.push_back(ClsResampleClip{g.total_src, n, g.total_dst, nd, rates[s]});
    g.total_src += n; g.total_dst += (nd + 7) / 8 * 8;
  }
  if (g.total_dst > (1ll << 30)) return fail(ctx, TTS_ERR_LIMIT, "%s: %lld samples at %d kHz in one call, at most 2^30", fn, (long long)g.total_dst, rate / 1000);
  for (int64_t i = 0; i < g.total_src; i++)
    if (!std::isfinite(audio[i])) return fail(ctx, TTS_ERR_ARG, "%s: the audio holds a non-finite sample (element %lld)", fn, (long long)i);
  return TTS_OK;
}
// Floats of clip_upload's transfer: what the caller reserves `in` for
inline size_t clip_upload_floats(const ClipIngest &g, const LevelTable &t) { return (size_t)g.total_src + t.tab.size(); }
// One transfer (samples | tables) into `in`; then the clips at `rate` Hz in `wav`, clip s at its level-0 record's int 4: a clip already at `rate` Hz reaches
// the network bit for bit, the others go through the audio front end's resampler, one stage. *d_tab: the tables on the device.
inline int clip_upload(tts_ctx *ctx, ClipIngest &g, const LevelTable &t, const float *audio, const int32_t *rates, int rate, DevBuf &in, float *wav,
                       ClsResampleFn resample, const int **d_tab) {
  g.up.resize(clip_upload_floats(g, t));
  memcpy(g.up.data(), audio, (size_t)g.total_src * 4);
  memcpy(g.up.data() + g.total_src, t.tab.data(), t.tab.size() * 4);
  TTS_HIP(ctx, hipMemcpyAsync(in.p, g.up.data(), g.up.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  const float *d_src = in.as<float>();
  *d_tab = (const int *)(d_src + g.total_src);
  for (int s = 0; s < t.B; s++)
    if (rates[s] == rate)
      TTS_HIP(ctx, hipMemcpyAsync(wav + t.rec(0, s)[4], d_src + g.src_off[s], (size_t)g.n_dst[s] * 4, hipMemcpyDeviceToDevice, ctx->stream));
  return g.rs.empty() ? TTS_OK : resample(ctx, d_src, wav, g.rs.data(), (int)g.rs.size());
}

} // namespace tts
