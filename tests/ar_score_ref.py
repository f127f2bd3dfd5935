"""The float64 reference of AR scoring (csrc/ar_score.h: ar_score_kernel + ar_score_reduce_kernel; tts_ar_score_codes), in two spellings, the derived bounds, a
float32 restatement in the kernel's order with seeded defects, and the row table restated in Python.

What is scored: for every row r of hn [R][K] and a target tgt[r]
    logit[r][v] = b[v] + hn[r] . W[:, v], v < N;  lse[r] = log sum_v exp(logit[r][v]);  logit[r][tgt[r]];  logit[r][N - 1] (stop);  argmax_v (lowest index on a tie)
The columns N .. NPAD - 1 of W and b are padding and never count.

The bounds (U = 2^-24, gamma(n) = n U / (1 - n U); nothing here is taken from what the kernel gives):
  logit   one fmaf per channel from 0 and one addition of the bias: |fl - exact| <= gamma(K + 1) (sum_k |x_k| |w_kv| + |b_v|) = B_logit[r][v];  B_dot[r] = max_v.
  lse     is 1-Lipschitz in the sup norm of the logits: B_dot[r], plus the rounding of the exp / sum / log chain on the computed logits. A term exp(l_i - M)
          reaches the sum through at most three subtractions whose differences add up to y_i = l_i - M <= 0 (lane -> wave maximum, wave -> workgroup, slab -> row:
          each rounds to U |difference| and moves its exponential by that much, relatively), three expf (accurate, taken as <= 2 ulp = 4 U each), two products
          (U each): relative error <= U (|y_i| + 16). The additions (two columns, 5 tree levels, 4 waves, the slabs; rounded up) add gamma(12 + slabs + 3) on the sum. So
          rel_S[r] = sum_i U (|y_i| + 16) e^{y_i} / S + gamma(12 + slabs + 3), and the logarithm turns a relative error of S into an absolute one, rel_S / (1 - rel_S),
          plus logf's own 4 U |log S| and the addition M + log S: U |lse|.
  logp    B_logit[r][tgt] + B_lse[r] + U |logp| (the subtraction).
  argmax  compared on rows whose float64 top-1 margin exceeds 2 B_dot[r] (both logits may move by B_dot); planted exact ties are compared always."""
import numpy as np

f32, f64, i32 = np.float32, np.float64, np.int32
U = 2.0 ** -24
SLAB, TILE = 256, 64
MAX_LEFT_OUT = 0.05  # the share of rows the argmax margin may leave out (a condition on the reference alone)


def gamma(n):
    return n * U / (1.0 - n * U)


def logits64(hn, W, b, N):
    """(float64 logits [R][N] of the float32 values, B_logit [R][N])"""
    x, w, bb = hn.astype(f64), W[:, :N].astype(f64), b[:N].astype(f64)
    return x @ w + bb[None, :], gamma(W.shape[0] + 1) * (np.abs(x) @ np.abs(w) + np.abs(bb)[None, :])


def direct64(l):
    """lse by the direct log-softmax spelling"""
    M = l.max(1)
    return M + np.log(np.exp(l - M[:, None]).sum(1))


def slabwise64(l, slab=SLAB):
    """lse by the slab-wise merge: per slab (m_s, s_s = sum exp(l - m_s)); M = max m_s, S = sum s_s exp(m_s - M), lse = M + log S"""
    ms, ss = [], []
    for c0 in range(0, l.shape[1], slab):
        blk = l[:, c0:c0 + slab]
        m = blk.max(1)
        ms.append(m)
        ss.append(np.exp(blk - m[:, None]).sum(1))
    ms, ss = np.stack(ms, 1), np.stack(ss, 1)
    M = ms.max(1)
    return M + np.log((ss * np.exp(ms - M[:, None])).sum(1))


class Ref(object):
    """Everything the tests compare against for one (hn, W, b, tgt, N): float64 values and bounds per row."""

    def __init__(self, hn, W, b, tgt, N):
        l, bl = logits64(hn, W, b, N)
        R = l.shape[0]
        rows = np.arange(R)
        self.N, self.logits, self.b_logit = N, l, bl
        self.lse = direct64(l)
        self.tgt_logit, self.stop_logit = l[rows, tgt], l[:, N - 1]
        self.logp, self.stop_logp = self.tgt_logit - self.lse, self.stop_logit - self.lse
        self.b_dot = bl.max(1)
        M = l.max(1)
        y = l - M[:, None]
        e = np.exp(y)
        S = e.sum(1)
        slabs = (N + SLAB - 1) // SLAB
        rel = (U * (np.abs(y) + 16.0) * e).sum(1) / S + gamma(12 + slabs + 3)
        self.b_chain = rel / (1.0 - rel) + 4.0 * U * np.abs(np.log(S)) + U * np.abs(self.lse)
        self.b_lse = self.b_dot + self.b_chain
        self.b_logp = bl[rows, tgt] + self.b_lse + U * np.abs(self.logp)
        self.b_stop_logp = bl[:, N - 1] + self.b_lse + U * np.abs(self.stop_logp)
        self.b_tgt_logit, self.b_stop_logit = bl[rows, tgt], bl[:, N - 1]
        o = np.argsort(-l, axis=1, kind="stable")[:, :2]
        self.top = o[:, 0].astype(i32)
        self.margin = l[rows, o[:, 0]] - l[rows, o[:, 1]] if N > 1 else np.full(R, np.inf)
        self.decided = self.margin > 2.0 * self.b_dot

    def rows(self, n):
        """the first n rows (a row's reference does not depend on the rows beside it)"""
        r = object.__new__(Ref)
        for k, v in self.__dict__.items():
            setattr(r, k, v[:n] if isinstance(v, np.ndarray) else v)
        return r

    def ratios(self, got):
        """{name: worst |got - float64| / bound} over the rows; got: dict of the kernel's arrays"""
        out = {}
        for k in ("lse", "logp", "stop_logp", "tgt_logit", "stop_logit"):
            if k in got:
                out[k] = float((np.abs(got[k].astype(f64) - getattr(self, k)) / getattr(self, "b_" + k)).max())
        return out

    def argmax_failures(self, greedy, planted=None):
        """rows that break the argmax rule: a planted exact tie resolves to its lower index; a decided row gives the float64 argmax; an undecided one an id whose
        float64 logit lies within 2 B_dot of the maximum"""
        fails = []
        for r in range(len(greedy)):
            g = int(greedy[r])
            if planted is not None and planted[r] >= 0:
                if g != planted[r]:
                    fails.append("row %d: argmax %d, the planted tie's lower index is %d" % (r, g, planted[r]))
            elif self.decided[r]:
                if g != self.top[r]:
                    fails.append("row %d (margin %.3e): argmax %d, float64's %d" % (r, self.margin[r], g, self.top[r]))
            elif not (0 <= g < self.N) or self.logits[r, self.top[r]] - self.logits[r, g] > 2.0 * self.b_dot[r]:
                fails.append("row %d (undecided): argmax %d is not within the bound of the maximum (%d)" % (r, g, self.top[r]))
        return fails


def _chain(g, wm):
    """acc = fma(g[:, i], wm[i], acc) for i ascending, in float32 (a float64 multiply-add of float32 values rounded to float32: fmaf up to a rare double rounding)"""
    acc = np.zeros((g.shape[0], wm.shape[1]), f32)
    for i in range(g.shape[1]):
        acc = (acc.astype(f64) + g[:, i:i + 1].astype(f64) * wm[i:i + 1].astype(f64)).astype(f32)
    return acc


DEFECTS = ("pad_counted", "stop_dropped", "target_off_by_one", "merge_no_rescale", "tie_ge", "last_slab_skipped")


def score32(hn, W, b, tgt, N, defect=None, slab=SLAB):
    """The kernels' arithmetic in float32 and their order of merging (32-column tiles w and w + 4 of a slab on wave w, the waves ascending, the slabs ascending;
    the 32 columns of a tile are summed pairwise as the xor tree does). defect: one of DEFECTS. Returns the dict of arrays the harness returns."""
    R = hn.shape[0]
    n_cols = W.shape[1] if defect == "pad_counted" else N
    l = (_chain(hn.astype(f32), W[:, :n_cols].astype(f32)) + b[None, :n_cols].astype(f32)).astype(f32)
    if defect == "stop_dropped":
        n_cols = N - 1
        l = l[:, :n_cols]
    pm, ps, pi = [], [], []
    for c0 in range(0, n_cols, slab):
        if defect == "last_slab_skipped" and c0 + slab >= n_cols and c0 > 0:
            break
        wm, wsum, wi = [], [], []
        for w in range(4):
            cols = [c for t in (w, w + 4) for c in range(c0 + 32 * t, min(c0 + 32 * t + 32, n_cols))]
            if not cols:
                continue
            blk = l[:, cols]
            li = blk.shape[1] - 1 - blk[:, ::-1].argmax(1) if defect == "tie_ge" else blk.argmax(1)
            m = blk[np.arange(R), li]
            lane = np.zeros((R, 32), f32)  # a lane's two columns first, then the xor tree over the 32 lanes
            for k, c in enumerate(cols):
                lane[:, (c - c0) % 32] += np.exp((blk[:, k] - m).astype(f32)).astype(f32)
            for d in (16, 8, 4, 2, 1):
                lane = (lane + lane[:, np.arange(32) ^ d]).astype(f32)
            wm.append(m); wsum.append(lane[:, 0]); wi.append(np.array(cols, i32)[li])
        m, i = wm[0].copy(), wi[0].copy()
        for k in range(1, len(wm)):
            take = (wm[k] >= m) if defect == "tie_ge" else (wm[k] > m)
            m, i = np.where(take, wm[k], m), np.where(take, wi[k], i)
        s = np.zeros(R, f32)
        for k in range(len(wm)):
            s = (s + wsum[k] * np.exp((wm[k] - m).astype(f32)).astype(f32)).astype(f32)
        pm.append(m); ps.append(s); pi.append(i)
    M, I = pm[0].copy(), pi[0].copy()
    for k in range(1, len(pm)):
        take = (pm[k] >= M) if defect == "tie_ge" else (pm[k] > M)
        M, I = np.where(take, pm[k], M), np.where(take, pi[k], I)
    S = np.zeros(R, f32)
    for k in range(len(pm)):
        scale = f32(1.0) if defect == "merge_no_rescale" else np.exp((pm[k] - M).astype(f32)).astype(f32)
        S = (S + ps[k] * scale).astype(f32)
    lse = (M + np.log(S).astype(f32)).astype(f32)
    t = np.minimum(tgt + 1, l.shape[1] - 1) if defect == "target_off_by_one" else np.minimum(tgt, l.shape[1] - 1)
    tl, sl = l[np.arange(R), t], l[:, min(N - 1, l.shape[1] - 1)]
    return {"lse": lse, "logp": (tl - lse).astype(f32), "stop_logp": (sl - lse).astype(f32), "greedy": I.astype(i32), "tgt_logit": tl, "stop_logit": sl}


# ---- the row table of tts_ar_score_codes, restated literally ----
def score_rows(codes, positions, off_by_one=False):
    """(input_ids, mel_pos, targets), each [n + 1]: row 0 feeds 8192 at mel position 0; row j feeds code j - 1 at mel position (j - 1) + 2 ("decode": what the decode
    step saw) or (j - 1) + 1 ("train": the latent pass's); row j predicts code j, the last row the stop token 8193. off_by_one: the seeded defect of the position rule."""
    n = len(codes)
    shift = {"decode": 2, "train": 1}[positions] + (1 if off_by_one else 0)
    ids = [8192] + [int(c) for c in codes[:n]]
    pos = [0] + [i + shift for i in range(n)]
    tgt = [int(c) for c in codes] + [8193]
    return np.array(ids[:n + 1], i32), np.array(pos[:n + 1], i32), np.array(tgt, i32)


# ---- the engine tests' inputs and their oracle sides (tests/test_ar_score_gpu.py; the conditions on the oracle alone in tests/test_ar_score_cpu.py) ----
HEAD_W, HEAD_B = "inference_model.lm_head.1.weight", "inference_model.lm_head.1.bias"
CAND_CODES = (5, 12, 40)  # 6 + 13 rows stay below the 32 rows at which the latent pass changes from the GEMV to the MFMA path, 3 x 41 lie above
DECODE_GATE = 1e-4        # tests/test_ar_gpu.py's gate on decode logits, relative to max |oracle logit|; a score gets twice that (logit error + lse error)


def candidates(seed=77):
    g = np.random.default_rng(seed)
    return [g.integers(0, 8192, n).astype(i32) for n in CAND_CODES]


def padded502(cands, pad=83):
    """[nb][502]: 8192, the codes, then `pad`: the input rows of the uniform pass as tts_ar_latents takes them"""
    out = np.full((len(cands), 502), pad, i32)
    for b, c in enumerate(cands):
        out[b, 0] = 8192
        out[b, 1:1 + len(c)] = c
    return out


def head(model):
    """lm_head.1 as (W [1024][8194], b [8194]) float32"""
    b = model.tensor(HEAD_B)
    return np.ascontiguousarray(model.tensor(HEAD_W).reshape(len(b), -1).T), b


def log_softmax64(l):
    l = l.astype(f64)
    return l - direct64(l.reshape(-1, l.shape[-1])).reshape(l.shape[:-1])[..., None]


def oracle_decode_logits(O, model_path, toks, voice, cands):
    """[nb][n_max + 1][8194]: oracle prefill() at row 0, step(code j - 1, j - 1) at row j: the distributions the sampler would have seen on these codes"""
    ar = O.AR(O.Model(model_path))
    n_max = max(len(c) for c in cands)
    ar.start(toks, voice, len(cands), len(toks) + 2 + n_max + 1)
    rows = [ar.prefill()]
    for i in range(n_max):
        rows.append(ar.step(np.array([c[i] if i < len(c) else 83 for c in cands], i32), i))
    return np.stack(rows, 1)


def oracle_train_logits(O, model_path, toks, voice, cands):
    """[nb][n_max + 1][8194] float64: the float64 head on the oracle's latents() of the same codes (the latent pass's positions)"""
    m = O.Model(model_path)
    ar = O.AR(m)
    n_rows = max(len(c) for c in cands) + 1
    ar.start(toks, voice, len(cands), len(toks) + 2 + n_rows + 1)
    lat = ar.latents(padded502(cands), n_rows)
    W, b = head(m)
    return lat.astype(f64) @ W.astype(f64) + b.astype(f64)
