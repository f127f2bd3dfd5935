"""The rule that defines the device sampler (option ar_sampler = 1; csrc/ar.hip: sample_device_kernel) as one plain function, and the planted rows the GPU test
feeds it. Stop mask, penalty, division and the survivor set are numpy float32 (exact steps: the kernel's survivor set is this one); softmax, top-p and the draw
are float64. tol(n) is the bound DESIGN.md "What pins the device sampler" derives from the kernel's summation order (13 f32 additions per cumulative value),
the device expf's 1 ulp and the rounding of x - max: (4 ln n + 64) * 2^-24 on the cumulative probabilities."""
import numpy as np

V, CAP = 8194, 1024  # TTS_SD_MAX_SURVIVORS
KINDS = ["plain", "ties", "edge0", "edge8193", "zeros", "quot"]  # the planted rows
QUOT_BASE = {0.05: 1.7, 0.8: 1.7, 3.0: 3.5}  # where consecutive floats are closer than an ulp of their quotient by the temperature
ITERATIONS, SEED = 12, 20260


def tol(n):
    return (4.0 * np.log(n) + 64.0) * 2.0 ** -24


def sample_ref(row, ids, u, temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, mask_stop=False):
    """-> (id, decided, neighbours): the draw, whether tol(n) decides it, and the ids next to it in ascending order; None for a row with more than CAP survivors."""
    v = np.array(row, np.float32)
    if mask_stop:
        v[V - 1] = np.float32(-1e30)
    ids = np.unique(ids)
    g = v[ids]
    v[ids] = np.where(g < 0, g * np.float32(penalty), g / np.float32(penalty))
    x = v / np.float32(temperature)
    surv = np.flatnonzero(x >= np.partition(x, V - top_k)[V - top_k])  # ties at the k-th value survive
    n = len(surv)
    if n > CAP:
        return None
    order = surv[np.lexsort((surv, x[surv]))]  # ascending (x, index)
    xs = x[order].astype(np.float64)
    e = np.exp(xs - xs[-1])
    C = np.cumsum(e / e.sum())
    cut = 1.0 - float(np.float32(top_p))
    m = 0
    if cut > 0:
        masked = C <= cut
        masked[-1] = False  # the last survivor is never masked
        m = int(np.argmin(masked))
    M = C[m - 1] if m else 0.0
    target = M + float(u) * (1.0 - M)  # the renormalised cumulative sum reaches u
    hit = np.flatnonzero(C[m:] >= target)
    r = m + int(hit[0]) if len(hit) else n - 1
    decided = np.abs(C - target).min() > tol(n) and (cut <= 0 or np.abs(C - cut).min() > tol(n))
    return int(order[r]), bool(decided), [int(i) for i in order[max(r - 1, 0):r + 2]]


# ---- the planted rows of tests/test_sample_device_gpu.py (the CPU test checks the undecided share of every one of them on sample_ref alone) ----
def planted_row(rs, kind, top_k, temperature):
    row = (2.0 * rs.randn(V)).astype(np.float32)
    kth = np.argpartition(row, V - top_k)[V - top_k]  # where the k-th largest value lies
    if kind == "ties":  # five copies of the k-th value: threads 255 / 0 and 1 / 2 hold neighbours in different registers
        row[[255, 256, 511, 512]] = row[kth]
    elif kind == "edge0":
        row[[0, kth]] = row[[kth, 0]]
    elif kind == "edge8193":  # the 33rd register of thread 1
        row[[V - 1, kth]] = row[[kth, V - 1]]
    elif kind == "zeros":  # +0 and -0 are the row's two largest values and tie
        row = -np.abs(row) - np.float32(1)
        row[[5, 300]] = [0.0, -0.0]
    elif kind == "quot":  # eight consecutive floats at the k-th place: some share a quotient, a tie that only the division creates
        a = np.float32(QUOT_BASE[temperature])
        row += a - row[kth]
        for i in range(8):
            row[1000 + 31 * i] = a
            a = np.nextafter(a, np.float32(9))
    return row


def planted_cases():
    """(n, top_k, top_p, temperature, ids kind, mask_stop): every top-k x top-p x temperature, the other three cycling through their values"""
    grid = [(k, p, t) for k in (1, 50, 100, 512) for p in (0.05, 0.8, 1.0) for t in (0.05, 0.8, 3.0)]
    return [((1, 3, 17)[i % 3], k, p, t, ("prompt", "one", "history")[(i // 3) % 3], bool((i // 2) % 2)) for i, (k, p, t) in enumerate(grid)]


def planted_inputs(case_index):
    """-> (rows [n, V], ids [n, k]) of planted_cases()[case_index]: row b is of kind KINDS[(b + case_index) % 6]"""
    n, top_k, top_p, temperature, ids_kind, mask = planted_cases()[case_index]
    rs = np.random.RandomState(1000 + case_index)
    rows = np.stack([planted_row(rs, KINDS[(b + case_index) % len(KINDS)], top_k, temperature) for b in range(n)])
    if ids_kind == "prompt":  # scope 0, iteration 0: [1 ... 1, 8192]
        ids = np.tile(np.array([1] * 5 + [8192], np.int32), (n, 1))
    elif ids_kind == "one":  # scope 0 afterwards: the token fed, here the row's largest logit
        ids = rows.argmax(1).astype(np.int32)[:, None]
    else:  # scope 1: a history
        ids = np.stack([np.concatenate([[1, 8192, 31, 32, 8193], np.argsort(rows[b])[-20::2]]) for b in range(n)]).astype(np.int32)
    return rows, ids
