"""The AR stage's five attention kernels and its ragged QKV epilogue, launched one at a time through the test-only harness (libtts_ar_test.so) and compared
element by element with the float64 reference of tests/ar_attn_cases.py under that module's derived bound; bit identities between launches that must not
differ (a row's bits depend on its own query and the keys before it only). tests/test_ar_attn_harness_cpu.py shows that the bound is sharp.
With TTS_AR_ATTN_REPORT=<file> the largest |error| / bound per kernel and input family is written there (profiles/ar_attention_direct.txt)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ar_attn_cases as A
from ar_attn_cases import ATTENTION, DECODE, DECODE_FAST, EPILOGUE, RAGGED, ROWS, D

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TTS_AR_ATTN_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"%s | %s" % k: v for k, v in sorted(RATIOS.items())}, f, indent=1)


def check(label, out, v, kind):
    """One variant's output against the reference: every element finite and within its bound."""
    r = A.ratio(out, v, kind)
    key = (label, v.family)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print("%-34s %-7s %-28s nk<=%-4d |err|/bound %.3f" % (label, v.family, v.tag, int(v.nk.max()), r))
    return r


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_rows(kernel, vs, S, n_past, lut=0):
    """Variants of one rows shape, three candidates per launch -> one [S, 1024] output per variant."""
    outs = []
    for i in range(0, len(vs), 3):
        grp = vs[i:i + 3]
        qkv, kc, vc = A.pack_rows(grp, S)
        if kernel == RAGGED:  # every candidate one item, slots in reverse order
            items = np.array([[c * S, S, n_past, c] for c in reversed(range(len(grp)))], np.int32)
            o = A.run_attention(RAGGED, qkv, kc, vc, items=items).payload
        else:
            o = A.run_attention(kernel, qkv, kc, vc, S=S, n_past=n_past, lut=lut).payload
        outs += [o[c * S:(c + 1) * S] for c in range(len(grp))]
    return outs


@pytest.mark.parametrize("S,n_past", A.ROWS_SHAPES)
def test_rows_shapes_within_bound(S, n_past):
    vs = A.rows_variants(S, n_past)
    worst = 0.0
    for label, kernel, kind in (("attention_rows_kernel", ROWS, "rows"), ("attention_rows_ragged_kernel", RAGGED, "rows"), ("attention_kernel lut=0", ATTENTION, "attention")):
        for v, o in zip(vs, run_rows(kernel, vs, S, n_past)):
            worst = max(worst, check(label, o, v, kind))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("S,n_past", A.ROWS_SHAPES)
def test_rows_shapes_within_bound_lut(S, n_past):
    vs = A.rows_variants(S, n_past, lut=1)
    worst = max(check("attention_kernel lut=1", o, v, "attention") for v, o in zip(vs, run_rows(ATTENTION, vs, S, n_past, lut=1)))
    assert worst <= 1.0, worst


def run_decode(kernel, vs, nk=None, lut=0, max_pos=None):
    """Single-row variants as the candidates of one launch. nk: the key count all share (template form <false>); None: each its own through row_off (<true>)."""
    q, kc, vc = A.pack_decode(vs, max_pos)
    if nk is None:
        ro = np.array([int(v.nk[0]) - 1 for v in vs], np.int32) - 5  # n_past = 5 and offsets of either sign
        return A.run_attention(kernel, q, kc, vc, n_past=5, lut=lut, row_off=ro).payload
    return A.run_attention(kernel, q, kc, vc, n_past=nk - 1, lut=lut).payload


@pytest.mark.parametrize("nk", A.DECODE_COUNTS)
def test_decode_counts_within_bound(nk):
    vs = A.decode_variants(nk)
    worst = 0.0
    for label, kernel, kind in (("attn_decode_fast_kernel<false>", DECODE_FAST, "dfast"), ("attn_decode_kernel<false> lut=0", DECODE, "decode")):
        for i in range(0, len(vs), 6):  # a handful of candidates per launch
            o = run_decode(kernel, vs[i:i + 6], nk)
            worst = max([worst] + [check(label, o[c], v, kind) for c, v in enumerate(vs[i:i + 6])])
    vl = A.decode_variants(nk, lut=1)
    for i in range(0, len(vl), 6):
        o = run_decode(DECODE, vl[i:i + 6], nk, lut=1)
        worst = max([worst] + [check("attn_decode_kernel<false> lut=1", o[c], v, "decode") for c, v in enumerate(vl[i:i + 6])])
    assert worst <= 1.0, worst


def _pick(nk, role, lut=0):
    """The variant of key count nk that plays `role`: a family's tag, or the peaked placement that targets a mutation (flat where the key does not exist)."""
    if role in ("flat", "up", "down", "peaked-last", "ramp-up"):
        return A.decode_variants(nk, lut, want=lambda fam, tag, tg: tag == role)[0]
    hit = A.decode_variants(nk, lut, want=lambda fam, tag, tg: fam == "peaked" and role in tg)
    return hit[0] if hit else A.decode_variants(nk, lut, want=lambda fam, tag, tg: fam == "flat")[0]


@pytest.mark.parametrize("role", ["flat", "drop_last", "drop_key0", "admit_one", "up", "down", "peaked-last", "ramp-up"])
def test_decode_row_offsets_one_launch_of_24_counts(role):
    """The <true> forms: 24 candidates with the 24 key counts in ONE launch, each within its bound and bit-equal to the <false> form at the same count."""
    lut_roles = ("flat", "drop_last", "up")
    vs = [_pick(nk, role) for nk in A.DECODE_COUNTS]
    worst = 0.0
    for label, kernel, kind in (("attn_decode_fast_kernel<true>", DECODE_FAST, "dfast"), ("attn_decode_kernel<true> lut=0", DECODE, "decode")):
        o = run_decode(kernel, vs, max_pos=1024)
        worst = max([worst] + [check(label, o[c], v, kind) for c, v in enumerate(vs)])
        for c, v in enumerate(vs):
            single = run_decode(kernel, [v], int(v.nk[0]))
            assert (bits(single[0]) == bits(o[c])).all(), (label, int(v.nk[0]))
    if role in lut_roles:
        vl = [_pick(nk, role, lut=1) for nk in A.DECODE_COUNTS]
        o = run_decode(DECODE, vl, lut=1, max_pos=1024)
        worst = max([worst] + [check("attn_decode_kernel<true> lut=1", o[c], v, "decode") for c, v in enumerate(vl)])
        for c in (0, 7, 17, 23):
            assert (bits(run_decode(DECODE, [vl[c]], int(vl[c].nk[0]), lut=1)[0]) == bits(o[c])).all()
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------- ragged launches

def test_ragged_launch_of_unequal_items():
    """Items of different S and n_past in one launch, slots and rows out of order, S = 3 beside S = 130 (blocks past a sequence leave early), an n_past + S that
    ends on a chunk edge; every cache row behind a sequence is NaN."""
    shapes = [(3, 125), (130, 300), (40, 281), (1, 128), (65, 0)]  # (S, n_past); 3 + 125 = 128
    slots = [2, 0, 4, 1, 3]
    order = [3, 1, 4, 0, 2]  # position of each item's rows in the packed row space
    picks = ["peaked-last", "ramp-up", "flat", "peaked-last", "up"]
    seqs = []
    for (S, n_past), tag in zip(shapes, picks):
        P = n_past + S
        q, K, V = A.gen(A._seed("ragged", S, n_past, tag), "peaked" if tag.startswith("peaked") else "flat" if tag == "flat" else "ramp", S, P, P, jstar=P - 1)
        seqs.append(A.Variant("poison", tag, [], q, K, V, n_past + 1 + np.arange(S), poison_from=None))
    n_rows = sum(s for s, _ in shapes)
    first, r = {}, 0
    for i in sorted(range(len(shapes)), key=lambda i: order[i]):
        first[i] = r
        r += shapes[i][0]
    qkv = np.full((n_rows, 3 * D), np.nan, np.float32)
    kc = np.full((5, 1024, D), A.F16_NAN, np.uint16)
    vc = np.full((5, 1024, D), A.F16_NAN, np.uint16)
    items = np.zeros((len(shapes), 4), np.int32)
    for i, ((S, n_past), v) in enumerate(zip(shapes, seqs)):
        qkv[first[i]:first[i] + S, :D] = v.q.reshape(S, D)
        kc[slots[i], :v.P] = v.bits(v.K).reshape(v.P, D)
        vc[slots[i], :v.P] = v.bits(v.V).reshape(v.P, D)
        items[i] = (first[i], S, n_past, slots[i])
    out = A.run_attention(RAGGED, qkv, kc, vc, items=items).payload
    again = A.run_attention(RAGGED, qkv, kc, vc, items=items[::-1].copy()).payload
    assert (bits(out) == bits(again)).all()
    worst = max(check("attention_rows_ragged_kernel", out[first[i]:first[i] + shapes[i][0]], v, "rows") for i, v in enumerate(seqs))
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------- bit identities

@pytest.fixture(scope="module")
def sequence():
    """One sequence of 200 rows from n_past = 0 in a cache of 3 slots (slot 1), and its attention_rows_kernel output."""
    S = 200
    q, K, V = A.gen(A._seed("identity"), "flat", S, S, S)
    v = A.Variant("flat", "identity", [], q, K, V, 1 + np.arange(S))
    qkv, kc1, vc1 = A.pack_rows([v], S)
    full = A.run_attention(ROWS, qkv, kc1, vc1, S=S, n_past=0).payload.copy()
    assert A.ratio(full, v, "rows") <= 1.0
    return S, v, qkv, kc1, vc1, full


@pytest.mark.parametrize("S1", [1, 37, 63, 64, 65, 127, 128, 129, 199])
def test_rows_kernel_two_passes_equal_one(sequence, S1):
    S, v, qkv, kc, vc, full = sequence
    a = A.run_attention(ROWS, qkv[:S1].copy(), kc, vc, S=S1, n_past=0).payload
    b = A.run_attention(ROWS, qkv[S1:].copy(), kc, vc, S=S - S1, n_past=S1).payload
    assert (bits(np.concatenate([a, b])) == bits(full)).all()
    again = A.run_attention(ROWS, qkv[S1:].copy(), kc, vc, S=S - S1, n_past=S1).payload
    assert (bits(again) == bits(b)).all()  # two launches of the same case


@pytest.mark.parametrize("cuts", [(), (64,), (1, 2), (37, 128, 129), (100, 36, 164)], ids=str)
def test_ragged_kernel_on_any_partition_equals_rows_kernel(sequence, cuts):
    S, v, qkv, kc, vc, full = sequence
    edges = sorted(set(cuts) | {0, S})
    parts = list(zip(edges[:-1], edges[1:]))
    if cuts and list(cuts) != sorted(cuts):
        parts = parts[::-1]  # items out of order
    items = np.array([[a, b - a, a, 0] for a, b in parts], np.int32)
    out = A.run_attention(RAGGED, qkv, kc, vc, items=items).payload
    assert (bits(out) == bits(full)).all()


def test_ragged_kernel_beside_unrelated_items_equals_rows_kernel(sequence):
    S, v, qkv, kc, vc, full = sequence
    rng = np.random.RandomState(3)
    other = [(3, 60, 0), (130, 300, 2)]  # (S, n_past, slot); the sequence sits in slot 1
    n_rows = S + sum(o[0] for o in other)
    q2 = np.full((n_rows, 3 * D), np.nan, np.float32)
    kc2 = A.f16(rng.randn(3, 512, D))[1]
    vc2 = A.f16(rng.randn(3, 512, D))[1]
    kc2[1, :S], vc2[1, :S] = kc[0], vc[0]
    kc2[1, S:], vc2[1, S:] = A.F16_NAN, A.F16_NAN
    q2[:3, :D] = A.f16(rng.randn(3, D))[0]
    q2[3:3 + S] = qkv
    q2[3 + S:, :D] = A.f16(rng.randn(130, D))[0]
    items = np.array([[3 + S, 130, 300, 2], [3, S, 0, 1], [0, 3, 60, 0]], np.int32)
    out = A.run_attention(RAGGED, q2, kc2, vc2, items=items).payload
    assert np.isfinite(out).all()
    assert (bits(out[3:3 + S]) == bits(full)).all()


# ---------------------------------------------------------------------------------------------------------------- one problem, five kernels

@pytest.mark.parametrize("S,n_past", [(40, 281), (9, 0)])
def test_all_kernels_on_one_problem(S, n_past):
    """LUT-range inputs (valid for every kernel): the four multi-row launches on all rows, the decode kernels on each candidate's last row."""
    vs = A.rows_variants(S, n_past, lut=1, want=lambda fam, tag, tg: tag in ("flat", "up") or (fam == "peaked" and "drop_last" in tg))[:3]
    worst, outs = 0.0, {}
    for label, kernel, kind, lut in (("attention_rows_kernel", ROWS, "rows", 0), ("attention_rows_ragged_kernel", RAGGED, "rows", 0),
                                     ("attention_kernel lut=0", ATTENTION, "attention", 0), ("attention_kernel lut=1", ATTENTION, "attention", 1)):
        outs[label] = run_rows(kernel, vs, S, n_past, lut)
        for v, o in zip(vs, outs[label]):
            v.lut = lut
            v._bounds = {}
            worst = max(worst, check(label, o, v, kind))
    assert any((bits(a) != bits(b)).any() for a, b in zip(outs["attention_kernel lut=0"], outs["attention_kernel lut=1"]))  # the switch does something
    assert all((bits(a) == bits(b)).all() for a, b in zip(outs["attention_rows_kernel"], outs["attention_rows_ragged_kernel"]))
    nk = n_past + S
    last = [A.Variant(v.family, v.tag, [], v.q[-1:], v.K, v.V, [nk]) for v in vs]
    dec = {}
    for label, kernel, kind, lut in (("attn_decode_fast_kernel<false>", DECODE_FAST, "dfast", 0), ("attn_decode_kernel<false> lut=0", DECODE, "decode", 0),
                                     ("attn_decode_kernel<false> lut=1", DECODE, "decode", 1)):
        dec[label] = run_decode(kernel, last, nk, lut)
        for c, v in enumerate(last):
            v.lut = lut
            v._bounds = {}
            worst = max(worst, check(label, dec[label][c], v, kind))
    assert (bits(dec["attn_decode_kernel<false> lut=0"]) != bits(dec["attn_decode_kernel<false> lut=1"])).any()
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------- QKV epilogues

def _epilogues(rows):
    """Both QKV epilogues on the same part, bias and pscale = 1 / 64, `rows` packed rows with destinations out of order in 3 slots of 70 positions."""
    f32 = np.float32
    rng = np.random.RandomState(rows)
    n_slots, max_pos, pscale = 3, 70, 1.0 / 64
    part = (rng.randn(rows, 3 * D) * 64).astype(f32)
    bias = rng.randn(3 * D).astype(f32)
    row_dst = rng.permutation(n_slots * max_pos)[:rows].astype(np.int32)
    g = dict(out=A.Guarded((rows, 3 * D), f32), out2=A.Guarded((rows, 3 * D), f32), kout=A.Guarded((n_slots * max_pos, D), np.uint16),
             vout=A.Guarded((n_slots * max_pos, D), np.uint16), kout2=A.Guarded((rows, D), np.uint16), vout2=A.Guarded((rows, D), np.uint16))
    kw = {k: v.raw.ctypes.data_as(C.c_void_p) for k, v in g.items()}
    kw.update(part=part.ctypes.data_as(C.c_void_p), bias=bias.ctypes.data_as(C.c_void_p), row_dst=row_dst.ctypes.data_as(C.c_void_p), pscale=pscale)
    cs = A.struct(EPILOGUE, n_cand=n_slots, max_pos=max_pos, n_rows=rows, **kw)
    assert A.harness().tts_ar_test_run(C.byref(cs)) == 0
    assert all(v.canaries_intact() for v in g.values())
    return part, bias, f32(pscale), row_dst, g


@pytest.mark.parametrize("rows", [1, 2, 130])
def test_ragged_qkv_epilogue_equals_the_plain_one_and_lands_at_row_dst(rows):
    part, bias, pscale, row_dst, g = _epilogues(rows)
    out = g["out"].payload
    assert (bits(out) == bits(g["out2"].payload)).all()
    h = out.astype(np.float16)
    assert (h.astype(np.float32) == out).all()  # out holds fp16 values: K and V in the cache are its conversion, exactly
    wk, wv = h[:, D:2 * D].view(np.uint16), h[:, 2 * D:].view(np.uint16)
    assert (g["kout2"].payload == wk).all() and (g["vout2"].payload == wv).all()
    for name, w in (("kout", wk), ("vout", wv)):
        cache = g[name].payload
        assert (cache[row_dst] == w).all(), name
        rest = np.ones(len(cache), bool)
        rest[row_dst] = False
        assert (cache[rest].view(np.uint8) == A.SENTINEL).all(), name  # every other cache byte keeps its sentinel


@pytest.mark.parametrize("rows", [1, 2, 130])
def test_ragged_qkv_epilogue_equals_numpy_rounding(rows):
    """out against NumPy's float32(v * pscale + bias) rounded to fp16 (pscale a power of two: the product is exact, the sum rounds once to f32, then to fp16).
    130 rows hold about 50 exact ties of the f32 sum between two fp16 values: a kernel that rounds the exact sum once to fp16 (the FMA and the conversion
    fused into v_fma_mixlo_f16, as hipcc did before the f32 sum was pinned in ar.hip) lands on the other neighbour at about half of them."""
    part, bias, pscale, row_dst, g = _epilogues(rows)
    want = (part * pscale + bias[None, :]).astype(np.float32).astype(np.float16)
    out = g["out"].payload
    bad = np.argwhere(bits(out) != bits(want.astype(np.float32)))
    print("rows %d: %d of %d elements differ from the NumPy rounding" % (rows, len(bad), out.size))
    assert len(bad) == 0, (len(bad), [(float(out[r, n]), float(want[r, n]), float(part[r, n] * pscale + bias[n])) for r, n in bad[:6]])
