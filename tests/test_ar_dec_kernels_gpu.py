"""The AR decode step's two GEMV kernels and the weight packers, launched one at a time through the test-only harness (libtts_dec_test.so): every
instantiation the product launches, on slabs built by the product's own packers, compared element by element with the float64 reference of
tests/ar_dec_cases.py under that module's derived bounds; exact cases that must be bit-equal; bit identities between launches that must not differ; the device
packers against the host packers byte for byte and against the NumPy restatement of every layout. tests/test_ar_dec_harness_cpu.py shows that the bound is sharp.
With TTS_AR_DEC_REPORT=<file> the largest |error| / bound per kernel and mode, and the split path's error in units of 2^-22 sum |xhat||w| per input family, are
written there (profiles/ar_dec_direct.txt)."""
import json
import os

import numpy as np
import pytest

import ar_dec_cases as A
from ar_dec_cases import COLS4, D, E4M3, F16, F32, FF, GELU, LOGITS, MFMA16H, QKV, SPLIT, SPLITW, STRIP, V, VPAD

pytestmark = pytest.mark.gpu

RATIOS, UNITS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TTS_AR_DEC_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"ratio": dict(sorted(RATIOS.items())), "split_units": dict(sorted(UNITS.items()))}, f, indent=1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def note(label, ratio):
    RATIOS[label] = max(RATIOS.get(label, 0.0), float(ratio))
    print("%-40s |err|/bound %.3f" % (label, ratio))


def ln_label(c):
    return "dec_ln_gemv %s SPLIT %d HT %d RO %d%s" % (A.EPI_NAMES[c.epi], c.split, c.ht, c.ro, " lut" if c.lut else "")


def check_ln(c, o=None):
    o = c.run() if o is None else o
    ratio, what = A.ln_check(A.ln_expected(c), o.out, o.kc, o.vc)
    note(ln_label(c), ratio)
    assert ratio <= 1.0, (c.tag, ratio, what)
    return o


SPLITS_OF_HT = {0: (0, 1), 1: (0, 1, 2, 3)}
HT_SPLIT = [(ht, s) for ht in (1, 0) for s in SPLITS_OF_HT[ht]]


# ---------------------------------------------------------------------------------------------------------------- packers

DEV_PACKS = [(STRIP, F32, 1024, 128, 0), (STRIP, F32, 1024, 3 * D, 0), (STRIP, F32, 4096, 1024, 0), (MFMA16H, SPLIT, 1024, 64, 1), (MFMA16H, SPLIT, 1024, 3 * D, 1),
             (COLS4, F32, 1024, 64, 0), (COLS4, F32, 4096, 1024, 0)]  # (the larger ones take the grid-stride loop: more than 8192 x 256 elements)


def big_matrix(K, N):
    w, g, b, c = A.make_weights(N if K == 1024 else 1024, 0, True)
    if K == 4096:
        w = np.ascontiguousarray(np.tile(w, (4, 1)) * np.linspace(0.5, 1.5, 4096, dtype=np.float32)[:, None])
    return w, np.resize(g, K), np.resize(b, K), c


@pytest.mark.parametrize("layout,enc,K,N,fold", DEV_PACKS)
def test_device_packer_equals_host_packer_and_the_restatement(layout, enc, K, N, fold):
    w, g, b, c = big_matrix(K, N)
    f = (g, b, c) if fold else (None, None, None)
    dev, host = A.pack(w, layout, enc, 1, *f), A.pack(w, layout, enc, 0, *f, want_fold=False)
    assert (dev.slab == host.slab).all(), "device and host slabs differ"
    wf = w
    if fold:
        wf, cf = A.fold_ref(w, g, b, c)
        assert (bits(dev.fold) == bits(wf)).all(), "pk_fold_kernel differs from float32(g w)"
        assert (bits(dev.bias) == bits(cf)).all() and (bits(host.bias) == bits(cf)).all(), "folded bias differs from the double sum in ascending k"
    want = A.encode(enc, wf, scale64=layout != COLS4)
    got = dev.stored
    for a, e in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
        assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(e).view(np.uint8)).all(), "slab differs from the restated layout"
    assert dev.absmax.view(np.uint32)[0] == np.abs(wf).max().view(np.uint32), "pk_absmax_kernel"


def test_head_path_transpose_pad_fold_and_split_weight():
    """lm_head's path: nn.Linear [V][1024] -> pk_transpose_pad_kernel -> fold -> slab, at a small V that is no multiple of anything; and split_weight_kernel's
    [N][2 K] copy from the strip-major one."""
    rs = np.random.RandomState(4)
    vrows, N = 50, 64
    lin = (0.02 * rs.randn(vrows, D)).astype(np.float32)
    _, g, b, _ = A.make_weights(64, 0, True)
    c = np.zeros(N, np.float32)
    c[:vrows] = rs.randn(vrows)
    wt = np.zeros((D, N), np.float32)
    wt[:, :vrows] = lin.T
    dev = A.pack(lin, MFMA16H, SPLIT, 1, g, b, c, transpose_vrows=vrows, N=N)
    host = A.pack(wt, MFMA16H, SPLIT, 0, g, b, c)
    assert (dev.slab == host.slab).all() and (bits(dev.bias) == bits(host.bias)).all() and (bits(dev.fold) == bits(host.fold)).all()
    plain = A.pack(lin, STRIP, F32, 1, transpose_vrows=vrows, N=N)
    assert (bits(plain.fold) == bits(wt)).all() and (bits(plain.stored) == bits(wt)).all()
    sw = A.pack(wt, SPLITW, SPLIT, 1)
    hi, lo = A.split_hilo(wt)
    assert (sw.stored[0].view(np.uint16) == hi.view(np.uint16)).all() and (sw.stored[1].view(np.uint16) == lo.view(np.uint16)).all()


# ---------------------------------------------------------------------------------------------------------------- dec_ln_gemv_kernel: the head

@pytest.mark.parametrize("rows,rot", A.ROW_CASES)
@pytest.mark.parametrize("ht,split", HT_SPLIT)
def test_head_rows_and_families_within_bound(ht, split, rows, rot):
    """A small head (N = 64, n_valid = 50, ldo = 70: the dropped columns and the row's slack keep the sentinel) over every row count and family rotation."""
    check_ln(A.ln_case(LOGITS, split, ht, rows, rot, n_valid=50, ldo=70))


@pytest.mark.parametrize("ht,split,rows", [(1, 0, 17), (1, 1, 17), (1, 2, 19), (1, 3, 32), (0, 0, 1), (0, 1, 1)])
def test_head_at_the_product_shape(ht, split, rows):
    """N = 8256, n_valid = 8194, row stride 8194: the last tile of columns is cut at column 8194, the next row begins right behind it."""
    check_ln(A.ln_case(LOGITS, split, ht, rows, 3, N=VPAD, n_valid=V, ldo=V))


ORDINARY = np.array([n for n in range(64) if n % 48 > 5])  # the columns of the N = 64 head without a special construction


@pytest.mark.parametrize("rows,rot", A.ROW_CASES)
def test_split_product_alone_and_its_error_in_units_of_2_pow_minus_22(rows, rot):
    """Three launches on the same rows (ln_f = identity): W = I under SPLIT 0 gives xhat as the LayerNorm left it, W = I under SPLIT 1 the operand xh + xl the
    matrix pipe was handed, and the head on real weights under SPLIT 1 is compared with the float64 product of THAT operand: the split product without the
    LayerNorm's error, under a bound of its own (A.split_only_expected). Recorded per input family: the error in the unit of the "2^-22 relative" statement,
    with the rounding of xl (against the SPLIT 0 xhat; this includes the two instantiations' different reduction order) and without (against xh + xl)."""
    one, zero = np.ones(D, np.float32), np.zeros(D, np.float32)
    h = A.make_rows(rows, rot)
    x0 = A.LnCase(LOGITS, 0, 1, h, A.identity_slab(0), g1=one, b1=zero).run().out
    y = A.LnCase(LOGITS, 1, 1, h, A.identity_slab(1), g1=one, b1=zero).run().out
    c = A.ln_case(LOGITS, 1, 1, rows, rot, g1=one, b1=zero)
    out = check_ln(c).out
    r = A.split_only_expected(c, y)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.nanmax(np.where(r.B > 0, np.abs(out - r.ref) / r.B, 0.0))
    note("dec_ln_gemv SPLIT 1, the product alone", ratio)
    # what the operand is: xh + xl of the SPLIT 0 xhat up to the reduction order (a few u), and the subnormal lo parts: kept or flushed?
    xl0 = x0.astype(np.float64) - x0.astype(np.float16).astype(np.float64)
    subn = (np.abs(xl0) < A.SUB16) & (np.abs(xl0) >= 2.0 ** -24)
    lost = subn & (y == y.astype(np.float16).astype(np.float32))
    un_y = A.split_units(r, out)
    r0 = A.split_only_expected(c, x0)
    un_0 = A.split_units(r0, out)
    un_y_ord, un_0_ord = A.split_units(r, out, ORDINARY), A.split_units(r0, out, ORDINARY)
    for i in range(rows):
        f = A.family_of(i, rot)
        for key, v in (("all columns, operand xh + xl", un_y[i]), ("all columns, SPLIT 0 xhat", un_0[i]), ("ordinary columns, operand xh + xl", un_y_ord[i]),
                       ("ordinary columns, SPLIT 0 xhat", un_0_ord[i]), ("fraction of lo parts that are fp16 subnormals", subn[i].mean()),
                       ("fraction of subnormal lo parts that reached the pipe as 0", lost[i].sum() / max(1, subn[i].sum()))):
            UNITS["%s | %s" % (f, key)] = max(UNITS.get("%s | %s" % (f, key), 0.0), float(v))
    assert ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------------------------------- dec_ln_gemv_kernel: QKV

def const_rows_exact(c, o):
    """xhat = 0 exactly on a constant row: q, K and V are the fp16 rounding of the folded bias, bit for bit."""
    b16 = c.slab.bias.astype(np.float16)
    for slot, pos, row in A.kv_targets(c):
        if A.family_of(row, c.rot) == "const":
            assert (bits(o.out[row, :D]) == bits(b16[:D].astype(np.float32))).all(), row
            assert (o.kc[slot, pos] == b16[D:2 * D].view(np.uint16)).all() and (o.vc[slot, pos] == b16[2 * D:].view(np.uint16)).all(), row


def qkv_decode_case(split, ro, rows, rot, n_past, max_pos, ldo=D):
    off = None
    if ro == 1:  # distinct positions per row, of either sign around n_past
        off = np.zeros((rows + 15) // 16 * 16, np.int32)
        off[:rows] = (np.arange(rows) * 7) % max_pos - n_past
    c = A.ln_case(QKV, split, 1, rows, rot, ro=int(ro > 0), n_past=n_past, max_pos=max_pos, row_off=off, ldo=ldo, n_slots=rows + 1)
    c.rot = rot
    return c


@pytest.mark.parametrize("split", [0, 1, 2, 3])
@pytest.mark.parametrize("ro,rows,rot,n_past,max_pos", [(0, 17, 0, 0, 3), (0, 16, 1, 4, 5), (1, 19, 2, 9, 23), (1, 32, 4, 0, 37)])
def test_qkv_decode_form_within_bound(split, ro, rows, rot, n_past, max_pos):
    """n_past 0 and max_pos - 1; under RO every row its own position. Every cache row that is no target, and the spare slot, keep the sentinel."""
    c = qkv_decode_case(split, ro, rows, rot, n_past, max_pos, ldo=D + 4 * (split % 2))
    const_rows_exact(c, check_ln(c))


@pytest.mark.parametrize("split", [0, 1, 2, 3])
def test_qkv_zero_offsets_equal_the_form_without_offsets(split):
    a, b = qkv_decode_case(split, 0, 19, 5, 2, 4), qkv_decode_case(split, 2, 19, 5, 2, 4)
    oa, ob = a.run(), b.run()
    assert (bits(oa.out) == bits(ob.out)).all() and (oa.kc == ob.kc).all() and (oa.vc == ob.vc).all()


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("prefill_B", [1, 3])
def test_qkv_prompt_form_within_bound(split, prefill_B):
    c = A.ln_case(QKV, split, 0, 19, 3, prefill_B=prefill_B, max_pos=21, n_slots=prefill_B + 1)
    c.rot = 3
    const_rows_exact(c, check_ln(c))


# ---------------------------------------------------------------------------------------------------------------- dec_ln_gemv_kernel: GELU

@pytest.mark.parametrize("lut", [0, 1])
@pytest.mark.parametrize("ht,split", HT_SPLIT)
def test_gelu_within_bound(ht, split, lut):
    check_ln(A.ln_case(GELU, split, ht, 19 if lut else 32, 1 + lut, lut=lut))


# ---------------------------------------------------------------------------------------------------------------- dec_ln_gemv_kernel: bit identities

def by_row(c, o):
    """Everything a launch left for each row, as one array per row."""
    if c.epi != QKV:
        return [o.out[r] for r in range(c.rows)]
    t = {row: (slot, pos) for slot, pos, row in A.kv_targets(c) if slot == (0 if c.prefill_B else row)}
    return [np.concatenate([bits(o.out[r, :D]), o.kc[t[r]].astype(np.uint32), o.vc[t[r]].astype(np.uint32)]) for r in range(c.rows)]


@pytest.mark.parametrize("epi,split", [(LOGITS, 0), (LOGITS, 1), (LOGITS, 2), (LOGITS, 3), (GELU, 1), (QKV, 1), (QKV, 3)])
def test_a_rows_bits_do_not_depend_on_its_neighbours_tile_or_slot(epi, split):
    """32 rows, then the same rows in another order (every row in another slot, most in the other tile), then the first 3 alone."""
    kw = dict(n_past=1, max_pos=2) if epi == QKV else {}
    c = A.ln_case(epi, split, 1, 32, 2, **kw)
    perm = (np.arange(32) * 13 + 5) % 32
    c2 = A.LnCase(epi, split, 1, c.h[perm], c.slab, g1=c.g1, b1=c.b1, **kw)
    c3 = A.LnCase(epi, split, 1, c.h[:3], c.slab, g1=c.g1, b1=c.b1, **kw)
    r1, r2, r3 = by_row(c, c.run()), by_row(c2, c2.run()), by_row(c3, c3.run())
    for i in range(32):
        assert (bits(r2[i]) == bits(r1[perm[i]])).all() if epi != QKV else (r2[i] == r1[perm[i]]).all(), i
    for i in range(3):
        assert (bits(r3[i]) == bits(r1[i])).all() if epi != QKV else (r3[i] == r1[i]).all(), i


@pytest.mark.parametrize("epi", [QKV, GELU, LOGITS])
@pytest.mark.parametrize("split", [0, 1])
def test_h4_equals_the_row_major_layout(epi, split):
    """The prompt pass's [row][1024] form and the decode step's h4 form of one instantiation give the same bits (QKV: the decode form's K/V at its own targets)."""
    a = A.ln_case(epi, split, 1, 19, 4, **(dict(n_past=1, max_pos=19) if epi == QKV else {}))
    b = A.ln_case(epi, split, 0, 19, 4, **(dict(prefill_B=2, max_pos=19) if epi == QKV else {}))
    ra, rb = by_row(a, a.run()), by_row(b, b.run())
    for i in range(19):
        assert (bits(ra[i]) == bits(rb[i])).all() if epi != QKV else (ra[i] == rb[i]).all(), i


@pytest.mark.parametrize("split", [2, 3])
def test_reduced_weight_modes_equal_the_split_path_on_weights_they_hold_exactly(split):
    """SPLIT 2 = SPLIT 1 where 64 w is an fp16 number, SPLIT 3 = SPLIT 1 where w is an e4m3 number times its column's power of two: the lo slab is zero, the
    hi operands are equal up to the power of two, every product and sum scales exactly."""
    a, b = A.ln_case(LOGITS, 1, 1, 32, 0, kind="exact"), A.ln_case(LOGITS, split, 1, 32, 0, kind="exact")
    assert (a.slab.wdec == b.slab.wdec).all() and not np.asarray(a.slab.wl).any()
    oa, ob = check_ln(a), check_ln(b)
    assert (bits(oa.out) == bits(ob.out)).all()


# ---------------------------------------------------------------------------------------------------------------- dec_gemv_resid_kernel

def resid_case(kg, wh, ht, rows, kind="real", seed=0):
    rs = np.random.RandomState(100 * kg + 10 * wh + rows + seed)
    K = 1024 * kg
    if kind == "real":
        X = rs.randn(rows, K).astype(np.float32)
        X[1::2] = rs.standard_t(3, X[1::2].shape).astype(np.float32)  # every other row heavy-tailed
        h = rs.randn(rows, D).astype(np.float32)
    elif kind == "int":
        X, h = rs.randint(-4, 5, (rows, K)).astype(np.float32), rs.randint(-64, 65, (rows, D)).astype(np.float32)
    else:  # one-hot: row r picks k_r, every output is one named weight element
        X, h = np.zeros((rows, K), np.float32), np.zeros((rows, D), np.float32)
        X[np.arange(rows), (np.arange(rows) * 997 + 1023) % K] = 1.0
    return A.ResidCase(kg, wh, ht, X, A.resid_weights(kg, wh, "real" if kind == "real" else "int"), h, exact=kind != "real")


def resid_label(c):
    return "dec_gemv_resid KG %d WH %d HT %d" % (c.kg, c.wh, c.ht)


@pytest.mark.parametrize("rows", A.ROW_COUNTS)
@pytest.mark.parametrize("kg,wh,ntw,ht", A.RESID_INSTANCES)
def test_resid_real_values_within_bound(kg, wh, ntw, ht, rows):
    c = resid_case(kg, wh, ht, rows)
    ratio = A.resid_ratio(A.resid_expected(c), c.run())
    note(resid_label(c), ratio)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("kind", ["int", "onehot"])
@pytest.mark.parametrize("kg,wh,ntw,ht", A.RESID_INSTANCES)
def test_resid_exact_cases_are_bit_equal(kg, wh, ntw, ht, kind):
    """Integer operands whose every partial sum is exact (the condition is evaluated on the reference): any summation tree gives the reference rounded once."""
    c = resid_case(kg, wh, ht, 19, kind)
    r = A.resid_expected(c)
    while not r.exact_ok.all():  # narrowed, never dropped
        c.X = (c.X / 2).astype(np.int32).astype(np.float32)
        r = A.resid_expected(c)
    assert np.abs(c.X).max() >= 1 and (r.ref == np.round(r.ref * 4) / 4).all()
    out = c.run()
    assert (bits(out) == bits(r.ref.astype(np.float32))).all()


@pytest.mark.parametrize("kg,wh,ntw,ht", A.RESID_INSTANCES)
def test_resid_association_is_the_one_the_source_states(kg, wh, ntw, ht):
    """The reduction is exact (a one-hot row picks t), and h + (t s + b) differs in float32 from both other associations."""
    t, b, h, want = A.find_association_probe()
    w = np.zeros((1024 * kg, D), np.float32)
    w[1024 * kg - 9] = 1.0  # (e4m3: the column scale becomes 2^-8 and the stored value 256, so t s is live)
    s = A.slab_of(A.pack(w, COLS4, A.WH_ENC[wh], 0), np.full(D, b, np.float32))
    X = np.zeros((3, 1024 * kg), np.float32)
    X[:, 1024 * kg - 9] = t
    out = A.run_resid(kg, wh, ht, X, s.slab, s.bias, np.full((3, D), h, np.float32), s.scales)
    assert (bits(out) == bits(np.float32(want))).all()


@pytest.mark.parametrize("kg", [1, 4])
def test_resid_identities(kg):
    """On weights every encoding holds exactly and real activations: WH 1 = WH 0 = WH 2 (the power-of-two column scale commutes with every rounding), the h4
    form = the row-major form (which also differ in the non-temporal weight loads), and a row's bits do not depend on its neighbours, tile or slot."""
    base = resid_case(kg, 0, 1, 32, "real")
    X, h = base.X, base.h_in
    outs = {}
    for wh, ht in ((0, 1), (1, 1), (2, 1), (0, 0)):
        s = A.resid_weights(kg, wh, "int")
        outs[wh, ht] = A.run_resid(kg, wh, ht, X, s.slab, s.bias, h, s.scales)
    for key in ((1, 1), (2, 1), (0, 0)):
        assert (bits(outs[key]) == bits(outs[0, 1])).all(), key
    perm = (np.arange(32) * 13 + 5) % 32
    s = A.resid_weights(kg, 0, "int")
    o2 = A.run_resid(kg, 0, 1, X[perm], s.slab, s.bias, h[perm], s.scales)
    o3 = A.run_resid(kg, 0, 1, X[:3], s.slab, s.bias, h[:3], s.scales)
    assert (bits(o2) == bits(outs[0, 1][perm])).all() and (bits(o3) == bits(outs[0, 1][:3])).all()


# ---------------------------------------------------------------------------------------------------------------- coverage (last: it reads what ran above)

def test_coverage():
    """Every instantiation the product launches and every layout x encoding x packer the loader builds was reached by the tests above (run the whole file)."""
    assert A.REACHED["ln"] == set(A.LN_INSTANCES), sorted(set(A.LN_INSTANCES) ^ A.REACHED["ln"])
    assert A.REACHED["resid"] == set(A.RESID_INSTANCES), sorted(set(A.RESID_INSTANCES) ^ A.REACHED["resid"])
    assert A.REACHED["pack"] >= set(A.PACK_PAIRS), sorted(set(A.PACK_PAIRS) - A.REACHED["pack"])
