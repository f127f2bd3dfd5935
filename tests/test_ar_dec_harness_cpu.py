"""CPU side of tests/test_ar_dec_kernels_gpu.py: the harness library builds for gfx950, loads and exports its surface; it refuses every invalid case before
any HIP call; the float64 reference is checked against naive loops; every host packer agrees with the NumPy restatement of its layout and encoding; a float32
restatement of each kernel's arithmetic (with and without flushed fp16 subnormals) stays inside the bound on every input family; and the SHARPNESS of the bound
is established here: every seeded defect, applied to the reference, moves some output element of a case built to expose it by at least 10 x its bound."""
import ctypes as C
import os

import numpy as np
import pytest

import ar_dec_cases as A
from ar_dec_cases import COLS4, D, E4M3, F16, F32, FF, GELU, LOGITS, MFMA16, MFMA16H, QKV, SPLIT, STRIP


def test_harness_library_builds_and_exports_its_surface():
    L = A.harness()  # builds it once if missing; raises otherwise
    for sym in ("tts_dec_test_pack", "tts_dec_test_ln_gemv", "tts_dec_test_resid", "tts_dec_test_pack_validate", "tts_dec_test_ln_gemv_validate",
                "tts_dec_test_resid_validate", "tts_dec_test_margin"):
        assert hasattr(L, sym), sym
    assert L.tts_dec_test_margin() == 4096
    src_t = max(os.path.getmtime(A.SRC), os.path.getmtime(os.path.join(A.PKG, "csrc", "ar.hip")))
    assert os.path.getmtime(A.LIB) >= src_t or os.environ.get("TTS_DEC_TEST_LIB"), "libtts_dec_test.so is older than its sources: run make"


def test_harness_is_not_part_of_the_product():
    mk = open(os.path.join(A.PKG, "Makefile")).read()
    assert "HIP_SRCS = $(wildcard csrc/*.hip)" in mk and not os.path.exists(os.path.join(A.PKG, "csrc", "ar_dec_harness.hip"))
    link = [l for l in mk.splitlines() if "-o $@ $(OBJS)" in l]
    assert len(link) == 1 and "testlib" not in link[0] and "dec_test" not in link[0]
    assert "libtts_dec_test.so" in [l for l in mk.splitlines() if l.startswith("all:")][0]
    assert "libtts_dec_test.so" in mk.split("clean:")[1]
    src = open(A.SRC).read()
    assert '#include "../csrc/ar.hip"' in src and "asm" not in src and "__global__" not in src  # the product's kernels, none of its own


def test_instance_tables_name_what_the_product_launches():
    assert len(A.LN_INSTANCES) == 22 and len(A.RESID_INSTANCES) == 8
    assert len({i for i in A.LN_INSTANCES if i[3] == 0}) == 6 and len({i for i in A.LN_INSTANCES if i[4] == 1}) == 4


# ---------------------------------------------------------------------------------------------------------------- the reference against naive loops

def test_layernorm_reference_agrees_with_naive_loops():
    h = A.make_rows(6, 0)
    y, _ = A.ln_stage(h.astype(np.float64))
    for r in range(6):
        x = [float(v) for v in h[r]]
        mean = sum(x) / D
        var = sum((v - mean) ** 2 for v in x) / D
        for k in (0, 1, 255, 256, 1023):
            assert abs(y[r, k] - (x[k] - mean) / (var + 1e-5) ** 0.5) <= 1e-9 * (1 + abs(y[r, k]))


@pytest.mark.parametrize("split", [0, 1, 2, 3])
def test_kernel_reference_agrees_with_naive_loops(split):
    """ln_expected's matrix product on the slab's decoded values against a loop over the HOLDS of the slab, element by element through the prose of the layout."""
    c = A.ln_case(LOGITS, split, 1, 3, 0, N=32)
    r = A.ln_expected(c)
    raw = c.slab.slab
    g1, b1 = [a.astype(np.float64) for a in A.head_affine()]
    for row, n in ((0, 0), (1, 17), (2, 31)):
        x = c.h[row].astype(np.float64)
        x = (x - x.mean()) / np.sqrt(x.var() + 1e-5) * g1 + b1
        x = (x - x.mean()) / np.sqrt(x.var() + 1e-5)
        acc = float(c.slab.bias[n])
        cb, m = n // 16, n % 16
        for k in range(D):
            if split == 0:  # mfma16: wave k / 256, group (k % 256) / 16, lane quarter (k % 16) / 4, j = k % 4
                wv, g, q, j = k // 256, (k % 256) // 16, (k % 16) // 4, k % 4
                w = float(raw.view(np.float32)[(((cb * 4 + wv) * 16 + g) * 64 + 16 * q + m) * 4 + j])
            else:           # mfma16h: wave, K step (k % 256) / 32, quarter (k % 32) / 8, e = k % 8
                wv, s, q, e = k // 256, (k % 256) // 32, (k % 32) // 8, k % 8
                i = (((cb * 4 + wv) * 8 + s) * 64 + 16 * q + m) * 8 + e
                if split == 1:
                    hl = raw.view(np.float16)
                    w = (float(hl[(i // 8) * 16 + e]) + float(hl[(i // 8) * 16 + 8 + e])) / 64
                elif split == 2:
                    w = float(raw.view(np.float16)[i]) / 64
                else:
                    byte = raw[((((cb * 4 + wv) * 4 + s // 2) * 64 + 16 * q + m) * 2 + s % 2) * 8 + e]
                    w = A.E4M3_TABLE[byte] * float(c.slab.scales[n])
            acc += x[k] * w
        assert abs(acc - r.ref[row, n]) <= 1e-11 * (1 + abs(acc)), (row, n)


def test_resid_reference_agrees_with_naive_loops():
    s = A.resid_weights(4, 0, "real")
    rs = np.random.RandomState(0)
    c = A.ResidCase(4, 0, 1, rs.randn(3, 4096).astype(np.float32), s, rs.randn(3, D).astype(np.float32))
    r = A.resid_expected(c)
    raw = s.slab.view(np.float32)
    for row, n in ((0, 0), (2, 1023), (1, 514)):
        acc = float(c.h_in[row, n]) + float(s.bias[n])
        for k in range(4096):  # cols4: workgroup n / 4, K group k / 1024, kk = k % 4, thread (k % 1024) / 4, column n % 4
            acc += float(c.X[row, k]) * float(raw[((((n // 4) * 4 + k // 1024) * 4 + k % 4) * 256 + (k % 1024) // 4) * 4 + n % 4])
        assert abs(acc - r.ref[row, n]) <= 1e-11 * (1 + abs(acc))


def test_h4_restatement_agrees_with_the_source():
    L = A.harness()
    for r, k in ((0, 0), (1, 0), (0, 1), (0, 4), (15, 1023), (16, 0), (17, 5), (31, 1023), (33, 258)):
        assert int(A.h4_index(r, k)) == L.tts_dec_test_h4_index(r, k)
    idx = A.h4_index(np.arange(32)[:, None], np.arange(D)[None, :]).reshape(-1)
    assert sorted(idx.tolist()) == list(range(32 * D))


def test_e4m3_restatement():
    L = A.harness()
    t = A.E4M3_TABLE
    assert t[0x7e] == 448.0 and t[0x08] == 2.0 ** -6 and t[0x01] == 2.0 ** -9 and np.isnan(t[0x7f])
    rs = np.random.RandomState(0)
    xs = np.concatenate([t[np.isfinite(t)], (t[:0x7e] + t[1:0x7f]) / 2, rs.randn(2000) * 50, rs.randn(2000) * 0.01, [448.0, 464.0, 500.0, -1e9, 2.0 ** -10, 3 * 2.0 ** -10]])
    got = np.array([L.tts_dec_test_fp8(float(np.float32(x))) for x in xs], np.uint8)
    want = A.e4m3_encode(xs.astype(np.float32))
    zero = (got & 0x7f) == 0  # the sign of a value that rounds to zero is kept on both sides; compare values
    assert (got[~zero] == want[~zero]).all() and ((want[zero] & 0x7f) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- host packers against the restatement

PACKS = [(STRIP, F32, 1024, 128), (STRIP, F32, 96, 64), (MFMA16, F32, 1024, 48), (MFMA16H, SPLIT, 1024, 48), (MFMA16H, F16, 1024, 48), (MFMA16H, E4M3, 1024, 48),
         (COLS4, F32, 1024, 20), (COLS4, F32, 4096, 20), (COLS4, F16, 1024, 20), (COLS4, F16, 4096, 20), (COLS4, E4M3, 1024, 20), (COLS4, E4M3, 4096, 20)]


def packer_matrix(K, N):
    w, g, b, c = A.make_weights(64, 0, True)
    w = np.tile(w, (max(1, K // D), 2))[:K, :N].copy()
    return w, np.resize(g, K), np.resize(b, K), np.resize(c, N)


def stored_equal(got, want):
    if isinstance(want, tuple):
        return all(stored_equal(a, b) for a, b in zip(got, want))
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(np.uint8) == b.view(np.uint8)).all())


@pytest.mark.parametrize("layout,enc,K,N", PACKS)
@pytest.mark.parametrize("fold", [0, 1])
def test_host_packer_agrees_with_the_restatement(layout, enc, K, N, fold):
    w, g, b, c = packer_matrix(K, N)
    p = A.pack(w, layout, enc, 0, *((g, b, c) if fold else (None, None, None)))
    wf = w
    if fold:
        wf, cf = A.fold_ref(w, g, b, c)
        assert stored_equal(p.bias, cf), "folded bias differs from the double sum in ascending k"
    assert stored_equal(p.fold, wf), "folded matrix differs from float32(g w)"
    assert stored_equal(p.scales, A.fp8_scales(wf)), "fp8 column scales differ from their definition"
    assert stored_equal(p.stored, A.encode(enc, wf, scale64=layout != COLS4))


def test_fp8_scales_at_the_edge():
    w = np.zeros((4, 8), np.float32)
    top = np.float32(448.0 * 2.0 ** -12)
    w[1] = [top, np.nextafter(top, np.float32(1)), np.nextafter(top, np.float32(0)), 0.0, 448.0, 1e-30, 0.5, 449.0]
    s = A.fp8_scales(w)
    assert s.tolist()[:5] == [2.0 ** -12, 2.0 ** -11, 2.0 ** -12, 1.0, 1.0]
    p = A.pack(np.tile(w, (256, 1)), COLS4, E4M3, 0)
    assert stored_equal(p.scales, A.fp8_scales(np.tile(w, (256, 1))))


# ---------------------------------------------------------------------------------------------------------------- validation (no HIP call is reached)

def _ln_kw(epi=QKV, split=1, ht=1, ro=0, rows=3, **kw):
    N = {QKV: 3 * D, GELU: FF, LOGITS: 64}[epi]
    s = A.ln_slab(N, split)
    d = dict(epi=epi, split=split, ht=ht, ro=ro, h=A.make_rows(rows, 0), slab=s.slab, bias=s.bias, N=N, wscale=s.scales, n_past=1, max_pos=4, n_slots=4)
    if epi == LOGITS:
        d.update(g1=A.head_affine()[0], b1=A.head_affine()[1])
    d.update(kw)
    return d


def _ln_rc(kw, patch=None):
    cs = A.run_ln(validate_only=True, **kw)
    for k, v in (patch or {}).items():
        setattr(cs, k, v)
    L = A.harness()
    rc = L.tts_dec_test_ln_gemv_validate(C.byref(cs))
    if rc != 0:  # refused by the run entry too, before any HIP call (this machine has no GPU: a HIP call would return another code)
        assert L.tts_dec_test_ln_gemv(C.byref(cs)) == A.HIP_INVALID_VALUE
    return rc


def test_valid_ln_cases_validate():
    for inst in A.LN_INSTANCES:
        epi, split, ntw, ht, ro = inst
        kw = _ln_kw(epi, split, ht, ro, rows=3, prefill_B=(2 if epi == QKV and not ht else 0), row_off=np.array([1, -1, 2] + [0] * 13, np.int32) if ro else None)
        assert _ln_rc(kw) == 0, inst


def _bad_slab(split, value):
    s = A.ln_slab(3 * D, split).slab.copy()
    s.view(np.float16)[12345] = value
    return s


LN_INVALID = [
    ("prompt form on SPLIT 2", dict(split=2, ht=0, prefill_B=1), {}), ("prompt form on SPLIT 3", dict(split=3, ht=0, prefill_B=1), {}),
    ("RO outside QKV", dict(epi=GELU), dict(ro=1)), ("NTW false on SPLIT 1", {}, dict(ntw=0)), ("NTW true on SPLIT 2", dict(split=2), dict(ntw=1)),
    ("unknown epilogue", {}, dict(epi=3)), ("unknown split", {}, dict(split=4)), ("decode form off h4", dict(ht=0), {}), ("prompt form on h4", dict(prefill_B=1), {}),
    ("rows 0", {}, dict(rows=0)), ("rows above the cap", {}, dict(rows=65)), ("N no multiple of 16", dict(epi=LOGITS), dict(N=56)),
    ("n_valid > N", dict(epi=LOGITS), dict(n_valid=65)), ("n_valid 0", dict(epi=LOGITS), dict(n_valid=0)), ("ldo < n_valid", dict(epi=LOGITS, n_valid=50), dict(ldo=49)),
    ("q ldo < 1024", {}, dict(ldo=1020)), ("q ldo no multiple of 4", {}, dict(ldo=1026)), ("QKV N", {}, dict(N=3056)), ("GELU N", dict(epi=GELU), dict(N=4080)),
    ("n_past = max_pos", dict(n_past=4), {}), ("n_past < 0", dict(n_past=-1), {}),
    ("row_off past the cache", dict(ro=1, row_off=np.array([0, 3, 0] + [0] * 13, np.int32)), {}),
    ("row_off before the cache", dict(ro=1, row_off=np.array([0, -2, 0] + [0] * 13, np.int32)), {}),
    ("row_off padding not zero", dict(ro=1, row_off=np.array([0, 0, 0, 1] + [0] * 12, np.int32)), {}),
    ("RO without row_off", dict(ro=1), {}), ("rows > slots", dict(n_slots=2), {}), ("max_pos 0", dict(max_pos=0), {}), ("max_pos 1025", dict(max_pos=1025), {}),
    ("prefill_B 0 slots", dict(ht=0, prefill_B=5), {}), ("prefill_B < 0", dict(ht=0), dict(prefill_B=-1)), ("prompt rows > max_pos", dict(ht=0, prefill_B=1, max_pos=2), {}),
    ("split slab past the range guard", dict(slab=_bad_slab(1, 60000.0)), {}), ("fp16 slab holds an infinity", dict(split=2, slab=_bad_slab(2, np.inf)), {}),
    ("split slab holds a NaN", dict(slab=_bad_slab(1, np.nan)), {}),
    ("fp8 scale no power of two", dict(split=3, wscale=np.full(3 * D, 3.0, np.float32)), {}), ("fp8 scale 0", dict(split=3, wscale=np.zeros(3 * D, np.float32)), {}),
    ("fp8 scale negative", dict(split=3, wscale=np.full(3 * D, -2.0, np.float32)), {}), ("fp8 without scales", dict(split=3), dict(wscale=None)),
    ("no h", {}, dict(h=None)), ("no slab", {}, dict(slab=None)), ("no bias", {}, dict(bias=None)), ("no out", {}, dict(out=None)), ("no K cache", {}, dict(kc=None)),
    ("no V cache", {}, dict(vc=None)), ("head without g1", dict(epi=LOGITS), dict(g1=None)), ("head without b1", dict(epi=LOGITS), dict(b1=None)),
    ("slab size", {}, dict(slab_bytes=100)), ("lut 2", {}, dict(lut=2)),
]


@pytest.mark.parametrize("name,kw,patch", LN_INVALID, ids=[i[0] for i in LN_INVALID])
def test_invalid_ln_cases_are_refused(name, kw, patch):
    assert _ln_rc(_ln_kw(**kw), patch) == A.HIP_INVALID_VALUE


def _resid_rc(kg=1, wh=0, ht=1, patch=None, **kw):
    s = A.resid_weights(kg, wh, "int")
    d = dict(kg=kg, wh=wh, ht=ht, X=np.zeros((3, 1024 * kg), np.float32), slab=s.slab, bias=s.bias, h_in=np.zeros((3, D), np.float32), wscale=s.scales)
    d.update(kw)
    cs = A.run_resid(validate_only=True, **d)
    for k, v in (patch or {}).items():
        setattr(cs, k, v)
    L = A.harness()
    rc = L.tts_dec_test_resid_validate(C.byref(cs))
    if rc != 0:
        assert L.tts_dec_test_resid(C.byref(cs)) == A.HIP_INVALID_VALUE
    return rc


def test_resid_validation():
    for kg, wh, ntw, ht in A.RESID_INSTANCES:
        assert _resid_rc(kg, wh, ht) == 0
    bad = [dict(kg=2), dict(wh=1, ht=0), dict(wh=2, ht=0), dict(patch=dict(ntw=0)), dict(ht=0, patch=dict(ntw=1)), dict(wh=1, patch=dict(ntw=1)),
           dict(patch=dict(rows=0)), dict(patch=dict(rows=65)), dict(patch=dict(X=None)), dict(patch=dict(slab=None)), dict(patch=dict(bias=None)),
           dict(patch=dict(h_in=None)), dict(patch=dict(h_out=None)), dict(patch=dict(slab_bytes=8)), dict(wh=2, patch=dict(wscale=None)),
           dict(wh=2, wscale=np.full(D, 0.75, np.float32)), dict(wh=2, wscale=np.zeros(D, np.float32)), dict(patch=dict(wh=3))]
    for b in bad:
        if b.get("kg") == 2:
            with pytest.raises(Exception):
                _resid_rc(**b)  # no such slab exists; the validator is reached below
            assert _resid_rc(patch=dict(kg=2)) == A.HIP_INVALID_VALUE
            continue
        assert _resid_rc(**b) == A.HIP_INVALID_VALUE, b


def test_pack_validation():
    L = A.harness()
    w = np.zeros((1024, 64), np.float32)

    def rc(**kw):
        d = dict(K=1024, N=64, layout=MFMA16H, enc=SPLIT, where=0, transpose=0, vrows=0, W=w, slab_bytes=A.slab_bytes(1024, 64, MFMA16H, SPLIT),
                 slab=A.Guarded((A.slab_bytes(1024, 64, MFMA16H, SPLIT),), np.uint8))
        d.update(kw)
        cs = A.fill_struct(A.PackStruct(), **d)
        r = L.tts_dec_test_pack_validate(C.byref(cs))
        if r != 0:
            assert L.tts_dec_test_pack(C.byref(cs)) == A.HIP_INVALID_VALUE
        return r

    assert rc() == 0
    for bad in (dict(W=None), dict(K=512), dict(N=56), dict(layout=5), dict(enc=F32), dict(where=2), dict(slab_bytes=64), dict(g=w[0]), dict(transpose=1, vrows=10),
                dict(layout=MFMA16, enc=F32, where=1, slab_bytes=1024 * 64 * 4), dict(layout=MFMA16H, enc=F16, where=1, slab_bytes=1024 * 64 * 2),
                dict(layout=COLS4, enc=E4M3, where=1, slab_bytes=1024 * 64), dict(layout=COLS4, enc=F32, K=2048, slab_bytes=2048 * 64 * 4),
                dict(layout=STRIP, enc=F32, N=32, slab_bytes=1024 * 32 * 4), dict(layout=A.SPLITW, enc=SPLIT, where=0), dict(K=0), dict(N=0)):
        assert rc(**bad) == A.HIP_INVALID_VALUE, bad


# ---------------------------------------------------------------------------------------------------------------- the bound admits plain float32 arithmetic

@pytest.mark.parametrize("split", [0, 1, 2, 3])
def test_f32_restatement_of_ln_gemv_passes_the_bound_on_every_family(split):
    seen = set()
    for rows, rot in A.ROW_CASES:
        c = A.ln_case(LOGITS, split, 1, rows, rot, n_valid=50, ldo=70)
        seen |= {(A.family_of(r, rot), r % 16) for r in range(rows)}
        e = A.ln_expected(c)
        for flush in (False, True):
            ratio, what = A.ln_check(e, *A.emulate_ln(c, flush))
            assert ratio <= 1.0, (c.tag, flush, ratio, what)
    assert {f for f, s in seen if s == 0} == set(A.FAMILIES) and {f for f, s in seen if s == 15} == set(A.FAMILIES)


@pytest.mark.parametrize("epi,split,lut", [(QKV, 1, 0), (QKV, 3, 0), (GELU, 0, 0), (GELU, 1, 1), (GELU, 2, 0)])
def test_f32_restatement_of_the_epilogues_passes_the_bound(epi, split, lut):
    c = A.ln_case(epi, split, 1, 19, 2, n_past=2, max_pos=4, lut=lut, ro=int(epi == QKV), row_off=np.array([(r % 3) - 1 for r in range(19)] + [0] * 13, np.int32))
    e = A.ln_expected(c)
    for flush in (False, True):
        ratio, what = A.ln_check(e, *A.emulate_ln(c, flush))
        assert ratio <= 1.0, (flush, ratio, what)


@pytest.mark.parametrize("kg,wh", [(1, 0), (4, 0), (1, 1), (4, 2)])
def test_f32_restatement_of_gemv_resid_passes_the_bound(kg, wh):
    c = resid_real_case(kg, wh, 19)
    assert A.resid_ratio(A.resid_expected(c), A.emulate_resid(c)) <= 1.0


def resid_real_case(kg, wh, rows):
    rs = np.random.RandomState(kg + wh)
    X = rs.randn(rows, 1024 * kg).astype(np.float32)
    X[1::2] = rs.standard_t(3, X[1::2].shape).astype(np.float32)
    return A.ResidCase(kg, wh, 1, X, A.resid_weights(kg, wh, "real"), rs.randn(rows, D).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- sharpness: every seeded defect is seen

def aligned_case(split, which="x", epi=LOGITS):
    """A case whose column n < 32 is aligned with row n % 16: w_k = c sign(xhat_k) (which = x), or c sign(xl_k) on the channels whose lo part is at least 0.8 of
    its largest (which = xl), with 64 c = 1 + 0.9 x 2^-11, a weight whose own lo part is as large as lo parts get. GELU: one LayerNorm, the pre-activation
    sum |xhat| c ~ 12, where GELU is the identity to 1e-30."""
    rows, N = 16, 32 if epi == LOGITS else FF
    h = np.random.RandomState(9).randn(rows, D).astype(np.float32)  # plain Gaussian rows
    g1, b1 = A.head_affine()
    xhat = h.astype(np.float64)
    if epi == LOGITS:
        xhat, _ = A.ln_stage(xhat, None, g1.astype(np.float64), b1.astype(np.float64))
    xhat, _ = A.ln_stage(xhat)
    cw = (1.0 + 0.9 * 2.0 ** -11) / 64
    w = np.zeros((D, N), np.float32)
    for n in range(32):
        x = xhat[n % rows].astype(np.float32)
        if which == "x":
            w[:, n] = cw * np.sign(x)
        else:
            xl = x.astype(np.float64) - x.astype(np.float16).astype(np.float64)
            w[:, n] = np.where(np.abs(xl) >= 0.8 * 2.0 ** -12 * np.abs(x), cw * np.sign(xl), 0.0)
    c = np.zeros(N, np.float32)
    return A.LnCase(epi, split, 1, h, A.custom_slab(w, c, split), g1=g1 if epi == LOGITS else None, b1=b1 if epi == LOGITS else None)


def gelu_probe(lut):
    """GELU on tiny weights and a bias that sweeps [-4, 4]: the pre-activation is the bias, the bound a few u."""
    w = (1e-5 * np.random.RandomState(2).randn(D, FF)).astype(np.float32)
    c = np.linspace(-4, 4, FF).astype(np.float32)
    return A.LnCase(GELU, 0, 1, A.make_rows(16, 0), A.custom_slab(w, c, 0), lut=lut)


def qkv_case():
    return A.ln_case(QKV, 1, 1, 19, 0, ro=1, n_past=1, max_pos=4, row_off=np.array([(r % 3) - 1 for r in range(19)] + [0] * 13, np.int32))


EXPOSE = {
    "eps_dropped": lambda: A.ln_case(LOGITS, 1, 1, 16, 0), "eps_wrong": lambda: A.ln_case(LOGITS, 1, 1, 16, 0),
    "unbiased_var": lambda: aligned_case(1), "one_ln_head": lambda: A.ln_case(LOGITS, 1, 1, 16, 0),
    "lohi_dropped": lambda: aligned_case(1, "x", GELU), "hilo_dropped": lambda: aligned_case(1, "xl", GELU),
    "fp8_neighbour_scale": lambda: A.ln_case(LOGITS, 3, 1, 16, 0),
    "kv_late": qkv_case, "row_off_ignored": qkv_case, "kv_swapped": qkv_case, "q_unrounded": qkv_case,
    "erf_gelu": lambda: gelu_probe(0), "wrong_lut": lambda: gelu_probe(0),
    "drop_last_valid": lambda: A.ln_case(LOGITS, 1, 1, 3, 0, n_valid=50, ldo=70), "store_n_valid": lambda: A.ln_case(LOGITS, 1, 1, 3, 0, n_valid=50, ldo=70),
}


@pytest.mark.parametrize("defect", A.DEFECTS_LN)
def test_every_ln_defect_moves_an_element_by_ten_bounds(defect):
    c = EXPOSE[defect]()
    assert A.ln_check(A.ln_expected(c), *A.ln_render(A.ln_expected(c)))[0] <= 1.0  # the unmutated reference passes its own check
    assert A.ln_defect_ratio(c, defect) >= 10.0, (defect, A.ln_defect_ratio(c, defect))


def test_wrong_lut_is_seen_from_the_lut_side_too():
    assert A.ln_defect_ratio(gelu_probe(1), "wrong_lut") >= 10.0


@pytest.mark.parametrize("defect", A.DEFECTS_FOLD)
def test_every_fold_defect_moves_an_element_by_ten_bounds(defect):
    """The slab's reference against the UNFOLDED formula (LN(x) g + b) . w + c: equal within the bound plus the fold's own roundings (u |g w| per weight, u |cf|);
    a fold without the gain, or without b . w, is not."""
    w, g, b, c = A.make_weights(64, 0, True)
    case = A.ln_case(LOGITS, 0, 1, 16, 0)
    r = A.ln_expected(case)
    g1, b1 = [a.astype(np.float64) for a in A.head_affine()]
    y, _ = A.ln_stage(case.h.astype(np.float64), None, g1, b1)
    xhat, _ = A.ln_stage(y)
    g64, b64, w64 = g.astype(np.float64), b.astype(np.float64), w.astype(np.float64)
    unfolded = (xhat * g64 + b64) @ w64 + c
    B = r.B + A.U * (np.abs(xhat) @ np.abs(g64[:, None] * w64)) + A.U * np.abs(case.slab.bias)
    assert (np.abs(unfolded - r.ref) <= B).all()
    wrong = xhat @ w64 + case.slab.bias.astype(np.float64) if defect == "gain_not_folded" else xhat @ (g64[:, None] * w64) + c
    assert (np.abs(wrong - r.ref) / B).max() >= 10.0


RESID_EXPOSE = {"last_kgroup_dropped": (4, 0), "cols_swapped": (1, 0), "cand_mirror": (1, 2), "bias_twice": (4, 1), "resid_dropped": (1, 0)}


@pytest.mark.parametrize("defect", A.DEFECTS_RESID)
def test_every_resid_defect_moves_an_element_by_ten_bounds(defect):
    c = resid_real_case(*RESID_EXPOSE[defect], rows=19)
    r = A.resid_expected(c)
    assert A.resid_ratio(r, A.resid_expected(c, defect).ref.astype(np.float32)) >= 10.0


def test_association_probe_separates_the_three_associations():
    t, b, h, want = A.find_association_probe()
    f = np.float32
    assert want == f(h + f(t + b)) and want != f(f(h + t) + b) and want != f(f(h + b) + t)
