"""CPU side of tests/test_ar_attn_kernels_gpu.py: the harness library builds for gfx950, loads and exports its surface; it refuses every invalid case before
any HIP call; the float64 reference is checked against naive loops; and the SHARPNESS of the case matrix is established here: every mutation of the reference
a variant is built to expose moves some output element by at least 10 x that element's bound, so the bound cannot hide a kernel that drops or admits a key."""
import ctypes as C
import os

import numpy as np
import pytest

import ar_attn_cases as A
from ar_attn_cases import ATTENTION, DECODE, DECODE_FAST, EPILOGUE, RAGGED, ROWS, D


def test_harness_library_builds_and_exports_its_surface():
    L = A.harness()  # builds it once if missing; raises otherwise
    for sym in ("tts_ar_test_run", "tts_ar_test_validate", "tts_ar_test_margin"):
        assert hasattr(L, sym), sym
    assert L.tts_ar_test_margin() == 4096
    src_t = max(os.path.getmtime(A.SRC), os.path.getmtime(os.path.join(A.PKG, "csrc", "ar.hip")))
    assert os.path.getmtime(A.LIB) >= src_t or os.environ.get("TTS_AR_TEST_LIB"), "libtts_ar_test.so is older than its sources: run make"


def test_harness_is_not_part_of_the_product():
    mk = open(os.path.join(A.PKG, "Makefile")).read()
    assert "HIP_SRCS = $(wildcard csrc/*.hip)" in mk and not os.path.exists(os.path.join(A.PKG, "csrc", "ar_attn_harness.hip"))
    link = [l for l in mk.splitlines() if "-o $@ $(OBJS)" in l]
    assert len(link) == 1 and "testlib" not in link[0] and "ar_test" not in link[0]
    src = open(A.SRC).read()
    assert '#include "../csrc/ar.hip"' in src and "asm" not in src and "__global__" not in src  # the product's kernels, none of its own


# ---------------------------------------------------------------------------------------------------------------- validation (no HIP call is reached)

def _valid_case(kernel):
    """A small valid case of every kind, as keyword arguments of A.struct()."""
    f32, u16 = np.float32, np.uint16
    kc, vc = np.zeros((2, 16, D), u16), np.zeros((2, 16, D), u16)
    if kernel in (ATTENTION, ROWS):
        return dict(kernel=kernel, q=np.zeros((2 * 5, 3 * D), f32), kc=kc, vc=vc, n_cand=2, S=5, n_past=3, max_pos=16, out=A.Guarded((10, D), f32))
    if kernel == RAGGED:
        return dict(kernel=kernel, q=np.zeros((9, 3 * D), f32), kc=kc, vc=vc, n_cand=2, max_pos=16, n_rows=9,
                    items=np.array([[0, 4, 2, 1], [4, 5, 0, 0]], np.int32), out=A.Guarded((9, D), f32))
    if kernel in (DECODE_FAST, DECODE):
        return dict(kernel=kernel, q=np.zeros((2, D), f32), kc=kc, vc=vc, n_cand=2, n_past=4, max_pos=16, ro=1, row_off=np.array([0, -3], np.int32),
                    out=A.Guarded((2, D), f32))
    raise ValueError(kernel)


def _rc(kw, run=True):
    cs = A.struct(**kw)
    L = A.harness()
    rc = L.tts_ar_test_validate(C.byref(cs))
    if rc != 0 and run:  # an invalid case is refused by the run entry too, before any HIP call (this machine has no GPU: a HIP call would return another code)
        assert L.tts_ar_test_run(C.byref(cs)) == A.HIP_INVALID_VALUE
    return rc


@pytest.mark.parametrize("kernel", [ATTENTION, ROWS, RAGGED, DECODE_FAST, DECODE])
def test_valid_cases_validate(kernel):
    assert _rc(_valid_case(kernel), run=False) == 0


INVALID = [
    ("max_pos 0", ROWS, dict(max_pos=0)), ("max_pos 1025", ROWS, dict(max_pos=1025)), ("max_pos 1025 attention", ATTENTION, dict(max_pos=1025)),
    ("n_past < 0", ROWS, dict(n_past=-1)), ("S 0", ROWS, dict(S=0)), ("S 0 attention", ATTENTION, dict(S=0)),
    ("n_past + S > max_pos", ROWS, dict(n_past=12)), ("n_past + S > max_pos attention", ATTENTION, dict(n_past=12)),
    ("n_past overflow", ROWS, dict(n_past=2 ** 31 - 1)),
    ("n_cand 0", ROWS, dict(n_cand=0)), ("rows kernel has no lut", ROWS, dict(lut=1)), ("no q", ROWS, dict(q=None)), ("no cache", ROWS, dict(kc=None)),
    ("no out", ATTENTION, dict(out=None)), ("unknown kernel", ROWS, dict(kernel=7)),
    ("decode nk 0", DECODE_FAST, dict(row_off=np.array([0, -5], np.int32))), ("decode nk 0 exact", DECODE, dict(row_off=np.array([0, -5], np.int32))),
    ("decode nk < 0", DECODE_FAST, dict(row_off=np.array([-9, 0], np.int32))), ("decode nk > max_pos", DECODE_FAST, dict(row_off=np.array([0, 12], np.int32))),
    ("decode nk > max_pos exact", DECODE, dict(row_off=np.array([12, 0], np.int32))),
    ("decode n_past -1 without row_off", DECODE_FAST, dict(n_past=-1, ro=0, row_off=None)), ("decode n_past = max_pos", DECODE, dict(n_past=16, ro=0, row_off=None)),
    ("decode ro without row_off", DECODE_FAST, dict(row_off=None, ro=1)), ("decode fast has no lut", DECODE_FAST, dict(lut=1)),
    ("ragged slot out of range", RAGGED, dict(items=np.array([[0, 4, 2, 2], [4, 5, 0, 0]], np.int32))),
    ("ragged slot < 0", RAGGED, dict(items=np.array([[0, 4, 2, -1], [4, 5, 0, 0]], np.int32))),
    ("ragged rows past the row space", RAGGED, dict(items=np.array([[0, 4, 2, 1], [5, 5, 0, 0]], np.int32))),
    ("ragged first row < 0", RAGGED, dict(items=np.array([[-1, 4, 2, 1], [4, 5, 0, 0]], np.int32))),
    ("ragged items overlap", RAGGED, dict(items=np.array([[0, 5, 2, 1], [4, 5, 0, 0]], np.int32))),
    ("ragged S 0", RAGGED, dict(items=np.array([[0, 0, 2, 1], [4, 5, 0, 0]], np.int32))),
    ("ragged n_past + S > max_pos", RAGGED, dict(items=np.array([[0, 4, 13, 1], [4, 5, 0, 0]], np.int32))),
    ("ragged n_past < 0", RAGGED, dict(items=np.array([[0, 4, -1, 1], [4, 5, 0, 0]], np.int32))),
    ("ragged without items", RAGGED, dict(items=None)), ("ragged n_rows 0", RAGGED, dict(n_rows=0)),
]


@pytest.mark.parametrize("name,kernel,change", INVALID, ids=[i[0].replace(" ", "_") for i in INVALID])
def test_invalid_cases_are_refused_before_any_launch(name, kernel, change):
    kw = _valid_case(kernel)
    kw.update(change)
    assert _rc(kw) == A.HIP_INVALID_VALUE


def test_invalid_epilogue_cases_are_refused():
    f32 = np.float32
    part, bias = np.zeros((3, 3 * D), f32), np.zeros(3 * D, f32)

    def rc(row_dst, n_cand=2, max_pos=4, pscale=1.0 / 64, n_rows=3, drop=()):
        g = dict(out=A.Guarded((n_rows, 3 * D), f32), out2=A.Guarded((n_rows, 3 * D), f32), kout=A.Guarded((n_cand, max_pos, D), np.uint16),
                 vout=A.Guarded((n_cand, max_pos, D), np.uint16), kout2=A.Guarded((n_rows, D), np.uint16), vout2=A.Guarded((n_rows, D), np.uint16))
        rd = np.array(row_dst, np.int32)
        ptr = dict(part=part, bias=bias, row_dst=rd)
        kw = dict(pscale=pscale)
        for k, v in list(ptr.items()) + [(k, v.raw) for k, v in g.items()]:
            if k not in drop:
                kw[k] = v.ctypes.data_as(C.c_void_p)
        cs = A.struct(EPILOGUE, n_cand=n_cand, max_pos=max_pos, n_rows=n_rows, **kw)
        cs._keep2 = (g, rd)
        L = A.harness()
        r = L.tts_ar_test_validate(C.byref(cs))
        if r:
            assert L.tts_ar_test_run(C.byref(cs)) == A.HIP_INVALID_VALUE
        return r

    assert rc([5, 0, 7]) == 0
    assert rc([5, 0, 8]) == A.HIP_INVALID_VALUE       # cache row out of range
    assert rc([5, -1, 7]) == A.HIP_INVALID_VALUE
    assert rc([5, 0, 5]) == A.HIP_INVALID_VALUE       # two rows, one destination
    assert rc([5, 0, 7], pscale=0.0) == A.HIP_INVALID_VALUE
    assert rc([5, 0, 7], n_rows=0) == A.HIP_INVALID_VALUE
    for missing in ("part", "bias", "row_dst", "out", "out2", "kout", "vout", "kout2", "vout2"):
        assert rc([5, 0, 7], drop=(missing,)) == A.HIP_INVALID_VALUE, missing


# ---------------------------------------------------------------------------------------------------------------- reference

@pytest.mark.parametrize("R,P,n_past", [(1, 1, 0), (3, 5, 2), (4, 9, 0)])
def test_reference_against_naive_loops(R, P, n_past):
    rng = np.random.RandomState(R * 100 + P)
    q, K, V = (A.f16(rng.randn(n, A.NH, A.HD))[0] for n in (R, P, P))
    nk = n_past + 1 + np.arange(R)
    ref = A.reference(q, K, V, A.causal_mask(nk, P))["out"]
    for r in range(R):
        for h in (0, 7, 15):
            s = [sum(float(q[r, h, i]) * float(K[j, h, i]) for i in range(A.HD)) / 8.0 for j in range(nk[r])]
            w = [np.exp(x - max(s)) for x in s]
            for d in (0, 31, 63):
                o = sum(w[j] * float(V[j, h, d]) for j in range(nk[r])) / sum(w)
                assert abs(o - ref[r, h, d]) <= 1e-13 * max(1.0, abs(o))


def test_reference_poison_and_empty_rows():
    rng = np.random.RandomState(5)
    q, K, V = (A.f16(rng.randn(n, A.NH, A.HD))[0] for n in (2, 6, 6))
    v = A.Variant("poison", "t", [], q, K, V, [3, 4], poison_from=4)
    assert np.isfinite(v.ref()["out"]).all() and np.isfinite(v.bound("rows")).all() and (v.bound("rows") > 0).all()
    assert (v.bits(v.K)[4:] == A.F16_NAN).all() and (v.bits(v.V)[:4] != A.F16_NAN).all()
    admitted = A.reference(v.q, v.K, v.V, A.mutate("admit_one", A.ROWS_STRUCT, v.nk, v.P))["out"]
    assert np.isfinite(admitted[0]).all() and np.isnan(admitted[1]).all()  # row 0 admits key 3 (data), row 1 admits the poisoned key 4
    assert np.isnan(A.reference(q, K, V, np.zeros((2, 6), bool))["out"]).all()


def test_inputs_are_fp16_without_subnormals_and_ramps_are_strict():
    for v in A.rows_variants(40, 281) + A.decode_variants(289):
        for a in (v.q, np.where(np.isnan(v.K), 1.0, v.K), np.where(np.isnan(v.V), 1.0, v.V)):
            assert (a.astype(np.float16).astype(np.float32) == a).all()
            assert ((a == 0) | (np.abs(a) >= 2.0 ** -14)).all()
        if v.family == "ramp":
            s = v.ref()["s"][:, :, :int(v.nk[-1])]
            d = np.diff(s, axis=2)
            assert (d > 0).all() if v.tag == "up" else (d < 0).all()
        if v.family == "flat":
            assert 0.8 < v.ref()["s"][:, :, :int(v.nk[-1])].std() < 1.25
        if v.family == "peaked":
            sc = v.ref()["s"][-1]  # all cache rows: the placement `beyond` is visible to no row
            assert sc.max() > 25 and sc.min() < -22 and ((sc > 0).sum(axis=1) == 1).all()


# ---------------------------------------------------------------------------------------------------------------- sharpness

def _moved(v, st, name, kinds):
    """max over elements of |mutated reference - reference| / bound for mutation `name` of variant v, or None where the mutation touches no key."""
    m = A.mutate(name, st, v.nk, v.P)
    if m is None:
        return None
    mut = A.reference(v.q, v.K, v.V, m, s=v.ref()["s"])["out"]
    b = np.maximum.reduce([v.bound(k) for k in kinds])
    d = np.abs(mut - v.ref()["out"])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(d == 0, 0.0, d / b)
    return float(np.where(np.isnan(r), np.inf, r).max())


def _check_sharp(vs, st, kinds, lut):
    exists = {n for n in A.mutation_names(st) if A.mutate(n, st, vs[0].nk, vs[0].P) is not None}
    fams = {}
    for v in vs:
        if lut:
            assert A.lut_condition(v.ref(), v.mask()), (v.family, v.tag)
        if v.family != "flat":
            fams.setdefault(v.family, []).append(v)
    assert set(fams) == {"peaked", "ramp", "poison"}  # no family, hence no case, is left out
    for fam, fv in fams.items():
        targeted = set(t for v in fv for t in v.targets)
        if fam == "peaked":  # every mutation whose key exists has a placement
            assert targeted == exists, (sorted(exists - targeted), sorted(targeted - exists))
        else:
            assert targeted and targeted <= exists
        for name in sorted(targeted):
            best = max(_moved(v, st, name, kinds) for v in fv if name in v.targets)
            assert best >= 10.0, (fam, name, best)


@pytest.mark.parametrize("lut", [0, 1])
@pytest.mark.parametrize("S,n_past", A.ROWS_SHAPES)
def test_rows_cases_are_sharp(S, n_past, lut):
    _check_sharp(A.rows_variants(S, n_past, lut), A.ROWS_STRUCT, ["attention"] if lut else ["rows", "attention"], lut)


@pytest.mark.parametrize("lut", [0, 1])
@pytest.mark.parametrize("nk", A.DECODE_COUNTS)
def test_decode_cases_are_sharp(nk, lut):
    _check_sharp(A.decode_variants(nk, lut), A.DECODE_STRUCT, ["decode"] if lut else ["dfast", "decode"], lut)
