"""CPU: locally typical sampling (option "ar_typical_mass", tts_ar_request.typical_mass, probes tts_host_typical_keep / tts_host_sample_row_typical /
tts_host_sample_prefiltered_typical, CLI flag --typical-mass). No device: tts_create(-1), the host probes and `tortoise --dry-run 1`.

The literal definition (host_logic.cpp: typical_keep) is held to HF's TypicalLogitsWarper evaluated in float64 and to `np_typical` below, a NumPy restatement of
the same definition; the engine's full-row path and the list path (the host building the list under the device's decision rule) are held to the literal.
tests/test_typical_gpu.py imports the helpers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_ar_session_controls_cpu import crafted_bias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 8194
f32 = np.float32
OK, ERR_ARG = 0, -1
DEFAULTS = dict(temperature=0.8, top_k=50, top_p=0.8, penalty=2.0)
MASSES = [0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.9, 0.98]
SYMBOLS = ["tts_host_typical_keep", "tts_host_sample_row_typical", "tts_host_sample_prefiltered_typical"]


def penalise(row, ids, penalty):
    out = np.asarray(row, f32).copy()
    ids = np.unique(np.asarray(ids, np.int64))
    g = out[ids]
    out[ids] = np.where(g < 0, g * f32(penalty), g / f32(penalty)).astype(f32)
    return out


def np_typical(x, mass, defect=None):
    """The definition in float64: the kept set of the (penalised) row x. defect: one seeded mistake (test_the_row_set_is_sharp)."""
    x = np.asarray(x, f32).astype(np.float64)
    m = x.max()
    Z = np.exp(x - m).sum()
    lnp = (x - m) - np.log(Z)
    p = np.exp(lnp)
    H = -(p[p != 0] * lnp[p != 0]).sum()
    if defect == "entropy_sign":
        H = -H
    d = np.abs(-lnp - H)
    key = -d if defect == "descending" else d
    order = np.argsort(key, kind="stable")
    c = np.cumsum(p[order])
    hit = np.nonzero(c > mass if defect == "count_le" else c >= mass)[0]   # (c <= mass).sum() for (c < mass).sum(): the first c > mass
    js = int(hit[0]) if len(hit) else V - 1
    cut = key[order[js]]
    if defect == "crossing_excluded":
        return (key < cut) | (np.arange(V) == order[0])
    return key <= cut


def hf_typical(x, mass):
    """HF's TypicalLogitsWarper on the float64 row: the kept set."""
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    scores = torch.from_numpy(np.asarray(x, f32).astype(np.float64))[None]
    out = tr.TypicalLogitsWarper(mass=float(mass), min_tokens_to_keep=1)(torch.zeros((1, 1), dtype=torch.long), scores)
    return torch.isfinite(out[0]).numpy()


def row_set():
    """The seeded (raw row, penalty ids, mass) cases, 368 of them: the crafted head of tests/test_sampler_controls_gpu.py with and without the -1e30 stop mask
    and with hot ids penalised, Gaussian rows at scales 0.02 .. 4 with and without 40 hot ids; every row at every mass of MASSES."""
    rs = np.random.RandomState(2022)
    bias, hot = crafted_bias()
    masked = bias.copy()
    masked[8193] = -1e30
    rows = [(bias, [1, 8192]), (masked, [1, 8192]), (bias, hot[:20]), (masked, hot[5:45])]
    for seed in range(3):
        for scale in (0.02, 0.1, 0.5, 1.0, 2.0, 3.0, 4.0):
            for with_hot in (False, True):
                row = (rs.randn(V) * scale).astype(f32)
                if with_hot:
                    row[rs.choice(V, 40, replace=False)] += rs.uniform(4, 6, 40).astype(f32)
                if seed == 2:
                    row[8193] = -1e30
                rows.append((row, np.argsort(-row)[:3]))
    return [(row, np.asarray(ids, np.int32), float(f32(mass))) for row, ids in rows for mass in MASSES]


@pytest.fixture(scope="module")
def cases():
    out = row_set()
    assert len(out) >= 300
    return [(row, ids, mass, penalise(row, ids, 2.0)) for row, ids, mass in out]


@pytest.fixture(scope="module")
def literal_sets(pkg, cases):
    return [pkg.host_typical_keep(pen, mass) for _, _, mass, pen in cases]


def test_literal_equals_the_numpy_restatement_on_every_row(cases, literal_sets):
    sizes = []
    for n, ((row, ids, mass, pen), got) in enumerate(zip(cases, literal_sets)):
        want = np_typical(pen, mass)
        assert np.array_equal(got, want), (n, mass, int(got.sum()), int(want.sum()))
        assert got[np.argmin(np.abs(np_distance(pen)))]   # the smallest d is always kept
        sizes.append(int(got.sum()))
    assert min(sizes) < 64 and max(sizes) > 1000, (min(sizes), max(sizes))


def np_distance(x):
    x = np.asarray(x, f32).astype(np.float64)
    lnp = (x - x.max()) - np.log(np.exp(x - x.max()).sum())
    p = np.exp(lnp)
    return np.abs(-lnp + (p[p != 0] * lnp[p != 0]).sum())


def test_literal_equals_hf_typical_logits_warper_in_float64(cases, literal_sets):
    """Every row of the set, none left out: the kept ids are those HF's warper leaves finite."""
    pytest.importorskip("transformers")
    for n, ((row, ids, mass, pen), got) in enumerate(zip(cases, literal_sets)):
        want = hf_typical(pen, mass)
        assert np.array_equal(got, want), (n, mass, int(got.sum()), int(want.sum()))


def test_the_features_figures_on_the_crafted_head(pkg):
    """What the feature does on the crafted head: at mass 0.9 the argmax is dropped, at 0.05 none of the 60 hot ids is kept."""
    bias, hot = crafted_bias()
    k9, k2, k05 = (pkg.host_typical_keep(bias, m) for m in (0.9, 0.2, 0.05))
    assert not k9[np.argmax(bias)] and k9.sum() > 4000
    assert 64 < k2.sum() < k9.sum()
    assert not k05[hot].any() and 16 <= k05.sum() <= 128


def test_the_row_set_is_sharp(cases):
    """Each restatement with one seeded defect gives another set than the definition somewhere on the row set. `<=` for `<` in the count differs from the
    definition only where a cumulative sum EQUALS the mass: for that defect the set is extended by the same rows at masses that are cumulative sums of the
    restatement itself (float64 masses, compared between restatements only)."""
    for defect in ("entropy_sign", "descending", "crossing_excluded"):
        n = sum(not np.array_equal(np_typical(pen, mass), np_typical(pen, mass, defect)) for _, _, mass, pen in cases[::3])
        assert n > 0, defect
    n = 0
    for _, _, _, pen in cases[::40]:
        x = pen.astype(np.float64)
        lnp = (x - x.max()) - np.log(np.exp(x - x.max()).sum())
        c = np.cumsum(np.exp(lnp)[np.argsort(np_distance(pen), kind="stable")])
        for j in (3, 40, 400):
            n += not np.array_equal(np_typical(pen, c[j]), np_typical(pen, c[j], "count_le"))
    assert n > 0, "count_le"
    # the stage's place in the order: after the penalty, before the temperature
    after_temp = sum(not np.array_equal(np_typical(pen, mass), np_typical((pen / f32(0.8)).astype(f32), mass)) for _, _, mass, pen in cases[::3])
    before_pen = sum(not np.array_equal(np_typical(pen, mass), np_typical(row, mass)) for row, _, mass, pen in cases[::3])
    assert after_temp > 0 and before_pen > 0


def _param_sets():
    from test_sampler_controls_gpu import PARAM_SETS
    return PARAM_SETS


def _agree(pkg, row, ids, u, mass, kw, keep):
    lit = pkg.host_sample_row_typical(row, ids, u, typical_mass=mass, mode=1, **kw)
    eng = pkg.host_sample_row_typical(row, ids, u, typical_mass=mass, mode=0, **kw)
    lst = pkg.host_sample_prefiltered_typical(row, ids, u, typical_mass=mass, keep=keep, **kw)
    assert 0 <= lit < V and eng == lit, (lit, eng)
    assert lst in (lit, -1), (lit, lst)
    return lst


def test_paths_agree_over_the_grid(pkg):
    """Mode 0 (the engine's full-row path) returns what mode 1 (the literal) returns, and the list path returns the same id or -1: masses x the controls'
    PARAM_SETS x penalty ids of scope 0 (one id) and scope 1 (a history), on rows whose typical sets have fewer than 64, 64 .. 128 and more than 128 members."""
    rs = np.random.RandomState(404)
    bias, hot = crafted_bias()
    gauss = (rs.randn(V) * 3).astype(f32)
    rows = [bias, gauss, (rs.randn(V) * 1.5).astype(f32)]
    rows[1][8193] = -1e30
    sizes, undecided, total = set(), 0, 0
    for row in rows:
        order = np.argsort(-row)
        for mass in (0.05, 0.2, 0.5, 0.9):
            for ps in _param_sets():
                kw = {k: ps[k] for k in ("temperature", "top_k", "top_p", "penalty")}
                for scope in (0, 1):
                    ids = order[rs.randint(0, 30, 1)] if scope == 0 else np.unique(np.concatenate([[1, 8192], order[rs.randint(0, 200, 40)]]))
                    n = int(pkg.host_typical_keep(penalise(row, ids, kw["penalty"]), mass).sum())
                    sizes.add(0 if n < 64 else 1 if n <= 128 else 2)
                    for u in rs.rand(2):
                        undecided += _agree(pkg, row, ids, float(u), mass, kw, min(kw["top_k"] + 14, 128)) < 0
                        total += 1
    assert sizes == {0, 1, 2}, sizes
    assert undecided * 20 <= total, (undecided, total)   # the list path decides all but a few rows (near ties in d or in the tempered values)


def test_paths_agree_at_adversarial_masses(pkg):
    """For several prefixes j of the crafted row's typical order: the two floats either side of the cumulative mass c_j. The literal set changes between the two;
    every path follows, the list path where it does not return -1."""
    bias, hot = crafted_bias()
    ids = np.array([int(hot[3])], np.int32)
    pen = penalise(bias, ids, 2.0)
    x = pen.astype(np.float64)
    lnp = (x - x.max()) - np.log(np.exp(x - x.max()).sum())
    order = np.argsort(np_distance(pen), kind="stable")
    c = np.cumsum(np.exp(lnp)[order])
    rs = np.random.RandomState(9)
    changed = 0
    for j in (0, 1, 15, 16, 60, 63, 64, 127, 128, 500, 4000):
        lo = f32(c[j])
        if float(lo) > c[j]:
            lo = np.nextafter(lo, f32(0))
        hi = np.nextafter(lo, f32(1))
        sets = [pkg.host_typical_keep(pen, float(m)) for m in (lo, hi)]
        assert np.array_equal(sets[0], np_typical(pen, float(lo))) and np.array_equal(sets[1], np_typical(pen, float(hi)))
        changed += int(sets[0].sum() != sets[1].sum())
        for m in (lo, hi):
            for u in rs.rand(2):
                _agree(pkg, bias, ids, float(u), float(m), DEFAULTS, 64)
    assert changed >= 8


def test_mass_zero_is_the_ex_probes(pkg):
    rs = np.random.RandomState(5)
    for trial in range(40):
        row = (rs.randn(V) * rs.choice([0.5, 1.0, 2.0])).astype(f32)
        ids = np.argsort(-row)[rs.randint(0, 60, 1 + trial % 3)]
        u = float(rs.rand())
        for mode in (0, 1):
            assert pkg.host_sample_row_typical(row, ids, u, typical_mass=0.0, mode=mode, **DEFAULTS) == pkg.host_sample_row_ex(row, ids, u, mode=mode, **DEFAULTS)
        assert pkg.host_sample_prefiltered_typical(row, ids, u, typical_mass=0.0, keep=64, **DEFAULTS) == \
            pkg.host_sample_prefiltered_ex(row, ids, u, keep=64, already_penalised=True, **DEFAULTS)


VALUES = [0, 1e-46, 0.9, 1 - 1e-9, 1, -0.1, float("nan"), float("inf"), 1e-30, 0.05, 0.999, 1.0000001, -0.0]
ACCEPTED = {0, 0.9, 1e-30, 0.05, 0.999, -0.0}


def test_option_descriptor_and_probes_agree_on_every_value(pkg):
    """tts_set_option("ar_typical_mass"), the descriptor's check and the probes accept the same values: 0 (off) and 0 < x < 1 also after narrowing to float (1e-46
    narrows to 0 and 1 - 1e-9 to 1: refused). A refused value changes nothing."""
    eng = pkg.Engine(-1)
    try:
        row = np.zeros(V, f32)
        for v in VALUES:
            accepted = eng.L.tts_set_option(eng.h, b"ar_typical_mass", float(v)) == OK
            assert accepted == (v in ACCEPTED and v == v), v
            assert pkg.host_ar_request_check(4, 8, typical_mass=v) == (OK if accepted else ERR_ARG), v
            assert (pkg.host_sample_row_typical(row, [1], 0.5, typical_mass=v) != -2) == accepted, v
            assert (pkg.host_sample_prefiltered_typical(row, [1], 0.5, typical_mass=v) != -2) == accepted, v
            keep = np.zeros(V, np.uint8)
            assert (pkg.lib().tts_host_typical_keep(row, float(v), keep.ctypes.data_as(C.c_void_p)) != -2) == (accepted and v != 0), v
        # sticky, and a refusal leaves the stored value alone: tts_sample reads it
        bias, hot = crafted_bias()
        logits = np.tile(bias, (3, 1))
        ids = np.tile(np.array([1, 8192], np.int32), (3, 1))
        eng.set_option("ar_typical_mass", 0.9)
        assert eng.L.tts_set_option(eng.h, b"ar_typical_mass", 1.5) == ERR_ARG
        eng.seed(3)
        got = eng.sample(logits, ids)
        eng.seed(3)
        u = [(eng.rng_uniform(), eng.rng_uniform())[1] for _ in range(3)]
        assert [pkg.host_sample_row_typical(bias, [1, 8192], x, typical_mass=0.9, mode=1, **DEFAULTS) for x in u] == list(got)
        eng.set_option("ar_typical_mass", 0)
        eng.seed(3)
        off = eng.sample(logits, ids)
        assert [pkg.host_sample_row_ex(bias, [1, 8192], x, mode=1, **DEFAULTS) for x in u] == list(off)
    finally:
        eng.close()


def test_symbols_are_exported_declared_and_bound(pkg):
    L = pkg.lib()
    declared = set(pkg.header_symbols())
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert getattr(L, name).argtypes is not None, name
    assert pkg.AR_CONTROL_FIELDS["typical_mass"] == "typical_mass"
    assert [f[0] for f in pkg.ArRequest._fields_][-1] == "typical_mass"
    assert L.tts_version() == 8
    hdr = open(pkg.HEADER).read()
    assert "ar_typical_mass" in hdr and "double typical_mass;" in hdr


def test_struct_size_rule(pkg):
    """The first use of the descriptor's growth rule: the size before the field is accepted (its request runs under the session's mass: the field is not read), the
    sizes in between are no header's struct, the present size and anything longer are accepted."""
    R = pkg.ArRequest
    old, new = pkg.AR_REQUEST_SIZE_V0, C.sizeof(R)
    assert (old, new, R.typical_mass.offset) == (64, 72, 64)
    check = pkg.host_ar_request_check
    assert check(4, 8, struct_size=old) == OK
    assert check(4, 8, struct_size=old, typical_mass=7.0) == OK   # not covered by struct_size: not read
    for size in range(old + 1, new):
        assert check(4, 8, struct_size=size) == ERR_ARG, size
    assert check(4, 8, struct_size=old - 1) == ERR_ARG
    assert check(4, 8, struct_size=new) == OK and check(4, 8, struct_size=new + 8) == OK
    assert check(4, 8, struct_size=new, typical_mass=7.0) == ERR_ARG and check(4, 8, struct_size=new + 8, typical_mass=0.3) == OK


def test_grown_descriptor_layout_as_c99_sees_it(pkg, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "req.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include <stdint.h>
#include "tortoise_mi355x.h"
int main(void) {
  tts_ar_request r;
  r.struct_size = (uint32_t)sizeof r; r.n_cand = 1; r.seed = 5u; r.max_steps = 0; r.stop_at = NULL;
  r.temperature = 0.8; r.top_k = 50; r.top_p = 0.8; r.repetition_penalty = 2.0; r.penalty_scope = 0; r.typical_mass = 0.2;
  printf("%d %d %d\n", (int)sizeof r, (int)offsetof(tts_ar_request, penalty_scope), (int)offsetof(tts_ar_request, typical_mass));
  printf("%d ", tts_host_ar_request_check(&r, 4, 8));
  r.typical_mass = 1.0;
  printf("%d ", tts_host_ar_request_check(&r, 4, 8));
  r.struct_size = (uint32_t)offsetof(tts_ar_request, typical_mass);
  printf("%d ", tts_host_ar_request_check(&r, 4, 8));
  r.struct_size += 4u;
  printf("%d\n", tts_host_ar_request_check(&r, 4, 8));
  return 0;
}
''')
    exe = tmp_path / "req"
    inc = os.path.join(os.path.dirname(os.path.dirname(pkg.LIB_PATH)), "include")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-ltortoise_mi355x",
                    "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    R = pkg.ArRequest
    assert [int(x) for x in out[0].split()] == [C.sizeof(R), R.penalty_scope.offset, R.typical_mass.offset]
    assert [int(x) for x in out[1].split()] == [OK, ERR_ARG, OK, ERR_ARG]


def test_cli_flag(tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    models = os.path.join(ROOT, "models")
    base = [exe, "--dry-run", "1", "--models", models, "--voice", os.path.join(models, "mol.bin"), "--seed", "11", "--codes", "5", "--candidates", "2",
            "--output", str(tmp_path / "o.wav"), "--timing", "1"]
    for bad in ("1", "-0.1", "nan", "1.5", "1e-46"):
        r = subprocess.run(base + ["--typical-mass", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--typical-mass" in r.stderr and "[timing]" not in r.stderr, (bad, r.stderr)
    r = subprocess.run(base + ["--typical-mass", "0.2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[timing] ar sampler temperature 0.8, top-k 50, top-p 0.8, repetition-penalty 2, penalty-scope last, typical-mass 0.2\n" in r.stderr, r.stderr
