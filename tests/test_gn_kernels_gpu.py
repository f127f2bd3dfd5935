"""The diffusion stage's GroupNorm kernels (gn_reg_kernel<512,14>, gn_reg_kernel<1024,18>, gn_fused_kernel<0>, gn_stats_kernel + gn_apply_f32_kernel,
gn_apply_kernel) and the three row kernels on the same layout, launched one at a time through the test-only harness (libtts_gn_test.so) and compared element by
element with the float64 reference of tests/gn_cases.py under that module's acceptance rule; every row of the layout is written and guard rows are +0; bit
identities between launches that must not differ. tests/test_gn_harness_cpu.py shows that the rule passes a correct f32 implementation and is sharp.
With TTS_GN_REPORT=<file> the largest error over bound per kernel and input family is written there (profiles/gn_direct.txt)."""
import faulthandler
import os

import numpy as np
import pytest

import gn_cases as G
from gn_cases import APPLY, AUTO, FUSED, GATHER_F16, GATHER_F32, REG512, REG1024, STATS, STATS_APPLY_F32, TO_F16, CH

pytestmark = pytest.mark.gpu

RATIOS = {}   # (kernel, family) -> [largest error / bound, fp16 outputs that differ from rn16(reference), fp16 outputs]
PIVOT = []    # (T, observed relative variance error, the bound's) of gn_stats_kernel with the pivot on the outlier


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a launch that never returns ends the process instead of holding the GPU"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TTS_GN_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("%-40s %-14s %12s %s\n" % ("kernel", "family", "|err|/bound", "fp16 outputs != rn16(reference)"))
            for (k, fam), (r, diff, n) in sorted(RATIOS.items()):
                f.write("%-40s %-14s %12.4f %s\n" % (k, fam, r, "%.4f %%" % (100.0 * diff / n) if n else "-"))
            for T, seen, rho in PIVOT:
                f.write("gn_stats_kernel, pivot on the outlier, T = %d: relative variance error %.3g observed, %.3g allowed by the bound\n" % (T, seen, rho))


def _record(label, fam, r, diff=0, n=0):
    e = RATIOS.setdefault((label, fam), [0.0, 0, 0])
    e[0], e[1], e[2] = max(e[0], r), e[1] + diff, e[2] + n


def _given(c):
    if c.kind != APPLY:
        return None, None
    st, mean, var = G.stripes(c)
    return st, (mean, var)


def check16(c, bits, label=None, given=None, ref=None):
    """An fp16 output [rows][1024] (uint16) of case c: every element accepted, guard rows +0. -> the number of rejected elements (0 to pass)"""
    label = (label or G.KIND_NAMES[c.kind]) + (" lut=1" if c.do_silu and c.lut == 1 else "")  # two fp16 roundings: neighbouring fp16 values are both right
    ref = ref or G.reference(c, given=given)
    lo, hi = G.interval(c, ref)
    ok = G.accept16(bits, lo, hi)
    m = c.lay.row_mask()
    guard_bad = int((bits[~m] != 0).sum())  # bit pattern 0x0000, not -0 and not the sentinel
    o = bits.view(np.float16).astype(np.float64)
    z = ref["z"]
    with np.errstate(invalid="ignore", divide="ignore"):
        tol = np.maximum(np.maximum(hi - z, z - lo), 1e-300)
        r = np.maximum(np.abs(o - z) - 0.5 * G.ulp16(o), 0.0) / tol  # the part of the error the output rounding does not explain
        r = np.where(np.isnan(r), np.inf, r)
    differs = o != G.rn16(z)
    for s in range(c.lay.ns):
        rows = c.lay.seq_rows(s)
        T = rows.stop - rows.start
        rg, dg = r[rows].reshape(T, 32, 32).max(axis=(0, 2)), differs[rows].reshape(T, 32, 32).sum(axis=(0, 2))
        for gi, (fam, _, _) in enumerate(c.plans[s]):
            _record(label, fam + (" poison" if c.poison else ""), float(rg[gi]), int(dg[gi]), T * 32)
    bad = int((~ok).sum())
    # an element the launch never wrote still holds the sentinel (-15.59 as fp16): rejected above unless its reference is that very value, never a whole row of them
    bad += int((bits == G.SENTINEL * 0x0101).all(axis=1).sum())
    print("%-60s rejected %d guard %d worst |err|/bound %.3f" % (c.name() if label.startswith(G.KIND_NAMES[c.kind]) else label + " " + c.name(), bad, guard_bad, float(r[m].max())))
    if bad:
        i = np.argwhere(~ok)[0]
        print("   first rejected: row %d channel %d out %r reference %r interval [%r, %r]" % (i[0], i[1], o[tuple(i)], z[tuple(i)], lo[tuple(i)], hi[tuple(i)]))
    return bad + guard_bad


def run_checked(c, **kw):
    st, given = _given(c)
    out = G.run(c, st=st, **kw)
    return check16(c, out.payload, given=given), out


MATRIX = [(k, T) for k in (REG512, REG1024, FUSED, APPLY) for T in G.LENGTHS[k]]
_ids = lambda m: ["%s-T%d" % (G.KIND_NAMES[k].replace(" ", ""), T) for k, T in m]


@pytest.mark.parametrize("kind,T", MATRIX, ids=_ids(MATRIX))
def test_every_length_and_family_is_accepted(kind, T):
    bad = 0
    for cfg in G.configs(kind, T):
        bad += run_checked(G.single(kind, T, cfg))[0]
    assert bad == 0


@pytest.mark.parametrize("kind", [REG512, REG1024, FUSED, APPLY])
def test_three_sequence_layouts_are_accepted(kind):
    """(T, 1, T'): guard rows before the first, between and behind the last sequence, ns * 32 workgroups, seq_step = (2, 0, 1) with rows 2112 floats apart"""
    bad = 0
    for cfg in G.configs(kind):
        bad += run_checked(G.triple(kind, cfg))[0]
    c = G.Case(kind, G.TRIPLES[kind], G.CONFIGS[1], pad=128)  # the product pads its layouts to 128 rows: a long tail of guard rows
    bad += run_checked(c)[0]
    assert bad == 0


def _check_stats(c, out):
    ref = G.reference(c)
    z, lo, hi = G.stats_interval(c, ref)
    ok = G.accept32(out, lo, hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(out == z, 0.0, np.abs(out - z) / (0.5 * (hi - lo)))
        r = np.where(np.isnan(r), np.inf, r)
    for s in range(c.lay.ns):
        for gi, (fam, _, _) in enumerate(c.plans[s]):
            _record("gn_stats_kernel", fam + (" poison" if c.poison else ""), float(r[s, gi].max()))
    print("%-60s rejected %d worst |err|/bound %.3f" % (c.name(), int((~ok).sum()), float(r.max())))
    return int((~ok).sum()), ref


@pytest.mark.parametrize("T", G.LENGTHS[STATS])
def test_statistics_every_length_and_family(T):
    bad = 0
    for cfg in G.configs(STATS, T):
        c = G.single(STATS, T, cfg)
        bad += _check_stats(c, G.run(c).payload.astype(np.float64))[0]
    c = G.triple(STATS, G.STATS_CONFIGS[1])
    bad += _check_stats(c, G.run(c).payload.astype(np.float64))[0]
    assert bad == 0


@pytest.mark.parametrize("T", [257, 500, 2305])
def test_outlier_pivot_variance_error_is_inside_its_bound(T):
    """The one-pass form's recorded property: with the pivot on the outlier the variance loses digits to E[d^2] - E[d]^2, inside what the bound charges."""
    c = G.single(STATS, T, G.STATS_CONFIGS[0])
    out = G.run(c).payload.astype(np.float64)
    bad, ref = _check_stats(c, out)
    grp = [f for f, _, _ in c.plans[0]].index("outlier-pivot")
    _, _, rho = G.stat_bounds(STATS, c.x.astype(np.float64)[c.lay.seq_rows(0)], ref["mean"][0], ref["var"][0], float(np.float32(c.eps)), T)
    seen = abs((1.0 / out[0, grp, 1] ** 2 - float(np.float32(c.eps))) / ref["var"][0, grp] - 1.0)
    PIVOT.append((T, seen, float(rho[grp])))
    print("T = %d: relative variance error %.3g observed, %.3g allowed" % (T, seen, rho[grp]))
    assert bad == 0 and seen <= rho[grp] < 1.0


def _check_f32(c, out, label):
    ref = G.reference(c)
    lo, hi = G.interval(c, ref)
    ok = G.accept32(out, lo, hi)
    m = c.lay.row_mask()
    guard_bad = int((np.ascontiguousarray(out[~m]).view(np.uint32) != 0).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(out == ref["z"], 0.0, np.abs(out.astype(np.float64) - ref["z"]) / np.maximum(np.maximum(hi - ref["z"], ref["z"] - lo), 1e-300))
        r = np.where(np.isnan(r), np.inf, r)
    for s in range(c.lay.ns):
        rows = c.lay.seq_rows(s)
        rg = r[rows].reshape(-1, 32, 32).max(axis=(0, 2))
        for gi, (fam, _, _) in enumerate(c.plans[s]):
            _record(label, fam + (" poison" if c.poison else ""), float(rg[gi]))
    print("%-60s rejected %d guard %d worst |err|/bound %.3f" % (c.name(), int((~ok).sum()), guard_bad, float(r[m].max())))
    return int((~ok).sum()) + guard_bad


@pytest.mark.parametrize("T", G.LENGTHS[STATS])
def test_code_norm_f32_every_length_and_family(T):
    """gn_stats_kernel then gn_apply_f32_kernel on one stream, the voice table's only row for every sequence (seq_voice == nullptr)"""
    bad = 0
    for cfg in G.configs(STATS_APPLY_F32, T):
        c = G.single(STATS_APPLY_F32, T, cfg)
        bad += _check_f32(c, G.run(c).payload, G.KIND_NAMES[STATS_APPLY_F32])
    assert bad == 0


def test_code_norm_f32_reads_each_sequences_own_voice_row():
    bad = 0
    for cfg in G.F32_CONFIGS:
        c = G.triple(STATS_APPLY_F32, cfg)  # seq_voice = (2, 0, 1) into a table of three voices
        out = G.run(c).payload
        bad += _check_f32(c, out, G.KIND_NAMES[STATS_APPLY_F32] + " seq_voice")
        for s, row in enumerate((2, 0, 1)):  # the same bits as the launch without seq_voice given that voice alone
            one = G.run(c, ss=np.ascontiguousarray(c.ss[row * 2 * CH:(row + 1) * 2 * CH]), seq_rows=None).payload
            assert (one[c.lay.seq_rows(s)].view(np.uint32) == out[c.lay.seq_rows(s)].view(np.uint32)).all(), s
    assert bad == 0


@pytest.mark.parametrize("T,cls", G.AUTO_LENGTHS)
def test_dispatch_picks_the_class_of_the_longest_sequence(T, cls):
    """AUTO launches what Layout::gn_class names, as gn_fused() does; gn_fused()'s own if chain draws the same lines (896, 2304)."""
    c = G.Case(cls, [5, T, 1], G.CONFIGS[1])
    picked = []
    auto = G.run(c, kind=AUTO, picked=picked).payload
    assert picked == [cls] and G.harness().tts_gn_test_class(T) == cls
    assert check16(c, auto, label="gn_fused() dispatch") == 0
    assert (auto == G.run(c).payload).all()  # the bits of the class named explicitly


# ---------------------------------------------------------------------------------------------------------------- bit identities

def _alone(c, s, first=8):
    """sequence s of case c alone in a layout of its own (first: its start row) -> (case-like launch arguments, rows)"""
    lay = G.Lay([int(c.lay.len[s])], first=first)
    x = np.zeros((lay.rows, CH), np.float32)
    if c.poison:
        x[:] = np.nan
    x[lay.seq_rows(0)] = c.x[c.lay.seq_rows(s)]
    return lay, x


@pytest.mark.parametrize("kind", [REG512, REG1024, FUSED, APPLY, STATS])
def test_a_sequences_bits_do_not_depend_on_its_neighbours_index_or_start(kind):
    for cfg in (G.configs(kind)[0], G.configs(kind)[-1]):
        c = G.triple(kind, cfg)
        st, given = _given(c)
        whole = G.run(c, st=st).payload
        again = G.run(c, st=st).payload
        assert (whole == again).all()  # repeat launches are identical
        for s in range(3):
            for first in (8, 24):
                lay, x = _alone(c, s, first)
                sr = None if c.seq_rows is None else c.seq_rows[s:s + 1]
                one = G.run(c, lay=lay, x=x, st=None if st is None else np.ascontiguousarray(st[:, s:s + 1]), seq_rows=sr).payload
                if kind == STATS:
                    assert (one[0].view(np.uint32) == whole[s].view(np.uint32)).all(), (s, first)
                else:
                    assert (one[lay.seq_rows(0)] == whole[c.lay.seq_rows(s)]).all(), (s, first)
                    assert (one[~lay.row_mask()] == 0).all()


@pytest.mark.parametrize("kind", [REG512, REG1024, APPLY])
def test_the_weight_touch_changes_nothing(kind):
    c = G.triple(kind, G.CONFIGS[1])
    st, given = _given(c)
    base = G.run(c, st=st).payload
    assert check16(c, base, given=given) == 0
    w0, w1 = np.full(16384 * 128, 0x5A, np.uint8), np.full(1000 * 128, 0xA5, np.uint8)
    for l0, l1 in ((0, 0), (1, 0), (0, 1), (1000, 1000), (16384, 1), (16384, 1000)):
        out = G.run(c, st=st, touch=(w0, l0, w1, l1)).payload
        assert (out == base).all(), (l0, l1)


@pytest.mark.parametrize("kind", [REG512, REG1024, FUSED, APPLY])
def test_seq_step_equals_the_plain_launch_with_that_row(kind):
    c = G.triple(kind, G.CONFIGS[1])  # seq_step = (2, 0, 1), rows 2112 floats apart
    st, given = _given(c)
    whole = G.run(c, st=st).payload
    for s, row in enumerate((2, 0, 1)):
        plain = G.run(c, st=st, ss=np.ascontiguousarray(c.ss[row * c.stride:row * c.stride + 2 * CH]), seq_rows=None).payload
        assert (plain[c.lay.seq_rows(s)] == whole[c.lay.seq_rows(s)]).all(), s


@pytest.mark.parametrize("kind", [REG512, REG1024, FUSED])
def test_a_partition_part_gives_the_bits_of_the_whole_layout(kind):
    """Layout::gn_parts: consecutive sequences launched as a layout of their own on rows [row0, row0 + rows) of the same buffers, starts relative to row0"""
    c = G.triple(kind, G.CONFIGS[1])
    whole = G.run(c).payload
    lay = c.lay
    for s0, s1 in ((0, 1), (1, 3), (0, 2), (2, 3)):
        row0 = 0 if s0 == 0 else int(lay.start[s0])
        rows = (int(lay.start[s1]) if s1 < lay.ns else lay.rows) - row0
        part = G.Lay([1])
        part.ns, part.len, part.start, part.rows = s1 - s0, np.ascontiguousarray(lay.len[s0:s1]), np.ascontiguousarray(lay.start[s0:s1] - row0), rows
        out = G.run(c, lay=part, row0=row0, x_rows=lay.rows, seq_rows=c.seq_rows[s0:s1]).payload
        assert (out[row0:row0 + rows] == whole[row0:row0 + rows]).all(), (s0, s1)
        rest = np.ones(lay.rows, bool)
        rest[row0:row0 + rows] = False
        assert (out[rest] == G.SENTINEL * 0x0101).all(), (s0, s1)  # nothing outside the part's rows is written


# ---------------------------------------------------------------------------------------------------------------- the row kernels

def _special_rows(rows):
    rng = np.random.RandomState(7)
    x = rng.randn(rows, CH).astype(np.float32)
    x[:, 0:8] = np.array([2049.0, 2051.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -2049.0, 65520.0, 65519.996, -65520.0], np.float32)  # ties to even; 65520 -> inf
    x[:, 8:16] = np.array([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3e-8, -2.0 ** -25, 6.1e-5, -6.0e-5, 1e-10], np.float32)  # fp16 subnormals and what rounds to 0
    x[:, 16:20] = np.array([-0.0, 0.0, np.inf, -np.inf], np.float32)
    return x


def test_to_f16_is_round_to_nearest_even_with_guard_rows_zeroed():
    lay = G.Lay([5, 1, 9])
    x = _special_rows(lay.rows)
    x[~lay.row_mask()] = np.nan  # a guard row is never read
    c = G.Case(REG512, [5, 1, 9], G.CONFIGS[0])
    out = G.run(c, kind=TO_F16, x=x).payload
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16).copy()
    want[~lay.row_mask()] = 0
    assert (out == want).all()
    assert out[8, 5] == 0x7C00 and out[8, 16] == 0x8000 and out[8, 0] == np.float16(2048).view(np.uint16) and out[8, 1] == np.float16(2052).view(np.uint16)


@pytest.mark.parametrize("kind", [GATHER_F16, GATHER_F32])
def test_gathers_copy_the_rows_they_are_given(kind):
    x = _special_rows(24)
    src = np.array([-1, 0, 23, 5, 5, -1, 7, 22] * 4, np.int32)
    out = G.Guarded((32, CH), np.uint16 if kind == GATHER_F16 else np.float32)
    cs = G.struct(kind, out=out, rows_total=32, x_rows=24, x=x, src_row=src)
    assert G.harness().tts_gn_test_run(G.C.byref(cs)) == 0 and out.canaries_intact()
    with np.errstate(over="ignore"):
        conv = x.astype(np.float16).view(np.uint16) if kind == GATHER_F16 else x.view(np.uint32)
    want = np.where((src >= 0)[:, None], conv[np.maximum(src, 0)], 0)
    got = out.payload if kind == GATHER_F16 else out.payload.view(np.uint32)
    assert (got == want).all()
