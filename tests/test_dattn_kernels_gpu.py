"""The diffusion AttentionBlock core (diff_attn_kernel<2,2>, diff_attn_kernel<2,1> and diff_attn_f32_kernel of csrc/diffusion.hip), launched one at a time
through the test-only harness (libtts_dattn_test.so) with the product's launch parameters and compared element by element with the float64 reference of
tests/dattn_cases.py under that module's derived bounds. Stated as tests besides: nothing outside a sequence's rows is written (the sentinel is still there bit
for bit, halo rows and out_lo included, and the canaries are intact); 64-query workgroups give the bits of 128-query ones; a sequence gives the same bits alone
and beside others; +-60000 on every row outside the sequences changes no bit; two runs give the same bits. tests/test_dattn_harness_cpu.py shows that the bounds
pass a NumPy restatement of the kernels' arithmetic and are sharp.
With TTS_DATTN_REPORT=<file> the largest error over bound per kernel, input family and bias table, and the share of fp16 outputs that differ from the rounded
reference, are written there (profiles/diff_attn_direct.txt)."""
import faulthandler
import os

import numpy as np
import pytest

import dattn_cases as D
from dattn_cases import F16_Q128, F16_Q64, F32, CH, NH

pytestmark = pytest.mark.gpu

RATIOS = {}  # (kernel, family, table) -> [largest error / bound, fp16 outputs that differ from rn16(reference), fp16 outputs, cases]
SENT16 = D.SENTINEL * 0x0101
LDS = {F16_Q128: 2 * 16384 + 320 * 4, F16_Q64: 2 * 16384 + 320 * 4, F32: 2 * 32768 + 128 * 4}


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a launch that never returns ends the process instead of holding the GPU"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TTS_DATTN_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("%-24s %-10s %-7s %6s %12s %s\n" % ("kernel", "family", "table", "cases", "|err|/bound", "fp16 outputs != rn16(reference)"))
            for (k, fam, tab), (r, diff, n, cases) in sorted(RATIOS.items()):
                f.write("%-24s %-10s %-7s %6d %12.4f %s\n" % (k, fam, tab, cases, r, "%.4f %%" % (100.0 * diff / n) if n else "-"))
            for k in D.KIND_NAMES:
                rs = [v for (kk, _, _), v in RATIOS.items() if kk == k]
                if rs:
                    f.write("%s: %d cases, largest |err|/bound %.4f\n" % (k, sum(v[3] for v in rs), max(v[0] for v in rs)))


def launch(c, kind, poison=False):
    """one launch; a failed HIP call (a fault included) ends the session: nothing more is started on a GPU that may have faulted"""
    try:
        out = D.run(c, kind, poison)
    except D.HipError as e:
        pytest.exit(str(e), returncode=3)
    assert out.canaries_intact(), (c.name(), D.KIND_NAMES[kind])
    qw = 64 if kind == F16_Q64 else 128
    nq = (max(c.lens) + qw - 1) // qw
    assert out.launch.tolist() == [nq * 16 * c.lay.ns, 256, LDS[kind], nq]  # attention_block()'s grid, block, dynamic LDS and nq
    return out


def untouched(c, out, kind):
    """-> the number of 16-bit words outside the sequences' rows that no longer hold the sentinel: the halo row in front (row -1), the rows behind the layout, every
    guard and padding row, in out and (split kernel) out_lo"""
    bad = 0
    m = c.lay.row_mask()
    for g in (out.hi, out.lo) if kind == F32 else (out.hi,):
        p = g.payload
        bad += int((p[0] != SENT16).sum() + (p[-1] != SENT16).sum() + (p[1:-1][~m] != SENT16).sum())
    return bad


def check(c, out, kind, record=True):
    """every element of every sequence inside its bound, nothing else written -> the number of offending elements (0 to pass)"""
    bad = untouched(c, out, kind)
    worst = 0.0
    for s, (r, ref, o) in enumerate(D.ratios(c, out.value(kind == F32), kind)):
        bad += int((~(r <= 1.0)).sum())
        worst = max(worst, float(r.max()))
        if record:
            e = RATIOS.setdefault((D.KIND_NAMES[kind], c.family, c.table), [0.0, 0, 0, 0])
            e[0], e[3] = max(e[0], float(r.max())), e[3] + (1 if s == 0 else 0)
            if kind != F32:
                e[1], e[2] = e[1] + int((o != D.rn16(ref)).sum()), e[2] + o.size
        if not (r <= 1.0).all():
            i = np.unravel_index(np.argmax(np.where(np.isnan(r), np.inf, r)), r.shape)
            print("   first offender: sequence %d head %d query %d channel %d out %r reference %r ratio %r" % (s, i[0], i[1], i[2], o[i], ref[i], r[i]))
    print("%-24s %-32s offending %d, worst |err|/bound %.3f" % (D.KIND_NAMES[kind], c.name(), bad, worst))
    return bad


def configs(T):
    return [("flat", "sharp")] if T == 577 else D.CONFIGS  # one case of 577


MATRIX = [(T, fam) for T in D.LENGTHS for fam in D.FAMILIES if T != 577 or fam == "flat"]


@pytest.mark.parametrize("T,family", MATRIX, ids=["T%d-%s" % m for m in MATRIX])
def test_every_element_is_inside_its_bound(T, family):
    bad = 0
    for cfg in configs(T):
        if cfg[0] != family:
            continue
        c = D.single(T, cfg)
        for kind in D.KINDS:
            bad += check(c, launch(c, kind), kind)
    assert bad == 0


def test_split_output_halves_agree_on_an_f32_tie():
    """Regression. flat / smooth, T = 15, head 4, query 9, channel 18: o / l is, as an f32 number, the tie 1987.5 / 2048 between two fp16 values (the exact value
    lies 1.4e-8 below it). diff_attn_f32_kernel used to store out_hi = 1988 / 2048 with out_lo = + 2^-12: the compiler had fused the product o * inv into one of
    the two fp16 conversions, so the halves rounded different numbers and out_hi + out_lo was one fp16 unit (4.9e-4, 2.7 bounds) off. The halves must describe
    one f32 value: their sum is inside the element's bound, here and on every element of the case."""
    c = D.single(15, ("flat", "smooth"))
    sq = c.seqs[0]
    ref = D.reference(sq, c.bias, True)["out"][4, 9, 18]
    assert abs(ref - 1987.5 / 2048) < 2.0 ** -25  # the case still lands on the tie
    out = launch(c, F32)
    r, _, o = D.ratios(c, out.value(True), F32)[0]
    print("out_hi + out_lo %r reference %r: %.4f bounds" % (o[4, 9, 18], ref, r[4, 9, 18]))
    assert abs(o[4, 9, 18] - ref) < 2.0 ** -20 and r[4, 9, 18] <= 1.0
    assert check(c, out, F32, record=False) == 0


SOME = [("flat", "sharp"), ("peaked", "sharp"), ("ramp-up", "smooth"), ("wide", "sharp")]


@pytest.mark.parametrize("lens", D.TRIPLES, ids=["-".join(map(str, t)) for t in D.TRIPLES])
def test_three_sequence_layouts(lens):
    """(T, 1, T'): nq is set by the longest sequence, the upper workgroups of the short ones leave at q0 >= T; each sequence's bits are those it gives alone"""
    bad = 0
    for cfg in SOME:
        c = D.triple(lens, cfg)
        raw = {}
        for kind in D.KINDS:
            out = launch(c, kind)
            raw[kind] = out.hi.raw
            bad += check(c, out, kind)
            for s in range(3):
                one = D.alone(c, s)
                o1 = launch(one, kind)
                for which in ("hi", "lo") if kind == F32 else ("hi",):
                    assert (o1.rows(which)[one.lay.seq_rows(0)] == out.rows(which)[c.lay.seq_rows(s)]).all(), (c.name(), D.KIND_NAMES[kind], s, which)
        assert (raw[F16_Q64] == raw[F16_Q128]).all(), c.name()  # 64-query workgroups: the same bits here too
    assert bad == 0


def test_eight_sequences():
    bad = 0
    for cfg in (("flat", "sharp"), ("wide", "smooth")):
        c = D.Case(D.EIGHT, cfg[0], cfg[1])
        for kind in D.KINDS:
            out = launch(c, kind)
            bad += check(c, out, kind)
            for s in (0, 3, 7):
                one = D.alone(c, s)
                assert (launch(one, kind).rows()[one.lay.seq_rows(0)] == out.rows()[c.lay.seq_rows(s)]).all(), (c.name(), D.KIND_NAMES[kind], s)
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------- bit identities

@pytest.mark.parametrize("T", D.LENGTHS)
def test_q64_gives_the_bits_of_q128_and_runs_repeat(T):
    for cfg in configs(T):
        c = D.single(T, cfg)
        a, b, again = launch(c, F16_Q128), launch(c, F16_Q64), launch(c, F16_Q128)
        assert (a.hi.raw == b.hi.raw).all(), c.name()      # the code claims it: the same arithmetic in the same key order
        assert (a.hi.raw == again.hi.raw).all(), c.name()  # run to run
    c = D.single(T, configs(T)[0])
    a, again = launch(c, F32), launch(c, F32)
    assert (a.hi.raw == again.hi.raw).all() and (a.lo.raw == again.lo.raw).all()


@pytest.mark.parametrize("T", D.LENGTHS)
def test_poison_outside_the_sequence_changes_no_bit(T):
    """+-60000 on the guard row, the rows in front and the 128 slack rows, in Q, K and V^T (and their low halves): the output buffer is the unpoisoned run's, whole"""
    for cfg in configs(T):
        c = D.single(T, cfg)
        for kind in D.KINDS:
            clean, dirty = launch(c, kind), launch(c, kind, poison=True)
            assert untouched(c, dirty, kind) == 0, (c.name(), D.KIND_NAMES[kind])
            assert (clean.hi.raw == dirty.hi.raw).all(), (c.name(), D.KIND_NAMES[kind])
            if kind == F32:
                assert (clean.lo.raw == dirty.lo.raw).all(), c.name()


@pytest.mark.parametrize("lens", D.TRIPLES[:2], ids=["-".join(map(str, t)) for t in D.TRIPLES[:2]])
def test_poison_between_sequences_changes_no_bit(lens):
    for cfg in SOME:
        c = D.triple(lens, cfg)
        for kind in D.KINDS:
            clean, dirty = launch(c, kind), launch(c, kind, poison=True)
            assert (clean.hi.raw == dirty.hi.raw).all() and (kind != F32 or (clean.lo.raw == dirty.lo.raw).all()), (c.name(), D.KIND_NAMES[kind])
