"""The UnivNet vocoder's kernels (conv_direct_kernel, convt_kernel, lvc_gate_kernel, lvc_mfma_kernel, voc_dconv_mfma_kernel, conv_post_kernel, the three row
kernels and voc_philox_kernel of csrc/vocoder.hip), launched one at a time through the test-only harness (libtts_voc_test.so) and compared element by element with
the float64 references of tests/voc_cases.py under that module's derived bounds. Stated as tests besides: every producer writes +0 on every guard position and
every live position; the LVC kernels leave the guard positions of x alone; kernels that check bounds themselves give the same bits with NaN on the guard frames of
their input; the two implementations of the LVC and of the dilated conv agree within their bounds; a candidate gives the same bits alone and in a batch; two runs
give the same bits. tests/test_voc_harness_cpu.py shows that the rule passes a correct f32 implementation and is sharp.
With TTS_VOC_REPORT=<file> the largest error over bound per kernel and input family, and the distances between the twin kernels, are written there
(profiles/voc_direct.txt)."""
import faulthandler
import os

import numpy as np
import pytest

import voc_cases as V
from voc_cases import COND_F16, CONV, CONVT, DCONV, LVC_GATE, LVC_MFMA, MEL_ROWS, NOISE_ROWS, POST

pytestmark = pytest.mark.gpu

RATIOS = {}  # (kernel, family) -> largest error / bound
GATE = []    # (what, largest |gate_dev - g|, largest |gate_dev - g| / |g| over 0 < |b| <= 1e-2, |a| <= 20)
TWINS = []   # (what, largest |a - b|, largest |a - b| / (bound a + bound b))
KINDS = [CONV, CONVT, LVC_GATE, LVC_MFMA, DCONV, POST, MEL_ROWS, NOISE_ROWS, COND_F16]
CHECKS_BOUNDS = (CONV, CONVT, LVC_GATE, POST)  # the two MFMA kernels get zero guards: that is their documented contract


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a launch that never returns ends the process instead of holding the GPU"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TTS_VOC_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("%-24s %-18s %12s\n" % ("kernel", "family", "|err|/bound"))
            for (k, fam), r in sorted(RATIOS.items()):
                f.write("%-24s %-18s %12.4f\n" % (k, fam, r))
            for what, e, rel in GATE:
                f.write("%s: largest |gate_dev - sigmoid(a) tanh(b)| %.3g = %.2f x 2^-24; over 0 < |b| <= 1e-2, |a| <= 20 the largest error relative to the value %.3g\n"
                        % (what, e, e / V.U, rel))
            for what, d, r in TWINS:
                f.write("%s: largest distance %.3g, %.4f of the sum of the two bounds\n" % (what, d, r))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _or_end(f, *a):
    """a failed HIP call (a fault included) ends the session: nothing more is started on a GPU that may have faulted"""
    try:
        return f(*a)
    except V.HipError as e:
        pytest.exit(str(e), returncode=3)


def launch(c):
    out = _or_end(V.run, c)
    assert out.canaries_intact(), c.name()
    return out.payload


def philox(n, seed, stream):
    out = _or_end(V.run_philox, n, seed, stream)
    assert out.canaries_intact()
    return out.payload


def checked(c, ref=None):
    """launch c; every element within its bound, guards as the contract says -> (payload, reference)"""
    ref = ref or V.reference(c)
    o = launch(c)
    bad, r = V.judge(o, ref)
    fam = c.family
    RATIOS[(V.KIND_NAMES[c.kind], fam)] = max(RATIOS.get((V.KIND_NAMES[c.kind], fam), 0.0), r)
    print("%-90s rejected %d worst |err|/bound %.4f" % (c.name(), bad, r))
    if bad:
        with np.errstate(invalid="ignore"):
            i = tuple(np.argwhere(~(np.abs(o.astype(np.float64) - ref["z"]) <= ref["bound"]))[0])
        print("   first rejected: %r out %r reference %r bound %r" % (i, o[i], ref["z"][i], ref["bound"][i]))
    assert bad == 0, (c.name(), bad, r)
    assert V.guards_ok(c, o, ref), c.name()
    return o, ref


ALL = [(k, i) for k in KINDS for i in range(len(V.matrix(k)))]


def _id(ki):
    l, f, p = V.matrix(ki[0])[ki[1]]
    return "-".join([V.KIND_NAMES[ki[0]].replace("_kernel", ""), l, f] + ["%s%s" % kv for kv in sorted(p.items())])


@pytest.mark.parametrize("ki", ALL, ids=[_id(ki) for ki in ALL])
def test_every_case_is_accepted(ki):
    l, f, p = V.matrix(ki[0])[ki[1]]
    c = V.make(ki[0], l, f, **p)
    o, ref = checked(c)
    assert np.array_equal(_bits(launch(c)), _bits(o)), "two runs differ"
    if c.kind in CHECKS_BOUNDS:  # NaN on every guard frame of the input: nothing may change
        assert np.array_equal(_bits(launch(V.poisoned(c))), _bits(o)), "the launch read a guard frame"


def test_conv_post_last_valid_sample():
    """the last sample of every sequence, len * 256 - 7, reads the last 7 positions of the sequence and nothing behind them"""
    c = V.make(POST, "C", "ramp", seed=2)
    c.a["x"][~c.lay.live(256)] = np.nan
    o, ref = checked(c)
    ends = np.cumsum([l * 256 - 6 for l in c.lay.len]) - 1
    assert np.isfinite(o[ends]).all() and (np.abs(o[ends] - ref["z"][ends]) <= ref["bound"][ends]).all()


@pytest.mark.parametrize("kind,hop", [(LVC_GATE, 8), (LVC_GATE, 64), (LVC_MFMA, 64), (LVC_MFMA, 256)])
def test_gate_dev_alone(kind, hop):
    """predicted kernel 0 and x = 0: the output IS gate_dev(a, b) over the grid. Held to the derived bound; what it reaches is recorded: absolute near tanh(0)"""
    c = V.make(kind, "B", "gate0", seed=31, hop=hop, layer=1)
    o, ref = checked(c)
    live = ref["live"]
    z, kb = ref["z"][live], np.repeat(c.a["kbl"].astype(np.float64), hop, axis=0)[live]
    err = np.abs(o[live].astype(np.float64) - z)
    small = (np.abs(kb[:, 32:]) <= 1e-2) & (np.abs(kb[:, :32]) <= 20) & (z != 0)  # |a| <= 20: the sigmoid is a normal f32 number
    GATE.append(("gate_dev in %s hop %d" % (V.KIND_NAMES[kind], hop), float(err.max()), float((err[small] / np.abs(z[small])).max())))
    assert set(np.unique(np.abs(c.a["kbl"][c.lay.live()]))) == set(np.abs(V.GATE_GRID))  # the whole grid is in the launch


@pytest.mark.parametrize("hop", [64, 256])
@pytest.mark.parametrize("family", ["gauss", "gate", "outlier"])
def test_lvc_gate_and_lvc_mfma_agree(hop, family):
    c = V.make(LVC_MFMA, "B", family, seed=11, hop=hop, layer=hop // 128)
    a, ref = checked(c)
    b, _ = checked(V.twin(c), ref)
    d = np.abs(a.astype(np.float64) - b)
    TWINS.append(("lvc_gate_kernel vs lvc_mfma_kernel hop %d %s" % (hop, family), float(d.max()), float((d / np.maximum(2 * ref["bound"], 1e-300)).max())))
    assert (d <= 2 * ref["bound"]).all()


@pytest.mark.parametrize("hop", [64, 256])
@pytest.mark.parametrize("dil", [1, 27])
def test_conv_direct_and_voc_dconv_mfma_agree(hop, dil):
    c = V.make(DCONV, "B", "straddle" if dil == 1 else "gauss", seed=12, hop=hop, dil=dil)
    a, ref = checked(c)
    t = V.twin(c)
    rt = V.reference(t)
    assert np.array_equal(rt["z"], ref["z"])  # one operation, one reference; conv_direct's bound counts one more rounding (c = 3 without a residual to add)
    b, _ = checked(t, rt)
    d = np.abs(a.astype(np.float64) - b)
    TWINS.append(("conv_direct_kernel vs voc_dconv_mfma_kernel hop %d dil %d" % (hop, dil), float(d.max()),
                  float((d / np.maximum(ref["bound"] + rt["bound"], 1e-300)).max())))
    assert (d <= ref["bound"] + rt["bound"]).all()


def _seq_out(c, o, s):
    if c.kind == POST:
        off = int(sum(l * 256 - 6 for l in c.lay.len[:s]))
        return o[off:off + c.lay.len[s] * 256 - 6]
    return o[c.lay.seq(s, o.shape[0] // c.lay.rows)]


ALONE = [(CONV, dict(Cin=64, Cout=32, K=7, reflect=1)), (CONV, dict(Cin=64, Cout=64, K=3, post=1, resid=1)), (CONV, dict(Cin=32, Cout=32, K=3, pre=1, post=1, hop=8, dil=27)),
         (CONVT, dict(hop=1, s=8)), (CONVT, dict(hop=8, s=8)), (CONVT, dict(hop=64, s=4)), (LVC_GATE, dict(hop=8, layer=1)), (LVC_GATE, dict(hop=64, layer=2)),
         (LVC_MFMA, dict(hop=64, layer=0)), (LVC_MFMA, dict(hop=256, layer=3)), (DCONV, dict(hop=64, dil=27)), (DCONV, dict(hop=256, dil=9)), (POST, {}),
         (MEL_ROWS, {}), (NOISE_ROWS, {}), (COND_F16, {})]


@pytest.mark.parametrize("kind,p", ALONE, ids=["-".join([V.KIND_NAMES[k].replace("_kernel", "")] + ["%s%s" % kv for kv in sorted(p.items())]) for k, p in ALONE])
def test_a_candidate_of_layout_c_equals_the_same_candidate_alone(kind, p):
    c = V.make(kind, "C", "gauss", seed=21, **p)
    o, _ = checked(c)
    for s in range(c.lay.ns):
        one = V.alone(c, s)
        o1, _ = checked(one)
        assert np.array_equal(_bits(_seq_out(one, o1, 0)), _bits(_seq_out(c, o, s))), (c.name(), s)


SEEDS = [(0x1234, 0), (0x1234, 3), (0x9e3779b97f4a7c15, 0), (0x9e3779b97f4a7c15, 3)]  # the second seed has a non-zero high word


@pytest.mark.parametrize("seed,stream", SEEDS)
def test_philox_kernel_against_the_restatement(seed, stream):
    n = 4096
    o = philox(n, seed, stream)
    x, bound = V.philox_reference(n, seed, stream)
    err = np.abs(o.astype(np.float64) - x)
    r = float((err / bound).max())
    RATIOS[("voc_philox_kernel", "seed %#x" % seed)] = max(RATIOS.get(("voc_philox_kernel", "seed %#x" % seed), 0.0), r)
    print("voc_philox_kernel seed %#x stream %d: worst |err|/bound %.4f" % (seed, stream, r))
    assert (err <= bound).all()
    assert np.array_equal(_bits(philox(n, seed, stream)), _bits(o))
    assert np.array_equal(_bits(philox(n - 1, seed, stream)), _bits(o[:n - 1]))  # n that is no multiple of the block: nothing is written behind the last element


def test_philox_kernel_is_standard_normal():
    """loose sanity, 64 streams x 1024 samples: mean and variance of each within 5 sigma of N(0, 1) (holds for the restatement: test_voc_harness_cpu.py)"""
    xs = np.stack([philox(1024, 77, s).astype(np.float64) for s in range(64)])
    assert (np.abs(xs.mean(axis=1)) < 5 / np.sqrt(1024)).all() and (np.abs(xs.var(axis=1, ddof=1) - 1) < 5 * np.sqrt(2.0 / 1023)).all()
    assert abs(xs.mean()) < 5 / 256.0 and abs(xs.var() - 1) < 5 * np.sqrt(2.0 / 65535)
