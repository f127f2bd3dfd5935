"""The HiFi-GAN decoder's kernels (hfg_conv_kernel<1> / <2>, hfg_conv_small_kernel, hfg_interp_kernel, hfg_cond_kernel, hfg_post_kernel of csrc/hifigan.hip),
launched one at a time through the test-only harness (libtts_hfg_test.so) and compared element by element with the float64 references of tests/hfg_cases.py under
that module's derived bounds; the exact family bit for bit. Stated as tests besides: no store leaves a candidate's live rows (every other row of the output keeps
the 0xCB pattern, canaries intact); NaN on every input row outside the candidates gives the same bits; hfg_conv_kernel and hfg_conv_small_kernel give the same
bits; a candidate gives the same bits alone and in a batch; two runs give the same bits; and the harness, driven through hifigan_run's whole launch sequence from
Python, gives the bytes of Engine.hifigan_decode. tests/test_hfg_harness_cpu.py shows that the rule passes a correct f32 implementation and is sharp.
With TTS_HFG_REPORT=<file> the largest error over bound per kernel and input family, the tanhf error seen and what the MFMA probe saw are written there
(profiles/hfg_direct.txt)."""
import faulthandler
import os

import numpy as np
import pytest

import hfg_cases as V
from hfg_cases import COND, CONV, CONV_SMALL, INTERP, POST
from test_hifigan_cpu import hifigan_model, inputs  # noqa: F401  (session fixture: the synthetic model file)

pytestmark = pytest.mark.gpu

RATIOS = {}  # (kernel, family) -> largest error / bound
NOTES = []   # measurements that are no ratios
KINDS = [CONV, CONV_SMALL, INTERP, COND, POST]


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a launch that never returns ends the process instead of holding the GPU"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TTS_HFG_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("%-24s %-18s %12s\n" % ("kernel", "family", "|err|/bound"))
            for (k, fam), r in sorted(RATIOS.items()):
                f.write("%-24s %-18s %12.4f\n" % (k, fam, r))
            for n in NOTES:
                f.write(n + "\n")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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


def checked(c, fam=None):
    """launch c; every element within its bound (the exact family: bit-equal), no store outside the live rows -> (payload, reference)"""
    ref = V.reference(c)
    o = launch(c)
    bad, r = V.judge(o, ref)
    key = (V.KIND_NAMES[c.kind], fam or c.family)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print("%-110s rejected %d worst |err|/bound %.4f" % (c.name(), bad, r))
    if bad:
        with np.errstate(invalid="ignore"):
            i = tuple(np.argwhere(~(np.abs(o.astype(np.float64) - ref["z"]) <= ref["bound"]) & ref["live"].reshape((-1,) + (1,) * (o.ndim - 1)))[0])
        print("   first rejected: %r out %r reference %r bound %r" % (i, o[i], ref["z"][i], ref["bound"][i]))
    assert bad == 0, (c.name(), bad, r)
    u = c.p.get("phases", 1) if c.kind in (CONV, CONV_SMALL) else 1
    if u > 1:  # every phase of a transposed convolution on its own
        for ph in range(u):
            sub = dict(z=ref["z"][ph::u], bound=ref["bound"][ph::u], live=ref["live"][ph::u])
            bp, rp = V.judge(o[ph::u], sub)
            assert bp == 0 and sub["live"].any(), (c.name(), ph, bp, rp)
            kp = (V.KIND_NAMES[c.kind], "phase %d of %d" % (ph, u))
            RATIOS[kp] = max(RATIOS.get(kp, 0.0), rp)
    if ref["exact"]:
        assert V.exact_family_is_exact(c, ref) and V.exact_ok(o, ref), c.name()
    assert V.guards_ok(c, o), c.name()
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
    pz = V.poisoned(c)
    if pz is not None:  # NaN on every row of the inputs outside the candidates' live rows: nothing may change
        assert np.array_equal(_bits(launch(pz)), _bits(o)), "the launch read a row outside the candidates"
    if c.kind == CONV_SMALL:  # the 256-row tile on the same inputs: the same chain of the same instructions, hence the same bits
        assert np.array_equal(_bits(launch(V.twin(c))), _bits(o)), "hfg_conv_kernel and hfg_conv_small_kernel differ"


@pytest.mark.parametrize("kind", [CONV, CONV_SMALL])
@pytest.mark.parametrize("family", ["gauss", "exact"])
def test_acc_mode_2_on_top_of_an_out_written_by_modes_0_and_1(kind, family):
    """the three-ResBlock mean as hifigan_run builds it: =, +=, (+) / 3 into the same buffer, each launch held to its own reference on what the one before left"""
    out = None
    for acc in (0, 1, 2):
        c = V.make(kind, "B", family, seed=40 + acc, cin=64, cout=128, taps=(3, 7, 11)[acc], dil=1, rate=8, slope=0.5 if family == "exact" else 0.1, acc=acc, resid=1)
        if acc:
            c.a["out0"] = out
        out, _ = checked(c, family + " mean")
    assert V.guards_ok(c, out)


def test_resid_may_be_the_output_buffer():
    """resid == out (hifigan_run's second dilation of a ResBlock): the same bits as the same tensor passed as a buffer of its own"""
    for kind in (CONV, CONV_SMALL):
        a = V.make(kind, "C", "gauss", seed=50, cin=64, cout=128, taps=7, dil=1, rate=8, resid=2)
        b = V.Case(kind, a.lay, a.family, dict(a.p, resid=1), dict(a.a, resid=a.a["out0"]), a.lname)
        del b.a["out0"]
        oa, _ = checked(a)
        ob, _ = checked(b)
        assert np.array_equal(_bits(oa), _bits(ob))


def test_conv_post_first_and_last_samples_of_every_candidate():
    """the first and the last three samples of a candidate read three rows fewer on one side, and nothing of the rows beside the candidate"""
    c = V.poisoned(V.make(POST, "C", "ramp", seed=2))
    o, ref = checked(c, "ramp ends")
    for s in range(c.lay.ns):
        n = c.lay.keep_n[s] * 256
        e = np.r_[0:3, n - 3:n] + c.lay.before[s] * 256
        assert np.isfinite(o[e]).all() and (np.abs(o[e] - ref["z"][e]) <= ref["bound"][e]).all()
    d = V.make(POST, "D", "outlier", seed=3)  # windows that keep interior frames only; the `before` offsets of a ragged batch
    o, ref = checked(d)
    assert d.lay.before == [0, 4] and o.shape == (6 * 256,)


def test_interp_first_and_last_frames():
    """L = 1, 2, 3 whole and the first 12 / last 12 frames of L = 500: the clamps at 0 and at the last latent row act within the first and the last 9 frames"""
    for lname in ("I", "J"):
        c = V.make(INTERP, lname, "ramp", seed=4)
        o, ref = checked(c, "ramp ends")
        for s in range(c.lay.ns):
            assert c.lay.w0[s] + c.lay.W[s] <= V.harness().tts_hfg_test_frames(c.lay.L[s])
    c = V.make(INTERP, "I", "outlier", seed=5)
    o, ref = checked(c)
    row = c.a["in_"][0].astype(np.float64)
    assert (np.abs(o[:4] - row[None, :]) <= 8 * V.U * np.abs(row)[None, :]).all()  # L = 1: the row itself, to the value roundings alone


def test_tanhf_error_seen():
    """weight 1 on one tap of one channel, zero bias, inputs >= 0: the pre-activation is the input element exactly and the output is device tanhf of it"""
    c = V.make(POST, "B", "tanh", seed=6)
    o, ref = checked(c)
    x = np.concatenate([c.a["in_"][c.lay.rows(s, 256), 0] for s in range(c.lay.ns)]).astype(np.float64)
    assert np.array_equal(ref["pre"], x)
    z = ref["z"]
    ulp = np.spacing(np.abs(z).astype(np.float32)).astype(np.float64)
    e = np.abs(o.astype(np.float64) - z) / ulp
    NOTES.append("device tanhf over %d arguments in [1e-6, 1200]: largest error %.3f ulp (allowance %.0f ulp), %.1f %% correctly rounded"
                 % (len(x), e.max(), V.TANH_ULP, 100.0 * (e <= 0.5).mean()))
    print(NOTES[-1])
    assert e.max() <= V.TANH_ULP


def test_mfma_product_probe():
    """Measurements, recorded: (1) channel 0 holds -fl(a b) x 1 and channel 2 holds a x b, one MFMA apart on the same lane half: the output is a b - fl(a b)
    exactly if the f32 MFMA keeps the product unrounded into the add, 0 if it rounds the product first. (2) a product of 2^-130: kept or flushed."""
    c = V.make(CONV, "A", "gauss", seed=7, cin=32, cout=32, taps=1, dil=1, rate=1, slope=1.0)
    rs = np.random.RandomState(1)
    a, b = (1 + rs.rand(4)).astype(np.float32), np.float32(1.2345678)
    x = np.zeros((8, 32), np.float32)
    x[:4, 0] = -(a * b)
    x[:4, 2] = a
    c.a["in_"] = x
    c.a["w"][:] = 0
    c.a["w"][0, 0, :] = 1
    c.a["w"][0, 2, :] = b
    c.a["bias"][:] = 0
    o, ref = checked(c, "probe")
    resid = a.astype(np.float64) * float(b) - (a * b).astype(np.float64)
    assert (resid != 0).all() and np.array_equal(ref["z"][:4], np.repeat(resid[:, None], 32, 1))
    fused, rounded = bool((o[:4] == resid[:, None].astype(np.float32)).all()), bool((o[:4] == 0).all())
    NOTES.append("v_mfma_f32_32x32x2_f32 probe, -fl(ab) + a b: %s" % ("a b - fl(a b) exactly: the product enters the add unrounded (fused)" if fused else
                                                                      "0: the product is rounded before the add" if rounded else "neither: %r" % (o[:4, 0],)))
    c.a["in_"] = np.zeros((8, 32), np.float32)
    c.a["in_"][:4, 0] = np.float32(2.0 ** -100)
    c.a["w"][:] = 0
    c.a["w"][0, 0, :] = np.float32(2.0 ** -30)
    o, ref = checked(c, "probe")
    NOTES.append("a product of 2^-130 through the MFMA and the epilogue's add of a zero bias: %s" % ("kept" if (o[:4] == np.float32(2.0 ** -130)).all() else
                                                                                                  "flushed to zero" if (o[:4] == 0).all() else repr(o[:4, 0])))
    print("\n".join(NOTES[-2:]))


ALONE = [(CONV, dict(cin=32, cout=32, taps=11, dil=5, rate=1, resid=1, cbias=1)), (CONV, dict(cin=64, cout=64, taps=7, dil=3, rate=59, acc=2, cbias=1)),
         (CONV, dict(cin=64, cout=128, taps=3, dil=1, rate=8, acc=1, resid=2)), (CONV, dict(cin=64, cout=32, taps=2, phases=8, rate=1, cbias=1)),
         (CONV, dict(cin=64, cout=64, taps=2, phases=2, rate=59)), (CONV_SMALL, dict(cin=64, cout=128, taps=11, dil=5, rate=1, resid=1, cbias=1)),
         (CONV_SMALL, dict(cin=32, cout=256, taps=7, dil=3, rate=8, acc=2, cbias=1)), (CONV_SMALL, dict(cin=64, cout=128, taps=2, phases=8, rate=8, cbias=1)),
         (INTERP, {}), (COND, {}), (POST, {})]


@pytest.mark.parametrize("kind,p", ALONE, ids=["-".join([V.KIND_NAMES[k].replace("_kernel", "")] + ["%s%s" % kv for kv in sorted(p.items())]) for k, p in ALONE])
def test_a_candidate_of_layout_c_equals_the_same_candidate_alone(kind, p):
    c = V.make(kind, "C", "gauss", seed=21, **p)
    o, _ = checked(c)
    for s in range(c.lay.ns):
        one = V.alone(c, s)
        o1, _ = checked(one)
        assert np.array_equal(_bits(V.seq_out(one, o1, 0)), _bits(V.seq_out(c, o, s))), (c.name(), s)


def test_the_harness_driven_chain_is_byte_equal_to_hifigan_decode(pkg, hifigan_model):
    """hifigan_run's whole launch sequence for L = 3 (T = 13), one harness launch per kernel, on the synthetic model file: the buffers x, u, t, m and their aliasing
    as hifigan_run has them, the weights repacked from the file's PyTorch layouts by hfg_cases.repack_conv / repack_convt. The samples are the bytes of
    Engine.hifigan_decode: the loader's [k][cin][cout] / [phase][2][cin][cout] packing and the harness's restated launch parameters are the product's."""
    from tortoise_cpp_amd import synth_weights as sw
    W = sw.read_ggml(hifigan_model)
    lat, voice = inputs(3)
    lay = V.Layout([V.whole(13, 0, 3)])
    assert lay.frames == 16 and V.harness().tts_hfg_test_frames(3) == 13

    def go(kind, p, **a):
        return launch(V.Case(kind, lay, "model", p, {k: np.ascontiguousarray(v, np.float32) for k, v in a.items() if v is not None}, "chain"))

    def conv(in_, name, cin, cout, taps, dil, phases, rate, slope, acc=0, cbias=None, resid=None, out0=None, alias=False):
        w = W[name + ".weight"]
        p = dict(cin=cin, cout=cout, taps=taps, dil=dil, phases=phases, rate=rate, slope=slope, acc=acc, cbias=int(cbias is not None), resid=2 if alias else int(resid is not None))
        return go(CONV, p, in_=in_, w=w if phases > 1 else V.repack_conv(w), bias=W[name + ".bias"], cbias=cbias, resid=resid, out0=out0)
    z = go(INTERP, {}, in_=lat)
    cb = go(COND, {}, in_=voice.reshape(1, 1024), w=W["hifigan.cond_layer.weight"].reshape(512, 1024), bias=W["hifigan.cond_layer.bias"])
    x = conv(z, "hifigan.conv_pre", 1024, 512, 7, 1, 1, 1, 1.0, cbias=cb)
    cur, ch, rate, m = x, 512, 1, None
    for i, u_ in enumerate(V.UP):
        u = conv(cur, "hifigan.ups.%d" % i, ch, ch // 2, 2, 1, u_, rate, 0.1)
        ch //= 2
        rate *= u_
        for j, k in enumerate(V.RES_K):
            rb = "hifigan.resblocks.%d" % (3 * i + j)
            r = u  # the ResBlock's stream: u for the first dilation, then x
            for n, d in enumerate(V.RES_D):
                t = conv(r, "%s.convs1.%d" % (rb, n), ch, ch, k, d, 1, rate, 0.1)
                if n == 0:
                    x = conv(t, "%s.convs2.%d" % (rb, n), ch, ch, k, 1, 1, rate, 0.1, resid=r)
                elif n == 1:
                    x = conv(t, "%s.convs2.%d" % (rb, n), ch, ch, k, 1, 1, rate, 0.1, out0=x, alias=True)  # resid == out == x
                else:
                    m = conv(t, "%s.convs2.%d" % (rb, n), ch, ch, k, 1, 1, rate, 0.1, acc=j, resid=x, out0=m if j else None)  # the mean: =, +=, (+) / 3
                r = x
        cur = m
    audio = go(POST, {}, in_=cur, w=V.repack_conv(W["hifigan.conv_post.weight"])[:, :, 0], bias=W["hifigan.conv_post.bias"])
    eng = pkg.Engine(0)
    try:
        eng.load_hifigan(hifigan_model)
        want = eng.hifigan_decode([lat], voice)[0]
    finally:
        eng.close()
    assert audio.shape == want.shape == (13 * 256,) and np.isfinite(want).all() and want.std() > 0.01
    assert np.array_equal(_bits(audio), _bits(want)), "max abs difference %.3g" % np.abs(audio - want).max()
