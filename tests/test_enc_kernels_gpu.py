"""The eleven kernels of csrc/extras.hip and csrc/cvvp.hip (CLVP / CVVP encoder layers, the voice encoder, the diffusion conditioning encoder, CVVP's stem),
launched one at a time through the test-only harness (libtts_enc_test.so) and compared element by element with the float64 references of tests/enc_cases.py under
that module's derived bounds: every element of every case counts; the four copy kernels (embed, mel_rows, im2col3, im2col5) are compared bit for bit. Besides:
two runs agree in every bit; a sequence alone equals the same sequence in a batch; NaN in every row outside the sequences and in the input's margins changes no
bit; what the kernel may not write still holds the sentinel; the canary margins around every output are intact. tests/test_enc_harness_cpu.py shows that the
bounds pass a correct f32 implementation and are sharp.
With TTS_ENC_REPORT=<file> the largest error over bound per kernel and input family is written there (profiles/enc_direct.txt)."""
import faulthandler
import os
import re

import numpy as np
import pytest

import enc_cases as V

pytestmark = pytest.mark.gpu

RATIOS = {}  # (kernel, family) -> largest error / bound


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a launch that never returns ends the process instead of holding the GPU"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TTS_ENC_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("%-36s %-18s %12s\n" % ("kernel", "family", "|err|/bound"))
            for (k, fam), r in sorted(RATIOS.items()):
                f.write("%-36s %-18s %12.4f\n" % (k, fam, r))


def launch(c):
    """a failed HIP call (a fault included) ends the session: nothing more is started on a GPU that may have faulted"""
    try:
        out = V.run(c)
    except V.HipError as e:
        pytest.exit(str(e), returncode=3)
    assert out.canaries_intact(), c.name()
    return out.payload


def checked(c):
    """launch c; every written element within its bound (the copy kernels: equal bits), everything else still the sentinel -> the payload's bits"""
    bits = launch(c)
    ref, bound, wr = V.reference(c)
    assert bits.shape == wr.shape, c.name()
    sentinel = V.SENTINEL * (0x0101 if bits.dtype == np.uint16 else 0x01010101)
    assert (bits[~wr] == sentinel).all(), c.name()
    key = (c.kernel(), re.sub(r"\d+", "", c.family))
    if bound is None:
        bad = int((bits[wr] != ref[wr]).sum())
        RATIOS[key] = max(RATIOS.get(key, 0.0), float(bad))
        assert bad == 0, (c.name(), bad)
        return bits
    got = V.values(bits, c.op in V.F16_OUT)
    bad, r = V.judge(got[wr], ref[wr], bound[wr])
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print("%-120s rejected %d worst |err|/bound %.4f" % (c.name()[:120], bad, r))
    assert bad == 0, (c.name(), bad, r)
    return bits


def rows_of(c, bits, s, width):
    r0, n = int(c.start[s]), int(c.len[s])
    return bits.reshape(-1, width)[r0:r0 + n]


def test_copy_kernels_bit_for_bit():
    for c in V.copy_cases():
        bits = checked(c)
        assert (bits == launch(c)).all(), c.name()


@pytest.mark.parametrize("op", [V.RMSNORM, V.ROWNORM, V.POOL, V.ROWMEAN, V.GEGLU], ids=lambda o: V.OP_NAMES[o])
def test_row_kernels(op):
    n = 0
    for c in V.norm_cases():
        if c.op != op:
            continue
        n += 1
        bits = checked(c)
        assert (bits == launch(c)).all(), c.name()
        if op == V.RMSNORM:  # the all-zero row: exact zeros through the 1e-8 clamp, no NaN
            assert (V.values(bits, True).reshape(c.rows, c.dim)[3] == 0.0).all(), c.name()
    assert n


@pytest.mark.parametrize("D", [512, 1024, 2048])
def test_groupnorm(D):
    for c in V.norm_cases():
        if c.op != V.GROUPNORM or c.dim != D:
            continue
        bits = checked(c)
        assert (bits == launch(c)).all(), c.name()
        if c.nseq > 1:  # a clip alone: its neighbours (1e4 in the `neighbour` family) reach no statistic
            for s in range(c.nseq):
                assert (rows_of(c, bits, s, D) == launch(V.alone(c, s)).reshape(-1, D)).all(), (c.name(), s)


def _attn_groups(variant):
    cs = V.attn_cases(variant)
    nl = len(V.attn_lengths(variant)) * (2 if variant == V.BIAS128 else 1)
    return {"lengths": cs[:nl], "ramps": cs[nl:nl + 6], "dominant": cs[nl + 6:nl + 12], "layouts": cs[nl + 12:]}


@pytest.mark.parametrize("group", ["lengths", "ramps", "dominant", "layouts"])
@pytest.mark.parametrize("variant", [V.ROT64, V.PLAIN64, V.BIAS128], ids=["rot64", "plain64", "bias128"])
def test_attention_matrix(variant, group):
    cs = _attn_groups(variant)[group]
    assert cs
    for c in cs:
        bits = checked(c)
        assert (bits == launch(V.attn_poisoned(c))).all(), c.name()  # NaN in every row outside the sequences and in the margins
        if group == "layouts":
            assert (bits == launch(c)).all(), c.name()
            for s in range(c.nseq):  # positions are taken within the sequence: the same bits alone at row 0
                assert (rows_of(c, bits, s, c.dim) == launch(V.attn_alone(c, s)).reshape(-1, c.dim)).all(), (c.name(), s)


def test_attention_product_head_counts():
    for c in V.attn_product_cases():
        bits = checked(c)
        assert (bits == launch(V.attn_poisoned(c))).all(), c.name()
