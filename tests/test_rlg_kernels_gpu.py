"""The two kernels of csrc/random_voice.h, one launch at a time through the test-only harness (libtts_rlg_test.so), marked gpu: rlg_layer_kernel against float64
under the bounds tests/rlg_cases.py derives from its operation order, at dims 256 (the smallest the kernel accepts), 1024 and 2048, batch sizes 1, 2, tile - 1,
tile, tile + 1 and 2 tile + 1, with and without the activation; canary bytes around the output; NaN-poisoned rows beyond n; the exact family bit for bit; a voice
alone against the same voice at every position of a batch of tile + 1; two runs; rlg_noise_kernel inside the Philox bound.

Operands and references are made once per dim at the largest batch (a row's result does not depend on the rows beside it, which is itself asserted below)."""
import faulthandler

import numpy as np
import pytest

import rlg_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def problems():
    """{dim: (w, bias, x [2 tile + 1, dim], {act: (ref, bound)})}"""
    out = {}
    nmax = max(K.batch_sizes())
    for dim in K.DIMS:
        w, b, x = K.layer_operands(dim, nmax, 100 + dim)
        refs = {act: K.layer_reference(w, b, x, act) for act in (0, 1)}
        for a in (w, b, x) + refs[0] + refs[1]:
            a.setflags(write=False)
        out[dim] = (w, b, x, refs)
    return out


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dim", K.DIMS)
def test_layer_against_float64_under_the_derived_bound(problems, dim, act):
    w, b, x, refs = problems[dim]
    ref, bound = refs[act]
    assert K.batch_sizes() == (1, 2, K.tile() - 1, K.tile(), K.tile() + 1, 2 * K.tile() + 1)
    worst = 0.0
    for n in K.batch_sizes():
        out = K.run_layer(w, b, x[:n], act)
        assert out.canaries_intact(), n
        got = out.data
        assert np.isfinite(got).all(), n
        ratio = float((np.abs(got.astype(np.float64) - ref[:n]) / bound[:n]).max())
        worst = max(worst, ratio)
        print("dim %d act %d n %d: worst error / bound %.3f" % (dim, act, n, ratio))
    assert worst <= 1.0


@pytest.mark.parametrize("dim", K.DIMS)
def test_rows_beyond_n_are_never_read(problems, dim):
    w, b, x, _ = problems[dim]
    t = K.tile()
    for n in (1, t - 1, t + 1, 2 * t + 1):
        clean, poisoned = K.run_layer(w, b, x[:n], 1, poison=0), K.run_layer(w, b, x[:n], 1, poison=1)
        assert clean.canaries_intact() and poisoned.canaries_intact()
        assert np.isfinite(poisoned.data).all() and (_bits(clean.data) == _bits(poisoned.data)).all(), n


@pytest.mark.parametrize("dim", K.DIMS)
def test_exact_family_is_bit_for_bit(dim):
    n = K.tile() + 1
    w, b, x = K.layer_operands(dim, n, 7, "exact")
    ref = (x.astype(np.int64) @ w.astype(np.int64).T + b.astype(np.int64)).astype(np.float32)
    out = K.run_layer(w, b, x, 0)
    assert out.canaries_intact() and (_bits(out.data) == _bits(ref)).all()
    act = K.run_layer(w, b, x, 1).data  # with the activation: the positive results are ref * fl(sqrt 2) rounded once, the others ref * 0.2f rounded, then the gain
    want = np.where(ref > 0, ref, (ref * K.SLOPE32).astype(np.float32)).astype(np.float32) * K.GAIN32
    assert (_bits(act) == _bits(want.astype(np.float32))).all()


@pytest.mark.parametrize("dim", [256, 2048])
def test_alone_equals_every_position_of_a_batch_and_a_second_run(problems, dim):
    w, b, x, _ = problems[dim]
    n = K.tile() + 1
    voice = x[n]  # a row the batch below does not hold
    alone = K.run_layer(w, b, voice[None], 1).data[0].copy()
    again = K.run_layer(w, b, voice[None], 1).data[0]
    assert (_bits(alone) == _bits(again)).all()
    base = K.run_layer(w, b, x[:n], 1).data.copy()
    for p in range(n):
        xb = x[:n].copy()
        xb[p] = voice
        got = K.run_layer(w, b, xb, 1).data
        assert (_bits(got[p]) == _bits(alone)).all(), p
        others = [q for q in range(n) if q != p]
        assert (_bits(got[others]) == _bits(base[others])).all(), p  # and the rows beside it do not notice


def test_noise_inside_the_philox_bound_and_keyed_by_seed_and_side():
    seeds = [0, 1, 7, 5, 2 ** 32 + 5, 2 ** 64 - 1]
    got = {}
    for side, dim in ((0, 1024), (1, 2048), (1, 256)):
        out = K.run_noise(seeds, side, dim)
        assert out.canaries_intact()
        for k, s in enumerate(seeds):
            ref, bound = K.noise_reference(dim, s, side)
            assert (np.abs(out.data[k].astype(np.float64) - ref) <= bound).all(), (side, dim, s)
            got[(side, dim, s)] = out.data[k].copy()
        one = K.run_noise(seeds[2:3], side, dim)
        assert (_bits(one.data[0]) == _bits(out.data[2])).all()  # a seed's row does not depend on the batch
    assert (got[(1, 2048, 7)][:256] == got[(1, 256, 7)]).all()     # nor on the channel count
    assert (got[(0, 1024, 7)][:256] != got[(1, 256, 7)]).mean() > 0.99
    assert (got[(0, 1024, 7)] != got[(0, 1024, 1)]).mean() > 0.99
    assert (got[(0, 1024, 2 ** 32 + 5)] != got[(0, 1024, 5)]).mean() > 0.99  # the high word of the seed is part of the key
