"""GPU: option aligner_precision (0 f32, 1 fp16 operands, 2 fp16 hi + lo pairs: the encoder's Linears on w2v_linear_h_kernel, csrc/w2v_linear_h.h) through the C
ABI, on tests/aligner_ref.py's two configurations at its clip lengths. tests/test_aligner_cpu.py asserts that the float64 top-two margin exceeds twice the gate
on every frame of those clips, so in mode 2 no frame is excluded: logits within R.GATE (1e-3) of float64 and every id the float64 argmax. Mode 1 is measured, not
gated (the distance is printed; profiles/aligner_f16.txt records it): its ids must be the float64 argmax wherever the margin exceeds twice the measured distance.
Both modes: ids == argmax of the engine's own logits, two calls agree, the ragged batch gives each clip alone bit for bit. Mode 0 set explicitly returns the bytes
of the option left unset, and a model loaded without planes refuses modes 1 / 2 with TTS_ERR_STATE."""
import numpy as np
import pytest

import aligner_ref as R
from test_aligner_gpu import S, _raw

pytestmark = pytest.mark.gpu
CASES = [(name, n) for name in R.CONFIGS for n in R.GPU_SAMPLES[name]]


@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(name, mode):  # mode None: the option is never touched
        if (name, mode) not in made:
            e = pkg.Engine(0)
            if mode is not None:
                e.set_option("aligner_precision", mode)  # before the load: tts_load_aligner packs the planes
            e.load_aligner(R.model(name)[0])
            made[name, mode] = e
        return made[name, mode]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("name,n", CASES, ids=["%s-n%d" % c for c in CASES])
def test_engine_vs_float64(engines, name, n, mode):
    eng, want = engines(name, mode), R.reference(name, n)
    ids, logits = eng.aligner_ids([R.wave(name, n)], 16000, logits=True)
    assert logits[0].shape == want.shape and np.isfinite(logits[0]).all()
    err = np.abs(logits[0] - want).max()
    print("aligner %s n = %d aligner_precision %d: %d frames, logits max abs distance from float64 %.2e (gate %.0e, smallest margin %.4f)"
          % (name, n, mode, want.shape[0], err, R.GATE, R.margin(want).min()))
    assert np.array_equal(ids[0], logits[0].argmax(1))
    if mode == 2:
        assert err <= R.GATE and np.array_equal(ids[0], want.argmax(1)), "an id differs from the float64 argmax"
    else:
        sure = R.margin(want) > 2 * err
        assert np.array_equal(ids[0][sure], want.argmax(1)[sure])
    again = eng.aligner_ids([R.wave(name, n)], 16000, logits=True)
    assert np.array_equal(again[1][0], logits[0]) and np.array_equal(again[0][0], ids[0]), "two calls differ"


@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
def test_ragged_batch_is_each_clip_alone(engines, mode):
    eng = engines("even", mode)
    clips = [R.wave("even", n, k=1 + i) for i, n in enumerate(R.RAGGED)]
    ia, la = eng.aligner_ids(clips, 16000, logits=True)
    ib, lb = eng.aligner_ids(clips, 16000, logits=True)
    for i, c in enumerate(clips):
        i1, l1 = eng.aligner_ids([c], 16000, logits=True)
        assert np.array_equal(la[i], lb[i]) and np.array_equal(ia[i], ib[i]), "two calls differ"
        assert np.array_equal(l1[0], la[i]) and np.array_equal(i1[0], ia[i]), "clip %d differs from itself alone" % i


def test_mode_0_is_the_default_and_planes_are_needed(engines):
    unset, zero = engines("even", None), engines("even", 0)
    clips = [R.wave("even", n, k=1 + i) for i, n in enumerate(R.RAGGED)]
    (iu, lu), (iz, lz) = unset.aligner_ids(clips, 16000, logits=True), zero.aligner_ids(clips, 16000, logits=True)
    assert all(np.array_equal(a, b) for a, b in zip(iu + lu, iz + lz))
    x, n, r = clips[0], np.array([len(clips[0])], np.int64), np.array([16000], np.int32)
    ids, nf = np.full(64, 7, np.int32), np.full(1, 7, np.int32)
    for mode in (1, 2):  # loaded at 0: no planes
        zero.set_option("aligner_precision", mode)
        assert _raw(zero, x, n, r, 1, ids, nf, 64, None) == S and b"no fp16 planes" in zero.L.tts_last_error(zero.h)
    zero.set_option("aligner_precision", 0)
    assert (ids == 7).all() and nf[0] == 7, "a refused call wrote its output"
    assert np.array_equal(zero.aligner_ids(clips, 16000)[0], iu[0])
