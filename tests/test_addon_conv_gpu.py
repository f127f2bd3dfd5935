"""GPU: option addon_conv_precision (0 f32; 1 fp16, 2 fp16 hi + lo pairs: hfg_conv_h_kernel and cls_down_h_kernel) through the C ABI on the small models of
tests/aligner_ref.py and tests/classifier_ref.py against float64. Clips: one whose every level is one row, and ones whose levels cross the strided kernel's 64-row
tile (aligner 261 / 130 / 65 and 1029 / 514 / 257 rows, classifier 4097 / 1025 / 257 and 1025 / 257 / 65 / 17 / 5 / 2). Mode 2 is gated at 1e-3, mode 1 measured."""
import numpy as np
import pytest

import aligner_ref as AR
import classifier_ref as CR

pytestmark = pytest.mark.gpu
ALIGNER_N = (40, 1310, 5150)  # 1, 65 and 257 frames
CLS = [("tiny", 1), ("tiny", 4097), ("upstream", 1025)]
LOAD = {"aligner": lambda e, name: e.load_aligner(AR.model(name)[0]), "classifier": lambda e, name: e.load_classifier(CR.model(name)[0])}

@pytest.fixture(scope="module")
def engines(pkg):
    made = {}
    def get(kind, name, conv=2, lin=0):  # conv, lin: addon_conv_precision and aligner_precision at the load
        if (kind, name, conv, lin) not in made:
            e = pkg.Engine(0)
            e.set_option("addon_conv_precision", conv)
            e.set_option("aligner_precision", lin)
            LOAD[kind](e, name)
            e.set_option("addon_conv_precision", 0)
            made[kind, name, conv, lin] = e
        return made[kind, name, conv, lin]
    yield get
    for e in made.values():
        e.close()

@pytest.mark.parametrize("others", [0, 2], ids=["alone", "with-linears-and-attention-split"])
@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("n", ALIGNER_N)
def test_aligner_vs_float64(engines, n, mode, others):
    eng, want = engines("aligner", "even", lin=others), AR.reference("even", n)
    assert AR.margin(want).min() > 2 * AR.GATE  # the argmax condition below excludes no frame
    eng.set_option("addon_conv_precision", mode)
    eng.set_option("addon_attn_precision", others)
    ids, logits = eng.aligner_ids([AR.wave("even", n)], 16000, logits=True)
    eng.set_option("addon_conv_precision", 0)
    eng.set_option("addon_attn_precision", 0)
    assert logits[0].shape == want.shape and np.isfinite(logits[0]).all() and np.array_equal(ids[0], logits[0].argmax(1))
    err = np.abs(logits[0] - want).max()
    print("aligner n = %d addon_conv_precision %d aligner_precision %d addon_attn_precision %d: logits max abs distance from float64 %.2e (gate %.0e)"
          % (n, mode, others, others, err, AR.GATE))
    sure = AR.margin(want) > (0 if mode == 2 else 2 * err)  # mode 2: every frame
    assert (mode == 1 or err <= AR.GATE) and np.array_equal(ids[0][sure], want.argmax(1)[sure]), "an id differs from the float64 argmax"

@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("name,n", CLS, ids=["%s-n%d" % c for c in CLS])
def test_classifier_vs_float64(engines, name, n, mode):
    eng, want = engines("classifier", name), CR.reference(name, n)
    eng.set_option("addon_conv_precision", mode)
    logits = eng.classify_audio([CR.wave(name, n)], 24000)[1]
    eng.set_option("addon_conv_precision", 0)
    err = np.abs(logits[0] - want).max()
    print("classifier %s n = %d addon_conv_precision %d: logits max abs distance from float64 %.2e (gate %.0e)" % (name, n, mode, err, CR.GATE))
    assert np.isfinite(logits).all() and (mode == 1 or err <= CR.GATE)

def test_batch_is_each_clip_alone_mode_0_is_the_default_and_planes_are_needed(pkg, engines):
    ac, cc = [AR.wave("even", n, k=1 + i) for i, n in enumerate(AR.RAGGED)], [CR.wave("tiny", n, k=1 + i) for i, n in enumerate(CR.RAGGED)]
    runs = [("aligner", "even", lambda e, c: e.aligner_ids(c, 16000, logits=True)[1], ac), ("classifier", "tiny", lambda e, c: list(e.classify_audio(c, 24000)[1]), cc)]
    for kind, name, call, clips in runs:
        eng = engines(kind, name)
        for mode in (1, 2):
            eng.set_option("addon_conv_precision", mode)
            batch = call(eng, clips)
            for i, c in enumerate(clips):
                assert np.array_equal(call(eng, [c])[0], batch[i]), "mode %d: clip %d differs from itself alone" % (mode, i)
        eng.set_option("addon_conv_precision", 0)
        never = pkg.Engine(0)
        LOAD[kind](never, name)
        assert all(np.array_equal(a, b) for a, b in zip(call(eng, clips), call(never, clips))), "mode 0 on a model loaded at 2 is not the default"
        for mode in (1, 2):  # loaded at 0: no planes
            never.set_option("addon_conv_precision", mode)
            with pytest.raises(pkg.TtsError, match=r"no fp16 planes.*\(status -5\)"):
                call(never, clips)
        never.close()
