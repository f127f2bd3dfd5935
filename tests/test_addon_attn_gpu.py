"""GPU: option addon_attn_precision (0 f32: cls_attn_kernel; 1 fp16 operands, 2 fp16 hi + lo pairs: addon_attn_h_kernel, csrc/addon_attn_h.h) through the C ABI,
on the small aligner (head dimension 64) and classifiers (128) of tests/aligner_ref.py and tests/classifier_ref.py against float64. Mode 2: logits within the
1e-3 gate and every aligner id the float64 argmax (the float64 top-two margin is asserted to exceed twice the gate first: no frame is excluded), also with
aligner_precision 2. Mode 1 is measured, not gated: ids are held to the argmax where the margin exceeds twice the measured distance."""
import numpy as np
import pytest

import aligner_ref as AR
import classifier_ref as CR

pytestmark = pytest.mark.gpu
ALIGNER_N = (40, 1310, 5150)  # 1, 65 and 257 frames
CLS = [(name, CR.GPU_SAMPLES[name][-1]) for name in ("tiny", "upstream")]

@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(kind, name, lin=0):  # lin: aligner_precision at the load
        if (kind, name, lin) not in made:
            e = pkg.Engine(0)
            if kind == "aligner":
                e.set_option("aligner_precision", lin)
                e.load_aligner(AR.model(name)[0])
            else:
                e.load_classifier(CR.model(name)[0])
            made[kind, name, lin] = e
        return made[kind, name, lin]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("lin", [0, 2], ids=["linears-f32", "linears-split"])
@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("n", ALIGNER_N)
def test_aligner_vs_float64(engines, n, mode, lin):
    eng, want = engines("aligner", "even", lin), AR.reference("even", n)
    assert AR.margin(want).min() > 2 * AR.GATE  # the argmax condition below excludes no frame
    eng.set_option("addon_attn_precision", mode)
    ids, logits = eng.aligner_ids([AR.wave("even", n)], 16000, logits=True)
    eng.set_option("addon_attn_precision", 0)
    assert logits[0].shape == want.shape and np.isfinite(logits[0]).all() and np.array_equal(ids[0], logits[0].argmax(1))
    err = np.abs(logits[0] - want).max()
    print("aligner n = %d addon_attn_precision %d aligner_precision %d: logits max abs distance from float64 %.2e (gate %.0e)" % (n, mode, lin, err, AR.GATE))
    sure = AR.margin(want) > (0 if mode == 2 else 2 * err)  # mode 2: every frame
    assert (mode == 1 or err <= AR.GATE) and np.array_equal(ids[0][sure], want.argmax(1)[sure]), "an id differs from the float64 argmax"


@pytest.mark.parametrize("mode", [1, 2], ids=["f16", "split"])
@pytest.mark.parametrize("name,n", CLS, ids=["%s-n%d" % c for c in CLS])
def test_classifier_vs_float64(engines, name, n, mode):
    eng, want = engines("classifier", name), CR.reference(name, n)
    eng.set_option("addon_attn_precision", mode)
    logits = eng.classify_audio([CR.wave(name, n)], 24000)[1]
    eng.set_option("addon_attn_precision", 0)
    err = np.abs(logits[0] - want).max()
    print("classifier %s n = %d addon_attn_precision %d: logits max abs distance from float64 %.2e (gate %.0e)" % (name, n, mode, err, CR.GATE))
    assert np.isfinite(logits).all() and (mode == 1 or err <= CR.GATE)


def test_mode_0_after_1_and_2_is_the_default_and_a_clip_alone_is_the_clip_in_a_batch(pkg, engines):
    ac, cc = [AR.wave("even", n, k=1 + i) for i, n in enumerate(AR.RAGGED)], [CR.wave("tiny", n, k=1 + i) for i, n in enumerate(CR.RAGGED)]
    runs = [(engines("aligner", "even"), lambda e, c: e.aligner_ids(c, 16000, logits=True)[1], ac, lambda e: e.load_aligner(AR.model("even")[0])),
            (engines("classifier", "tiny"), lambda e, c: list(e.classify_audio(c, 24000)[1]), cc, lambda e: e.load_classifier(CR.model("tiny")[0]))]
    for eng, call, clips, load in runs:
        for mode in (1, 2):
            eng.set_option("addon_attn_precision", mode)
            batch = call(eng, clips)
            for i, c in enumerate(clips):
                assert np.array_equal(call(eng, [c])[0], batch[i]), "mode %d: clip %d differs from itself alone" % (mode, i)
        eng.set_option("addon_attn_precision", 0)
        never = pkg.Engine(0)
        load(never)
        assert all(np.array_equal(a, b) for a, b in zip(call(eng, clips), call(never, clips))), "mode 0 after 1 and 2 is not the default"
        never.close()
