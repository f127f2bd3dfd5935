"""The audio front-end's kernels (afe_resample_kernel, afe_mel_kernel<80, 2> / <100, 1>, afe_nonfinite_kernel of csrc/audio_frontend.hip), launched one at a time
through the test-only harness (libtts_afe_test.so) and compared element by element with the float64 references of tests/afe_cases.py under that module's derived
bounds: every element counts. Bit for bit besides: silence is the floor constant in every cell; a clip shorter than its window equals the host-zero-padded clip; a
cropped window equals the cropped clip; two runs agree; a clip in a batch of three ragged clips equals that clip alone; the canary words around every output are
intact. tests/test_afe_harness_cpu.py shows that the bounds pass a correct f32 implementation and are sharp.
With TTS_AFE_REPORT=<file> the largest error over bound per kernel and input family is written there (profiles/voice_from_audio.txt)."""
import faulthandler
import os

import numpy as np
import pytest

import afe_cases as V
from afe_cases import MEL80, MEL100, NONFINITE, RESAMPLE, Case

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
    path = os.environ.get("TTS_AFE_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("%-24s %-18s %12s\n" % ("kernel", "family", "|err|/bound"))
            for (k, fam), r in sorted(RATIOS.items()):
                f.write("%-24s %-18s %12.4f\n" % (k, fam, r))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(c):
    """a failed HIP call (a fault included) ends the session: nothing more is started on a GPU that may have faulted"""
    try:
        out = V.run(c)
    except V.HipError as e:
        pytest.exit(str(e), returncode=3)
    assert out.canaries_intact(), c.name()
    return out.payload


def split(c, payload):
    if c.kind == RESAMPLE:
        sizes = [V.res_len(c.p["orig"], c.p["new"], len(x)) for x in c.clips]
    else:
        sizes = [(80 if c.kind == MEL80 else 100) * (w // 256 + 1) for w in c.p["win"]]
    assert sum(sizes) == len(payload), c.name()
    return np.split(payload, np.cumsum(sizes)[:-1])


def checked(c):
    """launch c; every element of every clip within its bound -> the payload"""
    o = launch(c)
    for got, (ref, bound) in zip(split(c, o), V.reference(c)):
        assert got.shape == ref.shape, c.name()
        bad, r = V.judge(got, ref, bound)
        key = (V.KIND_NAMES[c.kind], c.family)
        RATIOS[key] = max(RATIOS.get(key, 0.0), r)
        print("%-100s rejected %d worst |err|/bound %.4f" % (c.name(), bad, r))
        assert bad == 0, (c.name(), bad, r)
    return o


# ---- resampler ----
@pytest.mark.parametrize("pair", V.RATE_PAIRS, ids=["%d_%d" % p for p in V.RATE_PAIRS])
def test_resampler_matrix(pair):
    assert V.lib().tts_afe_test_block() == V.BLOCK
    for c in V.res_cases():
        if (c.p["orig"], c.p["new"]) == pair:
            checked(c)


def test_resampler_equal_rates_copy_and_limit_pair():
    x = V.res_input("noise", 1000, 9)
    x[3] = np.float32(-0.0)
    o = launch(Case(RESAMPLE, [x], "copy", orig=22050, new=22050))
    assert (_bits(o) == _bits(x)).all()
    c = Case(RESAMPLE, [x], "limit", orig=V.LIMIT_PAIR[0], new=V.LIMIT_PAIR[1])
    assert V.validate(c) == V.ERR_LIMIT
    with pytest.raises(V.HipError):
        V.run(c)  # refused before any device call


def test_resampler_identities():
    a, b = 16000, 22050
    clips = [V.res_input("noise", n, 40 + i) for i, n in enumerate((961, 37, 400))]
    batch = Case(RESAMPLE, clips, "batch", orig=a, new=b)
    o1 = checked(batch)
    assert (_bits(o1) == _bits(launch(batch))).all()  # two runs
    for s, part in enumerate(split(batch, o1)):
        assert (_bits(part) == _bits(launch(batch.alone(s)))).all(), s


# ---- mel ----
@pytest.mark.parametrize("bands", [80, 100])
def test_mel_matrix(bands):
    assert V.lib().tts_afe_test_fpw() == V.FPW
    for c in V.mel_cases(bands):
        o = checked(c)
        if c.family == "zeros":
            assert (_bits(o) == _bits(V.LOG_FLOOR)).all(), c.name()


@pytest.mark.parametrize("bands,win,frames", [(80, V.WIN80, 517), (100, V.WIN100, 401)])
def test_mel_upstream_window(bands, win, frames):
    kind = MEL80 if bands == 80 else MEL100
    x = V.mel_input("noise", win, 1234, bands)
    o = checked(Case(kind, [x], "noise_window", start=[0], win=[win]))
    assert len(o) == bands * frames
    z = launch(Case(kind, [np.zeros(win, np.float32)], "zeros", start=[0], win=[win]))
    assert (_bits(z) == _bits(V.LOG_FLOOR)).all()


@pytest.mark.parametrize("bands,with_norms", [(80, False), (80, True), (100, False)])  # the product divides the 80-band side only (the harness refuses norms on the other)
def test_mel_window_handling(bands, with_norms):
    kind = MEL80 if bands == 80 else MEL100
    norms = V.mel_norms() if with_norms else None
    kw = dict(norms=norms) if with_norms else {}
    x = V.mel_input("noise", 1500, 5, bands)
    # shorter than the window: the zeros behind the clip are never stored anywhere
    short = checked(Case(kind, [x[:700]], "short_clip", start=[0], win=[1000], **kw))
    padded = launch(Case(kind, [np.concatenate([x[:700], np.zeros(300, np.float32)])], "padded", start=[0], win=[1000], **kw))
    assert (_bits(short) == _bits(padded)).all()
    # longer than the window: from the front, and from the last offset that keeps the window inside the clip
    for start in (0, 500):
        crop = checked(Case(kind, [x], "crop_%d" % start, start=[start], win=[1000], **kw))
        assert (_bits(crop) == _bits(launch(Case(kind, [x[start:start + 1000]], "cropped", start=[0], win=[1000], **kw)))).all()
    if with_norms:
        z = launch(Case(kind, [np.zeros(700, np.float32)], "zeros", start=[0], win=[700], **kw))
        want = np.repeat((V.LOG_FLOOR / norms)[:, None], 700 // 256 + 1, axis=1).astype(np.float32)
        assert (_bits(z) == _bits(want.reshape(-1))).all()


@pytest.mark.parametrize("bands", [80, 100])
def test_mel_identities(bands):
    kind = MEL80 if bands == 80 else MEL100
    lens = (1300, 513, 2200)  # 6, 3 and 9 frames: ragged, and none a multiple of the frames per workgroup
    clips = [V.mel_input("noise" if i != 1 else "tone_over_noise", n, 60 + i, bands) for i, n in enumerate(lens)]
    batch = Case(kind, clips, "batch", start=[0, 0, 100], win=[1300, 513, 2100])
    o1 = checked(batch)
    assert (_bits(o1) == _bits(launch(batch))).all()
    for s, part in enumerate(split(batch, o1)):
        assert (_bits(part) == _bits(launch(batch.alone(s)))).all(), s


def test_nonfinite_count():
    x = V.res_input("noise", 70000, 3)
    assert launch(Case(NONFINITE, [x], "finite")).view(np.uint32)[0] == 0
    x[[0, 255, 256, 40000, 69999]] = [np.nan, np.inf, -np.inf, np.nan, np.nan]
    assert launch(Case(NONFINITE, [x, x[:300]], "five_and_three")).view(np.uint32)[0] == 8
