"""CPU: what pins AR scoring (tts_ar_score_codes / tts_host_ar_score_rows, csrc/ar_score.h) without a GPU: the float64 reference in two spellings, a float32
restatement of the kernels' order under the derived bounds (tests/ar_score_ref.py), seeded defects that the bounds or the argmax rule must catch, the row table
against a literal restatement, every refusal a host-only context and the harness's validation can give, the CLI's usage errors, and the two conditions the GPU
tests rely on, checked on the references alone: the share of rows the argmax margin leaves out, and that the two position modes give different scores."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ar_score_cases as A
import ar_score_ref as R
from conftest import DEFAULT_TOKENS

ROOT = A.ROOT
ARG, HIP, STATE, LIMIT = -1, -4, -5, -6
FULL_SUBSET = (0, 1, 2, 3, 4, 5, 6, 7, 8, 66, 67, 128, 129)  # the planted ties and the edge targets of the full head: a 1024-step chain over 13 rows


def _subset(c, rows):
    rows = list(rows)
    return A.Case(c.label + "-subset", c.hn[rows], c.W, c.b, c.tgt[rows], c.N, c.planted[rows])


def _cpu_cases():
    return [A.small_case(), A.extreme_case(A.SMALL), A.extreme_case(A.FULL), A.tail_tie_case(), _subset(A.full_case(), FULL_SUBSET)]


def test_the_two_float64_spellings_agree():
    for c in (A.small_case(), A.full_case(), A.extreme_case(A.SMALL), A.extreme_case(A.FULL)):
        l = c.reference().logits
        d = np.abs(R.direct64(l) - R.slabwise64(l)).max()
        print("%s: direct against slab-wise %.2e" % (c.label, d))
        assert d <= 1e-14 * max(1.0, float(np.abs(c.reference().lse).max()))


def test_the_float32_restatement_stays_inside_the_bounds():
    for c in _cpu_cases():
        ref = R.Ref(c.hn, c.W, c.b, c.tgt, c.N)
        got = R.score32(c.hn, c.W, c.b, c.tgt, c.N)
        ratios = ref.ratios(got)
        print("%s: worst ratio to the bound %s" % (c.label, ", ".join("%s %.3f" % kv for kv in ratios.items())))
        assert max(ratios.values()) <= 1.0, (c.label, ratios)
        assert not ref.argmax_failures(got["greedy"], c.planted), c.label


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_a_seeded_defect_falls_ten_bounds_outside_or_fails_the_argmax_rule(defect):
    caught = []
    for c in (A.small_case(), A.extreme_case(A.SMALL), A.tail_tie_case()):
        ref = R.Ref(c.hn, c.W, c.b, c.tgt, c.N)
        got = R.score32(c.hn, c.W, c.b, c.tgt, c.N, defect=defect)
        worst = max(ref.ratios(got).values())
        fails = ref.argmax_failures(got["greedy"], c.planted)
        if worst >= 10.0 or fails:
            caught.append((c.label, worst, len(fails)))
    print(defect, caught)
    assert caught, defect


def test_the_argmax_margin_leaves_out_at_most_five_percent_of_the_rows():
    for c in (A.small_case(), A.full_case(), A.tail_tie_case()):
        ref = c.reference()
        free = c.planted < 0
        share = float((~ref.decided[free]).mean())
        print("%s: %.4f of the rows under the margin" % (c.label, share))
        assert share <= R.MAX_LEFT_OUT
        # the planted ties are exact in float64 too, and their lower index is the maximum
        for r in np.nonzero(~free)[0]:
            assert ref.margin[r] == 0.0 and ref.top[r] == c.planted[r]


@pytest.mark.parametrize("mode", ("decode", "train"))
def test_row_table_matches_a_literal_restatement(pkg, mode):
    g = np.random.default_rng(3)
    for n in (1, 2, 500):
        codes = g.integers(0, 8192, n).astype(np.int32)
        got, want = pkg.host_ar_score_rows(codes, mode), R.score_rows(codes, mode)
        for a, b in zip(got, want):
            assert a.dtype == np.int32 and np.array_equal(a, b)
        assert got[0][0] == 8192 and got[1][0] == 0 and got[2][-1] == 8193 and got[1].max() < 608
        assert not np.array_equal(got[1], R.score_rows(codes, mode, off_by_one=True)[1])  # the seeded defect of the position rule
    assert np.array_equal(pkg.host_ar_score_rows([5, 6, 7], "decode")[1], [0, 2, 3, 4]) and np.array_equal(pkg.host_ar_score_rows([5, 6, 7], "train")[1], [0, 1, 2, 3])


def test_row_table_refusals(pkg):
    L = pkg.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    codes = np.array([1, 2, 3], np.int32)
    outs = [np.full(502, 7, np.int32) for _ in range(3)]
    call = lambda c=codes, n=3, pos=0, o=outs: L.tts_host_ar_score_rows(p(c), n, pos, p(o[0]), p(o[1]), p(o[2]))  # noqa: E731
    assert call(n=0) == ARG and call(pos=2) == ARG and call(pos=-1) == ARG and call(c=None) == ARG
    assert call(o=[None, outs[1], outs[2]]) == ARG and call(o=[outs[0], None, outs[2]]) == ARG and call(o=[outs[0], outs[1], None]) == ARG
    assert call(c=np.array([1, 8192, 3], np.int32)) == ARG and call(c=np.array([-1, 2, 3], np.int32)) == ARG
    assert call(c=np.zeros(501, np.int32), n=501) == LIMIT
    assert all((o == 7).all() for o in outs), "a refused call wrote its output"
    assert call() == 0 and list(outs[0][:4]) == [8192, 1, 2, 3] and (outs[0][4:] == 7).all()
    with pytest.raises(pkg.TtsError):
        pkg.host_ar_score_rows(codes, "sideways")


def test_refusals_on_a_host_only_context(pkg):
    e = pkg.Engine(-1)
    L, h = e.L, e.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ids, voice, codes, n = np.array([1, 2, 3], np.int32), np.zeros(1024, np.float32), np.zeros((1, 8), np.int32), np.array([8], np.int32)
    outs = [np.full(9, 7, dt) for dt in (np.float32, np.float32, np.int32, np.float32)]
    for pos in (0, 1, 5):  # the device is asked for first, as every stage call does
        assert L.tts_ar_score_codes(h, p(ids), 3, p(voice), p(codes), p(n), 1, 8, pos, *[p(o) for o in outs]) == HIP
        assert "host-only" in L.tts_last_error(h).decode()
    assert L.tts_ar_score_codes(None, p(ids), 3, p(voice), p(codes), p(n), 1, 8, 0, *[p(o) for o in outs]) == ARG
    assert all((o == 7).all() for o in outs), "a refused call wrote its output"
    with pytest.raises(pkg.TtsError):
        e.ar_score_codes(ids, voice, [codes[0]], "sideways")
    e.close()


def test_header_exports_and_bindings(pkg):
    names = pkg.header_symbols()
    for n in ("tts_ar_score_codes", "tts_host_ar_score_rows"):
        assert n in names and hasattr(pkg.lib(), n), n
    assert hasattr(pkg.Engine, "ar_score_codes") and hasattr(pkg, "host_ar_score_rows")
    txt = open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read()
    assert "#define TTS_SCORE_POS_DECODE 0" in txt and "#define TTS_SCORE_POS_TRAIN 1" in txt
    assert pkg.SCORE_POSITIONS == {"decode": 0, "train": 1}


# ---- the harness validates a case completely before any HIP call ----
def test_harness_constants_and_valid_cases():
    L = A.harness()
    assert L.tts_score_test_tile() == R.TILE and L.tts_score_test_slab() == R.SLAB and L.tts_score_test_margin() == 4096
    assert 0 < L.tts_score_test_lds(1024) <= 160 * 1024 and L.tts_score_test_lds(64) < L.tts_score_test_lds(1024) and L.tts_score_test_lds(0) == -1
    full = A.full_case()
    for c in [A.small_case(), A.tail_tie_case(), A.extreme_case(A.SMALL), A.extreme_case(A.FULL)] + [full.first(n) for n in A.FULL_ROWS]:
        assert c.validate() == 0, c.label
    assert L.tts_score_test_validate(None) == A.HIP_INVALID_VALUE and L.tts_score_test_run(None) == A.HIP_INVALID_VALUE


@pytest.mark.parametrize("name,override", A.invalid_overrides(), ids=[n for n, _ in A.invalid_overrides()])
def test_harness_refuses_an_invalid_case_before_any_hip_call(name, override):
    c = A.small_case()
    assert c.validate(**override) == A.HIP_INVALID_VALUE
    dummy = np.zeros(8, np.uint8)
    assert A.harness().tts_score_test_run(C.byref(c.struct([dummy] * 6, **override))) == A.HIP_INVALID_VALUE  # (no GPU here: a HIP call would give another status)
    assert (dummy == 0).all()


# ---- the CLI's usage errors: exit 1 with a usage message, before a model is loaded ----
def _wav(pkg, path, seconds, rate=22050):
    n = int(seconds * rate)
    x = (0.1 * np.sin(np.arange(n) * 0.05)).astype(np.float32)
    assert pkg.lib().tts_write_wav(str(path).encode(), x, n, rate) == 0
    return str(path)


CLI_ERRORS = [(["--score-audio", "IN"], "--score-audio needs --dvae"), (["--score-audio", "IN", "--dvae", "d.bin", "--score-codes", "CODES"], "cannot be combined"),
              (["--score-positions", "train"], "--score-positions needs --score-audio or --score-codes"),
              (["--score-codes", "CODES", "--score-positions", "sideways"], "--score-positions sideways: decode or train"),
              (["--score-codes", "CODES", "--dry-run", "1"], "cannot be combined with --dry-run 1"),
              (["--score-codes", "CODES", "--split-text", "100"], "cannot be combined with --split-text"),
              (["--score-codes", "CODES", "--stream", "--decoder", "hifigan"], "cannot be combined with --stream"),
              (["--score-codes", "CODES", "--voice", "a.bin", "--voice", "b.bin"], "cannot be combined with several voices"),
              (["--score-codes", "CODES", "--devices", "2"], "--devices > 1 or --exchange rccl"),
              (["--score-audio", "IN", "--dvae", "d.bin", "--revoice", "IN"], "cannot be combined with --revoice"),
              (["--score-codes", "CODES", "--message", ""], "need --message"),
              (["--score-audio", "LONG", "--dvae", "d.bin"], "codes, at most 500"), (["--score-audio", "nowhere.wav", "--dvae", "d.bin"], "not a readable RIFF WAV"),
              (["--score-audio", ",", "--dvae", "d.bin"], "no clip given"),
              (["--score-codes", "nowhere.txt"], "cannot be opened"), (["--score-codes", "EMPTY"], "no codes"), (["--score-codes", "BADCODE"], "code 8192 (0 .. 8191)"),
              (["--score-codes", "WORDS"], "1 .. 500 space-separated codes"), (["--score-codes", "TOOLONG"], "1 .. 500 space-separated codes"),
              (["--score-codes", "MANY"], "at most 64 in one call")]


@pytest.mark.parametrize("extra,what", CLI_ERRORS, ids=[" ".join(e) for e, _ in CLI_ERRORS])
def test_cli_usage_errors(pkg, tmp_path, extra, what):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    files = {"CODES": "1 2 3\n4 5\n", "EMPTY": "\n \n", "BADCODE": "1 8192 3\n", "WORDS": "1 two 3\n", "TOOLONG": " ".join(["7"] * 501) + "\n", "MANY": "1 2\n" * 65}
    names = {"IN": _wav(pkg, tmp_path / "in.wav", 1.0), "LONG": _wav(pkg, tmp_path / "long.wav", 24.0)}  # 24 s: 517 codes
    for k, v in files.items():
        open(tmp_path / (k + ".txt"), "w").write(v)
        names[k] = str(tmp_path / (k + ".txt"))
    extra = [names.get(e, e) for e in extra]
    r = subprocess.run([exe, "--models", str(tmp_path / "nowhere"), "--message", "hello there", "--output", str(tmp_path / "o.wav")] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and what in r.stderr, r.stderr
    assert ("usage:" in r.stderr or "not a readable" in r.stderr) and "model_load" not in r.stderr and "score:" not in r.stdout  # before a model is loaded


# ---- the condition tests/test_ar_score_gpu.py relies on, on the oracle alone ----
def test_the_two_position_modes_differ_by_more_than_the_gate_on_the_oracle(oracle, small_models, voice):
    path, cands = small_models + "/ggml-model.bin", R.candidates()
    dec = R.oracle_decode_logits(oracle, path, DEFAULT_TOKENS, voice, cands)
    trn = R.oracle_train_logits(oracle, path, DEFAULT_TOKENS, voice, cands)
    gate = 2.0 * R.DECODE_GATE * float(np.abs(dec).max())
    a, b = R.log_softmax64(dec), R.log_softmax64(trn)
    for i, c in enumerate(cands):
        n = len(c)
        t = np.concatenate([c, [8193]])
        rows = np.arange(n + 1)
        assert abs(a[i, 0, t[0]] - b[i, 0, t[0]]) <= gate  # row 0 sits at position 0 in both modes
        d = np.abs(a[i, rows, t] - b[i, rows, t])[1:]
        print("%d codes: the modes' log-probs differ by %.3f at most (gate %.2e)" % (n, d.max(), gate))
        assert d.max() > gate
        # and the round trip's margin condition leaves rows to compare
        top2 = np.sort(dec[i, :n + 1].astype(np.float64), axis=1)[:, -2:]
        assert (top2[:, 1] - top2[:, 0] > 2.0 * gate).mean() >= 0.5
