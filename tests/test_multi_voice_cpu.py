"""CPU: the host side of several voices in one batch (API version 8). tts_split_turns on a host-only context (device = -1, tokenizer loaded) — the rule is the
project's own (include/tortoise_mi355x.h): turns are lines, "<decimal index>|" in front of a turn names its voice and is not text, a turn without it keeps
the voice of the turn before (the first: voice 0), every turn is split by the tts_split_text rule, empty turns give no chunk, an index >= n_voices is
TTS_ERR_ARG — and the CLI's plumbing under --dry-run 1 (repeated --voice / --diffusion-latent, usage errors before any model is loaded)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import MODELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")


@pytest.fixture(scope="module")
def host(pkg):
    L = pkg.lib()
    h = L.tts_create(-1)
    assert h
    eng = pkg.Engine.__new__(pkg.Engine)
    eng.L, eng.h = L, h
    eng.tokenizer_load(os.path.join(MODELS, "tokenizer.json"))
    yield eng
    eng.close()


def raw_turns(host, msg, n_voices, max_ids):
    """(start, length, voice) byte ranges as the C call returns them"""
    raw = msg.encode("utf-8")
    cap = len(raw) + 1
    st, ln, vo = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int32)
    n = host.L.tts_split_turns(host.h, raw, n_voices, max_ids, st, ln, vo, cap)
    assert n >= 0, n
    return [(int(st[k]), int(ln[k]), int(vo[k])) for k in range(n)]


def test_version_and_exports(pkg):
    L = pkg.lib()
    assert L.tts_version() == 8
    syms = pkg.header_symbols()
    for s in ("tts_ar_begin_multi_voice", "tts_autoregressive_multi_voice", "tts_diffusion_multi_voice", "tts_split_turns"):
        assert s in syms and hasattr(L, s), s
    assert "#define TTS_API_VERSION 8" in open(pkg.HEADER).read()


def test_prefixes_inheritance_and_default(host):
    msg = "hello there.\n1|how are you?\ni am fine!\n0|good.\n2|bye."
    assert host.split_turns(msg, 3, 404) == [("hello there.", 0), ("how are you?", 1), ("i am fine!", 1), ("good.", 0), ("bye.", 2)]
    # blanks in front of the digits, several digits, blanks after the bar
    assert host.split_turns("  11| eleven speaks.\nstill eleven.", 12, 404) == [("eleven speaks.", 11), ("still eleven.", 11)]
    # no bar, or no digits in front of it: text
    assert host.split_turns("1 is a number.\n|a bar.", 2, 404) == [("1 is a number.", 0), ("|a bar.", 0)]
    # only the start of a turn is a prefix
    assert host.split_turns("1|one says 0|zero.", 2, 404) == [("one says 0|zero.", 1)]


def test_empty_turns_give_no_chunk(host):
    assert host.split_turns("", 2, 404) == []
    assert host.split_turns("\n\n  \n", 2, 404) == []
    assert host.split_turns("\n\n1|\n\nlate start.\n\n0|   \nback to zero.\n", 2, 404) == [("late start.", 1), ("back to zero.", 0)]
    assert host.split_turns("one.\r\n1|two.\r\n", 2, 404) == [("one.", 0), ("two.", 1)]  # a carriage return is whitespace


def test_byte_ranges_exclude_the_prefix_and_chunks_fit(host):
    a, b, c = "hello there.", "how are you?", "i am fine!"
    m = len(host.tokenize(a + " " + b))
    assert m < len(host.tokenize(" ".join([a, b, c])))
    msg = "1|" + " ".join([a, b, c]) + "\n" + "0|short.\n" + "12|" + "abcdefghij" * 20
    raw = msg.encode("utf-8")
    got = raw_turns(host, msg, 13, m)
    texts = [raw[s:s + n].decode("utf-8") for s, n, _ in got]
    assert texts[:3] == [a + " " + b, c, "short."] and [v for _, _, v in got[:3]] == [1, 1, 0]  # max_ids splits inside a turn, never across turns
    assert len(got) > 4 and all(v == 12 for _, _, v in got[3:]) and "".join(texts[3:]) == "abcdefghij" * 20  # a hard-cut turn
    for (s, n, _), t in zip(got, texts):
        assert n > 0 and "|" not in t and t == t.strip()
        assert len(host.tokenize(t)) <= m, (t, m)
    assert got[0][0] == 2 and got[2][0] == raw.index(b"short.")
    starts = [s for s, _, _ in got]
    assert starts == sorted(starts) and all(s0 + n0 <= s1 for (s0, n0, _), s1 in zip(got, starts[1:]))
    # the Python wrapper returns the same chunks
    assert host.split_turns(msg, 13, m) == [(t, v) for t, (_, _, v) in zip(texts, got)]


def test_voice_index_out_of_range_and_bad_arguments(host, pkg):
    L, cap = host.L, 8
    st, ln, vo = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    assert L.tts_split_turns(host.h, b"0|fine.\n2|too far.", 2, 404, st, ln, vo, cap) == -1
    assert b"voice 2 of 2" in L.tts_last_error(host.h)
    assert L.tts_split_turns(host.h, b"99999999999999999999|far too far.", 2, 404, st, ln, vo, cap) == -1
    assert L.tts_split_turns(host.h, b"1|fine.", 2, 404, st, ln, vo, cap) == 1
    assert L.tts_split_turns(host.h, b"fine.", 0, 404, st, ln, vo, cap) == -1  # n_voices < 1
    for m in (2, 405):
        assert L.tts_split_turns(host.h, b"fine.", 2, m, st, ln, vo, cap) == -1
    with pytest.raises(pkg.TtsError, match="status -1"):
        host.split_turns("3|x.", 3, 404)
    h = L.tts_create(-1)
    try:  # no tokenizer loaded
        assert L.tts_split_turns(h, b"a.", 1, 50, st, ln, vo, cap) == -5
    finally:
        L.tts_destroy(h)
    # only the first `cap` chunks are written, the count is the full one
    st[:] = -7
    assert L.tts_split_turns(host.h, b"a.\nb.\nc.", 1, 404, st, ln, vo, 2) == 3 and list(st[:3]) == [0, 3, -7]


def test_without_newline_and_prefix_it_is_split_text(host):
    rs = np.random.RandomState(99)
    alphabet = list("abcdefghijklmnopqrstuvwxyz") * 3 + [" "] * 12 + list(".,!?;:'-") + ["  "]
    for trial in range(40):
        msg = "".join(rs.choice(alphabet, int(rs.randint(0, 300))))
        if msg.lstrip(" \t")[:1].isdigit():
            msg = "x" + msg
        max_ids = int(rs.randint(3, 80))
        assert host.split_turns(msg, 1, max_ids) == [(c, 0) for c in host.split_text(msg, max_ids)], (msg, max_ids)


# ---- the command line under --dry-run 1 -----------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def files(tmp_path):
    rs = np.random.RandomState(5)
    out = {}
    for name, n in (("v0", 1024), ("v1", 1024), ("d0", 2048), ("d1", 2048)):
        p = tmp_path / (name + ".bin")
        rs.randn(n).astype(np.float32).tofile(str(p))
        out[name] = str(p)
    out["wav"] = str(tmp_path / "out.wav")
    return out


def cli(args):
    assert os.path.exists(EXE), "the CLI is not built (__graft_entry__.build())"
    return subprocess.run([EXE, "--dry-run", "1", "--models", MODELS, "--seed", "11", "--codes", "9"] + args, capture_output=True, text=True, timeout=120)


MSG = "1|hello there, how are you?\n0|i am fine. thank you for asking!\nand you?"


def test_cli_dry_run_prints_the_chunks_and_their_voices(host, files):
    r = cli(["--message", MSG, "--voice", files["v0"], "--voice", files["v1"], "--output", files["wav"]])
    assert r.returncode == 0, r.stdout + r.stderr
    n = [len(host.tokenize(t)) for t in ("hello there, how are you?", "i am fine. thank you for asking!", "and you?")]
    assert r.stdout.splitlines() == ["chunk 0: voice 1, %d text ids" % n[0], "chunk 1: voice 0, %d text ids" % n[1], "chunk 2: voice 0, %d text ids" % n[2]]
    assert not os.path.exists(files["wav"])
    # one latent per voice is fine too; --split-text N is the ids per chunk inside a turn
    r2 = cli(["--message", MSG, "--voice", files["v0"], "--diffusion-latent", files["d0"], "--voice", files["v1"], "--diffusion-latent", files["d1"],
              "--output", files["wav"]])
    assert r2.returncode == 0 and r2.stdout == r.stdout, r2.stdout + r2.stderr
    m = len(host.tokenize("i am fine."))
    r3 = cli(["--message", MSG, "--voice", files["v0"], "--voice", files["v1"], "--split-text", str(max(m, n[2])), "--output", files["wav"]])
    assert r3.returncode == 0, r3.stdout + r3.stderr
    voices = [int(l.split()[3].rstrip(",")) for l in r3.stdout.splitlines()]
    assert len(voices) > 3 and voices[0] == 1 and voices[-1] == 0 and sorted(voices, reverse=True) == voices
    # a turn that names a voice that was not given
    r4 = cli(["--message", "2|nobody.", "--voice", files["v0"], "--voice", files["v1"], "--output", files["wav"]])
    assert r4.returncode == 1 and "voice 2 of 2" in r4.stderr


def test_cli_usage_errors_before_any_model(files):
    two = ["--message", MSG, "--voice", files["v0"], "--voice", files["v1"], "--output", files["wav"]]
    r = cli(two + ["--diffusion-latent", files["d0"]])  # one latent for two voices
    assert r.returncode == 1 and "--diffusion-latent" in r.stderr and r.stdout == ""
    r = cli(["--message", MSG, "--voice", files["v0"], "--diffusion-latent", files["d0"], "--diffusion-latent", files["d1"], "--output", files["wav"]])
    assert r.returncode == 1 and "--diffusion-latent" in r.stderr and r.stdout == ""
    r = cli(two + ["--candidates", "2", "--devices", "2"])
    assert r.returncode == 1 and "--voice" in r.stderr and "--devices" in r.stderr and r.stdout == ""
    r = cli(two[:-2] + ["--voice", os.path.join(os.path.dirname(files["v0"]), "missing.bin"), "--output", files["wav"]])
    assert r.returncode == 1 and "missing.bin" in r.stderr
    assert not os.path.exists(files["wav"])


def test_cli_one_voice_is_unchanged(files):
    """One --voice (with or without one --diffusion-latent): the dry run of the parent commit — the host sampler's stand-in, one WAV per candidate, this stdout."""
    base = ["--message", "0|not a dialogue: one voice.\nstill one prompt.", "--candidates", "2", "--output", files["wav"]]
    r = cli(base + ["--voice", files["v0"]])
    assert r.returncode == 0 and r.stdout == "WAV file saved successfully. :^)\n", r.stdout + r.stderr
    a = (open(files["wav"], "rb").read(), open(files["wav"] + ".1.wav", "rb").read())
    r = cli(base + ["--voice", files["v0"], "--diffusion-latent", files["d0"]])
    assert r.returncode == 0 and r.stdout == "WAV file saved successfully. :^)\n", r.stdout + r.stderr
    r = cli(base + ["--voice", files["v0"], "--clvp", "unused-in-dry-run"])
    assert r.returncode == 0 and r.stdout.startswith("clvp: candidate ") and r.stdout.endswith("WAV file saved successfully. :^)\n"), r.stdout + r.stderr
    r = cli(base + ["--voice", files["v1"]])  # the dry run's stand-in does not read the voice: same seed, same files
    assert r.returncode == 0 and a == (open(files["wav"], "rb").read(), open(files["wav"] + ".1.wav", "rb").read())
