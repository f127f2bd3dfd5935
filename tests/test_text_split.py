"""CPU: tts_split_text, the splitter behind `tortoise --split-text N` (host only: a device = -1 context with the tokenizer loaded). The rule is the
project's own (include/tortoise_mi355x.h): sentences end after '.', '!' or '?' followed by whitespace or the end; whole sentences are packed greedily while
the chunk tokenizes to <= max_ids ids; a sentence that does not fit alone is cut after the last ',', ';', ':' or whitespace at which the piece fits, else
hard-cut; chunks are trimmed and never empty."""
import os
import re

import numpy as np
import pytest

from conftest import MODELS


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


def n_ids(host, text):
    return len(host.tokenize(text))


def squash(s):
    return re.sub(r"\s+", "", s)


def check_invariants(host, msg, max_ids, chunks):
    for c in chunks:
        assert c and c == c.strip(), (msg, chunks)
        assert n_ids(host, c) <= max_ids, (c, n_ids(host, c), max_ids)
    assert squash("".join(chunks)) == squash(msg), (msg, chunks)
    pos = 0
    for c in chunks:  # in order, each a substring of the message
        k = msg.find(c, pos)
        assert k >= pos, (msg, chunks)
        pos = k + len(c)


def test_one_chunk_when_the_message_fits(host):
    msg = "hello there. how are you? i am fine!"
    assert host.split_text(msg, 404) == [msg]
    assert host.split_text("  " + msg + "  ", 404) == [msg]


def test_sentences_are_packed_greedily(host):
    a, b, c = "hello there.", "how are you?", "i am fine!"
    msg = " ".join([a, b, c])
    m = n_ids(host, a + " " + b)
    assert m < n_ids(host, msg)
    assert host.split_text(msg, m) == [a + " " + b, c]
    assert host.split_text(msg, n_ids(host, b)) == [a, b, c]  # no two sentences fit together
    # a sentence end needs whitespace (or the end) after the mark: "mr.smith" does not split
    msg2 = "mr.smith is here today. it is."
    assert host.split_text(msg2, n_ids(host, "mr.smith is here today.")) == ["mr.smith is here today.", "it is."]


def test_over_long_sentence_is_cut_at_the_last_break_that_fits(host):
    head, tail = "one two three, four five six;", "seven eight nine: ten"
    msg = head + " " + tail + "."
    m = n_ids(host, head)
    assert n_ids(host, tail + ".") <= m < n_ids(host, msg)
    assert host.split_text(msg, m) == [head, tail + "."]
    # one id less: the cut moves back to the space before "six;"
    got = host.split_text(msg, m - 1)
    assert got[0] == "one two three, four five"
    check_invariants(host, msg, m - 1, got)


def test_no_punctuation_no_spaces_is_hard_cut(host):
    msg = "abcdefghij" * 30
    got = host.split_text(msg, 20)
    assert len(got) > 1 and "".join(got) == msg
    check_invariants(host, msg, 20, got)
    # a chunk is the longest prefix that fits: one more character would not
    assert n_ids(host, got[0] + msg[len(got[0])]) > 20


def test_whitespace_trailing_multiple_and_empty(host):
    msg = "  first one.   second one.  \t "
    assert host.split_text(msg, 404) == ["first one.   second one."]
    assert host.split_text(msg, n_ids(host, "second one.")) == ["first one.", "second one."]
    assert host.split_text("", 50) == []
    assert host.split_text("   \t  ", 50) == []


def test_bad_arguments(host, pkg):
    for m in (2, 405):
        with pytest.raises(pkg.TtsError, match="max_ids"):
            host.split_text("a b c.", m)
    L = pkg.lib()
    h = L.tts_create(-1)
    try:  # no tokenizer loaded
        assert L.tts_split_text(h, b"a.", 50, np.zeros(4, np.int32), np.zeros(4, np.int32), 4) == -5
    finally:
        L.tts_destroy(h)


def test_random_text_property(host):
    rs = np.random.RandomState(2024)
    alphabet = list("abcdefghijklmnopqrstuvwxyz") * 3 + [" "] * 12 + list(".,!?;:'-") + ["  "]
    for trial in range(60):
        n = int(rs.randint(0, 400))
        msg = "".join(rs.choice(alphabet, n))
        max_ids = int(rs.randint(3, 80))
        got = host.split_text(msg, max_ids)
        check_invariants(host, msg, max_ids, got)
        if msg.strip() and n_ids(host, msg.strip()) <= max_ids:
            assert got == [msg.strip()], (msg, max_ids, got)
