"""Shared by the harness CPU tests of the models that load through csrc/model_io.h (HiFi-GAN, BigVGAN, classifier, aligner, DVAE): the one shape of
ModelReader's messages, and an independent numpy spelling of the per-level HFG_SEQ tables (level_table) that each model's *_levels function is held to."""
import re

import numpy as np

SEQ = 9
MISSING = r"^tensor '%s' missing from %s model file$"
SHAPE = r"^tensor '%s' has wrong shape in %s model file: got \[(\d+), (\d+), (\d+)\] \((\d) dims\), expected \[(\d+), (\d+), (\d+)\]$"
UNKNOWN = r"^unknown tensors in %s model file '.*' \((\d+) tensors, (\d+) expected\)$"


def reader_messages(load, tensors, model, vec, fmt, unknown=True, extent=True):
    """load(tensors) -> (status, message) runs the model's parser on a file with these tensors. vec names a vector the parser reads with ModelReader::need only.
    One case each: the tensor missing, of another rank, of another extent, and a tensor nobody asks for; every model answers in the same words."""
    n = len(tensors[vec])
    name = re.escape(vec)

    def run(edit):
        t = dict(tensors)
        edit(t)
        rc, msg = load(t)
        assert rc == fmt, (rc, msg)
        return msg

    msg = run(lambda t: t.pop(vec))
    assert re.match(MISSING % (name, model), msg), msg
    m = re.match(SHAPE % (name, model), run(lambda t: t.__setitem__(vec, np.zeros((n, 1), np.float32))))
    assert m and [int(v) for v in m.groups()][:2] == [1, n] and m.group(4) == "2" and [int(v) for v in m.groups()[4:]] == [n, 1, 1], m
    if extent:
        m = re.match(SHAPE % (name, model), run(lambda t: t.__setitem__(vec, np.zeros(n + 1, np.float32))))
        assert m and int(m.group(1)) == n + 1 and m.group(4) == "1" and [int(v) for v in m.groups()[4:]] == [n, 1, 1], m
    if unknown:
        m = re.match(UNKNOWN % model, run(lambda t: t.__setitem__(vec + ".extra", np.zeros(3, np.float32))))
        assert m and (int(m.group(1)), int(m.group(2))) == (len(tensors) + 1, len(tensors)), m


def levels(n0, nxt, L, align, tile, every_level, unit=1):
    """Level l's record of clip s: {first row, rows, 0, first tile, unit x the clip's first row on level 0}; ints 3 and 4 on level 0 only unless every_level.
    Written level by level from cumulative sums, not clip by clip as the C++ walks: (tab [L][B][9], rows [L], tiles [L], max_n [L])"""
    n = [np.asarray(n0, np.int64)]
    for l in range(L - 1):
        n.append(np.array([nxt(int(v), l) for v in n[-1]], np.int64))
    n = np.stack(n)
    pad = (n + align - 1) // align * align
    first = np.cumsum(pad, axis=1) - pad
    t = (n + tile - 1) // tile if tile else np.zeros_like(n)
    first_t = np.cumsum(t, axis=1) - t
    tab = np.zeros((L, len(n0), SEQ), np.int32)
    tab[:, :, 0], tab[:, :, 1] = first, n
    keep = slice(None) if every_level else slice(0, 1)
    tab[keep, :, 3] = first_t[keep]
    tab[keep, :, 4] = unit * first[0]
    return tab, pad.sum(axis=1), t.sum(axis=1), n.max(axis=1)
