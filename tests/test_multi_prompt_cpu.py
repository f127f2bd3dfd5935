"""CPU: the host logic of several prompts in one autoregressive pass (tts_autoregressive_multi). Random-init weights never sample the stop token, so the
per-group stop rule is driven here with scripted samples through tts_host_ar_stop_run, which runs the driver's own bookkeeping (host_logic.cpp: ArStopBook).
Also: the padded step-0 penalty rows the driver feeds the sampler penalise exactly what each group's own prompt-shaped row does."""
import numpy as np
import pytest

STOP = 8193


def script(B, steps, events):
    """samples [steps, B]: 100 + b + i (never a stop token) except events {(i, b): id}"""
    s = np.array([[100 + b + i for b in range(B)] for i in range(steps)], np.int32)
    for (i, b), v in events.items():
        s[i, b] = v
    return s


def test_group_ends_while_others_continue_and_frozen_sequences(pkg):
    n_cand = [2, 1, 2]  # candidates 0-1 | 2 | 3-4
    steps = 10
    s = script(5, steps, {
        (1, 0): STOP, (2, 0): 55, (4, 0): STOP, (4, 1): STOP,  # group 0: candidate 0 stops at 1, samples on, group ends at 4
        (2, 2): STOP,                                          # group 1 ends at 2
        (3, 3): STOP, (6, 3): STOP, (6, 4): STOP,              # group 2 ends at 6
    })
    rc, codes, stopped, n, inputs = pkg.host_ar_stop_run(n_cand, s, steps)
    assert rc == 0 and n == 7
    assert list(stopped) == [1] * 5
    # candidate 0: frozen at its first stop token (strict mode), later samples are not part of its sequence
    assert list(codes[0, :4]) == [8192, s[0, 0], STOP, 83]
    assert list(codes[1, 1:7]) == [s[0, 1], s[1, 1], s[2, 1], s[3, 1], STOP, 83]
    assert list(codes[2, 1:5]) == [s[0, 2], s[1, 2], STOP, 83]
    assert list(codes[3, 1:6]) == [s[0, 3], s[1, 3], s[2, 3], STOP, 83]
    # inputs of the next decode step: a candidate of a running group is fed what it sampled (also after its own stop token: the reference's strict rule),
    # an ended group's rows are fed 8193 whatever they sample
    assert inputs[2, 0] == 55 and inputs[3, 0] == s[3, 0]
    assert inputs[2, 2] == STOP and (inputs[3:7, 2] == STOP).all()
    assert (inputs[5:7, 0:2] == STOP).all()
    assert inputs[5, 3] == s[5, 3] and inputs[5, 4] == s[5, 4]


def test_strict_mode_fails_at_max_steps_and_masked_runs_are_cut(pkg):
    s = script(3, 6, {(1, 0): STOP, (2, 1): STOP})  # groups [1, 2]: group 0 ends at 1, group 1 never (candidate 2 does not stop)
    rc, codes, stopped, n, _ = pkg.host_ar_stop_run([1, 2], s, 6)
    assert rc == -6 and n == 6  # TTS_ERR_LIMIT
    rc, codes, stopped, n, _ = pkg.host_ar_stop_run([1, 2], s, 6, flags=pkg.AR_MASK_STOP)
    assert rc == 0 and n == 6 and list(stopped) == [1, 1, 0]
    assert list(codes[2, 1:7]) == list(s[:, 2]) and codes[2, 7] == 83


def test_one_group_is_the_single_prompt_rule(pkg):
    """G = 1: the loop of tts_autoregressive (ends only in an iteration where ALL candidates sample 8193), restated here."""
    rs = np.random.RandomState(5)
    for trial in range(40):
        B, steps = int(rs.randint(1, 6)), int(rs.randint(2, 12))
        s = np.where(rs.rand(steps, B) < 0.45, STOP, rs.randint(0, 8192, (steps, B))).astype(np.int32)
        seq, n, end = [[] for _ in range(B)], 0, False
        for i in range(steps):
            for b in range(B):
                if not (seq[b] and seq[b][-1] == STOP):
                    seq[b].append(int(s[i, b]))
            n += 1
            if (s[i] == STOP).all():
                end = True
                break
        rc, codes, stopped, got_n, _ = pkg.host_ar_stop_run([B], s, steps)
        assert rc == (0 if end else -6) and got_n == n
        if end:
            for b in range(B):
                assert list(codes[b, 1:1 + len(seq[b])]) == seq[b]


def test_retire_mode_with_a_schedule_uses_global_indices(pkg):
    flags = pkg.AR_MASK_STOP | pkg.AR_RETIRE
    s = script(4, 8, {})
    rc, codes, stopped, n, inputs = pkg.host_ar_stop_run([1, 3], s, 8, flags, stop_at=[2, 5, 3, 9])
    assert rc == 0 and n == 8  # candidate 3 is cut at max_steps
    assert list(stopped) == [1, 1, 1, 0]
    for b, k in enumerate([2, 5, 3]):
        assert list(codes[b, 1:2 + k]) == list(s[:k, b]) + [STOP]
        assert (inputs[k:, b] == STOP).all()


def test_padded_step0_penalty_rows_are_the_groups_own(pkg):
    """The driver pads every step-0 penalty row ([1, .., 1, 8192]) to the longest prompt's length with more 1s: the sampler penalises each DISTINCT id
    once, so the padded row samples what the group's own row samples — on the fast path and on the literal (tie) path."""
    rs = np.random.RandomState(17)
    for trial in range(200):
        row = rs.randn(8194).astype(np.float32) * 3
        if trial % 2:  # ties among the survivors force the literal formulation
            row = np.round(row, 1).astype(np.float32)
        row[1] = rs.randn() * 4
        row[8192] = rs.randn() * 4
        p_own, p_pad = int(rs.randint(3, 50)), 406
        own = np.array([1] * (p_own - 1) + [8192], np.int32)
        pad = np.array([1] * (p_pad - 1) + [8192], np.int32)
        u = float(rs.rand())
        assert pkg.host_sample_row(row, own, u) == pkg.host_sample_row(row, pad, u)
