"""CPU: what the device sampler (option ar_sampler = 1) can be held to without a GPU: its uniform against the Philox known-answer restatement, the undecided share
of the reference rule on every input the GPU test uses, every refusal a host-only context reaches, the CLI's usage errors."""
import os
import subprocess

import numpy as np
import pytest

import sample_device_ref as R
from voc_cases import philox4x32_10_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_HIP = -1, -4


def test_host_ar_uniform_is_philox_under_its_own_tag(pkg):
    seen = set()
    for seed, cand, it in [(0, 0, 0), (7, 3, 11), (0xFFFFFFFF, 1 << 20, 499), (0x123456789ABCDEF, 5, 2), (7, 4, 11), (7, 3, 12), (8, 3, 11)]:
        u = pkg.host_ar_uniform(seed, cand, it)
        word = philox4x32_10_int([0, it, cand, 0x7718], [seed & 0xFFFFFFFF, seed >> 32])[0]
        assert u == (word >> 8) * 2.0 ** -24 and 0.0 <= u < 1.0
        seen.add(u)
    assert len(seen) == 7  # another candidate, iteration or seed: another uniform


@pytest.mark.parametrize("case", range(len(R.planted_cases())))
def test_reference_decides_the_planted_draws(pkg, case):
    """At most 2 % of a case's draws may lie within tol(n) of a cumulative value: the GPU test compares the others id for id."""
    n, top_k, top_p, temperature, _, mask = R.planted_cases()[case]
    rows, ids = R.planted_inputs(case)
    res = [R.sample_ref(rows[b], ids[b], pkg.host_ar_uniform(R.SEED, b, it), temperature, top_k, top_p, 2.0, mask) for b in range(n) for it in range(R.ITERATIONS)]
    assert all(r is not None for r in res)
    assert sum(not r[1] for r in res) <= 0.02 * len(res)


def test_refusals_on_a_host_only_context(pkg):
    eng = pkg.Engine(-1)
    L, h = eng.L, eng.h
    for key, bad in [("ar_sampler", 2), ("ar_sampler", -1), ("ar_sampler", 0.5), ("ar_sync_steps", 0), ("ar_sync_steps", 65), ("ar_sync_steps", 1.5)]:
        assert L.tts_set_option(h, key.encode(), float(bad)) == ERR_ARG, (key, bad)
    for key, ok in [("ar_sampler", 1), ("ar_sync_steps", 64), ("ar_sync_steps", 1), ("ar_sampler", 0)]:
        assert L.tts_set_option(h, key.encode(), float(ok)) == 0
    rows, ids, out = np.zeros((1, R.V), np.float32), np.array([[1]], np.int32), np.full(1, -7, np.int32)
    call = lambda lg=rows, i=ids, o=out, n=1, k=1, it=0, c0=0, fl=0: L.tts_sample_device(h, lg.ctypes.data if lg is not None else None, n, i.ctypes.data if i is not None else None, k, it, c0, fl, o.ctypes.data if o is not None else None)
    assert call(lg=None) == call(i=None) == call(o=None) == call(n=0) == call(k=0) == call(it=-1) == call(c0=-1) == call(fl=2) == ERR_ARG
    assert call(i=np.array([[R.V]], np.int32)) == ERR_ARG
    eng.set_option("ar_typical_mass", 0.2)
    assert call() == ERR_ARG and b"typical" in L.tts_last_error(h)
    eng.set_option("ar_typical_mass", 0)
    eng.set_option("ar_top_k", 513)
    assert call() == ERR_ARG and b"512" in L.tts_last_error(h)
    eng.set_option("ar_top_k", 512)
    assert call() == ERR_HIP and out[0] == -7  # every check passed: the host-only context has no device, and nothing was written
    eng.close()


def test_cli_usage_errors(tmp_path):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    assert os.path.exists(exe), "CLI binary not built"
    models = os.path.join(ROOT, "models")
    base = [exe, "--dry-run", "1", "--models", models, "--voice", os.path.join(models, "mol.bin"), "--seed", "11", "--codes", "5", "--output", str(tmp_path / "o.wav"),
            "--timing", "1"]
    for bad in (["--ar-sampler", "gpu"], ["--ar-sampler", "device", "--ar-sync-steps", "0"], ["--ar-sampler", "device", "--ar-sync-steps", "65"],
                ["--ar-sync-steps", "4"], ["--ar-sampler", "device", "--typical-mass", "0.2"], ["--ar-sampler", "device", "--top-k", "513"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--ar-s" in r.stderr and "[timing]" not in r.stderr, (bad, r.stderr)
    r = subprocess.run(base + ["--ar-sampler", "device", "--ar-sync-steps", "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "penalty-scope last, ar-sampler device, ar-sync-steps 8\n" in r.stderr, r.stdout + r.stderr
