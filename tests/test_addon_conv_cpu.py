"""CPU: option addon_conv_precision on a host-only context (0, 1 and 2 are stored; anything else is TTS_ERR_ARG) and the CLI's --addon-conv-precision usage error."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_option_values(pkg):
    e = pkg.Engine(-1)
    for v in (0, 1, 2, 0):
        e.set_option("addon_conv_precision", v)
    for bad in (3, -1, 0.5, float("nan")):
        assert e.L.tts_set_option(e.h, b"addon_conv_precision", float(bad)) == -1 and b"addon_conv_precision" in e.L.tts_last_error(e.h)
        with pytest.raises(pkg.TtsError, match="addon_conv_precision"):
            e.set_option("addon_conv_precision", bad)
    e.close()

def test_cli_refuses_another_name_before_any_model_is_loaded():
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    r = subprocess.run([exe, "--models", "/nonexistent", "--addon-conv-precision", "bogus"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--addon-conv-precision bogus: f32, f16 or split" in r.stderr
