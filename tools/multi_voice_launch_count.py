"""Developer tool: ONE diffusion call of 3 candidates x 8 steps on the mid-size synthetic weights, for `rocprofv3 --kernel-trace --stats` (graphs off so that
every kernel is traced):

    TTS_NO_GRAPH=1 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/plain  -o p -- python tools/multi_voice_launch_count.py plain
    TTS_NO_GRAPH=1 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/voices -o v -- python tools/multi_voice_launch_count.py voices

`plain` calls tts_diffusion, `voices` calls tts_diffusion_multi_voice with ONE voice (the model's own latent) for all candidates: the two traces must hold the
same number of kernel launches (the voice table adds an upload, not a launch) — profiles/multi_voice_launch_count.txt — and the two calls return the same bits
(printed as a checksum)."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

pkg = tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd import synth_weights as sw  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "plain"
d = os.path.join(os.environ.get("TTS_SYNTH_DIR", "/tmp/tts_synth"), "mid_diffusion_only")
path = os.path.join(d, "ggml-diffusion-model.bin")
if not os.path.exists(os.path.join(d, ".done")):
    os.makedirs(d, exist_ok=True)
    sw.write_diffusion(path, 3, 1, 1, 2, seed=777)
    open(os.path.join(d, ".done"), "w").write("ok")
own = sw.read_ggml(path)["diffusion_conditioning_latent"].reshape(2048)
eng = pkg.Engine(0)
eng.load(diffusion=path)
lats = [np.random.RandomState(s).randn(L, 1024).astype(np.float32) for s, L in ((1, 61), (2, 130), (3, 17))]
rs = np.random.RandomState(8)
n_steps = 8
noise = [rs.randn(n_steps + 1, 100 * eng.frames(len(l))).astype(np.float32) for l in lats]
if mode == "voices":
    mel = eng.diffusion(lats, n_steps=n_steps, noise=noise, voice_latents=own[None], voice_of_candidate=[0, 0, 0])
else:
    mel = eng.diffusion(lats, n_steps=n_steps, noise=noise)
print("%s: crc32 of the mel %08x" % (mode, zlib.crc32(np.concatenate([m.reshape(-1) for m in mel]).tobytes())))
eng.close()
