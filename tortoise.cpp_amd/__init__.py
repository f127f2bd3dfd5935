"""tortoise.cpp_amd — ctypes binding of libtortoise_mi355x.so (the C ABI in include/tortoise_mi355x.h).

This is plumbing only: every stage runs in hand-written HIP kernels inside the shared library. There
is no CPU / PyTorch fallback — importing works without a GPU (for the symbol-export test), but
`Engine()` raises if the library or a HIP device is missing.

Import name: the directory is literally `tortoise.cpp_amd/`; use tortoise_cpp_amd_loader.load().
"""
import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTS_LIB_PATH") or os.path.join(HERE, "libtortoise_mi355x.so")  # TTS_LIB_PATH: developer A/B of another build of the same sources
HEADER = os.path.join(os.path.dirname(HERE), "include", "tortoise_mi355x.h")
VOCAB_MEL = 8194
DMODEL = 1024
AR_MASK_STOP = 1
AR_RETIRE = 2
AR_ROW_CONTROLS = 8  # tts_ar_session_open only
NOISE_REFERENCE, NOISE_DEVICE = 0, 1
SAMPLER_DDPM, SAMPLER_DDIM, SAMPLER_DPMPP_2M = 0, 1, 3  # option diff_sampler, tts_diff_request.sampler (2 is not a sampler)
SCORE_POSITIONS = {"decode": 0, "train": 1}  # TTS_SCORE_POS_DECODE / TTS_SCORE_POS_TRAIN (tts_ar_score_codes)

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
AUDIO_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int)  # tts_audio_cb


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of the library + CLI (in-tree, cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", HERE, "-j8", "all"], stdout=None if verbose else subprocess.DEVNULL)


class ArRequest(C.Structure):
    """tts_ar_request: one session request's candidates, seed, stop schedule, step limit and sampler controls (tts_ar_session_admit_ex)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_cand", C.c_int32), ("seed", C.c_uint32), ("max_steps", C.c_int32), ("stop_at", C.c_void_p),
                ("temperature", C.c_double), ("top_k", C.c_double), ("top_p", C.c_double), ("repetition_penalty", C.c_double), ("penalty_scope", C.c_double),
                ("typical_mass", C.c_double)]   # appended within version 8; a descriptor of the size before it (AR_REQUEST_SIZE_V0) runs under the session's mass


AR_REQUEST_SIZE_V0 = ArRequest.typical_mass.offset


class DiffRequest(C.Structure):
    """tts_diff_request: one diffusion-session request's candidates, step count, sampler controls, voice latent and noise (tts_diff_session_admit)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_cand", C.c_int32), ("latents", C.c_void_p), ("rows", C.c_void_p), ("voice_latent2048", C.c_void_p),
                ("n_steps", C.c_int32), ("sampler", C.c_int32), ("ddim_eta", C.c_double), ("cond_free_k", C.c_double), ("noise", C.c_void_p), ("seed", C.c_uint32),
                ("temperature", C.c_double), ("cond_free", C.c_int32)]  # appended within version 8 at offset 72 (the struct's size before them)


class VoiceAudioOpts(C.Structure):
    """tts_voice_audio_opts: the AR side's per-band norms, its crop offset, and full_clips (tts_voice_from_audio, tts_audio_mel)."""
    _fields_ = [("struct_size", C.c_uint32), ("mel_norms80", C.c_void_p), ("crop_offset", C.c_int64), ("full_clips", C.c_int32)]


# the keys of ar_session_admit(controls=...) and the descriptor fields they set
AR_CONTROL_FIELDS = {"temperature": "temperature", "top_k": "top_k", "top_p": "top_p", "penalty": "repetition_penalty", "scope": "penalty_scope",
                     "typical_mass": "typical_mass"}


class TtsError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TtsError("libtortoise_mi355x.so is not built (run __graft_entry__.build()); there is no fallback path")
    L = C.CDLL(LIB_PATH)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    sig = {
        "tts_version": (ci, []), "tts_create": (vp, [ci]), "tts_destroy": (None, [vp]), "tts_last_error": (C.c_char_p, [vp]),
        "tts_set_option": (ci, [vp, C.c_char_p, C.c_double]),
        "tts_load_ar": (ci, [vp, C.c_char_p]), "tts_load_diffusion": (ci, [vp, C.c_char_p]),
        "tts_load_vocoder": (ci, [vp, C.c_char_p]), "tts_load_clvp": (ci, [vp, C.c_char_p]),
        "tts_load_diffusion_conditioning_encoder": (ci, [vp, C.c_char_p]), "tts_diffusion_conditioning_latent": (ci, [vp, _f32p, _i32p, ci, _f32p]),
        "tts_set_diffusion_conditioning_latent": (ci, [vp, _f32p]),
        "tts_load_voice_encoder": (ci, [vp, C.c_char_p]), "tts_voice_latent": (ci, [vp, _f32p, _i32p, ci, _f32p]),
        "tts_load_cvvp": (ci, [vp, C.c_char_p]), "tts_cvvp_latent_dim": (ci, [vp]), "tts_cvvp_rows": (ci, [ci]),
        "tts_cvvp_voice": (ci, [vp, vp, vp, ci, vp]), "tts_cvvp_voice_audio": (ci, [vp, vp, vp, vp, ci, vp, vp]),
        "tts_cvvp_score": (ci, [vp, vp, ci, vp, vp, ci, ci, vp]),
        "tts_clvp_score": (ci, [vp, _i32p, ci, _i32p, _i32p, ci, ci, _f32p]), "tts_ar_layers": (ci, [vp]), "tts_diffusion_layers": (ci, [vp]),
        "tts_seed": (None, [vp, C.c_uint32]), "tts_rng_load_state": (ci, [vp, C.c_char_p]), "tts_rng_save_state": (ci, [vp, C.c_char_p]),
        "tts_rng_uniform": (cf, [vp]), "tts_rng_normal": (None, [vp, _f32p, C.c_int64]),
        "tts_tokenizer_load": (ci, [vp, C.c_char_p]), "tts_tokenize": (ci, [vp, C.c_char_p, _i32p, ci]),
        "tts_ar_begin": (ci, [vp, _i32p, ci, _f32p, ci, ci]), "tts_ar_prefill": (ci, [vp, _f32p]),
        "tts_ar_step": (ci, [vp, _i32p, ci, _f32p]), "tts_ar_latents": (ci, [vp, _i32p, ci, ci, _f32p]),
        "tts_sample": (ci, [vp, _f32p, _i32p, ci, ci, _i32p]),
        "tts_ar_step_sample": (ci, [vp, _i32p, ci, C.c_uint, _i32p]), "tts_ar_topk_fallbacks": (ci, [vp]), "tts_diffusion_time_mlp_retries": (ci, [vp]), "tts_diffusion_fp16_check": (ci, [vp, C.POINTER(C.c_int64)]),
        "tts_device_numa_node": (ci, [vp, C.c_char_p, ci]), "tts_pin_to_device_numa_node": (ci, [vp]),
        "tts_host_sample_row": (ci, [_f32p, _i32p, ci, cf]), "tts_host_sample_prefiltered": (ci, [_f32p, _i32p, ci, cf, ci]),
        "tts_host_sample_row_ex": (ci, [_f32p, _i32p, ci, cf, cf, ci, cf, cf, ci]), "tts_host_sample_prefiltered_ex": (ci, [_f32p, _i32p, ci, cf, cf, ci, cf, cf, ci, ci]),
        "tts_host_typical_keep": (ci, [_f32p, C.c_double, vp]),
        "tts_host_sample_row_typical": (ci, [_f32p, _i32p, ci, cf, cf, ci, cf, cf, C.c_double, ci]),
        "tts_host_sample_prefiltered_typical": (ci, [_f32p, _i32p, ci, cf, cf, ci, cf, cf, C.c_double, ci]),
        "tts_autoregressive": (ci, [vp, _i32p, ci, _f32p, ci, ci, C.c_uint, _i32p, _i32p, vp, _i32p]),
        "tts_ar_stop_status": (ci, [vp, _i32p, ci]), "tts_ar_set_stop_schedule": (ci, [vp, C.c_void_p, ci]),
        "tts_ar_begin_multi": (ci, [vp, _i32p, _i32p, ci, _f32p, _i32p, ci]),
        "tts_autoregressive_multi": (ci, [vp, _i32p, _i32p, ci, _f32p, _i32p, ci, C.c_uint, _i32p, _i32p, vp, _i32p]),
        "tts_split_text": (ci, [vp, C.c_char_p, ci, _i32p, _i32p, ci]),
        "tts_ar_begin_multi_voice": (ci, [vp, _i32p, _i32p, ci, vp, ci, vp, _i32p, ci]),
        "tts_autoregressive_multi_voice": (ci, [vp, _i32p, _i32p, ci, vp, ci, vp, _i32p, ci, C.c_uint, _i32p, _i32p, vp, _i32p]),
        "tts_diffusion_multi_voice": (ci, [vp, _f32p, _i32p, ci, vp, ci, vp, ci, vp, ci, _f32p]),
        "tts_split_turns": (ci, [vp, C.c_char_p, ci, ci, _i32p, _i32p, _i32p, ci]),
        "tts_host_ar_stop_run": (ci, [_i32p, ci, _i32p, ci, C.c_uint, vp, _i32p, _i32p, _i32p, vp]),
        "tts_diffusion_frames": (ci, [ci]),
        "tts_load_hifigan": (ci, [vp, C.c_char_p]), "tts_hifigan_samples": (ci, [ci]),
        "tts_hifigan_decode": (ci, [vp, vp, vp, ci, vp, ci, vp, vp]),
        "tts_hifigan_chunk": (ci, [vp, vp, vp, ci, vp, ci, vp, vp, vp, vp]),
        "tts_load_bigvgan": (ci, [vp, C.c_char_p]), "tts_bigvgan_samples": (ci, [ci]), "tts_bigvgan": (ci, [vp, vp, vp, ci, vp]),
        "tts_bigvgan_config": (ci, [vp, vp]),
        "tts_load_classifier": (ci, [vp, C.c_char_p]), "tts_classifier_positions": (ci, [ci]), "tts_classify_audio": (ci, [vp, vp, vp, vp, ci, vp, vp]),
        "tts_load_aligner": (ci, [vp, C.c_char_p]), "tts_aligner_frames": (ci, [ci]), "tts_aligner_clip_frames": (ci, [vp, C.c_int64, ci]),
        "tts_aligner_vocab": (ci, [vp, vp, ci, vp]), "tts_aligner_ids": (ci, [vp, vp, vp, vp, ci, vp, vp, ci, vp]),
        "tts_align_audio": (ci, [vp, vp, C.c_int64, ci, C.c_char_p, vp, ci]), "tts_redact_audio": (C.c_int64, [vp, vp, C.c_int64, ci, C.c_char_p, vp, C.c_int64]),
        "tts_host_ctc_decode": (ci, [vp, ci, vp, ci, ci, vp, ci]), "tts_host_max_alignment": (ci, [C.c_char_p, C.c_char_p, vp, ci]),
        "tts_host_ctc_align": (ci, [vp, ci, vp, ci, ci, C.c_char_p, C.c_int64, vp, ci]), "tts_host_redact_spans": (ci, [C.c_char_p, vp, ci, vp, ci]),
        "tts_load_random_voice": (ci, [vp, C.c_char_p, C.c_char_p]), "tts_random_voice_dim": (ci, [vp, ci]),
        "tts_random_voice": (ci, [vp, vp, ci, vp, vp, vp, vp]), "tts_random_voice_noise": (ci, [vp, C.c_uint64, ci, vp, ci]),
        "tts_load_dvae": (ci, [vp, C.c_char_p]), "tts_dvae_rows": (ci, [ci]), "tts_dvae_tokens": (ci, [vp]), "tts_dvae_dim": (ci, [vp]),
        "tts_dvae_codes": (ci, [vp, vp, vp, ci, vp, vp, ci, vp]), "tts_dvae_codes_audio": (ci, [vp, vp, vp, vp, ci, vp, vp, vp, ci, vp]),
        "tts_ar_latents_for_codes": (ci, [vp, vp, ci, vp, vp, ci, vp, vp]),
        "tts_ar_score_codes": (ci, [vp, vp, ci, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]), "tts_host_ar_score_rows": (ci, [vp, ci, ci, vp, vp, vp]),
        "tts_host_blend_voices": (ci, [vp, vp, ci, ci, vp]), "tts_host_random_voice_fold": (ci, [vp, vp, ci, ci, vp, vp]),
        "tts_hifigan_stream": (ci, [vp, vp, ci, vp, ci, C.c_uint, ci, vp, vp, vp, vp, vp, vp]), "tts_hifigan_stream_recaptures": (ci, [vp]),
        "tts_host_stream_final_rows": (ci, [vp, ci]),
        "tts_ar_session_open": (ci, [vp, ci, ci, ci, ci, C.c_uint]), "tts_ar_session_admit": (ci, [vp, vp, ci, vp, ci, C.c_uint32, vp]),
        "tts_ar_session_room": (ci, [vp]), "tts_ar_session_step": (ci, [vp]), "tts_ar_session_finished": (ci, [vp, vp, ci]),
        "tts_ar_session_collect": (ci, [vp, ci, vp, vp, vp, vp, vp]), "tts_ar_session_logits": (ci, [vp, ci, vp]),
        "tts_ar_session_cancel": (ci, [vp, ci]), "tts_ar_session_close": (ci, [vp]), "tts_ar_session_recaptures": (ci, [vp]),
        "tts_ar_session_enable_audio": (ci, [vp, ci]), "tts_ar_session_audio": (ci, [vp, ci, vp, ci, vp]),
        "tts_host_session_first_fit": (ci, [vp, ci, ci]),
        "tts_ar_request_init": (ci, [vp, C.POINTER(ArRequest)]), "tts_ar_session_admit_ex": (ci, [vp, vp, ci, vp, C.POINTER(ArRequest)]),
        "tts_host_ar_request_check": (ci, [C.POINTER(ArRequest), ci, ci]),
        "tts_diff_request_init": (ci, [vp, C.POINTER(DiffRequest)]), "tts_diff_session_open": (ci, [vp, ci, ci]),
        "tts_diff_session_admit": (ci, [vp, C.POINTER(DiffRequest)]), "tts_diff_session_room": (ci, [vp]), "tts_diff_session_step": (ci, [vp]),
        "tts_diff_session_finished": (ci, [vp, vp, ci]), "tts_diff_session_collect": (ci, [vp, ci, vp]), "tts_diff_session_cancel": (ci, [vp, ci]),
        "tts_diff_session_close": (ci, [vp]), "tts_diff_session_captures": (ci, [vp]),
        "tts_host_diff_packed_rows": (ci, [vp, ci]), "tts_host_diff_packed_rows_ex": (ci, [vp, ci, ci]),
        "tts_diffusion_last_layout": (ci, [vp, _i32p, _i32p]), "tts_host_diff_request_check": (ci, [C.POINTER(DiffRequest), ci]),
        "tts_diffusion_forward": (ci, [vp, _f32p, ci, _f32p, ci, ci, _f32p]),
        "tts_diffusion": (ci, [vp, _f32p, _i32p, ci, ci, vp, ci, _f32p]),
        "tts_vocoder_samples": (ci, [ci]),
        "tts_vocoder": (ci, [vp, _f32p, _i32p, ci, vp, ci, _f32p]),
        "tts_vocoder_chunk": (ci, [vp, _f32p, ci, _f32p, ci, ci, _f32p, C.POINTER(ci)]),
        "tts_write_wav": (ci, [C.c_char_p, _f32p, C.c_int64, ci]), "tts_read_wav": (C.c_int64, [C.c_char_p, vp, C.c_int64, vp]),
        "tts_voice_audio_opts_init": (ci, [C.POINTER(VoiceAudioOpts)]),
        "tts_voice_from_audio": (ci, [vp, vp, vp, vp, ci, vp, vp, vp]), "tts_audio_mel": (ci, [vp, vp, C.c_int64, ci, ci, vp, vp, C.c_int64]),
        "tts_host_schedule": (ci, [ci, _i32p] + [_f32p] * 7), "tts_host_schedule_ddim": (ci, [ci, C.c_double, _f64p, _f64p, _f32p, _f32p, _f32p]),
        "tts_host_schedule_dpmpp": (ci, [ci, _f32p, _f32p, _f32p, _i32p]), "tts_host_timestep_embedding": (None, [ci, _f32p]),
        "tts_host_rel_bucket": (ci, [ci, ci]), "tts_host_pad_codes": (ci, [_i32p, ci, _i32p]), "tts_host_trimmed_rows": (ci, [_i32p]),
        "tts_host_fp8_e4m3": (C.c_uint8, [cf]), "tts_host_mel_frames": (ci, [C.c_int64]),
        "tts_host_mel_diffusion100": (ci, [_f32p, C.c_int64, ci, _f32p]), "tts_host_mel_voice80": (ci, [_f32p, C.c_int64, vp, _f32p]),
        "tts_prof_reset": (ci, [vp, ci]), "tts_prof_get": (ci, [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def header_symbols():
    """Function names declared in include/tortoise_mi355x.h (for the export test)."""
    import re
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", txt)))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def blend_scores(clvp, cvvp, cvvp_amount):
    """clvp() * (1 - cvvp_amount) + cvvp() * cvvp_amount in float32 (upstream tortoise-tts api.py); a side whose weight is 0 is not called."""
    a = float(cvvp_amount)
    if not 0.0 <= a <= 1.0:
        raise TtsError("cvvp_amount %r: 0 .. 1" % (cvvp_amount,))
    if a == 0.0:
        return np.asarray(clvp(), np.float32)
    if a == 1.0:
        return np.asarray(cvvp(), np.float32)
    return (np.asarray(clvp(), np.float32) * np.float32(1.0 - a) + np.asarray(cvvp(), np.float32) * np.float32(a)).astype(np.float32)


class Engine:
    """One tts_ctx on one GPU. Mirrors the reference's stage drivers (autoregressive / diffusion / vocoder)."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = self.L.tts_create(device)
        if not self.h:
            raise TtsError("tts_create(%d) failed: no usable HIP device (this engine has no CPU path)" % device)
        self._diff_frames = {}  # frames per candidate of the diffusion session's requests, by id (diff_session_collect sizes its buffer from it)

    def close(self):
        if getattr(self, "h", None):
            self.L.tts_destroy(self.h)
            self.h = None

    __del__ = close

    def _ck(self, rc):
        if rc < 0:
            raise TtsError("%s (status %d)" % (self.L.tts_last_error(self.h).decode(), rc))
        return rc

    # ---- setup ----
    def set_option(self, key, value):
        self._ck(self.L.tts_set_option(self.h, key.encode(), float(value)))

    def load(self, model_dir=None, ar=None, diffusion=None, vocoder=None):
        if model_dir:
            ar = ar or os.path.join(model_dir, "ggml-model.bin")
            diffusion = diffusion or os.path.join(model_dir, "ggml-diffusion-model.bin")
            vocoder = vocoder or os.path.join(model_dir, "ggml-vocoder-model.bin")
        if ar:
            self._ck(self.L.tts_load_ar(self.h, ar.encode()))
        if diffusion:
            self._ck(self.L.tts_load_diffusion(self.h, diffusion.encode()))
        if vocoder:
            self._ck(self.L.tts_load_vocoder(self.h, vocoder.encode()))

    @property
    def ar_layers(self):
        return self.L.tts_ar_layers(self.h)

    def seed(self, s):
        self.L.tts_seed(self.h, s)

    def rng_load_state(self, path):
        self._ck(self.L.tts_rng_load_state(self.h, path.encode()))

    def rng_save_state(self, path):
        self._ck(self.L.tts_rng_save_state(self.h, path.encode()))

    def rng_uniform(self):
        return self.L.tts_rng_uniform(self.h)

    def rng_normal(self, n):
        out = np.empty(n, np.float32)
        self.L.tts_rng_normal(self.h, out, n)
        return out

    def tokenizer_load(self, path):
        return self._ck(self.L.tts_tokenizer_load(self.h, path.encode()))

    def tokenize(self, message):
        out = np.empty(4096, np.int32)
        n = self._ck(self.L.tts_tokenize(self.h, message.encode("utf-8"), out, 4096))
        return out[:n].copy()

    # ---- autoregressive ----
    def ar_begin(self, tokens, voice, B, max_steps):
        self.B = B
        self._ck(self.L.tts_ar_begin(self.h, np.ascontiguousarray(tokens, np.int32), len(tokens),
                                     np.ascontiguousarray(voice, np.float32), B, max_steps))

    def ar_prefill(self):
        out = np.empty((self.B, VOCAB_MEL), np.float32)
        self._ck(self.L.tts_ar_prefill(self.h, out.reshape(-1)))
        return out

    def ar_step(self, prev_ids, i):
        out = np.empty((self.B, VOCAB_MEL), np.float32)
        self._ck(self.L.tts_ar_step(self.h, np.ascontiguousarray(prev_ids, np.int32), i, out.reshape(-1)))
        return out

    def ar_step_sample(self, prev_ids, i, mask_stop=False):
        """tts_ar_step + tts_sample(penalty ids = prev_ids) with the sampler's top-k selected on the device."""
        out = np.empty(self.B, np.int32)
        self._ck(self.L.tts_ar_step_sample(self.h, np.ascontiguousarray(prev_ids, np.int32), i, 1 if mask_stop else 0, out))
        return out

    def topk_fallbacks(self):
        return self.L.tts_ar_topk_fallbacks(self.h)

    def numa_node(self):
        """(NUMA node of this context's GPU or -1, that node's cpulist)"""
        buf = C.create_string_buffer(1024)
        node = self.L.tts_device_numa_node(self.h, buf, 1024)
        return node, buf.value.decode()

    def pin_to_numa_node(self):
        """restrict this process (and the sampler threads created later) to the CPUs of the GPU's NUMA node; returns the number of CPUs, 0 = unchanged"""
        return self.L.tts_pin_to_device_numa_node(self.h)

    def fp16_check(self):
        """(non-finite, saturated) fp16 operand values seen since option fp16_check was set (+ the split weights of the loaded diffusion model)."""
        c = (C.c_int64 * 2)()
        self._ck(self.L.tts_diffusion_fp16_check(self.h, c))
        return int(c[0]), int(c[1])

    def time_mlp_retries(self):
        return self.L.tts_diffusion_time_mlp_retries(self.h)

    def ar_latents(self, codes502, n_mel=502):
        codes502 = np.ascontiguousarray(codes502, np.int32).reshape(-1, 502)
        nb = codes502.shape[0]
        out = np.empty((nb, min(500, n_mel), DMODEL), np.float32)
        self._ck(self.L.tts_ar_latents(self.h, codes502.reshape(-1), nb, n_mel, out.reshape(-1)))
        return out

    def sample(self, logits, penalty_ids):
        logits = np.ascontiguousarray(logits, np.float32)
        ids = np.ascontiguousarray(penalty_ids, np.int32).reshape(logits.shape[0], -1)
        out = np.empty(logits.shape[0], np.int32)
        self._ck(self.L.tts_sample(self.h, logits.reshape(-1), ids.reshape(-1), ids.shape[1], logits.shape[0], out))
        return out

    def set_stop_schedule(self, stop_at=None):
        """candidate b of the following autoregressive() calls samples the stop token after stop_at[b] codes (None clears): a reproducible ragged batch"""
        if stop_at is None:
            self._ck(self.L.tts_ar_set_stop_schedule(self.h, None, 0))
        else:
            a = np.ascontiguousarray(stop_at, np.int32)
            self._ck(self.L.tts_ar_set_stop_schedule(self.h, a.ctypes.data_as(C.c_void_p), len(a)))

    def autoregressive(self, tokens, voice, B, max_steps, mask_stop=False, want_latents=True, retire=False):
        """Returns (codes [B,502], rows [B], list of trimmed latents [rows_c,1024], steps)."""
        codes = np.empty((B, 502), np.int32)
        rows = np.empty(B, np.int32)
        steps = np.zeros(1, np.int32)
        lat = np.empty((B * 500, DMODEL), np.float32) if want_latents else None
        self._ck(self.L.tts_autoregressive(self.h, np.ascontiguousarray(tokens, np.int32), len(tokens),
                                           np.ascontiguousarray(voice, np.float32), B, max_steps,
                                           (AR_MASK_STOP if mask_stop else 0) | (AR_RETIRE if retire else 0), codes.reshape(-1), rows, _ptr(lat), steps))
        lats = None
        if want_latents:
            lats, off = [], 0
            for r in rows:
                lats.append(lat[off:off + r].copy())
                off += r
        return codes, rows, lats, int(steps[0])

    def ar_begin_multi(self, prompts, voice=None, n_cand=1, max_steps=1, voices=None, voice_of_prompt=None):
        """Several prompts in one batch: prompt g (text ids) gets n_cand[g] candidates, candidates in prompt order. ar_prefill / ar_step / ar_step_sample /
        ar_latents then work on all sum(n_cand) rows. One `voice` [1024] for all, or `voices` [V, 1024] with `voice_of_prompt` [G] (tts_ar_begin_multi_voice)."""
        ids, lens, nc = _prompt_args(prompts, n_cand)
        self.B = int(nc.sum())
        if voices is None and voice_of_prompt is None:
            self._ck(self.L.tts_ar_begin_multi(self.h, ids, lens, len(lens), np.ascontiguousarray(voice, np.float32), nc, max_steps))
            return
        tab, nv, idx = _voice_args(voice, voices, voice_of_prompt, DMODEL)
        self._ck(self.L.tts_ar_begin_multi_voice(self.h, ids, lens, len(lens), _ptr(tab), nv, _ptr(idx), nc, max_steps))

    def autoregressive_multi(self, prompts, voice=None, n_cand=1, max_steps=1, mask_stop=False, retire=False, want_latents=True, voices=None, voice_of_prompt=None):
        """autoregressive() of every prompt inside one decode loop. Returns (codes, rows, latents, steps): per prompt g codes [n_cand[g], 502], rows
        [n_cand[g]] and the list of its candidates' trimmed latents (None without want_latents); steps = sampling iterations of the shared loop.
        One `voice` [1024] for all, or `voices` [V, 1024] with `voice_of_prompt` [G] (tts_autoregressive_multi_voice)."""
        ids, lens, nc = _prompt_args(prompts, n_cand)
        B = int(nc.sum())
        codes = np.empty((B, 502), np.int32)
        rows = np.empty(B, np.int32)
        steps = np.zeros(1, np.int32)
        lat = np.empty((B * 500, DMODEL), np.float32) if want_latents else None
        flags = (AR_MASK_STOP if mask_stop else 0) | (AR_RETIRE if retire else 0)
        if voices is None and voice_of_prompt is None:
            self._ck(self.L.tts_autoregressive_multi(self.h, ids, lens, len(lens), np.ascontiguousarray(voice, np.float32), nc, max_steps, flags,
                                                     codes.reshape(-1), rows, _ptr(lat), steps))
        else:
            tab, nv, idx = _voice_args(voice, voices, voice_of_prompt, DMODEL)
            self._ck(self.L.tts_autoregressive_multi_voice(self.h, ids, lens, len(lens), _ptr(tab), nv, _ptr(idx), nc, max_steps, flags, codes.reshape(-1), rows,
                                                           _ptr(lat), steps))
        c0 = np.concatenate([[0], np.cumsum(nc)])
        out_codes = [codes[c0[g]:c0[g + 1]].copy() for g in range(len(nc))]
        out_rows = [rows[c0[g]:c0[g + 1]].copy() for g in range(len(nc))]
        out_lats = None
        if want_latents:
            out_lats, off = [], 0
            for g in range(len(nc)):
                lg = []
                for r in out_rows[g]:
                    lg.append(lat[off:off + r].copy())
                    off += r
                out_lats.append(lg)
        return out_codes, out_rows, out_lats, int(steps[0])

    def split_text(self, message, max_ids):
        """Chunks of `message` that each tokenize to at most max_ids ids (tts_split_text's rule): a list of strings."""
        raw = message.encode("utf-8")
        cap = len(raw) + 1
        starts, lens = np.empty(cap, np.int32), np.empty(cap, np.int32)
        n = self._ck(self.L.tts_split_text(self.h, raw, max_ids, starts, lens, cap))
        return [raw[starts[k]:starts[k] + lens[k]].decode("utf-8") for k in range(n)]

    def split_turns(self, message, n_voices, max_ids=404):
        """Chunks of a multi-speaker message (tts_split_turns' rule: one turn per line, "<index>|" in front of a turn names its voice): a list of
        (text, voice index)."""
        raw = message.encode("utf-8")
        cap = len(raw) + 1
        starts, lens, vo = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int32)
        n = self._ck(self.L.tts_split_turns(self.h, raw, n_voices, max_ids, starts, lens, vo, cap))
        return [(raw[starts[k]:starts[k] + lens[k]].decode("utf-8"), int(vo[k])) for k in range(n)]

    def ar_stop_status(self, B):
        """Per candidate of the last autoregressive() call: 1 = ended in a sampled stop token, 0 = cut at max_steps."""
        out = np.zeros(B, np.int32)
        self._ck(self.L.tts_ar_stop_status(self.h, out, B))
        return out

    # ---- in-flight batching: requests join and leave a running batch (tts_ar_session_*) ----
    def ar_session_open(self, n_slots, max_cand, max_text, max_steps, mask_stop=False, retire=False, row_controls=False):
        """A batch of n_slots rows that requests of up to max_cand candidates and max_text ids join and leave at any step. The sampler controls, ar_weights,
        ggml_lut and device_topk are read here and hold until ar_session_close(). row_controls: requests may bring sampler controls of their own
        (ar_session_admit(controls=...)); the step then ends with the per-row prefilter."""
        flags = (AR_MASK_STOP if mask_stop else 0) | (AR_RETIRE if retire else 0) | (AR_ROW_CONTROLS if row_controls else 0)
        self._ck(self.L.tts_ar_session_open(self.h, n_slots, max_cand, max_text, max_steps, flags))
        self._session_cand = {}

    def ar_request(self, n_cand=1, seed=0, stop_at=None, controls=None, max_steps=None):
        """A tts_ar_request filled from the open session's pinned options (tts_ar_request_init), then from the arguments. controls: a dict with any of
        temperature, top_k, top_p, penalty, scope, typical_mass. The stop_at array must outlive the descriptor's use."""
        req = ArRequest()
        req.struct_size = C.sizeof(ArRequest)
        self._ck(self.L.tts_ar_request_init(self.h, C.byref(req)))
        req.n_cand, req.seed, req.max_steps = n_cand, seed, 0 if max_steps is None else max_steps
        req.stop_at = None if stop_at is None else stop_at.ctypes.data
        for k, v in (controls or {}).items():
            if k not in AR_CONTROL_FIELDS:
                raise ValueError("controls: any of %s, not %r" % (", ".join(AR_CONTROL_FIELDS), k))
            setattr(req, AR_CONTROL_FIELDS[k], v)
        return req

    def ar_session_admit(self, tokens, voice, n_cand, seed, stop_at=None, controls=None, max_steps=None):
        """Admits a request into the lowest run of n_cand free slots and returns its id; TtsError (status -6) when there is no such run. controls (a dict with
        any of temperature, top_k, top_p, penalty, scope, typical_mass; missing keys take the session's values) and max_steps (at most the session's): the request's own;
        with either the call goes through tts_ar_session_admit_ex. Controls that differ from the session's need ar_session_open(row_controls=True)."""
        tok = np.ascontiguousarray(tokens, np.int32)
        v = np.ascontiguousarray(voice, np.float32)
        sa = None if stop_at is None else np.ascontiguousarray(stop_at, np.int32)
        if v.size != DMODEL or (sa is not None and len(sa) != n_cand):
            raise ValueError("voice [1024]; stop_at [n_cand]")
        if controls is not None or max_steps is not None:
            req = self.ar_request(n_cand, seed, sa, controls, max_steps)
            rid = self._ck(self.L.tts_ar_session_admit_ex(self.h, _ptr(tok), len(tok), _ptr(v), C.byref(req)))
        else:
            rid = self._ck(self.L.tts_ar_session_admit(self.h, _ptr(tok), len(tok), _ptr(v), n_cand, seed, _ptr(sa)))
        self._session_cand[rid] = n_cand
        return rid

    def ar_session_room(self):
        return self._ck(self.L.tts_ar_session_room(self.h))

    def ar_session_step(self):
        """One decode step for every live row; returns the number of live requests left."""
        return self._ck(self.L.tts_ar_session_step(self.h))

    def ar_session_finished(self):
        """Ids of the finished, not yet collected requests, oldest first."""
        out = np.zeros(max(1, len(self._session_cand)), np.int32)
        n = self._ck(self.L.tts_ar_session_finished(self.h, _ptr(out), len(out)))
        return [int(x) for x in out[:min(n, len(out))]]

    def ar_session_collect(self, request, want_latents=True):
        """A finished request's (codes [n_cand,502], rows [n_cand], list of trimmed latents, steps, stopped [n_cand]); its slots are free afterwards."""
        B = self._session_cand[request]
        codes = np.empty((B, 502), np.int32)
        rows = np.empty(B, np.int32)
        steps = np.zeros(1, np.int32)
        stopped = np.zeros(B, np.int32)
        lat = np.empty((B * 500, DMODEL), np.float32) if want_latents else None
        rc = self.L.tts_ar_session_collect(self.h, request, _ptr(codes), _ptr(rows), _ptr(lat), _ptr(steps), _ptr(stopped))
        if rc == -6:  # a strict request that reached max_steps: gone, its slots are free
            self._session_cand.pop(request, None)
        self._ck(rc)
        self._session_cand.pop(request, None)
        lats = None
        if want_latents:
            lats, off = [], 0
            for r in rows:
                lats.append(lat[off:off + r].copy())
                off += r
        return codes, rows, lats, int(steps[0]), stopped

    def ar_session_logits(self, request):
        """Diagnostic: the request's rows of the last step's logits [n_cand, 8194]."""
        out = np.empty((self._session_cand[request], VOCAB_MEL), np.float32)
        self._ck(self.L.tts_ar_session_logits(self.h, request, _ptr(out)))
        return out

    def ar_session_cancel(self, request):
        self._ck(self.L.tts_ar_session_cancel(self.h, request))
        self._session_cand.pop(request, None)

    def ar_session_close(self):
        self._ck(self.L.tts_ar_session_close(self.h))
        self._session_cand = {}

    def ar_session_recaptures(self):
        return self._ck(self.L.tts_ar_session_recaptures(self.h))

    def ar_session_enable_audio(self, stride):
        """Right after ar_session_open(): every one-candidate request receives HiFi-GAN audio while it decodes; an audio pass runs on every stride-th step of
        the session and on the step in which a request finishes (load_hifigan() first)."""
        self._ck(self.L.tts_ar_session_enable_audio(self.h, stride))

    def ar_session_audio(self, request):
        """Drains the request's decoded audio: (float32 samples, a multiple of 256, possibly none; is_last: the request has finished and nothing is left)."""
        cap = 256 * self.frames(500)  # a whole utterance
        buf = getattr(self, "_session_pcm", None)
        if buf is None:
            buf = self._session_pcm = np.empty(cap, np.float32)
        last = np.zeros(1, np.int32)
        n = self._ck(self.L.tts_ar_session_audio(self.h, request, _ptr(buf), cap, _ptr(last)))
        return buf[:n].copy(), bool(last[0])

    # ---- voice-conditioning encoder (not in the reference) ----
    def load_voice_encoder(self, path):
        self._ck(self.L.tts_load_voice_encoder(self.h, path.encode()))

    def voice_latent(self, mels):
        """mels: list of [80, T_c] log-mel spectrograms of the reference clips. Returns the 1024-float voice latent (a --voice file)."""
        frames = np.array([m.shape[1] for m in mels], np.int32)
        mel = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in mels]))
        out = np.empty(1024, np.float32)
        self._ck(self.L.tts_voice_latent(self.h, mel, frames, len(mels), out))
        return out

    # ---- a voice from audio clips, on the device (not in the reference) ----
    def _audio_opts(self, mel_norms, crop_offset, full_clips, struct_size=None):
        o = VoiceAudioOpts()
        o.struct_size = C.sizeof(VoiceAudioOpts)
        if self.L.tts_voice_audio_opts_init(C.byref(o)):
            raise TtsError("tts_voice_audio_opts_init failed")
        mn = None if mel_norms is None else np.ascontiguousarray(mel_norms, np.float32).reshape(80)
        o.mel_norms80, o.crop_offset, o.full_clips = _ptr(mn), int(crop_offset), int(full_clips)
        if struct_size is not None:
            o.struct_size = struct_size
        return o, mn  # mn: kept alive by the caller for the call's duration

    def voice_from_audio(self, clips, rates, mel_norms=None, crop_offset=0, full_clips=False, want=(True, True)):
        """clips: list of mono float32 sample arrays, rates: their sample rates (one int for all, or one per clip). Returns (voice latent [1024], diffusion
        conditioning latent [2048]); want = (AR side, diffusion side): a side that is not wanted is None and its encoder need not be loaded."""
        rates = [int(rates)] * len(clips) if np.isscalar(rates) else [int(r) for r in rates]
        if len(rates) != len(clips):
            raise TtsError("%d rates for %d clips" % (len(rates), len(clips)))
        n = np.array([len(c) for c in clips], np.int64)
        a = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in clips])) if len(clips) else np.zeros(1, np.float32)
        r = np.array(rates, np.int32)
        o, keep = self._audio_opts(mel_norms, crop_offset, full_clips)
        out1 = np.empty(1024, np.float32) if want[0] else None
        out2 = np.empty(2048, np.float32) if want[1] else None
        self._ck(self.L.tts_voice_from_audio(self.h, _ptr(a), _ptr(n), _ptr(r), len(clips), C.addressof(o), _ptr(out1), _ptr(out2)))
        return out1, out2

    # ---- random voices (not in the reference): upstream's RandomLatentConverter, what tts() runs when it is given neither clips nor latents ----
    RANDOM_VOICE_SIDES = {"auto": 0, "diffusion": 1}

    def load_random_voice(self, auto=None, diffusion=None):
        """auto: rlg_auto converted (the AR conditioning latent's model), diffusion: rlg_diffuser converted; either may be None (tts_load_random_voice)."""
        self._ck(self.L.tts_load_random_voice(self.h, None if auto is None else auto.encode(), None if diffusion is None else diffusion.encode()))

    def random_voice_dim(self, side):
        return self.L.tts_random_voice_dim(self.h, self.RANDOM_VOICE_SIDES[side])

    def random_voice(self, seeds, z_auto=None, z_diff=None, sides=("auto", "diffusion")):
        """n voices in one call. seeds: n unsigned 64-bit integers (or None where every requested side has a z); z_auto [n, 1024] / z_diff [n, 2048]: the
        model's input in place of the device generator's (torch.randn values reproduce upstream). Returns (auto [n, 1024] or None, diffusion [n, 2048] or
        None): a side not named in `sides` is None and need not be loaded."""
        for s in sides:
            if s not in self.RANDOM_VOICE_SIDES:
                raise TtsError("side %r: 'auto' or 'diffusion'" % (s,))
        sd = None if seeds is None else np.array([int(v) for v in (seeds if np.ndim(seeds) else [seeds])], np.uint64).reshape(-1)
        za = None if z_auto is None else np.ascontiguousarray(z_auto, np.float32)
        zd = None if z_diff is None else np.ascontiguousarray(z_diff, np.float32)
        n = len(sd) if sd is not None else len(za) if za is not None and za.ndim == 2 else len(zd) if zd is not None and zd.ndim == 2 else 0
        outs = []
        for side, z in (("auto", za), ("diffusion", zd)):
            dim = self.random_voice_dim(side)
            if z is not None and side in sides and (z.ndim != 2 or z.shape != (n, dim)):
                raise TtsError("z of the %s side has shape %s, (%d, %d) expected" % (side, z.shape, n, dim))
            outs.append(np.empty((max(n, 0), dim), np.float32) if side in sides and dim > 0 and n > 0 else None)
        # a side that is wanted but not loaded (or n = 0) is still handed to the library: the refusal and its text are the library's
        dummy = np.empty(1, np.float32)
        pa = _ptr(outs[0]) if outs[0] is not None else (_ptr(dummy) if "auto" in sides else None)
        pd = _ptr(outs[1]) if outs[1] is not None else (_ptr(dummy) if "diffusion" in sides else None)
        self._ck(self.L.tts_random_voice(self.h, _ptr(sd), n, _ptr(za) if "auto" in sides else None, _ptr(zd) if "diffusion" in sides else None, pa, pd))
        return outs[0], outs[1]

    def random_voice_noise(self, seed, side):
        """the input the device generator gives `seed` on `side` ('auto' / 'diffusion'): random_voice(z = this) is random_voice(seeds = [seed])"""
        dim = self.random_voice_dim(side)
        out = np.empty(max(dim, 1), np.float32)
        self._ck(self.L.tts_random_voice_noise(self.h, int(seed), self.RANDOM_VOICE_SIDES[side], _ptr(out), dim))
        return out[:dim]

    def audio_mel(self, audio, rate, bands, mel_norms=None, crop_offset=0, full_clips=False):
        """[bands, frames] log-mel the front-end hands to the encoder for one clip: bands 80 (the input of voice_latent) or 100 (of
        diffusion_conditioning_latent)."""
        a = np.ascontiguousarray(audio, np.float32).reshape(-1)
        o, keep = self._audio_opts(mel_norms, crop_offset, full_clips)
        frames = self._ck(self.L.tts_audio_mel(self.h, _ptr(a), len(a), int(rate), int(bands), C.addressof(o), None, 0))
        out = np.empty((int(bands), frames), np.float32)
        self._ck(self.L.tts_audio_mel(self.h, _ptr(a), len(a), int(rate), int(bands), C.addressof(o), _ptr(out), out.size))
        return out

    def load_diffusion_conditioning_encoder(self, path):
        self._ck(self.L.tts_load_diffusion_conditioning_encoder(self.h, path.encode()))

    def diffusion_conditioning_latent(self, mels):
        """mels: list of [100, T_c] mel spectrograms of the reference clips. Returns the 2048-float diffusion conditioning latent."""
        frames = np.array([m.shape[1] for m in mels], np.int32)
        mel = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in mels]))
        out = np.empty(2048, np.float32)
        self._ck(self.L.tts_diffusion_conditioning_latent(self.h, mel, frames, len(mels), out))
        return out

    def set_diffusion_conditioning_latent(self, latent):
        self._ck(self.L.tts_set_diffusion_conditioning_latent(self.h, np.ascontiguousarray(latent, np.float32).reshape(2048)))

    # ---- candidate re-ranking (not in the reference) ----
    def load_clvp(self, path):
        self._ck(self.L.tts_load_clvp(self.h, path.encode()))

    def clvp_score(self, text_ids, codes_list):
        """codes_list: per candidate its sampled mel codes (< 8192, no start / stop token). Returns scores [n_candidates]."""
        lens = np.array([len(c) for c in codes_list], np.int32)
        stride = int(lens.max())
        codes = np.zeros((len(codes_list), stride), np.int32)
        for i, c in enumerate(codes_list):
            codes[i, :len(c)] = c
        out = np.empty(len(codes_list), np.float32)
        self._ck(self.L.tts_clvp_score(self.h, np.ascontiguousarray(text_ids, np.int32), len(text_ids), codes.reshape(-1), lens, len(codes_list), stride, out))
        return out

    # ---- CVVP: the candidates' codes against the voice clips (not in the reference) ----
    def load_cvvp(self, path):
        self._ck(self.L.tts_load_cvvp(self.h, path.encode()))

    @property
    def cvvp_latent_dim(self):
        n = self.L.tts_cvvp_latent_dim(self.h)
        if n < 0:
            raise TtsError("tts_load_cvvp not called (status %d)" % n)
        return n

    @staticmethod
    def cvvp_rows(mel_frames):
        """rows the CVVP stem's two strided convolutions make of mel_frames frames (pure: no context, no GPU)"""
        return lib().tts_cvvp_rows(int(mel_frames))

    def cvvp_voice(self, mels):
        """mels: list of [80, T_c] log-mels of the conditioning clips (audio_mel(clip, rate, 80, mel_norms)). Returns one normalised conditioning latent per
        clip [n_clips, latent dim]: computed once per voice, reused for every cvvp_score of that voice."""
        frames = np.array([np.shape(m)[1] for m in mels], np.int32)
        mel = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in mels])) if len(mels) else np.zeros(1, np.float32)
        out = np.empty((len(mels), self.cvvp_latent_dim), np.float32)
        self._ck(self.L.tts_cvvp_voice(self.h, _ptr(mel), _ptr(frames), len(mels), _ptr(out)))
        return out

    def cvvp_voice_audio(self, clips, rates, mel_norms=None, crop_offset=0, full_clips=False):
        """the same from samples: clips and rates as voice_from_audio; the mel never leaves the device"""
        rates = [int(rates)] * len(clips) if np.isscalar(rates) else [int(r) for r in rates]
        if len(rates) != len(clips):
            raise TtsError("%d rates for %d clips" % (len(rates), len(clips)))
        n = np.array([len(c) for c in clips], np.int64)
        a = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in clips])) if len(clips) else np.zeros(1, np.float32)
        r = np.array(rates, np.int32)
        o, keep = self._audio_opts(mel_norms, crop_offset, full_clips)
        out = np.empty((len(clips), self.cvvp_latent_dim), np.float32)
        self._ck(self.L.tts_cvvp_voice_audio(self.h, _ptr(a), _ptr(n), _ptr(r), len(clips), C.addressof(o), _ptr(out)))
        return out

    def cvvp_score(self, voice_latents, codes_list):
        """voice_latents [n_clips, latent dim] from cvvp_voice / cvvp_voice_audio; codes_list as clvp_score. Returns scores [n_candidates]: the mean over the clips."""
        lat = np.ascontiguousarray(voice_latents, np.float32).reshape(-1, self.cvvp_latent_dim)
        lens = np.array([len(c) for c in codes_list], np.int32)
        stride = max(int(lens.max()), 1) if len(lens) else 1
        codes = np.zeros((len(codes_list), stride), np.int32)
        for i, c in enumerate(codes_list):
            codes[i, :len(c)] = c
        out = np.empty(len(codes_list), np.float32)
        self._ck(self.L.tts_cvvp_score(self.h, _ptr(lat), len(lat), _ptr(codes), _ptr(lens), len(codes_list), stride, _ptr(out)))
        return out

    def rerank(self, text_ids, codes_list, voice_latents=None, cvvp_amount=0.0):
        """Upstream's blend of the two re-rankers, clvp * (1 - cvvp_amount) + cvvp * cvvp_amount; the caller keeps the arg-max. The side whose weight is 0 is not
        evaluated (and its model need not be loaded)."""
        return blend_scores(lambda: self.clvp_score(text_ids, codes_list), lambda: self.cvvp_score(voice_latents, codes_list), cvvp_amount)

    # ---- BigVGAN vocoder (not in the reference): the diffusion stage's mel -> 24 kHz audio, beside vocoder() ----
    def load_bigvgan(self, path):
        self._ck(self.L.tts_load_bigvgan(self.h, path.encode()))

    @staticmethod
    def bigvgan_samples(frames):
        return lib().tts_bigvgan_samples(frames)

    def bigvgan_config(self):
        """(C0, strides) of the loaded model, read from its tensor shapes (tts_bigvgan_config)."""
        out = np.zeros(8, np.int32)
        self._ck(self.L.tts_bigvgan_config(self.h, _ptr(out)))
        return int(out[0]), tuple(int(u) for u in out[2:2 + out[1]])

    def bigvgan(self, mels):
        """mels: list of [100, T_c] (normalised, as diffusion() returns them). Returns a list of float32 waveforms, 256 * T_c samples each
        (tts_bigvgan: one call, no noise)."""
        frames = np.array([np.asarray(m).shape[-1] for m in mels], np.int32)
        mel = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in mels]))
        if mel.size != 100 * int(frames.sum()):
            raise TtsError("bigvgan: every mel is [100, T]")
        ns = [self.bigvgan_samples(int(t)) for t in frames]
        audio = np.empty(sum(ns), np.float32)
        self._ck(self.L.tts_bigvgan(self.h, _ptr(mel), _ptr(frames), len(frames), _ptr(audio)))
        out, off = [], 0
        for n in ns:
            out.append(audio[off:off + n].copy())
            off += n
        return out

    # ---- tortoise-detect (not in the reference): upstream's synthesized-speech classifier on the raw waveform ----
    def load_classifier(self, path):
        self._ck(self.L.tts_load_classifier(self.h, path.encode()))

    @staticmethod
    def classifier_positions(n_samples_24k):
        return lib().tts_classifier_positions(n_samples_24k)

    def classify_audio(self, clips, rates):
        """clips: list of mono float32 sample arrays, rates: their sample rates (one int for all, or one per clip). Returns (prob [n], logits [n, 2]):
        prob = softmax(logits)[:, 0], "the probability that the clip is Tortoise's" (tts_classify_audio: one call for the ragged batch)."""
        rates = [int(rates)] * len(clips) if np.isscalar(rates) else [int(r) for r in rates]
        if len(rates) != len(clips):
            raise TtsError("%d rates for %d clips" % (len(rates), len(clips)))
        n = np.array([len(c) for c in clips], np.int64)
        a = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in clips])) if len(clips) else np.zeros(1, np.float32)
        r = np.array(rates, np.int32)
        prob, logits = np.empty(len(clips), np.float32), np.empty((len(clips), 2), np.float32)
        self._ck(self.L.tts_classify_audio(self.h, _ptr(a), _ptr(n), _ptr(r), len(clips), _ptr(prob), _ptr(logits)))
        return prob, logits

    # ---- the DVAE encoder (not in the reference): speech codes from audio ----
    def load_dvae(self, path):
        self._ck(self.L.tts_load_dvae(self.h, path.encode()))

    @staticmethod
    def dvae_rows(mel_frames):
        """codes the DVAE encoder's two strided convolutions make of mel_frames frames (pure: no context, no GPU)"""
        return lib().tts_dvae_rows(int(mel_frames))

    @property
    def dvae_tokens(self):
        return self.L.tts_dvae_tokens(self.h)

    def _dvae_out(self, n_clips, stride, z):
        codes, nc = np.zeros((n_clips, stride), np.int32), np.zeros(n_clips, np.int32)
        zz = np.zeros((n_clips, stride, self.L.tts_dvae_dim(self.h)), np.float32) if z else None
        return codes, nc, zz

    @staticmethod
    def _dvae_split(codes, nc, zz):
        out = [codes[i, :nc[i]].copy() for i in range(len(nc))]
        return out if zz is None else (out, [zz[i, :nc[i]].copy() for i in range(len(nc))])

    def dvae_codes(self, mels, z=False):
        """mels: list of [80, T_c] log-mels (audio_mel(clip, rate, 80, mel_norms, full_clips=True)). Returns a list of int32 code arrays, one per clip
        (tts_dvae_codes: one call for the ragged batch); z=True: (codes, list of float32 [codes, dim], the encoder's output in front of the quantiser)."""
        if not len(mels):
            raise TtsError("dvae_codes: no clips")
        frames = np.array([np.shape(m)[1] for m in mels], np.int32)
        mel = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in mels]))
        stride = max(1, max(self.dvae_rows(int(f)) for f in frames))
        codes, nc, zz = self._dvae_out(len(mels), stride, z)
        self._ck(self.L.tts_dvae_codes(self.h, _ptr(mel), _ptr(frames), len(mels), _ptr(codes), _ptr(nc), stride, None if zz is None else _ptr(zz)))
        return self._dvae_split(codes, nc, zz)

    def dvae_codes_audio(self, clips, rates, mel_norms=None, z=False):
        """the same from samples: clips and rates as voice_from_audio, always the whole clip; the mel never leaves the device"""
        rates = [int(rates)] * len(clips) if np.isscalar(rates) else [int(r) for r in rates]
        if len(rates) != len(clips) or not len(clips):
            raise TtsError("%d rates for %d clips" % (len(rates), len(clips)))
        n = np.array([len(c) for c in clips], np.int64)
        a = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in clips]))
        r = np.array(rates, np.int32)
        o, keep = self._audio_opts(mel_norms, 0, True)
        frames = [self._ck(self.L.tts_audio_mel(self.h, _ptr(np.ascontiguousarray(c, np.float32)), len(c), rt, 80, C.addressof(o), None, 0)) for c, rt in zip(clips, rates)]
        stride = max(1, max(self.dvae_rows(f) for f in frames))
        codes, nc, zz = self._dvae_out(len(clips), stride, z)
        self._ck(self.L.tts_dvae_codes_audio(self.h, _ptr(a), _ptr(n), _ptr(r), len(clips), C.addressof(o), _ptr(codes), _ptr(nc), stride,
                                             None if zz is None else _ptr(zz)))
        return self._dvae_split(codes, nc, zz)

    def ar_score_codes(self, tokens, voice, codes_list, positions="decode"):
        """Teacher-forced scores of given code sequences under a text and a voice (tts_ar_score_codes): one batched latent pass and one fused head launch, no
        sampling. positions "decode" (code i at mel position i + 2: what the sampler saw) or "train" (i + 1: the latent pass's). Per candidate a dict of arrays
        [n + 1]: logp (log P of code j, the last entry the stop token's), stop_logp, greedy (the argmax id) and lse."""
        if positions not in SCORE_POSITIONS:
            raise TtsError("positions %r: 'decode' or 'train'" % (positions,))
        tokens, voice = np.ascontiguousarray(tokens, np.int32), np.ascontiguousarray(voice, np.float32)
        seqs = [np.ascontiguousarray(c, np.int32).reshape(-1) for c in codes_list]
        n = np.array([len(s) for s in seqs], np.int32)
        stride = max(1, int(n.max())) if len(seqs) else 1
        codes = np.zeros((len(seqs), stride), np.int32)
        for b, s in enumerate(seqs):
            codes[b, :len(s)] = s
        logp, stop, lse = (np.full((len(seqs), stride + 1), np.nan, np.float32) for _ in range(3))
        greedy = np.full((len(seqs), stride + 1), -1, np.int32)
        self._ck(self.L.tts_ar_score_codes(self.h, _ptr(tokens), len(tokens), _ptr(voice), _ptr(codes), _ptr(n), len(seqs), stride, SCORE_POSITIONS[positions],
                                           _ptr(logp), _ptr(stop), _ptr(greedy), _ptr(lse)))
        return [{"logp": logp[b, :n[b] + 1].copy(), "stop_logp": stop[b, :n[b] + 1].copy(), "greedy": greedy[b, :n[b] + 1].copy(), "lse": lse[b, :n[b] + 1].copy()}
                for b in range(len(seqs))]

    def ar_latents_for_codes(self, tokens, voice, codes):
        """latents [rows, 1024] of GIVEN speech codes (a recording's, from dvae_codes) under a text and a voice: ar_begin + ar_prefill + host_pad_codes +
        ar_latents + host_trimmed_rows as one call (tts_ar_latents_for_codes), bit for bit; no sampling, the generator is not touched."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        codes = np.ascontiguousarray(codes, np.int32)
        voice = np.ascontiguousarray(voice, np.float32)
        rows = C.c_int32(0)
        out = np.empty((500, DMODEL), np.float32)
        self._ck(self.L.tts_ar_latents_for_codes(self.h, _ptr(tokens), len(tokens), _ptr(voice), _ptr(codes), len(codes), C.byref(rows), _ptr(out)))
        return out[:rows.value].copy()

    # ---- the wav2vec2 CTC aligner (not in the reference): redact bracketed prompt text from the audio ----
    def load_aligner(self, path):
        self._ck(self.L.tts_load_aligner(self.h, path.encode()))

    @staticmethod
    def aligner_frames(n_samples_16k):
        return lib().tts_aligner_frames(n_samples_16k)

    def aligner_vocab(self):
        """(vocab int32 [V]: the code point of every token or -1, blank id) of the loaded aligner"""
        blank = C.c_int32(0)
        V = self._ck(self.L.tts_aligner_vocab(self.h, None, 0, C.byref(blank)))
        vocab = np.empty(V, np.int32)
        self._ck(self.L.tts_aligner_vocab(self.h, _ptr(vocab), V, None))
        return vocab, blank.value

    def aligner_ids(self, clips, rates, logits=False):
        """clips: list of mono float32 sample arrays, rates: one int for all or one per clip. Returns a list of int32 id arrays [frames], one per clip
        (tts_aligner_ids: one call for the ragged batch); logits=True: (ids, list of float32 [frames, V])."""
        rates = [int(rates)] * len(clips) if np.isscalar(rates) else [int(r) for r in rates]
        if len(rates) != len(clips) or not clips:
            raise TtsError("%d rates for %d clips" % (len(rates), len(clips)))
        n = np.array([len(c) for c in clips], np.int64)
        stride = max(1, max(self._ck(self.L.tts_aligner_clip_frames(self.h, len(c), r)) for c, r in zip(clips, rates)))
        a = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in clips]))
        r = np.array(rates, np.int32)
        ids, nf = np.zeros((len(clips), stride), np.int32), np.zeros(len(clips), np.int32)
        lg = np.zeros((len(clips), stride, self.aligner_vocab()[0].size), np.float32) if logits else None
        self._ck(self.L.tts_aligner_ids(self.h, _ptr(a), _ptr(n), _ptr(r), len(clips), _ptr(ids), _ptr(nf), stride, None if lg is None else _ptr(lg)))
        out = [ids[i, :nf[i]].copy() for i in range(len(clips))]
        return (out, [lg[i, :nf[i]].copy() for i in range(len(clips))]) if logits else out

    def align_audio(self, clip, rate, text):
        """one sample offset (in samples of `clip`) per character of `text` (tts_align_audio)"""
        clip = np.ascontiguousarray(clip, np.float32)
        out = np.zeros(max(1, len(text)), np.int64)
        n = self._ck(self.L.tts_align_audio(self.h, _ptr(clip), len(clip), int(rate), text.encode(), _ptr(out), len(out)))
        return out[:n]

    def redact_audio(self, clip, rate, text):
        """`clip` without the audio of the bracketed parts of `text` (tts_redact_audio)"""
        clip = np.ascontiguousarray(clip, np.float32)
        out = np.zeros(max(1, len(clip)), np.float32)
        n = self._ck(self.L.tts_redact_audio(self.h, _ptr(clip), len(clip), int(rate), text.encode(), _ptr(out), len(out)))
        return out[:n]

    # ---- HiFi-GAN decoder (not in the reference): latents + speaker latent -> 24 kHz audio ----
    def load_hifigan(self, path):
        self._ck(self.L.tts_load_hifigan(self.h, path.encode()))

    @staticmethod
    def hifigan_samples(L):
        return lib().tts_hifigan_samples(L)

    def hifigan_decode(self, latents_list, voices, voice_of=None):
        """latents_list: list of [L_c, 1024] (the trimmed rows of autoregressive()); voices: [1024] or [V, 1024]; voice_of [B] or None (every
        candidate uses voice 0). Returns a list of float32 waveforms, 256 * frames(L_c) samples each (tts_hifigan_decode: one call)."""
        rows = np.array([len(l) for l in latents_list], np.int32)
        lat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.float32).reshape(-1, DMODEL) for l in latents_list]))
        tab = np.ascontiguousarray(voices, np.float32).reshape(-1, DMODEL)
        idx = None if voice_of is None else np.ascontiguousarray(voice_of, np.int32)
        if idx is not None and len(idx) != len(rows):
            raise TtsError("voice_of names %d candidates, %d given" % (len(idx), len(rows)))
        ns = [self.hifigan_samples(int(r)) for r in rows]
        audio = np.empty(sum(ns), np.float32)
        self._ck(self.L.tts_hifigan_decode(self.h, _ptr(lat), _ptr(rows), len(rows), _ptr(tab), len(tab), _ptr(idx), _ptr(audio)))
        out, off = [], 0
        for n in ns:
            out.append(audio[off:off + n].copy())
            off += n
        return out

    def hifigan_chunk(self, latents_list, voices, frame0, n_frames, voice_of=None):
        """Frames [frame0[c], frame0[c] + n_frames[c]) of every candidate's utterance (latents_list, voices, voice_of as hifigan_decode: the whole latents).
        Returns a list of float32 waveforms, 256 * n_frames[c] samples each, the bits of hifigan_decode's slice (tts_hifigan_chunk: one call)."""
        rows = np.array([len(l) for l in latents_list], np.int32)
        lat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.float32).reshape(-1, DMODEL) for l in latents_list]))
        tab = np.ascontiguousarray(voices, np.float32).reshape(-1, DMODEL)
        idx = None if voice_of is None else np.ascontiguousarray(voice_of, np.int32)
        f0 = np.ascontiguousarray(np.broadcast_to(np.asarray(frame0, np.int32), rows.shape))
        nf = np.ascontiguousarray(np.broadcast_to(np.asarray(n_frames, np.int32), rows.shape))
        if idx is not None and len(idx) != len(rows):
            raise TtsError("voice_of names %d candidates, %d given" % (len(idx), len(rows)))
        audio = np.empty(256 * int(np.maximum(nf, 0).sum()), np.float32)
        self._ck(self.L.tts_hifigan_chunk(self.h, _ptr(lat), _ptr(rows), len(rows), _ptr(tab), len(tab), _ptr(idx), _ptr(f0), _ptr(nf), _ptr(audio)))
        return [a.copy() for a in np.split(audio, np.cumsum(256 * nf)[:-1])]

    def hifigan_stream(self, tokens, voice, max_steps, flags=0, stride=16, on_chunk=None):
        """tts_hifigan_stream: one candidate whose audio leaves while the loop samples. Returns (codes [502], rows, latents [rows, 1024], chunks, steps): chunks
        is the list of (samples, is_last) in arrival order, steps the loop's step count as autoregressive() returns it. on_chunk(samples, is_last) is called
        for each chunk as it arrives; a true return cancels the call (TtsError), and so does an exception it raises, which is raised again here once the
        call has returned."""
        codes = np.empty(502, np.int32)
        rows = np.zeros(1, np.int32)
        steps = np.zeros(1, np.int32)
        lat = np.empty((500, DMODEL), np.float32)
        chunks, raised = [], []

        @AUDIO_CB
        def cb(_user, samples, n, is_last):
            try:  # ctypes would print and swallow an exception that leaves a callback, and the call would go on
                a = np.ctypeslib.as_array(samples, (n,)).copy()
                chunks.append((a, bool(is_last)))
                return 1 if (on_chunk is not None and on_chunk(a, bool(is_last))) else 0
            except BaseException as e:
                raised.append(e)
                return 1

        tok = np.ascontiguousarray(tokens, np.int32)
        v = np.ascontiguousarray(voice, np.float32)
        rc = self.L.tts_hifigan_stream(self.h, _ptr(tok), len(tok), _ptr(v), max_steps, flags, stride, C.cast(cb, C.c_void_p), None, _ptr(codes), _ptr(rows),
                                       _ptr(lat), _ptr(steps))
        if raised:
            raise raised[0]
        self._ck(rc)
        return codes, int(rows[0]), lat[:int(rows[0])].copy(), chunks, int(steps[0])

    def hifigan_stream_recaptures(self):
        return self.L.tts_hifigan_stream_recaptures(self.h)

    # ---- diffusion ----
    @staticmethod
    def frames(L):
        return lib().tts_diffusion_frames(L)

    def diffusion_forward(self, latents, x_t, timestep, conditioning_free):
        latents = np.ascontiguousarray(latents, np.float32).reshape(-1, DMODEL)
        x_t = np.ascontiguousarray(x_t, np.float32)
        T = x_t.shape[1]
        out = np.empty((200, T), np.float32)
        self._ck(self.L.tts_diffusion_forward(self.h, latents.reshape(-1), latents.shape[0], x_t.reshape(-1),
                                              timestep, 1 if conditioning_free else 0, out.reshape(-1)))
        return out

    def diffusion(self, latents_list, n_steps=80, noise=None, noise_mode=NOISE_REFERENCE, voice_latents=None, voice_of_candidate=None):
        """latents_list: list of [L_c,1024]. noise: list of [(n_steps+1), 100*T_c] or None (option diff_sampler = 1 with ddim_eta = 0, and
        diff_sampler = 3: list of x_T [100*T_c]). Returns list of mel [100,T_c]. The sampler, its eta and the guidance strength are engine options (set_option:
        diff_sampler 0 = ancestral DDPM, 1 = DDIM, 3 = DPM-Solver++(2M), deterministic: ddim_eta is checked and not read; ddim_eta; cond_free_k; cond_free 0 =
        unguided, the conditioned sequences only; diff_temperature: x_T = temperature * z_T).
        voice_latents [V, 2048] + voice_of_candidate [B]: candidate c is conditioned on voice_latents[voice_of_candidate[c]] instead of the loaded model's
        latent (tts_diffusion_multi_voice)."""
        rows = np.array([len(l) for l in latents_list], np.int32)
        lat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.float32).reshape(-1, DMODEL) for l in latents_list]))
        Ts = [self.frames(int(r)) for r in rows]
        mel = np.empty(sum(100 * t for t in Ts), np.float32)
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(np.concatenate([np.asarray(n, np.float32).reshape(-1) for n in noise]))
        if voice_latents is None and voice_of_candidate is None:
            self._ck(self.L.tts_diffusion(self.h, lat.reshape(-1), rows, len(rows), n_steps, _ptr(nz), noise_mode, mel))
        else:
            tab, nv, idx = _voice_args(None, voice_latents, voice_of_candidate, 2 * DMODEL)
            self._ck(self.L.tts_diffusion_multi_voice(self.h, lat.reshape(-1), rows, len(rows), _ptr(tab), nv, _ptr(idx), n_steps, _ptr(nz), noise_mode, mel))
        out, off = [], 0
        for t in Ts:
            out.append(mel[off:off + 100 * t].reshape(100, t).copy())
            off += 100 * t
        return out

    def diffusion_last_layout(self):
        """(packed rows, sequences) of the step layout of the last diffusion() call (tts_diffusion_last_layout): 2 sequences per candidate guided, 1 with the
        option cond_free 0."""
        rows, seqs = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.L.tts_diffusion_last_layout(self.h, rows, seqs))
        return int(rows[0]), int(seqs[0])

    # ---- in-flight batching for the diffusion stage: requests join and leave a running layout (tts_diff_session_*) ----
    def diff_session_open(self, max_packed_rows, max_requests):
        """Opens a diffusion session for layouts of up to max_packed_rows rows (host_diff_packed_rows says what a request takes) and max_requests requests.
        The options attn_f32, share_uncond, hoist_integrator, diff_graph and the sampler defaults are read here and hold until diff_session_close()."""
        self._ck(self.L.tts_diff_session_open(self.h, max_packed_rows, max_requests))
        self._diff_frames = {}

    def diff_session_admit(self, latents_list, n_steps=None, sampler=None, ddim_eta=None, cond_free_k=None, voice_latent=None, noise=None, seed=0, cond_free=None,
                           temperature=None):
        """Admits one request: latents_list as in diffusion(); noise: list of [(n_steps+1), 100*T_c] (deterministic DDIM and sampler = 3, DPM-Solver++(2M):
        x_T [100*T_c]) or None = the device generator under `seed`; sampler: SAMPLER_DDPM (0), SAMPLER_DDIM (1) or SAMPLER_DPMPP_2M (3); voice_latent [2048] or None = the loaded model's; cond_free: 1 guided, 0 unguided (the request's conditioned sequences only; host_diff_packed_rows(rows, cond_free) says what it takes); temperature: x_T = temperature * z_T. Arguments left None take the session's pinned value (tts_diff_request_init).
        Returns the request id. The mel diff_session_collect() returns is bit for bit what diffusion() returns for the request alone."""
        req = DiffRequest()
        req.struct_size = C.sizeof(DiffRequest)
        self._ck(self.L.tts_diff_request_init(self.h, C.byref(req)))
        rows = np.array([len(l) for l in latents_list], np.int32)
        lat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.float32).reshape(-1, DMODEL) for l in latents_list]))
        nz = None if noise is None else np.ascontiguousarray(np.concatenate([np.asarray(n, np.float32).reshape(-1) for n in noise]))
        v = None if voice_latent is None else np.ascontiguousarray(voice_latent, np.float32).reshape(2 * DMODEL)
        req.n_cand, req.latents, req.rows, req.voice_latent2048, req.noise, req.seed = len(rows), _ptr(lat), _ptr(rows), _ptr(v), _ptr(nz), seed
        for field, value in (("n_steps", n_steps), ("sampler", sampler), ("ddim_eta", ddim_eta), ("cond_free_k", cond_free_k), ("temperature", temperature),
                             ("cond_free", None if cond_free is None else int(cond_free))):
            if value is not None:
                setattr(req, field, value)
        rid = self._ck(self.L.tts_diff_session_admit(self.h, C.byref(req)))
        self._diff_frames[rid] = [self.frames(int(r)) for r in rows]
        return rid

    def diff_session_room(self):
        return self._ck(self.L.tts_diff_session_room(self.h))

    def diff_session_step(self):
        """One sampling step for every running request, each at its own step; returns how many are still running."""
        return self._ck(self.L.tts_diff_session_step(self.h))

    def diff_session_finished(self):
        out = np.zeros(4096, np.int32)
        n = self._ck(self.L.tts_diff_session_finished(self.h, _ptr(out), len(out)))
        return [int(x) for x in out[:n]]

    def diff_session_collect(self, request):
        """A finished request's list of mel [100, T_c]; the request leaves the session."""
        Ts = self._diff_frames.get(request) or []  # an id this engine never admitted: the library refuses it
        mel = np.empty(max(1, sum(100 * t for t in Ts)), np.float32)
        self._ck(self.L.tts_diff_session_collect(self.h, request, _ptr(mel)))
        self._diff_frames.pop(request, None)
        out, off = [], 0
        for t in Ts:
            out.append(mel[off:off + 100 * t].reshape(100, t).copy())
            off += 100 * t
        return out

    def diff_session_cancel(self, request):
        self._ck(self.L.tts_diff_session_cancel(self.h, request))
        self._diff_frames.pop(request, None)

    def diff_session_close(self):
        self._ck(self.L.tts_diff_session_close(self.h))
        self._diff_frames = {}

    def diff_session_captures(self):
        return self._ck(self.L.tts_diff_session_captures(self.h))

    # ---- vocoder ----
    def vocoder(self, mels, noise=None, noise_mode=NOISE_REFERENCE):
        frames = np.array([m.shape[1] for m in mels], np.int32)
        mel = np.ascontiguousarray(np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in mels]))
        ns = [self.L.tts_vocoder_samples(int(t)) for t in frames]
        audio = np.empty(sum(ns), np.float32)
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(np.concatenate([np.asarray(n, np.float32).reshape(-1) for n in noise]))
        self._ck(self.L.tts_vocoder(self.h, mel, frames, len(frames), _ptr(nz), noise_mode, audio))
        out, off = [], 0
        for n in ns:
            out.append(audio[off:off + n].copy())
            off += n
        return out

    def vocoder_chunk(self, mel, noise, frame0, n_frames):
        """Samples of frames [frame0, frame0 + n_frames) of one utterance (mel [100,T], noise [64,T+10] of the whole utterance)."""
        mel = np.ascontiguousarray(mel, np.float32)
        noise = np.ascontiguousarray(noise, np.float32)
        out = np.empty(n_frames * 256, np.float32)
        n = C.c_int(0)
        self._ck(self.L.tts_vocoder_chunk(self.h, mel.reshape(-1), mel.shape[1], noise.reshape(-1), frame0, n_frames, out, C.byref(n)))
        return out[:n.value].copy()

    # ---- profiling ----
    def prof_reset(self, enable=True):
        self.L.tts_prof_reset(self.h, 1 if enable else 0)

    def prof_get(self, family):
        """(device ms, launches, algorithmic work) of a kernel family since prof_reset."""
        ms, n, w = C.c_double(0), C.c_int64(0), C.c_double(0)
        self.L.tts_prof_get(self.h, family.encode(), C.byref(ms), C.byref(n), C.byref(w))
        return ms.value, n.value, w.value


HOST_SCHED_KEYS = ["max_log", "min_log", "cfk", "sqrt_recip", "sqrt_recipm1", "coef1", "coef2"]


def host_schedule(n_steps):
    """The diffusion driver's respaced schedule and per-step scalars (host arithmetic, no device needed)."""
    tm = np.empty(n_steps, np.int32)
    arrs = [np.empty(n_steps, np.float32) for _ in HOST_SCHED_KEYS]
    rc = lib().tts_host_schedule(n_steps, tm, *arrs)
    if rc:
        raise TtsError("tts_host_schedule failed (%d)" % rc)
    return tm, dict(zip(HOST_SCHED_KEYS, arrs))


def host_schedule_ddim(n_steps, eta=0.0):
    """The DDIM scalars of option diff_sampler = 1 (host arithmetic, no device needed), index = respaced t: dict of acp, acp_prev (float64), c_x0, c_eps,
    sigma (float32)."""
    acp, prev = np.empty(n_steps, np.float64), np.empty(n_steps, np.float64)
    f = [np.empty(n_steps, np.float32) for _ in range(3)]
    rc = lib().tts_host_schedule_ddim(n_steps, float(eta), acp, prev, *f)
    if rc:
        raise TtsError("tts_host_schedule_ddim failed (%d)" % rc)
    return dict(acp=acp, acp_prev=prev, c_x0=f[0], c_eps=f[1], sigma=f[2])


def host_schedule_dpmpp(n_steps):
    """The DPM-Solver++(2M) scalars of option diff_sampler = 3 (host arithmetic, no device needed), index = respaced t: dict of a, b, c (float32) and order (int32;
    1 at t = n_steps - 1, 1 and 0, else 2): x_next = a x + b x0 + c x0_prev."""
    f = [np.empty(n_steps, np.float32) for _ in range(3)]
    order = np.empty(n_steps, np.int32)
    rc = lib().tts_host_schedule_dpmpp(n_steps, *f, order)
    if rc:
        raise TtsError("tts_host_schedule_dpmpp failed (%d)" % rc)
    return dict(a=f[0], b=f[1], c=f[2], order=order)


def host_timestep_embedding(t):
    out = np.empty(1024, np.float32)
    lib().tts_host_timestep_embedding(int(t), out)
    return out


def host_sample_row(row, ids, uniform):
    """The sampler's pure per-candidate function on a full logits row (host_logic.cpp: sample_one)."""
    ids = np.ascontiguousarray(ids, np.int32)
    return lib().tts_host_sample_row(np.ascontiguousarray(row, np.float32), ids, len(ids), float(uniform))


def host_sample_prefiltered(row, ids, uniform, keep=64):
    """The same from a host restatement of the device prefilter's list (the `keep` largest logits + ties of the smallest). -1: the list
    cannot decide and the engine would fetch the full row."""
    ids = np.ascontiguousarray(ids, np.int32)
    return lib().tts_host_sample_prefiltered(np.ascontiguousarray(row, np.float32), ids, len(ids), float(uniform), keep)


def host_sample_row_ex(row, ids, uniform, temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, mode=0):
    """host_sample_row with the sampler's controls explicit. mode 0: the production path (fast scan, literal fallback); 1: the literal formulation only."""
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    return lib().tts_host_sample_row_ex(np.ascontiguousarray(row, np.float32), ids, len(ids), float(uniform), float(temperature), int(top_k), float(top_p),
                                        float(penalty), int(mode))


def host_sample_prefiltered_ex(row, ids, uniform, temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, keep=64, already_penalised=False):
    """host_sample_prefiltered with the controls explicit. already_penalised: the list is taken from the penalised row (penalty scope 1). -1: the engine
    would fetch the full row."""
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    return lib().tts_host_sample_prefiltered_ex(np.ascontiguousarray(row, np.float32), ids, len(ids), float(uniform), float(temperature), int(top_k),
                                                float(top_p), float(penalty), int(keep), int(bool(already_penalised)))


def host_typical_keep(row, mass):
    """The literal typical set of a (penalised) row [8194] at `mass` (narrowed to float, as the option is): a bool array [8194]."""
    keep = np.zeros(VOCAB_MEL, np.uint8)
    n = lib().tts_host_typical_keep(np.ascontiguousarray(row, np.float32), float(mass), _ptr(keep))
    if n < 0:
        raise TtsError("tts_host_typical_keep refused its arguments (%d)" % n)
    assert n == int(keep.sum())
    return keep.astype(bool)


def host_sample_row_typical(row, ids, uniform, temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, typical_mass=0.0, mode=0):
    """host_sample_row_ex with the typical stage between the penalty and the temperature (typical_mass 0: that very call)."""
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    return lib().tts_host_sample_row_typical(np.ascontiguousarray(row, np.float32), ids, len(ids), float(uniform), float(temperature), int(top_k), float(top_p),
                                             float(penalty), float(typical_mass), int(mode))


def host_sample_prefiltered_typical(row, ids, uniform, temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, typical_mass=0.0, keep=64):
    """The list path under typical sampling: the host builds the list as the device does (penalised row, the typical set under the device's decision rule)
    and runs the list tail. -1: the engine would fetch the full row."""
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    return lib().tts_host_sample_prefiltered_typical(np.ascontiguousarray(row, np.float32), ids, len(ids), float(uniform), float(temperature), int(top_k),
                                                     float(top_p), float(penalty), float(typical_mass), int(keep))


def host_rel_buckets(n):
    L = lib()
    return np.array([[L.tts_host_rel_bucket(i, c) for c in range(n)] for i in range(n)], np.int32)


def host_pad_codes(codes):
    codes = np.ascontiguousarray(codes, np.int32)
    out = np.empty(502, np.int32)
    rc = lib().tts_host_pad_codes(codes, len(codes), out)
    if rc:
        raise TtsError("tts_host_pad_codes failed (%d)" % rc)
    return out


def host_ar_score_rows(codes, positions="decode"):
    """The row table of tts_ar_score_codes for one candidate (tts_host_ar_score_rows; pure): (input_ids, mel_pos, targets), each [len(codes) + 1]."""
    if positions not in SCORE_POSITIONS:
        raise TtsError("positions %r: 'decode' or 'train'" % (positions,))
    codes = np.ascontiguousarray(codes, np.int32).reshape(-1)
    ids, pos, tgt = (np.zeros(len(codes) + 1, np.int32) for _ in range(3))
    rc = lib().tts_host_ar_score_rows(_ptr(codes), len(codes), SCORE_POSITIONS[positions], _ptr(ids), _ptr(pos), _ptr(tgt))
    if rc:
        _host_fail("tts_host_ar_score_rows", rc)
    return ids, pos, tgt


def _prompt_args(prompts, n_cand):
    lens = np.array([len(p) for p in prompts], np.int32)
    ids = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32).reshape(-1) for p in prompts]) if len(prompts) else np.zeros(0, np.int32), np.int32)
    nc = np.ascontiguousarray(np.broadcast_to(np.asarray(n_cand, np.int32), lens.shape) if np.ndim(n_cand) == 0 else np.asarray(n_cand, np.int32), np.int32)
    return ids, lens, nc


def _voice_args(voice, voices, index, width):
    """(table [V, width] or None, V, indices or None) for the multi-voice entry points. Nothing is checked here beyond the row width: a missing table or index
    list, an index out of range and a non-finite value are the library's to refuse (TTS_ERR_ARG)."""
    if voices is None and voice is not None:
        voices = np.asarray(voice, np.float32).reshape(1, -1)
    tab = None if voices is None else np.ascontiguousarray(voices, np.float32).reshape(-1, width)
    idx = None if index is None else np.ascontiguousarray(index, np.int32).reshape(-1)
    return tab, (0 if tab is None else tab.shape[0]), idx


def host_ar_stop_run(n_cand, samples, max_steps, flags=0, stop_at=None):
    """tts_autoregressive_multi's stop bookkeeping on scripted samples [max_steps, B] (no device). Returns (status, codes [B,502], stopped [B], steps,
    inputs [max_steps, B]: the tokens fed to the decode step after each iteration)."""
    nc = np.ascontiguousarray(n_cand, np.int32)
    B = int(nc.sum())
    smp = np.ascontiguousarray(samples, np.int32).reshape(max_steps, B)
    sa = None if stop_at is None else np.ascontiguousarray(stop_at, np.int32)
    codes = np.zeros((B, 502), np.int32)
    stopped = np.zeros(B, np.int32)
    steps = np.zeros(1, np.int32)
    inputs = np.full((max_steps, B), -1, np.int32)
    rc = lib().tts_host_ar_stop_run(nc, len(nc), smp.reshape(-1), max_steps, flags, _ptr(sa), codes.reshape(-1), stopped, steps, _ptr(inputs))
    return rc, codes, stopped, int(steps[0]), inputs


def host_ar_request_check(max_cand, max_steps, struct_size=None, n_cand=1, seed=0, req_max_steps=0, temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, scope=0,
                          typical_mass=0.0):
    """The status tts_ar_session_admit_ex's descriptor checks return for these fields in a session of max_cand candidates and max_steps steps (no GPU)."""
    req = ArRequest(C.sizeof(ArRequest) if struct_size is None else struct_size, n_cand, seed, req_max_steps, None, temperature, top_k, top_p, penalty, scope,
                    typical_mass)
    return lib().tts_host_ar_request_check(C.byref(req), max_cand, max_steps)


def host_diff_packed_rows(latent_rows, cond_free=True):
    """Packed rows a diffusion-session request of these latent row counts takes (conditioned + unconditioned sequences, Layout::build's rule; no GPU).
    cond_free False / 0: an unguided request, the conditioned sequences only (tts_host_diff_packed_rows_ex)."""
    r = np.ascontiguousarray(latent_rows, np.int32).reshape(-1)
    if cond_free is True or cond_free == 1:
        return lib().tts_host_diff_packed_rows(_ptr(r), len(r))
    return lib().tts_host_diff_packed_rows_ex(_ptr(r), len(r), int(cond_free))


def host_diff_request_check(max_packed_rows, latents=None, rows=None, n_cand=None, n_steps=80, sampler=0, ddim_eta=0.0, cond_free_k=2.0, voice=None, struct_size=None,
                            null_latents=False, null_rows=False, cond_free=1, temperature=1.0):
    """The status tts_diff_session_admit's descriptor checks return for these fields in a session with max_packed_rows free rows (no GPU). latents: list of
    [L_c, 1024]; rows / n_cand override what the list implies. sampler: 0, 1 or 3 (DPM-Solver++(2M)) pass, as for tts_set_option("diff_sampler")."""
    lat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.float32).reshape(-1, DMODEL) for l in latents]))
    rw = np.ascontiguousarray([len(l) for l in latents] if rows is None else rows, np.int32)
    v = None if voice is None else np.ascontiguousarray(voice, np.float32).reshape(2 * DMODEL)
    req = DiffRequest(C.sizeof(DiffRequest) if struct_size is None else struct_size, len(latents) if n_cand is None else n_cand, None if null_latents else _ptr(lat),
                      None if null_rows else _ptr(rw), _ptr(v), n_steps, int(sampler), ddim_eta, cond_free_k, None, 0, temperature, 0)
    req.cond_free = int(cond_free)
    return lib().tts_host_diff_request_check(C.byref(req), max_packed_rows)


def host_session_first_fit(busy, n_cand):
    """The session allocator's rule: the first index of the lowest run of n_cand free slots of the busy map, or -1."""
    b = np.ascontiguousarray(busy, np.uint8)
    return lib().tts_host_session_first_fit(_ptr(b), len(b), n_cand)


def host_trimmed_rows(codes502):
    return lib().tts_host_trimmed_rows(np.ascontiguousarray(codes502, np.int32))


def host_mel_diffusion100(audio24k, normalize=False):
    """[100, frames] log-mel of 24 kHz audio. normalize=False: log(clamp(mel, 1e-5)), the input of Engine.diffusion_conditioning_latent
    (upstream feeds its contextual_embedder the un-normalised mel); normalize=True: mapped to [-1, 1] like the diffusion stage's output."""
    a = np.ascontiguousarray(audio24k, np.float32)
    frames = lib().tts_host_mel_frames(len(a))
    out = np.empty((100, frames), np.float32)
    rc = lib().tts_host_mel_diffusion100(a, len(a), 1 if normalize else 0, out.reshape(-1))
    if rc < 0:
        raise TtsError("tts_host_mel_diffusion100 failed (%d): the clip must be longer than 512 samples" % rc)
    return out


def host_mel_voice80(audio22k, mel_norms=None):
    """[80, frames] log-mel of 22.05 kHz audio (divided per band by mel_norms if given): the input of Engine.voice_latent."""
    a = np.ascontiguousarray(audio22k, np.float32)
    frames = lib().tts_host_mel_frames(len(a))
    out = np.empty((80, frames), np.float32)
    mn = None if mel_norms is None else np.ascontiguousarray(mel_norms, np.float32).reshape(80)
    rc = lib().tts_host_mel_voice80(a, len(a), _ptr(mn), out.reshape(-1))
    if rc < 0:
        raise TtsError("tts_host_mel_voice80 failed (%d): the clip must be longer than 512 samples" % rc)
    return out


def host_fp8_e4m3(values):
    """OCP fp8 e4m3 codes (uint8) of an array of floats: the quantiser of option ar_weights = 2."""
    L = lib()
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    return np.array([L.tts_host_fp8_e4m3(float(x)) for x in v], np.uint8).reshape(np.shape(values))


# ---- the host rules of alignment and redaction (tts_host_*; no context, no GPU). A failure raises TtsError whose .status is the C status. ----
def _host_fail(what, rc):
    e = TtsError("%s failed (status %d)" % (what, rc))
    e.status = rc
    raise e


def host_ctc_decode(ids, vocab, blank):
    ids, vocab = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vocab, np.int32)
    buf = C.create_string_buffer(4 * len(ids) + 1)
    rc = lib().tts_host_ctc_decode(_ptr(ids), len(ids), _ptr(vocab), len(vocab), int(blank), buf, len(buf))
    if rc < 0:
        _host_fail("tts_host_ctc_decode", rc)
    return buf.raw[:rc].decode()


def host_max_alignment(s1, s2):
    buf = C.create_string_buffer(4 * len(s1) + 1)
    rc = lib().tts_host_max_alignment(s1.encode(), s2.encode(), buf, len(buf))
    if rc < 0:
        _host_fail("tts_host_max_alignment", rc)
    return buf.raw[:rc].decode()


def host_ctc_align(ids, vocab, blank, text, n_samples):
    ids, vocab = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vocab, np.int32)
    out = np.zeros(max(1, len(text)), np.int64)
    rc = lib().tts_host_ctc_align(_ptr(ids), len(ids), _ptr(vocab), len(vocab), int(blank), text.encode(), int(n_samples), _ptr(out), len(out))
    if rc < 0:
        _host_fail("tts_host_ctc_align", rc)
    return out[:rc]


def host_redact_spans(text):
    """(text without brackets, [(first char, last char), ...] of the kept pieces)"""
    buf = C.create_string_buffer(4 * len(text) + 1)
    iv = np.zeros((len(text) + 1, 2), np.int32)
    rc = lib().tts_host_redact_spans(text.encode(), buf, len(buf), _ptr(iv), len(iv))
    if rc < 0:
        _host_fail("tts_host_redact_spans", rc)
    return buf.value.decode(), [tuple(int(v) for v in r) for r in iv[:rc]]


def host_blend_voices(latents, weights=None):
    """upstream's load_voices rule for several voices, the mean of their latents, with optional weights (tts_host_blend_voices): latents [n, dim] -> [dim]"""
    x = np.ascontiguousarray(latents, np.float32)
    if x.ndim != 2:
        raise TtsError("latents: [n, dim] expected, got shape %s" % (x.shape,))
    w = None if weights is None else np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w is not None and len(w) != len(x):
        raise TtsError("%d weights for %d voices" % (len(w), len(x)))
    out = np.empty(x.shape[1], np.float32)
    rc = lib().tts_host_blend_voices(_ptr(x), _ptr(w), x.shape[0], x.shape[1], _ptr(out))
    if rc < 0:
        _host_fail("tts_host_blend_voices", rc)
    return out


def host_random_voice_fold(w, b, equal=True):
    """the loader's fold of one random-voice layer (tts_host_random_voice_fold): (w * scale, b * lr_mul) in float32, or copies for the last layer"""
    w, b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    wo, bo = np.empty_like(w), np.empty_like(b)
    rc = lib().tts_host_random_voice_fold(_ptr(w), _ptr(b), len(b), int(bool(equal)), _ptr(wo), _ptr(bo))
    if rc < 0:
        _host_fail("tts_host_random_voice_fold", rc)
    return wo, bo


def read_wav(path):
    """(mono float32 samples, sample rate) of a RIFF/WAVE file with PCM16, PCM24 or float32 samples (tts_read_wav); TtsError carries the status."""
    rate = C.c_int32(0)
    n = lib().tts_read_wav(path.encode(), None, 0, C.byref(rate))
    if n < 0:
        raise TtsError("tts_read_wav(%s) failed (status %d)" % (path, n))
    out = np.empty(n, np.float32)
    n = lib().tts_read_wav(path.encode(), _ptr(out), n, C.byref(rate))
    if n < 0:
        raise TtsError("tts_read_wav(%s) failed (status %d)" % (path, n))
    return out[:n], int(rate.value)


def write_wav(path, samples, rate=24000):
    s = np.ascontiguousarray(samples, np.float32)
    return lib().tts_write_wav(path.encode(), s, len(s), rate)
