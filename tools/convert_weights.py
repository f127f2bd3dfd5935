#!/usr/bin/env python3
"""PyTorch checkpoints of tortoise-tts -> the reference's weight container.

The reference's README promises export scripts that are not in its repository (/root/reference/README.md:34, 77); its loaders
(main.cpp:682-792, 1244-1536, 1808-1923) define the contract: legacy-ggml container (magic 0x67676d6c, F32 records,
no alignment), tensor names = the PyTorch state_dict keys of the inference modules, PyTorch dim order reversed into ne[], k = 1
convolutions stored squeezed to 2-D. This tool produces exactly that from

  autoregressive.pth      UnifiedVoice state dict. Either the `inference_model.*` keys (GPT2InferenceModel, present after
                          post_init_gpt2_config) or the training-time names (gpt.h.N..., gpt.ln_f, final_norm, mel_head), which are mapped.
  diffusion_decoder.pth   DiffusionTts state dict (+ --diffusion-conditioning-latent: the [1, 2048] diffusion conditioning latent of the
                          voice, which the reference bakes into the file as `diffusion_conditioning_latent`).
  vocoder.pth             UnivNet generator state dict (optionally under 'model_g'); weight_norm parametrisations (weight_g / weight_v) are fused.

    python tools/convert_weights.py --ar autoregressive.pth --diffusion diffusion_decoder.pth --diffusion-conditioning-latent voice_diff.pth \\
                                    --vocoder vocoder.pth --out models/

The trained checkpoints are not available offline: tests/test_convert_weights.py round-trips synthetic weights through PyTorch-style state
dicts (3-D k=1 convs, weight_norm pairs, training-time AR names) and requires the converter to reproduce the original container.
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tortoise_cpp_amd_loader  # noqa: E402

tortoise_cpp_amd_loader.load()
from tortoise_cpp_amd.synth_weights import (GgmlWriter, aligner_tensor_shapes, bigvgan_filter, bigvgan_tensor_shapes, classifier_tensor_shapes,  # noqa: E402
                                            dvae_tensor_shapes, random_voice_tensor_shapes)


def _np(t):
    return t.detach().cpu().float().numpy() if hasattr(t, "detach") else np.asarray(t, np.float32)


def fuse_weight_norm(sd):
    """weight = g * v / ||v|| (norm over every dim but 0: torch.nn.utils.weight_norm's default dim=0)."""
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_g"):
            base = k[:-len(".weight_g")]
            g, w = _np(v), _np(sd[base + ".weight_v"])
            norm = np.sqrt((w.astype(np.float64) ** 2).sum(axis=tuple(range(1, w.ndim)), keepdims=True))
            out[base + ".weight"] = (g.astype(np.float64) * w / norm).astype(np.float32)
        elif k.endswith(".weight_v"):
            continue
        else:
            out[k] = _np(v)
    return out


# ---- autoregressive (main.cpp:682-792) --------------------------------------------------------------------------------------------
AR_GLOBAL = ["text_embedding.weight", "text_pos_embedding.emb.weight", "mel_embedding.weight", "mel_pos_embedding.emb.weight"]
AR_TRAIN_TO_INFER = [(r"^gpt\.h\.", "inference_model.transformer.h."), (r"^gpt\.ln_f\.", "inference_model.transformer.ln_f."),
                     (r"^final_norm\.", "inference_model.lm_head.0."), (r"^mel_head\.", "inference_model.lm_head.1.")]
AR_LAYER = ["ln_1.weight", "ln_1.bias", "attn.c_attn.weight", "attn.c_attn.bias", "attn.c_proj.weight", "attn.c_proj.bias", "ln_2.weight",
            "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias"]


def convert_ar(sd, path):
    sd = {k: _np(v) for k, v in sd.items()}
    if not any(k.startswith("inference_model.") for k in sd):
        for k in list(sd):
            for pat, rep in AR_TRAIN_TO_INFER:
                if re.match(pat, k):
                    sd[re.sub(pat, rep, k)] = sd[k]
    w = GgmlWriter(path)
    for k in AR_GLOBAL:
        w.add(k, sd[k])
    n = 0
    while "inference_model.transformer.h.%d.ln_1.weight" % n in sd:
        for t in AR_LAYER:
            w.add("inference_model.transformer.h.%d.%s" % (n, t), sd["inference_model.transformer.h.%d.%s" % (n, t)])
        n += 1
    for k in ("inference_model.transformer.ln_f.weight", "inference_model.transformer.ln_f.bias", "inference_model.lm_head.0.weight",
              "inference_model.lm_head.0.bias", "inference_model.lm_head.1.weight", "inference_model.lm_head.1.bias"):
        w.add(k, sd[k])
    w.close()
    return n


# ---- diffusion (main.cpp:1244-1536) -----------------------------------------------------------------------------------------------
def _attn_names(p):
    return [p + s for s in (".norm.weight", ".norm.bias", ".qkv.weight", ".qkv.bias", ".proj_out.weight", ".proj_out.bias",
                            ".relative_pos_embeddings.relative_attention_bias.weight")]


def _res_names(p):
    return [p + s for s in (".in_layers.0.weight", ".in_layers.0.bias", ".in_layers.2.weight", ".in_layers.2.bias", ".emb_layers.1.weight",
                            ".emb_layers.1.bias", ".out_layers.0.weight", ".out_layers.0.bias", ".out_layers.3.weight", ".out_layers.3.bias")]


SQUEEZE_K1 = re.compile(r"(\.qkv\.weight|\.proj_out\.weight|\.in_layers\.2\.weight|^integrating_conv\.weight)$")


def convert_diffusion(sd, cond_latent, path):
    sd = {k: _np(v) for k, v in sd.items()}
    names = ["latent_conditioner.0.weight", "latent_conditioner.0.bias"]
    n_lc = 0
    while "latent_conditioner.%d.norm.weight" % (n_lc + 1) in sd:
        n_lc += 1
        names += _attn_names("latent_conditioner.%d" % n_lc)
    names += ["code_norm.weight", "code_norm.bias", "time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight", "time_embed.2.bias"]
    n_integ = 0
    while "conditioning_timestep_integrator.%d.resblk.in_layers.0.weight" % n_integ in sd:
        names += _res_names("conditioning_timestep_integrator.%d.resblk" % n_integ) + _attn_names("conditioning_timestep_integrator.%d.attn" % n_integ)
        n_integ += 1
    names += ["inp_block.weight", "inp_block.bias", "integrating_conv.weight", "integrating_conv.bias"]
    n_main = 0
    while "layers.%d.resblk.in_layers.0.weight" % n_main in sd:
        names += _res_names("layers.%d.resblk" % n_main) + _attn_names("layers.%d.attn" % n_main)
        n_main += 1
    n_tail = 0
    while "layers.%d.in_layers.0.weight" % (n_main + n_tail) in sd:
        names += _res_names("layers.%d" % (n_main + n_tail))
        n_tail += 1
    names += ["out.0.weight", "out.0.bias", "out.2.weight", "out.2.bias"]
    w = GgmlWriter(path)
    w.add("diffusion_conditioning_latent", _np(cond_latent).reshape(1, 2048))
    for k in names:
        t = sd[k]
        if SQUEEZE_K1.search(k) and t.ndim == 3:  # k = 1 convolutions are stored 2-D (main.cpp:1260, 1308, 1379)
            assert t.shape[2] == 1, (k, t.shape)
            t = t[:, :, 0]
        w.add(k, t)
    w.add("unconditioned_embedding", sd["unconditioned_embedding"].reshape(-1))
    w.close()
    return n_lc, n_integ, n_main, n_tail


# ---- vocoder (main.cpp:1808-1923) -------------------------------------------------------------------------------------------------
def convert_vocoder(sd, path):
    if "model_g" in sd:
        sd = sd["model_g"]
    sd = fuse_weight_norm(sd)
    w = GgmlWriter(path)
    for k in ("conv_pre.weight", "conv_pre.bias"):
        w.add(k, sd[k])
    i = 0
    while "res_stack.%d.convt_pre.1.weight" % i in sd:
        p = "res_stack.%d." % i
        kp = p + "kernel_predictor."
        names = [kp + "input_conv.0.weight", kp + "input_conv.0.bias"]
        c = 0
        while kp + "residual_convs.%d.1.weight" % c in sd:
            for j in (1, 3):
                names += [kp + "residual_convs.%d.%d.weight" % (c, j), kp + "residual_convs.%d.%d.bias" % (c, j)]
            c += 1
        names += [kp + "kernel_conv.weight", kp + "kernel_conv.bias", kp + "bias_conv.weight", kp + "bias_conv.bias", p + "convt_pre.1.weight",
                  p + "convt_pre.1.bias"]
        c = 0
        while p + "conv_blocks.%d.1.weight" % c in sd:
            names += [p + "conv_blocks.%d.1.weight" % c, p + "conv_blocks.%d.1.bias" % c]
            c += 1
        for k in names:
            w.add(k, sd[k])
        i += 1
    post = sd["conv_post.1.weight"]
    w.add("conv_post.1.weight", post.reshape(post.shape[-2], post.shape[-1]))  # [1, 32, 7] -> [32, 7] (main.cpp:1919-1923)
    w.add("conv_post.1.bias", sd["conv_post.1.bias"])
    w.close()
    return i


def convert_conditioning_encoder(sd, path):
    """ggml-conditioning-model.bin for tts_load_voice_encoder: the `conditioning_encoder.*` tensors of upstream tortoise-tts' autoregressive.pth
    (the tensors convert_ar leaves out: the reference reads the finished voice latent from a file), under their state-dict names."""
    w = GgmlWriter(path)
    n = 0
    for k in sorted(sd):
        if k.startswith("conditioning_encoder."):
            if ".relative_pos_embeddings." in k:
                raise SystemExit("convert_conditioning_encoder: '%s' — an encoder with relative position embeddings is not the UnifiedVoice one" % k)
            w.add(k, _np(sd[k]))
            n += k.endswith(".norm.weight")
    w.close()
    if n == 0:
        raise SystemExit("convert_conditioning_encoder: no conditioning_encoder.* tensors in the checkpoint")
    return n


def convert_diffusion_conditioning_encoder(sd, path):
    """ggml-diffusion-conditioning-model.bin for tts_load_diffusion_conditioning_encoder: the `contextual_embedder.*` tensors of upstream
    tortoise-tts' diffusion_decoder.pth (left out of ggml-diffusion-model.bin, which carries one voice's finished latent instead)."""
    w = GgmlWriter(path)
    n = 0
    for k in sorted(sd):
        if k.startswith("contextual_embedder."):
            w.add(k, _np(sd[k]))
            n += k.endswith(".norm.weight")
    w.close()
    if n == 0:
        raise SystemExit("convert_diffusion_conditioning_encoder: no contextual_embedder.* tensors in the checkpoint")
    return n


def convert_clvp(sd, path):
    """ggml-clvp-model.bin for tts_load_clvp: upstream tortoise-tts CLVP (clvp2.pth, use_xformers=True), tensors under their state-dict names.
    Kept: embeddings, latent projections, temperature (0-dim -> [1]), every `*.attn_layers.layers.N.{0.g, 1.*}` parameter and the final norms;
    the rotary inv_freq buffers are recomputed by the loader (kept if present); anything else (e.g. positional embeddings of the non-xformers
    variant) is an error, so that a checkpoint of the other CLVP flavour is not silently mis-read."""
    w = GgmlWriter(path)
    depth = 0
    for k in sorted(sd):
        v = _np(sd[k])
        known = (k in ("text_emb.weight", "speech_emb.weight", "to_text_latent.weight", "to_speech_latent.weight", "temperature")
                 or ".attn_layers.layers." in k or k.endswith((".transformer.norm.weight", ".transformer.norm.bias", "rotary_pos_emb.inv_freq")))
        if not known:
            raise SystemExit("convert_clvp: unexpected tensor '%s' (not the use_xformers=True CLVP of tortoise-tts?)" % k)
        if k == "temperature":
            v = v.reshape(1)
        if k.startswith("text_transformer.") and k.endswith(".0.g"):
            depth += 1
        w.add(k, v)
    w.close()
    return depth // 2


def strip_wrap(sd):
    """upstream's checkpoint wrapper puts a `.wrap.` component into the names of wrapped modules: the same tensors under the plain names"""
    out = {}
    for k, v in sd.items():
        k2 = k.replace(".wrap.", ".")
        if k2 in out:
            raise SystemExit("convert_cvvp: '%s' appears with and without .wrap." % k2)
        out[k2] = v
    return out


def convert_cvvp(sd, path):
    """ggml-cvvp-model.bin for tts_load_cvvp: upstream tortoise-tts CVVP (cvvp.pth), tensors under their state-dict names (a `.wrap.` path component is
    stripped; temperature 0-dim -> [1]; the rotary inv_freq buffers are kept if present, the loader recomputes them). A missing, unknown or mis-shaped tensor is
    an error: the names and shapes are restated from memory (--list-expected cvvp), so a real checkpoint that differs must be seen, not mis-read."""
    sd = {k: _np(v) for k, v in strip_wrap(sd).items()}
    depth = 0
    while "speech_transformer.transformer.attn_layers.layers.%d.0.g" % (2 * depth) in sd:
        depth += 1
    if depth == 0:
        raise SystemExit("convert_cvvp: no speech_transformer layers (not the CVVP of tortoise-tts?)")
    dim = sd["speech_emb.emb.weight"].shape[1] if "speech_emb.emb.weight" in sd else 512
    exp = expected_tensors("cvvp", depth=depth, dim=dim)
    for k in sorted(sd):
        if k not in exp and not k.endswith("rotary_pos_emb.inv_freq"):
            raise SystemExit("convert_cvvp: unexpected tensor '%s' (not the CVVP of tortoise-tts?)" % k)
    w = GgmlWriter(path)
    for k, shape in exp.items():
        if k not in sd:
            raise SystemExit("convert_cvvp: tensor '%s' is missing" % k)
        if tuple(sd[k].shape) != tuple(shape):
            raise SystemExit("convert_cvvp: tensor '%s' has shape %s, expected %s" % (k, list(sd[k].shape), list(shape)))
        w.add(k, sd[k].reshape(container_shape("cvvp", k, shape)))
    for k in sorted(sd):
        if k.endswith("rotary_pos_emb.inv_freq"):
            w.add(k, sd[k])
    w.close()
    return depth


def convert_bigvgan(sd, path):
    """ggml-bigvgan-model.bin for tts_load_bigvgan: NVIDIA BigVGAN v1's generator (bigvgan_base_24khz_100band / bigvgan_24khz_100band; the state dict, or the one
    under 'generator'), tensors under their state-dict names with the prefix `bigvgan.`. weight_g / weight_v are folded where present. The activations' fixed
    low-pass buffers (`*.upsample.filter`, `*.downsample.lowpass.filter`) are not stored: each is checked against the closed form the kernels hold
    (synth_weights.bigvgan_filter) to 1e-6 and dropped. C0 and the strides are read from the shapes; a missing, unknown or mis-shaped tensor is an error: the
    names and shapes are restated from memory (--list-expected bigvgan), so a real checkpoint that differs must be seen, not mis-read."""
    sd = fuse_weight_norm(sd["generator"] if "generator" in sd else sd)
    f = bigvgan_filter()
    for k in [k for k in sd if k.endswith(".filter")]:
        v = sd.pop(k).astype(np.float64).reshape(-1)
        if v.shape != (12,) or np.abs(v - f).max() > 1e-6:
            raise SystemExit("convert_bigvgan: buffer '%s' is not the 12-tap Kaiser-windowed sinc the kernels hold (largest difference %s)"
                             % (k, np.abs(v - f).max() if v.shape == (12,) else "shape %s" % list(v.shape)))
    if "conv_pre.weight" not in sd or sd["conv_pre.weight"].ndim != 3:
        raise SystemExit("convert_bigvgan: no conv_pre.weight (not a BigVGAN generator?)")
    c0, rates = sd["conv_pre.weight"].shape[0], []
    while "ups.%d.0.weight" % len(rates) in sd and len(rates) < 6:
        rates.append(sd["ups.%d.0.weight" % len(rates)].shape[-1] // 2)
    if int(np.prod(rates or [0])) != 256 or c0 % (1 << len(rates)):
        raise SystemExit("convert_bigvgan: %d channels and strides %s: the strides must multiply to 256 (BigVGAN v1, 24 kHz, hop 256)" % (c0, rates))
    exp = bigvgan_tensor_shapes(c0, tuple(rates))
    for k in sorted(sd):
        if "bigvgan." + k not in exp:
            raise SystemExit("convert_bigvgan: unexpected tensor '%s'" % k)
    w = GgmlWriter(path)
    for name, shape in exp.items():
        k = name[len("bigvgan."):]
        if k not in sd:
            raise SystemExit("convert_bigvgan: tensor '%s' is missing" % k)
        if tuple(sd[k].shape) != tuple(shape):
            raise SystemExit("convert_bigvgan: tensor '%s' has shape %s, expected %s" % (k, list(sd[k].shape), list(shape)))
        w.add(name, sd[k])
    w.close()
    return c0, tuple(rates)


def classifier_arch(sd):
    """(b0, depth, K, E, rb, attn) of a classifier state dict, read from its names and shapes as tts_load_classifier reads them"""
    if "enc.init.weight" not in sd or sd["enc.init.weight"].ndim != 3:
        raise SystemExit("convert_classifier: no enc.init.weight (not an AudioMiniEncoderWithClassifierHead?)")
    b0, depth, blocks, i = sd["enc.init.weight"].shape[0], 0, 0, 0
    while True:
        if "enc.res.%d.op.weight" % i in sd:
            depth += 1
        elif "enc.res.%d.in_layers.2.weight" % i in sd:
            blocks += 1
        else:
            break
        i += 1
    if depth < 1 or blocks < 1 or blocks % depth or "enc.final.2.weight" not in sd:
        raise SystemExit("convert_classifier: %d ResBlocks and %d Downsamples under enc.res, enc.final.2.weight %s" % (blocks, depth, "enc.final.2.weight" in sd))
    attn = 0
    while "enc.attn.%d.norm.weight" % attn in sd:
        attn += 1
    return dict(b0=b0, depth=depth, K=sd["enc.res.0.in_layers.2.weight"].shape[-1], E=sd["enc.final.2.weight"].shape[0], rb=blocks // depth, attn=attn)


def convert_classifier(sd, path, downsample_factor=4, heads=4):
    """ggml-classifier-model.bin for tts_load_classifier: upstream tortoise-tts' classifier.pth (AudioMiniEncoderWithClassifierHead: enc.init, enc.res.*,
    enc.final.*, enc.attn.*, head), tensors under their state-dict names with the prefix `classifier.`. What the shapes cannot give, the downsample factor and
    the number of attention heads, is written into the 2-element tensor `classifier.config` (upstream: 4 and 4). The zero_module convolutions (out_layers.3,
    proj_out) are written as the checkpoint holds them. A missing, unknown or mis-shaped tensor is an error: the names and shapes are restated from memory
    (--list-expected classifier), so a real checkpoint that differs must be seen, not mis-read."""
    sd = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    arch = classifier_arch(sd)
    if arch["E"] % heads or arch["E"] // heads not in (64, 128):
        raise SystemExit("convert_classifier: %d channels in %d heads: the head dimension must be 64 or 128" % (arch["E"], heads))
    exp = classifier_tensor_shapes(F=downsample_factor, H=heads, config=False, **arch)
    for k in sorted(sd):
        if "classifier." + k not in exp:
            raise SystemExit("convert_classifier: unexpected tensor '%s'" % k)
    w = GgmlWriter(path)
    for name, shape in exp.items():
        k = name[len("classifier."):]
        if k not in sd:
            raise SystemExit("convert_classifier: tensor '%s' is missing" % k)
        if tuple(sd[k].shape) != tuple(shape):
            raise SystemExit("convert_classifier: tensor '%s' has shape %s, expected %s" % (k, list(sd[k].shape), list(shape)))
        w.add(name, sd[k])
    w.add("classifier.config", np.array([downsample_factor, heads], np.float32))
    w.close()
    return arch["b0"], arch["depth"], arch["E"], heads


def convert_random_voice(sd, path):
    """One side's file for tts_load_random_voice: rlg_auto.pth (1024 channels) or rlg_diffuser.pth (2048) of upstream tortoise-tts, the state dict of a
    RandomLatentConverter: layers.{0..L-1}.weight [D][D] and layers.{0..L-1}.bias [D], written under their own names and unchanged - weight * scale and
    bias * lr_mul are the loader's, one f32 multiply per element as torch performs it, so nothing is folded here. L and D are read from the state dict; a
    missing, unknown, non-square or mis-sized tensor is an error (the names are restated from memory: --list-expected random_voice). Returns (L, D)."""
    L = 0
    while "layers.%d.weight" % L in sd:
        L += 1
    if L < 2:
        raise SystemExit("convert_random_voice: %d layers.N.weight tensors (not a RandomLatentConverter state dict?)" % L)
    D = int(sd["layers.0.weight"].shape[0])
    exp = random_voice_tensor_shapes(D, L)
    for k in sorted(sd):
        if k not in exp:
            raise SystemExit("convert_random_voice: unexpected tensor '%s'" % k)
    w = GgmlWriter(path)
    for name, shape in exp.items():
        if name not in sd:
            raise SystemExit("convert_random_voice: tensor '%s' is missing" % name)
        if tuple(sd[name].shape) != tuple(shape):
            raise SystemExit("convert_random_voice: tensor '%s' has shape %s, expected %s" % (name, list(sd[name].shape), list(shape)))
        w.add(name, _np(sd[name]))
    w.close()
    return L, D


DVAE_DROPPED = ("decoder.", "codebook.cluster_size", "codebook.embed_avg", "codebook.initted", "codes", "total_codes", "loss_fn.")


def convert_dvae(sd, path, stride=2):
    """dvae.pth of upstream tortoise-tts (DiscreteVAE's state dict) -> the file tts_load_dvae reads: the encoder's convolutions and codebook.embed under
    `dvae.`, unchanged, plus dvae.config = (stride,) (no shape holds it; upstream: 2). Only get_codebook_indices is wanted, so the decoder, the EMA buffers
    (codebook.cluster_size, codebook.embed_avg, codebook.initted), the recorded codes and the loss are DROPPED; any other unknown tensor is an error, as is a
    missing or mis-sized one (the names are restated from memory: --list-expected dvae). Every size is read from the state dict. Returns
    (strided layers, ResBlocks, hidden channels, codebook dim, tokens)."""
    sd = {k: v for k, v in sd.items() if not k.startswith(DVAE_DROPPED)}
    L = 0
    while "encoder.%d.0.weight" % L in sd:
        L += 1
    nb = 0
    while "encoder.%d.net.0.weight" % (L + nb) in sd:
        nb += 1
    if L < 1 or "codebook.embed" not in sd or "encoder.%d.weight" % (L + nb) not in sd:
        raise SystemExit("convert_dvae: no encoder.N.0.weight, encoder.%d.weight or codebook.embed (not a DiscreteVAE state dict?)" % (L + nb))
    w0 = sd["encoder.0.0.weight"]
    dim, tokens = (int(v) for v in sd["codebook.embed"].shape)
    exp = dvae_tensor_shapes(channels=int(w0.shape[1]), hidden=int(w0.shape[0]), layers=L, blocks=nb, dim=dim, tokens=tokens, k=int(w0.shape[2]), stride=stride)
    for k in sorted(sd):
        if "dvae." + k not in exp:
            raise SystemExit("convert_dvae: unexpected tensor '%s'" % k)
    w = GgmlWriter(path)
    for name, shape in exp.items():
        if name == "dvae.config":
            w.add(name, np.array([stride], np.float32))
            continue
        k = name[len("dvae."):]
        if k not in sd:
            raise SystemExit("convert_dvae: tensor '%s' is missing" % k)
        if tuple(sd[k].shape) != tuple(shape):
            raise SystemExit("convert_dvae: tensor '%s' has shape %s, expected %s" % (k, list(sd[k].shape), list(shape)))
        w.add(name, _np(sd[k]))
    w.close()
    return L, nb, int(sd["encoder.%d.0.weight" % (L - 1)].shape[0]), dim, tokens


# ---- what each checkpoint is expected to hold (--list-expected) ---------------------------------------------------------------------
# name -> PyTorch shape as tortoise-tts stores it, for the upstream architecture (or the one given). Written from the loaders' contracts
# (main.cpp:682-792, 1244-1536, 1808-1923; csrc/extras.hip for the three containers the reference does not have), NOT from a checkpoint:
# the trained files are not obtainable offline, so the first person who has them gets a name / shape diff instead of a silent mismatch
# (check_against below; tests/test_convert_weights.py requires this list and the synthetic writers to agree).
def aligner_vocab_table(vocab, V):
    """(int32 [V] code points, blank id) from HF's vocab.json {token: id}: a single-character token gives its lower-case code point (the prompt is lowered
    before it is aligned), the word delimiter '|' is stored as a space (32), every other token - <pad>, <s>, </s>, <unk> - is -1; the CTC blank is <pad>."""
    if sorted(vocab.values()) != list(range(V)):
        raise SystemExit("convert_aligner: the vocabulary holds the ids %s, lm_head has %d rows" % (sorted(vocab.values())[:8] + ["..."], V))
    if "<pad>" not in vocab:
        raise SystemExit("convert_aligner: the vocabulary has no <pad> token (the CTC blank)")
    table = np.full(V, -1, np.int32)
    for tok, i in vocab.items():
        if tok == "|":
            table[i] = 32
        elif len(tok) == 1:
            table[i] = ord(tok.lower())
    return table, int(vocab["<pad>"])


def convert_aligner(sd, vocab, path, heads=16, strides=None):
    """ggml-aligner-model.bin for tts_load_aligner: HF's Wav2Vec2ForCTC state dict (stable-layer-norm configuration, e.g. wav2vec2-large-robust-ft-*) with
    `wav2vec2.` -> `aligner.` and `lm_head.` -> `aligner.lm_head.`. pos_conv_embed's weight-norm pair (weight_g / weight_v, or parametrizations.weight.original0 /
    original1) is folded into one weight, w = g v / |v| with the norm over output and input channels per tap (weight_norm dim = 2); masked_spec_embed is
    ignored. `aligner.config` = (heads, blank id, strides) and `aligner.vocab` are the converter's. Names and shapes are checked against
    aligner_tensor_shapes (--list-expected aligner)."""
    sd = {k: v for k, v in sd.items() if not k.endswith("masked_spec_embed")}
    pc = "wav2vec2.encoder.pos_conv_embed.conv."
    for g_name, v_name in ((pc + "weight_g", pc + "weight_v"), (pc + "parametrizations.weight.original0", pc + "parametrizations.weight.original1")):
        if g_name in sd and v_name in sd:
            g, v = sd.pop(g_name).double(), sd.pop(v_name).double()
            sd[pc + "weight"] = (v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())).float()
    t = {}
    for k, v in sd.items():
        if k.startswith("wav2vec2."):
            t["aligner." + k[len("wav2vec2."):]] = v
        elif k.startswith("lm_head."):
            t["aligner." + k] = v
        else:
            raise SystemExit("convert_aligner: unexpected tensor '%s'" % k)
    fe = "aligner.feature_extractor.conv_layers.%d."
    N = 0
    while fe % N + "conv.weight" in t:
        N += 1
    if N == 0 or "aligner.lm_head.weight" not in t or "aligner.feature_projection.projection.weight" not in t or "aligner.encoder.pos_conv_embed.conv.weight" not in t:
        raise SystemExit("convert_aligner: no feature_extractor.conv_layers / feature_projection / pos_conv_embed / lm_head (not a Wav2Vec2ForCTC state dict?)")
    if any(fe % i + "layer_norm.weight" not in t or fe % i + "conv.bias" not in t for i in range(N)):
        raise SystemExit("convert_aligner: a convolution layer without LayerNorm or bias: the group-norm (base-model) variant is not supported")
    depth = 0
    while "aligner.encoder.layers.%d.layer_norm.weight" % depth in t:
        depth += 1
    strides = tuple(strides) if strides else (5,) + (2,) * (N - 1)
    if len(strides) != N:
        raise SystemExit("convert_aligner: %d strides for %d convolution layers" % (len(strides), N))
    pw = t["aligner.encoder.pos_conv_embed.conv.weight"]
    D, V = int(pw.shape[0]), int(t["aligner.lm_head.weight"].shape[0])
    if D % heads or D // heads != 64:
        raise SystemExit("convert_aligner: %d channels in %d heads: the head dimension must be 64" % (D, heads))
    ffw = t.get("aligner.encoder.layers.0.feed_forward.intermediate_dense.weight")
    table, blank = aligner_vocab_table(vocab, V)
    arch = dict(N=N, C=int(t[fe % 0 + "conv.weight"].shape[0]), k=tuple(int(t[fe % i + "conv.weight"].shape[2]) for i in range(N)), s=strides, D=D,
                K=int(pw.shape[2]), G=D // int(pw.shape[1]), depth=depth, FF=int(ffw.shape[0]) if ffw is not None else 4 * D, V=V, H=heads, blank=blank)
    exp = aligner_tensor_shapes(config=False, **arch)
    del exp["aligner.vocab"]
    for k in t:
        if k not in exp:
            raise SystemExit("convert_aligner: unexpected tensor '%s'" % k[len("aligner."):])
    w = GgmlWriter(path)
    for name, shape in exp.items():
        if name not in t:
            raise SystemExit("convert_aligner: tensor '%s' is missing" % name[len("aligner."):])
        if tuple(t[name].shape) != tuple(shape):
            raise SystemExit("convert_aligner: tensor '%s' has shape %s, expected %s" % (name[len("aligner."):], list(t[name].shape), list(shape)))
        w.add(name, t[name].float().numpy())
    w.add("aligner.config", np.array([heads, blank] + list(strides), np.float32))
    w.add("aligner.vocab", table.astype(np.float32))
    w.close()
    return arch["N"], arch["C"], D, depth, V


def expected_tensors(kind, **arch):
    D = 1024
    out = {}

    def attn(p, d, rel=True, conv=True):
        out[p + ".norm.weight"] = (d,); out[p + ".norm.bias"] = (d,)
        out[p + ".qkv.weight"] = (3 * d, d, 1) if conv else (3 * d, d); out[p + ".qkv.bias"] = (3 * d,)
        out[p + ".proj_out.weight"] = (d, d, 1) if conv else (d, d); out[p + ".proj_out.bias"] = (d,)
        if rel:
            out[p + ".relative_pos_embeddings.relative_attention_bias.weight"] = (32, 16)

    def res(p):
        out[p + ".in_layers.0.weight"] = (D,); out[p + ".in_layers.0.bias"] = (D,)
        out[p + ".in_layers.2.weight"] = (D, D, 1); out[p + ".in_layers.2.bias"] = (D,)
        out[p + ".emb_layers.1.weight"] = (2 * D, D); out[p + ".emb_layers.1.bias"] = (2 * D,)
        out[p + ".out_layers.0.weight"] = (D,); out[p + ".out_layers.0.bias"] = (D,)
        out[p + ".out_layers.3.weight"] = (D, D, 3); out[p + ".out_layers.3.bias"] = (D,)

    if kind == "ar":  # autoregressive.pth, inference names (the training-time names gpt.h.N / gpt.ln_f / final_norm / mel_head are mapped onto them)
        out.update({"text_embedding.weight": (256, D), "text_pos_embedding.emb.weight": (404, D), "mel_embedding.weight": (8194, D),
                    "mel_pos_embedding.emb.weight": (608, D)})
        for i in range(arch.get("layers", 30)):
            p = "inference_model.transformer.h.%d." % i
            out.update({p + "ln_1.weight": (D,), p + "ln_1.bias": (D,), p + "attn.c_attn.weight": (D, 3 * D), p + "attn.c_attn.bias": (3 * D,),
                        p + "attn.c_proj.weight": (D, D), p + "attn.c_proj.bias": (D,), p + "ln_2.weight": (D,), p + "ln_2.bias": (D,),
                        p + "mlp.c_fc.weight": (D, 4 * D), p + "mlp.c_fc.bias": (4 * D,), p + "mlp.c_proj.weight": (4 * D, D), p + "mlp.c_proj.bias": (D,)})
        out.update({"inference_model.transformer.ln_f.weight": (D,), "inference_model.transformer.ln_f.bias": (D,), "inference_model.lm_head.0.weight": (D,),
                    "inference_model.lm_head.0.bias": (D,), "inference_model.lm_head.1.weight": (8194, D), "inference_model.lm_head.1.bias": (8194,)})
    elif kind == "diffusion":  # diffusion_decoder.pth (+ the voice's latent from --diffusion-conditioning-latent)
        out["latent_conditioner.0.weight"] = (D, D, 3); out["latent_conditioner.0.bias"] = (D,)
        for i in range(1, 1 + arch.get("lc", 4)):
            attn("latent_conditioner.%d" % i, D)
        out.update({"code_norm.weight": (D,), "code_norm.bias": (D,), "time_embed.0.weight": (D, D), "time_embed.0.bias": (D,),
                    "time_embed.2.weight": (D, D), "time_embed.2.bias": (D,)})
        for i in range(arch.get("integ", 3)):
            res("conditioning_timestep_integrator.%d.resblk" % i); attn("conditioning_timestep_integrator.%d.attn" % i, D)
        out.update({"inp_block.weight": (D, 100, 3), "inp_block.bias": (D,), "integrating_conv.weight": (D, 2 * D, 1), "integrating_conv.bias": (D,)})
        n_main, n_tail = arch.get("main", 10), arch.get("tail", 3)
        for i in range(n_main):
            res("layers.%d.resblk" % i); attn("layers.%d.attn" % i, D)
        for i in range(n_main, n_main + n_tail):
            res("layers.%d" % i)
        out.update({"out.0.weight": (D,), "out.0.bias": (D,), "out.2.weight": (200, D, 3), "out.2.bias": (200,), "unconditioned_embedding": (1, D, 1)})
    elif kind == "vocoder":  # vocoder.pth ['model_g'], weight_norm pairs fused: shapes of the fused `weight`
        out["conv_pre.weight"] = (32, 64, 7); out["conv_pre.bias"] = (32,)
        for i, stride in enumerate((8, 8, 4)):
            p, kp = "res_stack.%d." % i, "res_stack.%d.kernel_predictor." % i
            out[kp + "input_conv.0.weight"] = (64, 100, 5); out[kp + "input_conv.0.bias"] = (64,)
            for c in range(3):
                for j in (1, 3):
                    out[kp + "residual_convs.%d.%d.weight" % (c, j)] = (64, 64, 3); out[kp + "residual_convs.%d.%d.bias" % (c, j)] = (64,)
            out[kp + "kernel_conv.weight"] = (24576, 64, 3); out[kp + "kernel_conv.bias"] = (24576,)
            out[kp + "bias_conv.weight"] = (256, 64, 3); out[kp + "bias_conv.bias"] = (256,)
            out[p + "convt_pre.1.weight"] = (32, 32, 2 * stride); out[p + "convt_pre.1.bias"] = (32,)
            for c in range(4):
                out[p + "conv_blocks.%d.1.weight" % c] = (32, 32, 3); out[p + "conv_blocks.%d.1.bias" % c] = (32,)
        out["conv_post.1.weight"] = (1, 32, 7); out["conv_post.1.bias"] = (1,)
    elif kind == "clvp":  # clvp2.pth (use_xformers=True)
        dim, heads, ffm = arch.get("dim", 768), arch.get("heads", 12), arch.get("ff_mult", 2)
        inner, ff = heads * 64, dim * ffm
        out.update({"text_emb.weight": (256, dim), "speech_emb.weight": (8192, dim), "to_text_latent.weight": (dim, dim), "to_speech_latent.weight": (dim, dim),
                    "temperature": ()})
        for enc in ("text_transformer", "speech_transformer"):
            for i in range(arch.get("depth", 20)):
                a, f = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i), "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i + 1)
                out[a + "0.g"] = (dim,)
                for nm in ("to_q", "to_k", "to_v"):
                    out[a + "1.%s.weight" % nm] = (inner, dim)
                out[a + "1.to_out.weight"] = (dim, inner); out[a + "1.to_out.bias"] = (dim,)
                out[f + "0.g"] = (dim,)
                out[f + "1.net.0.proj.weight"] = (2 * ff, dim); out[f + "1.net.0.proj.bias"] = (2 * ff,)
                out[f + "1.net.3.weight"] = (dim, ff); out[f + "1.net.3.bias"] = (dim,)
            out[enc + ".transformer.norm.weight"] = (dim,); out[enc + ".transformer.norm.bias"] = (dim,)
    elif kind == "cvvp":  # cvvp.pth (names and shapes restated from memory: csrc/cvvp.hip), in write_cvvp's order
        dim = arch.get("dim", 512)
        ff, half = dim * arch.get("ff_mult", 1), dim // 2
        out.update({"temperature": (), "cond_emb.0.weight": (half, 80, 5), "cond_emb.0.bias": (half,), "cond_emb.1.weight": (dim, half, 3), "cond_emb.1.bias": (dim,),
                    "speech_emb.emb.weight": (8192, dim), "to_conditioning_latent.weight": (dim, dim), "to_speech_latent.weight": (dim, dim)})
        for enc in ("conditioning_transformer", "speech_transformer"):
            for i in range(arch.get("depth", 8)):
                a, f = "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i), "%s.transformer.attn_layers.layers.%d." % (enc, 2 * i + 1)
                out[a + "0.g"] = (dim,)
                for nm in ("to_q", "to_k", "to_v"):
                    out[a + "1.%s.weight" % nm] = (dim, dim)
                out[a + "1.to_out.weight"] = (dim, dim); out[a + "1.to_out.bias"] = (dim,)
                out[f + "0.g"] = (dim,)
                out[f + "1.net.0.proj.weight"] = (2 * ff, dim); out[f + "1.net.0.proj.bias"] = (2 * ff,)
                out[f + "1.net.3.weight"] = (dim, ff); out[f + "1.net.3.bias"] = (dim,)
            out[enc + ".transformer.norm.weight"] = (dim,); out[enc + ".transformer.norm.bias"] = (dim,)
            out[enc + ".pre_combiner.0.weight"] = (dim, dim, 1); out[enc + ".pre_combiner.0.bias"] = (dim,)
            attn(enc + ".pre_combiner.1", dim, rel=False)
            out[enc + ".pre_combiner.2.weight"] = (dim, dim, 1); out[enc + ".pre_combiner.2.bias"] = (dim,)
    elif kind == "conditioning-encoder":  # autoregressive.pth: conditioning_encoder.*
        out["conditioning_encoder.init.weight"] = (D, 80, 1); out["conditioning_encoder.init.bias"] = (D,)
        for i in range(arch.get("blocks", 6)):
            attn("conditioning_encoder.attn.%d" % i, D, rel=False)
    elif kind == "diffusion-conditioning-encoder":  # diffusion_decoder.pth: contextual_embedder.*
        out["contextual_embedder.0.weight"] = (1024, 100, 3); out["contextual_embedder.0.bias"] = (1024,)
        out["contextual_embedder.1.weight"] = (2048, 1024, 3); out["contextual_embedder.1.bias"] = (2048,)
        for i in range(arch.get("blocks", 5)):
            attn("contextual_embedder.%d" % (2 + i), 2048)
    elif kind == "bigvgan":  # the generator's state dict after weight-norm folding, without the *.filter buffers; default: the base model
        out.update({k[len("bigvgan."):]: v for k, v in bigvgan_tensor_shapes(arch.get("c0", 512), arch.get("rates", (8, 8, 2, 2))).items()})
    elif kind == "classifier":  # classifier.pth: AudioMiniEncoderWithClassifierHead's state dict (classifier.config is the converter's, not the checkpoint's)
        out.update({k[len("classifier."):]: v for k, v in classifier_tensor_shapes(config=False, **arch).items()})
    elif kind == "aligner":  # Wav2Vec2ForCTC after the weight-norm fold (aligner.config and aligner.vocab are the converter's, not the checkpoint's)
        out.update({k[len("aligner."):]: v for k, v in aligner_tensor_shapes(config=False, **arch).items() if k != "aligner.vocab"})
    elif kind == "random_voice":  # rlg_auto.pth (dim 1024, the default) / rlg_diffuser.pth (dim 2048): a RandomLatentConverter's state dict
        out.update(random_voice_tensor_shapes(arch.get("dim", 1024), arch.get("layers", 6)))
    elif kind == "dvae":  # dvae.pth: DiscreteVAE's encoder and codebook.embed (the decoder and the EMA buffers are dropped; dvae.config is the converter's)
        out.update({k[len("dvae."):]: v for k, v in dvae_tensor_shapes(config=False, **arch).items()})
    else:
        raise ValueError(kind)
    return out


EXPECTED_KINDS = ("ar", "diffusion", "vocoder", "clvp", "conditioning-encoder", "diffusion-conditioning-encoder", "cvvp", "bigvgan", "classifier", "aligner", "random_voice", "dvae")


def container_shape(kind, name, shape):
    """shape of the tensor as the CONTAINER holds it (the reference's loaders: k = 1 convolutions of the diffusion model squeezed to 2-D, conv_post
    [1, 32, 7] -> [32, 7], unconditioned_embedding flattened, a 0-dim temperature as [1]); everything else as in the checkpoint"""
    if kind == "diffusion" and SQUEEZE_K1.search(name) and len(shape) == 3:
        return shape[:2]
    if kind == "diffusion" and name == "unconditioned_embedding":
        return (int(np.prod(shape)),)
    if kind == "vocoder" and name == "conv_post.1.weight":
        return shape[-2:]
    if kind in ("clvp", "cvvp") and name == "temperature":
        return (1,)
    return tuple(shape)


def check_against(kind, sd, prefix=""):
    """name / shape diff of a state dict against expected_tensors(kind) (architecture counts taken from the state dict where they are discoverable);
    returns a list of human-readable lines, empty when everything expected is there with the expected shape"""
    have = {k: tuple(getattr(v, "shape", ())) for k, v in sd.items() if k.startswith(prefix)}

    def count(fmt, start=0):
        n = start
        while fmt % n in have:
            n += 1
        return n - start
    arch = {}
    if kind == "ar":
        arch["layers"] = count("inference_model.transformer.h.%d.ln_1.weight") or count("gpt.h.%d.ln_1.weight") or 30
    elif kind == "diffusion":
        arch = {"lc": count("latent_conditioner.%d.norm.weight", 1) or 4, "integ": count("conditioning_timestep_integrator.%d.resblk.in_layers.0.weight") or 3,
                "main": count("layers.%d.resblk.in_layers.0.weight") or 10}
        arch["tail"] = (count("layers.%d.in_layers.0.weight", arch["main"])) or 3
    elif kind == "clvp":
        n = 0
        while "text_transformer.transformer.attn_layers.layers.%d.0.g" % (2 * n) in have:
            n += 1
        arch["depth"] = n or 20
    elif kind == "conditioning-encoder":
        arch["blocks"] = count("conditioning_encoder.attn.%d.norm.weight") or 6
    elif kind == "diffusion-conditioning-encoder":
        arch["blocks"] = count("contextual_embedder.%d.norm.weight", 2) or 5
    lines = []
    for name, shape in expected_tensors(kind, **arch).items():
        if name not in have:
            lines.append("missing  %-80s expected %s" % (name, list(shape)))
        elif have[name] != tuple(shape) and int(np.prod(have[name] or (1,))) != int(np.prod(shape or (1,))):
            lines.append("shape    %-80s expected %s, checkpoint has %s" % (name, list(shape), list(have[name])))
    return lines


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ar")
    ap.add_argument("--diffusion")
    ap.add_argument("--diffusion-conditioning-latent", help=".pth / .npy / raw f32 file holding the voice's [1, 2048] diffusion conditioning latent")
    ap.add_argument("--vocoder")
    ap.add_argument("--conditioning-encoder", action="store_true", help="with --ar: also write ggml-conditioning-model.bin (the checkpoint's "
                                                                         "conditioning_encoder.* tensors: mel -> voice latent, tts_load_voice_encoder; not in the reference)")
    ap.add_argument("--diffusion-conditioning-encoder", help="diffusion_decoder.pth -> ggml-diffusion-conditioning-model.bin (its contextual_embedder.* tensors: "
                                                              "100-band mel -> the diffusion conditioning latent, tts_load_diffusion_conditioning_encoder; not in the reference)")
    ap.add_argument("--clvp", help="clvp2.pth of upstream tortoise-tts -> ggml-clvp-model.bin (candidate re-ranking, tts_load_clvp; not in the reference)")
    ap.add_argument("--cvvp", help="cvvp.pth of upstream tortoise-tts -> ggml-cvvp-model.bin (candidate re-ranking against the voice clips, tts_load_cvvp; not in the reference)")
    ap.add_argument("--bigvgan", help="NVIDIA BigVGAN v1 generator (bigvgan_base_24khz_100band or bigvgan_24khz_100band: g_*.zip / .pt) -> ggml-bigvgan-model.bin "
                                      "(the second vocoder, tts_load_bigvgan; not in the reference)")
    ap.add_argument("--classifier", help="classifier.pth of upstream tortoise-tts (tortoise-detect: AudioMiniEncoderWithClassifierHead) -> ggml-classifier-model.bin "
                                         "(tts_load_classifier; not in the reference)")
    ap.add_argument("--classifier-downsample-factor", type=int, default=4, help="with --classifier: the encoder's downsample factor (no shape holds it; upstream: 4)")
    ap.add_argument("--classifier-heads", type=int, default=4, help="with --classifier: the attention blocks' heads (no shape holds it; upstream: 4)")
    ap.add_argument("--aligner", help="pytorch_model.bin of a Wav2Vec2ForCTC checkpoint in the stable-layer-norm configuration (upstream tortoise-tts loads "
                                      "jbetker/wav2vec2-large-robust-ft-libritts-voxpopuli) -> ggml-aligner-model.bin (tts_load_aligner; not in the reference)")
    ap.add_argument("--aligner-vocab", help="with --aligner: the tokenizer's vocab.json {token: id}")
    ap.add_argument("--aligner-heads", type=int, default=16, help="with --aligner: attention heads (no shape holds it; upstream: 16)")
    ap.add_argument("--aligner-strides", help="with --aligner: the convolution strides, comma-separated (no shape holds them; upstream: 5,2,2,2,2,2,2)")
    ap.add_argument("--random-voice", help="rlg_auto.pth of upstream tortoise-tts (RandomLatentConverter, 1024 channels) -> ggml-random-voice-model.bin "
                                           "(the AR side of tts_load_random_voice; not in the reference)")
    ap.add_argument("--random-diffusion-voice", help="rlg_diffuser.pth of upstream tortoise-tts (RandomLatentConverter, 2048 channels) -> "
                                                     "ggml-random-diffusion-voice-model.bin (the diffusion side of tts_load_random_voice; not in the reference)")
    ap.add_argument("--dvae", help="dvae.pth of upstream tortoise-tts (DiscreteVAE) -> ggml-dvae-model.bin (speech codes from audio, tts_load_dvae: the encoder and "
                                   "the codebook; the decoder and the EMA buffers are dropped; not in the reference)")
    ap.add_argument("--dvae-stride", type=int, default=2, help="with --dvae: the strided layers' stride (no shape holds it; upstream: 2)")
    ap.add_argument("--out")
    ap.add_argument("--list-expected", nargs="*", metavar="KIND", help="print every tensor name / shape the converter looks for per checkpoint kind (%s; "
                                                                        "default: all, upstream architecture) and exit" % ", ".join(EXPECTED_KINDS))
    a = ap.parse_args()
    if a.list_expected is not None:
        for kind in (a.list_expected or EXPECTED_KINDS):
            for label, arch in ((("random_voice (rlg_auto)", dict(dim=1024)), ("random_voice (rlg_diffuser)", dict(dim=2048))) if kind == "random_voice" else ((kind, {}),)):
                exp = expected_tensors(kind, **arch)
                print("# %s: %d tensors" % (label, len(exp)))
                for name, shape in exp.items():
                    print("%-28s %-88s %s" % (label, name, "x".join(map(str, shape)) or "scalar"))
        return
    if not a.out:
        ap.error("--out is required")
    os.makedirs(a.out, exist_ok=True)
    load = lambda p: torch.load(p, map_location="cpu", weights_only=True)

    def checked(kind, sd, what):  # a name / shape diff before the conversion touches anything: no silent mismatch, no bare KeyError
        if kind == "ar" and not any(k.startswith("inference_model.") for k in sd):
            sd = dict(sd)
            for k in list(sd):
                for pat, rep in AR_TRAIN_TO_INFER:
                    if re.match(pat, k):
                        sd[re.sub(pat, rep, k)] = sd[k]
        if kind == "vocoder":
            sd = fuse_weight_norm(sd["model_g"] if "model_g" in sd else sd)
        diff = check_against(kind, sd)
        if diff:
            sys.exit("%s does not look like the expected %s checkpoint (python tools/convert_weights.py --list-expected %s prints the full list):\n  "
                     % (what, kind, kind) + "\n  ".join(diff[:40]) + ("\n  ... %d more" % (len(diff) - 40) if len(diff) > 40 else ""))

    if a.ar:
        checked("ar", load(a.ar), a.ar)
        print("ggml-model.bin: %d transformer layers" % convert_ar(load(a.ar), os.path.join(a.out, "ggml-model.bin")))
    if a.conditioning_encoder:
        if not a.ar:
            sys.exit("--conditioning-encoder needs --ar (the encoder's tensors live in autoregressive.pth)")
        checked("conditioning-encoder", load(a.ar), a.ar)
        print("ggml-conditioning-model.bin: %d attention blocks" % convert_conditioning_encoder(load(a.ar), os.path.join(a.out, "ggml-conditioning-model.bin")))
    if a.diffusion:
        if not a.diffusion_conditioning_latent:
            sys.exit("--diffusion needs --diffusion-conditioning-latent (the reference bakes the voice's diffusion latent into the weight file)")
        checked("diffusion", load(a.diffusion), a.diffusion)
        p = a.diffusion_conditioning_latent
        lat = np.load(p) if p.endswith(".npy") else load(p) if p.endswith((".pth", ".pt")) else np.fromfile(p, np.float32)
        print("ggml-diffusion-model.bin: blocks (latent conditioner, integrator, main, tail) = %s"
              % (convert_diffusion(load(a.diffusion), lat, os.path.join(a.out, "ggml-diffusion-model.bin")),))
    if a.diffusion_conditioning_encoder:
        checked("diffusion-conditioning-encoder", load(a.diffusion_conditioning_encoder), a.diffusion_conditioning_encoder)
        print("ggml-diffusion-conditioning-model.bin: %d attention blocks"
              % convert_diffusion_conditioning_encoder(load(a.diffusion_conditioning_encoder), os.path.join(a.out, "ggml-diffusion-conditioning-model.bin")))
    if a.clvp:
        checked("clvp", load(a.clvp), a.clvp)
        print("ggml-clvp-model.bin: %d encoder layers" % convert_clvp(load(a.clvp), os.path.join(a.out, "ggml-clvp-model.bin")))
    if a.cvvp:
        print("ggml-cvvp-model.bin: %d encoder layers per side" % convert_cvvp(load(a.cvvp), os.path.join(a.out, "ggml-cvvp-model.bin")))
    if a.bigvgan:
        print("ggml-bigvgan-model.bin: %d channels, strides %s" % convert_bigvgan(load(a.bigvgan), os.path.join(a.out, "ggml-bigvgan-model.bin")))
    if a.classifier:
        print("ggml-classifier-model.bin: base %d channels, depth %d, embedding %d, %d heads"
              % convert_classifier(load(a.classifier), os.path.join(a.out, "ggml-classifier-model.bin"), a.classifier_downsample_factor, a.classifier_heads))
    if a.aligner:
        if not a.aligner_vocab:
            sys.exit("--aligner needs --aligner-vocab (the tokenizer's vocab.json)")
        import json
        print("ggml-aligner-model.bin: %d convolution layers of %d channels, dimension %d, %d encoder layers, %d tokens"
              % convert_aligner(load(a.aligner), json.load(open(a.aligner_vocab)), os.path.join(a.out, "ggml-aligner-model.bin"), a.aligner_heads,
                                [int(v) for v in a.aligner_strides.split(",")] if a.aligner_strides else None))
    if a.random_voice:
        print("ggml-random-voice-model.bin: %d layers of %d channels" % convert_random_voice(load(a.random_voice), os.path.join(a.out, "ggml-random-voice-model.bin")))
    if a.random_diffusion_voice:
        print("ggml-random-diffusion-voice-model.bin: %d layers of %d channels"
              % convert_random_voice(load(a.random_diffusion_voice), os.path.join(a.out, "ggml-random-diffusion-voice-model.bin")))
    if a.dvae:
        print("ggml-dvae-model.bin: %d strided layers, %d ResBlocks of %d channels, codebook %d x %d tokens"
              % convert_dvae(load(a.dvae), os.path.join(a.out, "ggml-dvae-model.bin"), a.dvae_stride))
    if a.vocoder:
        checked("vocoder", load(a.vocoder), a.vocoder)
        print("ggml-vocoder-model.bin: %d res stacks" % convert_vocoder(load(a.vocoder), os.path.join(a.out, "ggml-vocoder-model.bin")))


if __name__ == "__main__":
    main()
