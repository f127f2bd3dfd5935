// What extras.hip (CLVP, the two conditioning encoders) shares with cvvp.hip: the x-transformers encoder layers CLVP and CVVP have in common and the
// AttentionBlock of the voice encoder, as host functions around extras.hip's kernels. One definition of each; both files launch through these.
#pragma once
#include "common.h"
#include <hip/hip_fp16.h>

namespace tts {

// One (attention, GEGLU feed-forward) pair: RMSNorm gains, biases (f32) and the fp16 GEMM weights; w_qkv = to_q | to_k | to_v rows, one projection launch
struct EncLayer {
  float *g_attn = nullptr, *g_ff = nullptr, *b_out = nullptr, *b_ff1 = nullptr, *b_ff2 = nullptr;
  __half *w_qkv = nullptr, *w_out = nullptr, *w_ff1 = nullptr, *w_ff2 = nullptr;
};
// AttentionBlock (GroupNorm32, k = 1 qkv, QKVAttentionLegacy, proj_out, residual); w_qkv / b_qkv rows already in q | k | v order, head h at columns h * 64
struct AttnBlockW {
  float *g = nullptr, *b = nullptr, *b_qkv = nullptr, *b_proj = nullptr;
  __half *w_qkv = nullptr, *w_proj = nullptr;
};
// The packed sequences a launch works on: sequence s = rows [d_start[s], + d_len[s]) of x[M][dim] (f32 residual stream, M = rows padded to 128); the fp16 / f32
// scratch operands (y: M x max(dim, ff), qkv: M x 3 inner, att: M x inner, u: M x 2 ff) are the caller's, zeroed past the last row
struct EncWork {
  const int *d_start = nullptr, *d_len = nullptr;
  int nseq = 0, rows = 0, maxlen = 0, M = 0;
  float *x = nullptr, *u = nullptr;
  __half *y = nullptr, *qkv = nullptr, *att = nullptr;
};

// f32 / fp16 uploads that `owned` frees
int enc_up(tts_ctx *ctx, std::vector<void *> &owned, const std::vector<float> &src, float **dst);
int enc_up16(tts_ctx *ctx, std::vector<void *> &owned, const std::vector<const std::vector<float> *> &parts, __half **dst);
// `depth` layers "<enc>.transformer.attn_layers.layers.N." of a CLVP / CVVP file (`model`: the name in the messages); TTS_ERR_FORMAT for a missing or mis-shaped tensor
int enc_load_layers(tts_ctx *ctx, const WeightFile &wf, const std::string &enc, const char *model, int depth, int d, int in, int ff, std::vector<void *> &owned,
                    std::vector<EncLayer> &out);
// x[r] = emb[tok[r]]
void enc_embed(tts_ctx *ctx, const float *emb, const int *d_tok, int dim, int rows, float *x);
// the layers on w.x, in place: rotary attention (first 32 of 64 head dims of q, k and v) and GEGLU feed-forward with RMSNorm pre-norm and f32 residuals
int enc_run_layers(tts_ctx *ctx, const std::vector<EncLayer> &layers, int d, int in, int ff, const EncWork &w);
// one AttentionBlock of D = 512 or 1024 channels (heads of 64) on w.x, in place
int attn_block_run(tts_ctx *ctx, int D, const AttnBlockW &b, const EncWork &w);
// im2col of a k = 3 / stride 2 / padding 1 convolution over f32 rows [row][cin] (dcond_im2col_kernel<false>): fp16 rows of kpad >= 3 cin
void im2col3_rows(tts_ctx *ctx, const float *x, const int *in_start, const int *in_len, const int *out_start, const int *out_len, int max_out, int nseq, int cin,
                  int kpad, __half *a16);

} // namespace tts
