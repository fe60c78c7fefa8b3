/*
 * xgate_pos.h -- C ABI of the POS sequence generator in libxgate_hip.so (gfx950): the second model of the
 * reference pipeline (reference pos_src/SAModel.py), whose greedy rollout states become the captioner's
 * `pos_feats` (pos_src/eval_utils.py:36-75, caption_src/data_io.py:215-217).
 *
 * Inference only, eval mode, fp32 products.  The conventions are those of xgate.h:
 *   - extern "C", plain pointers and sizes; all tensor pointers are DEVICE pointers, fp32 unless noted,
 *     row-major and contiguous in the documented shape; token tensors are int64.
 *   - The caller owns all memory: scratch lives in one caller-provided workspace sized by
 *     xgp_workspace_bytes(), zero-filled once after allocation.
 *   - Every entry point only ENQUEUES work on `stream` (a hipStream_t passed as void*) and returns; there is
 *     no host synchronisation inside the library.  Results that decide a length (T', n) are written to device
 *     memory; the caller reads them when it needs them.
 *   - Return value: XG_OK or a negative XG_E* code (xgate.h; xg_strerror()).  Arguments are checked before
 *     anything is enqueued, so a bad call returns its error code without touching the device.
 *
 * Dimension names: B batch, K frames, R rnn_size, A att_size, E input_encoding_size, C categories,
 * F1 / F2 rgb / opfl feature sizes, T decoder steps of the call (cap_classes.size(1) for the teacher-forced
 * forward, seq_length + 1 for the greedy rollout).
 */
#ifndef XGATE_POS_H
#define XGATE_POS_H

#include <stddef.h>
#include <stdint.h>

#include "xgate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XGP_VERSION 1

typedef struct XgpDims {
    int32_t B, K, R, A, E, C, F1, F2, T;
} XgpDims;

/*
 * One device pointer per parameter of the reference model, in state_dict order (pos_src/SAModel.py:27-35,
 * pos_src/sub_modules.py:162-197,679-700,857-869).  The BatchNorm running statistics travel in XgBnState.
 * xgp_param_name(i) returns the state_dict key of field i.
 */
typedef struct XgpParams {
    float *emb_rgb_w, *emb_rgb_b, *bn_rgb_g, *bn_rgb_b;       /* two_fc_encoder.visual_emb_rgb.{0,1} */
    float *emb_opfl_w, *emb_opfl_b, *bn_opfl_g, *bn_opfl_b;   /* two_fc_encoder.visual_emb_opfl.{0,1} */
    float *lstm_rgb_wih, *lstm_rgb_whh, *lstm_rgb_bih, *lstm_rgb_bhh;     /* lstmcell_rgb  (gate order i,f,g,o) */
    float *lstm_opfl_wih, *lstm_opfl_whh, *lstm_opfl_bih, *lstm_opfl_bhh; /* lstmcell_opfl */
    float *fusion_w, *fusion_b;                                           /* fusion.late_fusion.0 */
    float *ih1_w, *ih1_b, *ic1_w, *ic1_b;                                 /* img_embed_{h_1,c_1} */
    float *i2h_w, *i2h_b, *a2h_w, *a2h_b, *h2h_w, *h2h_b;                 /* lstmcore.lstmcell (order i,f,o,g) */
    float *v2a_w, *v2a_b, *h2a_w, *h2a_b, *a2w_w, *a2w_b;                 /* lstmcore.{v2a,h2a,a2w} */
    float *embed_w;                                                       /* embed.weight (C,E) */
    float *logit_w, *logit_b;                                             /* logit (C,R) */
} XgpParams;

int xgp_version(void);
int xgp_param_count(void);
const char *xgp_param_name(int i);                        /* NULL when out of range */
int xgp_param_numel(const XgpDims *d, int i, int64_t *numel);
/* bytes of the workspace of every entry point below at dims d (0 for invalid dims) */
size_t xgp_workspace_bytes(const XgpDims *d);

/* Encoder (pos_src/sub_modules.py:199-239, eval mode): V (B,K,R) = relu(W [h_rgb ; h_opfl] + b) over the two
 * masked LSTMCell encoders of the BatchNorm'd embeddings.  d->T is not read. */
int xgp_encoder_fwd(void *stream, const XgpDims *d, const XgpParams *p, const XgBnState *bn,
                    const float *feats_rgb, const float *feats_opfl, const float *feat_mask,
                    float *V, void *ws, size_t ws_bytes);

/* Teacher-forced forward (pos_src/SAModel.py:62-90): cap_classes (B,T) int64 and new_mask (B,T) are the
 * already rolled inputs.  logp (B,T,C) receives the log-probabilities of all T steps; t_out (device int32[1])
 * receives T' = the first i >= 1 whose cap_classes column is all zero (T if none): the reference stops there,
 * so only logp[:, :T'] is its output. */
int xgp_forward_tf(void *stream, const XgpDims *d, const XgpParams *p, const XgBnState *bn,
                   const float *feats_rgb, const float *feats_opfl, const float *feat_mask,
                   const int64_t *cap_classes, const float *new_mask,
                   float *logp, int32_t *t_out, void *ws, size_t ws_bytes);

/* Greedy rollout collecting states (pos_src/SAModel.py:136-184), T = seq_length + 1 steps, all run on the
 * device: seq (B,T-1) int64, seq_logp (B,T-1), states (B,T,R) = the hidden state after each step, masks (B,T)
 * = the xt_mask of each step, n_out (device int32[1]) = the reference's sequence length n (it stops once every
 * row has finished).  The reference's outputs are seq[:, :n], seq_logp[:, :n], states[:, :n+1], masks[:, :n+1]. */
int xgp_sample_greedy(void *stream, const XgpDims *d, const XgpParams *p, const XgBnState *bn,
                      const float *feats_rgb, const float *feats_opfl, const float *feat_mask,
                      int64_t *seq, float *seq_logp, float *states, float *masks, int32_t *n_out,
                      void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif

#endif /* XGATE_POS_H */
