/*
 * vtc_hip.h -- C ABI of libvtc_hip.so: the MI355X (gfx950) implementation of the VTC
 * retrieval forward/eval hot path.
 *
 * The reference (unitaryai/VTC) is pure Python: its native boundary for this path is
 * torch / openai-CLIP / faiss internals, it has no FFI of its own.  These entry points are
 * therefore what a binding for this path would call; each one names the reference
 * interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - `stream` is a hipStream_t passed as void* (so this header needs no HIP headers);
 *   - functions only enqueue work on `stream`; they never allocate, free or synchronise;
 *   - scratch memory is caller-provided: ask vtc_*_workspace_bytes(), pass `ws`/`ws_bytes`;
 *   - return 0 on success, non-zero on error (see vtc_last_error); nothing throws;
 *   - `dtype` selects the arithmetic of the GEMM/attention operands: VTC_F32 (exact fp32
 *     MFMA) or VTC_BF16 (bf16 operands, fp32 accumulate).  LayerNorm, softmax, residual
 *     stream, biases and all outputs are fp32 in both modes;
 *   - weight matrices are row-major [out_features, in_features] (PyTorch Linear layout) in
 *     the compute dtype; biases and LayerNorm parameters are fp32.
 *
 * Process-wide state: the product library reads no environment variable (only the test build, libvtc_hip_testhooks.so, reads
 * VTC_CAM_TEST_GAVE_UP); the Python host layer's switches travel to it as per-call arguments / per-model flags.
 */
#ifndef VTC_HIP_H
#define VTC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { VTC_F32 = 0, VTC_BF16 = 1, VTC_U8 = 2 /* pixel_dtype only: raw 0..255 pixels */,
       VTC_F16 = 3 /* IEEE half operands, fp32 accumulate: vtc_gemm / vtc_layernorm / vtc_attention and the text tower */ };

/* residual activations of the CAM, model/model.py:65-77 (stateless ones) */
enum { VTC_ACT_NONE = 0, VTC_ACT_NORMALIZE = 1, VTC_ACT_SQUASH = 2, VTC_ACT_TANH = 3,
       VTC_ACT_SUB_MEAN = 4, VTC_ACT_BN = 5 };   /* eval-mode BatchNorm1d statistics, model/model.py:42-61 */

/* sweep precision: how q.g is formed from fp32 embeddings */
enum { VTC_SWEEP_F32 = 0,      /* fp32 MFMA, bitwise a k-ordered fmaf chain            */
       VTC_SWEEP_BF16X3 = 1,   /* hi/lo bf16 split, 3 products: |err| ~ 5e-7           */
       VTC_SWEEP_BF16 = 2,     /* plain bf16 operands: |err| ~ 1e-3, ranks may differ  */
       VTC_SWEEP_EXACT = 3 };  /* BF16X3 candidate lists (depth + 21, at least 32) re-ranked with
                                  fp64 distances sum_k (q_k - g_k)^2; a row whose candidate list is
                                  not provably a superset of its true top-`depth` is recomputed by
                                  fp64 brute force: ranks are those of exact fp64 arithmetic        */

/* One residual attention block.
 * upstream clip/model.py ResidualAttentionBlock; TimeSformer extras
 * model/timesformer_clip_alt.py:112-129 (NULL for ViT / text / CAM blocks). */
typedef struct {
  const float *ln1_g, *ln1_b;
  const void  *qkv_w;  const float *qkv_b;   /* attn.in_proj_{weight,bias}   [3W,W],[3W] */
  const void  *out_w;  const float *out_b;   /* attn.out_proj                [W,W],[W]   */
  const float *ln2_g, *ln2_b;
  const void  *fc_w;   const float *fc_b;    /* mlp.c_fc                     [4W,W],[4W] */
  const void  *proj_w; const float *proj_b;  /* mlp.c_proj                   [W,4W],[W]  */
  const float *lnt_g, *lnt_b;                /* ln_time                                  */
  const void  *tqkv_w; const float *tqkv_b;  /* timeattn.in_proj                         */
  const void  *tout_w; const float *tout_b;  /* timeattn.out_proj; NULL => tfc_* holds the
                                                pre-multiplied map temporal_fc o out_proj */
  const void  *tfc_w;  const float *tfc_b;   /* temporal_fc                  [W,W],[W]   */
  /* Folded LayerNorm (optional; all NULL => the LayerNorm kernels run).  16-bit modes only: the LayerNorm in front of a
   * projection is applied by that projection's epilogue,  LN(x) W^T + b = rstd_m (x W'^T - mean_m s_n) + c_n,  with
   * W' = (gamma . W) in the block's operand format, s[n] = sum_k W'[n][k] (of the rounded W'), c[n] = b[n] + sum_k beta[k] W[n][k].
   * Contract of the residual stream while the fold is on: between layer 0's cast and the final LayerNorm the stream is NOT the
   * fp32 `x` of the workspace (stale there) but a row-centred 16-bit pair (hi, lo) in the block's operand format, x - mean(x) ~=
   * hi + lo, which the residual GEMMs read and write (with per-row (mean, rstd)) and whose `hi` is the projections' A operand;
   * every buffer's rows are padded to a multiple of 256 and the pad rows hold garbage that only GEMM tiles touch. */
  const void  *qkv_wf;  const float *qkv_s,  *qkv_c;    /* ln_1    -> attn.in_proj     */
  const void  *fc_wf;   const float *fc_s,   *fc_c;     /* ln_2    -> mlp.c_fc         */
  const void  *tqkv_wf; const float *tqkv_s, *tqkv_c;   /* ln_time -> timeattn.in_proj */
} vtc_block_w;

/* Per-model path switches (vtc_vision_w.flags / vtc_text_w.flags).  They live in the weight struct -- two models in one
 * process may choose differently, nothing is process-wide -- and never change results beyond the stated tolerance
 * (FULL_LAST_LAYER: see below). */
enum { VTC_TOWER_NO_LN_FOLD = 1,       /* run the LayerNorm kernels even when the blocks carry folded weights (*_wf)              */
       /* 2, 4: retired in ABI 6 (the fused QKV + attention kernel of rounds 1-4 left the product: tools/probes/qkv_attn.hip) */
       VTC_TOWER_FULL_LAST_LAYER = 8,  /* By default the LAST block's queries, out_proj and MLP run only on the rows that reach the
                                          output (x[:, 0] behind ln_post, model/timesformer_clip_alt.py:281; the EOT row behind
                                          ln_final): on every other row of that block they are dead -- nothing reads them (its keys
                                          and values are computed for every row).  This flag computes them anyway (same embeddings
                                          within rounding; for measurements against the unpruned path)                          */
       VTC_TOWER_NO_SPLITK = 16        /* (ABI 7) At batch 1 - 2 (<= 1024 padded rows) the MLP's c_proj runs split over K: slices
                                          of K on 4x the workgroups, then one row pass that sums them, applies the residual update
                                          and writes the LayerNorm statistics.  This flag keeps the one-pass GEMM (same embeddings
                                          up to the summation order over K)                                                      */ };

/* Vision tower: upstream VisionTransformer (nframes == 0) or
 * model/timesformer_clip_alt.py:203-286 VisualTransformer (nframes > 0). */
typedef struct {
  int width, heads, layers, patch, grid, embed_dim, nframes;
  int variant;                    /* 0: timesformer_clip_alt.py (used by model.py); 1: timesformer_clip.py */
  int flags;                      /* VTC_TOWER_* (below): per-model choices of the kernel path, same results            */
  float pix_mean[3], pix_std[3];  /* pixel_dtype VTC_U8: x = (u8/255 - mean[c]) / std[c], i.e. ToTensor + Normalize of
                                     CLIP_TRANSFORM (dataset_loaders/dataset_loaders.py:40-49) fused into the patch gather */
  const void  *conv_w;            /* conv1.weight flattened [W, Kp], Kp = 3*patch*patch rounded up to a multiple of 64 (zero-padded
                                     columns: patch 14 -> 588 -> 640; patch 16 / 32 unchanged)   */
  const float *class_embedding;   /* [W]                                                  */
  const float *pos;               /* positional_embedding [1+grid*grid, W]                */
  const float *temporal;          /* temporal_embed [nframes, W] or NULL                  */
  const float *ln_pre_g, *ln_pre_b, *ln_post_g, *ln_post_b;
  const float *proj_t;            /* proj^T [embed_dim, W], fp32 in both modes            */
  const vtc_block_w *blocks;      /* HOST array of `layers` entries                       */
} vtc_vision_w;

/* Text tower: upstream CLIP.encode_text. */
typedef struct {
  int width, heads, layers, ctx, vocab, embed_dim;
  int half_layers;                /* dtype VTC_BF16 only: blocks [0, half_layers) hold IEEE-half (VTC_F16) weight matrices and
                                     run with half operands, the others bf16 (the bf16 rounding floor of
                                     this tower is above the 1e-3 budget; half has 3 more significant bits at the same rate) */
  int flags;                      /* VTC_TOWER_*                                          */
  const float *tok_emb;           /* token_embedding.weight [vocab, W] fp32               */
  const float *pos;               /* positional_embedding [ctx, W]                        */
  const float *ln_final_g, *ln_final_b;
  const float *proj_t;            /* text_projection^T [embed_dim, W], fp32 in both modes */
  const vtc_block_w *blocks;      /* HOST array                                           */
} vtc_text_w;

/* Context Adapter Module: model/model.py:141-205 + :396-400. */
typedef struct {
  int width, heads, layers;
  int init_from_avg;              /* model/model.py:156-161                               */
  int residual_activation;        /* VTC_ACT_*                                            */
  float squash_scale;             /* 1, 10, 1.2, 1.5, 1.8 for the squash* family          */
  const void  *final_linear;      /* [D,D] compute dtype (used when !init_from_avg)       */
  const float *mask_embedding;    /* [D]                                                  */
  const vtc_block_w *blocks;      /* HOST array                                           */
  const float *bn_mean, *bn_var;  /* mean_center_bn.running_mean / running_var [D]; SUB_MEAN, BN only (else NULL) */
  int flags;                      /* VTC_CAM_*                                            */
} vtc_cam_w;
/* vtc_cam_w.flags.  By default small batches (B (1 + nc) <= 512 tokens, fp32, init_from_avg) run the whole CAM -- token build,
 * both layers, finalisation -- as ONE cooperative launch (cam.hip) instead of ~30 generic ones; same arithmetic, fp32. */
enum { VTC_CAM_NO_FUSED = 1 };   /* always the multi-launch path */

const char *vtc_last_error(void);          /* thread-local message of the last failure   */
int vtc_abi_version(void);

/* ---- towers ------------------------------------------------------------------------ */

/* Replaces clip_model.encode_image (model/model.py:332,464) when w->nframes == 0 and
 * VisualTransformer.forward (model/timesformer_clip_alt.py:252-286, called at
 * model/model.py:497,613) when w->nframes > 0.
 * pixels: [n_items, F, 3, H, W] (F = 1 for images), fp32 (pixel_dtype VTC_F32), bf16, or raw uint8 (VTC_U8).
 * out:    [n_items, embed_dim] fp32 (not normalised). */
size_t vtc_vision_workspace_bytes(const vtc_vision_w *w, int n_items, int frames, int dtype);
int vtc_vision_forward(const vtc_vision_w *w, const void *pixels, int pixel_dtype, int n_items, int frames,
                       float *out, void *ws, size_t ws_bytes, int dtype, void *stream);

/* Replaces clip_model.encode_text (model/model.py:210,340,351,472,499,615).
 * ids: [n_seq, ctx] int64.  out: [n_seq, embed_dim] fp32. */
size_t vtc_text_workspace_bytes(const vtc_text_w *w, int n_seq, int dtype);
int vtc_text_forward(const vtc_text_w *w, const int64_t *ids, int n_seq, float *out, void *ws, size_t ws_bytes,
                     int dtype, void *stream);

/* The same tower over TWO id arrays -- sequences [0, n_a) from ids_a (titles), [n_a, n_a + n_b) from ids_b (comments; may be
 * NULL with n_b = 0) -- so that the wrappers need no concatenated copy (model/model.py:472 + :210 as one call), and, with
 * ragged != 0, on the ragged batch WITHOUT any host knowledge of the lengths: EOT positions, the prefix sums and the row count
 * are computed on the device and every kernel of the tower reads the row count from device memory (no host sync).
 * Workspace: vtc_text_workspace_bytes(w, n_a + n_b, dtype) (the dense upper bound).  Same outputs as vtc_text_forward. */
int vtc_text_forward2(const vtc_text_w *w, const int64_t *ids_a, int n_a, const int64_t *ids_b, int n_b, int ragged, float *out,
                      void *ws, size_t ws_bytes, int dtype, void *stream);

/* Same tower on a RAGGED batch: only tokens 0..EOT of each sequence are computed.  seq_offsets: int32
 * [n_seq+1] exclusive prefix sums of (argmax(ids[s]) + 1); total_rows = seq_offsets[n_seq] (host value).
 * Outputs are identical to vtc_text_forward: under the causal mask nothing after EOT reaches the EOT row. */
size_t vtc_text_ragged_workspace_bytes(const vtc_text_w *w, int n_seq, int total_rows, int dtype);
int vtc_text_forward_ragged(const vtc_text_w *w, const int64_t *ids, int n_seq, const int *seq_offsets, int total_rows,
                            float *out, void *ws, size_t ws_bytes, int dtype, void *stream);

/* Replaces PretrainedCLIPBase._load_comment_features' masking + _adapt_feature
 * (model/model.py:207-214, 141-205), eval semantics.
 * main: [B,D] fp32; comm_feats: [B*nc, D] fp32 = encode_text(comments.reshape(B*nc, ctx));
 * comments: [B,nc,ctx] int64 (only token 1 is read: the empty-string test :208).
 * adapted: [B,D] fp32 = normalize(normalize(main) + r). */
size_t vtc_cam_workspace_bytes(const vtc_cam_w *w, int B, int nc, int dtype);
int vtc_cam_forward(const vtc_cam_w *w, const float *main_feats, const float *comm_feats, const int64_t *comments,
                    int ctx, int B, int nc, float *adapted, void *ws, size_t ws_bytes, int dtype, void *stream);
/* Small batches run the whole module as ONE launch with software grid barriers (cam.hip).  A barrier that cannot complete --
 * a kernel this process cannot see holds CUs: another process on the card, a collective -- gives up after ~0.4 s: THAT call's
 * `adapted` rows are NaN, and every later call on the device takes the multi-launch path (same results; one line on stderr).
 * vtc_cam_fused_gave_up(device) = 1 once that has happened in this process (a host read of a pinned word, no synchronisation;
 * it speaks for a given forward once the forward's stream has been synchronised). */
int vtc_cam_fused_gave_up(int device);

/* The CAM with na extra tokens per item after the comments (the audio branch, model/model.py:220-230): item b's sequence is
 * [main[b], comment tokens as in vtc_cam_forward, aux[b*na + 0 .. b*na + na - 1]]; aux rows are normalised like the others and never
 * replaced by mask_embedding.  aux: [B*na, D] fp32 (NULL when na = 0).  1 + nc + na <= 80; the one-launch path takes
 * 1 + nc + na <= 15.  With na = 0 the result is bit-identical to vtc_cam_forward.  Workspace: vtc_cam_aux_workspace_bytes. */
size_t vtc_cam_aux_workspace_bytes(const vtc_cam_w *w, int B, int nc, int na, int dtype);
int vtc_cam_forward_aux(const vtc_cam_w *w, const float *main_feats, const float *comm_feats, const int64_t *comments,
                        const float *aux, int ctx, int B, int nc, int na, float *adapted, void *ws, size_t ws_bytes, int dtype,
                        void *stream);

/* The audio branch's feature MLP (model/model.py:80-94, eval mode), fp32, one launch (audio.hip):
 *   y = w2 relu(w1 x + b1) + b2,  x, y: [n, d] fp32, d = 512; w1, w2: [d, d] row-major ([out, in], as nn.Linear.weight), b1, b2: [d].
 * w1 / b1 carry the BatchNorm1d running statistics folded in by the caller.  ws: vtc_feature_mlp_workspace_bytes(n, d) bytes
 * (may be 0, then ws may be NULL). */
size_t vtc_feature_mlp_workspace_bytes(int n, int d);
int vtc_feature_mlp(const float *x, int n, int d, const float *w1, const float *b1, const float *w2, const float *b2, float *y,
                    void *ws, size_t ws_bytes, void *stream);

/* ---- frame preprocessing: the Resize(size, BICUBIC) + CenterCrop(size) half of CLIP_TRANSFORM
 * (dataset_loaders/dataset_loaders.py:40-49, video_retrieval_videodatasets.py:21-29); ToTensor + Normalize are the VTC_U8
 * pixel path of vtc_vision_forward ------------------------------------------------------------------------------------- */

/* Decoded RGB uint8 frames of in_h x in_w -> [n, 3, size, size] uint8, BIT FOR BIT what torchvision's Resize(size) +
 * CenterCrop(size) give on a PIL image (Pillow's 8-bit resampler, integer arithmetic):
 *   1. resize target: the shorter edge becomes `size`, the longer trunc((size * long) / short) (the double quotient of the exact
 *      product); in_w <= in_h: the width is the shorter edge;
 *   2. two separable passes, horizontal first, the intermediate image rounded to uint8.  Per output index xx of an axis of n_in
 *      input and n_out output samples: scale = n_in / n_out, fs = max(scale, 1), support = 2 fs, center = (xx + 0.5) scale,
 *      xmin = max(trunc(center - support + 0.5), 0), count = min(trunc(center + support + 0.5), n_in) - xmin, weights
 *      bicubic((x + xmin - center + 0.5) * (1 / fs)) with a = -0.5 in double, divided by their sum, each then
 *      trunc(w 2^22 +- 0.5) (the sign of w); pixel = clamp((2^21 + sum p_x k_x) >> 22, 0, 255), arithmetic shift.  A pass with
 *      n_in == n_out is the identity;
 *   3. crop: top = round((out_h - size) / 2), left likewise, ties to even (Python's round);
 *   only output pixels inside the crop are computed and only the source rows and columns in their support are read.
 * LIMITS (refused with a status + vtc_last_error, nothing is launched): size a positive multiple of 16 (a plane stays a multiple of
 * 16 pixels for the VTC_U8 path), at most 1024; 1 <= in_h, in_w <= 8192 (2160 x 3840 and 4320 x 7680 are inside).
 *
 * vtc_resize_plan (pure HOST code; plan_host is the one HOST pointer of this group) fills a relocatable table of int32 words:
 *   [0..15]  header: magic "VRP1", in_h, in_w, size, out_w, out_h, left, top, column taps kx, row taps ky, 0 ...
 *   then per cropped output COLUMN (size records of 2 + kx words): first source column, count, coefficients[kx] (zero padded),
 *   then per cropped output ROW    (size records of 2 + ky words): first source row,    count, coefficients[ky].
 * An identity pass has one tap of 2^22.  vtc_resize_plan_bytes = its size (0 for arguments the plan call refuses).  The caller
 * uploads the plan once per distinct (in_h, in_w, size).
 *
 * vtc_resize_crop_u8: layout 0 = frames [n, in_h, in_w, 3] (what decoders deliver), 1 = [n, 3, in_h, in_w]; frames need no
 * alignment (rows of in_w * 3 bytes, odd widths included); out [n, 3, size, size] must be 16-byte aligned (rows are written with
 * 16-byte stores).  One launch: a workgroup takes one frame and a band of 16 (8, 4, 2, 1 when the vertical support is long) output
 * rows, resamples the source rows in the band's support along x into LDS, then along y out of it; the intermediate image never
 * reaches memory.  The plan lives in device memory and the call only enqueues, so it cannot read it: the KERNEL compares the plan's
 * header with the header these arguments imply and, when they disagree, reads no frame and writes nothing (`out` keeps its bytes);
 * every index taken from the table is clamped, so a damaged plan cannot address outside `frames`, `out` or the LDS. */
size_t vtc_resize_plan_bytes(int in_h, int in_w, int size);
int vtc_resize_plan(int in_h, int in_w, int size, void *plan_host, size_t bytes);
int vtc_resize_crop_u8(const unsigned char *frames, int n, int in_h, int in_w, int layout, const void *plan_dev, int size,
                       unsigned char *out, void *stream);

/* ---- small fp32 ops of the wrappers (model/model.py:26-27, 338, 357-362, 369) -------- */
int vtc_normalize_rows(const float *x, float *out, int n, int d, void *stream);
/* Both embedding sets of a forward in one launch: outx = rows of x [nx, d] / their norms, outy likewise for y [ny, d] (the two
 * `normalize` calls that end every PretrainedCLIP*.forward, model/model.py:263-264, 366-367), and the non-finite watchdog with it:
 * flag[0] (int32, device; NULL: none) |= 1 when a row of x holds a NaN / inf OR has a squared norm of zero -- an all-zero row, or
 * one whose squares all underflow: its output row is 0/0 = NaN (x/0 = inf), as in the reference -- |= 2 for y: the word is raised
 * whenever vtc_nonfinite_flag2 would raise it on the two OUTPUTS (ABI 7). */
int vtc_normalize_rows2(const float *x, float *outx, int nx, const float *y, float *outy, int ny, int d, int *flag, void *stream);
/* out[g] = mean over `group` consecutive rows (frames -> video, title+comments -> text) */
int vtc_mean_groups(const float *x, float *out, int n_groups, int group, int d, void *stream);
/* Token packing: the array-building half of `_tokenise` (dataset_loaders/dataset_loaders.py:224-248; the BPE encoder and the RAKE
 * summariser in front of it stay host text processing).  tokens: the batch's BPE ids back to back (int32, device), offsets [n_seq + 1]
 * their prefix sums (device).  ids [n_seq, ctx] int64 = [sot] + tokens of the sequence + [eot], zero padded; a sequence that reaches
 * ctx keeps its first ctx - 1 ids and ends in eot (:240-243).  The output is what vtc_text_forward* take. */
int vtc_pack_tokens(const int *tokens, const int *offsets, int n_seq, int ctx, int sot, int eot, int64_t *ids, void *stream);

/* out[g] = (a[g] + sum_k b[g * group + k]) / (1 + group): the "averaging" comment fusion, mean of a title embedding and its
 * comments' (model/model.py:357-362), without stacking them first */
int vtc_mean_head_groups(const float *a, const float *b, float *out, int n_groups, int group, int d, void *stream);
/* out[g] = mean of rows [offsets[g], offsets[g+1]): per-video mean over a ragged number of 8-frame
 * chunks, NOT re-normalised (evaluation/retrieval_evaluation.py:254-259).  offsets: int32 [n_groups+1] */
int vtc_segment_mean(const float *x, const int *offsets, float *out, int n_groups, int d, void *stream);
/* flag[0] |= 1 when x[0..n) holds a non-finite value.  Range guard of the text tower's IEEE-half blocks (vtc_text_w.half_layers):
 * an overflow of the half format (|v| > 65504) shows as inf / NaN in the tower's output.  `flag` is int32 in device memory or in
 * pinned (device-visible) host memory, which the host can then poll without synchronising. */
int vtc_nonfinite_flag(const float *x, size_t n, int *flag, void *stream);
/* flag[0] |= 1 when x[0..n) holds a non-finite value, |= 2 when y[0..m) does -- one launch over the two embedding sets a wrapper's
 * forward returns (ABI 7).  Every `PretrainedCLIP*.forward` ends with it (vtc_amd/host/model.py: the flag travels to pinned host
 * memory by an asynchronous copy and is read at the model's next forward / check_finite()); RecallAtK and the eval entry points
 * check their inputs with it and raise: a NaN embedding (an IEEE-half overflow in the text blocks, a one-launch CAM whose grid
 * barrier gave up, non-finite weights or pixels) never reaches a recall figure silently. */
int vtc_nonfinite_flag2(const float *x, size_t n, const float *y, size_t m, int *flag, void *stream);
/* sim[nv,nt] = exp(*logit_scale) * v @ t^T, fp32 exact */
int vtc_similarity(const float *v, const float *t, int nv, int nt, int d, const float *logit_scale, float *sim,
                   void *stream);

/* Replaces model/loss.py:18-22 clip_loss.  sim: [n,n] fp32; loss: 1 float (device). */
size_t vtc_clip_loss_workspace_bytes(int n);
int vtc_clip_loss(const float *sim, int n, float *loss, void *ws, size_t ws_bytes, void *stream);

/* ---- N x N sweep: replaces faiss.GpuIndexFlatL2.add/search in RecallAtK.compute
 * (model/metric.py:137-146) and the hit counting (:148-160) --------------------------- */

/* ids[nq,depth] (int64) / dists[nq,depth] (fp32, may be NULL) = the `depth` rows of `gallery`
 * nearest to each row of `queries` by squared L2 = |q|^2 + |g|^2 - 2 q.g (fp32), ascending,
 * ties by lowest gallery index.  The fp32 distance matrix is materialised in `ws` in
 * row blocks of `rows_per_block` queries (0 = as many as fit).
 * LIMITS (refused with a status + vtc_last_error, nothing is launched): d % 64 == 0 -- zero-pad the feature columns, squared L2
 * distances are unchanged (faiss.IndexFlatL2 takes any d; vtc_amd/host/metric.py pads for its callers) -- and
 * 1 <= depth <= min(64, n_gallery): one list entry per lane of a wavefront; the reference searches depth max(k)+1 = 11
 * (model/metric.py:145).  The same limits hold for vtc_l2_topk_bidir and the sharded entry points below. */
size_t vtc_l2_topk_workspace_bytes(int n_gallery, int n_queries, int d, int precision, int rows_per_block);
int vtc_l2_topk(const float *gallery, const float *queries, int n_gallery, int n_queries, int d, int depth,
                int precision, int rows_per_block, int64_t *ids, float *dists, void *ws, size_t ws_bytes,
                void *stream);

/* Both retrieval directions from ONE distance matrix D[i][j] = |b_i - a_j|^2 (the reference runs two searches,
 * evaluation/eval.py:117-127 -> model/metric.py:137-146): ids_b2a [n_b, depth] = vtc_l2_topk(gallery = a, queries = b),
 * ids_a2b [n_a, depth] = vtc_l2_topk(gallery = b, queries = a); the second direction is read off the columns of the
 * blocks the first direction's GEMM has written (no second GEMM).  dists_* may be NULL.  depth <= min(64, n_a, n_b). */
size_t vtc_l2_topk_bidir_workspace_bytes(int n_a, int n_b, int d, int precision, int rows_per_block);
int vtc_l2_topk_bidir(const float *a, const float *b, int n_a, int n_b, int d, int depth, int precision, int rows_per_block,
                      int64_t *ids_b2a, float *dists_b2a, int64_t *ids_a2b, float *dists_a2b, void *ws, size_t ws_bytes,
                      void *stream);
/* Sharded sweep (one process per GPU; the reference is single-GPU, evaluation/eval.py:117-127 -> model/metric.py:137-146):
 * rank r holds rows [lo_r, hi_r) of both embedding sets and the all-gathered sets, and runs ONE distance GEMM
 * D_r[i][j] = |b_(lo_r + i) - a_j|^2, i < n_local, j < n_total, for BOTH directions:
 *   vtc_l2_sweep_shard_rows   ids [n_local, depth] = vtc_l2_topk(gallery = a_all, queries = b_local) -- complete, the rank
 *                             holds whole rows -- and col_planes [4, nblk_pad, n_total] (uint32): per column j and per block of
 *                             vtc_l2_sweep_row_block() local rows, the three smallest distance keys and the fourth as a bound
 *                             (blocks past the rank's rows: +inf).  nblk_pad = ceil(largest shard / row block), equal on all ranks.
 *   (host) all-to-all: rank r sends col_planes[:, :, lo_s:hi_s] to rank s
 *   vtc_l2_sweep_shard_cols   planes [n_src, 4, nblk_pad, n_local] = what the n_src ranks sent for this rank's columns, in
 *                             rank order; src_base[n_src] (device int32) = lo_r of each source.  ids [n_local, depth] =
 *                             vtc_l2_topk(gallery = b_all, queries = a_local), bit-identical to the single-GPU search
 *                             (certified candidates re-ranked in fp64, uncertified columns settled in fp64 from their own planes).
 * VTC_SWEEP_EXACT only; d % 64 == 0; vtc_l2_sweep_shard_supported tells whether the shape is covered (else: two vtc_l2_topk). */
int vtc_l2_sweep_row_block(void);
int vtc_l2_sweep_shard_supported(int n_total, int n_local, int depth);
size_t vtc_l2_sweep_shard_workspace_bytes(int n_total, int n_local, int d);
int vtc_l2_sweep_shard_rows(const float *a_all, const float *b_local, int n_total, int n_local, int d, int depth, int64_t *ids,
                            float *dists, unsigned *col_planes, int nblk_pad, void *ws, size_t ws_bytes, void *stream);
int vtc_l2_sweep_shard_cols(const float *b_all, const float *a_local, int n_total, int n_local, int d, int depth,
                            const unsigned *planes, int n_src, int nblk_pad, const int *src_base, int64_t *ids, float *dists,
                            void *ws, size_t ws_bytes, void *stream);
/* Query-time search: the exact nearest rows of a stored gallery for a FEW queries (no reference counterpart: the reference only evaluates).
 * With D(q, j) the fp64 value sum_k (queries[q][k] - gallery[j][k])^2 of the fp32 inputs (the one device function of the sweeps, so a
 * distance has the bits every other entry point gives it and exact ties are bit-equal):
 *   ids[q, 0 .. depth)  (int64)  = id_base + j for the `depth` gallery rows with the smallest (D(q, j), j), compared lexicographically, ascending
 *   dists[q, p]  (fp32, may be NULL) = (float) D
 * A gallery row whose distance is not finite is never returned; when fewer than `depth` rows have a finite distance the tail of the row is
 * ids = -1, dists = +inf, and so is the whole row of a query with a NaN / inf coordinate.  nonfinite[0] (int32, device, may be NULL; the
 * word of the rank family, here ORed into: the caller zeroes it) |= 1 if the gallery holds a NaN / inf, |= 2 if the queries do.
 * The gallery is streamed and never rewritten: no operand planes, no distance matrix, no candidate lists -- one pass over the gallery per
 * TILE of queries (1 query: 1 pass; 2: 1; 3-4: 1; more: ceil(n_queries / 8) passes), every workgroup of the scan leaving one sorted list per
 * query in the workspace, and a second small launch merging them.  Two launches, no allocation, no host sync.
 * The fp64 distances of the result stay in the workspace: after the call its first n_queries * depth doubles are D of ids[q, p] (+inf where
 * ids is -1) -- what vtc_l2_search_merge takes, since the fp32 dists alone would break ties that the fp64 values decide.
 * LIMITS (refused with a status + vtc_last_error, nothing is launched): 1 <= n_queries <= 64 (more: vtc_l2_topk), 1 <= depth <=
 * min(64, n_gallery), d % 64 == 0 and 64 <= d <= 2048, n_gallery >= 1, id_base >= 0, non-null gallery / queries / ids, ws_bytes >=
 * vtc_l2_search_workspace_bytes(...), which is 0 for arguments the call refuses. */
size_t vtc_l2_search_workspace_bytes(int n_gallery, int n_queries, int d, int depth);
int vtc_l2_search(const float *gallery, const float *queries, int n_gallery, int n_queries, int d, int depth, int64_t id_base,
                  int64_t *ids, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* vtc_l2_search over the LIVE rows of the gallery only: a deleted row, or a query that searches a subset (one subreddit, one split).
 * live (uint32, device, ceil(n_gallery / 32) words; only read): row j takes part iff bit (j & 31) of live[j >> 5] is set; the bits at
 * and above n_gallery in the last word are ignored, whatever they hold.  live == NULL: every row takes part -- the call IS vtc_l2_search
 * (same launches, same bits).
 * The result is that of vtc_l2_search over the gallery COMPACTED to its live rows in order, every returned position mapped back to the
 * row's original index: ids = id_base + j of the live rows with the smallest (D(q, j), j); ties go to the lower original row (compaction
 * keeps order); a live row with a non-finite distance is never returned; fewer than `depth` live finite rows leave a tail of -1 / +inf
 * (the ordinary outcome of a small subset).  A dead row influences nothing -- not ids, not dists, not nonfinite (a NaN in a removed row
 * does not set bit 0) -- and its memory is not read: a step of the scan none of whose rows is live issues no gallery load, so a filter
 * costs about its live fraction of the scan.  The fp64 distances stay at the head of the workspace as above, so vtc_l2_search_merge takes
 * masked partial lists unchanged.  No compaction: rows keep their index.
 * LIMITS: those of vtc_l2_search, including depth <= n_gallery, which counts the PHYSICAL rows (the number of live ones is not known on
 * the host); the workspace is vtc_l2_search_workspace_bytes(...).  vtc_l2_topk has no mask. */
int vtc_l2_search_masked(const float *gallery, const float *queries, const uint32_t *live, int n_gallery, int n_queries, int d, int depth,
                         int64_t id_base, int64_t *ids, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* Packs row flags into the words vtc_l2_search_masked reads: words[w] (ceil(n_rows / 32) of them) bit b = (flags[32 w + b] != 0), ANDed
 * with and_mask[w] when and_mask is non-null (a subset intersected with the rows that are still live); the bits past n_rows are written
 * as 0.  flags: uint8 [n_rows], device.  One launch, no atomics.  n_rows >= 1; null flags / words are refused (status + vtc_last_error). */
int vtc_row_mask_pack(const uint8_t *flags, int n_rows, const uint32_t *and_mask, uint32_t *words, void *stream);
/* The lists of n_parts searches over DISJOINT gallery windows (each with its window's id_base) -> the list of the union: ids_parts
 * [n_parts, n_queries, depth] (int64) and dists_parts of the same shape (DOUBLE: the head of each search's workspace), entries with a
 * negative id ignored; ids / dists (fp32, may be NULL) [n_queries, depth] = the first `depth` of the union by (dist, id), padded with
 * -1 / +inf.  1 <= n_parts <= 64, 1 <= n_queries <= 64, 1 <= depth <= 64; one launch. */
int vtc_l2_search_merge(const int64_t *ids_parts, const double *dists_parts, int n_parts, int n_queries, int depth, int64_t *ids,
                        float *dists, void *stream);
/* The GROUPED search: several rows per video (a title and its comments, 20 - 40 captions, the 8-frame chunks of a long video), and the
 * `depth` nearest distinct VIDEOS come back, each by its nearest row.  It is the group minimum E(u, v) of the video-unit ranks
 * (vtc_l2_rank_grouped_vunit above) used at query time.
 * Inputs: gallery rows j in [0, n_gallery); a group id groups[j] per row (int32, device, only read) with ANY value -- negative, sparse
 * or unsorted are all legal, and the rows of one group need not be adjacent; an optional live mask as vtc_l2_search_masked takes it
 * (NULL: every row).  D(q, j) is the fp64 squared distance of the fp32 rows that every sweep uses.
 * Take the complete list of live rows with a finite D(q, j), sorted by (D(q, j), j).  DELETE EVERY ROW THAT IS NOT THE FIRST OF ITS
 * GROUP IN THAT ORDER.  The first `depth` entries of what remains are the result.  Per entry:
 *   ids[q, p]        (int64) = id_base + j, the row: the video's best-matching caption, comment or chunk
 *   out_groups[q, p] (int32) = groups[j]
 *   dists[q, p]      (fp32, may be NULL) = (float) D(q, j); the fp64 value in the first n_queries * depth doubles of the workspace
 * Consequences: ties between groups go to the lower row, ties inside a group go to the lower row.  A row with a non-finite distance
 * never represents its group (its next row does; a group of such rows only never appears) and sets bit 1 of nonfinite as above.  A dead
 * row is never read and influences nothing.  Fewer than `depth` distinct live groups with a finite distance give a list that ends in
 * ids = -1, out_groups = -1, dists = +inf -- ids alone says "empty", -1 is also a legal group id.  A non-finite query gets a row of -1
 * and bit 2.  With every row in a group of its own the result is vtc_l2_search_masked's, bit for bit.
 * The same two launches on the same grid as vtc_l2_search; the scan reads 4 more bytes per row.
 * LIMITS and refusals: those of vtc_l2_search_masked (depth <= n_gallery counts PHYSICAL rows), and groups / out_groups must be
 * non-null; the workspace is vtc_l2_search_grouped_workspace_bytes(...), 0 for a refused shape. */
size_t vtc_l2_search_grouped_workspace_bytes(int n_gallery, int n_queries, int d, int depth);
int vtc_l2_search_grouped(const float *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int n_gallery, int n_queries,
                          int d, int depth, int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                          size_t ws_bytes, void *stream);
/* vtc_l2_search_merge for grouped lists: groups_parts [n_parts, n_queries, depth] (int32) beside ids_parts / dists_parts.  The windows'
 * rows are disjoint, their groups need not be: of a group that several parts list, the entry first by (dist, id) stays.  Exact: a group
 * of the union's first `depth` has its overall nearest row in some part, where fewer than `depth` groups are nearer, so that part lists
 * it.  Limits of vtc_l2_search_merge; a null groups_parts / out_groups is refused. */
int vtc_l2_search_merge_grouped(const int64_t *ids_parts, const double *dists_parts, const int32_t *groups_parts, int n_parts, int n_queries,
                                int depth, int64_t *ids, int32_t *out_groups, float *dists, void *stream);
/* vtc_l2_search_masked / vtc_l2_search_grouped over a gallery STORED AS IEEE binary16 (uint16 bit patterns, [n_gallery, d], row stride d,
 * 8-byte aligned; only IEEE half, not bf16): half the bytes a one-query scan streams, half the memory an index holds.  The queries stay
 * fp32.  D(q, j) is the fp64 sum over k of ((double)queries[q][k] - (double)(float)gallery[j][k])^2, formed with the summation order of
 * vtc_l2_search -- binary16 -> fp32 is exact, subnormal halves included (they are not flushed) -- so ids, dists and the fp64 distances
 * at the head of the workspace are, BIT FOR BIT, those of the fp32 entry over the gallery widened to fp32: exact over the rows as
 * stored, ties to the lower row, the same bits whichever kernel forms the distance.  A half row with a +-inf or NaN has a non-finite
 * distance: it is never returned and sets bit 1 of nonfinite.  live may be NULL; a dead row is never read.
 * groups == NULL: the ungrouped search (out_groups is then ignored; workspace vtc_l2_search_workspace_bytes).  groups != NULL: the
 * grouped search, out_groups is required (workspace vtc_l2_search_grouped_workspace_bytes).  The partial lists in the workspace are fp64
 * distances and ids, so vtc_l2_search_merge / vtc_l2_search_merge_grouped take windows of half and of fp32 galleries alike.
 * LIMITS and refusals: those of the fp32 entries (n_queries in [1, 64], depth in [1, min(64, n_gallery)], d a multiple of 64 in
 * [64, 2048], id_base >= 0, null gallery / queries / ids / ws, a workspace that is too small), and groups given without out_groups.
 * There is no many-query route for a half gallery through vtc_l2_topk, which reads fp32 rows: the one for a half gallery is
 * vtc_l2_search_many_half below. */
int vtc_l2_search_half(const uint16_t *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int n_gallery,
                       int n_queries, int d, int depth, int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists,
                       int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* MANY queries over a half gallery.  DEFINITION: the result is that of vtc_l2_search_half with groups == NULL on the same arguments, BIT
 * FOR BIT -- ids, dists, the n_queries * depth doubles at the head of the workspace, the bits ORed into nonfinite, the -1 / +inf tails,
 * the whole -1 row of a non-finite query, a dead row influencing nothing (not even bit 1), live == NULL meaning every row, id_base --
 * so vtc_l2_search_merge takes its windows unchanged.  The entry has no specification of its own.
 * MECHANISM (search_many.hip): four launches whatever the data, no host synchronisation, no allocation, nothing read back.  A prologue
 * over the QUERIES splits them into fp16 hi + lo (scaled by a power of two); ONE pass streams the gallery through
 * v_mfma_f32_16x16x32_f16 -- the stored rows are the operand, |g|^2 is formed from the loaded tile -- for an approximate distance A with
 * |A - D| <= eps = kappa (|q|^2 + max|g|^2) + 1e-35, kappa = (6 d + 8) 2^-24 + 2^-20 (derived in search_many.hip), and keeps per query
 * the cdepth = min(64, n_gallery, max(32, depth + 21)) smallest; a finish forms the candidates' fp64 distances with the scan's own device
 * function, orders them by (D, row) and accepts the list where the bound proves that every row outside it lies STRICTLY behind the
 * depth-th found (or the list is every live finite row).  A query the bound cannot certify -- near-duplicates deeper than the list,
 * magnitudes beyond fp16 / fp32 range or too small for the split, an A that overflowed while D is finite -- is finished on the device
 * by an exact fp64 scan of the live rows (one workgroup per such query: slow, and normally there is none).  A tile of 16 rows none of
 * which is live issues no gallery load.
 * COST: one gallery pass per call for up to 64 queries (the scan: one per 8); measured in profiles/search_many.md.
 * THE COUNTER: behind the fp64 head -- at byte align256(n_queries * depth * 8) of the workspace -- one int32 holds the number of
 * queries of this call that the fallback finished (the workspace is carved in 256-byte steps).
 * LIMITS and refusals (a status, vtc_last_error, nothing launched): those of vtc_l2_search_half, and depth <= 32 (at least 21 spare
 * ranks in a lane-per-entry list); 1 <= n_queries <= 64 (more: slice them).  The workspace is vtc_l2_search_many_workspace_bytes(...),
 * 0 for a refused shape; it does not grow with n_queries x n_gallery (no distance matrix: at most 1024 lists of cdepth per query).
 * NOT PROVIDED: groups; cursor, exclude and sets; fp32 galleries, masked or not; more than 64 queries per pass; depth above 32. */
size_t vtc_l2_search_many_workspace_bytes(int n_gallery, int n_queries, int d, int depth);
int vtc_l2_search_many_half(const uint16_t *gallery, const float *queries, const uint32_t *live, int n_gallery, int n_queries, int d,
                            int depth, int64_t id_base, int64_t *ids, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* SEARCH AFTER A CURSOR: results beyond depth 64, one page at a time.  The search order of a query is the total order of its live rows
 * with a finite distance by the key (D(q, j), j) -- fp64 distance, then row.  For every query q the call returns the `depth` rows whose
 * key lies STRICTLY AFTER the cursor key (after_d[q], after_i[q]) (double [n_queries] and int64 [n_queries], device, only read):
 *   row j is admitted iff D(q, j) > after_d[q], or D(q, j) == after_d[q] and id_base + j > after_i[q], both compared exactly;
 * everything else -- ids, dists, the tail of -1 / +inf, nonfinite, the fp64 distances at the head of the workspace, `live` (NULL: every
 * row), id_base -- is vtc_l2_search_masked's (gallery_is_half == 0, fp32 rows) or vtc_l2_search_half's without groups (gallery_is_half
 * != 0, IEEE binary16 bit patterns).  The call keeps no state.  With (after_d, after_i) = the last fp64 distance and id of the previous
 * page, the pages concatenated ARE the ranking to any depth, bit for bit what one deeper search would return: the previous page holds
 * exactly the keys up to its last one, so the next starts at its successor.  That needs after_d[q] to have the bits the scan forms for
 * the cursor row: take it from the head of the previous call's workspace, or from vtc_l2_pair_dists64 -- not from the fp32 dists.
 * after_d[q] = -inf admits every row (the call is then the plain search); +inf or a NaN admits none: the row of that query is empty.
 * after_i[q] is any int64: a cursor row below id_base lies before every row of this window at an equal distance, one at or above
 * id_base + n_gallery after them, so the windows of one gallery take the SAME cursor and vtc_l2_search_merge merges their lists.  The
 * cursor row need not be live: a cursor survives the removal of its row.
 * Two launches on the grid of vtc_l2_search; one gallery pass per tile of queries, whatever the cursor.
 * LIMITS and refusals: those of vtc_l2_search_masked, and after_d / after_i must be non-null; the workspace is
 * vtc_l2_search_workspace_bytes(...).  The grouped search has no cursor (of this entry: pages of distinct videos are
 * vtc_l2_search_grouped_after below, which needs a pass of its own first). */
int vtc_l2_search_after(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const double *after_d,
                        const int64_t *after_i, int n_gallery, int n_queries, int d, int depth, int64_t id_base, int64_t *ids, float *dists,
                        int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* SEARCH EXCLUDING ONE ROW OR ONE GROUP PER QUERY: "more like this" (the nearest rows of a stored row, that row left out) and hard
 * negatives (the nearest videos of text q other than its own video), for a whole batch in one call.  exclude: int64 [n_queries], device,
 * only read.  DEFINITION: take the search order of query q -- its live rows with a finite distance by (D(q, j), j) -- or, with groups, the
 * grouped order of vtc_l2_search_grouped (that order with every row deleted that is not the first of its group); DELETE the excluded
 * rows; THEN cut to `depth` (after the cursor, where one is given):
 *   groups == NULL: query q never gets the one row with id_base + j == exclude[q];
 *   groups != NULL: query q never gets a row with (int64) groups[j] == exclude[q] -- the whole group is deleted BEFORE the groups are
 *                   de-duplicated, so the result is the grouped search of the gallery without that group's rows.
 * A value that no row / no group has excludes nothing: -1 or any id outside [id_base, id_base + n_gallery) for rows, any value outside
 * int32 for groups (every int32, -1 included, is a legal group, which is why the key is an int64).  The windows of one gallery take the
 * SAME exclude (global ids / groups) and vtc_l2_search_merge / vtc_l2_search_merge_grouped merge their lists unchanged.
 * after_d / after_i: NULL together (no cursor), or the cursor of vtc_l2_search_after, ungrouped only; the cursor may stand on the excluded
 * row itself (its key is a key like any other), the page then starts right after it.  gallery_is_half / live (NULL: every row) / ids /
 * dists / nonfinite / the fp64 distances at the head of the workspace: as vtc_l2_search_after, and out_groups as vtc_l2_search_grouped.
 * The excluded key is one more compare per query on a row that has already beaten the depth-th entry: the gallery is read once.
 * LIMITS and refusals: those of vtc_l2_search_after (groups == NULL; workspace vtc_l2_search_workspace_bytes) or vtc_l2_search_grouped
 * (workspace vtc_l2_search_grouped_workspace_bytes, out_groups required); exclude must be non-null; after_d without after_i or the
 * reverse, and a cursor together with groups, are refused (vtc_l2_search_grouped_after takes both, and an excluded group with them).
 * A refused call launches nothing. */
int vtc_l2_search_excluding(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                            const int64_t *exclude, const double *after_d, const int64_t *after_i, int n_gallery, int n_queries, int d,
                            int depth, int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                            size_t ws_bytes, void *stream);
/* out[q] (double [n_queries], device) = D(queries[q], gallery row rows[q] - id_base): the fp64 squared distance of ONE pair per query,
 * formed by the device function of every search -- the bits vtc_l2_search* leaves in its workspace for that pair, so a valid after_d.
 * rows: int64 [n_queries], device.  rows[q] == -1, or any id outside [id_base, id_base + n_gallery), gives out[q] = +inf and reads no
 * gallery memory: never a fault.  THE ROW IS READ WHETHER OR NOT IT IS LIVE -- there is no mask; a row removed from an index keeps its
 * memory.  A query that holds a NaN / inf gives a non-finite out[q].  Any n_queries >= 1; one launch, one wave per query.
 * Refused: null gallery / queries / rows / out, n_gallery < 1, n_queries < 1, d not a multiple of 64 in [64, 2048], id_base < 0. */
int vtc_l2_pair_dists64(const void *gallery, int gallery_is_half, const float *queries, const int64_t *rows, int n_gallery, int n_queries,
                        int d, int64_t id_base, double *out, void *stream);
/* PAGES OF DISTINCT VIDEOS: the grouped search after a cursor, to any depth.  For query q the ADMISSIBLE rows are the live rows (of
 * `live`; NULL: every row) with a finite D(q, j), minus the rows with (int64) groups[j] == exclude[q] where exclude is given.  K(q, g) is
 * the smallest key (D(q, j), id_base + j) over the admissible rows of group g; the grouped order of q is the groups with an admissible
 * row sorted by K.  vtc_l2_search_grouped_after returns the first `depth` groups of that order with K(q, g) STRICTLY AFTER the cursor
 * key (after_d[q], after_i[q]) -- K.d > after_d[q], or K.d == after_d[q] and K.row > after_i[q], compared exactly -- each with its
 * nearest row and that row's distance; ids / out_groups / dists / the tail of -1 / -1 / +inf / nonfinite / the fp64 distances at the
 * head of the workspace are vtc_l2_search_grouped's.  With the cursor = the last (fp64 distance, id) of the previous page -- the fp64
 * value from the workspace or from vtc_l2_pair_dists64, never the fp32 dists -- the pages concatenated ARE the grouped order, bit for
 * bit, without repeats or gaps.  after_d[q] = -inf admits everything (the call is then vtc_l2_search_grouped), +inf or a NaN nothing;
 * the cursor row need not be live, and an id that is no row of the gallery is a key like any other (vtc_l2_pair_dists64 gives it +inf:
 * an empty page).
 * WHY TWO CALLS.  "After row r" is a compare on a row's own key; "the video's nearest row lies after r" is not: a row after the cursor
 * belongs on the page only if NO admissible row of its group lies at or before the cursor, and such a row can be anywhere in the
 * gallery.  So vtc_l2_group_mark_before makes one pass and sets bit g of ban[q] for every group g with a live row of finite distance at
 * or before the cursor -- ban: uint32 [n_queries][ceil(n_groups / 32)] in device memory of the caller, vtc_l2_group_ban_words(...)
 * words, bit g & 31 of word g >> 5 -- and vtc_l2_search_grouped_after drops the rows of the groups whose bit is set.  The mark pass
 * ONLY ORs: the caller zeroes the buffer (or carries bits forward: every group already returned may be marked by hand).  exclude is not
 * looked at by the mark pass: an excluded group is dropped by the scan anyway.
 * GROUP IDS ARE DENSE HERE: groups[j] in [0, n_groups), because the bitmap is indexed by the group.  A row whose group lies outside
 * that range marks nothing and is never returned.  (vtc_l2_search_grouped and the other grouped entries take any int32 and stay as
 * they are.)
 * WINDOWS: the cursor and the ids are global as in vtc_l2_search_after, the windows of one gallery take the SAME cursor and mark into
 * the SAME ban buffer, and EVERY window must be marked before ANY window is scanned -- a group's row before the cursor may lie in
 * another window.  vtc_l2_search_merge_grouped then merges the windows' pages unchanged.
 * Cost: two gallery passes per tile of queries (the mark pass keeps no lists), the scan's two launches plus one.
 * LIMITS and refusals: those of vtc_l2_search_grouped and vtc_l2_search_after (the mark pass has no depth); n_groups in [1, 2^31);
 * ban, after_d, after_i and groups must be non-null, exclude may be NULL (no group); the workspace is
 * vtc_l2_search_grouped_workspace_bytes(...).  vtc_l2_group_ban_words is 0 for n_queries outside [1, 64] or n_groups < 1.  A refused
 * call launches nothing. */
size_t vtc_l2_group_ban_words(int n_queries, int n_groups);
int vtc_l2_group_mark_before(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                             int n_groups, const double *after_d, const int64_t *after_i, int n_gallery, int n_queries, int d,
                             int64_t id_base, uint32_t *ban, void *stream);
int vtc_l2_search_grouped_after(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                                int n_groups, const uint32_t *ban, const int64_t *exclude, const double *after_d, const int64_t *after_i,
                                int n_gallery, int n_queries, int d, int depth, int64_t id_base, int64_t *ids, int32_t *out_groups,
                                float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* SET QUERIES: several vectors as ONE query, the minimum over them -- the videos nearest to a video by any of its captions or chunks,
 * the videos that match a title or any of its comments, any of these paraphrases.
 * A set query S is m >= 1 vectors, its members.  Its distance to gallery row j is
 *     E(S, j) = min over the members v of S with only finite components of D(v, j)
 * D is the fp64 squared distance every search forms (wave_dist64_core: same statements, same bits).
 *   UNGROUPED ORDER.  The live rows with a finite E, sorted by (E(S, j), j).  The first `depth` are the result.
 *   GROUPED ORDER.  Take the ungrouped order and delete every row that is not the first of its group.  The first `depth` are the
 *   result.  This is vtc_l2_search_grouped's sentence with E in place of D.
 *   EXCLUDED KEY PER SET.  A row when ungrouped, a group when grouped.  It is deleted from the order before the cut, as
 *   vtc_l2_search_excluding does.  -1, or a key that is not there, excludes nothing.
 *   NON-FINITE MEMBERS.  A member with a NaN or inf takes no part and sets bit 2 of `nonfinite`.  A set with no finite member returns
 *   -1 / (-1) / +inf.  Bit 1 means what it means today.
 *   EQUIVALENCES.  A set of one member is the plain search.  Every output, the fp64 list in the workspace included, has the bits
 *   vtc_l2_search / _masked / _half / _grouped / _excluding give for that vector.  Repeating a member changes nothing.  That is how the
 *   host pads ragged sets.
 *   THERE IS NO CURSOR.  A set search has no `after` and no deep form.  A set larger than one tile of 8 members is scanned as several
 *   tiles.  A tile knows only its own members' min.  A row that an earlier page returned on tile 1's distance would pass a cursor test
 *   against tile 2's larger one and come back.  Paging set queries needs the cursor test on the set-wide E, which these entries do not
 *   have; a range search over sets does not exist either.
 * queries: float [n_sets * set_size][d], device, set s being the rows [s * set_size, (s + 1) * set_size); all sets of a call have the
 * same size (pad a smaller one by repeating a member).  live (NULL: every row), groups (NULL: ungrouped; then out_groups is not looked
 * at), exclude (NULL: none; int64 [n_sets], device, a global row id or a group as vtc_l2_search_excluding reads them), gallery_is_half,
 * id_base, nonfinite: as in vtc_l2_search_excluding.  ids / out_groups / dists: [n_sets][depth], device; the fp64 distances of the
 * result are the first region of the workspace, double [n_sets][depth], as in every search.
 * Cost: one gallery pass per started tile of 8 members per set (a set of 1, 2 or up to 4 members is one tile of that shape), one merge
 * per set over the lists of all its tiles; the minimum is set_size - 1 fmin on distances the scan forms anyway, and a row that does
 * not beat the set's depth-th entry costs one compare.  Two launches.
 * LIMITS and refusals: n_sets >= 1, set_size >= 1, n_sets * set_size <= 64; n_gallery, d, depth, id_base as vtc_l2_search; gallery,
 * queries and ids non-null, out_groups non-null with groups; the workspace at least vtc_l2_search_sets_workspace_bytes(...), which is 0
 * for a refused shape.  A refused call launches nothing. */
size_t vtc_l2_search_sets_workspace_bytes(int n_gallery, int n_sets, int set_size, int d, int depth, int grouped);
int vtc_l2_search_sets(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                       const int64_t *exclude, int n_gallery, int n_sets, int set_size, int d, int depth, int64_t id_base, int64_t *ids,
                       int32_t *out_groups, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* RANGE SEARCH: every row of a stored gallery that lies within a threshold of a query, however many rows that is (near-duplicate
 * detection before a video is added, "everything that matches this title", counting matches).  vtc_l2_search cannot stand in: its depth
 * is capped at 64 and a depth guessed too small truncates silently.
 * D(q, j) is the fp64 squared distance of fp32 query q and gallery row j as vtc_l2_search forms it (the one device function of the
 * sweeps: the bits that call leaves at the head of its workspace for the pair), for an fp32 gallery and for a half gallery widened
 * exactly (gallery_is_half != 0: IEEE binary16 bit patterns, as vtc_l2_search_half takes them).  Row j is a HIT of query q iff
 *   its bit of `live` is set (live == NULL: every row; the mask of vtc_l2_search_masked, only read), and
 *   D(q, j) is finite, and
 *   D(q, j) <= radius2[q], compared in fp64 (radius2: double [n_queries], device).
 * No sum of another order decides membership.  A query that holds a NaN / inf has no hits and sets bit 2 of nonfinite[0] (int32, device,
 * may be NULL, ORed into as by vtc_l2_search); a live gallery row that holds one is never a hit and sets bit 1; a dead row is not read
 * and sets nothing.  A radius2 that is NaN or negative gives no hits, +inf gives every live finite row.
 *
 * vtc_l2_range_count: ONE pass over the gallery per tile of queries (vtc_l2_search's tiles) and a small prefix launch; nothing is read
 * back by the host.  Writes lims (int64 [n_queries + 1], device): lims[0] = 0, lims[q + 1] - lims[q] = the hits of query q.  WORKSPACE
 * HEAD: after the call the first n_queries * ceil(n_gallery / 32) uint32 of the workspace are the HIT WORDS, query-major, in
 * vtc_row_mask_pack's format: word w of query q is at [q * ceil(n_gallery / 32) + w], its bit b is row 32 w + b, the bits past
 * n_gallery are 0.  The words of one query are a valid `live` argument of vtc_l2_search_masked / vtc_l2_search_half ("the nearest k
 * among the rows within the threshold").  Behind them the workspace holds counts the fill pass needs.
 *
 * vtc_l2_range_fill: after vtc_l2_range_count, with the same gallery, queries, shape and workspace (untouched in between) and the lims
 * it wrote.  For every hit, at p = lims[q] + (the rank of the row among q's hits, ASCENDING ROW ORDER) when p < capacity:
 *   ids[p] (int64) = id_base + row,  dists[p] (fp32, may be NULL) = (float) D,  dists64[p] (double, may be NULL) = D.
 * Positions at or past `capacity` are not written: a truncated result, never a store out of bounds.  D is formed again by the same
 * function -- bit-equal to what the count pass compared.  Gallery rows are read only where a hit word is non-zero, in chunks of 512
 * rows.  One launch; the order of the result does not depend on the grid (no atomic decides a position).
 *
 * LIMITS (refused with a status + vtc_last_error, nothing is launched): 1 <= n_queries <= 64, d % 64 == 0 and 64 <= d <= 2048,
 * n_gallery >= 1, capacity >= 0, id_base >= 0 with id_base + n_gallery an int64, non-null gallery / queries / radius2 / lims / ids / ws,
 * ws_bytes >= vtc_l2_range_workspace_bytes(...), which is 0 for arguments the calls refuse.
 * NOT PROVIDED: a grouped (distinct-video) range search, sharding over devices, more than 64 queries per call (slice them). */
size_t vtc_l2_range_workspace_bytes(int n_gallery, int n_queries, int d);
int vtc_l2_range_count(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const double *radius2,
                       int n_gallery, int n_queries, int d, int64_t *lims, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
int vtc_l2_range_fill(const void *gallery, int gallery_is_half, const float *queries, int n_gallery, int n_queries, int d,
                      const int64_t *lims, int64_t capacity, int64_t id_base, int64_t *ids, float *dists, double *dists64, void *ws,
                      size_t ws_bytes, void *stream);
/* THE COUNT PASS FOR MANY QUERIES over a half gallery.  DEFINITION: the result is that of vtc_l2_range_count(gallery, 1, ...) on the same
 * arguments, BIT FOR BIT -- lims, the hit words at the head of the workspace (bits past n_gallery 0), the bits ORed into nonfinite, a
 * dead row influencing nothing, live == NULL meaning every row, a NaN / negative / +inf radius2 -- and behind the hit words the workspace
 * holds, at vtc_l2_range_workspace_bytes' offsets, what vtc_l2_range_fill(gallery, 1, ...) needs: that call follows on the SAME workspace,
 * unchanged.  The entry has no specification of its own.
 * MECHANISM (range_many.hip): three launches whatever the data, no host synchronisation, no allocation, nothing read back.  The query
 * prologue of vtc_l2_search_many_half; ONE pass that streams the gallery through v_mfma_f32_16x16x32_f16 for the approximate distance A
 * of that entry, whose bound holds per pair, |A - D| <= eps = kappa (|q|^2 + |g|^2) + 1e-35: a pair with A + eps <= radius2 is a hit,
 * one with A - eps > radius2 is not, and only a pair in between -- or one whose A is not finite, or whose query is too small for the
 * split -- is decided by its fp64 distance D, formed by the scan's own device function from the bits the scan reads; then
 * vtc_l2_range_count's prefix launch.  A hit word with no live row inside the gallery issues no gallery load.
 * COST: one gallery pass per call for up to 64 queries (vtc_l2_range_count: one per 8); measured in profiles/range_many.md.
 * THE COUNTER: behind vtc_l2_range_count's regions -- at byte vtc_l2_range_workspace_bytes(n_gallery, n_queries, d) +
 * ceil(n_queries / 16) * 64 * d + 768 of the workspace -- one int64 holds the number of (query, row) pairs of this call that were
 * decided by their fp64 distance.
 * LIMITS and refusals (a status, vtc_last_error, nothing launched): vtc_l2_range_count's -- 1 <= n_queries <= 64 (more: slice them),
 * d % 64 == 0 and 64 <= d <= 2048, n_gallery >= 1, non-null gallery / queries / radius2 / lims / ws -- and ws_bytes >=
 * vtc_l2_range_many_workspace_bytes(...), which is 0 for a refused shape and at least vtc_l2_range_workspace_bytes(...).
 * NOT PROVIDED: fp32 galleries (their rows are no MFMA operand), a grouped (distinct-video) range, more than 64 queries per call. */
size_t vtc_l2_range_many_workspace_bytes(int n_gallery, int n_queries, int d);
int vtc_l2_range_count_many_half(const uint16_t *gallery, const float *queries, const uint32_t *live, const double *radius2, int n_gallery,
                                 int n_queries, int d, int64_t *lims, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* ---- 8-BIT GALLERY STORAGE (q8): one signed byte per component and one fp32 scale per row, searched exactly AS STORED.
 * A Q8 ROW of width d (a multiple of 64 in [64, 2048]) is d + 16 = vtc_q8_row_bytes(d) bytes: d signed codes c_k (int8; -128 is legal),
 * then the row's fp32 scale s at byte d, then 12 bytes that are written as zero and never read.  A q8 gallery is [n][d + 16] bytes with
 * a 16-byte aligned base: one pointer.  THE STORED VALUE of component k is the IEEE single-precision product fl32(s * c_k), subnormal
 * results kept.  (The quantiser below only produces scales with 16 significant bits, low 8 mantissa bits zero: with |c| <= 128 the
 * product is then exact; a caller's scale with more bits gets the rounded product.)  A row whose scale is NaN or +-inf is a non-finite
 * row: it sets bit 1 of nonfinite and is never a candidate, as a half row with an inf is.  A scale of 0 is a row of zeros.
 * THE SEARCH over a q8 gallery is, BIT FOR BIT, the fp32 search over the fp32 gallery of those stored values -- ids, dists, the fp64
 * distances at the head of the workspace, groups, hit words and lims, in every mode: the kernels are the fp32 ones with another row
 * loader (4 bytes a lane a piece, one load of the scale a row, four conversions, four multiplies) and the same summation order.
 * Nothing about the search is defined a second time: each entry below is the named entry without gallery_is_half, with that entry's
 * workspace size (vtc_l2_search_workspace_bytes / _grouped_ / _sets_ / vtc_l2_range_workspace_bytes), limits, refusals and messages.
 * vtc_l2_search_merge / vtc_l2_search_merge_grouped take windows of q8 galleries as they are.
 *   vtc_l2_search_q8            all six scans: vtc_l2_search_masked (only live, nullable), vtc_l2_search_grouped (groups), vtc_l2_search_after
 *                               (after_d / after_i), vtc_l2_search_excluding (exclude; with groups or with a nullable cursor) and
 *                               vtc_l2_search_grouped_after (groups + ban + n_groups + the cursor; exclude nullable).  Everything from live to
 *                               after_i is nullable; n_groups is looked at only with ban; the combinations are those entries'.
 *   vtc_l2_search_sets_q8, vtc_l2_group_mark_before_q8, vtc_l2_pair_dists64_q8, vtc_l2_range_count_q8, vtc_l2_range_fill_q8
 * THE QUANTISER, vtc_quantize_rows_q8: x [n][d] fp32 -> rows_out [n][d + 16], one launch, a wave per row, all in fp32 arithmetic with
 * correctly rounded divisions:  m = max_k |x_k|;  t = fl32(m / 127);  s = t rounded UP to 16 significant bits, bits(s) = (bits(t) +
 * 0xFF) & ~0xFF;  s = 1 when m = 0;  c_k = clamp(rint(fl32(x_k / s)), -127, 127), rint to nearest even.  So |x_k - s c_k| <=
 * 0.5 (1 + 2^-15) s.  A row with a NaN / inf gets s = NaN and all-zero codes and sets bit 1 of nonfinite (nullable).
 * NOT PROVIDED: the many-query MFMA passes over q8 galleries; vtc_l2_topk; per-block or asymmetric scales; quantised queries. */
size_t vtc_q8_row_bytes(int d);      /* d + 16; 0 for a d the search refuses */
int vtc_quantize_rows_q8(const float *x, int n, int d, void *rows_out, int *nonfinite, void *stream);
int vtc_l2_search_q8(const void *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int n_groups, const uint32_t *ban,
                     const int64_t *exclude, const double *after_d, const int64_t *after_i, int n_gallery, int n_queries, int d, int depth,
                     int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
int vtc_l2_search_sets_q8(const void *gallery, const float *queries, const uint32_t *live, const int32_t *groups, const int64_t *exclude,
                          int n_gallery, int n_sets, int set_size, int d, int depth, int64_t id_base, int64_t *ids, int32_t *out_groups,
                          float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
int vtc_l2_group_mark_before_q8(const void *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int n_groups,
                                const double *after_d, const int64_t *after_i, int n_gallery, int n_queries, int d, int64_t id_base,
                                uint32_t *ban, void *stream);
int vtc_l2_pair_dists64_q8(const void *gallery, const float *queries, const int64_t *rows, int n_gallery, int n_queries, int d, int64_t id_base,
                           double *out, void *stream);
int vtc_l2_range_count_q8(const void *gallery, const float *queries, const uint32_t *live, const double *radius2, int n_gallery, int n_queries,
                          int d, int64_t *lims, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
int vtc_l2_range_fill_q8(const void *gallery, const float *queries, int n_gallery, int n_queries, int d, const int64_t *lims, int64_t capacity,
                         int64_t id_base, int64_t *ids, float *dists, double *dists64, void *ws, size_t ws_bytes, void *stream);
/* hits[j] +=#{ i : (target_offset + i) in ids[i, :k_vals[j]] }   (hits: int64 device) */
int vtc_recall_hits(const int64_t *ids, int n_queries, int depth, int64_t target_offset, const int *k_vals_host,
                    int nk, long long *hits, void *stream);
/* R@K of BOTH directions of n PAIRED rows (a_i <-> b_i: RecallAtK.result(), model/metric.py:166-187; evaluation/eval.py:117-127) without the
 * sorted neighbour lists (round 5).  The reference asks one thing of its search -- is the query's own index among the first k -- which is
 * the RANK of one gallery row: #{ j : (|q - g_j|^2, j) < (|q - g_t|^2, t) } < k.  One prologue, ONE distance GEMM (the block-minima
 * planes of vtc_l2_topk_bidir), ONE rank launch: entries whose key is more than the row's error bound away from the target's exact
 * distance are counted or dropped unseen, the few in reach are settled in fp64.  The counters are those of vtc_l2_topk_bidir(depth =
 * max k + 1, VTC_SWEEP_EXACT) followed by vtc_recall_hits_pair, exactly.  hits_*: nk device int64 each, ADDED to:
 *   hits_b_from_a[j] += #{ i : a_i is among the k_j nearest a's of b_i }   = RecallAtK.compute(a, b) x n
 *   hits_a_from_b[j] += #{ i : b_i is among the k_j nearest b's of a_i }   = RecallAtK.compute(b, a) x n
 * n >= 1024, d % 64 == 0 (vtc_l2_recall_bidir_supported; else the two-call form); nk <= 4; k_vals on the host.
 * Non-finite embeddings (ABI 7): a pair whose target distance |a_i - b_i|^2 is NaN / inf -- any NaN or inf in a_i or b_i -- is a MISS at
 * every k (an exact search never returns such a target), and the call ORs VTC_RECALL_NONFINITE (bit 40) into hits_b_from_a[0] and
 * hits_a_from_b[0]: the caller learns of it from the counters it reads anyway (counter = value & (VTC_RECALL_NONFINITE - 1); the host
 * layer raises).  The same holds for vtc_l2_recall_shard_rows / _cols (bit 40 survives the sum over <= 2^22 ranks). */
#define VTC_RECALL_NONFINITE (1ll << 40)
int vtc_l2_recall_bidir_supported(int n, int d);
size_t vtc_l2_recall_bidir_workspace_bytes(int n, int d);
int vtc_l2_recall_bidir(const float *a, const float *b, int n, int d, const int *k_vals_host, int nk, long long *hits_b_from_a,
                        long long *hits_a_from_b, void *ws, size_t ws_bytes, void *stream);
/* FULL ranks of both directions of n PAIRED rows (a_i <-> b_i), for median / mean rank, MRR and recall at ANY k:
 *   rank_a[i] = #{ j : (|b_i - a_j|^2, j) < (|b_i - a_i|^2, i) }   gallery a, query b_i   (the direction of RecallAtK.compute(a, b))
 *   rank_b[i] = #{ j : (|a_i - b_j|^2, j) < (|a_i - b_i|^2, i) }   gallery b, query a_i   (the direction of RecallAtK.compute(b, a))
 * 0-based int64 (device, n each); pairs compare lexicographically on the fp64 distances sum_k (q_k - g_k)^2 of the fp32 inputs, so exact
 * ties go to the lower index and  #{ i : rank[i] < k }  are the counters of vtc_l2_recall_bidir, bit for bit, for every k.
 * The sweep COUNTS instead of selecting: the split-bf16 distance GEMM of VTC_SWEEP_BF16X3 writes row blocks (rows_per_block as in
 * vtc_l2_topk; 0 = as many rows as fit 2 GiB; a row holds n rounded up to 4 columns, so rows are 16-byte aligned at every n and the padding
 * columns are never counted), a row pass and a column pass over each block count the entries that are closer than the
 * target by more than the BF16X3 error bound  eps = kappa (|q|^2 + max|g|^2),  kappa = the value vtc_l2_rank_kappa returns for d,  and
 * put the pairs within eps of it into a reach pool of reach_capacity pairs per direction (0 = the default, 512 n) that is settled in fp64.
 * An owner whose pairs did not fit is counted again by fp64 brute force: the ranks do not depend on the capacity.
 * A gallery row with a non-finite distance is never closer; a pair whose own distance |a_i - b_i|^2 is not finite (NaN / inf anywhere in
 * a_i or b_i) gets rank n in both directions: a miss at every k.  nonfinite[0] (int32, device) = 1 if a holds a NaN / inf, | 2 if b does.
 * n >= 1, d % 64 == 0.  After the call the first eight 64-bit words of the workspace hold the sweep's statistics, (direction a, direction
 * b) each: pairs in reach, the largest number of them for one owner, owners counted by brute force; then two unused words. */
float vtc_l2_rank_kappa(int d);
size_t vtc_l2_rank_bidir_workspace_bytes(int n, int d, int rows_per_block, int reach_capacity);
int vtc_l2_rank_bidir(const float *a, const float *b, int n, int d, int rows_per_block, int reach_capacity, int64_t *rank_a,
                      int64_t *rank_b, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* The paired sweep over a WINDOW of rows: one rank's share of a row-sharded evaluation.  The caller holds both gathered sets (a_all, b_all:
 * [n_total, d]) and owns the rows [row_base, row_base + n_local) of D(i, j) = |b_i - a_j|^2 (notation and arithmetic of vtc_l2_rank_bidir:
 * fp64 distances of the fp32 inputs from the sweep's one device function, pairs compared lexicographically).
 *   rank_a_local[i] = rank_a[row_base + i] of vtc_l2_rank_bidir(a_all, b_all)             i in [0, n_local): complete, the rank holds whole rows
 *   rank_b_part[j]  = #{ i in [row_base, row_base + n_local) : (D(i, j), i) < (D(j, j), j) }      if D(j, j) is finite
 *                   = n_total if row_base <= j < row_base + n_local, else 0                        otherwise
 * for EVERY j in [0, n_total), written, not added to.  Summed over any disjoint windows that cover [0, n_total), rank_b_part is rank_b of
 * vtc_l2_rank_bidir, element for element: counts are sums, and a pair without a finite distance gets its rank n_total from the one window
 * that owns its row.  A local pair without a finite distance has rank_a_local = n_total.  nonfinite[0] is that of the paired call, over
 * all of a_all and b_all: the same word on every rank.
 * The thresholds are the paired call's: a row's eps = kappa (|b_i|^2 + max_j |a_j|^2), a column's eps = kappa (|a_j|^2 + max_i |b_i|^2)
 * with the maximum over ALL of b_all, so the pairs a window settles in fp64 are exactly the paired call's pairs that lie in it.  The
 * statistics words keep their meaning, restricted to the window: direction a counts the local owners, direction b all columns against
 * the local rows.  With row_base = 0, n_local = n_total both outputs and the eight words are those of vtc_l2_rank_bidir, element for element.
 * n_total >= 1, 0 <= row_base, 0 <= n_local, row_base + n_local <= n_total, d % 64 == 0.  n_local = 0 is valid (fewer rows than ranks):
 * no distance GEMM runs and rank_b_part is all zero.  Workspace: what grows with the rank's share has n_local entries (the split-bf16
 * query operands, the distance block -- rows_per_block is capped at n_local --, the row direction's thresholds, counters and default
 * pool, 512 n_local pairs); the gallery operands and the column direction's arrays are O(n_total). */
size_t vtc_l2_rank_shard_workspace_bytes(int n_total, int n_local, int d, int rows_per_block, int reach_capacity);
int vtc_l2_rank_shard(const float *a_all, const float *b_all, int n_total, int row_base, int n_local, int d, int rows_per_block,
                      int reach_capacity, int64_t *rank_a_local /* [n_local] */, int64_t *rank_b_part /* [n_total] */, int *nonfinite,
                      void *ws, size_t ws_bytes, void *stream);
/* The same ranks for videos with SEVERAL captions each (MSR-VTT: 20 per video, MSVD: about 40).  a [n, d]: one row per video; b [m, d]: the
 * captions, those of one video contiguous and in video order; off [n + 1] (device int32): non-decreasing, off[0] = 0, off[n] = m.  Caption c
 * belongs to video g(c), the v with off[v] <= c < off[v + 1].  With D(c, j) the fp64 value sum_k (b_c[k] - a_j[k])^2 of the fp32 inputs
 * (formed by the one device function of the paired sweep, so exact ties are bit-equal) and pairs compared lexicographically:
 *   rank_a[c] = #{ j in [0, n) : (D(c, j), j) < (D(c, g(c)), g(c)) }    c in [0, m)   text -> video: the caption queries the videos
 *   rank_b[v] = #{ c in [0, m) : (D(c, v), c) < (D(c*, v), c*) }        v in [0, n)   video -> text: the video queries ALL captions;
 *               c* = the own caption (off[v] <= c < off[v + 1], D finite) with the smallest (D(c, v), c)
 * rank_b is the CAPTION-LEVEL convention of the image-text literature: the best rank any own caption reaches in the list of all m
 * captions.  No own caption can precede c*, so rank_b[v] counts captions of other videos.  (The video-unit convention -- the number of
 * other videos that have a closer caption -- is vtc_l2_rank_grouped_vunit, below.)
 * An entry with a non-finite distance is never closer; a caption whose own distance is not finite gets rank_a = n and is no candidate
 * for c*; a video without a finite own caption (an empty group too) gets rank_b = m; nonfinite[0] as above.  With m = n and
 * off = 0, 1, ..., n both outputs are those of the paired entry point, element for element.
 * The sweep is the paired one made rectangular (D is [m, n], rows padded alike, rows_per_block caption rows per block), the owner's target taken from a table;
 * the reach pool of a direction holds reach_capacity pairs (0 = the default, 512 per owner: 512 m for the captions, 512 n for the
 * videos, at least 4096).  Everything is on the device, off included: no host sync, no allocation.  n >= 1, m >= 1, d % 64 == 0.  The
 * statistics words at the head of the workspace are the paired entry point's (direction a = the captions' row direction). */
size_t vtc_l2_rank_grouped_workspace_bytes(int n, int m, int d, int rows_per_block, int reach_capacity);
int vtc_l2_rank_grouped(const float *a, const float *b, const int *off, int n, int m, int d, int rows_per_block, int reach_capacity,
                        int64_t *rank_a /* [m] */, int64_t *rank_b /* [n] */, int *nonfinite, void *ws, size_t ws_bytes, void *stream);
/* The same sweep with a third output, video -> text in the VIDEO-UNIT convention of the video-retrieval literature (multi-sentence
 * evaluation): the [caption, video] distances are first reduced to one best caption per (video, video) pair, then the video's own group
 * is ranked among the n groups.  With the notation above:
 *   E(u, v)   = min { D(c, v) : off[u] <= c < off[u + 1], D(c, v) finite }      (+inf if there is none)
 *   rank_v[v] = #{ u in [0, n), u != v : (E(u, v), u) < (E(v, v), v) }           if E(v, v) is finite
 *             = n                                                                otherwise (no finite own caption, an empty group too)
 * E(v, v) = D(c*, v), the target distance of rank_b.  A group without a finite distance to v (an empty group, a NaN video row, all of its
 * captions NaN) is never closer; an exact tie goes to the lower VIDEO index.  rank_v[v] <= rank_b[v], rank_v[v] == 0 exactly when
 * rank_b[v] == 0, and with m = n, off = 0, 1, ..., n rank_v is rank_b of the paired entry point, element for element.
 * rank_a and rank_b are those of vtc_l2_rank_grouped on the same inputs, element for element: one sweep, three outputs, all required.
 * A third pass over each distance block takes the smallest key of every (group, video) -- groups that lie across row blocks are joined
 * through a per-column carry before they are classified --, counts the groups below the video's lo, and puts those in reach of its
 * target into a pool of (video, group) pairs of the column direction's capacity, settled in fp64 over the group's captions; a video whose
 * pairs did not fit is counted again by fp64 brute force over all m captions, group by group: the ranks do not depend on the capacity.
 * Beyond the distance block nothing of size m x n or n x n is resident: the direction adds O(n) words and its pool to the workspace.
 * Whatever off holds, nothing is read or written out of bounds; results are defined for valid offsets only.
 * The first eight statistics words of the workspace keep their meaning; words 8, 9, 10 hold the video-unit direction's: (video, group)
 * pairs in reach, the largest number of them for one video, videos counted by brute force; then five unused words. */
size_t vtc_l2_rank_grouped_vunit_workspace_bytes(int n, int m, int d, int rows_per_block, int reach_capacity);
int vtc_l2_rank_grouped_vunit(const float *a, const float *b, const int *off, int n, int m, int d, int rows_per_block, int reach_capacity,
                              int64_t *rank_a /* [m] */, int64_t *rank_b /* [n] */, int64_t *rank_v /* [n] */, int *nonfinite, void *ws,
                              size_t ws_bytes, void *stream);
/* The sharded sweep (above) with the recall-only finish: rank r holds rows [row_base, row_base + n_local) of both sets and the gathered
 * sets, runs ONE [n_local, n_total] distance GEMM and adds its PARTIAL counters (the host all-reduces them: model/metric.py:148-160 counted
 * over this rank's queries):
 *   vtc_l2_recall_shard_rows   hits_b_from_a[j] += #{ i local : a_(row_base + i) among the k_j nearest a's of b_(row_base + i) };
 *                              col_planes [P, nblk_pad, n_total] in vtc_l2_sweep_shard_rows' layout, P = vtc_l2_recall_planes(k_vals, nk, n_total):
 *                              for max k <= 16 two planes (per column and block the smallest key + the second as a bound; n_total >= 16 384)
 *                              or three (two keys + bound), else four
 *   (host) all-to-all of the column planes, as above
 *   vtc_l2_recall_shard_cols   planes [n_src, P, nblk_pad, n_local]; src_bounds [n_src + 1] (device int32): source s ran rows
 *                              [src_bounds[s], src_bounds[s + 1]);  hits_a_from_b[j] += #{ i local : b_(row_base + i) among the k_j nearest
 *                              b's of a_(row_base + i) }
 * Summed over the ranks: the counters of vtc_l2_recall_bidir on the gathered sets, exactly.  n_total >= 1024, d % 64 == 0, nk <= 4;
 * workspace: vtc_l2_sweep_shard_workspace_bytes. */
int vtc_l2_recall_shard_supported(int n_total, int n_local, int d);
int vtc_l2_recall_planes(const int *k_vals_host, int nk, int n_total);
int vtc_l2_recall_shard_rows(const float *a_all, const float *b_local, int n_total, int n_local, int row_base, int d,
                             const int *k_vals_host, int nk, long long *hits_b_from_a, unsigned *col_planes, int nblk_pad, void *ws,
                             size_t ws_bytes, void *stream);
int vtc_l2_recall_shard_cols(const float *b_all, const float *a_local, int n_total, int n_local, int row_base, int d,
                             const int *k_vals_host, int nk, const unsigned *planes, int n_src, int nblk_pad, const int *src_bounds,
                             long long *hits_a_from_b, void *ws, size_t ws_bytes, void *stream);
/* the same for the two directions of one evaluation (RecallAtK.result(), model/metric.py:166-187: compute(a, b) and compute(b, a),
 * same number of queries and the same targets) in ONE launch */
int vtc_recall_hits_pair(const int64_t *ids_a, const int64_t *ids_b, int n_queries, int depth, int64_t target_offset,
                         const int *k_vals_host, int nk, long long *hits_a, long long *hits_b, void *stream);

/* ---- primitives (exported for parity tests and reuse) -------------------------------- */
enum { VTC_EPI_STORE = 0,   /* out = acc + bias                      (out dtype = out_dtype) */
       VTC_EPI_GELU = 1,    /* out = QuickGELU(acc + bias)                                     */
       VTC_EPI_RESID = 2 }; /* out(fp32) += acc + bias; rows with m % skip_mod == 0 untouched  */
/* out[M,N] = epi(A[M,K] @ W[N,K]^T + bias).  A, W in `dtype`; K % 64 == 0 (bf16) / % 32 (fp32). */
int vtc_gemm(const void *A, const void *W, const float *bias, void *out, int M, int N, int K, int dtype,
             int epilogue, int out_dtype, int skip_mod, void *stream);
/* Residual GEMM + the LayerNorm that follows it, one launch (16-bit operand formats; N a multiple of 256, <= 1024; problems
 * large enough for the 256 x 256 kernel -- ask vtc_gemm_resid_layernorm_supported):  out(fp32) += A W^T + bias with rows
 * m % skip_mod == 0 untouched, then ln_out[M,N] (operand format) = LayerNorm(out) * ln_g + ln_b.  Bit-identical to
 * vtc_gemm(VTC_EPI_RESID) + vtc_layernorm.  Replaces e.g. `x = x + attn(...)` followed by `ln_2(x)`
 * (model/timesformer_clip_alt.py:173-174).  ln_out may alias A (a row block's A rows are dead when its LayerNorm runs). */
size_t vtc_gemm_resid_layernorm_workspace_bytes(int M);
int vtc_gemm_resid_layernorm_supported(int M, int N, int K, int dtype);
int vtc_gemm_resid_layernorm(const void *A, const void *W, const float *bias, float *out, int M, int N, int K, int dtype,
                             int skip_mod, const float *ln_g, const float *ln_b, void *ln_out, void *ws, size_t ws_bytes,
                             void *stream);
/* y[r,:] = LN(x[row(r),:]) * g + b, row(r) = row_index ? row_index[r] : r * row_mul; out dtype selectable */
int vtc_layernorm(const float *x, const float *g, const float *b, void *y, int rows, int width, int out_dtype,
                  const int *row_index, int row_mul, void *stream);
/* softmax(q k^T / sqrt(64) [+causal]) v per (sequence, head) on a packed qkv buffer [rows, 3W];
 * token p of sequence s lives at row  (s / s2) * a1 + (s % s2) * a2 + a0 + (p ? 1 + (s % s2) * a3 + (p - 1) * pstride : 0).
 * out: [rows, W] (same row map).  If cls_out != NULL the p == 0 output goes to cls_out[s, W] (fp32) instead. */
int vtc_attention(const void *qkv, void *out, float *cls_out, int n_seq, int L, int heads, int causal, int s2, int a0,
                  int a1, int a2, int a3, int pstride, int dtype, void *stream);

/* ONE query per sequence (the last block of a tower, where only the row that reaches the output asks): sequence o attends
 * with the projected query q[o / s2] (q: [n_q, W], operand format, compact) over its keys and values in the packed qkv buffer (key rows:
 * the map of vtc_attention; the Q third of qkv is not read).  eot != NULL instead: the text tower's rows base .. eot[o], base =
 * offs ? offs[o] : o * ctx, query q[o].  out [n_out, W] fp32.  fp32 arithmetic throughout. */
int vtc_single_query_attention(const void *qkv, const void *q, float *out, int n_out, int L, int heads, int s2, int a0, int a1, int a2,
                               int a3, int pstride, const int *eot, const int *offs, int ctx, int dtype, void *stream);

/* ---- adapter-only training step: backward + optimizer primitives, fp32 -------------------
 * Replace, for PretrainedCLIP_finaltf with frozen towers (configs/pretrained_clip_comments_attn_frozen.jsonc), what
 * torch.autograd does behind `loss.backward()` (trainer/trainer.py) for clip_loss (model/loss.py:18-22), normalize
 * (model/model.py:26-27) and the CAM transformer (clip.model.Transformer, model/model.py:396-398), and
 * torch.optim.Adam(amsgrad=True).step().  Orchestrated by vtc_amd/host/adapter_train.py; dgrad / wgrad matrix
 * products are vtc_gemm calls on transposed operands. */
int vtc_transpose_f32(const float *x, float *y, int rows, int cols, void *stream);            /* y[c][r] = x[r][c] */
int vtc_colsum_f32(const float *x, float *out, int rows, int cols, void *stream);             /* bias gradients     */
/* dx (+)= LN'(x; gamma)(dy), dgamma = sum_r dy xhat, dbeta = sum_r dy (eps 1e-5, biased variance) */
int vtc_layernorm_bwd(const float *x, const float *gamma, const float *dy, float *dx, float *dgamma, float *dbeta, int rows,
                      int width, int accumulate_dx, void *stream);
/* unmasked attention backward, L <= 16, head_dim 64, sequences contiguous: qkv [n_seq*L, 3W], dout [n_seq*L, W] */
int vtc_attention_small_bwd(const float *qkv, const float *dout, float *dqkv, int n_seq, int L, int heads, void *stream);
/* QuickGELU: dy == NULL -> out = x sigmoid(1.702 x); else out = dy * d/dx */
int vtc_quickgelu(const float *x, const float *dy, float *out, size_t n, void *stream);
int vtc_normalize_rows_bwd(const float *x, const float *dy, float *dx, int n, int d, void *stream);
/* dsim = d clip_loss / d sim; ws >= 4 n floats */
int vtc_clip_loss_bwd(const float *sim, int n, float *dsim, void *ws, size_t ws_bytes, void *stream);
/* torch.optim.Adam single-tensor step (weight_decay 0); step counts from 1; vmax only when amsgrad (NULL otherwise).  The bias
 * corrections 1 - beta^step are formed in double from the float betas, as torch.optim forms them from its Python floats */
int vtc_adam_step(float *p, const float *g, float *m, float *v, float *vmax, size_t n, float lr, float beta1, float beta2,
                  float eps, int step, int amsgrad, void *stream);
int vtc_axpby(float *out, const float *x, const float *y, float a, float b, size_t n, void *stream);   /* out = a x + b y  */
int vtc_scale_rows(float *x, const float *s, int rows, int d, int group, void *stream);               /* x[r] *= s[r/group] */

/* ---- optional per-launch timing (HIP events on the launch stream; bench/diagnostics) ----
 * Between vtc_prof_begin() and vtc_prof_end() every kernel launch of the library is bracketed by
 * two events.  vtc_prof_end synchronises `stream` and returns, per class, the summed kernel time,
 * the launch count and the summed work (FLOPs = 2MNK for GEMM, 4*L*L*64 per (sequence, head) for
 * attention; bytes moved for the others).  Process-global, single-threaded use only. */
enum { VTC_PROF_GEMM_BF16 = 0, VTC_PROF_GEMM_F32 = 1, VTC_PROF_ATTN = 2, VTC_PROF_NORM = 3, VTC_PROF_EMBED = 4,
       VTC_PROF_TOPK = 5, VTC_PROF_NCLASS = 6 };
/* Launches also carry the region of the tower they belong to (per thread): the attention branches (LayerNorm + QKV
 * projection + attention core + output projection [+ temporal_fc] + cls bookkeeping -- what BASELINE.md calls
 * "TimeSformer attention" for the video tower), the MLP branches, everything else. */
enum { VTC_PROF_REGION_OTHER = 0, VTC_PROF_REGION_ATTN = 1, VTC_PROF_REGION_MLP = 2, VTC_PROF_NREGION = 3 };
int vtc_prof_begin(void);
int vtc_prof_end(void *stream, double *ms, long long *launches, double *work);
/* as vtc_prof_end, split by region: arrays of VTC_PROF_NCLASS * VTC_PROF_NREGION, index cls * VTC_PROF_NREGION + region */
int vtc_prof_end_regions(void *stream, double *ms, long long *launches, double *work);
/* as vtc_prof_end, one record per launch (at most `max`; returns the count through *n): class, region, time, work and, for
 * GEMM launches, tag[3 i ..] = (epilogue mode, N, K) -- bench.py groups them to report the dominant single instantiation */
int vtc_prof_end_records(void *stream, int max, int *n, int *cls, int *region, double *ms, double *work, int *tag);
/* kernel launches made by the library since it was loaded (every launch site counts; diagnostics / bench) */
long long vtc_debug_launch_count(void);

#ifdef __cplusplus
}
#endif
#endif /* VTC_HIP_H */
