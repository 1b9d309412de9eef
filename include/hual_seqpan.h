/* libhual_seqpan.so - C ABI of the MI355X-native SeqPAN hot path of renjie-liang/HUAL.
 *
 * The reference has no FFI, plugin or operator registry: its hot path is a TensorFlow-1 graph
 * (/root/reference/models/model.py:7-122) entered only through `sess.run(fetches, feed_dict)` at
 *   /root/reference/utils/runner_utils.py:147   [train_op, loss, start_index, end_index]
 *   /root/reference/utils/runner_utils.py:166   [start_index, end_index]
 *   /root/reference/utils/runner_utils.py:75-81 match_scores / [start_logits, end_logits]
 * This header is the boundary a binding for that path would sit on: the feeds of
 * model.py:15-27 (`_add_placeholders`) are `hual_batch` + `hual_labels`, the fetches are `hual_outputs`,
 * `train_op` (models/ops.py:119-132) is hual_seqpan_backward + hual_adamw_clip_step.
 *
 * Conventions
 *  - extern "C", plain C structs, plain pointers and sizes; no torch / C++ types.
 *  - EVERY pointer is DEVICE memory owned by the caller (parameters, inputs, outputs, workspace);
 *    the library never allocates, frees or synchronises.  All work is enqueued on `stream`
 *    (a hipStream_t passed as void*), so a whole step can be captured into a hipGraph.
 *  - return 0 on success, negative on error; message via hual_last_error() (thread local).
 *    No C++ exception crosses the ABI.
 *  - re-entrant: the compute entry points keep no global mutable state; one stream per device/rank is safe.  The one exception
 *    is the OPTIONAL per-kernel timing of bench.py's roofline leg (hual_prof_begin / hual_prof_end / hual_prof_get below): a
 *    thread-local recorder that is off unless armed, and whose hual_prof_end() is the only call that synchronises.
 *  - kernels are specialised for gfx950 and model.dim = 128, num_heads = 8 (the value in both
 *    configs/<task>/SeqPAN.yaml); other values are rejected by hual_seqpan_validate().
 */
#ifndef HUAL_SEQPAN_H
#define HUAL_SEQPAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HUAL_ABI_VERSION 9

#define HUAL_OK 0
#define HUAL_ERR_INVALID (-1)
#define HUAL_ERR_HIP (-2)
#define HUAL_ERR_UNSUPPORTED (-3)
#define HUAL_ERR_WORKSPACE (-4)

/* dropout call-site ids (Philox counter word c2); mirrors oracle/philox.py SITE_* and DESIGN.md */
#define HUAL_SITE_WORD 0
#define HUAL_SITE_CHAR 1
#define HUAL_SITE_VIDEO 2
#define HUAL_SITE_CONV 3
#define HUAL_SITE_DA 8
#define HUAL_SITE_TRI 24
#define HUAL_SITE_GUMBEL 28   /* gumbel noise of the matching head (layers.py:163-166): RNG row = b*T+t, one call = the 4 classes */
#define HUAL_SITE_FE 32
#define HUAL_SITE_SELECT 256  /* not a dropout site: the exponentials of hual_kcenter_sample, c0 = step, c1 = row, word x.  Above every
                                 dropout site (the largest is HUAL_SITE_FE + 16 * pass + 8) */

/* keys of configs/<task>/SeqPAN.yaml read by models/model.py (model.py:17,36-43,61,83,101,122) */
typedef struct hual_cfg {
  int32_t vdim;        /* model.vdim      */
  int32_t dim;         /* model.dim  (128) */
  int32_t num_heads;   /* model.num_heads (8) */
  int32_t word_dim;    /* model.word_dim  */
  int32_t char_dim;    /* model.char_dim  */
  int32_t max_vlen;    /* model.max_vlen = rows of both position tables */
  int32_t attn_layer;  /* model.attn_layer */
  int32_t num_chars;   /* configs.num_chars */
  int32_t num_words;   /* rows of [zero; unk; word_table] */
  int32_t no_gumbel;   /* loss.no_gumbel (both YAMLs set true); 0: gumbel noise on the matching logits, (logits + noise) / tau - needs rng_state */
  float match_lambda;  /* loss.match_lambda */
  float tau;           /* loss.tau (> 0; unused when no_gumbel) */
  float clip_norm;     /* train.clip_norm */
  int32_t finetune_word_emb;   /* model.finetune_word_emb (absent = 0; modules.py:8-16 `finetune`): 1 makes the GloVe table
                                  `word_embs/word_table` [num_words-2, word_dim] a trainable variable.  It is then the LAST entry
                                  of the flat parameter layout (every other offset unchanged), the forward reads the lookup table
                                  there, the backward scatters its gradient there (after the word-dropout mask; PAD rows add
                                  nothing, unk rows go to word_embs/unk as before), and clip + AdamWeightDecay treat it as any
                                  other decayed variable: a DENSE update of every row every step (ops.py:166-170). */
} hual_cfg;

int hual_abi_version(void);
/* sizeof(hual_cfg) as this library was compiled: a binding checks it against its own copy of the struct (the layout grew a
 * trailing field, finetune_word_emb, without a change of HUAL_ABI_VERSION) */
uint64_t hual_cfg_bytes(void);
const char* hual_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Parameters.  One flat fp32 device buffer in the layout reported by hual_seqpan_param_table():
 * every trainable TF variable of models/model.py under its TF scope name and TF
 * shape, each tensor 16-byte aligned.  Gradients and both Adam slots use the same layout.
 * The GloVe table `word_embs/word_table` [num_words-2, word_dim] (modules.py:10) is separate while it is frozen (the
 * reference's SeqPAN, model.py:36); with hual_cfg.finetune_word_emb it is the last entry of the layout.
 * ------------------------------------------------------------------------------------------ */
typedef struct hual_param_entry {
  char name[112];
  uint64_t offset;       /* in floats */
  uint64_t size;         /* in floats */
  int32_t ndim;
  int32_t shape[4];
  int32_t decay;         /* 1: AdamWeightDecay applies weight decay (ops.py:123,176-184) */
} hual_param_entry;

int hual_seqpan_validate(const hual_cfg* cfg);
/* *padded_floats = size of the flat buffer, *count = number of trainable scalars (1,186,508 for Charades; with
 * finetune_word_emb plus (num_words-2) * word_dim) */
int hual_seqpan_param_count(const hual_cfg* cfg, uint64_t* padded_floats, uint64_t* count);
/* returns the number of entries (fills at most max_entries) or a negative error */
int hual_seqpan_param_table(const hual_cfg* cfg, hual_param_entry* out, int max_entries);

/* feeds of model.py:15-27 (`_add_placeholders`); all device pointers */
#define HUAL_DTYPE_F32 0
#define HUAL_DTYPE_BF16 1
typedef struct hual_batch {
  const void* video;              /* video_inputs [B,T,vdim] of `video_dtype`, rows beyond video_seq_len zero padded */
  const int32_t* video_seq_len;   /* [B]; max must equal T (model.py:31) */
  const int32_t* word_ids;        /* [B,L], 0 = PAD, 1 = unk */
  const int32_t* char_ids;        /* [B,L,C], 0 = PAD, C >= 4 */
  int32_t B, T, L, C;
  int32_t video_dtype;            /* HUAL_DTYPE_F32 (the reference's float32 placeholder, model.py:17) or HUAL_DTYPE_BF16:
                                     bfloat16 clip features (BASELINE.json configs[1]), read as the float32 values they
                                     are - half the bytes of the feature-load phase, same arithmetic behind the load.
                                     Needs vdim % 256 == 0 and vdim <= 1024 (the K-split feature-load kernel). */
} hual_batch;

typedef struct hual_labels {
  const float* y1;                /* start_indexes f32 [B,T] (soft labels) */
  const float* y2;                /* end_indexes   f32 [B,T] */
  const int32_t* match_labels;    /* i32 [B,T] in 0..3 */
  const float* inner_labels;      /* f32 [B,T] */
} hual_labels;

/* fetches used by runner_utils.py:75-81,147,166 */
typedef struct hual_outputs {
  float* start_logits;            /* f32 [B,T] raw (unmasked beyond v_len, as the reference) */
  float* end_logits;              /* f32 [B,T] */
  float* match_scores;            /* f32 [B,T,4] */
  int64_t* start_index;           /* i64 [B] */
  int64_t* end_index;             /* i64 [B] */
  float* loss_terms;              /* f32 [4]: loss, loc_loss, match_loss, align_loss (written only with labels) */
} hual_outputs;

typedef struct hual_run_opts {
  float drop_rate;                /* the `dropout_rate` placeholder (0 = inference) */
  const uint32_t* rng_state;      /* device u32[3] = {seed lo, seed hi, offset}; may be NULL when drop_rate == 0 and cfg.no_gumbel */
  float match_denom_override;     /* > 0: denominator of the masked matching loss (exact data parallel) */
  int32_t align_external;         /* 1: the [B,B] alignment loss is evaluated by the caller through
                                        hual_align_loss() on gathered features (exact data parallel) */
  int32_t static_tables;          /* 1: the caller guarantees that a previous hual_seqpan_backward ran with the SAME
                                        cfg, shapes, params / grads / workspace / batch pointers, so the device-resident
                                        job tables it left in the workspace are still valid and are not rewritten
                                        (saves six tiny launches per step inside a replayed hipGraph) */
  const float* match_denom_dev;   /* non-NULL: the denominator of the masked matching loss is read from this DEVICE scalar
                                        when the kernels run (takes precedence over match_denom_override): a data-parallel
                                        step can all-reduce the valid-frame count on the stream without a host round trip */
  int32_t debug_taps;             /* 1: the forward also writes the tensors that only parity tests read (the relu outputs of the
                                        conv_block layers, "cb.y*" / "fe*.y*" of the workspace table); the backward pass never
                                        reads them (it reads the bit planes "*.rb*" / "*.kb*") */
  float* grads_prezero;           /* non-NULL together with prezero_token, hual_seqpan_forward with labels: this flat gradient
                                        buffer is zeroed by the forward's first launch (one launch fewer per step) */
  uint64_t* prezero_token;        /* HOST word owned by the caller, the receipt of that zeroing: the forward stores the address of
                                        the buffer it zeroed there once the launch is enqueued; hual_seqpan_backward skips its own
                                        zeroing launch only if the word holds the address of its `grads`, and clears it.  Any
                                        sequence that breaks the pairing (two backward calls, a forward that failed or had no
                                        labels) therefore zeroes the bucket in backward as before.  NULL: no pre-zeroing. */
  float* deferred_loss_terms;     /* non-NULL (ABI 7), a TRAIN step whose backward call follows on the same stream: the forward leaves the
                                        closing of the loss (matching-loss denominator, the four reported terms) to the backward pass,
                                        which writes float[4] = {total, loc, match, align} HERE from inside its matching-head launch -
                                        one launch fewer per step.  hual_outputs.loss_terms is then not written by the forward.
                                        Pass the same options to both calls.  NULL: the forward closes the loss itself (a launch). */
  void* dw_table;                 /* non-NULL (ABI 8): caller-owned DEVICE storage of >= hual_seqpan_dw_table_bytes() bytes, 16-byte aligned,
                                        for the job table of the backward's weight-gradient launch INSTEAD of the copy inside the
                                        workspace.  A caller that runs several padded shapes in ONE workspace (the epoch loop of
                                        runner_utils.py:139-159) keeps one such table per shape: `static_tables` then holds per
                                        TABLE - whatever other shapes did to the workspace in between - and every replayed step graph
                                        drops the table-writing launches.  NULL: the table lives in the workspace. */
  uint64_t dw_table_bytes;        /* size of dw_table (checked) */
} hual_run_opts;

/* bytes a hual_run_opts.dw_table must hold (any cfg, any shape) */
uint64_t hual_seqpan_dw_table_bytes(void);

/* bytes of workspace needed for one forward(+backward) of this shape */
int hual_seqpan_query_workspace(const hual_cfg* cfg, int B, int T, int L, int C, uint64_t* bytes);

/* named intermediate tensors inside the workspace (debugging / parity taps) */
typedef struct hual_ws_entry {
  char name[48];
  uint64_t offset;       /* bytes */
  uint64_t rows, cols;   /* fp32 elements */
} hual_ws_entry;
int hual_seqpan_ws_table(const hual_cfg* cfg, int B, int T, int L, int C, hual_ws_entry* out, int max_entries);

/* word_table: the frozen GloVe table [num_words-2, word_dim] (device).  With cfg->finetune_word_emb the table is the params entry
 * `word_embs/word_table`: pass NULL or exactly that address (any other pointer is an error, not a silent choice between the two);
 * the same rule holds for hual_video_proj_ln_fwd.
 * The graph of model.py:29-118: all five fetch tensors in ONE pass (the reference runs five).  With `labels`
 * it also evaluates model.py:76-120 (losses) and keeps what backward needs in the workspace.
 * Dense weights travel as fp16 hi + lo images scaled by 2^10: a weight with |w| >= 63 does not fit.  The pass does not fail
 * silently on one: with labels the four loss terms are NaN, without labels the start / end logits are NaN and the span
 * indices -1. */
int hual_seqpan_forward(const hual_cfg* cfg, const float* params, const float* word_table, const hual_batch* batch,
                        const hual_labels* labels, const hual_outputs* out, const hual_run_opts* opts, void* workspace,
                        uint64_t ws_bytes, void* stream);

/* tf.gradients(loss, tvars) (ops.py:126): fills `grads` (flat layout, overwritten; with finetune_word_emb the gradient of the
 * word table included, in the same launch as the unk row's).  Must follow a forward with labels on the same workspace, batch
 * and rng_state. */
int hual_seqpan_backward(const hual_cfg* cfg, const float* params, const float* word_table, const hual_batch* batch,
                         const hual_labels* labels, const hual_run_opts* opts, float* grads, void* workspace,
                         uint64_t ws_bytes, void* stream);

/* clip_by_global_norm + AdamWeightDecayOptimizer.apply_gradients (ops.py:127-132,149-174).
 * decay: per-element weight decay rate in the flat layout; lr: device scalar; grad_prescale multiplies the
 * gradient first (1/world after a sum all-reduce); sqnorm: device scratch of 256 floats. */
int hual_adamw_clip_step(float* params, const float* grads, float* adam_m, float* adam_v, const float* decay,
                         uint64_t n_padded, const float* lr, float clip_norm, float grad_prescale, float* sqnorm,
                         void* stream);

/* the same, and the Philox offset rng_state[2] of the training loop is advanced by one in the same launch (the step
 * counter of the dropout stream: one launch fewer per captured step than a separate increment) */
int hual_adamw_clip_step_rng(float* params, const float* grads, float* adam_m, float* adam_v, const float* decay,
                             uint64_t n_padded, const float* lr, float clip_norm, float grad_prescale, float* sqnorm,
                             uint32_t* rng_state, void* stream);

/* the same for an EPOCH LOOP whose position lives on the device (ABI 8; runner_utils.py:139-159): `cursor` = device i64[2] =
 * {ids consumed so far, words written to the span bank so far}.  The launch also copies `span_words` 8-byte words from `spans` (the step's
 * predicted start / end indices in the caller's fetch buffer) to bank + cursor[1], then cursor[0] += sel_inc, cursor[1] += bank_inc.
 * Together with hual_assemble_batch_cursor (which reads its batch's ids at ids + cursor[0]) a whole step - batch assembly, forward,
 * backward, optimizer, span banking - has the SAME arguments every time it runs with a given padded shape: one hipGraph per shape,
 * nothing launched between two graphs, nothing uploaded or fetched until the epoch ends. */
int hual_adamw_clip_step_loop(float* params, const float* grads, float* adam_m, float* adam_v, const float* decay,
                              uint64_t n_padded, const float* lr, float clip_norm, float grad_prescale, float* sqnorm,
                              uint32_t* rng_state, int64_t* cursor, const int64_t* spans, int64_t* bank, int span_words, int sel_inc,
                              int bank_inc, void* stream);

/* the same with AVERAGED WEIGHTS riding in the optimizer launch (an exponential moving average of the parameters, as the QANet family
 * of span predictors is evaluated on; HUAL_ABI_VERSION unchanged: a new symbol, nothing else moved).  rng_state, cursor, spans and bank
 * may be null as above (a null cursor: no loop position).  ema: flat shadow of `params` (same layout, n_padded floats, 16-byte aligned,
 * the word table of a fine-tuning model included), ema_count: device u32, the number of updates so far, zero at start.  Update k
 * (1-based) is
 *     ema <- ema + (1 - d_k) * (params_new - ema),   d_k = min(ema_decay, (1 + k) / (10 + k))  with ema_warmup,  d_k = ema_decay  without,
 * taken from the new parameter value while it is in registers (one 16-byte load and store more per four elements, no further launch).
 * k lives on the device because a step replayed from a hipGraph has frozen arguments: the call's FIRST launch (the gradient's square
 * norm) adds one to ema_count, its second launch (the update) only reads it - every block sees the same k, graph replays included.
 * ema and ema_count go together: one without the other is refused; both null is hual_adamw_clip_step_loop without its cursor
 * requirement.  ema_decay must lie in [0, 1). */
int hual_adamw_clip_step_ema(float* params, const float* grads, float* adam_m, float* adam_v, const float* decay,
                             uint64_t n_padded, const float* lr, float clip_norm, float grad_prescale, float* sqnorm,
                             uint32_t* rng_state, int64_t* cursor, const int64_t* spans, int64_t* bank, int span_words, int sel_inc,
                             int bank_inc, float* ema, uint32_t* ema_count, float ema_decay, int ema_warmup, void* stream);

/* ------------------------------------------------------------------------------------------
 * One-shot all-reduce of the flat gradient bucket over peer mappings (csrc/xgmi.hip; absent in the reference, which
 * pins one GPU: utils/runner_utils.py:11).  ONE launch per rank: flag barrier, reduce-scatter read straight from the peers' buckets
 * (rank order: identical bits on every rank), flag barrier, all-gather.  flat / scratch / flags: `world` device pointers each - entry
 * `rank` the rank's own memory, the others the peers' memory mapped into this process (hipIpcOpenMemHandle); scratch holds
 * ceil(n / world) floats rounded up to 4; flags are hual_xgmi_flags_bytes() of UNCACHED device memory (the setup helpers below own that
 * allocation - the one exception to "the library never allocates": the caller's allocator cannot provide it), zeroed once; seq: local
 * device u32, zero at start, advanced by the call itself (graph replays included); status: local device u32, 0 = ok, 1 = a peer did not
 * arrive within the spin limit (all waves left the kernel, the bucket is garbage).  Off by default (hual_amd/dist.py: HUAL_ALLREDUCE=custom). */
uint64_t hual_xgmi_flags_bytes(void);
int hual_xgmi_flags_alloc(void** p);
int hual_xgmi_flags_free(void* p);
int hual_xgmi_ipc_export(void* p, void* handle64, uint64_t* offset);      /* hipIpcGetMemHandle of p's allocation: 64 bytes + p's offset in it */
int hual_xgmi_ipc_open(const void* handle64, void** p);      /* hipIpcOpenMemHandle in ANOTHER process than the exporter's: the allocation's base */
int hual_xgmi_ipc_close(void* p);
int hual_xgmi_allreduce(int rank, int world, void* const* flat, void* const* scratch, void* const* flags, uint32_t* seq, uint32_t* status,
                        uint64_t n, uint64_t scratch_floats, void* stream);

/* cross-sample part of lossfun_aligment (layers.py:232-247) on [Bg,128] l2-normalised features
 * (all-gathered over ranks in exact data-parallel mode).  scratch: 2*Bg*Bg + Bg floats.
 * Writes d_that / d_vhat [Bg,128] (scaled by grad_scale) and WRITES the loss to *loss (device scalar: the row terms are summed
 * in row order by the second launch - no zeroing launch in front, no atomics). */
int hual_align_loss(const float* that, const float* vhat, int Bg, float* scratch, float* d_that, float* d_vhat,
                    float* loss, float grad_scale, void* stream);
/* the same for a rank of a data-parallel group: that / vhat are rows of stride `ld` floats (256 when the all-gather left
 * [that | vhat] side by side - the layout of the workspace buffer "align.tv" [B,256] the forward leaves), and only the gradient rows row0 .. row0 + nrows - 1 (the rank's own samples) are written,
 * to d_that / d_vhat [nrows,128] - straight into the workspace buffers "d.align.that" / "d.align.vhat" of the backward. */
int hual_align_loss_rows(const float* that, const float* vhat, int ld, int Bg, int row0, int nrows, float* scratch, float* d_that,
                         float* d_vhat, float* loss, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-block entry points: ONE block of the graph on caller-supplied activations, enqueued through the same launch
 * sequence the whole model uses (unit parity against the corresponding function of the reference).
 * Activations live in the unified row space: [B*T video rows, then B*L query rows] x 128 floats.  `batch` supplies the
 * shapes and the masks (video_seq_len, word_ids); `workspace` is the model workspace (hual_seqpan_query_workspace).  A *_bwd
 * call must follow the *_fwd call of the same block on the same workspace, batch and rng_state; it OVERWRITES `grads` (flat
 * parameter layout) with the gradients of the block's parameters (zero elsewhere).  Default kernel-fusion switches only.
 * ------------------------------------------------------------------------------------------ */
/* model.py:36-56: embeddings, query_conv1d / video_conv1d (the feature-load phase), q_/v_layer_norm, position embeddings
 * -> x0 [B*(T+L),128] */
int hual_video_proj_ln_fwd(const hual_cfg* cfg, const float* params, const float* word_table, const hual_batch* batch,
                           const hual_run_opts* opts, float* x0, void* workspace, uint64_t ws_bytes, void* stream);
/* its backward (HUAL_ABI_VERSION unchanged: a new symbol, nothing else moved): d_x0 [B*(T+L),128] = the gradient wrt x0.  Nothing is
 * returned but `grads`: the position table, the two input layer norms, video_conv1d / query_conv1d, the char CNN's filters and biases,
 * the char table, the unk row and - cfg->finetune_word_emb - the word table.  word_table as in the forward call */
int hual_input_bwd(const hual_cfg* cfg, const float* params, const float* word_table, const hual_batch* batch,
                   const hual_run_opts* opts, const float* d_x0, float* grads, void* workspace, uint64_t ws_bytes, void* stream);
/* modules.py:59-70 conv_block (shared weights, video and query rows in one pass): y = conv_block(x) */
int hual_conv_block_fwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, const float* x,
                        float* y, void* workspace, uint64_t ws_bytes, void* stream);
int hual_conv_block_bwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, const float* dy,
                        float* dx, float* grads, void* workspace, uint64_t ws_bytes, void* stream);
/* modules.py:73-89 + layers.py:59-111 dual_attn_block `layer` in both directions (v <- (v,q) and q <- (q,v), shared weights,
 * both from the OLD features, model.py:60-68): y = [dual_attn_block(v, q), dual_attn_block(q, v)] */
int hual_dual_attn_fwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, int layer,
                       const float* x, float* y, void* workspace, uint64_t ws_bytes, void* stream);
int hual_dual_attn_bwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, int layer,
                       const float* dy, float* dx, float* grads, void* workspace, uint64_t ws_bytes, void* stream);
/* layers.py:114-130 cq_attention in both directions (model.py:70-73): feats = [q2v_attn(v, q) on the video rows,
 * v2q_attn(q, v) on the query rows] */
int hual_cq_attn_fwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, const float* x,
                     float* feats, void* workspace, uint64_t ws_bytes, void* stream);
int hual_cq_attn_bwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, const float* dfeats,
                     float* dx, float* grads, void* workspace, uint64_t ws_bytes, void* stream);
/* the fuse stage and the close of the loss (HUAL_ABI_VERSION unchanged: new symbols, nothing else moved): layers.py:145-154 cq_concat,
 * model.py:82-97 matching head + label embeddings, model.py:76 / layers.py:205-248 alignment loss, on feats [B*(T+L),128] = what
 * hual_cq_attn_fwd returns -> outputs [B*T,128] (masked, the predictor's input) and match_scores [B*T,4].
 *  - labels NULL: the inference form (no alignment pooling, no loss; loc_part and loss_terms are not read / written).
 *  - labels given (match_labels and inner_labels are read; y1 / y2 are not): loc_part [B] (device) = the per-clip terms of the localizing
 *    loss as the heads launch leaves them (hual_localizing_loss); loss_terms float[4] (device) = {total, loc, match, align} as the whole
 *    model reports them, closed by the same launch - unless opts->deferred_loss_terms is set: then the forward leaves the loss open and
 *    the backward call's matching-head launch closes it into opts->deferred_loss_terms (pass the same options to both calls).
 *  - opts->align_external: no similarity rows in the forward; the caller writes the workspace buffers d.align.that / d.align.vhat [B,128]
 *    (hual_seqpan_ws_table) between the two calls, as an exact data-parallel step does through hual_align_loss_rows.
 * The backward takes the two parts of d outputs (what the encoders and what the heads' hidden layers send back: summed on the way in)
 * and returns d_feats [B*(T+L),128] and, in `grads`, the gradients of cq_cat, matching_loss/dense and label_emb (orthogonality term
 * included).  It must follow hual_fuse_fwd with the same labels on the same workspace; without labels it is refused (HUAL_ERR_INVALID). */
int hual_fuse_fwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, const hual_labels* labels,
                  const float* feats, const float* loc_part, float* outputs, float* match_scores, float* loss_terms, void* workspace,
                  uint64_t ws_bytes, void* stream);
int hual_fuse_bwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, const hual_labels* labels,
                  const float* d_outputs, const float* d_outputs_heads, float* d_feats, float* grads, void* workspace, uint64_t ws_bytes,
                  void* stream);
/* modules.py:143-160 conditioned_predictor on `outputs` [B*T,128] -> raw start / end logits [B,T] and the span argmax of
 * layers.py:194-203; the backward takes the gradients of the two logit tensors */
int hual_predictor_fwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, const float* outputs,
                       float* start_logits, float* end_logits, int64_t* start_index, int64_t* end_index, void* workspace,
                       uint64_t ws_bytes, void* stream);
int hual_predictor_bwd(const hual_cfg* cfg, const float* params, const hual_batch* batch, const hual_run_opts* opts, const float* d_start,
                       const float* d_end, float* d_outputs, float* grads, void* workspace, uint64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-kernel entry points (unit parity tests call these through ctypes).
 * ------------------------------------------------------------------------------------------ */

/* conv1d(kernel_size=1) == dense  (models/layers.py:20-29) on the 16-bit matrix cores with split operands (x = hi + lo, three
 * MFMA passes, fp32 accumulate; ~1e-6 relative to the fp32 product) - the kernel the model path uses for the dense layers outside
 * its fused kernels:
 *   trans_w = 0: Y[M,128] = act(A[M,K] . W[K,128] + bias), K % 8 == 0, act: 0 none, 1 relu; scratch >= ceil(K/128) * 65536 bytes
 *   trans_w = 1: Y[M,N]   = A[M,128] . W^T with W stored [N,128] (dX of a dense layer), N % 8 == 0;
 *                scratch >= ceil(N/128) * 65536 bytes
 * scratch (device) receives the pre-split weight image. */
int hual_linear_bf16x3(const float* A, int lda, const float* W, int trans_w, const float* bias, float* Y, int ldy, int M,
                       int K, int N, int act, void* scratch, uint64_t scratch_bytes, void* stream);

/* gradients of the dense above: dW[K,N] += A^T . dY ; db[N] += colsum(dY) (db may be NULL), through the persistent
 * weight-gradient launch of the training step: the 64-row tiles of the job dealt evenly to `workgroups` workgroups
 * (0 = one per CU), the job table living in `scratch` (device, >= 512 bytes).  N must be 128 (every dense layer of the
 * graph has 128 outputs).  Accumulates with float atomics: zero the destinations first.
 * Arithmetic (ABI 7): fp16-pair operands - A and dY each by a running power-of-two scale taken from the data (any magnitude: the
 * operands of a weight gradient are not bounded by construction - products of activations, unnormalised block outputs);
 * 2-5e-7 of the largest entry against a float64 product. */
int hual_linear_dw(const float* A, int lda, const float* dY, int ldy, float* dW, int ldw, float* db, int M, int K,
                   int N, int workgroups, void* scratch, uint64_t scratch_bytes, void* stream);

/* layer_norm (models/layers.py:7-17): y = (x - mean) * rsqrt(var + 1e-6) * gamma + beta over the 128 columns of each row;
 * mean / rstd (optional, [R]) are what the backward needs. */
int hual_layer_norm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int R,
                        void* stream);

/* multi-head attention core of dual_multihead_attention / top_self_attention (models/layers.py:80-96, modules.py:104-119):
 * 8 heads of size 16 kept merged in [rows,128]; scores / sqrt(16) + (1 - qmask x kmask) * (-1e30), softmax, P.V.
 * Q rows b*Tq + t, K/V rows b*Tk + t; masks are [B*Tq] / [B*Tk] floats (0/1).  Tq <= 256 and Tk <= 256
 * (longer queries: HUAL_ERR_INVALID - a launch's unit codes hold 16 query tiles per job).
 * Arithmetic (ABI 7): fp16-pair operands, Q / K / V scaled by 2^4 (|x| >= 4094 does not fit: Inf / NaN outputs, loudly); outputs within
 * 1e-6 of a float64 evaluation on O(1) inputs - the level of a float32 evaluation. */
int hual_attention_fwd(const float* Q, int ldq, const float* K, const float* V, int ldkv, float* O, int ldo, int B, int Tq,
                       int Tk, const float* qmask, const float* kmask, void* stream);

/* The same with what a backward pass needs: stats [2][B*Tq*8] (row max of the scaled scores in the log2 domain, 1 / row sum,
 * per query and head) and - when drop_rate > 0 - the dropout of layers.py:86,91 / modules.py:114 on the probabilities with
 * the build's Philox stream (rng_state = device u32[3] {seed lo, seed hi, offset}, call site `drop_site`, RNG row =
 * query row * 8 + head; 16-bit decisions with the exact 1 / (1 - rate) scale, see DESIGN.md "Dropout") and its keep words: an opaque
 * buffer of B*Tq*8 rows of `ldm` bytes, ldm >= hual_attention_keep_row_bytes(Tk), 8-byte aligned (layout: csrc/attn.h). */
int hual_attention_fwd_save(const float* Q, int ldq, const float* K, const float* V, int ldkv, float* O, int ldo, int B, int Tq,
                            int Tk, const float* qmask, const float* kmask, float* stats, uint8_t* keep_bytes, int ldm,
                            const uint32_t* rng_state, float drop_rate, int drop_site, void* stream);
int hual_attention_keep_row_bytes(int Tk);

/* gradient of the attention core (tf.gradients through layers.py:80-96): dQ, dK, dV [rows,128] (written, not accumulated)
 * from dO, the forward output O, `stats` and `keep_bytes` of hual_attention_fwd_save with the same arguments.  Tq, Tk <= 256. */
int hual_attention_bwd(const float* Q, int ldq, const float* K, const float* V, int ldkv, const float* O, int ldo,
                       const float* stats, const uint8_t* keep_bytes, int ldm, const float* dO, int lddo, float* dQ, int lddq,
                       float* dK, float* dV, int lddkv, int B, int Tq, int Tk, const float* qmask, const float* kmask,
                       const uint32_t* rng_state, float drop_rate, int drop_site, void* stream);

/* ans_predictor (models/layers.py:194-203): softmax of the masked logits, upper-triangular outer product, start = argmax
 * over rows of the row maxima, end = argmax over columns of the column maxima, first index on ties.  T <= 256. */
int hual_span_argmax(const float* start_logits, const float* end_logits, const float* vmask, int64_t* start_index,
                     int64_t* end_index, int B, int T, void* stream);
/* the same launch with labels (HUAL_ABI_VERSION unchanged: a new symbol): localizing_loss (layers.py:177-191) on given logits [B,T] and
 * soft labels y1 / y2 [B,T] (rows need not sum to 1) -> loc_part [B] = clip b's -(y1 . log_softmax(s) + y2 . log_softmax(e)) / B (their
 * sum is the loss), ds / de [B,T] = the gradient of that loss wrt the two logit tensors, and the spans of hual_span_argmax.  T <= 256. */
int hual_localizing_loss(const float* start_logits, const float* end_logits, const float* vmask, const float* y1, const float* y2,
                         float* ds, float* de, float* loc_part, int64_t* start_index, int64_t* end_index, int B, int T, void* stream);

/* the k best spans of each clip (R@k evaluation, ABI 9): softmax of the masked start / end logits exactly as hual_span_argmax computes
 * it, candidates p_s[i] * p_e[j] (one fp32 product) for 0 <= i <= j < video_seq_len[b] (and j - i < max_len when max_len > 0), greedy
 * temporal NMS.  1 <= k <= 16, 1 <= T <= 256, 0 < nms_iou <= 1 (1 = plain top-k of distinct spans), max_len >= 0.
 *  - order: higher score first; equal scores by the smaller key i * 256 + j (smaller i, then smaller j).
 *  - NMS on the half-open frame intervals [i, j + 1): inter = max(0, min(j1, j2) + 1 - max(i1, i2)), union = len1 + len2 - inter; a
 *    candidate is suppressed iff (float)inter >= nms_iou * (float)union (fp32) for any span already selected.
 *  - outputs [B, k] row major: start_index, end_index (int64), score (float).  Slots beyond the surviving candidates: -1, -1, -1.0f.
 *    A NaN logit at t < video_seq_len[b] gives the whole row -1 (the poison rule of hual_span_argmax).  video_seq_len[b] > T reads as
 *    T, < 1 as an empty clip (all -1).  Logits at t >= video_seq_len[b] are not read.
 *  - slot 0 equals hual_span_argmax whenever the maximal pairs form a product set (equal-probability plateaus included): both then pick
 *    the smallest start and the smallest end.  They can differ only when two DIFFERENT products round to the same maximal float and
 *    the smallest start and smallest end among those pairs are not a pair of them: ans_predictor then reports that mixed pair, which
 *    need not even be a maximal span, and this function the maximal pair with the smallest (i, j).
 * Allocates nothing and does not synchronise: capturable in a hipGraph.  Argument errors return before any HIP call. */
int hual_span_topk(const float* start_logits, const float* end_logits, const int32_t* video_seq_len, int B, int T, int k, int max_len,
                   float nms_iou, int64_t* start_index, int64_t* end_index, float* score, void* stream);

/* expected temporal IoU of k proposed spans per clip under the clip's own span distribution, that distribution's entropy, and the
 * minimum-Bayes-risk order of the proposals (ABI 9 unchanged, a new symbol).  With v = video_seq_len[b] read as hual_span_topk reads it
 * (> T as T, < 1 as empty), p_s / p_e are the masked softmaxes bit for bit as hual_span_topk and hual_span_argmax compute them; the
 * weights are w(i,j) = p_s[i] * p_e[j] (one fp32 product) for 0 <= i <= j < v, Z their sum, P = w / Z.  1 <= k <= 16, 1 <= T <= 256.
 *  - expected_iou [B, k] (float): for the candidate (a, b) = (start_index, end_index)[b][slot] the sum over the triangle of
 *    P(i,j) * iou on the half-open frame intervals of hual_span_topk's NMS: inter = max(0, min(b,j) + 1 - max(a,i)), union =
 *    (b - a + 1) + (j - i + 1) - inter - the time IoU of the spans in seconds, the evaluation's metric.  Arithmetic: each term is
 *    w * ((float)inter / (float)union), the division and the product rounded to fp32; the terms and Z are accumulated in float64 in a
 *    fixed order; the result is (float)(sum / Z), in [0, 1].
 *  - span_entropy [B] (float; may be NULL): H = log2(Z) - (1/Z) * sum w * (log2f(p_s[i]) + log2f(p_e[j])) in bits, the sum of the two
 *    logarithms in fp32, product and accumulation in float64, terms with w == 0 skipped, clamped at >= 0, <= log2(v (v + 1) / 2).
 *    v == 1: H = 0 and every valid candidate has expected IoU exactly 1.0f.
 *  - a slot is invalid when an index is negative, a > b or b >= v: its expected_iou is -1.0f (not an error).
 *  - an empty clip (v < 1), a NaN logit at t < v (the poison rule of hual_span_topk) or a Z that is not a positive finite number
 *    (every weight of the triangle underflowed, or an infinite logit): every expected_iou of the row is -1.0f, span_entropy is -1.0f
 *    and the row is never reordered.  Logits at t >= v are not read.
 *  - reorder != 0: the row's slots are sorted by expected_iou descending, stable (equal values and the invalid slots, last, keep their
 *    incoming order); start_index, end_index, score (when not NULL) and expected_iou are permuted alike, in place.  reorder == 0:
 *    start_index / end_index / score are only read.
 * Allocates nothing and does not synchronise: capturable in a hipGraph.  Argument errors (a null pointer other than score and
 * span_entropy, the ranges above, B < 1) return before any HIP call. */
int hual_span_expected_iou(const float* start_logits, const float* end_logits, const int32_t* video_seq_len, int B, int T, int k,
                           int64_t* start_index, int64_t* end_index, float* score, float* expected_iou, float* span_entropy,
                           int reorder, void* stream);

/* hit probability of spans under the clip's own span distribution: the chance that a span counts as a hit at IoU >= m, the confidence in
 * the metric that selects a checkpoint (R@1 at IoU 0.3 / 0.5 / 0.7), for k proposals per clip and - per threshold - for the span of the
 * whole triangle that maximises it, the Bayes decision for R@1 at that threshold (ABI 9 unchanged, a new symbol).  v, p_s, p_e as
 * hual_span_expected_iou (bit for bit those of hual_span_topk); the weights are w(i,j) = (double)p_s[i] * (double)p_e[j] for 0 <= i <= j
 * < v as hual_al_query takes them, Z their sum.  1 <= T <= 256, 0 <= k <= 16, 1 <= M <= 4.
 *  - thresholds: HOST int32 [M][2] = (num, den), exact rationals with 1 <= num <= den <= 1024, read before the launch and passed to the
 *    kernel by value.  A span (i,j) hits the candidate (a,b) iff den * inter >= num * union in integers, inter = max(0, min(b,j) + 1 -
 *    max(a,i)), union = (b - a + 1) + (j - i + 1) - inter on the half-open frame intervals of hual_span_topk's NMS: no float takes part
 *    in the hit test.  (al.iou_metrics compares a float32 ratio of float32 times with the threshold; it can differ from this rule only
 *    where the IoU equals the threshold exactly.)
 *  - hit_prob [B, k, M] (float; k >= 1): for the candidate (a, b) = (start_index, end_index)[b][slot] the sum of w over the spans that hit
 *    it, divided by Z, clamped to [0, 1].  Arithmetic: float64 throughout; the sum over the hitting ends of one start is taken as a
 *    DIFFERENCE of float64 prefix sums of p_e (an absolute error of a few 2^-53, far below the float32 result), the sums over starts and
 *    Z in a fixed order.  Columns do not increase with the threshold up to that rounding.  A slot is invalid when an index is negative,
 *    a > b or b >= v: -1.0f in all M columns (not an error).  k == 0 skips the proposals; start_index, end_index, score and hit_prob may
 *    then be NULL.
 *  - reorder_by = m in [0, M): the row's slots are sorted by column m of hit_prob descending, stable (equal values and the invalid slots,
 *    last, keep their incoming order); start_index, end_index, score (when not NULL) and all M columns of hit_prob are permuted alike, in
 *    place - hual_span_expected_iou's reorder.  reorder_by = -1: start_index / end_index / score are only read.
 *  - best_start, best_end (int64), best_prob (float), [B, M] each, all three or none: for threshold m the span of the triangle with the
 *    largest hit mass in the arithmetic above, among equal masses the first in row-major order (smallest a, then smallest b), and its
 *    hit probability.
 *  - an empty clip (v < 1), a NaN logit at t < v or a Z that is not a positive finite number (hual_span_expected_iou's rule): every
 *    hit_prob of the row is -1.0f, best_* are -1, -1, -1.0f and the row is never reordered.  v == 1: every valid candidate and every
 *    Bayes span is (0, 0) with probability exactly 1.0f.  Logits at t >= v are not read.
 * Allocates nothing and does not synchronise: capturable in a hipGraph.  Argument errors (a null pointer other than score, the best_*
 * and - with k == 0 - the proposal arrays; B < 1; T, k, M or a threshold out of range; only some of best_*; reorder_by outside [-1, M) or
 * set with k == 0; k == 0 without best_*) return HUAL_ERR_INVALID before any HIP call. */
int hual_span_hit_prob(const float* start_logits, const float* end_logits, const int32_t* video_seq_len, int B, int T,
                       const int32_t* thresholds, int M, int k, int64_t* start_index, int64_t* end_index, float* score, float* hit_prob,
                       int reorder_by, int64_t* best_start, int64_t* best_end, float* best_prob, void* stream);

/* coverage of span sets under the clip's own span distribution: the chance that AT LEAST ONE span of a set hits the truth at IoU >= m -
 * what R@k counts - for the cumulative sets of k proposals, and per threshold the greedy set of K spans of the whole triangle that covers
 * the most, the sequel of hual_span_hit_prob's Bayes span for R@k (ABI 9 unchanged, a new symbol).  v, p_s, p_e, w(i,j), Z, the
 * thresholds (HOST (num, den) pairs, by value), the integer hit rule and the float64 arithmetic over prefix differences are exactly
 * hual_span_hit_prob's.  The coverage of a set S is C(S) = (1/Z) * the sum of w(i,j) over the truths (i,j) that some span of S hits: monotone
 * and submodular in S, so the greedy set is within 1 - (1 - 1/K)^K of the best set of K spans.
 * 1 <= T <= 256, 1 <= M <= 4, 0 <= k <= 16, 0 <= K <= 16, k + K >= 1, 0 <= min_gain < 1.
 *  - set_prob [B, k, M] (float; k >= 1): set_prob[b][q][m] is the coverage at threshold m of the valid slots among slots 0..q of
 *    (start_index, end_index)[b]; for the proposals of hual_span_topk the chance that the clip counts for R@(q+1).  An invalid slot (an
 *    index negative, a > b or b >= v) adds nothing; the value is 0.0f while no valid slot has been seen; column 0 of a valid slot is its
 *    hit_prob (up to the order of one sum).  Each slot adds the mass of the truths it hits that no earlier slot hits, summed over the
 *    starts in a fixed order; the value is (float)(covered / Z) clamped to [0, 1].  start_index / end_index are only read.  k == 0 skips
 *    the proposals; start_index, end_index and set_prob may then be NULL.
 *  - cover_start, cover_end (int64), cover_prob (float), [B, M, K] each, all three (K >= 1) or none (K == 0): per threshold m, with nothing
 *    covered at the start, step s takes the span of the whole triangle with the largest GAIN - the mass of the truths it hits that no
 *    earlier pick hits - among equal gains the first in row-major order (smallest a, then smallest b); cover_prob[b][m][s] is the
 *    cumulative coverage after it, (float)(covered / Z) clamped to [0, 1].  The set stops at the first step whose best gain divided by Z
 *    is <= min_gain: that and every later slot is -1, -1 with the last cumulative coverage repeated (0.0f if step 0 stopped).  Step 0 is
 *    hual_span_hit_prob's search itself: with min_gain == 0, cover_*[b][m][0] equal its best_*[b][m] bit for bit.  A launch with a larger
 *    K extends one with a smaller K: the first columns are equal.  A start's uncovered mass is a difference of prefix differences, clamped
 *    at >= 0: a span whose truths are all covered has a gain of a few 2^-53 at most, so min_gain == 0 may go on with such spans.
 *  - an empty clip (v < 1), a NaN logit at t < v or a Z that is not a positive finite number: every set_prob of the row is -1.0f and
 *    cover_* are -1, -1, -1.0f.  v == 1: the set is (0, 0) with probability exactly 1.0f, then stopped slots.  Logits at t >= v are not
 *    read.
 * Float64 throughout, sums in a fixed order, no atomics: a second launch returns equal bits.  Allocates nothing and does not synchronise:
 * capturable in a hipGraph.  Argument errors (a null pointer among the logits, lengths, thresholds or the arrays of a part that is asked
 * for; B < 1; T, k, K, M, min_gain or a threshold out of range; k == 0 and K == 0; only some of cover_*) return HUAL_ERR_INVALID before
 * any HIP call. */
int hual_span_hit_cover(const float* start_logits, const float* end_logits, const int32_t* video_seq_len, int B, int T,
                        const int32_t* thresholds, int M, int k, const int64_t* start_index, const int64_t* end_index, float* set_prob,
                        int K, float min_gain, int64_t* cover_start, int64_t* cover_end, float* cover_prob, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-side batch assembly: TrainLoader.process_batch / TestLoader.process_batch
 * (/root/reference/utils/data_loader.py:30-98,145-164) from a training set that stays resident in HBM.
 * All arrays are device memory owned by the caller.  Videos: rows feat_off[v] .. feat_off[v+1] of feat_bank
 * [total_frames, vdim] (already down-sampled to <= max_vlen by visual_feature_sampling, data_utils.py:70-85).
 * Samples: video id, word ids word_bank[word_off[s] .. word_off[s+1]), chars of word w (global word index)
 * char_bank[char_off[w] .. char_off[w+1]), pseudo-label frame indices s_ind / e_ind (NULL for test sets).
 * ------------------------------------------------------------------------------------------ */
typedef struct hual_dataset {
  const float* feat_bank;
  const int64_t* feat_off;     /* [n_videos + 1] */
  int32_t vdim;
  const int32_t* sample_vid;   /* [n_samples] */
  const int32_t* word_off;     /* [n_samples + 1] */
  const int32_t* word_bank;
  const int32_t* char_off;     /* [n_words_total + 1] */
  const int32_t* char_bank;
  const int32_t* s_ind;        /* [n_samples] */
  const int32_t* e_ind;        /* [n_samples] */
} hual_dataset;

/* sel: i32 [B] sample ids of the batch.  T / L / C must be the maxima of the batch's video / word / char lengths
 * (the caller knows the lengths; C >= 4 for the model).  Writes the feeds of model.py:16-27: video f32 [B,T,vdim] zero
 * padded, video_seq_len i32 [B], word_ids i32 [B,L], char_ids i32 [B,L,C] and - unless y1 is NULL - the soft start/end
 * labels f32 [B,T], match_labels i32 [B,T], inner_labels f32 [B,T] exactly as data_loader.py:55-94 computes them. */
int hual_assemble_batch(const hual_dataset* ds, const int32_t* sel, int B, int T, int L, int C, float* video,
                        int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                        int32_t* match_labels, float* inner_labels, void* stream);
/* The same launch with a CARRY: one of its workgroups also copies carry_n 8-byte words from carry_src to carry_dst (carry_n = 0: none).
 * For epoch loops that bank what the PREVIOUS step left in its fetch buffers (the predicted spans, runner_utils.py:150-156) without an
 * operation of their own between two replayed step graphs: every eager operation there costs ~13 us of idle device. */
int hual_assemble_batch_carry(const hual_dataset* ds, const int32_t* sel, int B, int T, int L, int C, float* video,
                              int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                              int32_t* match_labels, float* inner_labels, const int64_t* carry_src, int64_t* carry_dst, int carry_n,
                              void* stream);

/* The same launch for an epoch loop with a device-side position: the batch's ids are ids[cursor[0] .. cursor[0] + B) (cursor: device
 * i64[2], advanced by hual_adamw_clip_step_loop at the end of the step). */
int hual_assemble_batch_cursor(const hual_dataset* ds, const int32_t* ids, const int64_t* cursor, int B, int T, int L, int C, float* video,
                               int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                               int32_t* match_labels, float* inner_labels, void* stream);

/* Soft-label banks beside the dataset (HUAL_ABI_VERSION unchanged: new symbols, nothing else moved; hual_dataset and the three entry
 * points above are what they were).  y1 / y2: device f32 [n_samples, ld] row major, a distribution over the frames of every sample's
 * clip to train the start / end head on instead of the reference's three-frame kernel around s_ind / e_ind (the rows
 * hual_al_span_marginals writes, say); w: device f32 [n_samples], 0 <= w <= 1, how far sample s moves towards its rows; ld >= the
 * longest clip of the set. */
typedef struct hual_soft_labels {
  const float* y1;
  const float* y2;
  const float* w;
  int32_t ld;
} hual_soft_labels;

/* hual_assemble_batch_carry / hual_assemble_batch_cursor - the same launch, arguments and checks, every other feed bit-identical - with
 * the labels blended towards the banks.  With r the value the plain entry points write at frame t of sample s (clip of n frames) and
 * lam = w[s]:
 *  - lam == 0, or t >= n (or t >= ld): r, untouched; bank[s][t] is not read, so a NaN in the row of an unweighted sample cannot leak.
 *  - else: r + lam * (bank[s][t] - r) as three float32 operations each rounded on its own, __fadd_rn(r, __fmul_rn(lam, __fsub_rn(bank, r))):
 *    no contraction, so a float32 restatement on the host reproduces it bit for bit.  lam == 1 gives the bank's value up to rounding.
 * match_labels and inner_labels stay those of the hard label s_ind / e_ind.  The weights are not validated on the device.
 * Argument errors (those of the plain entry points; a null soft, a null array of it, ld < 1, or soft labels without the label feeds)
 * return HUAL_ERR_INVALID before any HIP call: a null bank never turns the call into a plain assembly. */
int hual_assemble_batch_soft(const hual_dataset* ds, const int32_t* sel, int B, int T, int L, int C, float* video,
                             int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                             int32_t* match_labels, float* inner_labels, const int64_t* carry_src, int64_t* carry_dst, int carry_n,
                             const hual_soft_labels* soft, void* stream);
int hual_assemble_batch_cursor_soft(const hual_dataset* ds, const int32_t* ids, const int64_t* cursor, int B, int T, int L, int C,
                                    float* video, int32_t* video_seq_len, int32_t* word_ids, int32_t* char_ids, float* y1, float* y2,
                                    int32_t* match_labels, float* inner_labels, const hual_soft_labels* soft, void* stream);

/* ------------------------------------------------------------------------------------------
 * Active-learning label update (BASELINE.json configs[4]): what /root/reference/update_label.py does
 * per training sample between two training rounds, for the whole training set in two launches.
 *   hual_al_score  = the loop body of get_uncert_rank (update_label.py:125-169): sigmoid of the deterministic logits,
 *                    get_uncert_model (utils/utils_hual.py:144-161) of the two stochastic passes, get_distance_score
 *                    (:92-103) of the sample's active points, uncert_frame, uncert_video and the frame to annotate
 *                    (argmax of uncert_frame, update_label.py:194)
 *   hual_al_renew  = renew_label (update_label.py:85-123) for the selected samples, after the caller appended the
 *                    annotated frame to their active points (append_AP, utils_hual.py:133-139)
 * The ranking by uncert_video, the ground-truth lookup and the JSON/pickle files stay on the host (hual_amd/al.py).
 * A sample's logits occupy the first tlen[n] entries of its row (tlen = padded length of the batch the record came
 * from, `max_vlen = len(sprob)` in the reference); 2 <= tlen <= ld <= 1024, 1 <= vlen <= tlen.
 * ------------------------------------------------------------------------------------------ */
typedef struct hual_al_set {
  int32_t N, ld;
  const int32_t* vlen;     /* [N]   record['v_len'] */
  const int32_t* tlen;     /* [N]   len(prop_logits[0]) */
  const int32_t* ap_off;   /* [N+1] CSR offsets into ap_idx / ap_pos */
  const int32_t* ap_idx;   /* active points: frame index, in annotation order */
  const int8_t* ap_pos;    /* 1 = 'pos_idx' entry, 0 = 'neg_idx' entry */
} hual_al_set;

/* s0/e0: prop_logits, s1/e1: prop_logits1, s2/e2: prop_logits2, each f32 [N, ld].  Outputs: sprob, eprob f32 [N, ld];
 * uncert_frame f64 [N, ld]; uncert_video f32 [N]; observe_point i32 [N]. */
int hual_al_score(const hual_al_set* set, const float* s0, const float* e0, const float* s1, const float* e1,
                  const float* s2, const float* e2, float coff_uncert, float* sprob, float* eprob, double* uncert_frame,
                  float* uncert_video, int32_t* observe_point, void* stream);

/* sel: i32 [nsel] sample ids (NULL = all N); old_idx i32 [N,2]; coff6 (HOST pointer) = pos.{distance,model,old},
 * neg.{distance,model,old} of F_renew (update_label.py:11-37); new_idx i32 [N,2], written for the selected rows only. */
int hual_al_renew(const hual_al_set* set, const int32_t* sel, int nsel, const float* sprob, const float* eprob,
                  const int32_t* old_idx, const double* coff6, int32_t* new_idx, void* stream);

/* ------------------------------------------------------------------------------------------
 * K-pass MC-dropout uncertainty, folded on the device (HUAL_ABI_VERSION unchanged: new symbols, nothing else moved).
 * Replaces, for K >= 2 stochastic passes, the two fixed slots prop_logits1 / prop_logits2 of the results records
 * (utils/runner_utils.py:90-100) and the two-sample spread of get_uncert_model (utils/utils_hual.py:144-161): instead of
 * keeping every pass's logits, each pass is folded into per-frame statistics of the probabilities p = 1/(1+expf(-logit)) (float32;
 * p = 0 at t >= v_len, as get_uncert_model zeroes them).  The bank belongs to the caller, lives in device memory and covers
 * the whole training set: row n = sample n, each array [N, ld] row major, 2 <= ld <= 1024.
 * ------------------------------------------------------------------------------------------ */
typedef struct hual_al_bank {
  int32_t N, ld;
  int32_t* tlen;                       /* [N] length of the sample's logits (padded length of its batch), written by the k = 0 fold */
  float *s0, *e0;                      /* deterministic start / end logits (prop_logits) */
  float *lo_s, *hi_s, *mean_s, *m2_s;  /* start head: min, max, running mean, sum of squared deviations (Welford) of p */
  float *lo_e, *hi_e, *mean_e, *m2_e;  /* end head */
} hual_al_bank;

/* One launch folds one forward's start_logits / end_logits f32 [B, T_b] into the rows ids[b] (device i32 [B]: any rows in any order,
 * each at most once - the rows of a launch must be disjoint; an id outside [0, N) writes nothing).  v_len: device i32 [B].
 *   k = 0 (the deterministic pass): s0 / e0 <- the raw logits, tlen[ids[b]] <- T_b
 *   k = 1: lo = hi = mean = p, m2 = 0
 *   k >= 2: lo = fminf(lo, p), hi = fmaxf(hi, p), d = p - mean, mean += d / k, m2 += d * (p - mean), every operation rounded on its own
 * Writes columns [0, T_b) of the listed rows only; 2 <= T_b <= ld.  Allocates nothing, does not synchronise. */
int hual_al_mc_fold(const hual_al_bank* bank, const int32_t* ids, const int32_t* v_len, const float* start_logits,
                    const float* end_logits, int B, int T_b, int k, void* stream);

#define HUAL_AL_STAT_RANGE 0   /* (hi_s - lo_s) + (hi_e - lo_e): at K = 2 get_uncert_model's value bit for bit; grows with K */
#define HUAL_AL_STAT_STD 1     /* sqrtf(2) * (sqrtf(m2_s / (K-1)) + sqrtf(m2_e / (K-1))): |p1 - p2| sums at K = 2 up to rounding; its
                                  expectation does not grow with K, so coff_uncert keeps its meaning */
/* hual_al_score with the model-uncertainty term read from a bank of K >= 2 folded passes instead of from s1 .. e2 (the fold has
 * zeroed p at t >= v_len); s0 / e0 may be the bank's own.  Everything else - distance score, float64 mixture, uncert_video, the first
 * maximal frame - is hual_al_score's, in the same arithmetic types.  uncert_model (may be NULL): f32 [N, ld], the term itself, columns
 * [0, tlen[n]) of every row. */
int hual_al_score_mc(const hual_al_set* set, const float* s0, const float* e0, const hual_al_bank* bank, int K, int stat,
                     float coff_uncert, float* sprob, float* eprob, double* uncert_frame, float* uncert_video,
                     int32_t* observe_point, float* uncert_model, void* stream);

/* ------------------------------------------------------------------------------------------
 * Information-theoretic acquisition from the same K passes (HUAL_ABI_VERSION unchanged: new symbols, nothing else moved; hual_al_mc_fold
 * and hual_al_score_mc are what they were).  RANGE and STD measure the spread of p; neither separates "the passes disagree" from "every
 * pass is unsure", and RANGE grows with K.  With the binary entropy in bits
 *   h2(p) = 0.0f if p <= 0.0f or p >= 1.0f, else -(p * log2f(p) + q * log2f(q)), q = 1.0f - p
 * (float32, every operation rounded on its own) the fold also keeps, per head, the running mean `ent` of h2(p_k) over the stochastic
 * passes - p_k the very value the fold computes, 0 at t >= v_len, so a masked frame contributes exactly 0.  Per head each statistic
 * below lies in [0, 1] at every K, their sum over the two heads in [0, 2]: the interval RANGE lives in.
 * The arrays belong to the caller and sit beside its hual_al_bank: each f32 [N, ld] row major, device memory.
 * ------------------------------------------------------------------------------------------ */
typedef struct hual_al_info {
  float *ent_s, *ent_e;                /* start / end head: mean over the stochastic passes of h2(p_k) */
} hual_al_info;

/* hual_al_mc_fold - one launch, the same arguments and checks, every hual_al_bank array bit-identical to it - that also folds ent:
 *   k = 0: untouched;  k = 1: ent = h2(p);  k >= 2: ent += (h2(p) - ent) / k
 * Writes columns [0, T_b) of the listed rows only.  Allocates nothing, does not synchronise. */
int hual_al_mc_fold_info(const hual_al_bank* bank, const hual_al_info* info, const int32_t* ids, const int32_t* v_len,
                         const float* start_logits, const float* end_logits, int B, int T_b, int k, void* stream);

/* the sum over the start and end heads of (mean = the bank's Welford mean of p): */
#define HUAL_AL_STAT_BALD 2              /* fmaxf(0.0f, h2(mean) - ent): the mutual information between the prediction and the dropout
                                            mask - disagreement between the passes (epistemic).  >= 0 by Jensen in exact arithmetic; the
                                            clamp only removes negative rounding residue.  K identical passes give exactly 0 */
#define HUAL_AL_STAT_ENTROPY 3           /* h2(mean): total predictive uncertainty = BALD + EXPECTED_ENTROPY */
#define HUAL_AL_STAT_EXPECTED_ENTROPY 4  /* ent: what every single pass is unsure about (aleatoric) */
/* hual_al_score_mc with the model-uncertainty term one of the three statistics above (no other value of stat is accepted; K >= 2 for
 * BALD, K >= 1 for the two entropies; bank and set agree in N and ld).  Everything else - distance score, float64 mixture,
 * uncert_video, the first maximal frame, uncert_model (may be NULL) - is hual_al_score_mc's. */
int hual_al_score_info(const hual_al_set* set, const float* s0, const float* e0, const hual_al_bank* bank, const hual_al_info* info,
                       int K, int stat, float coff_uncert, float* sprob, float* eprob, double* uncert_frame, float* uncert_video,
                       int32_t* observe_point, float* uncert_model, void* stream);

/* ------------------------------------------------------------------------------------------
 * The frame to ask about, by expected information gain under the span posterior (HUAL_ABI_VERSION unchanged: one new symbol, nothing
 * else moved).  The annotator answers "is frame t inside the ground-truth span?" (append_AP, utils_hual.py:133-139); the answer is a
 * function of the true span, so its mutual information with the span is the entropy of the answer, h2(q(t)) bits, q(t) the posterior
 * probability that t lies inside the span given the answers so far.  Per sample n of the set, T = tlen[n], v = vlen[n] clamped to
 * [0, T], s0 / e0 f32 [N, ld] the deterministic logits (prop_logits, or a bank's s0 / e0):
 *  - p_s, p_e: the float32 softmaxes of the logits over [0, v), bit for bit those of hual_span_argmax (as hual_span_expected_iou);
 *    w(i,j) = (double)p_s[i] * (double)p_e[j] for 0 <= i <= j < v, Z = sum of w.
 *  - active points with a frame index outside [0, v) are ignored.  pos = the ap_pos = 1 entries, neg = the ap_pos = 0 entries.  The
 *    consistent set A: every span with i <= min(pos) and max(pos) <= j (when pos is not empty) and no neg frame in [i, j]; Z_A = the
 *    sum of w over A.
 *  - incl [N, ld] (may be NULL): q(t) = (sum of w over the spans of A with i <= t <= j) / Z_A, float64, clamped to [0, 1], stored as
 *    float32.  gain [N, ld] (may be NULL): h2((float)q(t)), the float32 binary entropy of hual_al_score_info.  Columns [0, T) are
 *    written, 0 at t >= v; columns [T, ld) are not touched.
 *  - query_point [N]: the first t < v of maximal gain (the first-maximal-frame rule of hual_al_score); query_gain [N]: that gain.
 *  - post_entropy [N]: the entropy of the posterior in bits, log2(Z_A) - (1/Z_A) * sum over A of w * (log2f(p_s[i]) + log2f(p_e[j])),
 *    terms with w == 0 skipped, float64 accumulation, clamped at >= 0, stored as float32.  With no active point it is the span_entropy
 *    of hual_span_expected_iou up to rounding.
 *  - agree [N]: (float)(Z_A / Z), the mass the model puts on the spans the annotator has not ruled out; 1 with no active point.
 *  - a poisoned row - v < 1, a NaN logit at t < v, a Z that is not a positive finite number, or T > 256 (T is device memory: the host
 *    cannot refuse it) -: query_point = -1, query_gain = post_entropy = agree = -1.0f, incl / gain columns [0, min(T, ld)) 0.
 *  - contradictory answers - Z_A is not positive: a negative inside the hull of the positives, every frame negative, or every weight
 *    of A underflowed -: agree = 0, query_point = -1, query_gain = post_entropy = -1.0f, incl / gain 0.
 *  - a collapsed posterior (one consistent span; v == 1) is not an error: every gain is 0 and query_point is the first frame.  Callers
 *    test query_gain > 0.
 * The sums are taken as segmented prefix / suffix sums of p_s, p_e, p_s log2f p_s and p_e log2f p_e (a negative frame closes a
 * segment) in float64, each a sum of terms of one sign in a fixed order: no walk over the triangle, no atomics, nothing grid wide.  One
 * launch over the whole set, one workgroup per sample.  Allocates nothing and does not synchronise: capturable in a hipGraph.
 * Argument errors (a null pointer other than incl and gain, N < 1, ld outside [2, 1024]) return before any HIP call. */
int hual_al_query(const hual_al_set* set, const float* s0, const float* e0, float* incl, float* gain, int32_t* query_point,
                  float* query_gain, float* post_entropy, float* agree, void* stream);

/* ------------------------------------------------------------------------------------------
 * The pseudo-label by minimum Bayes risk under the same posterior (HUAL_ABI_VERSION unchanged: one new symbol, nothing else moved).
 * Beside hual_al_renew, the reference's hand-tuned mix: the span of the consistent set that maximises the expected temporal IoU under
 * the span posterior given the answers - the decision of least expected loss in the evaluation's own metric - and that expectation as
 * its confidence.  Per selected sample n (sel: device i32 [nsel] sample ids in any order, each at most once, an id outside [0, N)
 * writes nothing; sel NULL: all N samples), with T, v, p_s, p_e, w, the ignored active points, A and Z_A exactly as hual_al_query
 * above defines them:
 *  - the expected tIoU of a span (a, e): R(a, e) = (1 / Z_A) * sum over (i, j) in A of w(i,j) * inter / union, inter = max(0, min(e, j)
 *    + 1 - max(a, i)), union = (e - a + 1) + (j - i + 1) - inter: the frame-count IoU of hual_span_expected_iou.  Float64 accumulation,
 *    clamped to [0, 1], stored as float32.
 *  - new_idx i32 [N, 2]: the member (a, e) of A of maximal R in the kernel's own float64 arithmetic; among equal values the first in
 *    row-major order (smallest a, then smallest e).  conf f32 [N]: that R.  Only the rows / entries of selected samples are written.
 *  - old_idx i32 [N, 2] and old_conf f32 [N] (both or neither; both NULL: not computed): old_conf = R of the sample's old span
 *    (old_idx[n][0], old_idx[n][1]), whether or not it lies in A; -1.0f where it is not a span of the clip (a < 0, a > e or e >= v).
 *  - a poisoned row (v < 1, a NaN logit at t < v, a Z that is not a positive finite number, or T > 256) and a contradictory row (Z_A
 *    not positive) give no label: new_idx = (-1, -1), conf = old_conf = -1.0f.  Callers test new_idx[n][0] >= 0.
 *  - a collapsed posterior (one consistent span; v == 1) is not an error: the label is that span and conf is 1.
 * No pair of spans is enumerated: A is a union of regions {sa <= i <= ihi, jlo <= j <= sb, i <= j} (a gap between negatives, or
 * (negL, lo] x [hi, negR) around the positive hull), a candidate overlaps only the spans of its own region, and within it Z_A R(a, e)
 * is the sum of four products of a prefix or suffix sum over i with G_e[m] = sum_{j = max(m, jlo) .. e} p_e[j] (j - m + 1) or
 * H_e[l] = sum_{j = e + 1 .. sb} p_e[j] / (j - l + 1) - sums of terms of one sign in float64 in a fixed order, no difference of
 * prefix sums, at most O(v^3) additions per clip, no atomics, nothing grid wide.  One launch, one workgroup per selected sample.
 * Allocates nothing and does not synchronise: capturable in a hipGraph.
 * Argument errors (a null pointer other than sel, old_idx and old_conf; exactly one of old_idx and old_conf null; nsel < 1 - also
 * where sel is NULL and nsel is otherwise not read -; N < 1; ld outside [2, 1024]) return HUAL_ERR_INVALID before any HIP call. */
int hual_al_mbr_label(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel, const int32_t* old_idx,
                      int32_t* new_idx, float* conf, float* old_conf, void* stream);

/* ------------------------------------------------------------------------------------------
 * Where to ask, by the expected gain of the pseudo-label's tIoU under the same posterior (HUAL_ABI_VERSION unchanged: one new symbol,
 * nothing else moved).  hual_al_query chooses the question in bits, hual_al_mbr_label the label in tIoU; this is the one-step lookahead
 * that joins them: the expected value of the answer at frame t in the metric itself - how much the expected tIoU of the label that
 * hual_al_mbr_label would produce after the answer exceeds that of today's label.  A frame can carry a full bit and leave the best
 * label where it was.  Per selected sample n (sel / nsel as in hual_al_mbr_label), with T, v, p_s, p_e, w, the ignored active points,
 * A, Z_A and the poisoned / contradictory / collapsed row rules exactly those of hual_al_query and hual_al_mbr_label, and a frame t
 * in [0, v):
 *  - A_t+ = the spans of A with i <= t <= j (the annotator says "inside"), A_t- = the rest of A; Z_t+ and Z_t- their masses,
 *    Z_t+ + Z_t- = Z_A.
 *  - M_b(t), b in {+, -} = the max over the members c of A_t^b of the sum over (i, j) in A_t^b of w(i,j) * IoU(c, (i,j)), the frame-count
 *    IoU of hual_al_mbr_label; 0 where Z_t^b is not positive.  The un-normalised value of the label after that answer.
 *  - V0 = the max over c in A of R(c): the conf of hual_al_mbr_label on the same set.
 *  - gain(t) = (M_+(t) + M_-(t)) / Z_A - V0, float64, clamped to [0, 1], stored as float32.  (The clamp at 0: the label is restricted
 *    to the consistent set, so non-negativity is not a theorem.)  A frame whose answer the posterior already determines - Z_t+ or Z_t-
 *    not positive - has gain exactly 0.0f, with no arithmetic.
 *  - cand i32 [N, M], 1 <= M <= 256, or NULL = every frame of the clip (M is then not read).  With cand only the frames cand[n][0..M)
 *    are evaluated, in that order; entries outside [0, v) (-1, say) are skipped.
 *  - gain f32 [N, ld] (may be NULL): columns [0, T) are written - the gain at the evaluated frames, 0 elsewhere -, columns [T, ld) are
 *    not touched.
 *  - ask_point i32 [N]: the first evaluated frame of maximal gain in the kernel's own float64 arithmetic; ask_gain f32 [N]: that gain.
 *    value f32 [N]: V0.  Only the rows / entries of selected samples are written.
 *  - a poisoned or contradictory row: ask_point = -1, ask_gain = value = -1.0f, gain columns [0, min(T, ld)) 0.
 *  - a collapsed posterior, or a candidate list with no frame inside the clip: every gain is 0 and ask_gain = 0; ask_point is the first
 *    evaluated frame, -1 if there was none.  Callers test ask_gain > 0.
 * Each branch is maximised as hual_al_mbr_label maximises A, over its regions: "inside" always leaves one, (negL', lo'] x [hi', negR');
 * "outside" beside a positive hull moves negL or negR; without a positive it splits the gap that holds t, and the other gaps keep
 * maxima computed once.  Both branches divide by the parent's Z_A, so a branch's best is M_b / Z_A.  Up to 2 v maximisations per clip,
 * each at most cubic in its region: float64 sums of terms of one sign in a fixed order, no atomics, nothing grid wide.  One launch, one
 * workgroup per selected sample.  Allocates nothing and does not synchronise: capturable in a hipGraph.
 * Argument errors (a null pointer other than sel, cand and gain; nsel < 1; N < 1; ld outside [2, 1024]; cand given with M outside
 * [1, 256]) return HUAL_ERR_INVALID before any HIP call. */
int hual_al_label_gain(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel, const int32_t* cand,
                       int M, float* gain, int32_t* ask_point, float* ask_gain, float* value, void* stream);

/* ------------------------------------------------------------------------------------------
 * What to train on, under the same posterior (HUAL_ABI_VERSION unchanged: one new symbol, nothing else moved).  hual_al_query reads the
 * posterior for the question, hual_al_mbr_label for one hard span; these are its two marginals - the distribution of the start frame
 * and of the end frame given the answers - in the shape of the model's y1 / y2 feeds, whose loss is a soft cross entropy: a clip whose
 * posterior still spreads over twenty frames is trained with that spread, and an answered negative carries no mass.  Per sample n of
 * the set, with T, v, p_s, p_e, w, the ignored active points, A and Z_A exactly as hual_al_query above defines them:
 *  - y_start f32 [N, ld]: y_start[n][i] = (1 / Z_A) * the sum over the j with (i, j) in A of w(i,j);
 *    y_end f32 [N, ld]: y_end[n][j] = (1 / Z_A) * the sum over the i with (i, j) in A of w(i,j).  Float64 accumulation, stored as
 *    float32; each row sums to 1 up to that rounding.  Columns [0, T) are written, 0 at t >= v; columns [T, ld) are not touched.
 *  - status i32 [N]: 1 for a live row; 0 for a poisoned row (v < 1, a NaN logit at t < v, a Z that is not a positive finite number, or
 *    T > 256) and for a contradictory one (Z_A not positive), whose columns [0, min(T, ld)) of both outputs are 0.
 *  - a collapsed posterior (one consistent span; v == 1) is not an error: the row is live and both outputs are one-hot.
 * No walk over the triangle: within A the partners of a frame form one interval.  Around a positive hull A = (negL, lo] x [hi, negR)
 * and the marginals are independent, p_s[i] / S and p_e[j] / E with S and E the sums over those two intervals; without a positive A is
 * the union of the triangles over the gaps between negatives, Z_A y_start[i] = p_s[i] * (the sum of p_e from i to the end of i's gap)
 * and Z_A y_end[j] = p_e[j] * (the sum of p_s from the start of j's gap to j).  Every sum adds terms of one sign in float64 in a fixed
 * order: no difference of prefix sums, no atomics, nothing grid wide.  One launch over the whole set, one workgroup per sample.
 * Allocates nothing and does not synchronise: capturable in a hipGraph.
 * Argument errors (a null pointer, N < 1, ld outside [2, 1024]) return HUAL_ERR_INVALID before any HIP call. */
int hual_al_span_marginals(const hual_al_set* set, const float* s0, const float* e0, float* y_start, float* y_end, int32_t* status,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * The same posterior under an annotator who errs (HUAL_ABI_VERSION unchanged: two new symbols, nothing else moved).  The launches above
 * take every answer as a hard constraint: one wrong click makes a row contradictory, or silently deletes the true span from A.  Let every
 * answer be wrong independently with probability eps, r = (1 - eps) / eps, and G(t) = (the positive answers at frames <= t) - (the
 * negative answers at frames <= t), G(-1) = 0, duplicated answers counted once each (independent clicks).  The likelihood of the
 * answers under the span (i, j) is eps^npos (1 - eps)^nneg r^(G(j) - G(i-1)), so
 *   posterior(i, j)  ~  p_s(i) r^(-G(i-1)) * p_e(j) r^(G(j))  on the whole triangle i <= j < v:
 * the product form of tilted logits with no constraint left.  hual_al_query, hual_al_mbr_label and hual_al_span_marginals read the noisy
 * posterior from the tilted rows and a set without answers (ap_off all 0), as they are; no row is contradictory any more.
 *
 * hual_al_noisy_tilt: per sample n of the set, with T, v, p_s, p_e, w, Z and the ignored active points exactly as hual_al_query
 * defines them and lam = (float)log((1.0 - (double)eps) / (double)eps) computed on the host:
 *  - s_t f32 [N, ld]: s_t[n][i] = s0[n][i] - (float)G(i-1) * lam for i < v; e_t f32 [N, ld]: e_t[n][j] = e0[n][j] + (float)G(j) * lam
 *    for j < v - one float32 product and one float32 subtraction / addition, each rounded on its own (no contraction); where the
 *    count or lam is 0 the logit is copied (eps = 0.5 returns the input bit for bit).  Columns [v, T) are copied from the input,
 *    columns [T, ld) are not touched.
 *  - log_evidence f32 [N]: ln P(the answers | the model, eps) = ln(sum over i <= j < v of w(i,j) * prod_k lik_k(i,j)) - ln Z, lik_k =
 *    1 - eps where answer k agrees with the span and eps where not, w and Z from the UNTILTED logits.  Float64, as sum_j b(j) sum_{i <=
 *    j} a(i) with the powers of r carried as integer exponents against the row's maxima (64 answers at eps = 1e-6 do not overflow), sums
 *    of terms of one sign in a fixed order, no atomics; stored as float32.  It takes the place of hual_al_query's agree as the measure
 *    of how far the model and the annotator disagree, and its sum over a set is the likelihood a caller maximises to choose eps.
 *  - a poisoned row (v < 1, a NaN logit at t < v, a Z that is not a positive finite number, or T > 256): columns [0, min(T, ld)) are
 *    copied raw - the launches that read them poison the row again - and log_evidence is a quiet NaN.
 * One launch over the whole set, one workgroup per sample.  Allocates nothing and does not synchronise: capturable in a hipGraph.
 * Argument errors (a null pointer, N < 1, ld outside [2, 1024], eps outside (0, 0.5] or NaN) return HUAL_ERR_INVALID before any HIP
 * call. */
int hual_al_noisy_tilt(const hual_al_set* set, const float* s0, const float* e0, float eps, float* s_t, float* e_t, float* log_evidence,
                       void* stream);

/* hual_al_label_gain rebuilt for the noisy annotator: an answer re-weights the triangle instead of cutting it, and the label after it
 * may be any span.  It reads N, ld, vlen and tlen of the set - the active points are NOT read: they are in the tilted rows s_t / e_t
 * already - and p_s, p_e, w, Z of those rows as the family computes them.  Per selected sample and frame t in [0, v), with
 *   F_in_t(c)  = the sum over the spans with i <= t <= j of w * IoU(c, .)      F_out_t(c) = the same over the other spans
 * (the frame-count IoU of hual_al_mbr_label), c any span of the clip:
 *  - M_yes(t) = max_c [(1 - eps) F_in_t(c) + eps F_out_t(c)];  M_no(t) = max_c [eps F_in_t(c) + (1 - eps) F_out_t(c)];
 *    V0 = max_c (F_in_t(c) + F_out_t(c)) / Z, independent of t: the conf of hual_al_mbr_label on the same rows and a set without answers.
 *  - gain(t) = (M_yes(t) + M_no(t)) / Z - V0, float64, clamped to [0, 1], stored as float32.  gain >= 0 is a theorem here - the
 *    candidates are not restricted - and the clamp only absorbs rounding.
 *  - sel / nsel, cand / M, gain f32 [N, ld], ask_point, ask_gain and value (= V0), the first-maximal-frame rule, the column ranges, the
 *    flags of a poisoned row and an id outside [0, N) writing nothing are hual_al_label_gain's, word for word.  No row is contradictory.
 * F_out_t is summed over the two triangles [0, t-1] and [t+1, v), F_in_t over the rectangle [0, t] x [t, v): the four prefix / suffix
 * products of hual_al_mbr_label with the bounds clamped per region, a candidate lying in any region or straddling them.  Float64 sums of
 * terms of one sign in a fixed order (no F - F_in), no atomics, nothing grid wide; about v^3 additions per evaluated frame, v^4 per clip
 * with every frame.  One launch, one workgroup per selected sample.  Allocates nothing and does not synchronise: capturable in a hipGraph.
 * Argument errors (those of hual_al_label_gain; eps outside (0, 0.5] or NaN) return HUAL_ERR_INVALID before any HIP call. */
int hual_al_label_gain_noisy(const hual_al_set* set, const float* s_t, const float* e_t, float eps, const int32_t* sel, int nsel,
                             const int32_t* cand, int M, float* gain, int32_t* ask_point, float* ask_gain, float* value, void* stream);

/* ------------------------------------------------------------------------------------------
 * Annotation sessions: several adaptive questions per clip in one launch (HUAL_ABI_VERSION unchanged: one new symbol, nothing else
 * moved).  The posterior above conditions on the answers, not on a new forward pass: after the annotator has answered frame t, the best
 * next frame is defined by the same logits.  hual_al_session spends up to qmax questions on every selected sample, each chosen after
 * the previous answer, the annotator simulated from the ground-truth span (append_AP, utils_hual.py:133-139), and stops as soon as the
 * posterior has collapsed far enough.  One workgroup per selected sample; the list of active points and the transcript live in LDS.
 *
 * Inputs: the set with the answers of earlier rounds; s0 / e0 f32 [N, ld], the UNTILTED deterministic logits; gt i32 [N, 2], the
 * ground-truth frame span (inclusive); sel / nsel as in hual_al_mbr_label (sel NULL: all N samples; rows not listed are left untouched;
 * an id outside [0, N) writes nothing; a repeated id writes the same values twice); qmax in [1, 16]; budget i32 [N] (may be NULL: qmax
 * everywhere), the per-sample cap, clamped to [0, qmax]; stop_entropy in bits (negative: off); min_gain in bits, >= 0; eps: 0 selects
 * the hard rule of hual_al_query, a value in (0, 0.5] the noisy annotator of hual_al_noisy_tilt; flip u32 [N] (may be NULL: no flip),
 * bit k flips the k-th answer of this session.
 *
 * Per selected sample, with k = the questions asked so far, the list = the set's points followed by this session's:
 *  1. the posterior on the list.  eps == 0: exactly hual_al_query on a set that holds the list (p_s, p_e and their log2f are computed
 *     once; the hull, the segments and the segmented float64 sums per step).  eps > 0: exactly hual_al_noisy_tilt of the list applied
 *     to s0 / e0 (never a tilt of a tilt), then hual_al_query on the tilted rows and a set without answers.
 *  2. the frame: hual_al_query's query_point - q(t), h2((float)q(t)), the first frame of maximal gain - and its post_entropy.
 *  3. the stop conditions, in this order: the row is poisoned (hual_al_query's rule; under eps > 0 also hual_al_noisy_tilt's)
 *     -> HUAL_AL_STOP_POISONED; contradictory (eps == 0 only) -> _CONTRADICTORY; stop_entropy >= 0 and post_entropy <= stop_entropy ->
 *     _ENTROPY; query_gain <= min_gain (a gain of 0 always stops) -> _GAIN; k == budget -> _BUDGET.
 *  4. otherwise the answer is (gt[n][0] <= t <= gt[n][1]) XOR bit k of flip[n]; it joins the list and k grows.
 * The list has room for 64 points: a sample whose points in the set plus its budget exceed that asks nothing and reports
 * HUAL_AL_STOP_OVERFLOW (checked first, before the row is opened).
 *
 * Outputs, each written for every selected sample: asked i32 [N, qmax] the frames in order; answer i8 [N, qmax] 1 / 0 as appended;
 * q_asked f32 [N, qmax] = incl of hual_al_query at the asked frame; gain f32 [N, qmax] = its query_gain; entropy f32 [N, qmax + 1] =
 * post_entropy before each question and after the last (the pass that stopped the session), -1 where that pass found the row
 * poisoned or contradictory; unused slots hold -1 in all five.  n_asked i32 [N]; stop_reason i32 [N].  Every stored float is bit for
 * bit what the launches it replaces store (one shared body: csrc/spanstep.h).
 * Allocates nothing and does not synchronise: capturable in a hipGraph.  Argument errors (a null pointer other than sel, budget and
 * flip, N < 1, ld outside [2, 1024], nsel < 1 with sel, qmax outside [1, 16], min_gain < 0 or NaN, eps neither 0 nor in (0, 0.5])
 * return HUAL_ERR_INVALID before any HIP call. */
#define HUAL_AL_STOP_BUDGET 0
#define HUAL_AL_STOP_ENTROPY 1
#define HUAL_AL_STOP_GAIN 2
#define HUAL_AL_STOP_CONTRADICTORY 3
#define HUAL_AL_STOP_POISONED 4
#define HUAL_AL_STOP_OVERFLOW 5
int hual_al_session(const hual_al_set* set, const float* s0, const float* e0, const int32_t* gt, const int32_t* sel, int nsel, int qmax,
                    const int32_t* budget, float stop_entropy, float min_gain, float eps, const uint32_t* flip, int32_t* asked,
                    int8_t* answer, float* q_asked, float* gain, float* entropy, int32_t* n_asked, int32_t* stop_reason, void* stream);

/* Sessions that stop once the pseudo-label is reliable (HUAL_ABI_VERSION unchanged: one new symbol, nothing else moved).  The stop
 * rules above are in bits, but the annotation is for a label: hual_al_session_label is hual_al_session with, per pass, the label the
 * list so far gives and the chance that this label counts as a hit, and one more stop rule on that chance - "ask until the label is
 * safe at IoU 0.7 with probability 0.9".
 *
 * Inputs: those of hual_al_session, word for word, plus thresholds / M as in hual_al_hit_label (HOST int32 [M][2] = (num, den), 1 <=
 * num <= den <= 1024, 1 <= M <= 4, passed by value), stop_m in [0, M), the threshold the rule reads, and stop_hit: negative = the rule
 * is off, else a probability in (0, 1].
 *
 * Per selected sample, with k = the questions asked so far:
 *  1. the posterior on the list and the frame: steps 1 and 2 of hual_al_session.
 *  2. on a live pass, the label: hual_al_mbr_label's new_idx and conf on a set that holds the list (eps == 0), or on the tilted rows
 *     and a set without answers (eps > 0: any span of the clip).
 *  3. its reliability: hual_al_hit_label's cand_hit of that one span at the M thresholds, on the same set and rows.
 *  4. the stop conditions, in this order: poisoned; contradictory; stop_hit >= 0 and the STORED float32 label_hit[k][stop_m] >=
 *     stop_hit -> HUAL_AL_STOP_RELIABLE; then stop_entropy, min_gain and the budget exactly as in hual_al_session.
 *  5. otherwise the question is asked, answered and appended as in hual_al_session.
 * The 64-point list and HUAL_AL_STOP_OVERFLOW are hual_al_session's.
 *
 * Outputs, each written for every selected sample: the seven outputs of hual_al_session with the same meaning, and label i32
 * [N, qmax + 1, 2], label_conf f32 [N, qmax + 1], label_hit f32 [N, qmax + 1, M]: slot k holds the pass before question k, slot
 * n_asked the pass that stopped the session - the final label, what hual_al_mbr_label gives on the list the session leaves.  Unused
 * slots, and passes that found the row poisoned or contradictory, hold -1 in all three.  With stop_hit off the seven session outputs
 * are hual_al_session's bit for bit.  Every stored value is bit for bit what hual_al_noisy_tilt (eps > 0), hual_al_query,
 * hual_al_mbr_label and hual_al_hit_label store on the same list (shared bodies: csrc/spansession.h, spanstep.h, spanmbr.h,
 * spanmass.h; the divisor Z_A is that of the two label launches), and every decision follows from the stored float32 values.
 * One 1024-thread workgroup per selected sample; each pass costs one label search, about v^3 / 2 float64 additions on a row without
 * answers.  No atomics, nothing grid wide: a second launch returns equal bits.  Allocates nothing and does not synchronise:
 * capturable in a hipGraph.  Argument errors (those of hual_al_session; a null thresholds, label, label_conf or label_hit; M, a
 * threshold or stop_m out of range; stop_hit 0, above 1 or NaN) return HUAL_ERR_INVALID before any HIP call. */
#define HUAL_AL_STOP_RELIABLE 6
int hual_al_session_label(const hual_al_set* set, const float* s0, const float* e0, const int32_t* gt, const int32_t* sel, int nsel,
                          int qmax, const int32_t* budget, float stop_entropy, float min_gain, float eps, const uint32_t* flip,
                          const int32_t* thresholds, int M, int stop_m, float stop_hit, int32_t* asked, int8_t* answer, float* q_asked,
                          float* gain, float* entropy, int32_t* n_asked, int32_t* stop_reason, int32_t* label, float* label_conf,
                          float* label_hit, void* stream);

/* ------------------------------------------------------------------------------------------
 * Question sets for an annotator who is not in the loop: M frames per clip in one launch (HUAL_ABI_VERSION unchanged: one new symbol,
 * nothing else moved).  hual_al_session answers each question inside the kernel, so it serves the simulated annotator only; a labelling
 * tool, a crowd batch or one viewing of a clip takes the frames of a clip TOGETHER.  The answer at frame t is [i <= t <= j], a function
 * of the span (i, j), so the information a set of frames D = (t_1 .. t_m) carries about the span is the entropy of its answer vector,
 *   I(D) = -sum over the outcomes o of P(o) log2 P(o),  P(o) = the mass of the spans of A with answer vector o, over Z_A,
 * with A, Z_A, p_s, p_e of a row exactly hual_al_query's; the expected entropy left after the answers is post_entropy - I(D).  The
 * positive answers of a span are a contiguous run of the sorted D and every span that holds no frame of D answers alike, so there are at
 * most m (m + 1) / 2 + 1 outcomes.  hual_al_design builds D greedily: step m takes the first frame t < v of maximal I(D + t).
 *
 * Inputs: the set, s0 / e0 f32 [N, ld] and sel / nsel as in hual_al_session (sel NULL: all N samples; rows not listed are left
 * untouched; an id outside [0, N) writes nothing; a repeated id writes the same values twice); mmax in [1, 16]; forced i32 [N, mmax]
 * (may be NULL: none): row n's leading entries >= 0 are the first frames of its design, placed in that order without a stop test - how
 * a hand-made grid or a bisection schedule is scored - and the greedy continues behind them; an entry < 0 ends the prefix; an entry
 * >= v is ignored, as the family ignores such active points: it takes no slot; a forced frame that repeats, or that the set has already
 * answered, carries 0 bits and stays in the list.  min_gain in bits, >= 0; stop_entropy in bits (negative: off).
 *
 * Per selected sample, with m = the frames placed so far, I = the running float64 information (0 at m = 0):
 *  1. the row is opened and read by hual_al_query's own code: a poisoned row -> HUAL_AL_STOP_POISONED, a contradictory one ->
 *     _CONTRADICTORY, nothing placed.  post_entropy f32 [N] is hual_al_query's, bit for bit (-1 on such a row).
 *  2. m == mmax -> _BUDGET.
 *  3. every frame's marginal gain g(t) = I(D + t) - I(D).  At m = 0 it is hual_al_query's gain, the float32 h2((float)q(t)), widened; at
 *     m >= 1 the chain rule, sum over the outcomes o of P(o) h2(q_o(t)) in float64, q_o(t) the inclusion probability of t under the
 *     posterior restricted to o: t lies inside or outside an outcome (q = 1, 0) or splits its start cell, its end cell or - the
 *     all-negative outcome - its triangle, each read from float64 sums of p_s / p_e that restart at every negative of the set and at
 *     every placed frame that carried information (no difference of whole-row prefix sums).  A placed or answered frame has g = 0.
 *  4. a pending forced frame is placed: I += g(t).  Otherwise, in this order: stop_entropy >= 0 and H_A - I <= stop_entropy (H_A
 *     post_entropy's float64) -> _ENTROPY; the best g <= min_gain (a gain of 0 always stops) -> _GAIN; else the first frame of
 *     maximal g is placed.  At m = 0 that frame and gain are hual_al_query's query_point and query_gain.
 * Outputs, each written for every selected sample: frames i32 [N, mmax] in the order placed; info f32 [N, mmax], info[n][m] = (float) of I
 * after m + 1 frames, non-decreasing, at most min(m + 1, post_entropy) up to rounding; unused slots hold -1 in both.  n_design i32 [N];
 * stop_reason i32 [N] (HUAL_AL_STOP_*).  No atomics, a fixed order: two launches give the same bits, and a design fed back as `forced`
 * returns itself with the same info (the forced frame's gain is read from the row the greedy step maximises).
 * One workgroup per selected sample; the design and its cell boundaries live in LDS.  Allocates nothing and does not synchronise:
 * capturable in a hipGraph.  Argument errors (a null pointer other than sel and forced, N < 1, ld outside [2, 1024], nsel < 1 with sel,
 * mmax outside [1, 16], min_gain < 0 or NaN, a NaN stop_entropy) return HUAL_ERR_INVALID before any HIP call. */
int hual_al_design(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel, int mmax,
                   const int32_t* forced, float min_gain, float stop_entropy, int32_t* frames, float* info, float* post_entropy,
                   int32_t* n_design, int32_t* stop_reason, void* stream);

/* ------------------------------------------------------------------------------------------
 * Calibrating the span posterior by the evidence of the answers (HUAL_ABI_VERSION unchanged: one new symbol, nothing else moved).  Every
 * launch above takes the softmaxes of s0 / e0 at face value and eps as the caller's number.  With a temperature tau,
 *   L(tau, eps) = sum over the samples n of ln P(the answers of n | softmax(s0[n] / tau), softmax(e0[n] / tau), eps)
 * is a proper likelihood of the pair (the policy that chose the questions depended on the answers only through earlier data: it drops
 * out); hual_al_evidence_grid evaluates it on a grid of A x B pairs in one call, for the caller to maximise.
 *
 * Inputs: the set with its answers; s0 / e0 f32 [N, ld], the UNTILTED, unscaled deterministic logits; sel / nsel as in
 * hual_al_mbr_label (sel NULL: all N samples, nsel >= 1 all the same; an id outside [0, N) writes nothing and is not summed; a repeated
 * id writes the same values twice and is summed twice); inv_tau HOST f32 [A], 1 <= A <= 32, the reciprocal temperatures, each finite and
 * > 0; eps HOST f32 [B], 1 <= B <= 16, each in (0, 0.5].  Both arrays are read before the call returns.
 *
 * Per selected sample n and cell c = a * B + b: the row is x_s[i] = s0[n][i] * inv_tau[a], x_e[j] = e0[n][j] * inv_tau[a] - one float32
 * product, rounded on its own (never fused with the softmax's subtraction behind it): the row `s0 * inv_tau` of a float32 tensor
 * library.  T, v, p_s, p_e (bit for bit the family's softmaxes of that row), w, Z, the ignored active points, G(t), r = (1 - eps[b]) /
 * eps[b] and the poison rule are hual_al_noisy_tilt's on that row and that eps.
 *  - table f64 [N, A * B]: table[n][c] = hual_al_noisy_tilt's log_evidence of that row, ln(sum over i <= j < v of w(i,j) * prod_k
 *    lik_k(i,j)) - ln Z, in float64 and NOT rounded to float32.  It is computed as sum_j p_e[j] r^G(j) sum_{i <= j} p_s[i] r^-G(i-1) with
 *    every partial sum held as a pair (mantissa, integer exponent of r) against the larger exponent of its two operands - a term of
 *    mantissa 0 carries no exponent -, the inner sum a prefix scan: O(v + answers) float64 operations per cell, no exponential per
 *    (start, end) pair, and 64 answers at eps = 1e-6 neither overflow nor underflow the spans that carry the sum.  ln eps, ln(1 - eps)
 *    and ln r are the host's float64 values of the float32 eps widened.
 *  - a poisoned cell - v < 1, a NaN logit at t < v, T > 256, or at THIS temperature a Z that is not a positive finite number (a
 *    scaled softmax that went one-hot with the start behind the end; a product that overflowed) - is a quiet NaN.
 *  - status i32 [N]: 1 if every one of the row's A * B cells is finite, else 0.
 *  - a sample without an answer inside [0, v) is live, and every cell that is not poisoned is exactly 0.
 *  - rows of samples that are not selected are not written, in table or status.
 * Then, on the same stream: total f64 [A * B], total[c] = the float64 sum of table[sel[k]][c] over the entries k = 0 .. nsel - 1 whose id
 * lies in [0, N) and whose status is 1 - a row with one poisoned cell is left out of EVERY cell, so that all totals sum the same rows
 * and their differences are likelihood ratios - in a fixed order: two calls give the same bits.  counts i32 [4]: the rows summed; the
 * answers inside [0, v) of those rows; the entries with an id in [0, N) left out; the first cell of maximal total, -1 if no row was
 * summed.
 * Three launches (one workgroup per selected sample; one per cell; one wave).  Allocates nothing and does not synchronise: capturable
 * in a hipGraph.  Argument errors (a null pointer other than sel, N < 1, nsel < 1, ld outside [2, 1024], A outside [1, 32], B outside
 * [1, 16], an inv_tau that is not finite and > 0, an eps outside (0, 0.5] or NaN) return HUAL_ERR_INVALID before any HIP call. */
int hual_al_evidence_grid(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel, const float* inv_tau,
                          int A, const float* eps, int B, double* table, int32_t* status, double* total, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * The span posterior as a Bayesian model average over K stochastic passes (HUAL_ABI_VERSION unchanged: two new symbols, nothing else
 * moved).  The launches above read the softmax of ONE deterministic forward at face value; a temperature (hual_al_evidence_grid) is
 * one scalar for the whole set.  With K MC-dropout passes the predictive distribution over spans is the mixture P(i,j) = (1/K) sum_k
 * P_k(i,j), every P_k the product form above, and conditioning on the answers keeps it a mixture: P(i,j | answers) = sum_k w_k
 * P_k(i,j | answers), w_k proportional to pass k's evidence of the answers - a pass the annotator contradicts is down-weighted, which
 * no scalar temperature can do.
 *
 * hual_al_ensemble_query: pass_s / pass_e f32 [K, N, ld], plane stride N * ld, 1 <= K <= 16 (a McBank's kept passes); logw f32 [K, N]
 * (may be NULL: 0), a finite log prior weight per pass and row, widened to float64.  Per sample n of the set and pass k, with T, v,
 * p_s,k, p_e,k, w, Z_k, the ignored active points, A and Z_A,k exactly as hual_al_query defines them on plane k (A depends on the
 * answers and v only: the passes share it):
 *  - u_k = ln(Z_A,k / Z_k) + logw[k][n]; a pass whose Z_A,k is not positive (or whose u_k is not finite) has w_k = 0; weight f32 [N, K]:
 *    weight[n][k] = w_k = exp(u_k - max u) / sum_k exp(u_k - max u), float64, stored as float32; log_evidence f32 [N] = max u +
 *    ln(sum_k exp(u_k - max u)) - ln K: ln P(the answers | the ensemble) with logw NULL.
 *  - incl [N, ld] (may be NULL): sum_k w_k q_k(t), q_k hual_al_query's q of pass k before its rounding, float64, clamped to [0, 1],
 *    stored as float32; gain [N, ld] (may be NULL): h2((float)incl); query_point / query_gain [N]: the first t < v of maximal gain and
 *    that gain.  Columns [0, T) are written, 0 at t >= v; columns [T, ld) are not touched.
 *  - y_start / y_end f32 [N, ld] (both, or both NULL): sum_k w_k of pass k's marginals as hual_al_span_marginals defines them; columns
 *    as incl.
 *  - expected_entropy f32 [N]: sum_k w_k H_k, H_k hual_al_query's post_entropy of pass k (its closed form, clamped at >= 0) in float64.
 *    post_entropy f32 [N]: the entropy in bits of the mixture m(i,j) = sum_k (w_k / Z_A,k) p_s,k[i] p_e,k[j] over A, -sum m log2 m,
 *    terms with m == 0 skipped, clamped at >= 0.  span_bald f32 [N] = max(0, post_entropy - expected_entropy), formed in float64
 *    before rounding: the mutual information between the span and the dropout mask given the answers - BALD in the span's own
 *    currency, a clip-level epistemic score.
 *  - every sum over the passes is taken in ascending k, passes without weight skipped.  With K = 1 and logw NULL w_1 is exactly 1 and
 *    incl, gain, query_point, query_gain, y_start, y_end and expected_entropy are the single-pass launches' outputs bit for bit.
 *  - status i32 [N]: 1 for a live row, 0 otherwise.  A poisoned row - ANY of its K passes poisoned by hual_al_query's rule (v < 1, a
 *    NaN logit at t < v, a Z_k that is not a positive finite number, T > 256) -: query_point = -1, query_gain = post_entropy =
 *    expected_entropy = span_bald = -1.0f, log_evidence a quiet NaN, weight 0, the written columns [0, min(T, ld)) 0.  A contradictory
 *    row - no pass has weight -: the same flags with log_evidence = -inf (the logarithm of an evidence of 0, as hual_al_query's agree
 *    is 0).  A collapsed posterior is not an error: every gain is 0, expected_entropy is the passes' closed form
 *    (0 within hual_al_query's rounding), post_entropy is 0 up to the float64 rounding of sum_k w_k (1e-15 bits) and span_bald is 0.
 * The mixture has no product form, so its entropy is a walk over the pairs of A: all K pairs of factor rows sit in LDS (K * 2 * 256
 * floats, 32 KB at K = 16), the four lanes of start i stride over the ends A allows it, float64 accumulation in a fixed order, one
 * block sum, no atomics: at most K v^2 / 2 multiply-adds and v^2 / 2 logarithms per clip.  Everything else is the family's per-pass
 * arithmetic (no walk).  One launch over the whole set, one workgroup per sample.  Allocates nothing and does not synchronise:
 * capturable in a hipGraph.
 * Argument errors (a null pointer other than logw, incl, gain and the y_start / y_end pair; exactly one of y_start and y_end null; K
 * outside [1, 16]; N < 1; ld outside [2, 1024]) return HUAL_ERR_INVALID before any HIP call.
 *
 * The noisy annotator needs nothing new: run hual_al_noisy_tilt once per plane (a plane is a valid [N, ld] tensor), and pass the tilted
 * planes, a set without answers (ap_off all 0) and the K log_evidence rows [K, N] as logw.  That IS the noisy ensemble posterior: on
 * the tilted rows Z_A,k = Z_k, so u_k = log_evidence_k = ln P(the answers | pass k, eps) - pass k's evidence of the answers is exactly
 * its weight -, the tilted product form is pass k's posterior given the noisy answers, and log_evidence is ln P(the answers | the
 * ensemble, eps).  (A logw that is not finite only takes its pass's weight away.  A row hual_al_noisy_tilt poisoned has a NaN logw
 * AND raw copies of the rows that made it poison: it is those rows, by hual_al_query's rule, that poison the row again here - a caller
 * who hands in a NaN logw beside sound rows gets a pass without weight, and a contradictory row if no pass is left.) */
int hual_al_ensemble_query(const hual_al_set* set, const float* pass_s, const float* pass_e, int K, const float* logw, float* weight,
                           float* log_evidence, float* incl, float* gain, int32_t* query_point, float* query_gain, float* y_start,
                           float* y_end, float* post_entropy, float* expected_entropy, float* span_bald, int32_t* status, void* stream);

/* hual_al_mbr_label under the same model average.  set, pass_s, pass_e, K, logw, the weights w_k and the poisoned / contradictory rules
 * are hual_al_ensemble_query's (one device function opens the row for both launches); sel / nsel, old_idx / old_conf, the flags of a
 * row that gives no label (new_idx = (-1, -1), conf = old_conf = -1.0f) and the tie rule (the first maximal member of A in row-major
 * order) are hual_al_mbr_label's.
 *  - R(a, e) = sum_k w_k R_k(a, e), R_k hual_al_mbr_label's expected tIoU under pass k, float64, the passes in ascending k; new_idx
 *    i32 [N, 2]: the member of A of maximal R; conf f32 [N]: that R, clamped to [0, 1]; old_conf f32 [N]: R of the old span.
 * Per pass the IoU-weighted mass of a candidate is hual_al_mbr_label's four products of prefix and suffix sums; the walk over the
 * ends e is shared and the passes are summed per candidate before the argmax: K times that launch's additions, one barrier per (e,
 * pass).  One launch, one workgroup per selected sample.  Allocates nothing and does not synchronise: capturable in a hipGraph.
 * Argument errors (a null pointer other than logw, sel, old_idx and old_conf; exactly one of old_idx and old_conf null; nsel < 1; K
 * outside [1, 16]; N < 1; ld outside [2, 1024]) return HUAL_ERR_INVALID before any HIP call. */
int hual_al_ensemble_label(const hual_al_set* set, const float* pass_s, const float* pass_e, int K, const float* logw, const int32_t* sel,
                           int nsel, const int32_t* old_idx, int32_t* new_idx, float* conf, float* old_conf, void* stream);

/* ------------------------------------------------------------------------------------------
 * Label reliability: the hit probability of pseudo-labels under the answered-point posterior (HUAL_ABI_VERSION unchanged: one new
 * symbol, nothing else moved).  hual_al_mbr_label's conf is an expected tIoU - a mean, which no yes/no outcome can check.  This launch
 * gives P(IoU(span, truth) >= m | the answers), hual_span_hit_prob's quantity with the truth drawn from hual_al_query's posterior: the
 * one confidence of a label that labelled data can check with a reliability curve (al.hit_calibration).  T, v, p_s, p_e, w(i,j) =
 * (double)p_s[i] * (double)p_e[j], the ignored active points, the consistent set A, Z_A and the poisoned / contradictory / collapsed
 * rules are hual_al_query's, word for word; sel / nsel are hual_al_mbr_label's (NULL: all N; an id outside [0, N) writes nothing; only
 * the entries of selected samples are written); thresholds / M are hual_span_hit_prob's: HOST int32 [M][2] = (num, den), 1 <= num <=
 * den <= 1024, 1 <= M <= 4, passed by value, the hit test den * inter >= num * union in integers on the half-open frame intervals.
 *  - cand_idx i32 [N, k, 2], cand_hit f32 [N, k, M], 0 <= k <= 16: for the candidate (a, b), a member of A or not, the sum of w over
 *    the truths (i, j) IN A that hit it, divided by Z_A, accumulated in float64, clamped to [0, 1].  A slot that is no span of the clip
 *    (a < 0, a > b or b >= v) holds -1.0f in all M columns.  k == 0: both arrays may be NULL.
 *  - best_idx i32 [N, M, 2], best_prob f32 [N, M], both or neither: per threshold the member of A with the largest hit mass in the
 *    kernel's float64 arithmetic, among equal masses the first in row-major order (smallest a, then smallest b), and its probability.
 *    Once answers shrink A, many members hit every remaining truth and tie exactly: a caller that moves a label to this span should
 *    ask for a margin over the label it holds (al.update_labels(renew_by='hit_prob') asks for 1e-6).
 *  - a poisoned or contradictory row: -1.0f in cand_hit and best_prob, (-1, -1) in best_idx.  A collapsed posterior (one span left in
 *    A) is not an error: the best span is that span, with probability 1.0f.
 * Arithmetic: as hual_span_hit_prob - per start i of the truth the hitting ends are one interval, clamped here to the interval of
 * ends A allows that start, and summed as a DIFFERENCE of float64 prefix sums of p_e; the starts are taken in that launch's order, so
 * on a row without active points the masses are its doubles, and the results differ from its results only by the divisor (Z_A and
 * its Z are two float64 sums of the same terms in different orders: at most one float32 ulp).  One 1024-thread workgroup per
 * selected sample, with best_* one per (sample, threshold); a launch without best_* does not search.  No atomics, nothing grid wide:
 * a second launch returns equal bits.  Allocates nothing and does not synchronise: capturable in a hipGraph.  Argument errors (a null
 * pointer among set, s0, e0, thresholds or the arrays of a part that is asked for; only one of best_*; k == 0 without best_*; nsel <
 * 1; N < 1; ld outside [2, 1024]; k, M or a threshold out of range) return HUAL_ERR_INVALID before any HIP call. */
int hual_al_hit_label(const hual_al_set* set, const float* s0, const float* e0, const int32_t* sel, int nsel, const int32_t* thresholds,
                      int M, const int32_t* cand_idx, int k, float* cand_hit, int32_t* best_idx, float* best_prob, void* stream);

/* ------------------------------------------------------------------------------------------
 * Core-set clip selection: greedy k-center in a feature space, weighted by a score (HUAL_ABI_VERSION unchanged: three new symbols,
 * nothing else moved).  Every launch above sharpens WHAT a clip is asked; this family decides WHICH clips are asked, as a set: a
 * top half by score may spend a round on near-duplicate clips of a few hard videos, greedy k-center spreads it over the feature
 * space.
 *
 * hual_clip_mean_features: one descriptor per video of a resident feature bank (hual_dataset's feat_bank f32 [frames, vdim] and
 * feat_off i64 [V + 1]: the frames of video v are the rows feat_off[v] .. feat_off[v + 1]).  out f32 [V, vdim] with row stride ld_out
 * >= vdim: the mean over the video's frames, a column's frames added in float32 in ascending frame order and divided by the count
 * (a video without frames: a zero row); with normalize != 0 every row is then divided by its L2 norm (summed in float64), a zero row
 * stays zero.  One workgroup per video, the bank read exactly once with loads coalesced along vdim; a fixed order, no atomics: a
 * second launch returns equal bits.  Argument errors (a null pointer, V < 1, vdim outside [1, 4096], ld_out < vdim) return
 * HUAL_ERR_INVALID before any HIP call. */
int hual_clip_mean_features(const float* feat_bank, const int64_t* feat_off, int V, int vdim, int normalize, float* out, int ld_out,
                            void* stream);

/* hual_kcenter_greedy: n_select picks among the N rows of x, all enqueued on `stream` by this one call, no host synchronisation
 * between the steps.
 * Inputs: x f32 [N, D] with row stride ld >= D, 1 <= D <= 4096; weight f32 [N] or NULL (every weight 1); init i32 [n_init] ON THE
 * DEVICE, rows that are centers before the first pick (n_init == 0: may be NULL); 0 <= n_select <= N; workspace: caller-owned,
 * 16-byte aligned, at least hual_kcenter_workspace_bytes(N) bytes, contents irrelevant on entry.
 * Outputs: picked i32 [n_select], pick_dist f32 [n_select], mind f32 [N], assign i32 [N].
 *  - Distance: d(i, c) = sum_k (x[i,k] - x[c,k])^2 in float32.  The columns are dealt to the 64 lanes of one wave in chunks of four
 *    (chunk k / 4 to lane (k / 4) % 64, ascending) and the lanes' sums are folded by one butterfly: the order depends on D alone, not
 *    on where row i sits in the grid, so two bit-equal rows get bit-equal distances to every center.
 *  - State: mind[i] is the minimum of d(i, c) over the centers so far - the init rows in their order, then the picks -, +inf while
 *    there is none; assign[i] is the ROW INDEX of the first center in that order that attains it (a strictly smaller distance
 *    replaces), -1 while there is none.  A NaN distance makes mind[i] NaN and leaves assign[i].
 *  - Eligibility: a row is eligible when it is not in init, has not been picked, its weight is >= 0 (a negative or NaN weight means
 *    "never ask"), its score is not NaN, and all its features are finite (d(i, i) == 0: a row that holds a NaN or an infinity is
 *    never picked, also while there is no center, and changes no other row's state).
 *  - Step s: score[i] = w[i] * mind[i]; while there is no center, score[i] = w[i].  The pick is the eligible row of maximal (score,
 *    w, -i) in lexicographic order: the largest score, then the larger weight, then the lower index.  Duplicate descriptors give
 *    exact zeros and exact ties, and the second key then sends the ask to the row the ranking prefers.
 *  - picked[s] is that row, pick_dist[s] its mind before the pick (+inf for a first pick without centers).  When no eligible row is
 *    left, picked[s] = -1 and pick_dist[s] = -1.0f for this and every later step.
 *  - On return mind and assign account for every center, the last pick included.
 * n_select == 0 returns at once: nothing is launched and nothing is written.
 * Launches: an opening launch (the state, and the finite test of every row), one update-only launch per init row, one launch per
 * step and one closing update - 2 + n_init + n_select in all, each over ceil(N / 16) workgroups.  A step stages the newest center's
 * row in LDS, updates the rows it owns (one wave per row), reduces their keys to one partial per workgroup, publishes it with an
 * agent-scope release and draws a ticket from a device-scope counter; the workgroup that draws the last ticket reduces the partials
 * behind an agent-scope acquire, writes picked[s] / pick_dist[s], marks the row taken and returns the counter to zero.  No workgroup
 * ever waits for another one: nothing polls, no grid barrier, no cooperative launch.  The keys are a total order, so the pick does
 * not depend on arrival order: a second call returns equal bits.  Every index read from device memory (picked[s - 1], init[j]) is
 * range-checked in the kernel before it becomes a row number: outside [0, N) - the -1 of an exhausted selection - the update is a
 * no-op.  Allocates nothing and does not synchronise: capturable in a hipGraph.  Argument errors (a null pointer other than weight,
 * and init with n_init == 0; N < 1; D outside [1, 4096]; ld < D; n_select outside [0, N]; n_init outside [0, N]; a workspace that is
 * too small or misaligned) return HUAL_ERR_INVALID before any HIP call. */
uint64_t hual_kcenter_workspace_bytes(int N);
int hual_kcenter_greedy(const float* x, int N, int D, int ld, const float* weight, const int32_t* init, int n_init, int n_select,
                        int32_t* picked, float* pick_dist, float* mind, int32_t* assign, void* workspace, uint64_t workspace_bytes,
                        void* stream);

/* hual_kcenter_sample: hual_kcenter_greedy's selection with two switches (HUAL_ABI_VERSION unchanged: one new symbol).  The same
 * arguments, outputs, workspace, launch count, eligibility rules and kernels (csrc/kcenter.h, templated on the switches; with
 * sample == 0 and origin == 0 the call returns hual_kcenter_greedy's bits).
 *  - origin != 0: the zero vector is a center before the first pick.  The opening launch writes mind[i] = |x_i|^2 in the distance
 *    routine's own order, so it equals d(i, 0) bit for bit; assign[i] = -1 means "the origin"; a center exists from step 0 on, so
 *    the first score is w[i] * |x_i|^2.  Over gradient embeddings the greedy first pick is then the row of largest gradient.
 *  - sample != 0: D^2 sampling (k-means++ seeding; BADGE, Ash et al. 2020).  The score of row i at step s is (w[i] * mind[i]) / E(i, s),
 *    w[i] / E(i, s) while there is no center: one float32 product, one correctly rounded float32 division.  E(i, s) =
 *    float32(-ln((k + 0.5) * 2^-24)), the logarithm evaluated in float64, k the top 24 bits of word x of Philox4x32-7 at counter
 *    (c0 = s, c1 = i, c2 = HUAL_SITE_SELECT, c3 = offset) under the key (seed low word, seed high word).  The E are independent unit
 *    exponentials (on a 2^24 grid), and the argmax of m_i / E_i is a draw with probability m_i / sum m: the pick is a draw
 *    proportional to w * mind.  The key stays the total order (score, w, -i): a row with w * mind == 0 - a duplicate of a center -
 *    scores an exact zero, has probability 0 and is taken only when nothing else is left, in (w, -i) order.  pick_dist is the
 *    row's mind, as in the greedy call.  The draws depend on (seed, offset, s, i) alone: arrival order and the ticket change nothing,
 *    and a second call or a graph replay with the same seed returns equal bits. */
int hual_kcenter_sample(const float* x, int N, int D, int ld, const float* weight, const int32_t* init, int n_init, int n_select,
                        uint64_t seed, uint32_t offset, int sample, int origin, int32_t* picked, float* pick_dist, float* mind,
                        int32_t* assign, void* workspace, uint64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient embeddings for batch-mode acquisition (HUAL_ABI_VERSION unchanged: one new symbol).  The descriptor space of
 * hual_clip_mean_features never saw the model; BADGE (Ash et al., ICLR 2020) describes a sample by the gradient of its loss with
 * respect to the last layer under the model's own hypothesised label.  For SeqPAN that layer is start_dense / end_dense, Dense(1) on
 * the hidden rows head.hs / head.he, under a softmax cross entropy: g_s = sum_t (p_s(t) - y_s(t)) h_s(t) in R^128, likewise g_e.
 *
 * hual_al_grad_embed: one launch, one 256-thread workgroup per sample of a batch, after a label-free forward.
 * Inputs: hs, he f32 [B * T, 128] (the forward's head.hs / head.he, row b * T + t); s_logits, e_logits f32 [B, ld]; v_len i32 [B];
 * hyp i32 [B, 2], the hypothesised (start, end) frame; rows i32 [B] or NULL, the bank row of sample b (NULL: b; an id outside [0, N)
 * writes nothing; two samples of one launch must not name one row); 1 <= T <= 256 (the forward's own limit), T <= ld <= 1024.
 * Outputs, banks over the whole set: desc f32 [N, ld_desc >= 256], columns 0..127 g_s and 128..255 g_e (columns beyond 255 are not
 * written); gnorm2 f32 [N] = |g_s|^2 + |g_e|^2; egl f32 [N] = sum over the two heads of sum_t p(t) |h(t) - mu|^2, mu = sum_t p(t)
 * h(t): the expectation of |g|^2 over y ~ p (the expected gradient length).
 *  - v = v_len[b] clamped to [0, T]; p_s, p_e are the span family's masked softmax over the first v frames (hual_span_argmax's
 *    numbers, bit for bit); y is one-hot at hyp.  A hyp entry outside [0, v) means "no label for this head": g = mu, the expected
 *    feature, so a caller that wants egl alone needs no hypothesis.
 *  - mu and g are accumulated in float32 in ascending t, one fused multiply-add per frame (the weight of the hypothesised frame is
 *    float32(p - 1)).  egl is a second pass over float32(h - mu), squared, weighted and added in float64 in ascending t - never
 *    E|h|^2 - |mu|^2.  The 256 columns' squares (gnorm2) and sums (egl) are added in float64 in a fixed order.
 *  - A row with v < 1 or a non-finite logit among its v frames gets NaN in its 256 descriptor columns - hual_kcenter_* never picks
 *    such a row and lets it move no other row - and -1.0f in gnorm2 and egl.
 * No atomics, nothing grid wide: a second launch returns equal bits.  Allocates nothing and does not synchronise: capturable.
 * Argument errors (a null pointer other than rows; B < 1; N < 1; T outside [1, 256]; ld outside [T, 1024]; ld_desc < 256) return
 * HUAL_ERR_INVALID before any HIP call. */
int hual_al_grad_embed(const float* hs, const float* he, const float* s_logits, const float* e_logits, const int32_t* v_len,
                       const int32_t* hyp, const int32_t* rows, int B, int T, int ld, int N, float* desc, int ld_desc, float* gnorm2,
                       float* egl, void* stream);

/* ------------------------------------------------------------------------------------------
 * Measurement hook for bench.py's roofline leg (not part of the reference's surface): between begin and end every
 * kernel launch carries its own start / stop events (hipExtLaunchKernelGGL: the begin / end timestamps of that
 * kernel's dispatch, the quantity rocprofv3 --kernel-trace reports).  hual_prof_end() synchronises those events (the
 * only synchronising call in the library), aggregates per kernel symbol and returns the number of distinct kernels;
 * hual_prof_get(i, ...) reads entry i: kernel name, launches, microseconds, algorithmic FLOPs and bytes. */
int hual_prof_begin(void);
int hual_prof_end(void);
int hual_prof_get(int i, char* name, int name_cap, int64_t* launches, double* usec, double* flops, double* bytes);
/* the matrix pipe kernel `kernel` (a name hual_prof_get returned) runs its products on, and the MFMA passes one algorithmic
 * product costs there (split operands: 3) - what a TFLOP/s figure of that kernel has to be priced against */
#define HUAL_PIPE_NONE 0       /* no matrix instructions */
#define HUAL_PIPE_MATRIX32 1   /* v_mfma_f32_*_f32: 157.3 TFLOP/s dense peak */
#define HUAL_PIPE_MATRIX16 2   /* v_mfma_f32_*_{f16,bf16}: 2516.8 TFLOP/s dense peak */
int hual_prof_kernel_pipe(const char* kernel, int* pipe, int* passes);

#ifdef __cplusplus
}
#endif
#endif /* HUAL_SEQPAN_H */
