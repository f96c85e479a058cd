/*
 * newsreclib_amd.h -- C ABI of the MI355X (gfx950) NRMS hot path.
 *
 * This is the drop-in boundary under the reference's operator API (plug point 3):
 * the Python modules `news_encoder` / `user_encoder` / `click_predictor` of
 * `newsreclib_amd.nrms_module.NRMSModule` call these entry points through ctypes
 * (newsreclib_amd/_lib.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - C linkage, plain pointers and sizes; no C++ or torch types cross the boundary.
 *   - every pointer except NrlBlockParams/NrlBlockGrads structs themselves is a DEVICE pointer on
 *     the current device; the caller (PyTorch's caching allocator) owns every buffer incl. the
 *     workspace; the library never allocates device memory and never synchronises.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it.
 *   - return value 0 = success, negative = error (NRL_E_*); nrl_last_error() returns a
 *     thread-local message.  Nothing throws.
 *   - all floating point is IEEE fp32 ("dtype": "f32"); token ids / offsets are int64.
 *   - reference citations are relative to andreeaiana/newsreclib.
 */
#ifndef NEWSRECLIB_AMD_H
#define NEWSRECLIB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRL_ABI_VERSION 19

#define NRL_OK 0
#define NRL_E_INVALID (-1)   /* bad argument (shape / alignment / null) */
#define NRL_E_WORKSPACE (-2) /* workspace too small */
#define NRL_E_HIP (-3)       /* a HIP runtime call failed */
/* Every entry point that takes a workspace reports a short one the same way: NRL_E_WORKSPACE with the message
 * "workspace too small: <given> < <needed> bytes", before anything is launched; a null or misaligned one is NRL_E_INVALID. */

/* One "multi-head self-attention + additive attention" block.  Field <-> reference state_dict key
 * (prefix `news_encoder.text_encoders.title.` or `user_encoder.`):
 *   in_proj_weight  multihead_attention.in_proj_weight   (3D, D) rows [Wq; Wk; Wv]
 *   in_proj_bias    multihead_attention.in_proj_bias     (3D)
 *   out_proj_weight multihead_attention.out_proj.weight  (D, D)
 *   out_proj_bias   multihead_attention.out_proj.bias    (D)
 *   att_weight      additive_attention.linear.weight     (Q, D)
 *   att_bias        additive_attention.linear.bias       (Q)
 *   att_query       additive_attention.query             (Q)
 * PyTorch Linear layout (out, in) row-major, used in place (no re-layout, no copies).
 * Replaces: nn.MultiheadAttention + AdditiveAttention as wired in text.py:199-220 (MHSAAddAtt)
 * and user/nrms.py:23-30 (UserEncoder). */
typedef struct NrlBlockParams {
  const float* in_proj_weight;
  const float* in_proj_bias;
  const float* out_proj_weight;
  const float* out_proj_bias;
  const float* att_weight;
  const float* att_bias;
  const float* att_query;
  int32_t embed_dim;  /* D, multiple of 4 */
  int32_t num_heads;  /* D / num_heads in {16, 20, 32, 48, 64} */
  int32_t query_dim;  /* Q, multiple of 4 */
  int32_t gemm_engine; /* projection engine of THIS call: 0 = process default (nrl_set_gemm_engine),
                        * 1 = exact fp32, 2 = bf16x3.  A backward must be given the value its forward ran under
                        * (the bf16 weight planes in the workspace exist only under bf16x3). */
  int32_t options;     /* kernel-selection switches of THIS call: 0 = the process defaults (nrl_set_option / NRL_*
                        * environment), otherwise NRL_OPTIONS_EXPLICIT | mask with the bit order of nrl_get_options().  The
                        * switches choose the private formats of the workspace: a backward must be given the word its
                        * forward ran under (a host stores NRL_OPTIONS_EXPLICIT | nrl_get_options() at the forward). */
} NrlBlockParams;
#define NRL_OPTIONS_EXPLICIT 0x40000000

/* Gradient accumulators, same shapes as NrlBlockParams; kernels ADD into them (callers zero
 * them, or pass the persistent .grad / flat DP gradient buffer to accumulate in place). */
typedef struct NrlBlockGrads {
  float* in_proj_weight;
  float* in_proj_bias;
  float* out_proj_weight;
  float* out_proj_bias;
  float* att_weight;
  float* att_bias;
  float* att_query;
} NrlBlockGrads;

int nrl_abi_version(void);
/* 32 hex digits: hash of the sources the library was built from (newsreclib_amd/_build.py source_hash()); a host that has
 * the sources beside the library compares the two instead of trusting file times. */
const char* nrl_build_id(void);
const char* nrl_last_error(void);

/* ---- projection GEMM engine: the process DEFAULT, used by calls whose params carry gemm_engine == 0 and by the
 * entry points whose params have no such field (the same entry points serve both engines) ------
 *   0 = exact fp32: v_mfma_f32_16x16x4_f32, bitwise an fmaf chain (the reference's arithmetic type)
 *   1 = "bf16x3" (default): fp32 operands split a = hi + lo (two bf16), three bf16 MFMAs per product
 *       (hi*hi + hi*lo + lo*hi) with fp32 accumulation; ~2^-16 relative per product, scores within
 *       1e-4 of the fp32 path (contract 1e-3), ~1.3-2x faster GEMMs.  Attention, softmax, pooling,
 *       loss and Adam are fp32 in both engines. */
/* DEPRECATED as an interface (ABI v16): process-global mutable state, which SURVEY section 8(b) asks the boundary not to have.
 * Hosts set NrlBlockParams.gemm_engine per call (newsreclib_amd/ops.py captures it at every forward and hands it to the
 * backward); the setter stays for A/B scripts, the test fixture that runs the suite under both engines, and the entry points
 * whose params struct has no engine field. */
int nrl_set_gemm_engine(int32_t engine);
int nrl_get_gemm_engine(void);

/* ---- kernel-selection switches for A/B measurements and the equivalence tests.  All paths compute the same function;
 * they differ in the kernels used and in the PRIVATE formats of the workspace.  The switches of a call are
 * NrlBlockParams.options (per call, thread-safe); nrl_set_option changes the process DEFAULTS that options == 0 refers
 * to (the environment variables NRL_<NAME>=0/1 set the same defaults at load time).  Bit order of the mask:
 *   0 "news_fused"      gather + in-projection + token attention of the news encoder in one kernel (bf16x3 engine,
 *                       L <= 32, D = 20 * heads in [288, 316])
 *   1 "news_fused_bwd"  RETIRED (ABI v14): reserved, always 0 -- nrl_set_option(.., 1) and an options word with the bit set are
 *                       rejected.  (q|k|v recomputed inside the attention backward: measured slower, kernel in tools/experimental/)
 *   2 "news_attn_mfma"  token-attention backward of the fused news path on the matrix cores from head-major q|k|v slabs
 *   3 "news_planes"     x / dqkv of that path as pre-split bf16 fragment-block planes (DMA-only weight gradient)
 *   4 "news_od_planes"  o / dy of that path as planes too
 *   5 "news_aa_planes"  y and d_pre as planes for the additive-attention GEMMs
 *   6 "wgrad_2step"     split-K partial tiles stored and reduced in a second kernel instead of atomics
 *   7 "wgrad_ws"        wave-specialised kernel for the 900-row weight gradient
 *   8 "rowpanel"        row-panel kernel for the N <= 320 projections
 *   9 "x3_dma"          LDS-DMA staged tiled GEMMs
 *  10 "news_tail"       out-projection + dropout + additive attention + pooling of the fused news path in ONE kernel
 *  11 "news_tail_bwd"   additive-attention backward of that path in ONE kernel that recomputes tanh from the y planes
 *  12 "user_fork"       (default OFF, measured slower) user-encoder backward: the in-projection dgrad and the three weight gradients side by side on two
 *                       library-internal streams (forked from and joined back into the caller's stream inside the call)
 *  13 "news_fork"       (default ON since ABI v16; off before) news-encoder backward: the additive-attention and out-projection weight gradients on a
 *                       library-internal stream beside the activation-gradient chain of phase 1 (forked after the tail
 *                       backward, joined before the phase-1 call returns; a phase-2 call then runs only the in-projection one)
 *  14 "news_qkv_planes" token-attention backward of the fused news path: q|k|v / d_o split once into (hi, lo) bf16 planes in LDS, operand
 *                       fragments read from them (bit-identical to the kernel that builds each fragment from fp32)
 *  15 "news_pad_share"  (ABI v13) evaluation forward of the fused news path (nothing saved, p_drop == 0): the run of padding tokens
 *                       from token 15 on is ONE row (identical embedding row, no dropout), so a news whose tokens 15 .. L - 1 are
 *                       all the padding id is computed on its first 16 token rows only; bit-identical to computing every row
 *  16 "news_tail_od"    RETIRED (ABI v14): reserved, always 0 (the out-projection's activation gradient inside the fused tail backward:
 *                       measured slower, code in tools/experimental/)
 *  17 "user_proj"       (ABI v13) the NRMS user encoder's in-projection inside its across-users attention kernel (bf16x3 engine,
 *                       32 <= users <= 128 per call, D = 20 * heads in [288, 316]) instead of a separate GEMM launch
 * Entry points whose params struct has no `options` field run under the process defaults: their forward and backward
 * must see the same defaults (newsreclib_amd/ops*.py compare nrl_get_options() at both). */
/* DEPRECATED as an interface (ABI v16), for the same reason as nrl_set_gemm_engine: per-call NrlBlockParams.options is the
 * path; the setter stays for A/B measurement scripts and equivalence tests. */
int nrl_set_option(const char* name, int32_t value);
/* Bit mask of the process-default switch values (bit order above). */
int32_t nrl_get_options(void);

/* ---- measurement hook (bench.py "roofline"): HIP-event timing of the dominant kernel of the step, recorded on the launch
 * stream.  The ProfScope wraps the news-encoder forward's first launch only: under the default bf16x3 engine the fused
 * kernel (embedding gather + dropout + in-projection + per-head token attention, nrl_news_fused.h), counted as
 * 2*M*3D*D + 4*M*L*D FLOPs per launch; under the exact-fp32 engine the in-projection GEMM with the fused gather,
 * 2*M*3D*D.  Diagnostic state, process-wide: enable it around a measurement pass, not in a timed region. */
int nrl_prof_enable(int32_t on);
int nrl_prof_read(double* total_ms, int64_t* launches, double* total_flops);

/* ---- dropout keep-mask specification (normative statement: oracle/nrms_oracle.py) ----------
 * keep(i) = lowbias32(i * 0x9E3779B1 + key) >= floor(p * 2^32), i = row * D + col (32-bit).
 * Replaces nn.Dropout at text.py:220,225,230 (torch's RNG stream is not reproducible on device). */
uint32_t nrl_dropout_key(uint64_t seed, uint32_t stream);
int nrl_dropout_mask(uint8_t* keep, int64_t n_elems, double p, uint64_t seed, uint32_t stream,
                     void* stream_handle);

/* ---- token-id grouping for the embedding-table gradient (embedding_dense_backward, text.py:215-217,224) -----
 * order (n + 1) int64 <- order[0 .. n): the positions 0..n-1 of the flat id vector grouped by ASCENDING id (counting sort
 * over the vocabulary: LDS-merged histogram, scan, scatter; ids must lie in [0, vocab), vocab <= 2^20; the order inside
 * one id's run is unspecified); order[n]: the number of positions whose id is 0 -- they come first, so order[order[n] .. n)
 * lists the LIVE positions (the padding id's embedding row has no gradient).  This is the `sorted_positions` argument of
 * the *_encoder_bwd entry points; nrl_news_encoder_bwd reads the count too (ABI v11: it computes the gradient of the
 * gathered rows for the live positions only), so a host that sorts by other means appends it. */
size_t nrl_sort_positions_workspace_bytes(int64_t n, int64_t vocab);
int nrl_sort_positions(const int64_t* ids, int64_t n, int64_t vocab, int64_t* order, void* ws, size_t ws_bytes,
                       void* stream);

/* ---- news encoder: MHSAAddAtt.forward, text.py:222-236 (behind NewsEncoder.forward,
 * news.py:134-160) ------------------------------------------------------------------------------
 * ids (N, L) int64 -> out (N, D).  Embedding gather (bit-exact; id 0 is an ordinary row,
 * text.py:215-217) fused into the in-projection GEMM's A-tile loader; dropout stream `stream0`
 * after the gather and `stream0 + 1` after the attention out-projection when p_drop > 0.
 * `save_for_backward` != 0 keeps activations in `ws` for nrl_news_encoder_bwd. */
size_t nrl_news_encoder_workspace_bytes(int64_t n_news, int32_t seq_len, int32_t embed_dim,
                                        int32_t num_heads, int32_t query_dim);
int nrl_news_encoder_fwd(const NrlBlockParams* p, const float* emb_table, int64_t vocab,
                         const int64_t* ids, int64_t n_news, int32_t seq_len, double p_drop,
                         uint64_t seed, uint32_t stream0, int32_t save_for_backward, float* out,
                         void* ws, size_t ws_bytes, void* stream);
/* ---- evaluation forwards from a per-token q|k|v table (ABI v16) --------------------------------------------------
 * Validation / test re-encode every news of every impression under FROZEN weights (rec_dataset.py:98-121,
 * nrms_module.py:398-535), and without dropout the q|k|v rows of a token position depend on its token id alone
 * (text.py:224,229).  nrl_token_table_build runs the in-projection ONCE per vocabulary id -- plus the weight images the
 * back half needs -- into a caller-owned buffer; nrl_news_encoder_fwd_table is MHSAAddAtt.forward (text.py:222-236,
 * evaluation mode) from it: ids (N, L) -> out (N, D), the per-head 32 x 64 q|k|v image gathered by token id instead of
 * computed.  A table row holds the bits the projection of nrl_news_encoder_fwd produces for that id, so `out` is EQUAL
 * (torch.equal) to that call's with p_drop = 0, save_for_backward = 0.  The buffer is valid for exactly the parameter values
 * (embedding table, in/out projection, additive-attention linear) it was built from: the CALLER rebuilds it after any
 * update; `att_query` is read from `p` at every call.  bf16x3 engine, fused-news-encoder geometry only
 * (nrl_token_table_supported; D = 300, 15 heads, L <= 32, Q <= 208); nrl_token_table_bytes returns 0 outside it. */
int32_t nrl_token_table_supported(int32_t seq_len, int32_t embed_dim, int32_t num_heads, int32_t query_dim);
size_t nrl_token_table_bytes(int64_t vocab, int32_t embed_dim, int32_t num_heads, int32_t query_dim);
int nrl_token_table_build(const NrlBlockParams* p, const float* emb_table, int64_t vocab, void* table, size_t table_bytes,
                          void* stream);
size_t nrl_news_encoder_fwd_table_workspace_bytes(int64_t n_news, int32_t seq_len, int32_t num_heads);
int nrl_news_encoder_fwd_table(const NrlBlockParams* p, const void* table, size_t table_bytes, int64_t vocab,
                               const int64_t* ids, int64_t n_news, int32_t seq_len, float* out, void* ws, size_t ws_bytes,
                               void* stream);
/* Backward of the above (autograd of text.py:222-236 incl. embedding_dense_backward with
 * padding_idx=0: rows of id 0 receive no gradient).  d_out (N, D).  Adds into `g` and into
 * d_emb_table (vocab, D).  `ws` must be the workspace the forward filled.
 * emb_table: the table the forward read (unchanged since); not read by any current path (the recomputing backward that
 * re-gathered rows from it was retired in ABI v14) -- may be NULL.
 * sorted_positions: optional (may be NULL) output of nrl_sort_positions over the flat (N*L) id vector: N*L + 1 entries,
 * the positions by ascending id and then the number of id-0 positions.  When given, the table gradient is reduced in
 * id-sorted order (one atomic per (id, 64-row segment)) instead of one atomic per element -- frequent tokens otherwise
 * serialise on their row -- and (fused path) the gradient of the gathered rows is computed for the LIVE positions only:
 * the padding id's rows, ~60 % of a MIND title batch, have no table gradient and nothing else reads theirs.
 * phase: 0 = whole backward; 1 = activation-gradient chain + table gradient only; 2 = the three
 * weight/bias-gradient GEMMs only (call 1 then 2: a data-parallel caller starts the all-reduce of the
 * table gradient, >96 % of the bytes, between them so it overlaps the weight-gradient GEMMs). */
int nrl_news_encoder_bwd(const NrlBlockParams* p, const NrlBlockGrads* g, const float* emb_table,
                         float* d_emb_table, int64_t vocab, const int64_t* ids, const int64_t* sorted_positions,
                         int64_t n_news, int32_t seq_len, double p_drop, uint64_t seed,
                         uint32_t stream0, const float* d_out, int32_t phase, void* ws,
                         size_t ws_bytes, void* stream);

/* ---- user encoder: nrms UserEncoder.forward, user/nrms.py:32-41 --------------------------------
 * hist (B, H, D) -> out (B, D).  Reproduces the reference's seq-first nn.MultiheadAttention call:
 * attention runs across the B rows of dim 0 for each slot of dim 1 (SURVEY.md headline fact 3), then
 * additive attention pools over dim 1.  With p_drop > 0 a dropout (stream0) is applied to the input
 * and another (stream0 + 1) between attention and pooling: that is exactly the tail of the PLM text
 * encoder, PLM.forward text.py:92-99, called with hist = last_hidden_state (N_news, L, D).
 * input_dropout = 0 applies only the second one: the long-term branch of the CenNewsRec user encoder
 * (user/cen_news_rec.py:66-72). */
size_t nrl_user_encoder_workspace_bytes(int64_t batch, int64_t hist_len, int32_t embed_dim,
                                        int32_t num_heads, int32_t query_dim);
int nrl_user_encoder_fwd(const NrlBlockParams* p, const float* hist, int64_t batch,
                         int64_t hist_len, double p_drop, uint64_t seed, uint32_t stream0,
                         int32_t input_dropout, int32_t save_for_backward, float* out, void* ws,
                         size_t ws_bytes, void* stream);
int nrl_user_encoder_bwd(const NrlBlockParams* p, const NrlBlockGrads* g, const float* hist,
                         int64_t batch, int64_t hist_len, double p_drop, uint64_t seed,
                         uint32_t stream0, int32_t input_dropout, const float* d_out, float* d_hist,
                         void* ws, size_t ws_bytes, void* stream);
/* The same backward in two parts (ABI v12).  phase 1: everything up to d_hist (and the additive-attention query gradient);
 * phase 2: the three weight gradients, which only read what phase 1 left in `ws` (d_out / d_hist are not touched and may be
 * NULL) -- they are off the path into the news-encoder backward, so a caller may issue them on another stream, ordered after
 * phase 1, and join before the optimizer; phase 0 = nrl_user_encoder_bwd. */
int nrl_user_encoder_bwd_phase(const NrlBlockParams* p, const NrlBlockGrads* g, const float* hist,
                               int64_t batch, int64_t hist_len, double p_drop, uint64_t seed,
                               uint32_t stream0, int32_t input_dropout, const float* d_out,
                               float* d_hist, int32_t phase, void* ws, size_t ws_bytes, void* stream);

/* ---- to_dense_batch (torch_geometric 2.3.0; call sites nrms_module.py:233,237,277-284) ---------
 * x (N, D) + offsets (B+1) int64 (prefix sums of the sorted assignment vector) ->
 * dense (B, max_len, D), zero-filled past each group's length.  _bwd is the adjoint gather. */
int nrl_to_dense_batch_fwd(const float* x, const int64_t* offsets, int64_t batch, int64_t max_len,
                           int32_t dim, float* dense, void* stream);
int nrl_to_dense_batch_bwd(const float* d_dense, const int64_t* offsets, int64_t batch,
                           int64_t max_len, int32_t dim, int64_t n_rows, float* d_x, void* stream);

/* ---- late fusion (late_fusion=True): user vector = mean of the clicked-news vectors, nrms_module.py:243-248 /
 * lstur_module.py:295-296: hist (B, max_len, D) zero-padded dense history, offsets (B+1) as above ->
 * user[b] = sum_h hist[b, h] / (offsets[b+1] - offsets[b]).  _bwd writes d_hist (B, max_len, D). */
int nrl_hist_mean_fwd(const float* hist, const int64_t* offsets, int64_t batch, int64_t max_len,
                      int32_t dim, float* user, void* stream);
int nrl_hist_mean_bwd(const float* d_user, const int64_t* offsets, int64_t batch, int64_t max_len,
                      int32_t dim, float* d_hist, void* stream);

/* ---- click predictor: DotProduct.forward, click_predictor.py:9-11 as called at
 * nrms_module.py:251-253: user (B, D), cand (B, C, D) -> scores (B, C) -------------------------- */
int nrl_dot_scores_fwd(const float* user, const float* cand, int64_t batch, int64_t n_cand,
                       int32_t dim, float* scores, void* stream);
int nrl_dot_scores_bwd(const float* d_scores, const float* user, const float* cand, int64_t batch,
                       int64_t n_cand, int32_t dim, float* d_user, float* d_cand, void* stream);

/* ---- loss: CrossEntropyLoss()(scores, y_true) with float targets, nrms_module.py:287-288 --------
 * loss = mean_b(-sum_c y * log_softmax(scores)_c); also writes d_scores = grad_scale * dloss/dscores
 * (pass grad_scale = 1 for plain backward, 1/world_size to pre-average for data parallel). */
int nrl_ce_loss_fwd_bwd(const float* scores, const float* y_true, int64_t batch, int64_t n_cand,
                        float grad_scale, float* loss, float* d_scores, void* stream);

/* ---- loss: SupConLoss over the score matrix, losses.py:6-40 as called at nrms_module.py:289-318 (on
 * pytorch-metric-learning 2.2.0: GenericPairLoss.mat_based_loss, AvgNonZeroReducer).  Row b: positives = slots
 * with y_true != 0, negatives = its other real candidates (slot < cand_sizes[b]); x = scores / temperature;
 * loss_b = -mean_p(x_p - logsumexp over the row's real candidates); loss = mean of the loss_b > 0 (0 when the
 * batch holds no positive or no negative pair).  Also writes d_scores = grad_scale * dloss/dscores (may be NULL). */
int nrl_supcon_loss_fwd_bwd(const float* scores, const float* y_true, const int64_t* cand_sizes, int64_t batch,
                            int64_t n_cand, float temperature, float grad_scale, float* loss, float* d_scores,
                            void* stream);

/* ---- optimizer: torch.optim.Adam(lr) dense step over a flat buffer, configs/model/nrms.yaml:49-52,
 * abstract_recommender.py:96.  `step` is the 1-based step count.  grad_scale multiplies g first
 * (1/world_size after a sum all-reduce).  zero_grad != 0 clears g after use. */
int nrl_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  double lr, double beta1, double beta2, double eps, int64_t step, float grad_scale,
                  int32_t zero_grad, void* stream);

/* ---- optimizer, lazy form for the embedding table (ABI v13).  Same arithmetic, same bits as nrl_adam_step: a row whose
 * gradient is zero evolves by a deterministic fp32 recurrence in (p, m, v, step), so its update may be applied later -- before
 * the row is next gathered, when it next receives a gradient, or when the state is exported.  `last_step[rows]` (int32, zeros
 * at step 0) records how far each row has been advanced; `mark[rows]` (int32) names the rows a step touches; `status[1]` is set
 * to 1 if a row was found more than 127 steps behind (the window of bias corrections a call carries) -- the caller's rolling
 * flush must keep every lag below that.
 *   nrl_adam_rows_mark     mark[id] = step for every id of the step's batch (ids outside [0, rows) are ignored)
 *   nrl_adam_rows_advance  candidate rows r = offset + j * stride (< rows); with `mark`: only those with mark[r] == upto_step + 1.
 *                          Each is advanced from last_step[r] to upto_step with zero gradients; with_grad != 0: then step
 *                          upto_step + 1 is applied with its gradient row (times grad_scale), the gradient row is cleared and
 *                          last_step[r] = upto_step + 1.  (catch-up before a forward: mark, upto_step = t - 1, with_grad 0;
 *                          update after the backward: mark, upto_step = t - 1, with_grad 1; flush: mark NULL, with_grad 0;
 *                          with_grad 2, mark NULL: "scan" -- every candidate row whose gradient row has a non-zero element is
 *                          updated, all-zero rows stay lazy: the update after a DENSE all-reduce, which leaves no list of rows.)
 *                          exclude_mark (ABI v14; NULL: none): rows with exclude_mark[r] == exclude_tag are skipped -- the EARLY
 *                          catch-up of step t + 1 (mark = the next batch's marks, upto_step = t, with_grad 0) issued on another
 *                          stream while step t runs must leave alone the rows step t owns (exclude_mark = step t's marks,
 *                          exclude_tag = t).  One rank only: a row outside step t's batch has a zero gradient at step t. */
int nrl_adam_rows_mark(const int64_t* ids, int64_t n_ids, int64_t rows, int32_t* mark, int64_t step, void* stream);
int nrl_adam_rows_advance(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t rows, int32_t dim,
                          int32_t* last_step, const int32_t* mark, int32_t* status, int64_t stride, int64_t offset,
                          int64_t upto_step, int32_t with_grad, double lr, double beta1, double beta2, double eps,
                          float grad_scale, const int32_t* exclude_mark, int32_t exclude_tag, void* stream);

/* ---- transformer-body glue (ABI v13; config 4, text.py:89-109: every layer of the PLM body ends its attention and its
 * feed-forward block with LayerNorm(dropout(dense_out) + residual)).  One launch each way instead of dropout + add + layer norm:
 *   fwd: z = x * keep / (1 - p) + residual;  y = (z - mean) * rstd * gamma + beta.  z_save / mean_save / rstd_save: all three
 *        (training) or all NULL (evaluation).  The keep mask is the library's counter-based one over the element index
 *        row * dim + col (seed, stream0), so the backward re-evaluates it instead of reading a stored mask.
 *   bwd: d_residual = LayerNorm backward of d_y; d_x = d_residual * keep / (1 - p) (d_x may be NULL when p_drop == 0: the two
 *        are equal); d_gamma / d_beta (both or neither; NULL for a frozen LayerNorm) are ACCUMULATED.
 * dim % 4 == 0, dim <= 2048, rows * dim < 2^32. */
int nrl_dropout_add_layernorm_fwd(const float* x, const float* residual, const float* gamma, const float* beta, int64_t rows,
                                  int32_t dim, float eps, double p_drop, uint64_t seed, uint32_t stream0, float* z_save,
                                  float* mean_save, float* rstd_save, float* y, void* stream);
int nrl_dropout_add_layernorm_bwd(const float* d_y, const float* z_saved, const float* gamma, const float* mean_saved,
                                  const float* rstd_saved, int64_t rows, int32_t dim, double p_drop, uint64_t seed,
                                  uint32_t stream0, float* d_x, float* d_residual, float* d_gamma, float* d_beta, void* stream);

/* =================================================================================================
 * LSTUR path (BASELINE config 5): CNN text encoder, row-masked embedding
 * lookups (category / long-term user vector) and the GRU user encoder.
 * ================================================================================================= */

/* CNN + additive-attention text encoder.  Field <-> reference state_dict key (prefix
 * `news_encoder.text_encoders.<attr>.`, ONE module shared by title and abstract, news.py:69-79):
 *   conv_weight  cnn.weight                        (F, 1, W, D) contiguous = (F, W*D), k = t*D + d
 *   conv_bias    cnn.bias                          (F)
 *   att_weight   additive_attention.linear.weight  (Q, F)
 *   att_bias     additive_attention.linear.bias    (Q)
 *   att_query    additive_attention.query          (Q)
 * Replaces nn.Conv2d + F.relu + AdditiveAttention as wired in text.py:146-176 (CNNAddAtt). */
typedef struct NrlCnnParams {
  const float* conv_weight;
  const float* conv_bias;
  const float* att_weight;
  const float* att_bias;
  const float* att_query;
  int32_t embed_dim;   /* D, multiple of 4 */
  int32_t num_filters; /* F, multiple of 4 */
  int32_t window;      /* W, odd, <= 7 (padding (W-1)/2 as text.py:152) */
  int32_t query_dim;   /* Q, multiple of 4 */
} NrlCnnParams;

typedef struct NrlCnnGrads { /* accumulators, kernels ADD */
  float* conv_weight;
  float* conv_bias;
  float* att_weight;
  float* att_bias;
  float* att_query;
} NrlCnnGrads;

/* CNNAddAtt.forward, text.py:163-176: ids (N, L) int64 -> out (N, F).
 * x = dropout(emb[ids]) (stream0, flat index over (N, L, D)); c = dropout(relu(conv(x))) (stream0 + 1,
 * flat index over (N, L, F)); out = additive attention over the L tokens.  The convolution runs as
 * ONE GEMM with K = W*D over overlapping rows of x (no im2col buffer).
 * save_for_backward != 0: the workspace then holds everything nrl_cnn_encoder_bwd reads (including, under the
 * bf16x3 engine at F % 16 == 12, F <= 304, Q <= 224, the (hi, lo) planes of c its additive-attention weight gradient is
 * fed from); a backward after a forward with save_for_backward == 0 is undefined. */
size_t nrl_cnn_encoder_workspace_bytes(int64_t n_news, int32_t seq_len, int32_t embed_dim,
                                       int32_t num_filters, int32_t window, int32_t query_dim);
int nrl_cnn_encoder_fwd(const NrlCnnParams* p, const float* emb_table, int64_t vocab,
                        const int64_t* ids, int64_t n_news, int32_t seq_len, double p_drop,
                        uint64_t seed, uint32_t stream0, int32_t save_for_backward, float* out,
                        void* ws, size_t ws_bytes, void* stream);
/* Backward (autograd of text.py:163-176 incl. embedding_dense_backward, padding_idx = 0).  d_out (N, F).
 * Adds into `g` and d_emb_table.  sorted_positions as in nrl_news_encoder_bwd (may be NULL; N*L + 1 entries: the
 * count of id-0 positions in the last one -- the convolution's activation gradient runs over the live positions only). */
int nrl_cnn_encoder_bwd(const NrlCnnParams* p, const NrlCnnGrads* g, float* d_emb_table,
                        int64_t vocab, const int64_t* ids, const int64_t* sorted_positions,
                        int64_t n_news, int32_t seq_len, double p_drop, uint64_t seed,
                        uint32_t stream0, const float* d_out, void* ws, size_t ws_bytes,
                        void* stream);

/* CNNMHSAAddAtt.forward, text.py:291-309 (CenNewsRec): ids (N, L) -> out (N, F).
 *   x = dropout(emb[ids]) (stream0); c = dropout(relu(conv1d(x))) (stream0 + 1, padding (W-1)/2);
 *   self-attention over the L tokens of each news on the F conv features, dropout (stream0 + 2), additive
 *   attention.  `cp` supplies conv_weight / conv_bias and the dims (its att_* fields are ignored); conv_weight
 *   in the (F, W*D) layout of NrlCnnParams (k = t*D + d; nn.Conv1d stores (F, D, W): permute on the host);
 *   `bp` is the attention block on embed_dim = F. */
size_t nrl_cnn_mhsa_encoder_workspace_bytes(int64_t n_news, int32_t seq_len, int32_t embed_dim,
                                            int32_t num_filters, int32_t window, int32_t num_heads,
                                            int32_t query_dim);
int nrl_cnn_mhsa_encoder_fwd(const NrlCnnParams* cp, const NrlBlockParams* bp, const float* emb_table,
                             int64_t vocab, const int64_t* ids, int64_t n_news, int32_t seq_len,
                             double p_drop, uint64_t seed, uint32_t stream0, int32_t save_for_backward,
                             float* out, void* ws, size_t ws_bytes, void* stream);
int nrl_cnn_mhsa_encoder_bwd(const NrlCnnParams* cp, const NrlCnnGrads* cg, const NrlBlockParams* bp,
                             const NrlBlockGrads* bg, float* d_emb_table, int64_t vocab,
                             const int64_t* ids, const int64_t* sorted_positions, int64_t n_news,
                             int32_t seq_len, double p_drop, uint64_t seed, uint32_t stream0,
                             const float* d_out, void* ws, size_t ws_bytes, void* stream);

/* nn.Embedding(padding_idx=0) lookup followed by a ROW mask: out[i] = table[ids[i]] * m(i),
 * m(i) in {0, 1/(1-p)} from dropout stream `stream_id` with flat index i (whole rows dropped).
 * p_row = 0: plain lookup = LinearEncoder.forward, category.py:72-73.  p_row > 0: the long-term user
 * vector of LSTUR, user/lstur.py:70-71 (nn.Dropout2d on a (1, B, D) tensor drops whole users).
 * _bwd adds d_out[i] * m(i) into d_table[ids[i]], skipping id 0 (padding_idx). */
int nrl_embedding_rows_fwd(const float* table, const int64_t* ids, int64_t n_ids, int32_t dim,
                           double p_row, uint64_t seed, uint32_t stream_id, float* out,
                           void* stream);
int nrl_embedding_rows_bwd(const float* d_out, const int64_t* ids, int64_t n_ids, int32_t dim,
                           double p_row, uint64_t seed, uint32_t stream_id, float* d_table,
                           void* stream);

/* Single-layer nn.GRU.  Field <-> reference state_dict key (prefix `user_encoder.gru.`):
 *   weight_ih  weight_ih_l0 (3*Hd, Din) rows [W_ir; W_iz; W_in]      bias_ih  bias_ih_l0 (3*Hd)
 *   weight_hh  weight_hh_l0 (3*Hd, Hd)  rows [W_hr; W_hz; W_hn]      bias_hh  bias_hh_l0 (3*Hd) */
typedef struct NrlGruParams {
  const float* weight_ih;
  const float* weight_hh;
  const float* bias_ih;
  const float* bias_hh;
  int32_t input_dim;  /* Din, multiple of 4 */
  int32_t hidden_dim; /* Hd, multiple of 4 */
} NrlGruParams;

typedef struct NrlGruGrads { /* accumulators, kernels ADD */
  float* weight_ih;
  float* weight_hh;
  float* bias_ih;
  float* bias_hh;
} NrlGruGrads;

/* gru(pack_padded_sequence(hist, lengths, batch_first=True, enforce_sorted=False), h0)[1], i.e. the
 * hidden state of every sequence after its own last valid step: user/lstur.py:74-83.
 * hist (B, T, Din), lengths (B) int64 in [1, T] (validated by the caller, as pack_padded_sequence
 * does on the host), h0 (B, Hd) or NULL for zeros ("con" variant, lstur.py:85) -> out (B, Hd).
 * The input projection of all steps is one GEMM; the recurrence runs one small GEMM + one gate kernel
 * per step, t = 0 .. T-1, rows with t >= lengths[b] frozen. */
size_t nrl_gru_workspace_bytes(int64_t batch, int64_t max_len, int32_t input_dim, int32_t hidden_dim);
int nrl_gru_fwd(const NrlGruParams* p, const float* hist, const int64_t* lengths, const float* h0,
                int64_t batch, int64_t max_len, int32_t save_for_backward, float* out, void* ws,
                size_t ws_bytes, void* stream);
/* Backward through time.  d_out (B, Hd) -> d_hist (B, T, Din) overwritten, d_h0 (B, Hd) overwritten
 * (may be NULL); adds into `g`. */
int nrl_gru_bwd(const NrlGruParams* p, const NrlGruGrads* g, const float* hist,
                const int64_t* lengths, const float* h0, int64_t batch, int64_t max_len,
                const float* d_out, float* d_hist, float* d_h0, void* ws, size_t ws_bytes,
                void* stream);

/* =================================================================================================
 * Generic blocks of the sibling recommenders (NAML: news-view combination, user encoder, category encoder).
 * ================================================================================================= */

/* AdditiveAttention.forward, layers/attention.py:24-42: y (G, S, D) -> out (G, D),
 *   t = tanh(y W_a^T + b_a); w = softmax_S(t . q_a); out = sum_s w_s y_s   (no mask).
 * Field <-> state_dict key: att_weight linear.weight (Q, D), att_bias linear.bias (Q), att_query query (Q). */
typedef struct NrlAddAttParams {
  const float* att_weight;
  const float* att_bias;
  const float* att_query;
  int32_t dim;       /* D, multiple of 4 */
  int32_t query_dim; /* Q, multiple of 4 */
} NrlAddAttParams;

typedef struct NrlAddAttGrads { /* accumulators, kernels ADD */
  float* att_weight;
  float* att_bias;
  float* att_query;
} NrlAddAttGrads;

size_t nrl_additive_attention_workspace_bytes(int64_t groups, int64_t len, int32_t dim, int32_t query_dim);
int nrl_additive_attention_fwd(const NrlAddAttParams* p, const float* y, int64_t groups, int64_t len,
                               int32_t save_for_backward, float* out, void* ws, size_t ws_bytes,
                               void* stream);
/* d_out (G, D) -> d_y (G, S, D) overwritten; adds into `g`.  `ws` must be the forward's workspace. */
int nrl_additive_attention_bwd(const NrlAddAttParams* p, const NrlAddAttGrads* g, const float* y,
                               int64_t groups, int64_t len, const float* d_out, float* d_y, void* ws,
                               size_t ws_bytes, void* stream);

/* act(A W^T + bias): nn.Linear followed by an activation (0 none, 1 tanh, 2 relu), e.g. the category
 * encoder's F.relu(self.linear(x)), category.py:78-80.  a (M, K), w (N, K), c (M, N); N, K multiples of 4.
 * _bwd: d_c (M, N) -> d_a (M, K) overwritten (may be NULL), d_w / d_bias ADDED; c = the forward output. */
size_t nrl_linear_act_workspace_bytes(int64_t m, int32_t n, int32_t k);
int nrl_linear_act_fwd(const float* a, const float* w, const float* bias, int64_t m, int32_t n, int32_t k,
                       int32_t act, float* c, void* ws, size_t ws_bytes, void* stream);
int nrl_linear_act_bwd(const float* a, const float* w, const float* c, const float* d_c, int64_t m,
                       int32_t n, int32_t k, int32_t act, float* d_a, float* d_w, float* d_bias,
                       void* ws, size_t ws_bytes, void* stream);

/* nn.MultiheadAttention(x, x, x) with batch_first=False on its own (no pooling): x (seq, batch, D) -> out
 * (seq, batch, D), attention over the `seq` axis for every (batch column, head).  Replaces the call at
 * user/mins.py:55-57 (which feeds (B, H, D), so seq = users, batch = history slots -- the NRMS quirk).
 * `scale` multiplies q before q k^T; 0 selects torch's 1/sqrt(D / num_heads).  A caller that zero-pads the
 * heads to a supported head dim (MINS: 50 -> 64) passes the un-padded 1/sqrt(50) here. */
typedef struct NrlMhaParams {
  const float* in_proj_weight;  /* (3D, D) rows [q; k; v] */
  const float* in_proj_bias;    /* (3D) */
  const float* out_proj_weight; /* (D, D) */
  const float* out_proj_bias;   /* (D) */
  int32_t embed_dim;            /* D, multiple of 4; D / num_heads in {16, 20, 32, 48, 64} */
  int32_t num_heads;
  float scale;
  int32_t gemm_engine;          /* as NrlBlockParams.gemm_engine */
} NrlMhaParams;

typedef struct NrlMhaGrads {
  float* in_proj_weight;
  float* in_proj_bias;
  float* out_proj_weight;
  float* out_proj_bias;
} NrlMhaGrads;

size_t nrl_mha_workspace_bytes(int64_t seq, int64_t batch, int32_t embed_dim, int32_t num_heads);
int nrl_mha_fwd(const NrlMhaParams* p, const float* x, int64_t seq, int64_t batch, int32_t save_for_backward,
                float* out, void* ws, size_t ws_bytes, void* stream);
/* d_out (seq, batch, D) -> d_x overwritten; adds into `g`.  `ws` must be the forward's workspace. */
int nrl_mha_bwd(const NrlMhaParams* p, const NrlMhaGrads* g, const float* x, int64_t seq, int64_t batch,
                const float* d_out, float* d_x, void* ws, size_t ws_bytes, void* stream);

/* ---- building blocks exported for unit parity tests and reuse ------------------------------- */
/* nn.Embedding lookup alone (bit-exact), text.py:224. */
int nrl_embedding_gather(const float* table, const int64_t* ids, int64_t n_ids, int32_t dim,
                         float* out, void* stream);
/* ABI v14: nn.Linear fused with the exact GELU of a BERT-family feed-forward block (HF RobertaIntermediate / RobertaOutput inside
 * self.plm_model(**text), text.py:89).  bf16x3 engine, wide side >= 256 (nrl_linear_gelu_supported(n_wide) != 0); workspace and
 * image_ready as nrl_linear_fwd_img / _bwd_img (nrl_linear_workspace_bytes(n, k)).
 *   nrl_linear_gelu_fwd_img    h (m, n) = a W^T + bias (the GELU's input, kept for the backward), g (m, n) = gelu(h) = h Phi(h)
 *   nrl_linear_dgrad_gelu_img  for the projection that CONSUMED g -- c = g W^T (+ bias), W (n, k), g (m, k):
 *                              d_pre (m, k) = (d_c W) * gelu'(pre), i.e. the gradient at the GELU's input straight from the epilogue */
int nrl_linear_gelu_fwd_img(const float* a, const float* w, const float* bias, int64_t m, int32_t n, int32_t k, float* h, float* g,
                            void* ws, size_t ws_bytes, int32_t image_ready, void* stream);
int nrl_linear_dgrad_gelu_img(const float* w, const float* d_c, const float* pre, int64_t m, int32_t n, int32_t k, float* d_pre,
                              void* ws, size_t ws_bytes, int32_t image_ready, void* stream);
int32_t nrl_linear_gelu_supported(int32_t n_wide);
/* ABI v15: the query / key / value projections of a transformer layer (HF RobertaSelfAttention.query / .key / .value inside
 * self.plm_model(**text), text.py:89) -- three nn.Linear (n, k) of ONE input -- as one GEMM each way, and activation gradients that
 * land on a residual stream with the other branch's gradient added in the epilogue.  bf16x3 engine; n and k multiples of 256 with
 * at most 12 column panels (nrl_linear3_supported(n, k) != 0); workspace nrl_linear3_workspace_bytes(n, k), image_ready as in
 * nrl_linear_fwd_img (one image of the three weights per direction).
 *   nrl_linear3_fwd_img       c (3, m, n): c[q] = a (m, k) W_q^T + b_q
 *   nrl_linear3_dgrad_img     d_a (m, k) = add + sum_q d_c[q] W_q, d_c (3, m, n) stacked like c; add (m, k) or NULL
 *   nrl_linear_dgrad_add_img  d_a (m, k) = add + d_c (m, n) W (n, k) (k >= 256; workspace nrl_linear_workspace_bytes(n, k))
 * The weight gradients stay three nrl_linear_bwd_img calls (d_a == NULL). */
int32_t nrl_linear3_supported(int32_t n, int32_t k);
size_t nrl_linear3_workspace_bytes(int32_t n, int32_t k);
int nrl_linear3_fwd_img(const float* a, const float* w0, const float* w1, const float* w2, const float* b0, const float* b1,
                        const float* b2, int64_t m, int32_t n, int32_t k, float* c, void* ws, size_t ws_bytes, int32_t image_ready,
                        void* stream);
int nrl_linear3_dgrad_img(const float* d_c, const float* w0, const float* w1, const float* w2, int64_t m, int32_t n, int32_t k,
                          const float* add, float* d_a, void* ws, size_t ws_bytes, int32_t image_ready, void* stream);
int nrl_linear_dgrad_add_img(const float* d_c, const float* w, int64_t m, int32_t n, int32_t k, const float* add, float* d_a,
                             void* ws, size_t ws_bytes, int32_t image_ready, void* stream);
/* ABI v14: embedding_dense_backward of ANY nn.Embedding (the word / position / token-type tables of the PLM body, text.py:89):
 * d_table[ids[p]] += d_out[p] for the n_ids positions in the id-sorted order `sorted_positions` (nrl_sort_positions: n_ids + 1
 * entries, the last one unused here), one atomic per (id, 64-position segment, element) instead of one per element; the row
 * `padding_idx` (< 0: none) receives nothing (nn.Embedding(padding_idx=...)).  dim <= 1024. */
int nrl_embedding_grad(const float* d_out, const int64_t* ids, const int64_t* sorted_positions, int64_t n_ids, int32_t dim,
                       int64_t padding_idx, float* d_table, void* stream);
/* C(M,N) = A(M,K) * W(N,K)^T + bias  (nn.Linear) through the selected GEMM engine -- the same code path
 * (tile choice, LDS-DMA staging) the encoders' forward projections take.  The bf16x3 engine needs
 * nrl_linear_workspace_bytes(n, k) of workspace for the split weight planes; ws == NULL forces the exact
 * fp32 engine. */
size_t nrl_linear_workspace_bytes(int32_t n, int32_t k);
int nrl_linear_fwd(const float* a, const float* w, const float* bias, int64_t m, int32_t n,
                   int32_t k, float* c, void* ws, size_t ws_bytes, void* stream);
/* Backward of nrl_linear_fwd (nn.Linear inside a third-party stack -- the PLM body of text.py:89-109 -- on this library's
 * matrix-core engines): d_a (m, k) = d_c (m, n) W; d_w (n, k) += d_c^T a; d_bias (n) += colsum(d_c).  d_a == NULL skips
 * the activation gradient; d_w == d_bias == NULL skips the weight gradient (a frozen layer whose input still needs a
 * gradient).  n, k multiples of 4; workspace as nrl_linear_workspace_bytes(n, k) (bf16x3 engine, d_a != NULL). */
int nrl_linear_bwd(const float* a, const float* w, const float* d_c, int64_t m, int32_t n, int32_t k, float* d_a,
                   float* d_w, float* d_bias, void* ws, size_t ws_bytes, void* stream);
/* The same two calls for a weight whose matrix-core images the caller keeps across calls (ABI v12): with image_ready != 0,
 * `ws` already holds the images a previous call of the SAME entry point built for this (w, n, k) under the same engine and
 * switches -- the forward's in one buffer, the backward's (the transposed weight, for d_a) in another -- and the build is
 * skipped.  For FROZEN weights only (the PLM body's layers 0-7, text.py:69-73): nothing here can tell that `w` changed.
 * Applies to the wide (n >= 256, resp. k >= 256) bf16x3 panel path; elsewhere the flag is ignored and the images rebuilt. */
int nrl_linear_fwd_img(const float* a, const float* w, const float* bias, int64_t m, int32_t n, int32_t k,
                       float* c, void* ws, size_t ws_bytes, int32_t image_ready, void* stream);
int nrl_linear_bwd_img(const float* a, const float* w, const float* d_c, int64_t m, int32_t n, int32_t k, float* d_a,
                       float* d_w, float* d_bias, void* ws, size_t ws_bytes, int32_t image_ready, void* stream);

/* ---- scaled dot-product attention of a transformer body: the self-attention inside `self.plm_model(**text)`, text.py:89
 * (HF RobertaSelfAttention -> F.scaled_dot_product_attention), ABI v12.  q, k, v, out (and their gradients): (n_batch, seq_len,
 * num_heads * head_dim) fp32, contiguous -- the projections' outputs as they are, no head transpose; key_keep (n_batch, seq_len)
 * uint8, 1 = the key takes part (the tokenizer's attention_mask), or NULL; `scale` multiplies q k^T; attention-probability
 * dropout with probability p_drop under the counter-based mask spec of nrl_dropout_mask: element (batch b, head h, query i,
 * key j) has flat index ((b * num_heads + h) * 128 + i) * 128 + j (uint32 arithmetic) in stream `stream0` of `seed`.
 * lse (n_batch * num_heads, seq_len): log-sum-exp of each query's scores, written by _fwd (may be NULL in inference), read by
 * _bwd.  bf16x3 arithmetic (hi, lo split operands on the bf16 matrix cores); seq_len <= 128, head_dim == 64
 * (nrl_sdpa_supported); anything else stays on the framework's attention. */
int32_t nrl_sdpa_supported(int64_t n_batch, int32_t seq_len, int32_t num_heads, int32_t head_dim);
int nrl_sdpa_fwd(const float* q, const float* k, const float* v, const uint8_t* key_keep, int64_t n_batch, int32_t seq_len,
                 int32_t num_heads, int32_t head_dim, float scale, double p_drop, uint64_t seed, uint32_t stream0, float* out,
                 float* lse, void* stream);
int nrl_sdpa_bwd(const float* q, const float* k, const float* v, const uint8_t* key_keep, const float* out, const float* d_out,
                 const float* lse, int64_t n_batch, int32_t seq_len, int32_t num_heads, int32_t head_dim, float scale,
                 double p_drop, uint64_t seed, uint32_t stream0, float* dq, float* dk, float* dv, void* stream);

/* ---- NPA (npa_module.py:208-252): personalized attention ----------------------------------------------------------------
 * Dropout streams of one NPA step (seed shared; flat indices row-major over the named shapes):
 *   stream0      x = dropout(emb[ids])            (N, L, D)   N = history rows then candidate rows
 *   stream0 + 1  c = dropout(relu(conv(x)))       (N, L, F)
 *   stream0 + 2  u = dropout(E_u[user_idx])       (B, U)      UserProjection
 *   stream0 + 3  history text query  dropout      (B, Pw)     first CNNPersAtt call
 *   stream0 + 4  candidate text query dropout     (B, Pw)     second CNNPersAtt call
 *   stream0 + 5  news query dropout               (B, Pn)     user encoder
 * The encoder takes stream0; nrl_npa_user_queries_* take the base of their four streams (stream0 + 2 above). */

/* CNNPersAtt.forward (text.py:376-392) over the history and candidate rows in one call: ids (N, L) -> out (N, F).
 * x and c as nrl_cnn_encoder_fwd (`p` supplies conv_weight / conv_bias and the dims; its att_* fields and query_dim are
 * ignored); then row n attends over ALL L tokens (pad tokens included, as the reference) with the query row
 * queries[owner[n]] of the (n_queries, F) table: s_t = q . c_t, w = softmax(s), out = sum_t w_t c_t.  owner (N) int32;
 * a row whose owner is outside [0, n_queries) gets a zero query. */
size_t nrl_npa_encoder_workspace_bytes(int64_t n_news, int32_t seq_len, int32_t embed_dim, int32_t num_filters,
                                       int32_t window);
int nrl_npa_encoder_fwd(const NrlCnnParams* p, const float* emb_table, int64_t vocab, const int64_t* ids, int64_t n_news,
                        int32_t seq_len, const float* queries, const int32_t* owner, int64_t n_queries, double p_drop,
                        uint64_t seed, uint32_t stream0, int32_t save_for_backward, float* out, void* ws, size_t ws_bytes,
                        void* stream);
/* Backward: adds into g->conv_weight, g->conv_bias and d_emb_table (the att_* fields of `g` are ignored); WRITES
 * d_queries (n_queries, F) = the sum of the rows' query gradients over the row ranges [query_offsets[i], query_offsets[i+1])
 * (n_queries + 1 int64, rows of one query contiguous), summed in row order.  sorted_positions as nrl_cnn_encoder_bwd. */
int nrl_npa_encoder_bwd(const NrlCnnParams* p, const NrlCnnGrads* g, float* d_emb_table, int64_t vocab, const int64_t* ids,
                        const int64_t* sorted_positions, int64_t n_news, int32_t seq_len, const float* queries,
                        const int32_t* owner, const int64_t* query_offsets, int64_t n_queries, double p_drop,
                        uint64_t seed, uint32_t stream0, const float* d_out, float* d_queries, void* ws, size_t ws_bytes,
                        void* stream);

/* Encode-once evaluation, step 1: the eval-mode conv feature maps c = relu(conv(emb[ids]) + b) (text.py:377-383 with dropout
 * off) of n_news rows, fp32, written straight into the caller's buffer out (n_news, L, F) -- a slice of a preallocated
 * (num_news, L, F) table.  The same lookup and convolution stages as nrl_npa_encoder_fwd under the current engine, so a cached
 * map has the bits the forward computes for that news.  `p` as for nrl_npa_encoder_fwd; out must be 16-byte aligned. */
size_t nrl_npa_conv_features_workspace_bytes(int64_t n_news, int32_t seq_len, int32_t embed_dim, int32_t num_filters,
                                             int32_t window);
int nrl_npa_conv_features(const NrlCnnParams* p, const float* emb_table, int64_t vocab, const int64_t* ids, int64_t n_news,
                          int32_t seq_len, float* out, void* ws, size_t ws_bytes, void* stream);

/* Every per-user query of an NPA step in one launch.  Field <-> reference state_dict key:
 *   user_table        user_projection.user_embed                                                   (num_users, U)
 *   text_proj_*       news_encoder.text_query_projection.preference_query_projection.{weight,bias}   (Pw, U), (Pw)
 *   text_att_*        news_encoder.personalized_attention.preference_query_projection.{weight,bias}  (F, Pw), (F)
 *   news_proj_*       user_encoder.news_query_projection.preference_query_projection.{weight,bias}   (Pn, U), (Pn)
 *   news_att_*        user_encoder.personalized_attention.preference_query_projection.{weight,bias}  (F, Pn), (F)
 * news_* NULL: late fusion (no user encoder).  Any U (no multiple-of-4 rule). */
typedef struct NrlNpaQueryParams {
  const float* user_table;
  const float* text_proj_weight;
  const float* text_proj_bias;
  const float* text_att_weight;
  const float* text_att_bias;
  const float* news_proj_weight;
  const float* news_proj_bias;
  const float* news_att_weight;
  const float* news_att_bias;
  int64_t num_users;
  int32_t user_dim;        /* U */
  int32_t text_query_dim;  /* Pw */
  int32_t news_query_dim;  /* Pn */
  int32_t num_filters;     /* F */
} NrlNpaQueryParams;

typedef struct NrlNpaQueryGrads { /* accumulators, kernels ADD */
  float* user_table;
  float* text_proj_weight;
  float* text_proj_bias;
  float* text_att_weight;
  float* text_att_bias;
  float* news_proj_weight;
  float* news_proj_bias;
  float* news_att_weight;
  float* news_att_bias;
} NrlNpaQueryGrads;

/* u = dropout(E_u[user_idx]) (stream0); per user b:
 *   text_queries[b]     = tanh(W_ta dropout(relu(W_tp u + b_tp)) + b_ta)   dropout stream0 + 1 (history)
 *   text_queries[B + b] = the same with dropout stream0 + 2                (candidates)
 *   news_queries[b]     = tanh(W_na dropout(relu(W_np u + b_np)) + b_na)   dropout stream0 + 3 (NULL under late fusion)
 * user_idx (B) int64; an index outside [0, num_users) reads a zero user vector and gets no gradient. */
size_t nrl_npa_user_queries_workspace_bytes(const NrlNpaQueryParams* p, int64_t batch);
int nrl_npa_user_queries_fwd(const NrlNpaQueryParams* p, const int64_t* user_idx, int64_t batch, double p_drop,
                             uint64_t seed, uint32_t stream0, float* text_queries, float* news_queries, void* stream);
/* Recomputes the forward and adds every gradient into `g`; a user that appears in several impressions of the batch gets the
 * sum over them, in batch order (no float atomics anywhere). */
int nrl_npa_user_queries_bwd(const NrlNpaQueryParams* p, const NrlNpaQueryGrads* g, const int64_t* user_idx, int64_t batch,
                             double p_drop, uint64_t seed, uint32_t stream0, const float* d_text_queries,
                             const float* d_news_queries, void* ws, size_t ws_bytes, void* stream);

/* NPA user encoder (user/npa.py:48-60) on the ragged history rows hist (n_hist, dim), rows of user b in
 * [hist_offsets[b], hist_offsets[b+1]): the reference runs it on the to_dense_batch output, so each user's softmax also
 * counts (max_hist - n_b) zero rows with score 0 -- a user's vector depends on the longest history of the batch.
 * out (B, dim) = sum_i w_i hist_i.  _bwd WRITES d_hist (n_hist, dim) and d_queries (B, dim). */
int nrl_personalized_user_attention_fwd(const float* hist, const int64_t* hist_offsets, int64_t batch, int32_t max_hist,
                                        int32_t dim, const float* queries, float* out, void* stream);
int nrl_personalized_user_attention_bwd(const float* hist, const int64_t* hist_offsets, int64_t batch, int32_t max_hist,
                                        int32_t dim, const float* queries, const float* d_out, float* d_hist,
                                        float* d_queries, void* stream);

/* Encode-once evaluation, step 2: NPAModule.forward in eval mode for a batch of impressions given by news-index lists, read
 * from the cached table (num_news, L, F) of nrl_npa_conv_features.  Plain fp32 vector code, the same under every engine.
 *   hist_idx (n_hist) / cand_idx (n_cand) int64 rows of the table; impression b owns [hist_offsets[b], hist_offsets[b+1]) and
 *   [cand_offsets[b], cand_offsets[b+1]) (batch + 1 int64 each).  An index outside [0, num_news) stands for an all-zero feature
 *   map (it pools to a zero vector) and is never dereferenced.
 *   q_hist, q_cand (batch, F): the tanh'd text queries of the two CNNPersAtt calls; q_news (batch, F): the user encoder's news
 *   query, or NULL for late fusion.
 * Per impression: every history row is pooled with q_hist[b] (softmax over ALL L tokens); the pooled rows are attended with
 * q_news[b], the softmax also counting max_hist - n_b zero rows of score 0 as nrl_personalized_user_attention_fwd does (late
 * fusion: their mean); every candidate row is pooled with q_cand[b] and dotted with the user vector.
 * WRITES user_vectors (batch, F) and scores (batch, max_cand), slots j >= n_cand_b exactly 0.  An empty history gives a zero
 * user vector.  Two launches: user vectors (one workgroup per impression, the waves' online-softmax states merged through
 * LDS), then one wave per candidate row of the whole batch.  Each table row is read once; no atomics; a fixed summation order.
 * F % 4 == 0, F <= 1024; max_hist / max_cand: the largest counts of the batch (longer lists are cut there). */
int nrl_npa_cached_scores(const float* table, int64_t num_news, int32_t seq_len, int32_t num_filters, const int64_t* hist_idx,
                          int64_t n_hist, const int64_t* hist_offsets, const int64_t* cand_idx, int64_t n_cand,
                          const int64_t* cand_offsets, int64_t batch, const float* q_hist, const float* q_cand,
                          const float* q_news, int32_t max_hist, int32_t max_cand, float* user_vectors, float* scores,
                          void* stream);

/* ---- DKN (dkn_module.py:207-240): knowledge-aware CNN news encoder + candidate-aware user attention -------------------
 * Field <-> reference state_dict key (news_encoder.*):
 *   word_table        text_embedding_layer.weight      (vocab, D)
 *   entity_table      entity_embedding_layer.weight    (num_entities, Ed)
 *   context_table     context_embedding_layer.weight   (num_entities, Ed); NULL: use_context = False (2 channels)
 *   transform_matrix  transform_matrix                 (Ed, D)
 *   transform_bias    transform_bias                   (D)
 *   conv_image[i]     conv_filters.{windows[i]}.weight (F, C, W, D) repacked as (F, W, C, D): the windowed GEMM's K order
 *   conv_bias[i]      conv_filters.{windows[i]}.bias   (F)
 * No dropout anywhere in DKN. */
typedef struct NrlDknParams {
  const float* word_table;
  const float* entity_table;
  const float* context_table;
  const float* transform_matrix;
  const float* transform_bias;
  const float* conv_image[4];
  const float* conv_bias[4];
  int32_t windows[4];
  int32_t num_windows;
  int32_t word_dim;    /* D */
  int32_t entity_dim;  /* Ed */
  int32_t num_filters; /* F */
} NrlDknParams;

typedef struct NrlDknGrads { /* accumulators, kernels ADD; conv_weight[i] in the reference (F, C, W, D) layout */
  float* word_table;
  float* entity_table;
  float* context_table;
  float* transform_matrix;
  float* transform_bias;
  float* conv_weight[4];
  float* conv_bias[4];
} NrlDknGrads;

/* KCNN.forward (news.py:255-299) on ids / entity_ids (N, L) int64 -> out (N, num_windows * F), windows in order, and the
 * argmax (N, num_windows * F) uint8 of each max over time (the first maximal position).  Window W has L - W + 1 valid
 * positions (no padding); W > L is refused.  The workspace of the forward must reach the backward unchanged. */
size_t nrl_dkn_encoder_workspace_bytes(const NrlDknParams* p, int64_t n_news, int32_t seq_len);
int nrl_dkn_encoder_fwd(const NrlDknParams* p, const int64_t* ids, const int64_t* entity_ids, int64_t n_news,
                        int32_t seq_len, float* out, uint8_t* argmax, void* ws, size_t ws_bytes, void* stream);
/* Backward: adds every gradient into `g`.  sorted_positions / entity_sorted_positions: the id-sorted visiting orders
 * (nrl_sort_positions) of ids and entity_ids; the entity and context tables share the second.  Row 0 of every table gets
 * nothing.  Only the convolution weight gradient (split-K) and the table gradients add partial sums atomically. */
int nrl_dkn_encoder_bwd(const NrlDknParams* p, const NrlDknGrads* g, const int64_t* ids, const int64_t* sorted_positions,
                        const int64_t* entity_ids, const int64_t* entity_sorted_positions, int64_t n_news, int32_t seq_len,
                        const float* out, const uint8_t* argmax, const float* d_out, void* ws, size_t ws_bytes,
                        void* stream);

/* DKN UserEncoder (user/dkn.py:40-107) + DNNPredictor (click_predictor.py:14-45) on ragged rows: hist (n_hist, dim) with
 * hist_offsets (B + 1), cand (n_cand, dim) with cand_offsets (B + 1).  Field <-> reference key:
 *   att_w1, att_b1, att_w2, att_b2      user_encoder.dnn.{0,1}.{weight,bias}     (Hd, 2 dim), (Hd), (1, Hd), (1)
 *   pred_w1, pred_b1, pred_w2, pred_b2  click_predictor.dnn.{0,2}.{weight,bias}  (Hd, 2 dim), (Hd), (1, Hd), (1)
 * scores (B, max_cand): 0 at padded candidates; user (B, dim) the user vector of every valid candidate (the affine attention
 * DNN makes it the same for all of them).  max_hist <= 1024, dim <= 1024, Hd <= 64.  _bwd WRITES d_hist and d_cand and
 * adds the parameter gradients (att_b1, att_b2 and att_w1[:, :dim] get exactly zero) in a fixed order: no float atomics. */
typedef struct NrlDknClickParams {
  const float* att_w1;
  const float* att_b1;
  const float* att_w2;
  const float* att_b2;
  const float* pred_w1;
  const float* pred_b1;
  const float* pred_w2;
  const float* pred_b2;
  int32_t hidden;
} NrlDknClickParams;

typedef struct NrlDknClickGrads {
  float* att_w1;
  float* att_b1;
  float* att_w2;
  float* att_b2;
  float* pred_w1;
  float* pred_b1;
  float* pred_w2;
  float* pred_b2;
} NrlDknClickGrads;

size_t nrl_dkn_click_workspace_bytes(int64_t batch, int32_t max_cand, int32_t dim, int32_t hidden);
int nrl_dkn_click_fwd(const NrlDknClickParams* p, const float* hist, const int64_t* hist_offsets, int32_t max_hist,
                      const float* cand, const int64_t* cand_offsets, int64_t batch, int32_t max_cand, int32_t dim,
                      float* scores, float* user, void* stream);
int nrl_dkn_click_bwd(const NrlDknClickParams* p, const NrlDknClickGrads* g, const float* hist, const int64_t* hist_offsets,
                      int32_t max_hist, const float* cand, const int64_t* cand_offsets, int64_t batch, int32_t max_cand,
                      int32_t dim, const float* user, const float* d_scores, float* d_hist, float* d_cand, void* ws,
                      size_t ws_bytes, void* stream);
/* The click predictor factored for a full-catalogue ranking (symbols added to ABI v19): its first layer splits by columns,
 * pred_w1 = [Wc | Wu], so pre[b, v, j] = P[v, j] + q[b, j] and nrl_topk_relu_scores ranks the whole table without the (B, V, dim)
 * work.  Neither entry needs a workspace; limits and messages are those of nrl_dkn_click_fwd.
 * nrl_dkn_user_query: one workgroup per user.  user (B, dim): the user vector, the bits nrl_dkn_click_fwd writes for the same
 *   history (the same attention code); q (B, Hd): q[b, j] = (sum_d pred_w1[j, dim + d] user[b, d]) + pred_b1[j].  An empty
 *   history gives user = 0 and q = pred_b1.
 * nrl_dkn_cand_project: out (N, Hd): out[n, j] = sum_d pred_w1[j, d] rows[n, d], no bias; rows (N, dim) fp32, N < 2^31; plain fp32
 *   fmaf code, once per table.
 * Every output element is one reduction whose order is fixed by dim alone: its bits do not depend on B, N, the grid or the
 * GEMM engine setting. */
int nrl_dkn_user_query(const NrlDknClickParams* p, const float* hist, const int64_t* hist_offsets, int32_t max_hist, int64_t B,
                       int32_t dim, float* user, float* q, void* stream);
int nrl_dkn_cand_project(const NrlDknClickParams* p, const float* rows, int64_t N, int32_t dim, float* out, void* stream);

/* ---- CAUM (caum_module.py:326-360, user/caum.py:81-125): candidate-aware user encoder, head-padded self-attention ------
 * nrl_caum_attn_*: attention over a packed (rows, 3 * heads * head_dim) q|k|v buffer -> o (rows, heads * head_dim), for every
 * (outer, head) group over `seq` positions; seq_first: row = s * outer + n (nn.MultiheadAttention, batch_first=False), else
 * row = n * seq + s.  lse (outer * heads, seq) is written by the forward and read by the backward; scale 0 = 1/sqrt(head_dim).
 * head_dim in {16, 20, 32, 48, 64}: a module with another head dim pads its projections per head (news_encoder.MHSAAddAtt).
 * dqkv is fully written. */
int nrl_caum_attn_fwd(const float* qkv, float* o, float* lse, int64_t outer, int64_t seq, int32_t heads, int32_t head_dim,
                      int32_t seq_first, float scale, void* stream);
int nrl_caum_attn_bwd(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv, int64_t outer,
                      int64_t seq, int32_t heads, int32_t head_dim, int32_t seq_first, float scale, void* stream);
/* y[k] = x[k] * mask(seed, stream_id, p)[k] (the nrl_dropout_mask spec, scaled by 1/(1-p)); also the backward. */
int nrl_caum_dropout(const float* x, float* y, int64_t n, double p, uint64_t seed, uint32_t stream_id, void* stream);
/* The user encoder over every candidate slot at once: rows r = (b, i, t), b < B users, i < C slots, t < H = max_hist.
 * Dropout streams of slot i: stream_base + 3i -> dropout1 of the candidate over (B, D); + 3i + 1 -> dropout2 of the history
 * over (B, H, D); + 3i + 2 -> dropout3 of [cnn, self] over (B, H, F + U); row-major flat indices.
 * expand: h (B, H, D), c (B, C, D) -> hd (B, C, H, D), cd (B, C, D); the backward sums the slots in order. */
int nrl_caum_expand_fwd(const float* h, const float* c, int64_t B, int32_t C, int32_t H, int32_t D, double p, uint64_t seed,
                        uint32_t stream_base, float* hd, float* cd, void* stream);
int nrl_caum_expand_bwd(const float* d_hd, const float* d_cd, int64_t B, int32_t C, int32_t H, int32_t D, double p,
                        uint64_t seed, uint32_t stream_base, float* d_h, float* d_c, void* stream);
/* combine: P (B * hist_slots * H, 3F + U) = history rows x [linear1 left | centre | right blocks ; linear2 history block]
 * (+ biases), Q (B * C, F + U) = candidate rows x [linear1 candidate block ; linear2 candidate block] ->
 *   cnn (R, F) = P[t-1, left] + P[t, centre] + P[t+1, right] + Q[cnn]  (circular in t over the dense, zero-padded history)
 *   s   (R, U) = P[t, linear2] + Q[linear2]
 * hist_slots = C (training: per-slot dropped-out history) or 1 (evaluation: one history for every slot).  _bwd writes
 * d_P and d_Q in a fixed order. */
int nrl_caum_combine_fwd(const float* P, const float* Q, int64_t B, int32_t C, int32_t H, int32_t F, int32_t U,
                         int32_t hist_slots, float* cnn, float* s, void* stream);
int nrl_caum_combine_bwd(const float* d_cnn, const float* d_s, int64_t B, int32_t C, int32_t H, int32_t F, int32_t U,
                         int32_t hist_slots, float* d_P, float* d_Q, void* stream);
/* z (R, F + U) = dropout3([cnn, a]); the backward splits d_z back under the same mask. */
int nrl_caum_concat_dropout_fwd(const float* cnn, const float* a, int64_t B, int32_t C, int32_t H, int32_t F, int32_t U,
                                double p, uint64_t seed, uint32_t stream_base, float* z, void* stream);
int nrl_caum_concat_dropout_bwd(const float* d_z, int64_t B, int32_t C, int32_t H, int32_t F, int32_t U, double p,
                                uint64_t seed, uint32_t stream_base, float* d_cnn, float* d_a, void* stream);
/* z (groups * rows_per_group, N) = tanh(a + g[row / rows_per_group]); _bwd writes d_a and d_g (the sum over the group). */
int nrl_caum_group_tanh_fwd(const float* a, const float* g, int64_t groups, int32_t rows_per_group, int32_t N, float* z,
                            void* stream);
int nrl_caum_group_tanh_bwd(const float* d_z, const float* z, int64_t groups, int32_t rows_per_group, int32_t N, float* d_a,
                            float* d_g, void* stream);
/* DenseAttention's last layer (w3 (N2), b3 (1)) on z2 (R, N2), softmax over the H slots (no mask), user (B * C, U) =
 * sum_t alpha_t x_t for x (R, U), scores (B, C) = cd . user, 0 where slot0 + i >= the impression's candidate count
 * (cand_offsets (B + 1)).  alpha (R) and user are kept for the backward.  _bwd writes d_z2, d_x, d_cd and ADDS d_w3, d_b3
 * (fixed-order reduction).  H <= 8192. */
int nrl_caum_score_fwd(const float* z2, const float* w3, const float* b3, const float* x, const float* cd,
                       const int64_t* cand_offsets, int64_t B, int32_t C, int32_t slot0, int32_t H, int32_t N2, int32_t U,
                       float* scores, float* alpha, float* user, void* stream);
size_t nrl_caum_score_workspace_bytes(int64_t B, int32_t C, int32_t H, int32_t N2);
int nrl_caum_score_bwd(const float* d_scores, const float* z2, const float* w3, const float* x, const float* cd,
                       const float* alpha, const float* user, const int64_t* cand_offsets, int64_t B, int32_t C,
                       int32_t slot0, int32_t H, int32_t N2, int32_t U, float* d_z2, float* d_x, float* d_cd, float* d_w3,
                       float* d_b3, void* ws, size_t ws_bytes, void* stream);
/* Factored evaluation (no dropout): the q|k|v row of (user b, slot i, position t) is qkv_h[b * H + t] + qkv_c[cand_offsets[b] + i]
 * (rows of 3 * heads * head_dim), qkv_h alone where user b has no slot i.  nrl_caum_eval_attn runs the across-users attention
 * (keys: all B users) for the queries [j0, j1) of the slot-major pair list: pair_row (n) = flat candidate row, pair_user (n) = its
 * user, ordered by (slot, user).  slot_tab (entries, 4) int32 = {slot, first pair, pair count, first work item} of every slot the
 * range touches, a slot taking ceil(pair count / 64) * H * heads work items; n_items = their total (< 2^31).
 * o ((j1 - j0) * H, heads * head_dim), row (j - j0) * H + t.  Every index taken from cand_offsets, the pair list or the table
 * is range-checked on the device: a violation ORs 1 into *status (int32, never cleared here) and that pair's rows are zeros.
 * Exact-fp32 matrix cores under either engine; no workspace, no float atomics, nothing read back.
 * nrl_caum_eval_add: x[(jj, t)] = y[(jj, t)] + xh[pair_user[j0 + jj] * H + t] + xc[j0 + jj] over pairs * H rows of U floats
 * (U % 4 == 0; x may be y; xc (n, U) in pair-list order); a user index out of range: zeros and status |= 1. */
int nrl_caum_eval_attn(const float* qkv_h, const float* qkv_c, const int64_t* cand_offsets, const int64_t* pair_row,
                       const int64_t* pair_user, const int32_t* slot_tab, int32_t entries, int64_t n_items, int64_t B, int32_t H,
                       int64_t n, int64_t j0, int64_t j1, int32_t heads, int32_t head_dim, float scale, float* o,
                       int32_t* status, void* stream);
int nrl_caum_eval_add(const float* y, const float* xh, const float* xc, const int64_t* pair_user, int64_t n, int64_t j0,
                      int64_t pairs, int64_t B, int32_t H, int32_t U, float* x, int32_t* status, void* stream);

/* ---- MINER (miner_module.py:258-323,398-406, layers/attention.py:93-166): poly attention, category bias, scores, ------------
 * disagreement loss.  History / candidate rows are FLAT (n_hist / n_cand rows) with int64 offsets (B + 1) and sorted int64
 * assignment vectors; every feature width is a multiple of 4.  No float atomics in these entries: what they reduce (context
 * codes, the two bias-free projection weights through nrl_miner_wgrad, the category sums, the loss) is bit-reproducible; the
 * GEMM engines' own weight gradients (reduce_dim, the transformer body) keep their split-K atomics.
 *
 * nrl_miner_slab_sum: out[j] = scale * sum_s slabs[s * n + j], s in order. */
int nrl_miner_tanh_grad(const float* d_c, const float* c, int64_t n, float* d_pre, void* stream);   /* d_c * (1 - c^2) */
/* d_w (N, K) = G^T X for G (R, N), X (R, K): slabs of 64 rows, then the slabs added in order. */
size_t nrl_miner_wgrad_workspace_bytes(int64_t R, int32_t N, int32_t K);
int nrl_miner_wgrad(const float* G, const float* X, int64_t R, int32_t N, int32_t K, float* d_w, void* ws, size_t ws_bytes,
                    void* stream);
int nrl_miner_slab_sum(const float* slabs, int64_t num_slabs, int64_t n, float scale, float* out, void* stream);
/* partial[g] = sum over k != l of cos(x[g, k], x[g, l]) for x (groups, R, D), rows divided by (norm + eps).  _bwd: d_x of
 * d_loss[0] * scale * sum_g partial[g] (d_loss: one float on the device). */
int nrl_miner_cos_fwd(const float* x, int64_t groups, int32_t R, int32_t D, float eps, float* partial, void* stream);
int nrl_miner_cos_bwd(const float* x, int64_t groups, int32_t R, int32_t D, float eps, const float* d_loss, float scale,
                      float* d_x, void* stream);
/* bias[t] = hh_t . (S_all - S_own[user(t)]) / n_cand over unit-normalised (no epsilon) category rows hc (n_hist, Dc),
 * cc (n_cand, Dc): the mean over ALL candidates of the batch of the cosine, the user's own candidates zeroed.  The workspace
 * of _fwd is handed to _bwd unchanged. */
size_t nrl_miner_categ_bias_workspace_bytes(int64_t B, int64_t n_hist, int64_t n_cand, int32_t Dc);
int nrl_miner_categ_bias_fwd(const float* hc, const float* cc, const int64_t* batch_hist, const int64_t* cand_off, int64_t B,
                             int64_t n_hist, int64_t n_cand, int32_t Dc, float* bias, void* ws, size_t ws_bytes,
                             void* stream);
int nrl_miner_categ_bias_bwd(const float* d_bias, const float* hc, const float* cc, const int64_t* hist_off,
                             const int64_t* batch_cand, const float* bias, int64_t B, int64_t n_hist, int64_t n_cand,
                             int32_t Dc, float* d_hc, float* d_cc, void* ws, size_t ws_bytes, void* stream);
/* user_vector (B, K, D) = softmax over max_hist positions of (P codes^T + bias)^T times E, for E (n_hist, D),
 * P (n_hist, Cd) = tanh(E W^T), codes (K, Cd), bias (n_hist) or NULL.  The max_hist - n_b padded positions of user b take
 * part with logit 1e-30 and a zero embedding (closed-form denominator term).  A (B, K, max_hist) is kept for _bwd, which
 * writes d_E, d_P, d_codes and d_bias (NULL without bias); workspace: the per-user slabs of d_codes. */
size_t nrl_miner_poly_workspace_bytes(int64_t B, int32_t K, int32_t Cd);
int nrl_miner_poly_fwd(const float* E, const float* P, const float* codes, const float* bias, const int64_t* hist_off,
                       int64_t B, int32_t max_hist, int32_t D, int32_t Cd, int32_t K, float* user_vector, float* A,
                       void* stream);
int nrl_miner_poly_bwd(const float* d_user_vector, const float* E, const float* P, const float* codes, const float* A,
                       const int64_t* hist_off, int64_t B, int32_t max_hist, int32_t D, int32_t Cd, int32_t K, float* d_E,
                       float* d_P, float* d_codes, float* d_bias, void* ws, size_t ws_bytes, void* stream);
/* scores (B, max_cand), 0 at padded slots, from cand (n_cand, D) and user_vector (B, K, D), K <= 255.  mode 0: max over K
 * (argmax (n_cand) bytes kept, lowest index on ties), 1: mean, 2: softmax_K(cand . gelu(Z)) weighted sum with Z (B, K, D) the
 * target-aware projection (G = gelu(Z), S, W (n_cand, K) kept).  G / S / W / argmax may be NULL when no backward follows. */
int nrl_miner_score_fwd(const float* cand, const float* user_vector, const float* Z, const int64_t* cand_off, int64_t B,
                        int32_t max_cand, int32_t D, int32_t K, int32_t mode, float* scores, float* G, float* S, float* W,
                        uint8_t* argmax, void* stream);
int nrl_miner_score_bwd(const float* d_scores, const float* scores, const float* cand, const float* user_vector,
                        const float* Z, const float* G, const float* S, const float* W, const uint8_t* argmax,
                        const int64_t* cand_off, int64_t B, int32_t max_cand, int32_t D, int32_t K, int32_t mode,
                        float* d_cand, float* d_user_vector, float* d_Z, void* stream);

/* ---- SentiDebias (fair_rec/senti_debias_module.py:164-263,406-411,475-530; encoders/news/aspect.py) -------------------------
 * The head around the NRMS encoders.  T (S, D) = tanh(E W^T + b) is the sentiment encoder evaluated on its S = num_sent_classes + 1
 * ids (S <= 8): every sentiment vector is a row of it.  ids: int64 sentiment ids of the flat news rows, history rows first
 * (n_hist of N); offsets: int64 (B + 1); D and the hidden width are multiples of 4.  No float atomics: row reductions are written
 * as one slab per 64 rows (nrl_sd_num_slabs(rows) of them) which the caller adds in order with nrl_miner_slab_sum.
 *
 * nrl_sd_rowcos_*: out2 = [mean over history rows, mean over candidate rows] of news_r . T[id_r] / (1e-8 + |news_r| |T[id_r]|);
 *   partial: 2 * nrl_sd_num_slabs(N) floats of scratch.  _bwd: d_out2 (2) on the device -> d_news (N, D) overwritten (NULL: skipped)
 *   and slabs of S * D floats for d_T (NULL: skipped).
 * nrl_sd_hist_*: out (B, H, D): T[id] at the real slots of each user's history, ZERO at padded slots; _bwd: slabs (per 64 slots) of d_T.
 * nrl_sd_late_fwd: frac (B, S) = class counts / history size, u (B, D) = frac T (late fusion); its gradient is nrl_sd_bt_matmul.
 * nrl_sd_bt_matmul: out (S, D) = W^T X for W (B, S), X (B, D), users added in order.
 * nrl_sd_scores_*: out (B, C) = free_scores + (u . T[id of candidate c]) at real slots; P (B, S) = u T^T kept (may be NULL).
 *   _bwd: d_out (B, C) -> dP (B, S), d_u (B, D) = dP T; d_T = nrl_sd_bt_matmul(dP, u); d_free_scores = d_out.
 * nrl_sd_disc_tail_*: hidden (N, Hd) = tanh(linear1(news)), w2 (O, Hd), b2 (O), O <= 8: out2 = the two side means of
 *   -log_softmax(hidden w2^T + b2) at column id - 1, id 0 wrapping to column O - 1 (:409); rows with id > O contribute nothing
 *   (the host raises before).  _bwd: d_pre (N, Hd) = d_hidden (1 - hidden^2) overwritten; slabs of nrl_sd_disc_slab_width(Hd, O)
 *   floats: O * Hd of d_w2, then O of d_b2, then padding (NULL: weight gradients skipped).  d_pre is always written: linear1's
 *   weight gradient needs it as much as the activation gradient does.
 * Edge cases: a side without rows (n_hist == 0 or n_hist == N) gives 0 for its mean where the reference's empty mean is NaN;
 * nrl_sd_late_fwd divides by the history size, so a user without history gives NaN rows, as the reference does. */
int64_t nrl_sd_num_slabs(int64_t rows);
int32_t nrl_sd_disc_slab_width(int32_t Hd, int32_t O);
int nrl_sd_rowcos_fwd(const float* news, const int64_t* ids, const float* T, int64_t N, int64_t n_hist, int32_t D, int32_t S,
                      float* partial, float* out2, void* stream);
int nrl_sd_rowcos_bwd(const float* news, const int64_t* ids, const float* T, const float* d_out2, int64_t N, int64_t n_hist,
                      int32_t D, int32_t S, float* d_news, float* slabs, void* stream);
int nrl_sd_hist_fwd(const int64_t* ids, const int64_t* hist_off, const float* T, int64_t B, int32_t H, int32_t D, int32_t S,
                    int64_t n_ids, float* out, void* stream);
int nrl_sd_hist_bwd(const float* d_out, const int64_t* ids, const int64_t* hist_off, int64_t B, int32_t H, int32_t D, int32_t S,
                    int64_t n_ids, float* slabs, void* stream);
int nrl_sd_late_fwd(const int64_t* ids, const int64_t* hist_off, const float* T, int64_t B, int32_t D, int32_t S, int64_t n_ids,
                    float* frac, float* u, void* stream);
int nrl_sd_bt_matmul(const float* W, const float* X, int64_t B, int32_t S, int32_t D, float* out, void* stream);
int nrl_sd_scores_fwd(const float* u, const float* T, const int64_t* ids, const int64_t* cand_off, const float* free_scores,
                      int64_t B, int32_t C, int32_t D, int32_t S, int64_t n_ids, float* P, float* out, void* stream);
int nrl_sd_scores_bwd(const float* d_out, const float* T, const int64_t* ids, const int64_t* cand_off, int64_t B, int32_t C,
                      int32_t D, int32_t S, int64_t n_ids, float* dP, float* d_u, void* stream);
int nrl_sd_disc_tail_fwd(const float* hidden, const float* w2, const float* b2, const int64_t* ids, int64_t N, int64_t n_hist,
                         int32_t Hd, int32_t O, float* partial, float* out2, void* stream);
int nrl_sd_disc_tail_bwd(const float* hidden, const float* w2, const float* b2, const int64_t* ids, const float* d_out2, int64_t N,
                         int64_t n_hist, int32_t Hd, int32_t O, float* d_pre, float* slabs, void* stream);

/* ---- MANNeR (fair_rec/manner_a_module.py:151-176, manner_module.py:152-204) ---------------------------------------------------
 * nrl_supcon_embed_fwd_bwd: pytorch-metric-learning 2.2.0 SupConLoss(temperature, DotProductSimilarity(normalize_embeddings=False))
 *   of embeddings E (N, D) with int64 labels (N), AvgNonZeroReducer, loss (1) and dE (N, D) = grad_scale * d loss / d E in one call.
 *   Pairs: positives = same label off the diagonal, negatives = different label; the log-sum-exp runs over everything off the
 *   diagonal; rows without a positive (or with a row loss <= 0) are dropped by the reducer.  The loss is exactly 0 with dE = 0 when
 *   the batch has no positive pair or no negative pair.  S = E E^T and dE = (dS + dS^T) E run on the exact-fp32 MFMA GEMM whatever
 *   nrl_set_gemm_engine says (a few MFLOP; the scores go through exp()).  1 <= N <= 1024, D a multiple of 4 up to 1024; workspace nrl_supcon_embed_workspace_bytes(N, D),
 *   256-byte aligned.  No atomics: two calls on the same input give the same bits.
 * nrl_manner_scores: out (B, max_cand) = sum_t weights[t] * zscore_b(mean(tables[t][hist of b]) . tables[t][cand of b]) for k in
 *   {1, 2, 3} news-vector tables (V, D); `tables` (k device pointers) and `weights` (k floats) are HOST arrays read during the call.
 *   hist_idx / cand_idx: int64 news rows concatenated over the impressions, *_offsets: int64 (B + 1).  The z-score uses the mean
 *   and the UNBIASED standard deviation of the impression's own candidates, without an epsilon: an impression with one candidate,
 *   with zero score variance or with an empty history gives a non-finite row, as the reference does.  Padded slots are written 0;
 *   indices outside [0, V) are clamped.  D a multiple of 4 up to 1024, max_cand <= 2048.  Forward only. */
size_t nrl_supcon_embed_workspace_bytes(int64_t N, int32_t D);
int nrl_supcon_embed_fwd_bwd(const float* E, const int64_t* labels, int64_t N, int32_t D, float temperature, float grad_scale,
                             float* loss, float* dE, void* ws, size_t ws_bytes, void* stream);
int nrl_manner_scores(const float* const* tables, const float* weights, int32_t k, int64_t V, const int64_t* hist_idx,
                      const int64_t* hist_offsets, const int64_t* cand_idx, const int64_t* cand_offsets, int64_t B,
                      int32_t max_cand, int32_t D, float* out, void* stream);

/* ---- streaming evaluation metrics (ABI v19).  Replaces: the torchmetrics objects wired at nrms_module.py:182-195 and computed at
 * :456-493 (RetrievalMRR, RetrievalNormalizedDCG, Diversity, Personalization -- the AUROC stays a global sort on the host side),
 * metrics/functional.py:8-127 (diversity, personalization, generalized_jaccard) and the per-query grouping with
 * empty_target_action="neg" of metrics/base.py:137-182.
 * nrl_impression_metrics: one batch of B ragged impressions.  preds / targets: N fp32, cand_offsets: (B + 1) int64.  n_aspects in
 *   {0, 1, 2}; aspect a has cand_aspects_a (N int64), hist_aspects_a (n_hist int64) and num_classes_a in [2, 1024]; hist_offsets
 *   (B + 1) int64 is shared by the aspects (all four may be null when n_aspects == 0).  top_k: n_k <= 4 values in [1, 1024], a HOST
 *   array read during the call.
 *   rank (N int32, nullable): 0-based position of every candidate in its impression's ranking, score descending, ties by ascending
 *     position (a stable descending sort; NaN sorts first, -0 == +0).  Candidates of a flagged impression get -1.
 *   rows (B, n_cols fp32, nullable), n_cols = 1 + n_k + 2 * n_k * n_aspects: rr | ndcg@k ... | per aspect: div@k ... then pers@k ...
 *     rr = 1 / (1 + rank of the best-ranked candidate with target > 0), 0 without one; ndcg: gain = target, discount
 *     1 / log2(pos + 2), ideal = the k largest targets, 0 when the ideal is 0, k > C uses all C; div = entropy of the aspect
 *     distribution of the top k / log(num_classes); pers = sum(min) / sum(max) of the top-k aspect counts against the history
 *     aspect counts; both 0 when every candidate aspect id of the impression is 0; pers = 0 for an empty history.
 *   sums (n_cols doubles) and count (one int64), nullable together: this call ADDS the column sums of its rows and the number of
 *     unflagged impressions.  The rows are reduced in a fixed order (a tree inside fixed 4096-row parts, a tree over the parts,
 *     one plain add per column): no floating-point atomics, the same inputs give the same bits.
 *   status (one int32, required): the kernel ORs NRL_METRICS_E_* into it.  A flagged impression writes zero rows, contributes
 *     nothing to sums / count, and is never indexed outside the buffers.
 *   Workspace: nrl_impression_metrics_workspace_bytes, 256-byte aligned.  B == 0 returns success without a launch.  Sizes beyond
 *   the limits above return NRL_E_INVALID.  No host synchronisation. */
#define NRL_METRICS_MAX_CAND 4096
#define NRL_METRICS_MAX_CLASSES 1024
#define NRL_METRICS_MAX_K 1024
#define NRL_METRICS_MAX_NK 4
#define NRL_METRICS_E_TOO_LONG 1 /* an impression has more than NRL_METRICS_MAX_CAND candidates */
#define NRL_METRICS_E_ASPECT 2   /* an aspect id is negative or >= num_classes */
#define NRL_METRICS_E_OFFSETS 4  /* an offset vector decreases or leaves [0, N] / [0, n_hist] */
size_t nrl_impression_metrics_workspace_bytes(int64_t N, int64_t B, int32_t n_aspects, int32_t n_k);
int nrl_impression_metrics(const float* preds, const float* targets, const int64_t* cand_offsets, int64_t N, int64_t B,
                           int32_t n_aspects, const int64_t* cand_aspects0, const int64_t* hist_aspects0, int32_t num_classes0,
                           const int64_t* cand_aspects1, const int64_t* hist_aspects1, int32_t num_classes1,
                           const int64_t* hist_offsets, int64_t n_hist, const int32_t* top_k, int32_t n_k, int32_t* rank,
                           float* rows, double* sums, int64_t* count, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- a grid of ensemble weights in one pass over the impressions (symbols added to ABI v19).  Replaces: one full evaluation per
 * (categ_weight, sent_weight) point of manner_module.py:152-204 -- the reference, too, re-scores and re-ranks everything per point.
 * nrl_manner_zscores: nrl_manner_scores with the combination left out.  out (k, N) fp32: out[t * N + cand_offsets[b] + c] = the
 *   z-score of candidate c of impression b under table t, flat and ragged in cand_offsets order (N = cand_offsets[B], the length
 *   of cand_idx); no padded block.  Row t has the bits nrl_manner_scores gives table t alone under weight 1.  The same quirks (one
 *   candidate, zero variance, an empty history: non-finite), the same clamping of indices, the same limits; candidates beyond
 *   max_cand or outside [0, N) are not written.
 * nrl_grid_metrics: nrl_impression_metrics for G score vectors that are linear combinations of T component vectors.  comp (T, N)
 *   fp32, T in [1, 4]; weights (G, T) fp32 ON THE DEVICE, G in [1, 4096]; targets, cand_offsets, the aspects, hist_offsets, top_k
 *   and status exactly as nrl_impression_metrics (same limits, same flags).  The score of candidate i under config g, over t
 *   ascending: terms with weights[g, t] == 0 are skipped (a NaN component cannot poison a config that does not use it), the first
 *   remaining term is the product w * comp[t, i], every later one fma(w, comp[t, i], acc) -- nrl_manner_scores's rounding; a row
 *   of zeros scores +0 everywhere.
 *   rows (G, B, n_cols fp32, nullable): row (g, b) has the bits nrl_impression_metrics writes for impression b when fed config
 *     g's scores.  preds (G, N fp32, nullable): those scores (a flagged impression's are not written).
 *   sums (G, n_cols doubles) and count (ONE int64), nullable together: ADDS, per config, the column sums of its rows by the fixed
 *     reduction of nrl_impression_metrics (same bits), and once the number of unflagged impressions (it does not depend on g).
 *   A flagged impression writes zero rows under every config and is absent from every sum and from count.
 *   configs_per_block: 0 = nrl_grid_metrics_configs_per_block(B, G), the plan (from G and B alone: about 2048 workgroups); a
 *     positive value overrides it.  No value changes a bit of the results.
 *   Workspace: nrl_grid_metrics_workspace_size (the name keeps it out of the *_workspace_bytes table), 256-byte aligned; it holds
 *   the (G, B, n_cols) rows only when the caller keeps none: caller_rows != 0 says that `rows` will be given and leaves them out.  B == 0 returns success without a launch; sizes beyond the limits return
 *   NRL_E_INVALID.  Three launches whatever G; no float atomics, no allocation, no host synchronisation. */
#define NRL_GRID_MAX_COMPONENTS 4
#define NRL_GRID_MAX_CONFIGS 4096
int nrl_manner_zscores(const float* const* tables, int32_t k, int64_t V, const int64_t* hist_idx, const int64_t* hist_offsets,
                       const int64_t* cand_idx, const int64_t* cand_offsets, int64_t N, int64_t B, int32_t max_cand, int32_t D,
                       float* out, void* stream);
int32_t nrl_grid_metrics_configs_per_block(int64_t B, int32_t G);
size_t nrl_grid_metrics_workspace_size(int64_t B, int32_t G, int32_t n_aspects, int32_t n_k, int32_t caller_rows);
int nrl_grid_metrics(const float* comp, int32_t T, const float* weights, int32_t G, const float* targets, const int64_t* cand_offsets,
                     int64_t N, int64_t B, int32_t n_aspects, const int64_t* cand_aspects0, const int64_t* hist_aspects0,
                     int32_t num_classes0, const int64_t* cand_aspects1, const int64_t* hist_aspects1, int32_t num_classes1,
                     const int64_t* hist_offsets, int64_t n_hist, const int32_t* top_k, int32_t n_k, int32_t configs_per_block,
                     float* rows, float* preds, double* sums, int64_t* count, int32_t* status, void* ws, size_t ws_bytes,
                     void* stream);

/* ---- full-catalogue top-k recommendation (symbols added to ABI v19; nothing of the reference is replaced: it can only re-rank the
 * candidates an impression lists).
 * nrl_topk_scores: for each of B users the k rows of `table` with the highest dot product with the user's vector, without ever
 *   writing the (B, V) score matrix.  user_vec (B, D) and table (V, D): fp32, row-major, device.  D a multiple of 4 up to 1024,
 *   k in [1, NRL_TOPK_MAX_K], V < 2^31, B < 2^31.
 *   excl_idx (int64) / excl_off ((B + 1) int64), nullable together: a ragged per-user list of table rows that are never returned
 *     for that user (the history): user b owns excl_idx[excl_off[b] .. excl_off[b + 1]).  Duplicates, empty lists and any length
 *     are fine.  excl_off[B] is the length of excl_idx and is trusted as such; every other offset is validated against it.
 *   eligible (V uint8, nullable): 0 = the row is never returned for anyone (a padding row, stale news).
 *   slices: 0 = the library chooses how many pieces of V are scanned in parallel per tile of 64 users; > 0 forces that count
 *     (clamped to the number of 128-row table tiles).  The result does not depend on it.
 *   out_idx (B, k) int64 / out_score (B, k) fp32: score descending, equal scores by ascending table row (-0 == +0); when fewer
 *     than k rows qualify the tail is -1 / -inf.
 *   status (one int32, required): the kernels OR NRL_TOPK_E_* into it.
 *   Arithmetic: every score is the exact-fp32 MFMA dot product accumulated over D in one fixed order, whatever the GEMM engine
 *     setting: the bits of score(u, v) do not depend on B, V, k, slices or the grid, and the selection is a pure function of those
 *     bits and the row numbers.  No floating-point atomics, no allocation, no host synchronisation.
 *   Workspace: nrl_topk_scores_workspace_bytes (callable without a device; B * slices * k * 8 bytes rounded up to 256, never
 *     O(B * V)), 256-byte aligned.  B == 0 returns success without a launch; V == 0 fills the output with -1 / -inf.  Sizes outside
 *     the limits above return NRL_E_INVALID, a short workspace NRL_E_WORKSPACE. */
#define NRL_TOPK_MAX_K 128
#define NRL_TOPK_MAX_D 1024
#define NRL_TOPK_E_EXCLUDE 1 /* an exclusion index is outside [0, V): that entry is ignored */
#define NRL_TOPK_E_OFFSETS 2 /* excl_off decreases or leaves [0, excl_off[B]]: that user's row is all -1 / -inf */
#define NRL_TOPK_E_NAN 4     /* a NaN score of an eligible, not excluded row: the row is left out for that user */
size_t nrl_topk_scores_workspace_bytes(int64_t B, int64_t V, int32_t D, int32_t k, int32_t slices);
int nrl_topk_scores(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k, const int64_t* excl_idx,
                    const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score,
                    int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_topk_interest_scores: the same ranking where a user is K interest vectors and the score of a table row is an aggregate over
 *   them (MINER, miner_module.py:298-308 and attention.py:162-166 with the candidate list replaced by the table).  interests
 *   (B, K, D), gate (B, K, D; required by mode 2, ignored otherwise) and table (V, D): fp32, row-major, device.  B counts users.
 *   With s_j = interests[u, j, :] . table[v, :] the score of (u, v) is
 *     mode 0 (max):      max_j s_j;
 *     mode 1 (mean):     (s_0 + s_1 + ... + s_{K-1}) / K, summed in fp32 in ascending j, then one fp32 division;
 *     mode 2 (weighted): with l_j = gate[u, j, :] . table[v, :], m = max_j l_j and e_j = expf(l_j - m):
 *                        (sum_j e_j s_j) / (sum_j e_j), both sums in fp32 in ascending j.  gate is gelu(user_vector Wt^T): it is
 *                        formed before the call and does not depend on the table row.
 *   K in [1, NRL_TOPK_MAX_INTERESTS]; D, k, V, B, excl_idx / excl_off, eligible, slices, out_idx / out_score and status as for
 *   nrl_topk_scores (slices 0: the count is chosen per tile of floor(64 / K) users).  A NaN aggregate (any NaN s_j or l_j, or
 *   inf - inf) of an eligible, not excluded row sets NRL_TOPK_E_NAN and the row is left out for that user.
 *   Arithmetic: every s_j and l_j is the one exact-fp32 MFMA accumulator chain of nrl_topk_scores and the aggregation order is
 *     fixed, so the bits of a user's score for a row depend on the user's K rows, the table row, D, K and the mode alone, not on B,
 *     V, k, slices, the grid or the GEMM engine setting; at K == 1 every mode returns the bits of nrl_topk_scores.  Neither the
 *     (B, V) nor the (B * K, V) matrix is written.  No floating-point atomics, no allocation, no host synchronisation.
 *   Workspace: there is no size function of its own.  nrl_topk_scores_workspace_bytes(B, V, D, k, slices) with B in users always
 *     suffices: the entry keeps B * lists * k * 8 bytes, where lists = min(slices, tiles) for slices > 0 and otherwise
 *     ceil(512 / ceil(B / floor(64 / K))) clamped to [1, tiles], which is never above the count that function sizes for
 *     (floor(64 / K) <= 64).  The entry carves with its own count and refuses a shorter buffer with NRL_E_WORKSPACE before any
 *     launch.  B == 0 returns success without a launch; V == 0 fills the output with -1 / -inf.  Sizes or a mode outside the
 *     limits, and mode 2 without gate, return NRL_E_INVALID. */
#define NRL_TOPK_MAX_INTERESTS 64
int nrl_topk_interest_scores(const float* interests, const float* gate, const float* table, int64_t B, int32_t K, int64_t V, int32_t D,
                             int32_t k, int32_t mode, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible,
                             int32_t slices, int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes,
                             void* stream);

/* nrl_topk_ensemble_scores: the same ranking by MANNeR's ensemble of standardised scores (manner_module.py:175-186 with the
 *   candidate list replaced by the table).  T in [1, NRL_TOPK_MAX_MODELS] sub-models, each a user matrix users[t] (B, D) and a table
 *   tables[t] (V, D), all of one shape, fp32, row-major, device, and a weight weights[t]; `users`, `tables` (T device pointers each)
 *   and `weights` (T floats) are HOST arrays read during the call, as nrl_manner_scores takes its tables.
 *   Population: P_u = { v in [0, V) : eligible[v] != 0 and v not on the exclusion list of u } -- the candidate list of a
 *     full-catalogue recommendation is every row the user may be recommended.  The exclusion list counts as a set.
 *   Raw score: s_t[u, v] = users[t][u] . tables[t][v], the bits of nrl_topk_scores.
 *   Statistics: mu_t[u] the mean and sd_t[u] the UNBIASED standard deviation (divisor n - 1, as torch.std and nrl_manner_scores)
 *     of s_t[u, v] over the v in P_u whose s_t is not NaN.  out_stats (B, T, 2) receives (mu, sd).
 *   Score: z[u, v] = w_0 ((s_0 - mu_0) / sd_0) + w_1 (...) + w_2 (...), in ascending t, every operation rounded to fp32 on its own
 *     (no contraction): a pure function of the raw-score bits and the user's statistics.  No epsilon is added anywhere.
 *   Ranking: the k rows of P_u of largest z, descending, equal z by ascending row, -1 / -inf where fewer rows qualify; D, k, V, B,
 *     excl_idx / excl_off, eligible, slices, out_idx / out_score as for nrl_topk_scores.
 *   status: NRL_TOPK_E_EXCLUDE and NRL_TOPK_E_OFFSETS as for nrl_topk_scores.  A NaN raw score of a row of P_u sets NRL_TOPK_E_NAN,
 *     stays out of that table's statistics (its n is smaller) and the row is left out for that user.  NRL_TOPK_E_STATS: some
 *     sd_t[u] is zero, NaN, infinite or undefined (fewer than two usable scores): that user's row is all -1 / -inf and the other
 *     users are untouched -- where nrl_manner_scores returns NaN or inf this entry refuses the user and says so.
 *   Invariance: the statistics are reduced in an order planned from V alone.  With nvt = ceil(V / 128) table tiles, a chunk is
 *     ceil(nvt / NRL_TOPK_STAT_CHUNKS) consecutive tiles (at most NRL_TOPK_STAT_CHUNKS chunks, none empty).  Per tile: the masked
 *     count, the sum by the fixed wave reduction, the tile mean, then M2 = sum (s - mean)^2 in a second pass.  Tiles are folded into
 *     the chunk's (n, mean, M2) in ascending order by the pairwise update d = mean_b - mean_a, mean = mean_a + d n_b / n,
 *     M2 = M2_a + M2_b + d d n_a n_b / n (an empty side is skipped), and the chunks in ascending order the same way.  So the bits
 *     of mu, sd and of every returned score and row depend on the user's T rows, the tables, eligible, the exclusion set and V
 *     alone: not on B, the user's position in the batch, k, slices, the grid, the GEMM engine setting or the run.  Neither a (B, V)
 *     matrix nor anything of that order is written.  No floating-point atomics, no allocation, no host synchronisation.
 *   moments: caller-provided device scratch of B * NRL_TOPK_STAT_CHUNKS * T * 3 floats (the chunks' n, mean, M2), overwritten.
 *   Workspace: there is no size function of its own: the partial lists are those of nrl_topk_scores, so
 *     nrl_topk_scores_workspace_bytes(B, V, D, k, slices) is exactly this entry's requirement; a shorter buffer is refused with
 *     NRL_E_WORKSPACE before any launch.  B == 0 returns success without a launch; V == 0 gives NRL_TOPK_E_STATS and -1 / -inf.
 *     T or sizes outside the limits and a null users[t], tables[t], out_stats, moments or status return NRL_E_INVALID. */
#define NRL_TOPK_E_STATS 8 /* a user's scores of some table cannot be standardised: that user's row is all -1 / -inf */
#define NRL_TOPK_MAX_MODELS 3
#define NRL_TOPK_STAT_CHUNKS 64
int nrl_topk_ensemble_scores(const float* const* users, const float* const* tables, const float* weights, int32_t T,
                             int64_t B, int64_t V, int32_t D, int32_t k, const int64_t* excl_idx, const int64_t* excl_off,
                             const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score,
                             float* out_stats /* (B, T, 2): mean, sd */,
                             float* moments   /* (B, NRL_TOPK_STAT_CHUNKS, T, 3) caller-provided scratch */,
                             int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_topk_scores_capped / nrl_topk_ensemble_scores_capped: nrl_topk_scores / nrl_topk_ensemble_scores under a diversity
 *   constraint on the list itself: the k best rows of a user with at most max_per_class of any one class.  Every argument of the
 *   uncapped entry keeps its meaning; two are added behind k:
 *   row_class (V int32, device): the class of every table row (a category, a subcategory, a sentiment class).  Every int32 value
 *     is a class of its own; rows with equal values share a cap.
 *   max_per_class: m >= 1.
 *   Selection: of the rows of user u that are inside V, eligible, not on u's exclusion list and not NaN-scored, ordered by the
 *     family's strict total order (score descending, equal scores by ascending row, -0 == +0), a row is taken if and only if fewer
 *     than m rows of its class have been taken before it; the first k taken are returned.  The tail is -1 / -inf when fewer
 *     qualify, which now also happens when sum_c min(m, n_c) < k.  Excluded, ineligible and NaN rows never count toward a cap.
 *     That list is the top k of the union of the classes' top-m sets: a pure function of the score bits, the row numbers and the
 *     class ids, whatever B, slices, the grid or the GEMM engine setting.  With m >= k the result is the uncapped entry's, bit
 *     for bit.  The ensemble's statistics are those of the uncapped entry: the population does not know the cap.
 *   k in [1, NRL_TOPK_CAP_MAX_K]: a capped list lives in one register per lane.  status: the flags of the uncapped entry, no new one.
 *   Workspace: that of the uncapped entry, nrl_topk_scores_workspace_bytes(B, V, D, k, slices): the classes are re-read from
 *     row_class when a list is loaded and are stored nowhere.  No (B, V) matrix, no floating-point atomics, no allocation, no host
 *     synchronisation.
 *   Checks: those of the uncapped entry in their order, then k > NRL_TOPK_CAP_MAX_K, a null row_class (with V > 0) or
 *     max_per_class < 1 return NRL_E_INVALID.  B == 0 and V == 0 as in the uncapped entries. */
#define NRL_TOPK_CAP_MAX_K 64
int nrl_topk_scores_capped(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k,
                           const int32_t* row_class, int32_t max_per_class, const int64_t* excl_idx, const int64_t* excl_off,
                           const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score, int32_t* status, void* ws,
                           size_t ws_bytes, void* stream);
int nrl_topk_ensemble_scores_capped(const float* const* users, const float* const* tables, const float* weights, int32_t T,
                                    int64_t B, int64_t V, int32_t D, int32_t k, const int32_t* row_class, int32_t max_per_class,
                                    const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                                    int64_t* out_idx, float* out_score, float* out_stats /* (B, T, 2): mean, sd */,
                                    float* moments /* (B, NRL_TOPK_STAT_CHUNKS, T, 3) caller-provided scratch */,
                                    int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_topk_bias_scores / nrl_topk_bias_scores_capped / nrl_catalogue_bias_ranks: nrl_topk_scores / nrl_topk_scores_capped /
 *   nrl_catalogue_ranks by a dot product plus a per-(user, class) additive term: the soft counterpart of the class cap (a user's
 *   category-affinity prior, a sentiment penalty) and the combined score SentiDebias's generator is trained on,
 *   u_free . n_v + (u_aware T^T)[u, sentiment(v)].  Every argument of the dot-product entry keeps its meaning; three are added
 *   behind D:
 *   bias (B, S) fp32, row-major, device: the term of user u and class c is bias[u * S + c].
 *   row_class (V int32, device): the class of every table row, for the bias.
 *   S in [1, NRL_TOPK_MAX_BIAS_CLASSES]: a workgroup keeps the bias rows of its 64 users in LDS.
 *   Score: score(u, v) = fl32(dot(u, v) + bias[u, row_class[v]]): dot(u, v) is the value of nrl_topk_scores for that pair, the same
 *     accumulator chain with the same bits, and the bias is added by ONE fp32 add behind the chain (never as a further k step).
 *     So with an all +0 bias the rows are those of nrl_topk_scores and the scores compare equal, and a score's bits do not depend
 *     on B, V, k, slices, the grid or the GEMM engine setting.
 *   A class id outside [0, S), negative ids included: the row is scored with bias +0 and NRL_TOPK_E_CLASS is ORed into status
 *     (for any such row inside V, eligible or not).  Nothing is read back and nothing is validated on the host.
 *   Order, exclusion lists, eligible, -1 / -inf padding, slices, the other flags and the workspace
 *     (nrl_topk_scores_workspace_bytes / nrl_catalogue_ranks_workspace_size) are those of the dot-product entries.  A NaN score
 *     (a NaN bias, inf - inf) of an eligible, not excluded row sets NRL_TOPK_E_NAN and the row is left out for that user.
 *   The capped entry adds cap_class (V int32) / max_per_class behind k as nrl_topk_scores_capped does: the cap's classes are an
 *     array of their own (the cap may go by category while the bias goes by sentiment; the same pointer is fine).  With
 *     max_per_class >= k it returns the bits of nrl_topk_bias_scores.
 *   The rank entry: targets, population, out_rank / out_score / out_ranked and NRL_RANK_E_* as for nrl_catalogue_ranks; a target's
 *     score is the same chain over the gathered row and the same single add, so out_score[j] has the bits nrl_topk_bias_scores
 *     returns for that (user, row) and out_rank[j] = r <= k if and only if out_idx[u, r - 1] == tgt_idx[j].
 *   Checks, in this order: those of the dot-product entry under this entry's name; S outside its range, a null bias or a null
 *     row_class with V > 0; for the capped entry those of nrl_topk_scores_capped.  All return NRL_E_INVALID before any launch.
 *     B == 0 returns success without a launch.  No floating-point atomics, no allocation, no host synchronisation. */
#define NRL_TOPK_MAX_BIAS_CLASSES 64
#define NRL_TOPK_E_CLASS 64 /* a class id outside [0, S): that row is scored with bias +0 */
int nrl_topk_bias_scores(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, const float* bias,
                         const int32_t* row_class, int32_t S, int32_t k, const int64_t* excl_idx, const int64_t* excl_off,
                         const uint8_t* eligible, int32_t slices, int64_t* out_idx, float* out_score, int32_t* status, void* ws,
                         size_t ws_bytes, void* stream);
int nrl_topk_bias_scores_capped(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, const float* bias,
                                const int32_t* row_class, int32_t S, int32_t k, const int32_t* cap_class, int32_t max_per_class,
                                const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                                int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes, void* stream);
int nrl_catalogue_bias_ranks(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, const float* bias,
                             const int32_t* row_class, int32_t S, const int64_t* tgt_idx, const int64_t* tgt_off,
                             int64_t n_targets, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible,
                             int32_t slices, int32_t* out_rank /* n_targets */, float* out_score /* n_targets */,
                             int32_t* out_ranked /* B */, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_mmr_rerank (symbol added to ABI v19): greedy Maximal Marginal Relevance over a pool of table rows per user -- the (idx, score)
 *   pair any nrl_topk_* entry returns -- trading relevance against similarity to what is already in the list.
 *   Inputs: pool_idx (B, N) int64, -1 = an empty slot; pool_score (B, N) fp32; table (V, D) fp32; k, lambda (fp32), similarity
 *     (0 = cosine, 1 = dot), normalize (0 / 1).
 *   Limits: 1 <= k <= N <= NRL_MMR_MAX_POOL = 128; D as for nrl_topk_scores, a multiple of 4 in [4, 1024]; lambda in [0, 1].
 *   Live slots: slot i of user u is live when its row is in [0, V) and its score is finite.  A row other than -1 outside [0, V) is
 *     dead and ORs NRL_MMR_E_ROW (1) into status; a NaN or +-inf score in a slot with a valid row is dead and ORs NRL_TOPK_E_NAN
 *     (4); a live slot whose own Gram diagonal is not finite is dead and ORs 4.  The pool need not be sorted.  Duplicate rows are
 *     two slots with similarity 1 (cosine); the kernel does not handle them specially.
 *   Gram matrix: G[i][j] is the exact-fp32 accumulator chain of nrl_topk_scores over the two table rows: it has the bits that entry
 *     returns for that pair, a function of the two rows and D alone, and it is bit-symmetric.
 *   Similarity: dot: sim[i][j] = G[i][j].  Cosine: sim[i][j] = fl(G[i][j] * fl(r_i * r_j)), r_i = fl(1 / fl(sqrt(G[i][i]))), and
 *     r_i = 0 where G[i][i] == 0.  Every operation is one correctly rounded fp32 operation (the operations __fsqrt_rn, __fdiv_rn,
 *     __fmul_rn, __fsub_rn name); nothing contracts to an fma.  A float32 numpy restatement reproduces the bits.
 *   Relevance: normalize = 0: rel_i = score_i.  normalize = 1: rel_i = fl(fl(score_i - s_min) / fl(s_max - s_min)) over the user's
 *     live slots (a -0 extreme counts as +0); all rel_i are +0 when s_max == s_min.
 *   Greedy steps t = 0 ... k - 1, pen_i = +0 before anything is selected.  After selecting c: the first selection sets
 *     pen_i = sim[c][i], every later one pen_i = max(pen_i, sim[c][i]) -- the true maximum, so it may be negative.
 *     obj_i = fl(fl(lambda * rel_i) - fl(fl(1 - lambda) * pen_i)).  The step selects the live, unselected slot of largest obj;
 *     equal obj (-0 == +0) goes to the lower slot; a NaN obj ranks below every number.
 *   Outputs: out_idx (B, k) int64 the row; out_score (B, k) fp32 that slot's pool_score, bits unchanged; out_mmr (B, k) fp32 the
 *     winning obj; -1 / -inf / -inf once the live slots run out.  status (one int32, required): integer atomicOr only.
 *   Properties: the result for k is a prefix of the result for k' > k.  Nothing depends on B, on the user's place in the batch, on
 *     the GEMM engine setting or on the run.  lambda = 1 with normalize = 0 returns the live slots in (score descending, slot
 *     ascending) order: on a pool that came from nrl_topk_scores, that pool's first k entries bit for bit.  No float atomics, no
 *     workspace, no allocation, no host synchronisation.
 *   Checks, in this order, each NRL_E_INVALID before any launch: negative sizes; N outside [1, 128]; k outside [1, N]; D, V, B
 *     outside the limits of nrl_topk_scores; lambda outside [0, 1] or NaN; similarity / normalize outside {0, 1}; a null status.
 *     B == 0 returns success without a launch.  After that, null pointers among the rest return NRL_E_INVALID; table may be null
 *     only when V == 0. */
#define NRL_MMR_MAX_POOL 128
#define NRL_MMR_E_ROW 1 /* a pool row other than -1 is outside [0, V): that slot is dead */
int nrl_mmr_rerank(const int64_t* pool_idx, const float* pool_score, const float* table, int64_t B, int32_t N, int64_t V, int32_t D,
                   int32_t k, float lambda, int32_t similarity, int32_t normalize, int64_t* out_idx, float* out_score,
                   float* out_mmr, int32_t* status, void* stream);

/* nrl_calibrated_rerank (symbol added to ABI v19): greedy re-ranking of a pool by relevance, MMR's redundancy penalty and a class
 *   calibration term: how close the class counts of the list come to a per-user class target (calibrated recommendation, Steck
 *   2018, with the generalised Jaccard overlap that Personalization@k measures as the closeness).
 *   Inputs: pool_idx (B, N) int64, pool_score (B, N) fp32, table (V, D) fp32, k, lambda, similarity, normalize as for
 *     nrl_mmr_rerank; row_class (V) int32 the class of every table row; target (B, S) fp32 the users' class targets; mu, gamma fp32.
 *   Limits: 1 <= k <= N <= NRL_MMR_MAX_POOL; 1 <= S <= NRL_CAL_MAX_CLASSES = 64; lambda, mu, gamma each in [0, 1] and not NaN;
 *     with mu != 0, D as for nrl_mmr_rerank.
 *   Live slots, rel_i (normalize 0 / 1), the Gram matrix G, sim (cosine / dot), the tie order (equal obj: the lower slot) and the
 *     NaN order (a NaN obj ranks below every number) are word for word those of nrl_mmr_rerank, with its flags NRL_MMR_E_ROW (1)
 *     and NRL_TOPK_E_NAN (4).
 *   mu == 0: no Gram matrix is computed, table may be null and is never read, D and similarity are neither checked nor used (V
 *     still bounds the rows), the launch needs no tile LDS, and pen_i is +0 at every step.  A slot is then dead only for a row
 *     outside [0, V) or a non-finite score: there is no Gram diagonal to be non-finite.
 *   Class of a slot: class_i = row_class[row_i] for a live slot.  Outside [0, S), negative ids included, the slot stays live, its
 *     calibration term is +0, it counts for no class and NRL_TOPK_E_CLASS (64) is ORed into status.
 *   Target: t_j = target[u][j] where that is finite and >= 0; otherwise t_j = +0 and NRL_CAL_E_TARGET (128) is ORed.
 *   Calibration term: with n_j the number of already selected slots of class j (an integer <= k, exact in fp32), for a class c
 *     M_c = sum_j min(n_j + [j == c], t_j), X_c = sum_j max(n_j + [j == c], t_j), each sum a chain of single fp32 additions in
 *     ascending j = 0 ... S - 1 from +0, and cal_c = fl(M_c / X_c), one correctly rounded division.  X_c >= 1, so nothing divides
 *     by zero, and 0 <= cal_c <= 1.  cal_c is the Personalization value of the list after adding a slot of class c.
 *   Greedy steps t = 0 ... k - 1, pen as in nrl_mmr_rerank (+0 before anything is selected, the true maximum of sim afterwards):
 *     obj_i = fl( fl( fl(lambda * rel_i) - fl(mu * pen_i) ) + fl(gamma * cal_{class_i}) ), every operation one correctly rounded
 *     fp32 operation, none contracted to an fma.  The step selects the live, unselected slot of largest obj.
 *   Outputs: out_idx (B, k) int64 the row; out_score (B, k) fp32 that slot's pool_score, bits unchanged; out_obj (B, k) fp32 the
 *     winning obj; out_cal (B, k) fp32 the winner's calibration term (+0 for a class outside [0, S)); -1 / -inf / -inf / -inf once
 *     the live slots run out.  status (one int32, required): integer atomicOr only.  No workspace, no float atomics, no
 *     allocation, no host synchronisation.
 *   Properties:
 *     1. The result for k is a prefix of the result for k' > k.
 *     2. Nothing depends on B, on the user's place in the batch, on the GEMM engine setting or on the run.
 *     3. With gamma = 0 and mu = fl(1 - lambda) the rows and scores are those of nrl_mmr_rerank(lambda) and out_obj compares equal
 *        to its out_mmr (a -0 there may be +0 here).  At lambda = 1 that is the mu == 0 form, which computes no Gram matrix: the
 *        statement then needs a pool whose Gram matrix is finite.
 *     4. With gamma = 0, mu = 0, lambda = 1, normalize = 0 the output is the pool's live slots in (score descending, slot
 *        ascending) order, and out_obj compares equal to out_score.
 *     5. For a user who raised no flag and whose list is full, out_cal[u][k - 1] has the bits of
 *        fl( sum_j min(cnt_j, t_j) / sum_j max(cnt_j, t_j) ) over the class counts cnt of the k listed slots (the sums as above).
 *        With the integer class counts of the user's history as the target that is Personalization@k of the list.
 *   Checks, in this order, each NRL_E_INVALID before any launch: negative sizes (B, N, V, S, k); N outside [1, 128]; k outside
 *     [1, N]; S outside [1, 64]; V, B outside the limits of nrl_topk_scores; lambda, then mu, then gamma outside [0, 1] or NaN;
 *     normalize outside {0, 1}; with mu != 0 only: D outside the limits of nrl_topk_scores, then similarity outside {0, 1}; a null
 *     status.  B == 0 returns success without a launch.  After that, null pointers among the rest return NRL_E_INVALID;
 *     row_class may be null only when V == 0, table only when V == 0 or mu == 0. */
#define NRL_CAL_MAX_CLASSES 64
#define NRL_CAL_E_TARGET 128 /* a target entry is negative, NaN or infinite: it is taken as +0 */
int nrl_calibrated_rerank(const int64_t* pool_idx, const float* pool_score, const float* table, int64_t B, int32_t N, int64_t V,
                          int32_t D, const int32_t* row_class, const float* target, int32_t S, int32_t k, float lambda, float mu,
                          float gamma, int32_t similarity, int32_t normalize, int64_t* out_idx, float* out_score, float* out_obj,
                          float* out_cal, int32_t* status, void* stream);

/* nrl_dpp_rerank (symbol added to ABI v19): greedy re-ranking of a pool by a determinantal point process (DPP), the set-level
 *   diversifier beside the pairwise nrl_mmr_rerank: the fast greedy MAP inference of Chen, Zhang and Zhou (NeurIPS 2018), an
 *   incremental Cholesky factorisation of the kernel matrix L = diag(q) sim diag(q), q_i a slot's quality and sim the similarity of
 *   the pool's table rows.  Each step lists the slot that multiplies det L_S of the listed set S by the most: a slot that is a
 *   mixture of listed ones gains little even where it is close to none of them.
 *   Inputs: pool_idx (B, N) int64, pool_score (B, N) fp32, table (V, D) fp32, k, similarity, normalize as for nrl_mmr_rerank;
 *     quality (B, N) fp32 or NULL; alpha, eps fp32.
 *   Limits: 1 <= k <= min(N, NRL_DPP_MAX_K = 64); N <= NRL_MMR_MAX_POOL; D, V, B as for nrl_mmr_rerank; alpha finite and >= 0;
 *     eps in [0, 1); similarity and normalize in {0, 1}.
 *   Live slots, the Gram matrix G, sim (cosine / dot, r_i) and rel_i (normalize 0 / 1) are word for word those of nrl_mmr_rerank,
 *     with its flags NRL_MMR_E_ROW (1) and NRL_TOPK_E_NAN (4): the row range check, the finite-score check, then (after the
 *     quality check below) the Gram diagonal check.
 *   Quality: with quality given, q_i = quality[u][i], read for a slot with a valid row and a finite score; a NaN, infinite or
 *     negative entry makes that slot dead and ORs NRL_DPP_E_QUALITY (256); -0 is taken as a zero.  alpha and normalize are then
 *     checked but not used.  With quality NULL, q_i = expf(fl(alpha * rel_i)): the device expf of the single product.  This is the
 *     ONE operation whose bits this header does not fix; every bit-for-bit statement here holds for a given quality.
 *     alpha = theta / (2 (1 - theta)) is the trade-off theta of Chen et al. (their kernel has q_i = exp(alpha r_i)): alpha = 0
 *     ranks by diversity alone, a large alpha by relevance.
 *   Kernel matrix: L[i][j] = fl(fl(q_i * q_j) * sim[i][j]), bit-symmetric.  A live slot whose L[i][i] is not finite is dead and
 *     ORs 4.
 *   State of slot i: d2_i = L[i][i], thr_i = fl(eps * L[i][i]); cv[s][i] the Cholesky rows.
 *   Greedy step t = 0, 1, ...: a slot is eligible when it is live, unselected, d2_i > 0 and d2_i >= thr_i (a NaN d2 satisfies
 *     neither, so it ranks below every number).  The step selects the eligible slot c of largest d2; equal d2 goes to the lower
 *     slot.  Then, for every other live, unselected slot i:
 *       acc     = the chain from +0 over s = 0 ... t - 1, ascending, of acc = fl(acc + fl(cv[s][c] * cv[s][i]))
 *       e_i     = fl(fl(L[c][i] - acc) / fl(sqrt(d2_c)))
 *       cv[t][i] = e_i
 *       d2_i    = fl(d2_i - fl(e_i * e_i))
 *     Every operation is one correctly rounded fp32 operation (the operations __fadd_rn, __fsub_rn, __fmul_rn, __fdiv_rn,
 *     __fsqrt_rn name), subnormal results kept; nothing contracts to an fma.  A float32 numpy restatement reproduces the bits.
 *   Fill phase: at the first step with no eligible slot the DPP phase is over for good (in exact arithmetic the listed set then
 *     spans every slot left, up to eps).  The remaining live, unselected slots are listed by pool_score descending, slot ascending
 *     (-0 counts as +0) with out_gain +0, and NRL_DPP_E_RANK (512) is ORed if at least one slot among the k is listed this way.
 *   Outputs: out_idx (B, k) int64 the row; out_score (B, k) fp32 that slot's pool_score, bits unchanged; out_gain (B, k) fp32 the
 *     winning d2, the marginal determinant ratio det L_{S + c} / det L_S; -1 / -inf / -inf once the live slots run out.  status
 *     (one int32, required): integer atomicOr only.
 *   Properties:
 *     1. The result for k is a prefix of the result for k' > k (the status word may gain NRL_DPP_E_RANK).
 *     2. Nothing depends on B, on the user's place in the batch, on the GEMM engine setting or on the run.
 *     3. The product of a user's DPP-phase gains is det L_S of the listed set S up to rounding.
 *     4. Cosine: after a row is listed, a live slot that duplicates it has a d2 at rounding-noise level (a few 2^-24 L[i][i]; +0
 *        where the step's arithmetic is exact), so with eps above that level -- 1e-4 is -- it is never chosen in the DPP phase.
 *        With eps = 0 the sign of that noise decides.
 *     5. No workspace, no float atomics, no allocation, no host synchronisation.
 *   Checks, in this order, each NRL_E_INVALID before any launch: negative sizes; N outside [1, 128]; k outside [1, min(N, 64)];
 *     alpha negative, infinite or NaN; eps outside [0, 1) or NaN; D, V, B outside the limits of nrl_topk_scores; similarity /
 *     normalize outside {0, 1}; a null status.  B == 0 returns success without a launch.  After that, null pointers among the
 *     rest return NRL_E_INVALID; quality may be null (see above); table may be null only when V == 0. */
#define NRL_DPP_MAX_K 64
#define NRL_DPP_E_QUALITY 256 /* a quality entry is negative, NaN or infinite: that slot is dead */
#define NRL_DPP_E_RANK 512    /* no slot was eligible before the list was full: the rest is listed by pool score, gain +0 */
int nrl_dpp_rerank(const int64_t* pool_idx, const float* pool_score, const float* quality /* (B, N) or null */,
                   const float* table, int64_t B, int32_t N, int64_t V, int32_t D, int32_t k, float alpha, float eps,
                   int32_t similarity, int32_t normalize, int64_t* out_idx, float* out_score, float* out_gain,
                   int32_t* status, void* stream);

/* nrl_topk_relu_scores: the same ranking by DKN's DNN click predictor (click_predictor.py:14-45: Linear(2 dim, Hd) -> ReLU ->
 *   Linear(Hd, 1) on [cand; user]) with the candidate list replaced by the table.  The first layer splits by columns,
 *   pred_w1 = [Wc | Wu], so with q (B, Hd) = user Wu^T + b1 (nrl_dkn_user_query) and proj (V, Hd) = table Wc^T
 *   (nrl_dkn_cand_project), both fp32, row-major, device:
 *     score(u, v) = b2 + sum_j w2[j] relu(proj[v, j] + q[u, j]).
 *   w2 (Hd) and b2 (one float) are DEVICE pointers (the module's parameters: nothing is read back).  Hd in
 *   [1, NRL_TOPK_MAX_HIDDEN], any value (no multiple-of-4 requirement); k, V, B, excl_idx / excl_off, eligible, slices,
 *   out_idx / out_score and status as for nrl_topk_scores.
 *   Arithmetic, fixed: x = proj[v, j] + q[u, j] (one fp32 addition); h_j = x < 0 ? 0 : x, so a NaN x stays NaN (unlike the
 *     fmaxf of nrl_dkn_click_fwd, which turns it into 0); s = b2, then s = fmaf(w2[j], h_j, s) for j = 0 ... Hd - 1: the order of
 *     nrl_dkn_click_fwd's last stage.  The bits of score(u, v) depend on q[u], proj[v], w2, b2 and Hd alone: not on B, V, k,
 *     slices, the grid or the GEMM engine setting (which this entry does not read).  A NaN score of an eligible, not excluded
 *     row sets NRL_TOPK_E_NAN and the row is left out for that user.  Plain vector loads / stores and LDS; no floating-point
 *     atomics, no allocation, no host synchronisation; neither (B, V) nor (B, V, Hd) is written.
 *   Workspace: there is no size function of its own: the partial lists are those of nrl_topk_scores, so
 *     nrl_topk_scores_workspace_bytes(B, V, 4, k, slices) -- D = 4 stands in, the size does not depend on D and Hd need not be
 *     a D that function accepts -- is exactly this entry's requirement; a shorter buffer is refused with NRL_E_WORKSPACE before
 *     any launch.  B == 0 returns success without a launch; V == 0 fills the output with -1 / -inf.  Sizes outside the limits and
 *     a null status, w2 or b2 return NRL_E_INVALID. */
#define NRL_TOPK_MAX_HIDDEN 64
int nrl_topk_relu_scores(const float* q, const float* proj, const float* w2, const float* b2, int64_t B, int64_t V, int32_t Hd,
                         int32_t k, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                         int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_topk_pooled_scores: the same ranking by NPA's eval-mode score (text.py:385-390 and user/npa.py with the candidate list
 *   replaced by the table), from the cached conv feature maps `features` (V, L, F) of nrl_npa_conv_features: with
 *     a[u, v, t] = features[v, t, :] . q[u]          q (B, F): the users' tanh'd candidate-side text queries
 *     s[u, v, t] = features[v, t, :] . user[u]       user (B, F): the user vectors (nrl_npa_cached_scores reports them)
 *     score(u, v) = sum_t softmax_t(a[u, v, :])[t] s[u, v, t],
 *   the dot product of user[u] with the news vector pooled by the user's own attention; the softmax runs over all L tokens with no
 *   mask, as nrl_npa_cached_scores pools.  All three fp32, row-major, device, 16-byte aligned; V * L * F is addressed in int64.
 *   L in [1, NRL_TOPK_MAX_TOKENS]; F a multiple of 4 in [4, NRL_TOPK_MAX_D]; k, V, B, excl_idx / excl_off, eligible, slices,
 *   out_idx / out_score and status as for nrl_topk_scores.
 *   Arithmetic, fixed: each a and s is the one exact-fp32 MFMA accumulator chain of nrl_topk_scores over F; the tokens are folded
 *     in ascending t into an online softmax, m' = fmaxf(m, a); r = exp(m - m'); p = exp(a - m'); l = fmaf(l, r, p);
 *     o = fmaf(o, r, p * s) from m = -inf, l = o = 0 (exp: the fast device exponential nrl_npa_cached_scores pools with), then one
 *     fp32 division o / l.  The bits of score(u, v) depend on q[u], user[u], the (L, F) map of v, L and F alone: not on B, V, k,
 *     slices, the user's place in the batch, the grid or the GEMM engine setting (which this entry does not read).  A NaN anywhere
 *     in the map (through p: fmaxf alone would drop a NaN logit) and inf - inf make the score NaN; a NaN score of an eligible, not
 *     excluded row sets NRL_TOPK_E_NAN and the row is left out for that user.  Neither (B, V, L) nor (B, V, F) is written.  No
 *     floating-point atomics, no allocation, no host synchronisation.
 *   Workspace: there is no size function of its own: the partial lists are those of nrl_topk_scores, so
 *     nrl_topk_scores_workspace_bytes(B, V, 4, k, slices) is exactly this entry's requirement; a shorter buffer is refused with
 *     NRL_E_WORKSPACE before any launch.  B == 0 returns success without a launch; V == 0 fills the output with -1 / -inf.  Sizes
 *     outside the limits and a null status, q, user or features return NRL_E_INVALID. */
#define NRL_TOPK_MAX_TOKENS 128
int nrl_topk_pooled_scores(const float* q, const float* user, const float* features, int64_t B, int64_t V, int32_t L, int32_t F,
                           int32_t k, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                           int64_t* out_idx, float* out_score, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_catalogue_ranks: where held-out rows (the clicks of a test split) land when a user is ranked against the whole table: the
 *   evaluation counterpart of nrl_topk_scores, with its scores, its order and its masks, again without the (B, V) matrix.
 *   user_vec, table, B, V, D, excl_idx / excl_off (and the trust in excl_off[B]), eligible, slices and the flags
 *   NRL_TOPK_E_EXCLUDE / NRL_TOPK_E_OFFSETS / NRL_TOPK_E_NAN as for nrl_topk_scores; duplicates and empty exclusion lists are
 *   fine and a duplicate exclusion entry removes its row once.
 *   Population: P_u = { v in [0, V) : eligible[v] != 0, v not on u's exclusion list, score(u, v) not NaN }.
 *     out_ranked[u] = |P_u| (0 for a user NRL_TOPK_E_OFFSETS refuses).
 *   Order: that of nrl_topk_scores: entry = score_key(score) << 32 | ~row, larger is better, so equal scores rank by ascending
 *     row and -0 equals +0.
 *   Targets: tgt_idx (n_targets int64) / tgt_off ((B + 1) int64; nullable only with n_targets == 0 and a null tgt_idx), a ragged
 *     per-user list laid out like the exclusion list: user b owns the slots tgt_off[b] .. tgt_off[b + 1].
 *     out_rank[j] = 1 + the number of rows of P_u whose entry is strictly above target j's entry; 0 when the target row is not
 *     itself in P_u (outside [0, V), ineligible, on the exclusion list or NaN-scored).  out_score[j] is the target's score, -inf
 *     when the rank is 0.  Other targets of the same user are ordinary rows; the same row listed twice gets the same rank twice.
 *   Bit identity: a score's bits are a function of the two rows and D alone (see nrl_topk_scores: one accumulator chain of the
 *     exact-fp32 MFMA, whatever the place of the rows in a tile); the target scores are computed by that same tile product over
 *     the gathered target rows, so out_score[j] has the bits nrl_topk_scores returns for that (user, row) and for every
 *     k <= NRL_TOPK_MAX_K: out_rank[j] = r <= k if and only if out_idx[u, r - 1] == tgt_idx[j].
 *   NRL_RANK_E_TARGETS: a user whose tgt_off decreases or leaves [0, n_targets], or who owns more than NRL_RANK_MAX_TARGETS
 *     slots, has ranks 0 and scores -inf; the other users are untouched and out_ranked is written for every user.  (Ranges can
 *     overlap only where the offsets decrease somewhere; a slot two sound ranges claim belongs to the later user, and a slot
 *     nobody owns holds 0 / -inf.)  NRL_RANK_E_TARGET_ROW: a target index outside [0, V): its rank is 0.
 *   Determinism: the counts are integers and the scores single chains: nothing depends on B, the batch split, slices, the grid or
 *     the GEMM engine setting.  No floating-point atomics, no allocation, no host synchronisation.
 *   Workspace: nrl_catalogue_ranks_workspace_size (callable without a device; named _size because the set of *_workspace_bytes
 *     functions is the one tests/data/workspace_sizes.json pins -- this one has its own table,
 *     tests/data/catalogue_rank_workspace_sizes.json): the gathered rows n_targets * D * 4, and
 *     (B + n_targets) * slices * 4 of per-slice counts, each region rounded up to 256; never O(B * V).  B == 0 returns success
 *     without a launch; V == 0 gives ranks 0 and out_ranked 0; n_targets == 0 still fills out_ranked.  Sizes outside the limits
 *     of nrl_topk_scores, n_targets >= 2^31, a null status and tgt_idx without tgt_off return NRL_E_INVALID, a short workspace
 *     NRL_E_WORKSPACE, all before any launch. */
#define NRL_RANK_MAX_TARGETS 32
#define NRL_RANK_E_TARGETS 16     /* tgt_off decreases / leaves [0, n_targets], or a user owns more than NRL_RANK_MAX_TARGETS */
#define NRL_RANK_E_TARGET_ROW 32  /* a target index outside [0, V): its rank is 0 */
size_t nrl_catalogue_ranks_workspace_size(int64_t B, int64_t V, int32_t D, int64_t n_targets, int32_t slices);
int nrl_catalogue_ranks(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D,
                        const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets,
                        const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                        int32_t* out_rank /* n_targets */, float* out_score /* n_targets */, int32_t* out_ranked /* B */,
                        int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_topk_window_scores / nrl_catalogue_window_ranks: nrl_topk_scores / nrl_catalogue_ranks with a time window of its own per user.
 *   Row v belongs to user u's population iff it does under the plain entries' rules (inside V, eligible, not on u's exclusion list,
 *   a score that is not NaN) and win_lo[u] <= row_time[v] <= win_hi[u].
 *     row_time (V) int32, win_lo / win_hi (B) int32, in any one unit; the interval is closed; (INT32_MIN, INT32_MAX) is no window;
 *     win_lo[u] > win_hi[u] is an empty window and a legitimate answer: a list of -1 / -inf, population 0, every rank 0, no flag.
 *   Scores, order (ties by ascending row, +0 for -0), slots beyond the population, determinism and the status bits are those of the
 *     plain entries; the score bits are theirs too (the window is applied to what the dot product has produced, never inside it).
 *     A target outside its owner's window has rank 0 and score -inf without a flag, like an ineligible target; NRL_TOPK_E_NAN is
 *     set only for a NaN score of a row inside that user's window.
 *   A table tile none of whose eligible rows has a time inside the union of the windows of the workgroup's 64 users is not read and
 *     not multiplied: on a table stored in time order the cost falls with the width of the windows.
 *   Workspace: nrl_topk_scores_workspace_bytes(B, V, D, k, slices) / nrl_catalogue_ranks_workspace_size(B, V, D, n_targets, slices),
 *     with the layouts of the plain entries.
 *   Checks (NRL_E_INVALID before any launch): those of the plain entry in its order, then row_time with V > 0, then win_lo and
 *     win_hi with B > 0. */
int nrl_topk_window_scores(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k,
                           const int32_t* row_time /* V */, const int32_t* win_lo /* B */, const int32_t* win_hi /* B */,
                           const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                           int64_t* out_idx /* B, k */, float* out_score /* B, k */, int32_t* status, void* ws, size_t ws_bytes,
                           void* stream);
int nrl_catalogue_window_ranks(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D,
                               const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets,
                               const int32_t* row_time /* V */, const int32_t* win_lo /* B */, const int32_t* win_hi /* B */,
                               const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                               int32_t* out_rank /* n_targets */, float* out_score /* n_targets */, int32_t* out_ranked /* B */,
                               int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_topk_sampled_scores / nrl_gumbel_noise: Gumbel top-k.  One draw without replacement from the Plackett-Luce policy over
 *   softmax(s / temperature) per user -- the k rows of the user's population with the largest perturbed key z = s * inv_temp + g --
 *   without the (B, V) score matrix and without a (B, V) matrix of noise.
 *   The noise (normative).  M = 2^32, lowbias32 the hash of the dropout masks (x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15;
 *     x *= 0x846CA68B; x ^= x >> 16, mod M), seed uint64, key = user_key[u] reinterpreted as uint64, row the table row (< 2^31):
 *       k0 = lowbias32((seed & 0xFFFFFFFF) ^ lowbias32(((seed >> 32) + 0x9E3779B9) mod M))          per call
 *       ku = lowbias32((key & 0xFFFFFFFF) ^ lowbias32((key >> 32) ^ k0))                             per user
 *       h  = lowbias32((row * 0x9E3779B1 + ku) mod M)                                               per (user, row)
 *       m  = h >> 9;  u = (2 m + 1) * 2^-24  (exact in fp32, 2^-24 <= u <= 1 - 2^-24: both logs are finite)
 *       x  = fl32(-log(u));  g = fl32(-log(x)): fp32, an accurate logf twice -- each log is evaluated in float64 and rounded once to
 *            fp32 (within half an ulp and a bit; the library's logf, up to 2 ulp, lets the two errors add up to 2^-21.9 max(1, |g|),
 *            and the fast intrinsic is off by the size of g itself near u = 1).
 *     z = fadd_rn(fmul_rn(s, inv_temp), g): s the bits nrl_topk_scores computes for the pair, two separate roundings, no fma.
 *     inv_temp (fp32, finite, >= 0) is 1 / temperature; 0 is legitimate: a uniformly random ordered k-subset of the population.
 *     u has 23 random bits, so two rows of one user can share a g; equal z then rank by ascending row like equal scores.
 *   Population, excl_idx / excl_off, eligible, slices, the order (z descending, equal z by ascending row), the -1 / -inf fill and
 *     the status bits are those of nrl_topk_scores with z in place of the score: a NaN z (a NaN s, or an infinite s with
 *     inv_temp == 0) is left out and sets NRL_TOPK_E_NAN.
 *   out_idx (B, k) int64; out_key (B, k) fp32: z; out_score (B, k) fp32: the raw score -- the bits nrl_topk_scores reports for
 *     (b, out_idx[b, j]) (the same accumulator chain over the same two rows, -0 as +0), -inf where out_idx is -1.
 *   Determinism: a user's lists are a pure function of (seed, its key, its vector, the table, its masks, inv_temp): they do not
 *     depend on B, the user's place in the batch, slices, the grid, the GEMM engine setting or what was sampled before.  No
 *     floating-point atomics, no allocation, no host synchronisation.
 *   Workspace: nrl_topk_sampled_scores_workspace_size (`_size`, as the rank entries' functions: the set of *_workspace_bytes names
 *     is pinned) == nrl_topk_scores_workspace_bytes: the partial lists; the raw scores read the selected rows in place, nothing is
 *     gathered.
 *   Checks (NRL_E_INVALID before any launch): those of nrl_topk_scores in its order, then inv_temp not finite or negative,
 *     B * k >= 2^31, and with B > 0 a null output or user_key; a short workspace NRL_E_WORKSPACE.  B == 0 succeeds without a launch.
 * nrl_gumbel_noise: the noise above for n pairs (user_key[i], row[i]) (int64, device; the low 32 bits of row are used) ->
 *   out_u (n) / out_g (n) fp32, either nullable: the device function the sampled walk calls, so the same bits. */
size_t nrl_topk_sampled_scores_workspace_size(int64_t B, int64_t V, int32_t D, int32_t k, int32_t slices);
int nrl_topk_sampled_scores(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k,
                            const int64_t* user_key /* B */, uint64_t seed, float inv_temp, const int64_t* excl_idx,
                            const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int64_t* out_idx /* B, k */,
                            float* out_key /* B, k */, float* out_score /* B, k */, int32_t* status, void* ws, size_t ws_bytes,
                            void* stream);
int nrl_gumbel_noise(const int64_t* user_key /* n */, const int64_t* row /* n */, int64_t n, uint64_t seed, float* out_u /* n */,
                     float* out_g /* n */, void* stream);

/* nrl_topk_sampled_draws: R Gumbel top-k draws per user from ONE walk over the table.
 *   The contract (normative).  Draw r (0 <= r < R) of every user is what nrl_topk_sampled_scores returns for that user under seed
 *     (seed + r) mod 2^64 with every other argument equal: out_idx[b, r, :], out_key[b, r, :] and out_score[b, r, :] match that
 *     call's out_idx[b, :], out_key[b, :] and out_score[b, :] bit for bit, and `status` is the OR of those R calls' words.
 *     Everything nrl_topk_sampled_scores promises therefore holds per draw: the noise statement above (k0 from seed + r), the tie
 *     rule (equal z by ascending row), NaN handling (a NaN z is left out and sets NRL_TOPK_E_NAN), the -1 / -inf / -inf fill, raw
 *     scores with the bits nrl_topk_scores reports, and independence from B, the user's place in the batch, slices, the grid and
 *     the GEMM engine setting.  The dot products are computed once per table tile and perturbed R times; the entry may run the
 *     draws in several walks of fewer draws each, which changes no output bit.
 *   out_idx (B, R, k) int64; out_key (B, R, k) fp32; out_score (B, R, k) fp32.
 *   Limits: R in [1, NRL_TOPK_MAX_DRAWS], R * k <= NRL_TOPK_MAX_K, B * R * k < 2^31.
 *   Workspace: nrl_topk_sampled_draws_workspace_size(B, V, D, k, R, slices) == nrl_topk_scores_workspace_bytes(B, V, D, R * k,
 *     slices): R lists of k entries are one list of R k (`_size`: the set of *_workspace_bytes names is pinned).  A shorter buffer
 *     is refused with NRL_E_WORKSPACE before any launch.
 *   Checks (NRL_E_INVALID before any launch): those of nrl_topk_sampled_scores in its order up to B * k >= 2^31, then the limits
 *     above, then with B > 0 a null output or user_key.  B == 0 succeeds without a launch; V == 0 gives -1 / -inf / -inf.
 *   No floating-point atomics, no allocation, no host synchronisation. */
#define NRL_TOPK_MAX_DRAWS 32
size_t nrl_topk_sampled_draws_workspace_size(int64_t B, int64_t V, int32_t D, int32_t k, int32_t R, int32_t slices);
int nrl_topk_sampled_draws(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, int32_t k, int32_t R,
                           const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible,
                           const int64_t* user_key /* B */, uint64_t seed, float inv_temp, int32_t slices,
                           int64_t* out_idx /* B, R, k */, float* out_key /* B, R, k */, float* out_score /* B, R, k */,
                           int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* nrl_list_class_exposure: how much position-weighted exposure L lists per user give each of S classes of table rows.
 *   list_idx (B, L, k) int64, -1 an empty slot (the L draws of nrl_topk_sampled_draws, or any lists); row_class (V) int32;
 *   pos_weight (k) fp32; out (B, S) fp32:
 *     out[b, s] = fl32((sum over l ascending, then j ascending, of (double)pos_weight[j] where row_class[list_idx[b, l, j]] == s) / L)
 *   accumulated in float64 in exactly that order, divided by L in float64 and rounded once: a pure function of the user's lists.
 *   A row outside [0, V) other than -1 counts for no class and ORs NRL_MMR_E_ROW (1) into status; a class outside [0, S) counts
 *     for no class and ORs NRL_TOPK_E_CLASS (64).
 *   Checks (NRL_E_INVALID before any launch): S outside [1, NRL_TOPK_MAX_BIAS_CLASSES], k outside [1, NRL_TOPK_MAX_K], L < 1,
 *     B >= 2^31, a null status, and with B > 0 a null argument.  B == 0 succeeds without a launch.  No workspace, no atomics on
 *     floats, no host synchronisation. */
int nrl_list_class_exposure(const int64_t* list_idx /* B, L, k */, const int32_t* row_class /* V */, const float* pos_weight /* k */,
                            int64_t B, int32_t L, int32_t k, int64_t V, int32_t S, float* out /* B, S */, int32_t* status,
                            void* stream);

/* nrl_catalogue_logz / nrl_list_logprob: how probable a list drawn by nrl_topk_sampled_scores was.  The policy is Plackett-Luce over
 *   softmax(t), t = fmul_rn(s, inv_temp): s the bits nrl_topk_scores computes for the pair, t the first rounding of the sampled
 *   entry's key (-0 counts as +0).  Neither the (B, V) scores nor their exponentials are written.
 * nrl_catalogue_logz: per user, over P'_u = the rows inside V that are eligible, not excluded and whose t is finite, minus the rows
 *   of drop_idx[u] (kd slots, -1 an empty slot; null with kd == 0; duplicates and rows outside P_u are harmless):
 *     out_pop[u] = n = |P'_u|;  out_max[u] = m = max t (the bits of one scaled score);  out_logsum[u] = log sum exp(t - m), inside
 *     [0, log n];  out_entropy[u] = log S - (sum (t - m) exp(t - m)) / S, the entropy of softmax(t) over P'_u in nats;
 *     out_dropped[u] (may be null when kd == 0) = the distinct rows of drop_idx[u] that were eligible, not excluded and finite.
 *     log Z = max + logsum; they are returned separately so that log p(row) = (t - max) - logsum keeps its precision.
 *     An empty P'_u: max -inf, logsum -inf, entropy 0, pop 0.
 *   status (one int32, required): NRL_TOPK_E_EXCLUDE / NRL_TOPK_E_OFFSETS as for nrl_topk_scores (a user with bad offsets gets the
 *     outputs of an empty population); a NaN t of a row that is eligible, not excluded and not dropped sets NRL_TOPK_E_NAN, an
 *     infinite one NRL_POLICY_E_INF, and the row is left out.
 *   Determinism: the table is cut into ceil(nvt / tiles_per_chunk) chunks of tiles_per_chunk = ceil(nvt / NRL_TOPK_STAT_CHUNKS)
 *     tiles of 128 rows (nvt = ceil(V / 128)): a function of V alone.  Inside a chunk, lane l of a wave folds columns l and 64 + l of
 *     the tiles in ascending order into its own (m, S, W) -- a new maximum m' rescales by r = exp(m - m'): S' = S r,
 *     W' = (W + (m - m') S) r -- the 64 lane states are merged by a butterfly over lane distances 1, 2, ..., 32, and the chunks are
 *     folded in ascending order in float64, each output rounded to fp32 once.  Every fp32 operation is rounded on its own; exp is the
 *     fast one (for a sum of exponentials the absolute error of a term counts, and |x| e^x <= 1 / e for x <= 0).  So a user's outputs
 *     have the same bits whatever B, the user's place in the batch, the GEMM engine setting and whether eligible is null or all
 *     ones.  No floating-point atomics, no allocation, no host synchronisation.
 *   Workspace: nrl_catalogue_logz_workspace_size(B, V, D) (`_size`: the set of *_workspace_bytes names is pinned): 5 words per (user,
 *     chunk).  Layout and carve are the same code; a short buffer is refused with NRL_E_WORKSPACE before any launch.
 *   Checks (NRL_E_INVALID before any launch): those of nrl_topk_scores on B, V, D and the exclusion pointers, then inv_temp not
 *     finite or negative, kd outside [0, NRL_TOPK_MAX_K], a null status; with B > 0 a null output, and with kd > 0 a null drop_idx or
 *     out_dropped.  B == 0 succeeds without a launch; V == 0 gives empty populations.
 * nrl_list_logprob: the log-probabilities of given lists, list_idx (B, k) int64 with -1 in TRAILING empty slots, against the tail
 *   nrl_catalogue_logz returned under drop_idx = list_idx (the same masks and inv_temp): tail_max / tail_logsum / tail_pop /
 *   tail_dropped (B).  out_score (B, k): the raw scores -- the bits nrl_topk_scores reports for (b, list_idx[b, j]), -inf in an
 *   empty slot.  Then per user in float64, with a_j = fmul_rn(score_j, inv_temp):
 *     R_j = exp(tail_max + tail_logsum) + sum_{i >= j} exp(a_i), accumulated from the last slot backwards and carried as its
 *       logarithm against the running maximum (L' = max(L, a) + log1p(exp(-|L - a|))), so that no term underflows;
 *     out_logp[b, j] = fl32(a_j - log R_j), +0 where slot j is all that is left (and in an empty slot);
 *     out_total[b] = fl32(sum_j of them).
 *   This tail form adds positive terms only; Z - sum_{i < j} exp(t_i) cancels to nothing once the first slots hold the mass.
 *   A list is invalid when it has a hole before a row, a row outside [0, V), a row twice, or a row that is not in the user's
 *     population (tail_dropped[b] differs from the number of its rows): that user's out_logp and out_total are NaN and
 *     NRL_POLICY_E_LIST is ORed into status.
 *   Checks (NRL_E_INVALID before any launch): those of nrl_topk_scores on B, V, D and k, inv_temp, a null status, B * k >= 2^31, and
 *     with B > 0 a null argument.  B == 0 succeeds without a launch.  No workspace. */
#define NRL_POLICY_E_LIST 128 /* an invalid list: that user's log-probabilities are NaN */
#define NRL_POLICY_E_INF 256  /* an infinite scaled score of an eligible, not excluded row: the row is left out for that user */
size_t nrl_catalogue_logz_workspace_size(int64_t B, int64_t V, int32_t D);
int nrl_catalogue_logz(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, float inv_temp,
                       const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible,
                       const int64_t* drop_idx /* (B, kd) or null */, int32_t kd, float* out_max /* B */, float* out_logsum /* B */,
                       float* out_entropy /* B */, int32_t* out_pop /* B */, int32_t* out_dropped /* B, may be null when kd == 0 */,
                       int32_t* status, void* ws, size_t ws_bytes, void* stream);
int nrl_list_logprob(const float* user_vec, const float* table, int64_t B, int64_t V, int32_t D, float inv_temp,
                     const int64_t* list_idx /* B, k */, int32_t k, const float* tail_max /* B */, const float* tail_logsum /* B */,
                     const int32_t* tail_pop /* B */, const int32_t* tail_dropped /* B */, float* out_score /* B, k */,
                     float* out_logp /* B, k */, float* out_total /* B */, int32_t* status, void* stream);

/* nrl_catalogue_interest_ranks / nrl_catalogue_relu_ranks / nrl_catalogue_pooled_ranks: nrl_catalogue_ranks under the scores of
 *   nrl_topk_interest_scores (MINER: interests (B, K, D), gate (B, K, D) or null, mode 0 max / 1 mean / 2 weighted), of
 *   nrl_topk_relu_scores (DKN: q (B, Hd), proj (V, Hd), w2 (Hd), b2 (1), all on the device) and of nrl_topk_pooled_scores (NPA:
 *   q (B, F), user (B, F), features (V, L, F), 16-byte aligned).  Population, order, targets, ownership of slots, flags, blanking rules,
 *   determinism and outputs are those of nrl_catalogue_ranks; shape limits are those of the matching nrl_topk_* call (k aside)
 *   plus NRL_RANK_MAX_TARGETS.
 *   Bit identity: the count walk runs the tile producer of the matching scores kernel (the same device functions), and the target
 *     scores are computed by the same chain -- MINER: the tile product of the owners' K interest (and gate) rows with the gathered
 *     target rows, then the same aggregate; DKN: the chain s = b2; s = fma(w2[j], relu(proj[row, j] + q[u, j]), s) in ascending
 *     j, read in place; NPA: the per-token tile products of the owners' (q, user) rows with the targets' feature maps, read in
 *     place through tgt_idx (nothing is gathered: a map is L F floats), tokens ascending, the same online softmax.  So out_score[j] has the bits the matching nrl_topk_* call returns for that (user, row), and for every
 *     k <= NRL_TOPK_MAX_K: out_rank[j] = r <= k if and only if out_idx[u, r - 1] == tgt_idx[j].  K = 1 (modes 0 and 1) is
 *     nrl_catalogue_ranks bit for bit.  A NaN in a user's interests, gate, q or user vector makes that user's scores NaN: its population is
 *     empty, its ranks are 0 and NRL_TOPK_E_NAN is set; the other users are unchanged.
 *   Workspace: nrl_catalogue_ranks_workspace_size(B, V, D, n_targets, slices) with B in users for the interests (its layout for
 *     64 / K users per workgroup never needs more), nrl_catalogue_ranks_workspace_size(B, V, 4, n_targets, slices) for the DNN
 *     and the pooling scorer (nothing is gathered: O(n_targets + (B + n_targets) slices), whatever L and F).  B == 0, V == 0, n_targets == 0 and the refusals (NRL_E_INVALID, NRL_E_WORKSPACE, before any
 *     launch) as for nrl_catalogue_ranks. */
int nrl_catalogue_interest_ranks(const float* interests, const float* gate, const float* table, int64_t B, int32_t K, int64_t V,
                                 int32_t D, int32_t mode, const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets,
                                 const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible, int32_t slices,
                                 int32_t* out_rank /* n_targets */, float* out_score /* n_targets */, int32_t* out_ranked /* B */,
                                 int32_t* status, void* ws, size_t ws_bytes, void* stream);
int nrl_catalogue_relu_ranks(const float* q, const float* proj, const float* w2, const float* b2, int64_t B, int64_t V, int32_t Hd,
                             const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets, const int64_t* excl_idx,
                             const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int32_t* out_rank /* n_targets */,
                             float* out_score /* n_targets */, int32_t* out_ranked /* B */, int32_t* status, void* ws,
                             size_t ws_bytes, void* stream);
int nrl_catalogue_pooled_ranks(const float* q, const float* user, const float* features, int64_t B, int64_t V, int32_t L, int32_t F,
                               const int64_t* tgt_idx, const int64_t* tgt_off, int64_t n_targets, const int64_t* excl_idx,
                               const int64_t* excl_off, const uint8_t* eligible, int32_t slices, int32_t* out_rank /* n_targets */,
                               float* out_score /* n_targets */, int32_t* out_ranked /* B */, int32_t* status, void* ws,
                               size_t ws_bytes, void* stream);

/* nrl_catalogue_ensemble_ranks: nrl_catalogue_ranks under the scores of nrl_topk_ensemble_scores (MANNeR): the evaluation
 *   counterpart of that entry, again without a (B, V) matrix.
 *   users, tables, weights (HOST arrays of T device pointers / T floats, read during the call), T, B, V, D, the raw scores, the
 *     statistics, the score z, the invariance statement, out_stats (B, T, 2), the caller-provided `moments` scratch
 *     (B * NRL_TOPK_STAT_CHUNKS * T * 3 floats, overwritten) and NRL_TOPK_E_STATS as for nrl_topk_ensemble_scores: the statistics
 *     pass is that entry's, launched over the same chunk plan from V, so out_stats has its bits.
 *   Population (P_u as for nrl_topk_ensemble_scores, less the rows whose z is NaN), order, targets, ownership of slots,
 *     out_rank / out_score / out_ranked, NRL_TOPK_E_EXCLUDE / NRL_TOPK_E_OFFSETS / NRL_TOPK_E_NAN, NRL_RANK_E_TARGETS and
 *     NRL_RANK_E_TARGET_ROW as for nrl_catalogue_ranks.
 *   NRL_TOPK_E_STATS: a user whose scores of some table cannot be standardised has ranks 0, scores -inf and out_ranked 0; its
 *     out_stats row says why.  The other users are untouched.
 *   Bit identity: the count walk runs the tile producer of the ensemble scores kernel (the same device function), and a target's
 *     score is computed by the same chain: per sub-model in ascending t the tile product of the owner's row of users[t] with the
 *     gathered target row of tables[t], folded as w_t ((s - mu_t) / sd_t) by the same rounded operations in the same order.  So
 *     out_score[j] has the bits nrl_topk_ensemble_scores returns for that (user, row), and for every k <= NRL_TOPK_MAX_K:
 *     out_rank[j] = r <= k if and only if out_idx[u, r - 1] == tgt_idx[j].
 *   Determinism: the statistics as above, the counts integers: nothing depends on B, the user's place in the batch, slices, the
 *     grid, the GEMM engine setting or the run.  No floating-point atomics, no allocation, no host synchronisation.
 *   Workspace: nrl_catalogue_ensemble_ranks_workspace_size (callable without a device; its table is
 *     tests/data/catalogue_ensemble_rank_workspace_sizes.json): the layout of nrl_catalogue_ranks with T gathered blocks,
 *     T * n_targets * D * 4, and (B + n_targets) * slices * 4 of per-slice counts, each region rounded up to 256; never O(B * V).
 *     B == 0 returns success without a launch; V == 0 gives ranks 0, out_ranked 0 and NRL_TOPK_E_STATS; n_targets == 0 still
 *     fills out_ranked and out_stats.  Negative sizes, T outside [1, NRL_TOPK_MAX_MODELS], sizes outside the limits of
 *     nrl_topk_scores, n_targets >= 2^31, a null status, tgt_idx without tgt_off, a null users / tables / weights array or
 *     users[t] / tables[t], a null out_stats or moments return NRL_E_INVALID, a short workspace NRL_E_WORKSPACE, all before any
 *     launch. */
size_t nrl_catalogue_ensemble_ranks_workspace_size(int32_t T, int64_t B, int64_t V, int32_t D, int64_t n_targets, int32_t slices);
int nrl_catalogue_ensemble_ranks(const float* const* users, const float* const* tables, const float* weights, int32_t T,
                                 int64_t B, int64_t V, int32_t D, const int64_t* tgt_idx, const int64_t* tgt_off,
                                 int64_t n_targets, const int64_t* excl_idx, const int64_t* excl_off, const uint8_t* eligible,
                                 int32_t slices, int32_t* out_rank /* n_targets */, float* out_score /* n_targets */,
                                 int32_t* out_ranked /* B */, float* out_stats /* (B, T, 2): mean, sd */,
                                 float* moments /* (B, NRL_TOPK_STAT_CHUNKS, T, 3) caller-provided scratch */,
                                 int32_t* status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEWSRECLIB_AMD_H */
