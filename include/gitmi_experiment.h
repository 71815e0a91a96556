/* gitmi_experiment.h -- entry points of the MEASUREMENT builds only (`make exp`: libgitmi_exp.so = the product sources compiled
 * with -DGITMI_EXPERIMENT, bf16 operands; libgitmi_f16_exp.so = the same with -DGITMI_OPS_F16, fp16 operands -- the kernels of
 * the benchmarked configuration, the folded-LayerNorm GEMM forms among them).  libgitmi.so / libgitmi_f16.so do not export them.
 * Both measurement builds export the same 71 gitmi_ symbols (the 40 of gitmi.h + the 31 below); gitmi_operand_dtype tells them apart.
 *
 * What lives here: debug hooks that exchange stage products between contexts (tools/error_attribution.py), force a GEMM
 * variant (tools/gemm_bench.py, tests of the forced tile heights) or set the timing bits of the decode-chain GEMMs
 * (tools/dgemm_bench.py).  The measurement build also reads GITMI_* environment overrides at gitmi_create (kernel shapes,
 * work-skipping switches for timing decompositions); the product libraries read no environment.
 *
 * Removed in round 5 (history and docs/LAB_NOTEBOOK.md keep them): the two-submission split of a call
 * (gitmi_generate_encode / gitmi_generate_decode, bench.py --phased) and decode groups (gitmi_clone_sized,
 * gitmi_set_decode_group, gitmi_group_decode) -- bit-identical to gitmi_generate and measured slower than the default mixed
 * schedule three rounds running (9.1-10.6k against 10.9k captions/s). */
#ifndef GITMI_EXPERIMENT_H_
#define GITMI_EXPERIMENT_H_
#include "gitmi.h"
#ifdef __cplusplus
extern "C" {
#endif

/* decoding constraints for the three hooks that see logits together with the rows' histories (vocab_topm_rules, row_topm,
 * sample_rows; tests/test_gpu_constraints_ops.py): the tables of GITMI_SEARCH_CONSTRAIN (include/gitmi.h; the rule itself:
 * csrc/ban_rules.h) as the engine keeps them for an armed call.  Row r belongs to sentence r / beams.  The hook fills the
 * launcher's BanArgs from it, so the launcher's choice of the BAN instantiation and its refusals are part of what runs.  NULL:
 * the hook behaves and launches exactly as without the argument.  Checked on host copies (the hook synchronises the stream
 * first) and refused by name, nothing launched: ban without ids or plen, W != (V + 31) / 32, n_sets < 0, null set_of / min_new /
 * ngram, words null while some set_of >= 0, a set_of outside [-1, n_sets), min_new < 0, ngram outside [0, 8], eos outside
 * [0, V). */
typedef struct gitmi_debug_ban {
    const uint32_t* words;      /* DEVICE uint32 [n_sets][W]; token c <-> bit c % 32 of word c / 32 */
    int n_sets, W;
    const int32_t *set_of, *min_new, *ngram;   /* DEVICE int32 [rows / beams] */
    int eos;
    const uint32_t* row_words;  /* DEVICE uint32 [rows][W] or NULL (as before the field existed): the rows' own sets of the step
                                 * (banned sequences; the row_words_out form of gitmi_debug_row_topm computes them), read in place of words[set_of]; set_of
                                 * is still checked, words may then be NULL */
    /* gitmi_debug_row_topm only: row_words_out != NULL turns the call into ban_rows_kernel alone (see there) */
    const int32_t* pool_host;   /* HOST int32 [n_pool]: the sequence pool of GITMI_SEARCH_CONSTRAIN's extension */
    int n_pool;
    uint32_t* row_words_out;    /* DEVICE uint32 [rows][W] */
} gitmi_debug_ban;

/* GITMI_EXPERIMENT_TYPES_ONLY: the types above without the entry points (csrc/abi_ops.hip in the product builds, which compile
 * the hooks as unused statics) */
#ifndef GITMI_EXPERIMENT_TYPES_ONLY

/* ---- error attribution hooks (tools/error_attribution.py; not part of the serving path).  Two contexts of the SAME
 * model in different precisions: import_stage hands the products of the image encoder (stage 1) or of encoder + prefill
 * (stage 2: the image K/V of every decoder layer) from `src` to `dst`, converted, so that gitmi_step_logits on `dst`
 * continues from there; head_from applies dst's (bf16, fused) vocabulary head to the last hidden state of src's (fp32)
 * most recent gitmi_step_logits over R rows -> logits_out fp32 [R, vocab] on the device. */
int  gitmi_debug_import_stage(gitmi_engine* dst, gitmi_engine* src, int stage, void* stream);
int  gitmi_debug_head_from(gitmi_engine* dst, gitmi_engine* src, int R, float* logits_out, void* stream);

/* encoder-GEMM selection for A/B measurements (process-wide): low byte -1 auto (default) | 0 register-staged tile kernel
 * only | 9 the LDS-DMA kernel wherever its shape rules hold; bits 8.. = variant / timing bits of the selected kernel
 * (tools/gemm_bench.py lists them: 64 / 128 / 16384 / 32768 / 65536 force the 192- / 256- / 160- / 224- / 128-row tile ...).
 * Any other low byte is refused (returns non-zero, selection unchanged). */
int  gitmi_debug_set_gemm_impl(int impl);

/* timing bits of the decode-chain GEMMs (kernels_dgemm.hip; tools/dgemm_bench.py) for gitmi_op_dgemm / gitmi_op_dgemm_res */
int  gitmi_debug_set_dgemm(int dbg);

/* every launch form of the decode-chain GEMMs (tests/test_gpu_dgemm_forms.py): an argument check + launch_dgemm, the launcher
 * the engine's decode step calls, with the three DGemmArgs fields the engine sets by policy and the gitmi_op_dgemm* hooks leave
 * at 0: rows_per_wg (N = hidden form and N < 1536: 0 / 16, 32, 64), strips_per_wg (wide form at 33..64 rows: 0 / 1, 2, 4, 6)
 * and no_row_walk (wide form above 64 rows: one workgroup per (strip, row block)).  One epilogue per call, the other's pointers
 * NULL: C (gitmi_op_dgemm's arguments: colsum / stats / strips / eps, c_frag, act) or x_out (gitmi_op_dgemm_res's: res_x,
 * res_stats / res_strips / res_gamma / res_beta / res_eps, xb_out, stats_out).  A, W fragment-major 16-bit operands of the
 * build's type; a_rows: the rows allocated behind A, at least round_up(M, 64) (every form loads whole 16-row tiles, up to the
 * next multiple of 64 rows).  Refused by name, nothing launched: null A / W / bias, both or neither of C and x_out, K % 32,
 * a_rows too small, c_frag with N % 32, stats without colsum, strips / res_strips outside 1..64, the x_out epilogue with
 * N % 16 or without xb_out / stats_out / res_x, res_stats without res_gamma / res_beta, arguments of the other epilogue.
 * M == 0 succeeds and launches nothing.  The timing bits of gitmi_debug_set_dgemm do not apply (dbg = 0). */
int  gitmi_debug_dgemm_form(const void* A, int a_rows, const void* W, const float* bias, const float* colsum, const float* stats,
                            int strips, float eps, void* C, int c_frag, int act, const float* res_x, const float* res_stats,
                            int res_strips, const float* res_gamma, const float* res_beta, float res_eps, float* x_out,
                            void* xb_out, float* stats_out, int M, int N, int K, int rows_per_wg, int strips_per_wg,
                            int no_row_walk, void* stream);

/* every launch form of the large-M GEMM and of the tile kernel (tests/test_gpu_gemm_forms.py): an argument check + launch_gemm
 * with everything the engine's gemm_args / gemm_run / ln_gemm / gemm_to_stream set.  A [M][lda], W [N][K] in in_dtype (fp32 or
 * the build's operand type); C [M][ldc] in out_dtype: fp32, the operand type, or GITMI_DTYPE_F16_STREAM (fp16 residual-stream
 * rows; `res` is then fp16 [M][ldr], fp32 otherwise).  A column slice of a wider buffer is ldc > N with C, W, bias and colsum
 * offset by the caller.  shared: the serving policy's tile choice (the 256-row tile).  Folded LayerNorm (fp16-operand build,
 * gemm_p8_kernel: more than 512 rows): consumer = ln_part fp32 [M][4][2] (sum, sumsq) row partials + colsum + ln_eps (K <= 1024,
 * operand-type output, no residual); producer = part_out [M][4][2] (stream rows out, no activation, N <= 1024; slot t = column
 * tile t, slots past N / 256 are not written) and, post-norm, res_part / res_gamma / res_beta / res_eps (the residual added is
 * LayerNorm(res) rebuilt from the partials).  Tile heights and XCD partitions: gitmi_debug_set_gemm_impl.  Refused by name,
 * nothing launched: null A / W / C, lda < K, ldc < N, ldr < N, K % 64 (fp32: % 16), a dtype of the other build, folded
 * arguments in the bf16 build or on a shape the tile kernel would run, colsum without ln_part and the reverse, consumer and
 * producer arguments together, res_part without res / res_gamma / res_beta. */
int  gitmi_debug_gemm_form(const void* A, int lda, const void* W, const float* bias, const void* res, int ldr, void* C, int ldc,
                           int M, int N, int K, int act, int in_dtype, int out_dtype, int shared, const float* ln_part,
                           const float* colsum, float ln_eps, float* part_out, const float* res_part, const float* res_gamma,
                           const float* res_beta, float res_eps, void* stream);

/* op hooks of the caption-scoring kernels (kernels_score.hip; tests/test_gpu_score_ops.py).  dtype: GITMI_DTYPE_F32 (the
 * kernels of the f32 parity mode) or the build's 16-bit operand dtype (gitmi_operand_dtype).
 *   score_attn: text-row attention of one layer -- qkv [Q * Lp][3 H 64] packed q|k|v text rows (sentence q, position j at
 *               row q * Lp + j), img_kv [B * N_img][3 H 64] prefill rows, image_of int32 [Q] -> out [Q * Lp][H 64]; every
 *               text row attends to all N_img image keys of its image and causally to its sentence's text keys, scale 1/8.
 *   score_attn_map: the same operands (ntok: int32 [B] DEVICE, the image keys of every image as in the ragged hooks below, or
 *               NULL) -> out fp32 [Q][Lp][N_img + Lp], the attention map of GITMI_SEARCH_ATTEND for one layer: the head mean of
 *               the probabilities row (q, j) gives the image keys (columns [0, N_img), 0 past ntok) and its text keys (columns
 *               N_img + t, 0 for t > j).  Runs the attention launch for its softmax statistics first; synchronises the stream.
 *   score_head: out fp32 [M][2] = (log_softmax(z)[tgt[m]], mean_c log_softmax(z)[c]) of z = A [M][K] W [V][K]^T + bias for
 *               rows with tgt[m] >= 0 (0 elsewhere).  Synchronises the stream.
 *   score_attn_tree: score_attn with the Lp rows of every "sentence" the nodes of a token tree in DFS pre-order
 *               (GITMI_SEARCH_TREE_SCORE, include/gitmi.h): packed int64 [Q][Lp] DEVICE (depth << 32 | token id), lens int32 [Q]
 *               DEVICE node counts (<= Lp), max_depth the bound of the depths (<= 8192), ntok as in score_attn_map -> out
 *               [Q * Lp][H 64]; every row attends to the image keys and to its own ancestors and itself.  Rows past a tree's
 *               nodes, and every row of a tree that breaks the depth rules, attend to the image and themselves; bad_out int32
 *               [Q] DEVICE (or NULL) = 1 for such a tree.  Runs the structure launch first; synchronises the stream. */
int  gitmi_debug_score_attn(const void* qkv, const void* img_kv, const int* image_of, void* out, int Q, int H, int N_img, int Lp,
                            int dtype, void* stream);
int  gitmi_debug_score_attn_map(const void* qkv, const void* img_kv, const int* image_of, const int* ntok, float* out, int Q, int H,
                                int N_img, int Lp, int dtype, void* stream);
int  gitmi_debug_score_head(const void* A, const void* W, const float* bias, const int* tgt, int M, int V, int K, int dtype,
                            float* out, void* stream);
int  gitmi_debug_score_attn_tree(const void* qkv, const void* img_kv, const int* image_of, const int* ntok, const int64_t* packed,
                                 const int* lens, int max_depth, void* out, int* bad_out, int Q, int H, int N_img, int Lp, int dtype,
                                 void* stream);

/* op hooks of the text pass around its attention and head (kernels_score.hip; tests/test_gpu_text_pass_ops.py): an argument
 * check + the launchers the score / tree-score calls run, in their order.  All pointers DEVICE memory.
 *   score_embed: tokens int64 [Q][ld] -> h_f fp32 [Q * Lp][D] and h_t [Q * Lp][D] (dtype) = LayerNorm(words[id] +
 *                positions[min(j, max_pos - 1)], eps) of row (q, j); ids clamp into [0, vocab), positions j >= ld embed id 0.
 *                node_tok / node_depth int32 [Q * Lp] (both or neither): the tree instantiation -- row i embeds words[node_tok[i]]
 *                + positions[node_depth[i]] and `tokens` is not read; the hook checks both tables on host copies (synchronises).
 *                Refused by name: null or misaligned pointers, D not a multiple of 4 up to 1024, a node outside the tables.
 *   tree_tables: packed int64 [Q][ld] (depth << 32 | token), lens int32 [Q] -> the structure launch's tok / depth / parent / end
 *                int32 [Q * Lp] and bad int32 [Q] (zeroed first).
 *   score_tail:  everything behind the last decoder layer.  A [Q * Lp][K] text rows, W [V][K] (dtype), bias fp32 [V], tokens
 *                int64 [Q][ld] (tree_max_depth > 0: the packed tree table), lens int32 [Q] -> out float2 [Q][ld] (NOT zeroed: only
 *                the entries the combine kernel writes change), bad int32 [Q] (zeroed first), info int32 [4] = {ld, 0, 0, bad
 *                sentences}; tgt_out int32 [Q * Lp] (or NULL): the target of every head row (-1: none; trees: -1 everywhere);
 *                zt_out fp32 [Q * Lp] (or NULL): the logit at the row's target (trees: of the node's token at its parent's row),
 *                NaN where none was stored.  Sentences: targets, head, combine, info; trees: structure, head with the gather,
 *                tree combine, info.  The head is launch_score_head_rows, the engine's own: fp32 in chunks of chunk_rows rows
 *                (GEMM, row statistics, gather), 16-bit the fused head (+ the gather dot).  Refused by name: null pointers, A or W
 *                not 16-byte aligned, K % 32, a dtype of the other build, fp32 with chunk_rows outside [1, Q * Lp], tree_max_depth outside [0, 8192], (sentences) a
 *                length outside [1, ld].  Synchronises the stream. */
int  gitmi_debug_score_embed(const int64_t* tokens, int Q, int ld, int Lp, const float* words, int vocab, const float* positions,
                             int max_pos, const float* gamma, const float* beta, float eps, int D, float* h_f, void* h_t, int dtype,
                             const int* node_tok, const int* node_depth, void* stream);
int  gitmi_debug_tree_tables(const int64_t* packed, const int* lens, int Q, int ld, int Lp, int V, int max_depth, int* tok, int* depth,
                             int* parent, int* end, int* bad, void* stream);
int  gitmi_debug_score_tail(const void* A, const void* W, const float* bias, const int64_t* tokens, const int* lens, int Q, int ld,
                            int Lp, int V, int K, int dtype, int chunk_rows, int tree_max_depth, float* out, int* bad, int* info,
                            int* tgt_out, float* zt_out, void* stream);

/* op hooks of the ragged-batch attention (gitmi_set_image_shape(e, 0, 0); tests/test_gpu_ragged_ops.py).  ntok: int32 [B] on the
 * device, the rows of image b (<= N / N_img, which stay the row stride of an image's block); keys past ntok[b] are never used.
 *   attention_ragged: gitmi_op_attention's layout and impl; query rows past ntok[b] are written as zeros.
 *   attn_decode_ragged: gitmi_op_attn_decode's layouts (bf16: the kv_repack operand layouts, N_pad = round_up(N_img, 32));
 *                       the ragged decode kernel is the two-wave MFMA form (16-bit) / the VALU form (f32).
 *   attn_decode_form:   the same operands (ntok may be NULL) and the rest of what the engine's decode step sets
 *                       (tests/test_gpu_attn_decode_forms.py): img_of int32 [B sentences] DEVICE, the image (< n_images) whose K/V
 *                       sentence b attends to, or NULL (sentence b <-> image b); img_k / img_v and ntok are indexed by image;
 *                       out_frag != 0: `out` is the fragment-major operand layout of the decode chain (16-bit only;
 *                       round_up(B * beams, 16) rows, rows past B * beams are not written); pairs_per_wg, waves_per_pair and
 *                       stream_wgs as in AttnDecodeArgs (0: the launcher's defaults).  An argument check + the launcher the
 *                       engine calls.  Refused: null pointers, beams outside 1..8, n_images < 1, out_frag with fp32, ntok with
 *                       stream_wgs > 0. */
int  gitmi_debug_attention_ragged(const void* qkv, void* out, const int* ntok, int B, int N, int H, int dtype, int impl, void* stream);
int  gitmi_debug_attn_decode_ragged(const void* qkv, const void* img_k, const void* img_v, void* txt_k, void* txt_v,
                                    const int* kv_src, void* out, const int* ntok, int B, int H, int N_img, int T_max, int pos,
                                    int beams, int dtype, void* stream);
int  gitmi_debug_attn_decode_form(const void* qkv, const void* img_k, const void* img_v, void* txt_k, void* txt_v,
                                  const int* kv_src, void* out, const int* ntok, const int* img_of, int n_images, int B, int H,
                                  int N_img, int T_max, int pos, int beams, int dtype, int out_frag, int pairs_per_wg,
                                  int waves_per_pair, int stream_wgs, void* stream);
/*   attn_decode_qkv:    the decode attention that computes its own q | k | v (tests/test_gpu_attn_decode_qkv.py): attn_decode_form's
 *                       operands without qkv, plus the QKV GEMM's as gitmi_debug_dgemm_form takes them -- x fragment-major
 *                       [x_rows >= round_up(B, 16)][K = H * 64], w fragment-major [3 K][K], bias / colsum fp32 [3 K], stats
 *                       fp32 [strips][B][2] strip partials of the folded LayerNorm or NULL, eps.  `out` and the appended text
 *                       K/V are, bit for bit, those of gitmi_debug_dgemm_form (C epilogue, N = 3 K) followed by attn_decode_form
 *                       with pairs_per_wg = 8, waves_per_pair = 1.  An argument check + the launcher the engine calls where its
 *                       policy packs 8 one-wave pairs per workgroup; the launch is of that form whatever B is.  Refused by name,
 *                       nothing launched: null pointers, fp32, beams != 1, ntok, waves_per_pair 2, stream_wgs != 0,
 *                       pairs_per_wg != 8, more than 256 padded image keys, H > 12, x_rows too small, stats without colsum. */
int  gitmi_debug_attn_decode_qkv(const void* x, int x_rows, const void* w, const float* bias, const float* colsum, const float* stats,
                                 int strips, float eps, const void* img_k, const void* img_v, void* txt_k, void* txt_v,
                                 const int* kv_src, void* out, const int* ntok, const int* img_of, int n_images, int B, int H,
                                 int N_img, int T_max, int pos, int beams, int dtype, int out_frag, int pairs_per_wg,
                                 int waves_per_pair, int stream_wgs, void* stream);

/* op hooks of the fused decode step (kernels_dgemm.hip vocab_topm_kernel, kernels_search.hip search_step_kernel;
 * tests/test_gpu_search_ops.py).  All list / id / plen pointers are DEVICE memory unless named _host.
 *   vocab_topm_rules:      gitmi_op_vocab_topm with the rule inputs of a real search step in place of suppress_tok: ids int32
 *                          [M][ld_ids] row histories (cur_len tokens each), plen int32 [M / beams] prefix lengths, suppress_kind
 *                          (1: no immediate repeat on rows with cur_len > plen), rep_penalty (0 or 1: off).  ids NULL: no rules.
 *                          ban (or NULL): the rows' decoding constraints, applied before the penalty and the no-repeat rule;
 *                          logits_out then carries the -10000 of the ban (and nothing of the other rules).  The head walks ids
 *                          per column block and keeps no history set: a constrained call has NO cap on cur_len (the penalty's
 *                          cap of 1024 tokens is the hook's own, as before).
 *   search_begin_prefixed: gitmi_search_begin with one prefix length per sentence (start_host int64 [B][ld], plen_host int32 [B]);
 *                          every sentence stands for its own batch-1 reference call, as in gitmi_generate_prefixed.
 *   search_advance_lists:  gitmi_search_advance on caller-supplied candidate lists in the fused head's format (part_val / part_idx
 *                          [R][nparts][slots] sorted, unused entries (-inf, 0x7fffffff); part_lse [R][nparts][2] = (max, sum exp));
 *                          nparts 1..256, slots one of 1 / 2 / 4 / 8 / 16 and at least what the step reads per row.  embed != 0:
 *                          the step also embeds the appended tokens with the engine's weights (input of the next decode step).
 *   read_hidden:           the embedded rows of the most recent step: hf_out fp32 [R][D]; ht_out round_up(R, 16) * D elements of the
 *                          compute type as stored, *ht_frag = 1 when fragment-major (include/gitmi.h), *ht_dtype a GITMI_DTYPE_*. */
int  gitmi_debug_vocab_topm_rules(const void* A, const void* W, const float* bias, const float* colsum, const float* stats,
                                  int strips, float eps, int M, int V, int K, int cols_per_wg, int mtop, const int* ids, int ld_ids,
                                  int cur_len, const int* plen, int beams, int suppress_kind, float rep_penalty, float* part_val,
                                  int* part_idx, float* part_lse, float* logits_out, int max_wgs, void* stream,
                                  const gitmi_debug_ban* ban);
int  gitmi_debug_search_begin_prefixed(gitmi_engine* e, const gitmi_search* sp, int B, const int64_t* start_host, int ld,
                                       const int32_t* plen_host, int vocab, void* stream);
int  gitmi_debug_search_advance_lists(gitmi_engine* e, const float* part_val, const int* part_idx, const float* part_lse,
                                      int nparts, int slots, int embed, void* stream);
int  gitmi_debug_read_hidden(gitmi_engine* e, int R, float* hf_out, void* ht_out, int* ht_frag, int* ht_dtype, void* stream);

/* op hooks of the image front end of the encoder (kernels_norm.hip; tests/test_gpu_frontend_ops.py): an argument check + the
 * launcher gitmi_encode_frames calls, so the launcher's kernel selection is part of what runs.  All pointers DEVICE memory;
 * 16-bit dtypes: the build's operand type (gitmi_operand_dtype); x_f16 / src_f16: fp16 residual-stream rows.
 *   im2col:        img fp32 [B][3][H][W] -> out [B * (H/p) * (W/p)][Kpad] (K = 3 p p, zeros past K).
 *   pos_resize:    pos fp32 [g*g + 1][D] -> out fp32 [gh*gw + 1][D] (bicubic, align_corners = False; row 0 copied).
 *   vit_assemble:  class row / patch_out [B * (N-1)][D] + pos [N][D], ln_pre -> X [B * N][D] (fp32, or fp16 with x_f16);
 *                  part (x_f16 only, or NULL): fp32 [B * N][4][2] folded-LayerNorm partials of the rows as stored.
 *   ragged_front:  one stage of a ragged batch (include/gitmi.h: int32 descriptors [B][4] = {h, w, offset, 0} padded to 256
 *                  bytes, then the planes).  stage 0: src -> slots fp32 [B][3 * max_pixels], meta int32 [B][4] = {h, w, ntok, bad},
 *                  ntok int32 [B].  stage 1: slots, meta -> patches [B][Nmax - 1][Kpad] (patches_dtype).  stage 2: patch_out
 *                  [B * (Nmax-1)][D], cls, pos [g*g + 1][D], meta -> X [B * Nmax][D], part as in vit_assemble.  Arguments of the
 *                  other stages are ignored.
 *   zero_pad_rows: rows t >= ntok[b] of x [B][Nmax][ld] (fp32 or 16-bit elements) set to zero.
 *   layernorm_map: LayerNorm of rows x [rows][D] (fp32, or fp16 with src_f16) + add_after [D] (or NULL) -> y_t (out_dtype, or
 *                  NULL) and y_s (the source's type, or NULL), input row r written to output row
 *                  (r / map_n_in) * map_n_out + map_off + r % map_n_in (map_n_in = 0: row r). */
int  gitmi_debug_im2col(const float* img, void* out, int out_dtype, int B, int H, int W, int p, int K, int Kpad, void* stream);
int  gitmi_debug_pos_resize(const float* pos, float* out, int g, int gh, int gw, int D, void* stream);
int  gitmi_debug_vit_assemble(const float* patch_out, const float* cls, const float* pos, const float* gamma, const float* beta,
                              float eps, void* X, int x_f16, int B, int N, int D, float* part, void* stream);
int  gitmi_debug_ragged_front(int stage, const float* src, float* slots, int* meta, int* ntok, void* patches, int patches_dtype,
                              const float* patch_out, const float* cls, const float* pos, int g, const float* gamma,
                              const float* beta, float eps, void* X, int x_f16, float* part, int B, int p, long long max_pixels,
                              int Nmax, int K, int Kpad, int D, void* stream);
int  gitmi_debug_zero_pad_rows(void* x, int is_f32, int ld, const int* ntok, int B, int Nmax, void* stream);
int  gitmi_debug_layernorm_map(const void* x, int src_f16, const float* gamma, const float* beta, float eps, const float* add_after,
                               void* y_t, int out_dtype, void* y_s, int rows, int D, int map_n_in, int map_n_out, int map_off,
                               void* stream);

/* op hook of the context kernel of GITMI_SEARCH_CONTEXT (kernels_norm.hip; tests/test_gpu_context_ops.py): the host table the
 * engine's context call builds + the launcher it calls.  tokens int64 [Q][ld] DEVICE; len_host / image_of_host int32 [Q] HOST
 * as in gitmi_generate_prefixed (image_of_host NULL: Q == B); words fp32 [vocab][D], positions fp32 [max_pos][D], gamma / beta
 * fp32 [D] DEVICE.  feats [B][stride][D] (dtype: fp32 or the build's operand type): rows [n_img, n_img + C_b) of block b =
 * LayerNorm(words[tok] + positions[p], eps), p from 0 in every segment, the segments of an image in increasing q; rows
 * [n_img + C_b, stride) zero; rows [0, n_img) not touched; feats_f32 (or NULL): an fp32 copy of the rows written; ntok int32
 * [B] DEVICE = n_img + C_b.  Refused by name, nothing launched: null or misaligned pointers, D not a multiple of 8 up to 1024,
 * a length outside [1, min(ld, max_pos)], an image outside [0, B), n_img + C_b > stride.  Synchronises the stream. */
int  gitmi_debug_context_embed(const int64_t* tokens, int ld, const int32_t* len_host, const int32_t* image_of_host, int Q,
                               const float* words, int vocab, const float* positions, int max_pos, const float* gamma,
                               const float* beta, float eps, void* feats, int dtype, float* feats_f32, int* ntok, int B, int n_img,
                               int stride, int D, void* stream);

/* op hooks of the whole-row selection kernels (kernels_search.hip; tests/test_gpu_select_ops.py): an argument check + the
 * launcher the engine calls, so the launcher's refusals and its choice of instantiation are part of what runs.  All pointers
 * DEVICE memory.  logits fp32 [rows][ldl], columns [V, ldl) never read; ids int32 [rows][ld_ids] row histories of cur_len
 * tokens; plen int32 [rows / beams] prefix lengths.
 *   row_topm:    the parity mode's / caller-supplied-logits selection: per row the M best (logit, token) pairs after the rules
 *                (suppress_kind 1: the last token to -10000 on rows with cur_len > plen; rep_penalty over the history, 0 or 1:
 *                off) -> part_val / part_idx [R][row_topm_slots(M)] (1, 2, 4, 8 or 16 slots; value descending, token ascending;
 *                entries past M hold the next best, entries past V (-inf, 0x7fffffff)), part_lse [R][2] = (max, sum exp(x - max))
 *                of the ruled row.  ids NULL: no rules.  Refused by name: null logits / outputs, ldl < V, ids without plen, R not
 *                a multiple of beams, cur_len outside [1, ld_ids]; by the launcher (invalid argument): M outside 1..16, a
 *                penalty or a ban over more than 1024 tokens.  Nothing is launched then.  ban (or NULL): the rows' decoding
 *                constraints, -10000 before the penalty and the no-repeat rule.
 *   trie_select: one step of GITMI_SEARCH_TRIE on a caller's CSR trie -- child_off int32 [n_nodes + 1], child_tok / child_node
 *                int32 [child_off[n_nodes]], cursor int32 [B] (node of every sentence, -1 unconstrained; read and updated) ->
 *                part_val / part_idx [B] (log-prob incl. the trie bonus, token), part_lse [B][2] = (0, 1).  Rows with cur_len <
 *                plen[b] are not written.  Child tokens outside [0, V) are skipped.  Refused by name: null pointers, V < 2,
 *                ldl < V, a child_off that does not start at 0 or decreases, an edge or a cursor that names no node (checked on
 *                host copies as gitmi_set_trie checks them; synchronises the stream first).
 *   sample_rows: gitmi_op_sample_rows with the rest of what the engine's sampling step sets: ldl, the histories of the
 *                repetition penalty (applied to the raw logits, before the temperature) and the list stride -- draw_logprob /
 *                draw_token [R][stride], entries ndraw..stride (-inf, 0x7fffffff); filtered_out [R][V] or NULL.  Refused by the
 *                launcher (invalid argument): V outside 2..32768, ndraw outside 1..16, stride < ndraw, temperature <= 0, a
 *                penalty or a ban over more than 1024 tokens.  ban (or NULL): the rows' decoding constraints on the raw
 *                logits, before the penalty, with plen int32 [R / beams] and beams (both read under a ban only; R a multiple of
 *                beams).  Synchronises the stream. */
/*   row_topm with ban->row_words_out != NULL: ban_rows_kernel ALONE, no selection (the measurement builds keep their symbol
 *                list, so the hook of the new kernel is a form of this one) -- the per-row ban sets of one step under banned token
 *                sequences (include/gitmi.h, the extension of GITMI_SEARCH_CONSTRAIN): row_words_out uint32 [R][W] DEVICE = the
 *                static set of the row's sentence (ban->words / n_sets / W / set_of; zeros without one) OR the last tokens of the
 *                sequences that the row's history ids[row][0 .. cur_len) ends with.  ban->pool_host int32 [n_pool]: the HOST pool
 *                { L, S, T, 0, list_of[R / beams], list_off[L + 1], seq_off[S + 1], tok[T] }, validated by the check the arming
 *                call makes (L at most the sentence count) and refused by the same messages; W above the kernel's LDS budget
 *                (8192 words) and ban->row_words together with row_words_out are refused.  Reads ids, ld_ids, cur_len, R, beams,
 *                V, stream; logits, plen, the rules and the list outputs are ignored.  Synchronises.  (To become a hook of its
 *                own, gitmi_debug_ban_rows, when the symbol list of the measurement builds is next revised.) */
int  gitmi_debug_row_topm(const float* logits, int ldl, int V, int R, const int* ids, int ld_ids, int cur_len, const int* plen,
                          int beams, int suppress_kind, float rep_penalty, int M, float* part_val, int* part_idx, float* part_lse,
                          void* stream, const gitmi_debug_ban* ban);
int  gitmi_debug_trie_select(const float* logits, int ldl, int V, int B, const int* ids, int ld_ids, int cur_len, const int* plen,
                             int eos, const int* child_off, const int* child_tok, const int* child_node, int n_nodes, int* cursor,
                             float* part_val, int* part_idx, float* part_lse, void* stream);
int  gitmi_debug_sample_rows(const float* logits, int R, int V, float temperature, int top_k, float top_p, int ndraw, uint64_t seed,
                             int step, float* draw_logprob, int* draw_token, float* filtered_out, int ldl, const int* ids, int ld_ids,
                             int cur_len, float rep_penalty, int stride, void* stream, const int* plen, int beams,
                             const gitmi_debug_ban* ban);

#endif /* GITMI_EXPERIMENT_TYPES_ONLY */
#ifdef __cplusplus
}
#endif
#endif /* GITMI_EXPERIMENT_H_ */
