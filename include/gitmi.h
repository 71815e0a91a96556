/*
 * gitmi.h -- C ABI of the MI355X-native GIT captioning / VQA inference engine.
 *
 * The reference (microsoft/GenerativeImage2Text) has no FFI / operator layer: its
 * extension seams are Python duck-typed.  This header is the drop-in
 * boundary a maintainer binds instead of those seams; every entry point names the
 * reference interface it replaces (paths relative to
 * /root/reference/generativeimage2text/).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain C, no torch types.  All tensor pointers are DEVICE pointers unless the
 *     parameter name ends in _host.  Caller owns inputs/outputs; the engine owns
 *     repacked weights, KV caches and workspaces sized at gitmi_create().
 *   - every call returns 0 on success, non-zero on error; gitmi_last_error() returns
 *     a thread-local message.  Nothing throws across the ABI.
 *   - one engine per device per process; calls on one engine are serialised by the
 *     caller and are asynchronous w.r.t. the host on the hipStream_t passed as
 *     `stream` (a void* so that this header needs no HIP include).
 *   - no CPU fallback exists: without a gfx950 device gitmi_create() fails.
 */
#ifndef GITMI_H_
#define GITMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GITMI_ABI_VERSION 10

/* compute precision of GEMM/attention operands (accumulation, LayerNorm statistics,
 * softmax, residual stream and logits are fp32 in both modes) */
#define GITMI_PREC_BF16 0   /* 16-bit MFMA operands (the type of the library: below) */
#define GITMI_PREC_F32  1   /* f32-input MFMA, exact fp32 -- parity-debug path        */

/* tensor dtypes accepted by gitmi_load_tensor */
#define GITMI_DTYPE_F32  0
#define GITMI_DTYPE_BF16 1
#define GITMI_DTYPE_F16  2
/* gitmi_op_gemm's out_dtype only: fp16 residual-stream rows (C fp16 [M, ldc]; the residual, if any, is fp16 rows too) */
#define GITMI_DTYPE_F16_STREAM 3

/* search strategies (layers/decoder.py) */
#define GITMI_SEARCH_AUTOREGRESSIVE 0  /* AutoRegressiveBeamSearch   decoder.py:208-440  */
#define GITMI_SEARCH_GENERATOR      1  /* GeneratorWithBeamSearch    decoder.py:1056-1290 */
#define GITMI_SEARCH_TRIE           2  /* TrieAutoRegressiveBeamSearch (beam 1, token trie: gitmi_set_trie)  trie_decoder.py:27-218 */
#define GITMI_SEARCH_SCORE          3  /* not a search: score given sentences (CaptioningModel.forward_one_ce, decoder.py:916-972);
                                        * gitmi_generate_prefixed only, see there */
#define GITMI_SEARCH_ATTEND         4  /* not a search: the attention the text rows of given sentences pay to the image tokens and
                                        * to their own text (BertSelfAttention.output_attentions, head mean); gitmi_generate_prefixed
                                        * only, see there */
#define GITMI_SEARCH_CONTEXT        5  /* not a search: context tokens (the reference's batch['context'], decoder.py:861-871) put into
                                        * the decoder memory behind the image tokens; gitmi_generate_prefixed only, see there */
#define GITMI_SEARCH_TREE_SCORE 6      /* not a search: score every node of given token trees (a closed candidate set as a trie) in one
                                        * text pass; gitmi_generate_prefixed only, see there */
#define GITMI_SEARCH_KEEP   7          /* not a search: copy the encoded memory of resident images into slots of a caller-owned
                                        * store; gitmi_generate_prefixed only, see there */
#define GITMI_SEARCH_RECALL 8          /* not a search: make any selection of kept slots the resident images of a context;
                                        * gitmi_generate_prefixed only, see there */
#define GITMI_SEARCH_FEATURES 9        /* not a search: make caller-supplied visual feature rows the resident images of a context
                                        * (the input side of gitmi_encode_frames' feats_out); gitmi_generate_prefixed only, see there */
#define GITMI_SEARCH_CONSTRAIN 10      /* not a search: arm per-sentence decoding constraints (banned tokens, a minimum length, no
                                        * repeated n-grams) for the next search call of a context; gitmi_generate_prefixed only, see there */
#define GITMI_SEARCH_TRACE 11          /* not a search: arm the per-token trace (log-prob of every emitted token and the n likeliest
                                        * alternatives) of the next search call of a context; gitmi_generate_prefixed only, see there */

typedef struct gitmi_engine gitmi_engine;

/* Model + capacity description.  Replaces the hyper-parameters hard-coded in
 * model.py:9-61 (decoder) / CLIP build_model (encoder) / aux_data/models/<m>/parameter.yaml. */
typedef struct gitmi_config {
    int32_t image_size;     /* test_crop_size, 224                                    */
    int32_t patch;          /* 16 (ViT-B/16) | 14 (ViT-L/14)                          */
    int32_t vit_width;      /* 768 | 1024  (== visual_feature_size)                   */
    int32_t vit_layers;     /* 12 | 24                                                */
    int32_t vit_heads;      /* 12 | 16   (head_dim must be 64)                        */
    int32_t dec_hidden;     /* 768                                                    */
    int32_t dec_layers;     /* 6                                                      */
    int32_t dec_heads;      /* 12  (head_dim must be 64)                              */
    int32_t dec_ffn;        /* 3072                                                   */
    int32_t vocab;          /* 30522                                                  */
    int32_t max_pos;        /* 1024 (max_caption_length, model.py:21)                 */
    int32_t num_frames;     /* num_image_with_embedding: temporal embeddings, 0=none  */
    int32_t sos;            /* tokenizer.cls_token_id = 101                           */
    int32_t eos;            /* tokenizer.sep_token_id = 102                           */
    int32_t precision;      /* GITMI_PREC_*                                           */
    int32_t max_batch;      /* capacity: images per call                              */
    int32_t max_beams;      /* capacity: beam_size                                    */
    int32_t max_frames;     /* capacity: frames per sample (>=1)                      */
    int32_t max_text_len;   /* capacity: prefix + generated tokens (KV-cache length)  */
    int32_t max_image_pixels; /* capacity: H*W of an input frame; 0 = image_size^2. Models with
                               * test_respect_ratio_max (MinMaxResizeForTest, inference.py:29-64):
                               * test_crop_size * test_respect_ratio_max               */
    int32_t max_image_tokens; /* capacity: (H/patch)*(W/patch)+1 per frame; 0 = native grid */
} gitmi_config;

/* Replaces the constructor arguments of the two search classes
 * (decoder.py:209-222, 1057-1081). */
typedef struct gitmi_search {
    int32_t kind;                 /* GITMI_SEARCH_*                                   */
    int32_t beam_size;
    int32_t per_node_beam_size;
    int32_t max_steps;            /* TOTAL length incl. [CLS]/prefix (decoder.py:313, 1111) */
    double  length_penalty;       /* GENERATOR only (double: the reference does this math in Python floats) */
    /* sampling branch of GeneratorWithBeamSearch.search (decoder.py:1146-1166): scores / temperature ->
     * top_k_top_p_filtering(min_tokens_to_keep = 2, decoder.py:1343-1375) -> per_node_beam_size draws WITHOUT replacement
     * from the filtered softmax -> log-probabilities of the draws; the beam bookkeeping that follows is the same.
     * torch.multinomial's random stream cannot be reproduced: draws come from a counter-based generator keyed by
     * (seed, step, row, token) through the Gumbel-top-k construction (exactly that sampling distribution). */
    int32_t do_sample;            /* 0 = greedy beam search (default); 1 = sample (GENERATOR only)     */
    int32_t top_k;                /* <= 0: off                                                         */
    double  top_p;                /* >= 1 or <= 0: off                                                 */
    double  temperature;          /* > 0; 1 = unchanged (0 is read as 1)                               */
    uint64_t seed;
    /* GENERATOR only: repetition penalty (decoder.py:1064, 1135-1144) -- before the log-softmax (and before the sampling
     * filter) the raw score of every token already in a row's history (start tokens included) is multiplied by it when
     * negative and divided by it otherwise.  >= 1; 0 and 1 both mean off. */
    double  repetition_penalty;
    /* GENERATOR only: `num_keep_best` of GeneratorWithBeamSearch.search (decoder.py:1087, 1113-1115, 1262-1290) -- every
     * sentence keeps its n best finished hypotheses (BeamHypotheses(n_hyp = n)) and returns all of them, best first:
     * tokens_out becomes [B, n, max_steps], logprob_out [B, n]; sequences the list cannot fill are all EOS with
     * log-prob -1e5, as in the reference.  1 .. 8; 0 is read as 1.  (The reference's `num_return_sequences` -- r independent
     * sentences per image -- is the host mirror's business: r sentences with the same image index, gitmi_generate_prefixed.) */
    int32_t num_keep_best;
    int32_t reserved_;
} gitmi_search;

/* per-phase device timings (ms) of the last profiled gitmi_generate(), see gitmi_profile_enable */
typedef struct gitmi_profile {
    float    vit_ms, prefill_ms, decode_ms, total_ms;
    float    gemm_ms;             /* sum over every GEMM launch of the call            */
    int32_t  gemm_launches;
    double   gemm_flops;          /* algorithmic 2*M*N*K summed over those launches    */
    float    vit_gemm_ms;         /* GEMM launches of the image encoder only           */
    int32_t  vit_gemm_launches;
    double   vit_gemm_flops;
    float    decode_step_ms;      /* average over executed decode steps                */
    int32_t  decode_steps;
    double   decode_step_bytes;   /* algorithmic bytes per step: weights + KV read     */
} gitmi_profile;

/* ---- lifecycle ------------------------------------------------------------------- */
int  gitmi_abi_version(void);
/* The 16-bit operand type of the library's fast mode (GITMI_PREC_BF16 of gitmi_config.precision means "the 16-bit operand
 * mode of this build"): GITMI_DTYPE_BF16 for libgitmi.so, GITMI_DTYPE_F16 for libgitmi_f16.so -- the benchmarked build since round 6 --,
 * the same sources built with -DGITMI_OPS_F16 (IEEE fp16 operands on v_mfma_f32_16x16x32_f16: same rate, 3 more
 * mantissa bits; 16-bit operands handed to the gitmi_op_* entry points are then fp16 too). */
int  gitmi_operand_dtype(void);
const char* gitmi_last_error(void);
/* replaces get_git_model(tokenizer, param) + model.cuda()  (model.py:9-61, inference.py:83-87) */
int  gitmi_create(const gitmi_config* cfg, int device, gitmi_engine** out);
void gitmi_destroy(gitmi_engine* e);

/* ---- checkpoint ingest:  replaces load_state_dict(model, ckpt) (torch_common.py:93-145).
 * `key` is the reference state-dict key, e.g.
 * "image_encoder.transformer.resblocks.3.attn.in_proj_weight".  `data_host` is a HOST
 * pointer to a dense row-major tensor. Unknown keys return an error; "image_encoder.proj"
 * is accepted and ignored (unused when output_grid=True, CLIP/model.py:263-268). */
int  gitmi_load_tensor(gitmi_engine* e, const char* key, const void* data_host,
                       const int64_t* shape, int ndim, int dtype);
/* repack for the device: fused QKV, K padding, compute-dtype copies; ties
 * textual.output.weight to embedding.words.weight if it was not loaded (decoder.py:503-505) */
int  gitmi_finalize_weights(gitmi_engine* e);

/* second execution context on the same device that borrows the packed weights of `src` (own
 * workspaces / KV caches / search state / graph): several batches in flight on different streams.
 * `src` must outlive the clone; destroy clones with gitmi_destroy. */
int  gitmi_clone(gitmi_engine* src, gitmi_engine** out);

/* serving schedule for several contexts of one device: the image encoder (+ decoder prefill) of `e`'s gitmi_generate
 * calls starts only after the encoder of `after`'s most recently submitted call has finished (decode steps are not
 * ordered).  Chain context i (in submission order) after context i - c: at most c MFMA-bound encoders run at a time while
 * the latency-bound decode chains of the other contexts fill in beside them (measured best on MI355X: 4 contexts, c = 2;
 * bench.py --encoder-chains).  after = NULL: no dependency (the context goes back to one hipGraph per call once no other
 * context waits for it either).  Destroying either context of a link removes the link. */
int  gitmi_set_encode_after(gitmi_engine* e, gitmi_engine* after);

/* serving policy: tell a context that other contexts keep the device busy beside it.  Kernel shapes are then chosen
 * for what a launch costs the device as a whole, not for its own duration: the image-encoder GEMMs always take the
 * 256x256 tile (a partial round's idle CUs are filled by the other contexts; measured +2.2 % captions/s in the mixed
 * schedule, -3 % for a context alone), the N = 768 GEMMs of the decode chain take 32 rows per workgroup (64 for beam
 * batches: beam-4 +4.5 %), the decode attention packs 8 instead of 4 (sentence, head) pairs per workgroup (+0.8 %), the wide
 * chain GEMMs take two 16-column strips per workgroup one after the other (+1.3 %) and, for beam batches, walk their row
 * blocks in one workgroup per weight strip (beam-4 +1.7 %), the vocabulary head runs on ~60 workgroups that each walk four
 * column blocks (+1 %).
 * Results are bit-identical either way.  Clones inherit the setting of their source at clone time. */
int  gitmi_set_shared_device(gitmi_engine* e, int on);
/* (new, ABI 9) LayerNorm folding in the image encoder and the prefill -- replaces the LayerNorm modules of
 * layers/CLIP/model.py:161-168,189-202 (ln_1 / ln_2) and layers/bert/modeling_bert.py:171-178,243-250 + layers/decoder.py:35
 * (post-norm LayerNorms over the image rows) for passes of more than 512 rows in the fp16-operand library: the producer
 * GEMM leaves (sum, sumsq) per row, the consumer GEMM reads the raw stream rows and applies the normalisation in its
 * epilogue.  on = 1 is the default where it is available; on = 0 runs one LayerNorm launch per module instead (what
 * libgitmi.so, the f32 mode and small batches always do).  Fails if on = 1 is asked of an engine that cannot fold. */
int  gitmi_set_ln_fold(gitmi_engine* e, int on);

/* ---- input resolution of the following encode/generate calls (default: image_size x image_size).
 * Replaces the run-time branch of VisualTransformer.forward for inputs that are not the native
 * resolution (CLIP/model.py:243-251): the token grid becomes (H / patch) x (W / patch) -- the stride-patch
 * convolution ignores the H % patch / W % patch remainder -- and the positional table is resized to it with
 * torch's bicubic (align_corners=False) kernel, class row kept.  H*W and the token count must fit the
 * max_image_pixels / max_image_tokens capacities given at gitmi_create(). */
int  gitmi_set_image_shape(gitmi_engine* e, int H, int W, void* stream);
/* ---- ragged input: gitmi_set_image_shape(e, 0, 0, stream) makes every image of the following calls carry its own size
 * (the aspect-preserving MinMaxResizeForTest models); any valid H, W returns to uniform input.  In ragged mode the calls
 * that take frames (gitmi_encode_frames, gitmi_generate, gitmi_generate_prefixed incl. GITMI_SEARCH_SCORE) need F == 1, and
 * frames[0] points to ONE device buffer:
 *     int32 desc[B][4] = { h, w, offset, 0 }, the block padded to 256 bytes;
 *     then the fp32 [3, h, w] plane of image b at (float*)buffer + offset (offset in floats, a multiple of 4: 16-byte aligned).
 * Image b owns token rows [b * Nmax, b * Nmax + n_b) of the encoder / feature / prefill blocks, n_b = (h/p)(w/p) + 1 and
 * Nmax = the max_image_tokens capacity; feats_out is [B, Nmax, vit_width] with zeros in the rows past n_b.  The shapes are
 * read and checked ON THE DEVICE (one captured graph serves every mix of shapes): an entry with h or w below one patch,
 * h * w above max_image_pixels, a grid above max_image_tokens, an offset inside the descriptor block or not a multiple of 4
 * is not read; its sentences come back with a NaN log-prob and are counted in info_out[3] (score: counted in info_out[3]),
 * the other images are unaffected.  The call has no buffer size to check against: the CALLER guarantees that frames[0] is
 * 16-byte aligned (the descriptor is read as int4) and that offset + 3*h*w floats of every entry lie inside its buffer --
 * an entry that passes the checks above is copied whole.
 * Each image gets what a call with that image alone gets (bit for bit in the f32 mode). */

/* ---- image encoder: replaces model.image_encoder(x) + the multi-frame branch of
 * CaptioningModel.forward_one (CLIP/model.py:240-274, decoder.py:845-857).
 * frames: F device pointers to fp32 [B,3,H,W] (H, W as set by gitmi_set_image_shape).  The visual features
 * [B, F*N, vit_width] stay resident in the engine; feats_out (optional, fp32) receives a copy. */
int  gitmi_encode_frames(gitmi_engine* e, const float* const* frames, int F, int B,
                         float* feats_out, void* stream);

/* batch['image'] given as a LIST of frames (on = 1, default) or as a bare tensor (on = 0): the reference adds
 * img_temperal_embedding[i] to frame i only in the list case (decoder.py:845-857). */
int  gitmi_set_temporal_embedding(gitmi_engine* e, int on);

/* ---- decoder prefill over image tokens (visual_projection + image rows of all layers);
 * builds the per-image K/V cache.  Mathematically the image part of
 * TransformerDecoderTextualHead.forward (decoder.py:521-600), computed once per image. */
int  gitmi_prefill(gitmi_engine* e, void* stream);

/* ---- teacher-forced step == the reference's `step` callable
 * (CaptioningModel.decoding_step, decoder.py:1013-1054): tokens int64 [R,t], R = B*beams with
 * rows of one image contiguous; writes fp32 next-token logits [R, vocab]. */
int  gitmi_step_logits(gitmi_engine* e, const int64_t* tokens, int R, int t,
                       float* logits_out, void* stream);

/* ---- whole hot path: replaces model({'image':..., 'prefix':...})
 * (CaptioningModel.forward/infer, decoder.py:838-877, 977-1011) incl. the search loop.
 *   frames       : F device pointers as for gitmi_encode_frames, or NULL: a follow-up call over the resident images (below);
 *   prefix       : int64 [P] starting with [CLS], or NULL for captioning (P ignored);
 *                  the reference requires B==1 with a prefix (decoder.py:988) -- here a
 *                  single prefix is shared by all B images.
 *   tokens_out, logprob_out, info_out (and sent_out of gitmi_generate_prefixed): device buffers OR page-locked host buffers
 *                  (hipHostMalloc / a pinned torch tensor): with host buffers the results are on the host when the stream reaches
 *                  the end of the call, no read-back has to be enqueued afterwards.
 *   tokens_out   : int64 [B, max_steps]; sequences INCLUDE the start tokens, EOS-padded.
 *   logprob_out  : fp32 [B]  (AUTOREGRESSIVE: sum/num_valid, decoder.py:429-438;
 *                              GENERATOR: length-normalised score, decoder.py:1310-1320)
 *   info_out     : int32 [4] = { seq_len, early_all_eos, steps_run, nonfinite }
 *                  seq_len = length of the tensor the reference returns (AUTOREGRESSIVE stops
 *                  when every beam ended, decoder.py:319; GENERATOR always max_steps);
 *                  early_all_eos=1 is the first-step early return of decoder.py:279-291;
 *                  steps_run = text positions appended (max_steps - 1 unless a long-budget call stopped early);
 *                  nonfinite = returned sequences whose log-prob is inf / NaN: an operand left the range of the 16-bit
 *                  operand format (fp16: 65504) somewhere upstream -- the ids of such a call are meaningless and the
 *                  caller must treat it as an error (the Python binding raises).  Weights are range-checked when they
 *                  are loaded (gitmi_load_tensor / gitmi_finalize_weights fail by name). */
/* ---- follow-up calls on resident images: frames == NULL.
 * gitmi_generate(e, frames = NULL, ...) and gitmi_generate_prefixed(e, frames = NULL, ...) -- every search kind and
 * GITMI_SEARCH_SCORE -- run over the images the engine already holds: no image encoder and, when the prefill is current, no
 * prefill; only the decode chain (or the score pass) runs.  A second question about the same images, a beam-4 pass after a
 * greedy one, the log-probs of the captions just generated, reranking of an n-best list.
 *   F is ignored.  B must equal the number of resident images (the B of the call that encoded them); anything else fails
 *   with a message naming both numbers.  Everything else keeps its meaning and its checks: prefixes, image_of_host (any
 *   subset, order or repetition of [0, B)), Q, the whole gitmi_search, the trie, the output buffers.
 * Residency: the images of a call are resident from the end of any call that encoded them -- gitmi_generate,
 * gitmi_generate_prefixed (score included), gitmi_encode_frames -- until something changes what an encode would produce: a
 * gitmi_set_image_shape that changes the shape or the mode, a gitmi_set_temporal_embedding or gitmi_set_ln_fold flip.
 * Decode steps and score passes write text caches only.  After gitmi_encode_frames alone the follow-up runs the prefill
 * first (as gitmi_step_logits does).  Without resident images the call fails before any launch.  An argument error found
 * before the first launch of any call leaves residency as it was; a call that fails after it started encoding clears it.
 * Every context has its own resident set; a clone starts with none.
 * Ragged mode: the shapes, token counts and rejected entries of the resident batch are used (no descriptor is read);
 * sentences over a rejected entry still come back NaN and are counted in info_out[3].
 * hipGraph: a follow-up captures and replays the decode part alone, in a slot of its own beside the full call's graph:
 * full, follow-up, full, follow-up with unchanged arguments replays both and re-captures neither.  Score follow-ups run
 * eagerly, as score does.  Serving schedule (gitmi_set_encode_after): a follow-up has no encoder -- it neither waits for
 * `after`'s encoder nor signals its own watchers, who keep waiting for the most recent real encoder.
 * Profiling: vit_ms, prefill_ms and vit_gemm_* of a follow-up are 0, decode_* as usual. */
int  gitmi_generate(gitmi_engine* e, const float* const* frames, int F, int B,
                    const int64_t* prefix, int P, const gitmi_search* search,
                    int64_t* tokens_out, float* logprob_out, int32_t* info_out, void* stream);

/* ---- batched VQA: Q sentences with their OWN prefixes over B images.  The reference answers one question per
 * model call (decoder.py:984-989 asserts a single prefix; inference.py:172-199 loops); here the questions of one
 * image share its encoded K/V and questions of different lengths share every decode step (all sentences sit at the
 * same text position; a sentence still inside its prefix just appends the given token).  Each sentence gets exactly
 * what its own batch-1 reference call returns.
 *   prefixes        : int64 [Q, ld_prefix] DEVICE, row q = its tokens incl. [CLS] (entries past its length ignored)
 *   prefix_len_host : int32 [Q] HOST, 1 <= len <= ld_prefix
 *   image_of_host   : int32 [Q] HOST, image index of every sentence, or NULL (Q == B, sentence q <-> image q)
 *   tokens_out      : int64 [Q, max_steps], logprob_out fp32 [Q] as in gitmi_generate
 *   sent_out        : int32 [Q, 2] = (length of the sequence returned for this sentence, its early-return flag) or NULL */
/* ---- caption scoring: search->kind == GITMI_SEARCH_SCORE turns gitmi_generate_prefixed into the mirror of the reference's
 * `forward` choosing forward_one_ce over infer (decoder.py:916-972): the textual head runs once over whole sentences and
 * the vocabulary head returns, for every position j >= 1 of sentence q, with z the fp32 logits at position j - 1 over
 * [image | tokens[q, 0..j)] (joint mask of decoder.py:111-149, 602-610):
 *     lp[q, j] = log_softmax(z)[tokens[q, j]],   mean_lp[q, j] = mean_c log_softmax(z)[c] = sum(z) / V - LSE(z)
 * (position 0 and positions >= len_q: 0).  The reference's CE and label-smoothed losses reduce exactly from these two.
 *   prefixes        : int64 [Q, ld] DEVICE, the sentences to score (each starts with [CLS]); ld <= max_text_len
 *   prefix_len_host : their lengths (>= 1); image_of_host as above; Q <= max_batch x max_beams (candidates per image)
 *   logprob_out     : fp32 [Q, ld, 2] = (lp, mean_lp), device or page-locked host buffer
 *   tokens_out, sent_out: ignored (may be NULL); info_out = { ld, 0, 0, sentences with a non-finite value }
 *   the other gitmi_search fields are ignored.  gitmi_generate and gitmi_search_begin refuse this kind.
 * Like a generate call it replaces the engine's encoded images and prefill (with frames == NULL it scores over the resident
 * images instead: follow-up calls, above gitmi_generate); its workspaces are allocated by the first score call (engines that
 * never score keep their footprint). */
/* ---- token trees: search->kind == GITMI_SEARCH_TREE_SCORE is GITMI_SEARCH_SCORE with trees in place of sentences: a closed
 * candidate set (answers of a VQA list, class names, captions to rerank) given as a trie is scored exactly in one call, every
 * shared prefix passing through the decoder and the vocabulary head once.  "Sentence" q is a tree in DFS pre-order:
 *   prefixes        : int64 [Q, ld] DEVICE; element i of row q is node i of tree q: low 32 bits = token id (clamped into the
 *                     vocabulary, as the context kind clamps), high 32 bits = depth.  Node 0 is the root ([CLS]) at depth 0; the
 *                     parent of node i is the last k < i with depth[k] == depth[i] - 1.
 *   prefix_len_host : the node counts, 1 <= n_q <= ld.  ld is NOT bounded by max_text_len; the depths are:
 *                     depth < min(max_text_len, max_pos) (a node's depth is its position embedding); an engine whose bound
 *                     exceeds 8192 is refused by message (the root path of the structure walk is held on chip).
 *   image_of_host, Q <= max_batch x max_beams (trees per call), frames or NULL (a follow-up over the resident images, which
 *                     may carry context: every node then sees [image | context | its ancestors]), ragged image mode: as for score.
 *   rows            : Q x round_up(max_q n_q, 16) <= 4 194 240 (65535 x 64).  Every row count and launch grid of the pass is a
 *                     32-bit int and byte offsets are 64-bit; the binding widths are the grids' 65535-block y / z dimensions
 *                     (attention: padded nodes of a tree / 64, head: rows / 128), and the cap is the smaller, reached by one tree
 *                     that has all the rows.  A call above it is refused before any launch, the message names the rows asked
 *                     for; below it, device memory bounds the call (out of memory is an error, nothing is truncated).
 *   validity        : local -- depth[0] == 0; 1 <= depth[i] <= depth[i-1] + 1 for i >= 1; depth below its bound.  The table is
 *                     device memory, so the first launch of the call checks it on the device: a tree that fails is rejected --
 *                     its outputs stay 0, it is counted in info_out[3], and it is given a trivial structure (every node a root)
 *                     before any other kernel reads it, so no address is ever formed from its depths.  The other trees of the
 *                     call are not affected.
 *   logprob_out     : fp32 [Q, ld, 2]; with z the fp32 logits at the row of parent(i), computed over
 *                     [image (| context) | the ancestors of i, root first]:
 *                         lp[q, i] = log_softmax(z)[token(i)],   mean_lp[q, i] = sum(z) / V - LSE(z)
 *                     node 0 and nodes >= n_q: 0.  A tree that is one chain (depth[i] = i) is a sentence and this is score's output.
 *   tokens_out, sent_out: ignored (may be NULL); info_out = { ld, 0, 0, trees rejected or with a non-finite value }
 *   the other gitmi_search fields are ignored.  gitmi_generate, gitmi_search_begin and the step seam refuse this kind.
 * Residency, the eager launch path and the serving schedule are those of a score call.  The node tables and the [Q, ld] output
 * join the score workspaces at the first tree call and grow on demand: engines that never score trees keep their footprint,
 * and every other kind returns exactly what it returns without this one. */
/* ---- attention maps: search->kind == GITMI_SEARCH_ATTEND runs the same text pass over the same inputs with the same checks
 * as GITMI_SEARCH_SCORE (prefixes [Q, ld] DEVICE, prefix_len_host, image_of_host, Q <= max_batch x max_beams, frames or NULL
 * for a follow-up over the resident images) and returns where every token looked instead of how likely it was: the
 * probabilities BertSelfAttention.output_attentions exposes (layers/bert/modeling_bert.py:99-158), text rows only, averaged
 * over the heads.  With q_{l,h}, k_{l,h} the query / key rows of decoder layer l, head h (head_dim 64, scale 1/8 in fp32):
 *     att[q, j, l, k] = (1/H) sum_h softmax_k'( q_{l,h}(q, j) . k_{l,h}(k') / 8 )[k]
 * k' over the image keys of image image_of[q] and the text keys 0..j of sentence q (the joint mask of decoder.py:111-149).
 *   logprob_out     : fp32 [Q, ld, dec_layers, Kc], device or page-locked host buffer; Kc = Nk + ld, Nk = the image key rows
 *                     of one image in this call: F * N for uniform input (F after the num_frames truncation), the
 *                     max_image_tokens capacity Nmax in ragged mode.
 *                     Column order: columns [0, Nk) are the image tokens in the row order of the prefill -- frame-major, the
 *                     class token first within each frame; column Nk + t is text position t.
 *                     The zeros: rows j >= len_q, text columns t > j and, in ragged mode, image columns >= n_b (the image's
 *                     own token count) are exactly 0.  Every other row sums to 1.
 *   tokens_out, sent_out: ignored (may be NULL); info_out = { ld, Kc, dec_layers, sentences with a non-finite value }
 *                     (ragged mode: sentences over a rejected image are counted there, as score counts them)
 *   the other gitmi_search fields are ignored; the vocabulary head does not run.  gitmi_generate and gitmi_search_begin
 *   refuse this kind.  Residency, the eager launch path (no hipGraph) and the serving schedule are those of a score call;
 *   score calls return exactly what they return without this kind.  The output workspace (Q ld dec_layers Kc floats) is
 *   allocated by the first attend call and grown on demand: engines that never attend keep their footprint. */
/* ---- context tokens: search->kind == GITMI_SEARCH_CONTEXT turns gitmi_generate_prefixed into the reference's 'context' input
 * (CaptioningModel.forward_one, decoder.py:861-871: OCR strings, tags, retrieved captions, dialogue history).  The reference
 * embeds every segment with the textual embedding -- LayerNorm(words[tok] + positions[p], eps 1e-8), positions restarting at 0
 * in every segment --, concatenates the rows to the visual features, runs the whole concatenation through the visual
 * projection into the decoder memory and masks the positions past every segment's length as keys (decoder.py:97-149, 569).
 * Embedded keys carry no position of their own, so the engine compacts an image's valid context rows directly behind its image
 * rows: image b's block of the memory is [F N image rows | C_b context rows | zero rows] with the key count
 * ntok[b] = F N + C_b -- the padded layout's mathematics, fp32 summation order aside.
 *   frames          : must be non-NULL: the context comes with the call that encodes its images (a NULL follow-up is refused;
 *                     appending context to resident images is not implemented)
 *   prefixes        : int64 [Q, ld] on the DEVICE, row q = one context segment, its tokens at positions 0 .. len_q - 1; ids past
 *                     the length are never read; ids outside the vocabulary are clamped into it (validate on the host)
 *   prefix_len_host : int32 [Q], 1 <= len_q <= min(ld, max_pos)
 *   image_of_host   : int32 [Q], the image of segment q (NULL: Q == B, segment q <-> image q).  The segments of one image are
 *                     appended to its memory in increasing q, any interleaving between images is allowed; an image without a
 *                     segment has no context
 *   info_out        : { row stride of an image's block, max_b C_b, sum_b C_b, 0 }; tokens_out, logprob_out, sent_out: ignored
 *                     (may be NULL); the other gitmi_search fields are ignored
 * It runs the image encoder, one launch that writes every context row, the zero rows and the key counts, and the prefill; no
 * decode step, no vocabulary head; eagerly (no hipGraph), as score does.  Afterwards the images AND their context are
 * resident and the batch is in key-count mode: prefill attention, decode attention and the text pass read ntok[b] keys of
 * image b.  Every follow-up form (frames == NULL) then runs over [image | context] with nothing changed at the interface:
 * gitmi_generate with any search and a shared prefix, gitmi_generate_prefixed with ragged prefixes, GITMI_SEARCH_SCORE;
 * gitmi_prefill / gitmi_step_logits see the same memory.  Every sentence gets what a batch-1 reference call with its image, its
 * context and its prefix returns (the reference itself fails for B > 1 with beams > 1, decoder.py:1018-1025).  The captured
 * decode graph of a follow-up is keyed on the row stride, the counts live in one device array: batches of equal stride and
 * different counts replay one graph.  GITMI_SEARCH_ATTEND over a context-carrying resident batch is refused (the map with
 * context columns is not implemented).  Any later call with frames replaces the resident set and leaves key-count mode: a
 * plain call after a context call returns exactly what it returns on a fresh engine.  A clone starts with nothing resident.
 * Capacity: F N + C_b, and the stride (F N + max_b C_b, rounded up to a multiple of 16 where that fits), must fit the
 * max_frames x max(N, max_image_tokens) rows per image the workspaces are sized for; beyond that the call fails before any
 * launch, the message names the rows asked for and the capacity, and the resident set stays as it was -- as for every
 * argument error.  Also refused before any launch: ragged image mode (gitmi_set_image_shape(e, 0, 0)), vit_width != dec_hidden
 * (the reference's torch.cat fails there too), a length outside its range.  gitmi_generate and gitmi_search_begin refuse this
 * kind.  The segment table's device copy is allocated by the first context call: engines that never take context keep their
 * footprint. */
/* ---- image memory snapshots: search->kind == GITMI_SEARCH_KEEP takes the encoded memory of resident images out of a context
 * into caller-owned device memory; GITMI_SEARCH_RECALL later puts any selection of kept images -- any order, repeats, from
 * different earlier calls and contexts -- back as the resident batch of any context of the same model.  Every follow-up form
 * (frames == NULL) then runs over the recalled batch unchanged: a late question about an image costs neither the image encoder
 * nor the prefill.  Both are "not a search": gitmi_generate and gitmi_search_begin refuse them by name, the other gitmi_search
 * fields are ignored, both run eagerly (no hipGraph) and synchronise the stream.
 * The store is the CALLER's: ONE device buffer of slots x slot_bytes, 256-byte aligned.  The engine allocates nothing for it and
 * keeps no pointer to it after a call returns.  slot_bytes depends on the engine's configuration alone:
 *     slot_bytes = round_up(256 + cap x (vit_width + dec_layers x 2 x dec_hidden) x esz, 256)
 * cap = max_frames x max(N, max_image_tokens), the rows per image the workspaces are sized for; esz = 4 (GITMI_PREC_F32) or 2.
 * A slot is [256-byte header | cap feature rows | per decoder layer: cap rows of the K | V columns of the prefill]; the first n
 * rows of each are written (n = the image's own key count: image rows + context rows), the rest of a slot is never read.
 * The header: a magic word and a format version; the fingerprint { vit_width, dec_hidden, dec_layers, dec_heads, element size,
 * element dtype (GITMI_DTYPE_*), cap }; n, image rows, context rows, frames F; the image's { h, w } and, for a ragged entry,
 * its rejected flag.  (gitmi_set_ln_fold changes roundings, not what the rows mean: it is not part of the fingerprint.)
 * The slots are plain bytes: copied through host memory or a file and recalled into any context of the same model, precision and
 * capacity they mean the same thing; clones are the main case.  Bytes of another model, precision or capacity are caught by the
 * fingerprint.  The engine CANNOT tell whether the weights are the same: recalling into a context that holds other weights of
 * the same shape is the caller's error and goes unnoticed.
 * KEEP, the argument mapping:
 *   frames          : must be NULL: KEEP runs over the resident images, B = their count (as for every follow-up call).  After
 *                     gitmi_encode_frames alone it runs the prefill first.
 *   logprob_out     : the store's base address (written as bytes), 256-byte aligned;  ld_prefix: the slots it has
 *   image_of_host   : int32 [Q], the resident image entry q keeps, or NULL: Q == B, entry q <-> image q
 *   prefix_len_host : int32 [Q], the destination slot of entry q, in [0, slots), each slot at most once per call
 *   Q               : 1 .. max_batch.  Q == 0 is the size query: info_out[0] = slot_bytes / 256, nothing else is read or
 *                     written (no store, no resident images needed)
 *   info_out        : { slot_bytes / 256, max_q n_q, sum_q n_q, 0 };  prefixes, tokens_out, sent_out: ignored (may be NULL)
 *   One launch writes, for every entry, the header, the image's n feature rows and the K | V columns of its n rows of every
 *   layer (the Q columns are dead after the prefill).  KEEP changes nothing about residency.
 * RECALL, the argument mapping:
 *   frames          : must be NULL; no resident images are needed (what is resident is replaced)
 *   B == Q          : the images to form, 1 .. max_batch;  image_of_host: must be NULL
 *   prefixes        : the store's base address (read as bytes), 256-byte aligned;  ld_prefix: the slots it has
 *   prefix_len_host : int32 [Q], the slot that becomes image q; repeats are allowed
 *   info_out        : { row stride of an image's block, max_q n_q, sum_q n_q, 0 };  tokens_out, logprob_out, sent_out: ignored
 *   The call synchronises the stream, copies the Q headers to the host and validates them BEFORE any launch: the magic and the
 *   version, every field of the fingerprint, 1 <= n <= cap, image rows + context rows == n, the rejected flag clear,
 *   1 <= F <= max_frames and the same F in all slots.  A failure is an argument error whose message names the slot and the
 *   field: nothing is launched and what was resident stays resident.  The kernels form no address from the bytes of a slot:
 *   n reaches them through the validated host copy.  Then one launch scatters every slot's rows into image block q of the
 *   feature tensor and of every layer's prefill K/V, zeroes the rows from n_q up to the block's stride and writes the key
 *   counts (and, in ragged image mode, the per-image descriptors); the decode layouts are rebuilt by the prefill's own repack
 *   launch per layer, so they keep a single writer.  Afterwards the engine is in the state of a prefilled encode.
 *   Mode: if every slot has n == F x N of the engine's current uniform image shape and no context rows, the batch is restored
 *   WITHOUT key counts: exactly the state the original call left, and a follow-up returns what it returned there bit for bit in
 *   every precision.  Otherwise (ragged image mode included) it is a key-count batch, as after a context call: stride =
 *   max_q n_q rounded up to a multiple of 16 where cap allows, attention reads n_q keys of image q, and the batch counts as
 *   context-carrying if any slot has context rows (GITMI_SEARCH_ATTEND keeps its refusal there).  Each sentence gets what a
 *   call with its image alone gets (bit for bit in the f32 mode).
 *   Afterwards gitmi_generate(NULL, ...) with every search, gitmi_generate_prefixed(NULL, ...), GITMI_SEARCH_SCORE, _TREE_SCORE,
 *   _ATTEND and KEEP itself run over the recalled images; the follow-up graph is keyed on B, the stride and the mode already.
 * Both kinds allocate one small device table (max_batch entries) at their first call: engines that never keep or recall keep
 * their footprint. */
/* ---- features in: search->kind == GITMI_SEARCH_FEATURES is the input side of gitmi_encode_frames' feats_out -- the reference's
 * textual(hidden_states = visual_features, ...) / CaptioningModel.infer(batch, visual_features, ...) (decoder.py:845-857,
 * 977-1011).  The caller hands in visual feature rows (what ln_post, plus the temporal embedding of a frame, produces: one row of
 * vit_width elements per image token) and the engine makes them the resident image batch and runs the prefill: cached features,
 * video windows composed from per-frame rows, features averaged over augmentations or produced by another tower of the same
 * width.  Every follow-up form (frames == NULL) then runs unchanged.  "Not a search": gitmi_generate, gitmi_search_begin and the
 * step seam refuse it by name, the other gitmi_search fields are ignored, it runs eagerly (no hipGraph) and synchronises the
 * stream.  The argument mapping:
 *   frames          : must be NULL; no resident images are needed (what is resident is replaced)
 *   B               : the images to form, 1 .. max_batch
 *   F               : the frames per image the caller claims, 1 .. max_frames and <= num_frames where that is > 0; recorded as the
 *                     batch's frame count (KEEP writes it into the slot header), it does not change what is computed
 *   prefixes        : the base address (read as bytes) of the caller's feature rows: DEVICE memory, 16-byte aligned, dense rows of
 *                     vit_width elements.  The caller owns it; the engine keeps no pointer to it after the call returns
 *   search->reserved_ : the element type of the rows: GITMI_DTYPE_F32 (0) or, in a 16-bit engine, gitmi_operand_dtype().  Anything
 *                     else -- the other 16-bit code, a 16-bit code in an fp32 engine -- is refused by name
 *   ld_prefix       : the rows the buffer holds; the host checks every piece against it
 *   Q               : the pieces, 1 .. max_batch x max_frames
 *   image_of_host   : int32 [Q], the image of piece q (NULL: Q == B, piece q <-> image q).  The pieces of one image are concatenated
 *                     in increasing q, any interleaving between images is allowed; every image needs at least one piece
 *   prefix_len_host : int32 [Q][3] = { first source row, rows (>= 1), temporal index t or -1 }.  t >= 0 adds
 *                     img_temperal_embedding[t] to the rows of the piece (0 <= t < num_frames; refused on a model without temporal
 *                     embeddings).  This is independent of gitmi_set_temporal_embedding, which only says how frame TENSORS are read
 *   info_out        : { row stride of an image's block, max_b n_b, sum_b n_b, 0 };  tokens_out, logprob_out, sent_out: ignored
 * With n_b the rows of image b: 1 <= n_b <= cap = max_frames x max(N, max_image_tokens), the rows per image the workspaces are
 * sized for; beyond that the call fails before any launch and the message names the rows asked for and the capacity.
 * vit_width % 8 != 0 is refused by message (a lane moves 8 elements).  Every check comes before the first launch: an argument
 * error leaves the resident set as it was; a failure after the first launch drops it.
 * One launch then writes every row of every image's block -- the rows of the pieces, zeros in rows [n_b, stride) --, the key
 * counts and, in ragged image mode, the per-image descriptors { 0, 0, n_b, 0 }; addresses are formed from the host-validated
 * table alone.  fp32 rows: the embedding is added in fp32 and the sum is stored as the encoder's own ln_post store does it -- as
 * is in an fp32 engine, rounded to nearest even to the operand type otherwise.  16-bit rows without t are copied bit for bit;
 * with t they are widened, added to and rounded once.  The prefill follows, so the engine is in the state of a prefilled encode.
 * Mode, by RECALL's rule: if the engine is not in ragged image mode and every n_b == F x N of the current uniform image shape, the
 * batch is installed WITHOUT key counts -- exactly the state gitmi_encode_frames leaves: the fp32 feats_out of an encode, handed
 * back in, makes every follow-up return what it returns after that encode bit for bit in every precision (so do those rows
 * rounded to the operand type by the caller).  Rows of per-frame encodes composed with t equal the list-form call bit for bit
 * when they came from an encoder pass of the same image count and order; rows of passes of another size may differ by the
 * rounding of another GEMM tile form.  Otherwise it is a key-count batch, as after a context call: stride = max_b n_b rounded up
 * to a multiple of 16 where cap allows, attention reads n_b keys of image b, no context rows; every image gets what a call with
 * its rows alone gets.  GITMI_SEARCH_ATTEND works over both (Kc counts the stride's columns; columns >= n_b are 0).
 * Unlike GITMI_SEARCH_CONTEXT this kind does not need vit_width == dec_hidden: the rows pass through the visual projection.
 * Serving schedule: as for any follow-up it neither waits for nor signals the gitmi_set_encode_after chain.
 * The engine CANNOT tell where the rows came from: features of another model of the same width go unnoticed, as for RECALL.
 * Non-finite or out-of-range values are not looked for here; they surface as info_out[3] of the calls that follow, as today.
 * The device table (max_batch x max_frames pieces, max_batch counts) is allocated by the first such call: engines that never
 * take features keep their footprint. */
/* ---- per-sentence decoding constraints: search->kind == GITMI_SEARCH_CONSTRAIN arms the constraints of the NEXT search call on
 * this context.  It is one-shot: that call consumes them.  Defined against the reference's `step` callable: let row r belong to
 * sentence s = r / beams and hold tokens x[0 .. t), start tokens and prefix (P_s tokens) included.  The constrained step returns
 * the reference's logits with z[c] = -10000 for every token c banned for (r, t); the search class then does what it does after
 * `step` (repetition penalty, the no-immediate-repeat rule, the forced [SEP] of an ended beam, temperature, the sampling filter,
 * log-softmax).  c is banned if any of
 *   set     bit c % 32 of word c / 32 of ban set set_of[s] is set (set_of[s] == -1: no set; an allowed-token list is the
 *           complement, built by the caller),
 *   length  c == eos and t - P_s < min_new[s]: at least min_new[s] generated tokens before [SEP] (0: off),
 *   n-gram  n = ngram[s] in 1 .. 8 (0: off), t >= n, and some i in [0, t - n] has x[i .. i + n - 1) == x[t - n + 1 .. t) and
 *           x[i + n - 1] == c: no n-gram of the row occurs twice (n == 1 bans every token of the history; the history includes
 *           the start tokens, as it does for repetition_penalty)
 * holds.  While a sentence is inside its prefix (t < P_s) the step appends the given token, as always.  -10000 keeps every number
 * finite, so info_out[3] keeps its meaning; a set that bans the whole vocabulary leaves a flat distribution and is the caller's
 * error.  "Not a search": gitmi_generate, gitmi_search_begin and the step seam refuse the kind by name, the other gitmi_search
 * fields are ignored.  The argument mapping:
 *   frames          : must be NULL; F and B are ignored.  Residency is neither needed nor touched
 *   prefixes        : a DEVICE pointer read as uint32 [n_sets][W], W = ceil(vocab / 32); may be NULL when ld_prefix == 0.  The engine
 *                     copies the words into a table of its own on `stream` and keeps no pointer; bits at or above vocab are ignored
 *   ld_prefix       : n_sets, 0 .. max_batch
 *   prefix_len_host : int32 [Q][3] = { set index or -1, min_new, ngram }
 *   image_of_host   : must be NULL
 *   Q               : the sentence count of the call to be constrained, 1 .. max_batch; Q == 0 disarms and reads nothing else
 *   info_out        : { Q, n_sets, W, 0 };  tokens_out, logprob_out, sent_out: ignored
 * Checked on the host before any launch, by message naming sentence and field: set index in [-1, n_sets), 0 <= min_new <=
 * max_text_len, 0 <= ngram <= 8.  A refused call leaves what was armed and what is resident unchanged.
 * Consumption: the next gitmi_generate (kinds 0 and 1) with B == Q, or the next gitmi_generate_prefixed search with that Q, runs
 * constrained and disarms; a follow-up (frames == NULL) works like any other.  Another sentence count is an argument error that
 * names both numbers and stays armed.  While armed, GITMI_SEARCH_TRIE and gitmi_search_begin refuse by name (the seam's caller
 * owns its logits; constraints on the trie search are not implemented).  The other "not a search" kinds run unconstrained and
 * leave the arming alone.  A clone starts disarmed.
 * The tables (the set words and three int [max_batch] arrays) are allocated by the first arming call: engines that never
 * constrain keep their footprint.  The hipGraph key of the decode part gains "constrained"; the values live in those tables, whose
 * pointers never change, so armed calls of equal shape and different values replay one graph.  A constrained 16-bit call runs
 * the vocabulary head in its generic form (the form the repetition penalty uses); an unconstrained call launches what it did.
 *
 * Banned token sequences (an optional extension of the arming call, selected by search->reserved_).  The rule: sentence s may name
 * one list of sequences a = (a_0 .. a_{m-1}), 2 <= m <= 16.  Token c is additionally banned for (r, t) if some sequence of the
 * list has a_{m-1} == c, t >= m - 1 and x[t - m + 1 .. t) == a[0 .. m - 1): the last token of a banned sequence is banned
 * exactly when the row's history (start tokens and prefix included, as for the n-gram rule) ends with the tokens before it.
 * Several sequences may hit at once; the union is banned.  Sequences of one token are bits of the sentence's set and are not
 * part of the extension.
 *   search->reserved_ == 0 is the call above, exactly.
 *   search->reserved_ = n > 0 : sent_out is read as a HOST const int32 [n] pool
 *                     { L, S, T, 0, list_of[Q], list_off[L + 1], seq_off[S + 1], tok[T] }: L lists, S sequences, T tokens;
 *                     list_of[q] the list of sentence q or -1; list l = sequences list_off[l] .. list_off[l + 1] - 1; sequence j =
 *                     tok[seq_off[j] .. seq_off[j + 1]).  Read before the call returns; the engine keeps no pointer.
 * Checked on the host before any launch, by message naming sentence, list and sequence: the sizes add up to n, both offset
 * arrays start at 0, never decrease and end at S and T, every length in [2, 16], every token in [0, vocab), list_of in [-1, L),
 * L <= max_batch, and at most 4096 sequences and 32768 tokens per call.  A vocabulary above 262144 tokens (8192 set words, the LDS
 * budget of the kernel below) is refused too.  A refused call leaves what was armed and what is resident unchanged.
 * The pool travels through page-locked staging to a device table of the engine's own, enqueued on `stream` with no host wait.
 * That table and a buffer of max_batch x max_beams x W words are allocated by the first arming call that carries sequences (their
 * pointers never change afterwards): engines that never use sequences keep their footprint.  info_out is as above.
 * A search armed with sequences launches one more kernel per decode step, before the vocabulary head: one workgroup per row ORs
 * the sentence's set and the last tokens of the sequences the row's history ends with into the row's own W words, which the
 * set rule of that step then reads.  The hipGraph key's "constrained" tells plain, armed and armed with sequences apart; calls of
 * equal shape armed with other sequences replay one graph.  Plain calls and set-only armed calls launch what they did; a set-only
 * arming after one with sequences carries none.  The trie search and the step seam keep refusing while armed. */
/* ---- per-token trace: search->kind == GITMI_SEARCH_TRACE arms the trace of the NEXT search call on this context.  One-shot: that
 * call consumes it and fills the buffers given here.  The rule, for returned sequence o of sentence q (prefix length P_q) and
 * position s: lp[o][s] is the entry of the search class's own class_logprobs for the token at position s, taken from the row
 * whose history is seq[0 .. s), after everything the class does before its log-softmax (the -10000 on the previous token and
 * the forced one-hot [SEP] of an ended beam, decoder.py:330-358; the repetition penalty, temperature and sampling filter of the
 * GENERATOR, decoder.py:1135-1175; armed constraint bans).  lp is 0 for s < P_q (given tokens) and past the end of the sequence.
 *   AUTOREGRESSIVE : positions [P_q, L_q), L_q the returned length (sent_out[2q]); a forced [SEP] after the first one has lp 0.
 *   GENERATOR      : positions [P_q, n_h) of the hypothesis; position n_h, where the output appends [SEP], holds the lp of the
 *                    candidate that finished the hypothesis: [SEP] itself, or the last word when cur_len + 1 == max_steps (the
 *                    reference scores that word and drops it).  Sequences the list could not fill (log-prob -1e5): all 0 / -1.
 *   alternatives   : alt_tok[o][s][j], alt_lp[o][s][j], j < n: the n likeliest tokens of that same distribution, descending, ties
 *                    to the lower token id.  An entry whose lp is -inf (the one-hot rows) is token -1 with lp -inf; prefix positions
 *                    and positions past the end are token -1, lp 0.
 * Sum: sum_s lp[o][s] reproduces logprob_out -- divided by num_valid (AUTOREGRESSIVE) or by len_norm(n_h) (GENERATOR) -- up to
 * the rounding of a sequential fp32 sum.  NOT for a sampled GENERATOR call with beam_size > 1: the reference attaches candidate c
 * to beam c % k but takes its score from beam c / per_node_beam_size (decoder.py:1161-1164); the engine reproduces that, so the
 * running sum does not follow the history there.  The lps themselves are still the scores the search added.
 * If the chosen token ranks below n it appears among the alternatives with the bit-identical lp.
 * The argument mapping:
 *   frames, prefixes, prefix_len_host, image_of_host : must be NULL; F, B, ld_prefix are ignored.  Residency is untouched
 *   Q                     : the sentence count of the call to trace, 1 .. max_batch; Q == 0 disarms and reads nothing else
 *   search->num_keep_best : sequences per sentence that call returns (nout; 0 and 1 both mean one)
 *   search->max_steps     : its max_steps T;   search->reserved_ : n, 0 .. 8
 *   logprob_out           : fp32 [Q * nout][T][1 + n]: column 0 the chosen lp, columns 1 .. n alt_lp
 *   tokens_out            : int64 [Q * nout][T][n] alt_tok, or NULL when n == 0
 *                           both DEVICE or page-locked host buffers, alive until the stream reaches the end of the traced call
 *   info_out              : { Q, nout, T, n }, or NULL: nothing is written and the host does not wait for the stream;  sent_out: ignored
 * Checked on the host before any launch, by message naming the field; a refused call leaves the arming and what is resident
 * unchanged.  Consumption: the next gitmi_generate (kinds 0 and 1), the next gitmi_generate_prefixed search, or the next seam
 * search (gitmi_search_begin consumes it under the kind of the search it starts; gitmi_search_finish fills the buffers).  Another
 * sentence count, nout or T is an argument error that names both numbers and stays armed.  Refused by name: GITMI_SEARCH_TRIE
 * while armed, and n > 0 with do_sample.  Composes with armed constraints (the lps are those after the bans).  A clone starts
 * disarmed.  gitmi_generate and gitmi_search_begin refuse the kind by name.
 * The step of a traced search logs one record per new row (its pick's lp and its parent row's n best) at [position][row]; the
 * beam reordering moves nothing more than it does in a plain call, the record of position s of a final row is found through the
 * same K/V row indirection the attention uses.  The vocabulary head and the whole-row top-M run with max(M, n) candidates; a
 * traced 16-bit call runs the head in its generic form.  The log and the engine's output copies are allocated by the first
 * arming call: engines that never trace keep their footprint, and a call that is not traced launches what it did.  The hipGraph
 * key gains "trace" (0, or 1 + n) and traced calls have graph slots of their own, so plain and traced calls alternate without
 * re-capture and traced calls of equal shape replay one graph. */
int  gitmi_generate_prefixed(gitmi_engine* e, const float* const* frames, int F, int B,
                             const int64_t* prefixes, int ld_prefix, const int32_t* prefix_len_host,
                             const int32_t* image_of_host, int Q, const gitmi_search* search,
                             int64_t* tokens_out, float* logprob_out, int32_t* sent_out, int32_t* info_out,
                             void* stream);

/* ---- search with caller-supplied logits: the seam decoder.search(start, step)
 * (decoder.py:224-231, 1083-1092) for scripted-step parity tests of the device search.
 * begin -> [ next_input -> (caller computes logits) -> advance ]* -> finish. */
/* ---- token trie of GITMI_SEARCH_TRIE: replaces TokenTrie (trie_decoder.py:224-257) as CSR arrays on the host (copied):
 * node 0 is the root; the children of node n are the edges child_off[n] .. child_off[n+1]-1, edge i = (token
 * child_tok[i] -> node child_node[i]), children in insertion order.  At every search step the log-probabilities of the
 * cursor's child tokens are raised by (max - min + 1) of the step's logits before the top-1 (trie_decoder.py:57-71,
 * 115-158) and the cursor follows the choice.  EVERY sentence of a call has its own cursor, i.e. behaves like its own
 * batch-1 reference call (the reference moves one cursor with row 0's choice).  n_nodes == 0 removes the trie. */
int  gitmi_set_trie(gitmi_engine* e, int n_nodes, const int32_t* child_off, const int32_t* child_tok,
                    const int32_t* child_node);

int  gitmi_search_begin(gitmi_engine* e, const gitmi_search* search, int B,
                        const int64_t* start_host, int P, int vocab, void* stream);
/* current rows the `step` callable would receive: int64 [R, cur_len]; returns cur_len via *t */
int  gitmi_search_rows(gitmi_engine* e, int64_t* tokens_out, int* R, int* t, void* stream);
int  gitmi_search_advance(gitmi_engine* e, const float* logits, void* stream);
/* sentences that need no further step (synchronises `stream`): GENERATOR -- sentences whose BeamHypotheses are done
 * (the reference leaves its loop at all(done), decoder.py:1251); AUTOREGRESSIVE -- sentences whose beams all ended with
 * EOS (decoder.py:319).  Steps past *done_out == B are idempotent; a host loop uses this to stop calling `step`. */
int  gitmi_search_done_count(gitmi_engine* e, int* done_out, void* stream);
int  gitmi_search_finish(gitmi_engine* e, int64_t* tokens_out, float* logprob_out,
                         int32_t* info_out, void* stream);

/* ---- profiling ---------------------------------------------------------------------- */
/* on = 1: eager launches with HIP events around phases, decode steps and every GEMM launch (per-kernel durations);
 * on = 2: hipGraph replays with the call split into an (encode + prefill) graph and a decode graph and events
 *         between them -- the production launch path, timed: vit_ms = encode + prefill, decode_ms, decode_step_ms;
 * on = 0: off. */
int  gitmi_profile_enable(gitmi_engine* e, int on);
int  gitmi_profile_read(gitmi_engine* e, gitmi_profile* out);   /* synchronises */
/* use hipGraph replay for gitmi_generate (default 1 unless profiling) */
int  gitmi_set_graph(gitmi_engine* e, int on);

/* ---- single-kernel entry points (unit parity tests through the C ABI).
 * dtype arguments are GITMI_DTYPE_F32 or the library's 16-bit operand type, gitmi_operand_dtype(): GITMI_DTYPE_BF16 in
 * libgitmi.so, GITMI_DTYPE_F16 in libgitmi_f16.so.  The other 16-bit code is refused (the call fails, gitmi_last_error names
 * it).  16-bit tensors of the hooks without a dtype argument (dgemm, dgemm_res, vocab_topm, kv_repack) are in the
 * operand type. ------------------------------- */
/* C[M,N] = act(A[M,K] * W[N,K]^T + bias) (+ residual);  act: 0 none, 1 QuickGELU, 2 erf-GELU.
 * A, W in `in_dtype`; bias fp32 (may be NULL); C in `out_dtype`. K % 64 == 0.  The residual (may be NULL) is fp32 rows,
 * except with out_dtype GITMI_DTYPE_F16_STREAM (16-bit operands, either library): C and the residual are fp16 rows. */
int  gitmi_op_gemm(const void* A, const void* W, const float* bias, const float* residual,
                   void* C, int M, int N, int K, int lda, int ldc, int in_dtype, int out_dtype,
                   int act, void* stream);
/* (ABI 10) the folded-LayerNorm forms of the large-M GEMM, one launch (libgitmi_f16.so only; M > 512, N % 256 == 0, K % 64 == 0):
 *  consumer (ln_part != NULL): C fp16 [M,N] = act(LayerNorm_K(A) W0^T + b0) computed from the RAW fp16 rows A [M,K] with the
 *    folded set W = f16(W0 . gamma) [N,K], bias = beta W0^T + b0, colsum[n] = sum_k W[n][k], ln_part = float2 [M][4]: (sum, sumsq)
 *    of row m over its 256-column tiles (unused slots 0);
 *  producer (ln_part == NULL): fp16 stream rows C [M,N] = A W^T + bias + r, r = residual rows (fp16 [M,N], may be NULL) or
 *    LayerNorm_N(residual rows) rebuilt from res_part / res_gamma / res_beta; part_out = float2 [M][4] of the rows as stored
 *    (N <= 1024).  This is what replaces the LayerNorm modules between the GEMMs of CLIP/model.py:189-202 and
 *    modeling_bert.py:171-178, 243-250 inside the engine (gitmi_set_ln_fold). */
int  gitmi_op_gemm_ln(const void* A, const void* W, const float* bias, const float* colsum, const float* ln_part,
                      float ln_eps, const void* residual, const float* res_part, const float* res_gamma,
                      const float* res_beta, float res_eps, void* C, float* part_out, int M, int N, int K, int act,
                      void* stream);
/* y = LayerNorm(x) (biased variance, eps), x fp32 [rows, D]; y_t (in out_dtype) and/or y_f32 */
int  gitmi_op_layernorm(const float* x, const float* gamma, const float* beta, float eps,
                        void* y_t, float* y_f32, int rows, int D, int out_dtype, void* stream);

/* full (unmasked) multi-head attention over packed qkv [B*N, 3*D] (q|k|v, head h = cols h*64..);
 * out [B*N, D].  impl: 0 = reference VALU kernel, 1 = MFMA flash kernel (16-bit operands only). */
int  gitmi_op_attention(const void* qkv, void* out, int B, int N, int H, int dtype, int impl,
                        void* stream);

/* decode-step GEMM chain (kernels_dgemm.hip; 16-bit operand A [M,K], W [N,K], K % 32 == 0).  BOTH operands are FRAGMENT-MAJOR:
 * 16-row x 32-k tiles in MFMA operand order, element (row, k) at
 *     (((row/16)*(K/32) + k/32)*64 + ((k%32)/8)*16 + row%16)*8 + k%8,   rows padded to a multiple of 16
 * (weights: zero rows; bias / colsum of the vocabulary head padded to a multiple of cols_per_wg), so that every
 * fragment load of a wave is one contiguous 1-KiB read.  The engine repacks weights once and its kernels write
 * activations in this order; xb_out and (with c_frag) C come out fragment-major too.  The post-norm BERT layer
 * (modeling_bert.py:171-178, 243-250) runs WITHOUT LayerNorm launches: the N = hidden GEMMs emit the pre-LayerNorm
 * sum and per-16-column-strip row partials (sum, sum of squares), the consumer GEMM folds the LayerNorm.
 * stats layout: fp32 [strips][M][2].
 *   gitmi_op_dgemm     : C 16-bit [M,N] = act( LN_fold(A) W^T + bias ); stats == NULL: plain A W^T + bias.
 *                        With stats: W must be W . gamma rounded to the operand type, bias = beta W^T + b,
 *                        colsum[n] = sum_k W'[n][k].
 *   gitmi_op_dgemm_res : x = A W^T + bias + r,  r = res_x (res_stats == NULL) or LayerNorm(res_x; res_gamma, res_beta)
 *                        rebuilt from res_stats; writes x fp32, its 16-bit copy and stats_out [N/16][M][2].  N % 16 == 0;
 *                        xb_out is fragment-major over round_up(N, 32) columns (round_up(M, 16) rows of that width; rows
 *                        past M and columns past N are not written).
 *                        strips_per_wg (QKV / FFN1 form, 33..64 rows): 16-column strips a workgroup computes one after
 *                        the other -- 0 / 1 (one workgroup per strip), 2, 4 or 6; results do not depend on it. */
int  gitmi_op_dgemm(const void* A, const void* W, const float* bias, const float* colsum, const float* stats,
                    int strips, float eps, void* C, int c_frag, int M, int N, int K, int act, int strips_per_wg,
                    void* stream);
int  gitmi_op_dgemm_res(const void* A, const void* W, const float* bias, const float* res_x, const float* res_stats,
                        int res_strips, const float* res_gamma, const float* res_beta, float res_eps,
                        float* x_out, void* xb_out, float* stats_out, int M, int N, int K, void* stream);
/* vocabulary head with the search's top-M and log-softmax statistics fused (replaces decoder.py:1054 + the
 * log_softmax/topk of :265-271, 358-366, 1169-1175): per COLUMN BLOCK of cols_per_wg = 128 columns and row, a sorted list
 * of `slots` = {1,2,4,8,16} >= mtop (logit, token) pairs + (max, sum exp):
 * part_val/part_idx [M][ceil(V/128)][slots], part_lse [..][2].  suppress_tok int32 [M] (or NULL): that
 * token's logit counts as -10000 (decoder.py:330).  logits_out fp32 [M,V] optional.  K <= 768.
 * max_wgs: workgroups of the launch -- 0 = one per column block; n > 0 = at most n, each WALKING its column blocks with a
 * rolling refill of the weight registers (at most 8 blocks per workgroup); results do not depend on it.
 * A rows must be readable up to the next multiple of 64, W rows / bias / colsum up to the next multiple of 128. */
int  gitmi_op_vocab_topm(const void* A, const void* W, const float* bias, const float* colsum, const float* stats,
                         int strips, float eps, int M, int V, int K, int cols_per_wg, int mtop,
                         const int* suppress_tok, float* part_val, int* part_idx, float* part_lse,
                         float* logits_out, int max_wgs, void* stream);

/* decode attention for one new text position (unit parity / timing): qkv [R,3d] (R = B*beams), text caches
 * [R][T_max][d] (position `pos` is appended), kv_src int32 [R][T_max], out [R,d].
 *   fp32 : image K/V head-major [B][H][N_img][64] (scalar kernel);
 *   16-bit: image K/V in the matrix-core operand layouts written by gitmi_op_kv_repack (keys padded to 32).
 * dbg: 0, or timing-experiment bits of the fp32 kernel (results undefined). */
int  gitmi_op_attn_decode(const void* qkv, const void* img_k, const void* img_v, void* txt_k, void* txt_v,
                          const int* kv_src, void* out, int B, int H, int N_img, int T_max, int pos, int beams,
                          int dtype, int dbg, void* stream);
/* 16-bit image-row K/V of the decoder prefill ([B*N, 3*H*64] packed q|k|v) -> decode layouts kf / vt, each
 * [B][H][round_up(N,32)][64]: K fragment-major (a wave's MFMA operand is one contiguous 1-KiB read), V transposed with
 * the key slots ordered so that softmax probabilities feed the P V product without leaving their registers. */
int  gitmi_op_kv_repack(const void* qkv_rows, void* kf, void* vt, int B, int N, int H, void* stream);

/* GPU-side image transform == get_image_transform(param) of the reference (inference.py:111-132):
 * Resize(crop, BICUBIC) -> CenterCrop(crop) -> ToTensor -> Normalize(CLIP mean/std), bit-exact with the
 * PIL/torchvision pipeline (Pillow's 8.22 fixed-point resampler is reproduced).  rgb_hwc: uint8 [H,W,3] on
 * the device (a decoded image); tmp: device workspace of >= H * W_resized * 3 bytes; out_chw: fp32 [3,crop,crop]. */
int  gitmi_preprocess_image(const uint8_t* rgb_hwc, int H, int W, int crop, uint8_t* tmp, size_t tmp_bytes,
                            float* out_chw, void* stream);
/* the same transform for a BATCH: n decoded images of any sizes lie in ONE device buffer `rgb` (rgb_bytes long; one upload per
 * batch), desc_host is a HOST array int64 [n][3] = (byte offset of image i, H, W).  One launch pair per 24 images instead of one
 * per image: at ~10k images/s the per-image form is bound by the submitting host thread, not by the device.
 * tmp: device workspace of >= sum_i H_i * W_resized_i * 3 bytes (+ 64 per image); out: fp32 [n, 3, crop, crop].
 * Bit-identical to n calls of gitmi_preprocess_image. */
int  gitmi_preprocess_batch(const uint8_t* rgb, size_t rgb_bytes, const int64_t* desc_host, int n, int crop, uint8_t* tmp,
                            size_t tmp_bytes, float* out, void* stream);
/* same arithmetic for MinMaxResizeForTest (inference.py:29-64, the test_respect_ratio_max models): resize to
 * out_h x out_w (the caller applies get_size()), no crop, ToTensor, Normalize -> fp32 [3, out_h, out_w].
 * tmp: uint8 workspace of H * out_w * 3 bytes. */
int  gitmi_preprocess_image_to(const uint8_t* rgb_hwc, int H, int W, int out_h, int out_w, uint8_t* tmp,
                               size_t tmp_bytes, float* out_chw, void* stream);

/* one step of the sampling branch of GeneratorWithBeamSearch.search on caller-supplied fp32 logits [R, V]
 * (decoder.py:1146-1166, 1343-1375): filtered_out (optional) receives top_k_top_p_filtering(logits / temperature,
 * min_tokens_to_keep = 2) with -inf for removed tokens; draw_token / draw_logprob [R, ndraw] the draws (without
 * replacement, in draw order) and their log-probabilities under the filtered softmax.  Synchronises the stream. */
int  gitmi_op_sample_rows(const float* logits, int R, int V, float temperature, int top_k, float top_p, int ndraw,
                          uint64_t seed, int step, float* draw_logprob, int* draw_token, float* filtered_out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GITMI_H_ */
