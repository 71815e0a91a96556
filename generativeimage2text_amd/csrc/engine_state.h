// Host state of the GIT engine, shared by engine.hip (schedule, search seam, generate / graph, scoring, setters, profiling)
// and engine_weights.hip (weight ingest, LayerNorm folds, clones, workspaces): the packed weights a clone borrows, the
// policy a clone inherits, and the per-context state every context owns.
#pragma once
#include "../../include/gitmi.h"
#include "abi_common.h"
#include "launchers.h"

#include <hip/hip_runtime.h>

#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <vector>

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// sequences a search returns per sentence (GeneratorWithBeamSearch's num_keep_best; 0 and 1 both mean one)
static inline int keep_best(const gitmi_search& sp) { return sp.num_keep_best > 1 ? sp.num_keep_best : 1; }

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    float amax = 0.f;                   // max |value| (gitmi_load_tensor; every value is finite)
    size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

// a matrix with the LayerNorm in front of it folded in (engine_weights.hip fold_layernorm): 16-bit(W . gamma),
// beta W^T + bias, column sums of the rounded matrix
struct Folded { void* w = nullptr; float* bias = nullptr; float* colsum = nullptr; };

struct VitLayerW {
    void *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;
    float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
    float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
    // LayerNorm folded into the consumer GEMM (fp16-operand build, kernels_gemm10.hip LNF), row-major
    Folded qkv_f;                       // ln_1
    Folded ffn1_f;                      // ln_2
};
struct DecLayerW {
    void *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;
    float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
    float *lnag = nullptr, *lnab = nullptr, *lnog = nullptr, *lnob = nullptr;
    // decode chain (bf16 mode): the LayerNorm in front of a GEMM folded into its weights (kernels_dgemm.hip).
    // All decode-chain matrices are fragment-major copies (gitmi_common.h frag_offset), rows padded to 16.
    Folded qkv_f;                       // previous layer's output LayerNorm (layer 0: plain, colsum == nullptr)
    Folded ffn1_f;                      // this layer's attention-output LayerNorm
    void *wo_p = nullptr, *w2_p = nullptr;                                 // plain, packed
    // prefill (image rows, large M): the same two folds in ROW-MAJOR layout for gemm_p8_kernel (layer 0: the visual projection's LayerNorm)
    Folded qkv_pf, ffn1_pf;
};

struct TimedSpan { hipEvent_t a, b; int tag; double flops; };
enum { TAG_VIT = 0, TAG_PREFILL = 1, TAG_DECODE = 2, TAG_GEMM_VIT = 10, TAG_GEMM_OTHER = 11, TAG_STEP = 20 };

// hipGraph cache key of gitmi_generate / gitmi_generate_prefixed: everything the captured launch sequence depends on
struct GraphKey {
    int B, Q, F, P, kind, k, pn, T, H, W, prefixed, ident, temb, resident, Nimg, keyed; double lp;
    int smp, top_k, nh; double top_p, temp, rp; unsigned long long seed;
    // 0 plain, 1 the decode part runs under armed constraints, 2 under constraints with banned sequences (one more launch per
    // step); their VALUES live in the engine's tables, not in the key
    int constrained;
    int trace;          // 0, or 1 + n: the decode part logs its picks (GITMI_SEARCH_TRACE) and the head lists hold max(M, n) candidates
    // resident: a follow-up call (frames == NULL) -- the decode part alone, over the images the engine holds: Nimg rows per
    // image block, with (keyed) or without per-image key counts; both 0 in a call with frames, which decides them itself
    auto fields() const {
        return std::tie(B, Q, F, P, kind, k, pn, T, H, W, prefixed, ident, temb, resident, Nimg, keyed, lp, smp, top_k, nh, top_p, temp,
                        rp, seed, constrained, trace);
    }
    bool operator==(const GraphKey& o) const { return fields() == o.fields(); }
};
struct GraphSlot { GraphKey key{}; bool valid = false; };

// one captured launch sequence: the hipGraph of a stream capture and its executable
struct CapturedGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    void reset() {
        if (exec) hipGraphExecDestroy(exec);
        if (graph) hipGraphDestroy(graph);
        exec = nullptr, graph = nullptr;
    }
    // replaces the graph by what fn() enqueues on `s` (engine.hip); on a failure of fn or of the capture the slot is left empty
    int capture(hipStream_t s, const std::function<int()>& fn);
    hipError_t launch(hipStream_t s) const { return hipGraphLaunch(exec, s); }
};

// what one gitmi_generate / gitmi_generate_prefixed call is (built once by the entry point; the capture paths pass a copy
// whose frames and outputs are the engine's own buffers).  start_dev / plen_dev / img_of_dev describe the Q sentences.
struct Request {
    const float* const* frames;         // F frames of B images, or nullptr: a follow-up call over the resident images
    int F, B, Q, minP, maxP;            // Q sentences with prefix lengths in [minP, maxP]
    bool prefixed;
    const gitmi_search* sp;
    long long* tokens; float* logprob; int32_t* info;
    int32_t* sent;                      // the caller's buffer, or e->out_sent
};

// packed weights on the device: produced by gitmi_finalize_weights, borrowed (the same pointers) by every clone
struct ModelWeights {
    void* conv_w = nullptr;
    float *cls = nullptr, *pos = nullptr, *lnpre_g = nullptr, *lnpre_b = nullptr, *lnpost_g = nullptr, *lnpost_b = nullptr;
    std::vector<VitLayerW> vit;
    std::vector<float*> temb;
    void* vp_w = nullptr;
    float *vp_b = nullptr, *vp_lng = nullptr, *vp_lnb = nullptr;
    float *words_f = nullptr, *positions_f = nullptr, *emb_lng = nullptr, *emb_lnb = nullptr;
    std::vector<DecLayerW> dec;
    void* out_w = nullptr;
    float* out_b = nullptr;
    Folded out_f;                       // vocabulary head folded with the last layer's output LayerNorm (bf16 mode)
    double dec_weight_bytes = 0;
};

// what a clone inherits from its source besides the weights, as it stands when the clone is made
struct Policy {
    bool f32 = false;
    size_t esz = 2;
    int attn_impl = 1;          // 1 = MFMA flash kernel for full attention (bf16), 0 = VALU kernel
    // residual streams of the image encoder and the prefill (v_x, p_y, p_hf) stored in fp16 instead of fp32 (bf16 mode
    // only, the default there; GITMI_STREAM_F16=0 keeps fp32): half the bytes of their read-modify-writes at 2^-11 relative
    // rounding.  Measured (profiles/r03_a_bench_f16_*.json, interleaved A/B): encode + prefill 5.31 -> 5.03 ms,
    // 9.48k -> 9.82k captions/s, logit error 0.01118 -> 0.01094, the same 50 of 64 rows identical to the reference.
    bool stream_f16 = false;
    // LayerNorm folding in the encoder and the prefill (round 6; fp16-operand build only: the fp16 stream rows are the
    // consumer GEMM's A operand as they are)
    bool ln_fold = false;
    bool ln_fold_ready = false;         // folded matrices and partial buffers exist (decided at gitmi_create; gitmi_set_ln_fold switches the use)
    bool skinny = true;                 // bf16 decode steps through the folded-LayerNorm GEMM chain (kernels_dgemm.hip)
    bool use_graph = true;
    bool use_temb = true;               // add img_temperal_embedding[i] to frame i (the reference does so only for a LIST of frames)
    bool shared_device = false;         // gitmi_set_shared_device: other contexts run beside this one
    int attn_dbg = 0, dgemm_dbg = 0;    // timing experiments (GITMI_ATTN_DBG, GITMI_DGEMM_DBG)
    int attn_pw = 0;                    // (sentence, head) pairs per workgroup of the decode attention (GITMI_ATTN_PW; 0 = by policy)
    int attn_nh = 0;                    // waves per (sentence, head) pair of the decode attention (GITMI_ATTN_NH: 1 / 2)
    int attn_stream = -1;               // workgroups of the streaming decode attention (0 = register kernels; -1 = by policy)
    int dgemm_no_row_walk = -1;         // A/B (GITMI_DGEMM_NO_ROW_WALK=0|1; -1 = by policy)
    int dgemm_strips = -1;              // 16-column strips per workgroup of the wide chain GEMMs at <= 64 rows (1, 2, 4, 6; -1 = by policy)
    int vocab_wgs = -1;                 // workgroups of the vocabulary head (each walks ceil(239 / n) column blocks; 0 = one per block; -1 = by policy)
    int gemm_tall = 1;                  // serving policy: encoder GEMMs always on 256-row tiles (1) or on the modelled height (0; GITMI_GEMM_TALL)
    int dgemm_rows = 0;                 // rows per workgroup of the N = 768 chain GEMMs (GITMI_DGEMM_ROWS: 16 / 32 / 64; 0 = by policy)
    int decode_skip = 0;                // MEASUREMENT BUILDS ONLY (GITMI_EXPERIMENT, GITMI_DECODE_SKIP): launches of the decode chain left
                                        // out -- 1 attention, 2 QKV / FFN1 GEMMs, 4 out-proj / FFN2 GEMMs, 8 vocabulary head, 16 the QKV GEMM alone
                                        // (ids are garbage)
};

struct gitmi_engine {
    gitmi_config cfg{};
    ModelWeights w;
    Policy pol;
    int device = 0;
    bool finalized = false;
    gitmi_engine* parent = nullptr;   // clone: packed weights are borrowed from this engine

    std::map<std::string, HostTensor> host_w;
    std::vector<void*> allocs;

    // derived dims (init_geometry): N/gh/gw/H/W describe the CURRENT input resolution (gitmi_set_image_shape); *_nat the stored grid
    int N = 0, gh = 0, gw = 0, H = 0, W = 0, Kp = 0, Kp_pad = 0;
    int N_nat = 0, g_nat = 0, Nmax = 0;
    size_t max_pixels = 0;
    float* pos_var = nullptr;          // [Nmax, D] positional table resized to the current grid
    const float* pos_cur = nullptr;    // w.pos (native grid) or pos_var
    // ragged batches (gitmi_set_image_shape(e, 0, 0)): every image of a call has its own size, read from the input's
    // descriptor on the device; image b owns rows [b * Nmax, b * Nmax + ntok[b]) of the encoder / prefill blocks (N = Nmax)
    bool ragged = false;
    int4* rg_meta = nullptr;           // [max_batch] {h, w, ntok, rejected} of the staged call
    int* rg_ntok = nullptr;            // [max_batch] key rows of every image: its token rows (class token included) in a ragged
                                       // batch, image rows + context rows after a context call
    // key counts in use: prefill attention, decode attention and the text pass read rg_ntok for the resident batch.  True for
    // every ragged batch and for a batch that carries context rows (GITMI_SEARCH_CONTEXT); the ragged FRONT END is `ragged` alone
    bool keyed = false;
    bool has_context = false;          // the resident images' blocks are [image rows | context rows | zeros], cur_Nimg rows each
    int* ctx_tab = nullptr;            // segment table of the last context call (engine.hip context_call), grown on demand
    size_t ctx_tab_ints = 0;
    // image memory snapshots (GITMI_SEARCH_KEEP / _RECALL, engine.hip memory_keep / memory_recall): the device table of a call,
    // allocated by the first such call, and what only the host knows about the resident images: {image rows, context rows, h, w}
    // of each after a context call or a recall (empty: every image is cur_Nimg image rows of the current shape, or -- ragged
    // front end -- what rg_meta says)
    gitmi::MemoryEntry* mem_tab = nullptr;
    size_t mem_tab_n = 0;
    std::vector<int4> res_desc;
    // features in (GITMI_SEARCH_FEATURES, engine.hip features_call): the device table of a call -- max_batch x max_frames pieces,
    // then max_batch row counts --, allocated by the first such call
    gitmi::FeaturePiece* feat_tab = nullptr;
    // per-sentence decoding constraints (GITMI_SEARCH_CONSTRAIN, engine.hip constrain_call): the engine's own copy of the ban
    // sets (uint32 [max_batch][ceil(vocab / 32)]) and, behind them, set_of | min_new | ngram (int [3][max_batch]), allocated
    // by the first arming call -- the pointers never change afterwards, so captured graphs stay valid whatever the values.
    // ban_armed: the sentence count the constraints are armed for (0: disarmed); the next search call consumes them.
    // ban_live: the search in progress runs constrained (decode_head_impl hands the tables to the head); set and cleared by generate_run.
    unsigned int* ban_words = nullptr;
    int* ban_stage = nullptr;           // page-locked staging of the table (+ info_out): the arming call enqueues copies, it does not wait
    hipEvent_t ban_staged = nullptr;    // the last copy out of ban_stage
    int ban_armed = 0;
    bool ban_live = false;
    // per-token trace (GITMI_SEARCH_TRACE, engine.hip trace_call): trace_armed = the sentence count the trace is armed for (0:
    // disarmed) with the nout / T / n and the caller's buffers of the arming; the next search call consumes them.  trace_live: the
    // search in progress is traced (the fields then describe it).  trace_buf: one device allocation, made by the first arming call
    // and grown by a larger one (captured traced graphs go with it), carved by trace_args / trace_out_*.
    int trace_armed = 0, trace_nout = 0, trace_T = 0, trace_n = 0;
    int trace_Q = 0;                    // the sentence count of the arming, kept when a call consumes it (the carving depends on it)
    float* trace_user_lp = nullptr; long long* trace_user_tok = nullptr;
    bool trace_live = false;
    char* trace_buf = nullptr; size_t trace_bytes = 0;
    // banned token sequences (the extension of GITMI_SEARCH_CONSTRAIN selected by search->reserved_): the device table ban_seq =
    // list_of [max_batch] | list_off [max_batch + 1] | seq_off [BAN_SEQ_MAX_SEQS + 1] | tok [BAN_SEQ_MAX_TOKS] at fixed offsets, its
    // page-locked staging twin (guarded by ban_staged, like ban_stage) and the per-row sets ban_row_words (uint32 [max_batch x
    // max_beams][W], written by ban_rows_kernel before the head of every step) -- allocated by the first arming call that
    // carries sequences, pointers fixed afterwards.  ban_seq_armed: the armed constraints carry sequences; ban_seq_live: so does
    // the search in progress.
    int* ban_seq = nullptr;
    int* ban_seq_stage = nullptr;
    unsigned int* ban_row_words = nullptr;
    bool ban_seq_armed = false;
    bool ban_seq_live = false;

    // ViT workspaces (one frame of max_batch images at a time)
    void *patches = nullptr, *v_h = nullptr, *v_qkv = nullptr, *v_ctx = nullptr, *v_u = nullptr;
    float *patch_out = nullptr, *v_x = nullptr;
    // visual features [B, F*N, vfs]
    void* feats = nullptr;
    // prefill workspaces
    float *p_y = nullptr, *p_hf = nullptr;
    void *p_ht = nullptr, *p_ctx = nullptr, *p_u = nullptr;
    std::vector<void*> img_kv;      // per layer [B*N_img, 3d] (prefill layout)
    std::vector<void*> img_kh, img_vh;   // per layer head-major [B][H][N_img][64] (decode layout)
    // decode workspaces
    float *d_y = nullptr, *d_hf = nullptr, *logits = nullptr;
    void *d_ht = nullptr, *d_qkv = nullptr, *d_ctx = nullptr, *d_u = nullptr;
    std::vector<void*> txt_k, txt_v;   // per layer [R_max, T_max, d]
    int ldl = 0;
    // decode chain workspaces: pre-LayerNorm sums of the two N = d GEMMs of a layer (fp32 + bf16) and their strip partials
    float *xa_f = nullptr, *xo_f = nullptr;
    void *xa_b = nullptr, *xo_b = nullptr;
    float2 *stats_a = nullptr, *stats_o = nullptr;
    // per-step candidate lists [R][nparts][slots] (+ (max, sum exp) per part)
    float* part_val = nullptr; int* part_idx = nullptr; float2* part_lse = nullptr;
    int vocab_cols = 128, vocab_nparts = 1;
    // search
    gitmi::SearchState ss{};
    int ss_cur = 0, ss_len = 0;
    long long* start_dev = nullptr;     // [max_batch][max_text_len] start tokens of every sentence
    int *plen_dev = nullptr, *img_of_dev = nullptr;
    bool img_identity = true;           // sentence b attends to image b
    // token trie of trie-constrained greedy decoding (gitmi_set_trie; trie_decoder.py) + one cursor per sentence
    int *trie_off = nullptr, *trie_tok = nullptr, *trie_child = nullptr, *trie_cursor = nullptr;
    bool trie_search = false;           // the current search is GITMI_SEARCH_TRIE
    gitmi_search sample{};              // sampling parameters of the current search (do_sample, top_k, top_p, temperature, seed)
    std::vector<int> plen_host, img_of_host;

    // state of the current batch.  have_feats also means "these images are RESIDENT": a follow-up call (frames == NULL,
    // include/gitmi.h) searches or scores over them without encoding.  Set at the end of an encode, cleared when an encode
    // starts (so a call that fails half-way leaves none) and by every setter that changes what an encode would produce.
    int cur_B = 0, cur_F = 0, cur_Nimg = 0;
    bool have_feats = false, have_prefill = false;

    // profiling: 1 = eager launches with HIP events around phases, decode steps and every GEMM;
    //            2 = hipGraph replays, the call split into an encode graph and a decode graph with events between them
    //                (what the production path costs: no per-launch host work, no event records inside the chain)
    int profile_mode = 0;
    bool profiling = false;             // profile_mode == 1
    // LayerNorm folding (pol.ln_fold): row partials (sum, sumsq) per 256-column tile: [rows][4], ping-pong for the
    // post-norm prefill (a producer tile reads the previous partials of a row while another tile writes the new ones)
    float2 *v_part = nullptr, *p_part[2] = {nullptr, nullptr};
    hipEvent_t gev[3] = {nullptr, nullptr, nullptr};
    // serving schedule: this context's image encoder starts only after `enc_after`'s has finished (at most one encoder
    // in flight on the device; decode chains of the other contexts fill in beside it)
    gitmi_engine* enc_after = nullptr;
    std::vector<gitmi_engine*> enc_watchers;   // contexts whose enc_after is this one (they wait on enc_done)
    hipEvent_t enc_done = nullptr;
    double split_encode_ms = 0, split_decode_ms = 0;
    int split_calls = 0, split_steps = 0;
    std::vector<TimedSpan> spans;
    std::vector<hipEvent_t> event_pool;
    size_t event_next = 0;
    double last_decode_step_bytes = 0;

    // hipGraph cache for gitmi_generate: a full call replays graph_full (the whole call) or, when something has to happen
    // between the two (graph_is_split), graph_full (encode + prefill) and graph_decode; both belong to full_slot.  A
    // follow-up call replays graph_follow (the decode part alone, GraphKey::resident) of follow_slot, so that full and
    // follow-up calls with unchanged arguments alternate without re-capturing either
    // graphs[1]: the same for traced calls (GITMI_SEARCH_TRACE), so that plain and traced calls alternate without re-capturing
    struct GraphSet {
        CapturedGraph graph_full, graph_decode, graph_follow;
        GraphSlot full_slot, follow_slot;
        bool graph_is_split = false;
    } graphs[2];
    std::vector<float*> frame_stage;   // engine-owned copies of the input frames (graph inputs)
    long long* out_tokens = nullptr;   // graph outputs, copied to the caller's buffers after the launch
    float* out_lp = nullptr;
    int* out_info = nullptr;
    int* out_sent = nullptr;           // [max_batch][2] per-sentence (length, early) of the last generate
    hipStream_t own_stream = nullptr;  // used when the caller passes the (uncapturable) null stream
    hipEvent_t fence_in = nullptr, fence_out = nullptr;

    // caption scoring (GITMI_SEARCH_SCORE, kernels_score.hip): workspaces of the text pass over (sentence, position) rows,
    // allocated by the first score call and grown to the rows of a larger call (score_alloc)
    size_t sc_rows = 0;                 // rows the current workspaces hold (0: none)
    std::vector<void*> sc_allocs;
    float *sc_hf = nullptr, *sc_y = nullptr, *sc_zt = nullptr;
    void *sc_ht = nullptr, *sc_qkv = nullptr, *sc_ctx = nullptr, *sc_u = nullptr;
    float4* sc_part = nullptr;
    int *sc_tgt = nullptr, *sc_lens = nullptr, *sc_img = nullptr, *sc_bad = nullptr, *sc_info = nullptr;
    float2* sc_out = nullptr;
    // token trees (GITMI_SEARCH_TREE_SCORE): the node tables (int32 [4][sc_rows]: token, depth, parent, end) and the [Q, ld]
    // output of a call, part of score_alloc's set once a tree call asked for them (tr_out_n: output elements held, 0: none)
    size_t tr_out_n = 0;
    int* tr_nodes = nullptr;
    float2* tr_out = nullptr;
    // attention maps (GITMI_SEARCH_ATTEND): the softmax statistics of one layer's text rows and the [Q, ld, layers, Kc] output,
    // allocated by the first attend call and grown on demand (attend_alloc)
    size_t at_floats = 0, at_stat_rows = 0;
    float* at_out = nullptr;
    float2* at_stats = nullptr;
};

namespace gitmi {
// the dims derived from cfg, at the native resolution (non-ragged): gitmi_create and gitmi_clone
void init_geometry(gitmi_engine* e);
}  // namespace gitmi
