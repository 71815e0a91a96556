// Host-side declarations of the kernel launchers (definitions live next to the kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace gitmi {

struct GemmArgs {
    const void* A; const void* W; const float* bias; const float* res; void* C;
    int M, N, K;
    int lda, ldc, ldr;
    int act;
    int tiles_n, nwg;
    int ng;     // XCD tile partition: N split into ng groups, M into 8/ng (kernels_gemm10.hip)
    int dbg;    // measurement builds only (gemm_p8_kernel): 1 no C stores, 2 no epilogue, 4 no MFMA, 8 no loads in loop
    int out_f16; // C and `res` are f16_t rows (residual stream of the bf16 engine mode); bf16 inputs, p8 + generic kernel only
    int shared;  // other contexts run beside this launch (serving schedule): tile choice by FLOP/byte, not by round fill
    // ---- LayerNorm folded into the large-M GEMMs (gemm_p8_kernel, fp16-operand build; kernels_gemm10.hip) ----
    // Row partials are [M][4] float2 (sum, sumsq), slot t = the 256-column tile t of the row (hidden sizes <= 1024; unused slots 0).
    // consumer (QKV / c_fc / FFN1): A = the RAW fp16 residual-stream rows, W = f16(W . gamma), bias = beta W^T + b, and
    //   C = act(rstd_m (A W^T - mean_m colsum) + bias); (mean, rstd) of row m from ln_part[m][0..4)
    const float2* ln_part; int ln_nparts; const float* ln_colsum; float ln_inv_d, ln_eps;
    // producer (N = hidden GEMMs writing stream rows): (sum, sumsq) of the STORED fp16 values of row m over the 256 columns
    //   of tile t -> part_out[m][t]
    float2* part_out;
    // post-norm residual: `res` points at RAW rows, the residual added is LayerNorm(res) rebuilt from res_part / res_gamma / res_beta
    const float2* res_part; int res_nparts; const float* res_gamma; const float* res_beta; float res_inv_d, res_eps;
};
bool gemm_uses_p8(const GemmArgs& g, bool in_f32, bool out_f32);   // would launch_gemm run this shape on gemm_p8_kernel?
hipError_t launch_gemm(const GemmArgs& g, bool in_f32, bool out_f32, hipStream_t s);
hipError_t launch_gemm_p8(GemmArgs g, bool out_f32, hipStream_t s);     // 256x256x64, half-tile pipeline, staggered wave groups
bool gemm_p8_supports(const GemmArgs& g);
int gemm_p8_cost(const GemmArgs& g, int bm);   // modelled launch time (ns) with bm-row tiles: rounds x (prologue + K loop + epilogue)
bool set_gemm_impl(int impl);   // measurement builds: -1 auto, 0 tile kernel only, 9 LDS-DMA kernel wherever it can run (+ dbg bits << 8); false = unknown selector

// ---- decode-step GEMM chain (kernels_dgemm.hip): LayerNorm folded into the consumer, row partials from the producer
struct DGemmArgs {
    const unsigned short* A; const unsigned short* W;   // bf16 [M, K], [N, K], BOTH fragment-major (gitmi_common.h frag_offset)
    const float* bias;          // [N]  bias, or the folded constant  beta W^T + bias
    const float* colsum;        // [N]  sum_k bf16(W gamma)[n][k] when the input LayerNorm is folded, else nullptr
    const float2* stats_in;     // [strips_in][M] (sum, sumsq) strip partials of the folded LayerNorm's input (nullptr: none)
    int strips_in; float inv_d, eps_in;
    void* C;                    // bf16 [M, ldc] output of the QKV / FFN1 form (row-major), or fragment-major [M, N] when c_frag
    int c_frag;
    // N = 768 form: x_out = A W^T + bias + residual (+ bf16 copy + strip partials of x_out)
    const float* res_x;         // fp32 [M, N]: the hidden state, or the raw x the residual LayerNorm is rebuilt from
    const float2* res_stats; int res_strips; const float* res_gamma; const float* res_beta; float res_inv_d, res_eps;
    float* x_out; unsigned short* xb_out; float2* stats_out;
    int M, N, K, lda, ldc, act;
    int dbg;                    // timing experiments only: 1 no activation loads, 2 no weight loads, 4 no MFMA, 8 no epilogue loads
    int rows_per_wg;            // N = 768 form: rows per workgroup (0 / 16 default, 32, 64)
    int strips_per_wg;          // wide form, 33..64 rows: 16-column strips per workgroup, one after the other (1, 2, 4, 6; serving policy: 2)
    int no_row_walk;            // A/B: wide form over > 64 rows as one workgroup per (strip, row block) instead of the row-walking kernel
};
hipError_t launch_dgemm(const DGemmArgs& g, hipStream_t s);
// The two argument records of the chain (the policy fields rows_per_wg / strips_per_wg / no_row_walk / dbg stay 0: the caller's).
// DLn: a LayerNorm of the chain, i.e. the strip partials of the rows it normalises and its (gamma, beta, eps)
struct DLn { const float2* stats; int strips; float inv_d, eps; const float* gamma; const float* beta; };
// consumer: C = act(LayerNorm(A) W^T + b) with the LayerNorm folded into (W, bias, colsum); ln == nullptr: plain A, colsum is not read
inline DGemmArgs dgemm_ln(const void* A, const void* W, const float* bias, const float* colsum, const DLn* ln, void* C, int c_frag,
                          int act, int M, int N, int K) {
    DGemmArgs g{};
    g.A = (const unsigned short*)A; g.lda = K; g.W = (const unsigned short*)W; g.bias = bias;
    if (ln) { g.colsum = colsum; g.stats_in = ln->stats; g.strips_in = ln->strips; g.inv_d = ln->inv_d; g.eps_in = ln->eps; }
    g.C = C; g.ldc = N; g.c_frag = c_frag; g.act = act; g.M = M; g.N = N; g.K = K;
    return g;
}
// producer: x_out = A W^T + b + residual (res_x itself, or LayerNorm(res_x) rebuilt from res_ln), its bf16 copy and strip partials
inline DGemmArgs dgemm_to_stream(const void* A, const void* W, const float* bias, const float* res_x, const DLn* res_ln, float* x_out,
                                 void* xb_out, float2* stats_out, int M, int N, int K) {
    DGemmArgs g{};
    g.A = (const unsigned short*)A; g.lda = K; g.W = (const unsigned short*)W; g.bias = bias; g.res_x = res_x;
    if (res_ln) {
        g.res_stats = res_ln->stats; g.res_strips = res_ln->strips; g.res_gamma = res_ln->gamma; g.res_beta = res_ln->beta;
        g.res_inv_d = res_ln->inv_d; g.res_eps = res_ln->eps;
    }
    g.x_out = x_out; g.xb_out = (unsigned short*)xb_out; g.stats_out = stats_out; g.M = M; g.N = N; g.K = K;
    return g;
}

// ---- per-sentence decoding constraints (GITMI_SEARCH_CONSTRAIN, include/gitmi.h; the rule itself: ban_rules.h) ----
// The engine's own tables of an armed call (DEVICE, host-validated): `words` uint32 [n_sets][W] ban sets, bit c % 32 of word
// c / 32 = token c; per sentence set_of (-1: none), min_new, ngram (0: off, else 1..8).  set_of == nullptr: unconstrained.
// row_words (or nullptr: as without it) uint32 [rows][W]: the row's own set for this step -- its sentence's set OR the last tokens
// of the banned sequences its history ends with (ban_rows_kernel) -- read in place of words[set_of].
struct BanArgs {
    const unsigned int* words; const int* set_of; const int* min_new; const int* ngram;
    int W, eos;
    const unsigned int* row_words;
};
// Banned token sequences of an armed call (the host-validated pool of GITMI_SEARCH_CONSTRAIN's extension, DEVICE): sentence q
// names list list_of[q] (-1: none) = sequences list_off[l] .. list_off[l + 1] - 1, sequence j = tokens tok[seq_off[j] ..
// seq_off[j + 1]), 2 .. BAN_SEQ_MAX_LEN of them, every token in [0, vocab).
struct BanSeqArgs {
    const int* list_of; const int* list_off; const int* seq_off; const int* tok;
};
constexpr int BAN_SEQ_MAX_LEN = 16;         // tokens of one banned sequence
constexpr int BAN_SEQ_MAX_SEQS = 4096;      // sequences of one arming call (all lists)
constexpr int BAN_SEQ_MAX_TOKS = 32768;     // their tokens
constexpr int BAN_ROW_MAX_WORDS = 8192;     // set words ban_rows_kernel holds in LDS (32 KB: vocabularies up to 262144 tokens)
// one workgroup per row: row_words[row] = set of the row's sentence | last tokens of the sequences its history ids[row][0 .. t) ends
// with.  ban: words / set_of / W are read.  Refuses (invalid value) W outside [1, BAN_ROW_MAX_WORDS], beams < 1, t < 1.
hipError_t launch_ban_rows(const BanArgs& ban, const BanSeqArgs& seq, const int* ids, int ld_ids, int t, int rows, int beams,
                           unsigned int* row_words, hipStream_t s);

// vocabulary head with the running top-M / log-sum-exp fused: one sorted candidate list per (row, workgroup)
struct VocabArgs {
    const unsigned short* A; int lda; const unsigned short* W; const float* bias; const float* colsum;
    const float2* stats_in; int strips_in; float inv_d, eps_in;
    int M, N, K, cols_per_wg;
    // no-immediate-repeat rule (decoder.py:330): rows of AUTOREGRESSIVE sentences past their first search step
    const int* ids; int ld_ids, cur_len; const int* plen; int beams, suppress_kind;
    float rep_penalty;          // GENERATOR repetition penalty over ids[row][0..cur_len) (decoder.py:1135-1144); 0 or 1: off
    float* part_val; int* part_idx; float2* part_lse;     // [M][column blocks][slots], [M][column blocks] (max, sum exp)
    float* logits_out; int ld_logits;                      // optional full logits (teacher-forced parity hook)
    int max_wgs;                // workgroups of the launch (0: one per column block); fewer = each walks several column blocks
    int nblk;                   // column blocks (set by the launcher)
    // decoding constraints of the rows' sentences (ids / plen / beams / cur_len above describe the rows); VOC_GENERIC only --
    // the launcher sends a constrained call there, VOC_GREEDY / VOC_BEAM never read these fields
    BanArgs ban;
};
// generic: run the generic form whatever the shape (a traced call, whose lists hold max(M, n) candidates)
hipError_t launch_vocab_topm(const VocabArgs& g, int mtop, hipStream_t s, bool generic = false);
int vocab_parts(int V, int cols_per_wg);
int vocab_mtop_slots(int mtop);

hipError_t launch_layernorm(const float* x, int ldx, const float* gamma, const float* beta, float eps,
                            const float* add_after, void* y_t, int ld_t, bool t_is_f32, float* y_f, int ld_f,
                            int rows, int D, int map_n_in, int map_n_out, int map_off, hipStream_t s);
hipError_t launch_im2col(const float* img, void* out, bool out_f32, int B, int H, int W, int p, int K, int Kpad,
                         hipStream_t s);
hipError_t launch_pos_bicubic(const float* pos, float* out, int g, int gh, int gw, int D, hipStream_t s);
// ---- ragged image batches (kernels_norm.hip) ----
// Input buffer: int32 desc[B][4] = {h, w, offset, 0} (the block padded to 256 bytes), then fp32 [3, h, w] planes at
// src + offset (floats, offset % 4 == 0).  ragged_stage validates every entry, copies the planes of the valid images to
// dst + b * slot (slot = 3 * max_pixels floats) and writes meta[b] = {h, w, ntok, bad}; a rejected image (bad = 1) becomes a
// one-token image (its class token only) whose planes are never read.
hipError_t launch_ragged_stage(const float* src, float* dst, size_t slot, int4* meta, int* ntok, int B, int p, size_t max_pixels,
                               int Nmax, hipStream_t s);
// patches[b][t][Kpad] for t < Nmax - 1: image b's patch t (t < gh * gw) or zeros
hipError_t launch_im2col_ragged(const float* stage, size_t slot, const int4* meta, void* out, bool out_f32, int B, int Nmax,
                                int p, int K, int Kpad, hipStream_t s);
// token row (b, t) of the [B, Nmax] block: class token / patch_out[b * (Nmax - 1) + t - 1] + the positional embedding resized
// to image b's grid (the arithmetic of launch_pos_bicubic; the stored table itself on the native grid), ln_pre; rows
// t >= ntok[b] are zeros (part: zero partials)
hipError_t launch_vit_assemble_ragged(const float* patch_out, const float* cls, const float* pos, int g, const int4* meta,
                                      const float* gamma, const float* beta, float eps, void* X, bool x_f16, int B, int Nmax,
                                      int p, int D, float2* part, hipStream_t s);
// zero rows t >= ntok[b] of a [B, Nmax, ld] feature tensor (fp32 or 16-bit elements)
hipError_t launch_zero_pad_rows(void* x, bool is_f32, int ld, const int* ntok, int B, int Nmax, hipStream_t s);
// sentences whose image was rejected: log-prob NaN, counted in info[3] (logprob [Q * nout_per] fp32; image_of nullptr: q)
hipError_t launch_ragged_report(const int4* meta, const int* image_of, int Q, int nout_per, float* logprob, int* info,
                                int* bad, hipStream_t s);
hipError_t launch_vit_assemble_ln(const float* patch_out, const float* cls, const float* pos, const float* gamma,
                                  const float* beta, float eps, void* X, bool x_f16, int B, int N, int D, float2* part,
                                  int nparts, hipStream_t s);   // part: row partials for the folded ln_1 of the first block (or nullptr)
hipError_t launch_layernorm_s16(const void* x, int ldx, const float* gamma, const float* beta, float eps,
                                const float* add_after, void* y_t, int ld_t, bool t_is_f32, void* y_s, int ld_s,
                                int rows, int D, int map_n_in, int map_n_out, int map_off, hipStream_t s);
hipError_t launch_embed_ln(const int* ids, int ld_ids, int pos, const float* words, const float* positions,
                           const float* gamma, const float* beta, float eps, float* h_f, void* h_t, bool t_is_f32,
                           int R, int D, int vocab, bool frag, hipStream_t s);
// context tokens of the decoder memory (GITMI_SEARCH_CONTEXT): tokens int64 [Q][ld] DEVICE, seg [Q] = {image, first context row of
// the segment within its image, length, 0} and cnt [B] context rows per image (DEVICE copies of context_table's output) ->
// rows [n_img, n_img + cnt[b]) of image b's block of `stride` rows in feats [B][stride][D] (fp32 or the operand type; feats_f:
// an optional fp32 copy) = LayerNorm(words[tok] + positions[p]), p from 0 in every segment; rows past them zero;
// ntok[b] = n_img + cnt[b].  Image rows are not touched.  D % 8 == 0, D <= 1024.
hipError_t launch_context_embed(const long long* tokens, int ld, const int4* seg, int Q, const int* cnt, const float* words,
                                const float* positions, const float* gamma, const float* beta, float eps, void* feats, bool t_is_f32,
                                float* feats_f, int* ntok, int B, int n_img, int stride, int D, int vocab, int max_pos, hipStream_t s);
hipError_t launch_frag_pack(const void* src_bf16, void* dst_bf16, int rows, int rows_out, int K, hipStream_t s);
hipError_t launch_convert_pad(const float* src, void* dst, bool dst_f32, size_t rows, int K, int Kpad,
                              hipStream_t s);
hipError_t launch_convert(const void* src, bool src_f32, void* dst, bool dst_f32, size_t n, hipStream_t s);
hipError_t launch_chain_input(const float* x, void* xb_frag, float2* stats, int R, int d, hipStream_t s);
hipError_t launch_copy_f32(const float* src, int lds, float* dst, int ldd, int rows, int cols, hipStream_t s);
hipError_t launch_fill_i32(int* dst, int value, int n, hipStream_t s);

// ---- image memory snapshots (GITMI_SEARCH_KEEP / _RECALL, include/gitmi.h; kernels_memory.hip) ----
// A slot of the caller's store: [256-byte header | feature plane: cap rows of feat_row bytes | one plane per decoder layer: cap
// rows of kv_row bytes, the K | V columns of a prefill row], cap = the engine's per-image row capacity; the first n rows of
// every plane are valid, the rest of a slot is never read.  Plane offsets depend on the configuration alone.
constexpr int MEMORY_MAX_LAYERS = 31;       // layer pointers travel by value
constexpr int MEMORY_HEADER_BYTES = 256, MEMORY_HEADER_WORDS = 16;
constexpr int MEMORY_MAGIC = 0x4d495447;    // "GTIM"
// header words: 0 magic, 1 format version, 2..8 the fingerprint (vit_width, dec_hidden, dec_layers, dec_heads, element size,
// element dtype, row capacity), 9 n, 10 image rows, 11 context rows, 12 frames F, 13 / 14 the image's {h, w}, 15 rejected
enum { MEMW_MAGIC = 0, MEMW_VERSION = 1, MEMW_FP0 = 2, MEMW_FP_END = 9, MEMW_N = 9, MEMW_IMG_ROWS = 10, MEMW_CTX_ROWS = 11,
       MEMW_F = 12, MEMW_H = 13, MEMW_W = 14, MEMW_REJECTED = 15 };
// one table entry per image of a call (DEVICE copy of what the host validated): the kernels take n and the header from here,
// never from the bytes of a slot
struct MemoryEntry {
    int image, slot, n, rsv;                // block of the engine's buffers, slot of the store, valid rows
    int hdr[MEMORY_HEADER_WORDS + 4];       // the slot header (pack: written as is; unpack: h, w for rg_meta); padded to 16 bytes
};
struct MemoryArgs {
    void* feats;                            // [B][stride][feat_row bytes]
    void* kv[MEMORY_MAX_LAYERS];            // per layer [B][stride][kv_ld bytes]; the K | V columns start kv_col bytes into a row
    int layers, stride;                     // stride: rows of an image's block in the engine's buffers
    int feat_row, kv_row, kv_ld, kv_col;    // bytes, multiples of 16
    size_t slot_bytes, feat_plane, kv_plane;        // bytes of a slot and of its planes (cap rows each)
    int* ntok; int4* meta;                  // unpack: ntok[q] = n (and meta[q] = {h, w, n, 0} when not nullptr)
};
// grid (row tiles of 16, 1 + layers, entries): slot <- the n valid rows of image `image`, and its header
hipError_t launch_memory_pack(const MemoryArgs& a, void* store, const MemoryEntry* tab, int entries, int max_n, hipStream_t s);
// block `image` <- the n rows of slot `slot`, zeros in rows [n, stride), the key count
hipError_t launch_memory_unpack(const MemoryArgs& a, const void* store, const MemoryEntry* tab, int entries, hipStream_t s);

// ---- features in (GITMI_SEARCH_FEATURES, include/gitmi.h; kernels_memory.hip feature_install_kernel) ----
// one piece of the call (DEVICE copy of what the host validated): rows [src0, src0 + rows) of the caller's buffer become rows
// [dst0, dst0 + rows) of image `image`'s block; temb: the temporal embedding added to them (fp32 [D]), or nullptr
struct FeaturePiece { int image, dst0, src0, rows; const float* temb; };
struct FeatureArgs {
    void* feats;                            // [B][stride][D], fp32 or the operand type
    const void* src;                        // the caller's dense rows of D elements, fp32 or the operand type
    const FeaturePiece* pieces; int pieces_n;
    const int* count;                       // [B] n_b: the rows of image b; rows [n_b, stride) of its block are written as zeros
    int stride, D;                          // D % 8 == 0
    int* ntok; int4* meta;                  // ntok[b] = n_b (and meta[b] = {0, 0, n_b, 0} when not nullptr)
};
// grid (row tiles of 16 over the stride, B images); src16 needs dst16 (an fp32 engine takes fp32 rows only)
hipError_t launch_feature_install(const FeatureArgs& a, int B, bool src16, bool dst16, hipStream_t s);

struct AttnFullArgs {
    const void* q; const void* k; const void* v; void* out;
    int ldq, ldk, ldv, ldo;
    int N, H;            // N = rows per image (the row stride of an image's block)
    float scale;
    // ragged batches (gitmi_set_image_shape(e, 0, 0)): image b has ntok[b] <= N real rows; keys past it are never read as
    // keys, query rows past it are written as zeros.  nullptr: every image has N rows (the uniform path, unchanged).
    const int* ntok;
};
hipError_t launch_attn_full(const AttnFullArgs& a, int B, bool is_f32, int impl, hipStream_t s);

struct AttnDecodeArgs {
    const void* qkv; const void* img_k; const void* img_v; void* txt_k; void* txt_v; void* out;   // img_k/v head-major [B][H][N_img][64]
    const int* kv_src;
    const int* img_of;   // [B] image whose K/V the sentence attends to (nullptr: sentence b <-> image b)
    int ld_src;
    int d;
    int N_img, T_max, pos, beams;
    int N_pad;           // MFMA kernel (bf16): image keys padded to a multiple of 32; img_k / img_v in the layouts of kv_repack_frag
    int out_frag;        // write `out` in the fragment-major operand layout of the decode chain (bf16)
    float scale;
    int dbg;             // timing experiments.  MFMA register kernel: 1 no image key steps, 2 no up-front text items, 4 no P V
                         // products, 8 zeros instead of the image K/V loads, 16 plain instead of non-temporal K/V loads; the
                         // fp32 kernel: 1 no image K/V loads; the streaming kernel reads none
    int pairs_per_wg;    // MFMA kernel: (sentence, head) pairs per workgroup (1, 2, 4, 8); > 1 packs the launch onto fewer CUs
    int stream_wgs;      // > 0: the streaming kernel (K/V through an LDS ring, 4 independent waves per workgroup) on at most this
                         // many workgroups -- each wave walks its share of the pairs; 0: the register kernels above
    int waves_per_pair;  // MFMA kernel: 0 / 1 = one wave walks all key steps of a pair (default); 2 = two waves split them (A/B)
    int n_pairs;         // set by the launcher
    const int* ntok;     // ragged batches: image keys of every image ([B images] <= N_img; N_img stays the row stride); nullptr:
                         // all N_img.  The streaming kernel does not serve ragged batches (stream_wgs must be 0).
    // launch_attn_decode_qkv only (qkv is not read): the rows' q | k | v = the consumer GEMM dgemm_ln(x, w, bias, colsum, ln) over
    // N = 3 d columns, K = d, M rows, computed inside the attention launch -- DGemmArgs' fields of the same names
    const unsigned short* x; const unsigned short* w; const float* bias; const float* colsum;
    const float2* stats_in; int strips_in; float inv_d, eps_in;
    int M;
};
// the f32 mode's decode attention (VALU, kernels_attn.hip) and its head-major fp32 K/V cache
hipError_t launch_kv_repack(const void* qkv, void* kh, void* vh, int B, int N, int H, int d, hipStream_t s);
hipError_t launch_attn_decode(const AttnDecodeArgs& a, int B, int H, hipStream_t s);
// bf16 decode attention on the matrix cores (kernels_attn_decode.hip) and its cache layouts
hipError_t launch_kv_repack_frag(const void* qkv, void* kf, void* vt, int B, int N, int N_pad, int H, int d, hipStream_t s);
hipError_t launch_attn_decode_mfma(const AttnDecodeArgs& a, int B, int H, hipStream_t s);
int attn_decode_pairs_per_wg(const AttnDecodeArgs& a, int B, int H);   // the packing launch_attn_decode_mfma gives its one-wave register kernel
// The 8-pair register form with the QKV projection inside (one launch instead of QKV GEMM + attention; bit-identical to the two):
// one beam, one wave per pair, N_pad <= 256, no ntok, stream_wgs == 0, K = d <= 768.  attn_decode_qkv_form: is this launch of
// that form?  (the engine adds the policy: only where attn_decode_pairs_per_wg is 8); anything else is hipErrorInvalidValue.
bool attn_decode_qkv_form(const AttnDecodeArgs& a, int B, int H);
inline void attn_decode_set_qkv(AttnDecodeArgs& a, const DGemmArgs& g) {          // g: the QKV launch this one replaces (a dgemm_ln)
    a.x = g.A; a.w = g.W; a.bias = g.bias; a.colsum = g.colsum;
    a.stats_in = g.stats_in; a.strips_in = g.strips_in; a.inv_d = g.inv_d; a.eps_in = g.eps_in; a.M = g.M;
}
hipError_t launch_attn_decode_qkv(const AttnDecodeArgs& a, int B, int H, hipStream_t s);

constexpr int SS_NHMAX = 8;            // num_keep_best supported by the device search
struct SearchState {
    int B, k, pn, T, V, eos, kind;      // B sentences of k beams; T = max_steps = row stride of ids / kv_src / hyp_tok
    int prefixed;                       // 1: every sentence has its own prefix and stands for its own batch-1 reference call
    int sampled;                        // GENERATOR sampling branch: candidates arrive as per_node draws per beam, in draw order
    double length_penalty;
    double* len_norm;                   // [T_max + 1] ((5 + len) / 6) ** length_penalty, filled by search_init
    const long long* start;             // [B][ld_start] start tokens of every sentence (its prefix, or [CLS])
    int ld_start;
    const int* plen;                    // [B] prefix length of every sentence (>= 1)
    int* ids[2];
    int* kv_src[2];
    float* score[2];
    int* done;
    // GENERATOR: BeamHypotheses of every sentence (decoder.py:1292-1341), nh = num_keep_best slots each
    int nh;                             // hypotheses kept per sentence (1 .. SS_NHMAX)
    int* hyp_n;                         // [B] hypotheses held
    int* hyp_cnt;                       // [B] hypotheses ever added (the next insertion number)
    double* hyp_worst;                  // [B] BeamHypotheses.worst_score (1e9 while empty)
    double* hyp_score;                  // [B][nh]
    int* hyp_len;                       // [B][nh]
    int* hyp_seq;                       // [B][nh] insertion number: the reference's list order (ties of its sorted())
    int* hyp_tok;                       // [B][nh][T]
    int* stop;                          // AUTOREGRESSIVE: cur_len at which every beam of the sentence had ended (0: not yet)
    int* early;                         // AUTOREGRESSIVE, k == 1: the sentence's first prediction was EOS
    int* info;                          // [0] sentences ended / done so far, [2] steps run
};
// candidate lists of a step: per row `nparts` sorted lists of `slots` (logit, token) pairs + (max, sum exp) per part
struct StepCands {
    const float* part_val; const int* part_idx; const float2* part_lse;
    int nparts, slots;
};
// embedding of the tokens a step appends = input of the next decode step (decoder.py:65-78); words == nullptr: skip
struct EmbedArgs {
    const float* words; const float* positions; const float* gamma; const float* beta; float eps;
    float* h_f; void* h_t; int D, vocab;
    int frag;            // h_t in the fragment-major operand layout of the decode chain
};
// per-token trace of a search (GITMI_SEARCH_TRACE, include/gitmi.h): the engine-owned log.  The step that writes position s of
// new row r stores one record at [s][r]: the log-prob of the pick and the n best (token, log-prob) of the row it was picked from.
// A position is written once per search, so the record of position s of any later row is log[s][kv_src[row][s]]; a GENERATOR
// hypothesis keeps the kv_src of its history and the record of the candidate that finished it.  log_lp == nullptr: no trace.
constexpr int TRACE_NMAX = 8;
struct TraceArgs {
    int n, rows;                        // alternatives per position (0 .. TRACE_NMAX); row stride of the log (>= B * k)
    float* log_lp; int* log_tok;        // [T][rows][1 + n], [T][rows][n]
    int* hyp_src;                       // [B][nh][T]
    float* fin_lp; int* fin_tok;        // [B][nh][1 + n], [B][nh][n]
};
int row_topm_slots(int M);
// sampling branch (decoder.py:1146-1166, 1343-1375): per row scores / temperature -> top-k / top-p filter (min 2 tokens
// kept) -> `ndraw` draws without replacement (Gumbel-top-k on a counter-based generator) -> their log-probabilities under
// the filtered softmax, in draw order, as one candidate list per row (part_lse = (0, 1): values are log-probs already).
// filtered_out (optional): the filtered logits [R, V] (-inf = removed) for parity checks.
hipError_t launch_sample_rows(const float* logits, int ldl, int V, int R, float temperature, int top_k, float top_p,
                              int ndraw, unsigned long long seed, int step, float* part_val, int* part_idx,
                              float2* part_lse, float* filtered_out, const int* ids, int ld_ids, int cur_len,
                              float rep_penalty, int stride, hipStream_t s,       // stride >= ndraw: entries of a row's list
                              const BanArgs* ban = nullptr, const int* plen = nullptr, int beams = 1);   // ban: rows of plen / beams sentences
// token trie on the device (CSR: the children of node n are edges child_off[n] .. child_off[n + 1]) + one cursor per sentence
struct TrieArgs {
    const int* child_off; const int* child_tok; const int* child_node;
    int* cursor;                 // [B] current node of every sentence (0 = root, -1 = unconstrained)
};
// trie-constrained greedy selection on materialised logits [B, ldl] (trie_decoder.py:57-71, 115-158): one candidate
// (log-prob incl. the trie bonus, token) per sentence in the candidate-list format of the search step; moves the cursors
hipError_t launch_trie_select(const float* logits, int ldl, int V, const int* ids, int ld_ids, int cur_len, const int* plen,
                              int eos, const TrieArgs& tr, int B, float* part_val, int* part_idx, float2* part_lse,
                              hipStream_t s);
hipError_t launch_row_topm(const float* logits, int ldl, int V, const int* ids, int ld_ids, int cur_len,
                           const int* plen, int beams, int suppress_kind, float rep_penalty, int M, int R,
                           float* part_val, int* part_idx, float2* part_lse, hipStream_t s, const BanArgs* ban = nullptr);
// tr (or nullptr: the plain kernel): the traced instantiation, which merges max(M, tr->n) candidates per row and logs the picks
hipError_t launch_search_step(const SearchState& st, int src, int cur_len, const StepCands& in, const EmbedArgs& em,
                              bool t_is_f32, hipStream_t s, const TraceArgs* tr = nullptr);
// beside launch_search_finish, in the order of its tokens_out: out_lp fp32 [B * nout][T][1 + n], out_tok int64 [B * nout][T][n]
// (nullptr when n == 0); every element is written
hipError_t launch_search_trace_gather(const SearchState& st, int cur, int cur_len, const TraceArgs& tr, float* out_lp,
                                      long long* out_tok, hipStream_t s);
hipError_t launch_search_init(const SearchState& st, hipStream_t s);
hipError_t launch_search_finish(const SearchState& st, int cur, int cur_len, long long* tokens_out,
                                float* logprob_out, int* info_out, int* sent_out, hipStream_t s);
hipError_t launch_search_rows(const SearchState& st, int cur, int cur_len, long long* out, hipStream_t s);
hipError_t launch_fill_start(long long* start, int ld, const long long* prefix, int ldp, int shared, int sos, int B, int P,
                             hipStream_t s);
hipError_t launch_load_ids(const long long* tokens, int R, int t, int* ids, int* kv_src, int ld, hipStream_t s);

// caption scoring (kernels_score.hip): rows of the text pass are (sentence q, position j) -> q * Lp + j
// token trees (GITMI_SEARCH_TREE_SCORE): the rows are tree nodes in DFS pre-order, described by four int32 [Q * Lp] tables
struct TreeNodes {
    int* tok;       // token id, clamped into the vocabulary
    int* depth;     // = position of the embedding
    int* parent;    // node index within the tree; -1: root, padding row, or any row of a rejected tree
    int* end;       // first node index past the subtree: k is an ancestor-or-self of i exactly when k <= i < end[k]
};
// tree: embed node rows (token / position from its tables; `tokens` is not read) instead of sentence positions
hipError_t launch_score_embed_ln(const long long* tokens, int ld, int Q, int Lp, const float* words, const float* positions,
                                 const float* gamma, const float* beta, float eps, float* h_f, void* h_t, bool t_is_f32,
                                 int D, int vocab, int max_pos, hipStream_t s, const TreeNodes* tree = nullptr);
// qkv [Q * Lp][3d] text rows, img_kv [B * N_img][3d] prefill rows of the same layer, image_of [Q] -> out [Q * Lp][d]
// ntok (ragged batches): image keys of every image (<= N_img, the row stride of an image's block); nullptr: N_img each
// stats (attention maps; nullptr: none, the score call's kernels): fp32 [Q][H][Lp] = (m, l), the softmax statistics of every row
// node_end (token trees; nullptr: sentences, causal): TreeNodes::end -- text key t is visible to row j when t <= j < node_end[t]
hipError_t launch_score_attn(const void* qkv, const void* img_kv, const int* image_of, void* out, int Q, int H, int d,
                             int N_img, int Lp, float scale, bool is_f32, hipStream_t s, const int* ntok = nullptr,
                             float2* stats = nullptr, const int* node_end = nullptr);
// attention map of one layer from launch_score_attn's operands and stats: out[q * out_sq + j * out_sj + col] = head mean of the
// probability text row (q, j) gives column col -- [0, N_img) the image keys of image_of[q] (0 past ntok), N_img + t (t < Tc) its
// text keys (0 for t > j).  Rows j >= lens[q] (nullptr: Lp rows each) are not written; bad[q] = 1 on a non-finite value (or nullptr).
hipError_t launch_score_attn_map(const void* qkv, const void* img_kv, const int* image_of, const int* ntok, const float2* stats,
                                 const int* lens, float* out, size_t out_sq, size_t out_sj, int Tc, int Q, int H, int N_img,
                                 int Lp, float scale, bool is_f32, int* bad, hipStream_t s);
int score_head_tiles(int V);      // 128-column tiles of the fused head
// part [M][score_head_tiles(V)] = (max, sum exp, sum z), zt [M] = z at tgt[row] (tgt < 0: none); 16-bit A [M][lda], W [V][K]
hipError_t launch_score_head(const void* A, int lda, const void* W, const float* bias, const int* tgt, int M, int V, int K,
                             float4* part, float* zt, hipStream_t s);
hipError_t launch_score_rowstats(const float* logits, int ldl, int V, const int* tgt, int row_off, int rows, float4* part,
                                 float* zt, hipStream_t s);
// The head of a whole text pass, as the score / tree-score calls and gitmi_debug_score_tail run it: A [M][K] text rows, W [V][K],
// tgt [M] -> part [M][*ntiles], zt [M].  f32: GEMM into `logits` [chunk_rows][ldl], launch_score_rowstats (one statistics row
// each, *ntiles = 1) and, with a tree, launch_tree_gather_logits, chunk_rows rows at a time; 16-bit: launch_score_head and, with
// a tree, launch_tree_gather_dot (logits and chunk_rows unused).  tree: zt[node row] = the node's token at its parent's row.
struct ScoreHeadArgs {
    const void* A; const void* W; const float* bias; const int* tgt;
    float4* part; float* zt;
    float* logits; int ldl, chunk_rows;
};
hipError_t launch_score_head_rows(const ScoreHeadArgs& h, bool f32, int M, int V, int K, const TreeNodes* tree, int Lp, int* ntiles,
                                  hipStream_t s);
hipError_t launch_score_targets(const long long* tokens, int ld, int Lp, const int* lens, int V, int M, int* tgt,
                                hipStream_t s);
hipError_t launch_score_combine(const float4* part, int ntiles, const float* zt, const int* tgt, int M, int Lp, int ld, int V,
                                float2* out, int* bad, hipStream_t s);
hipError_t launch_score_info(const int* bad, int Q, int ld, int* info, hipStream_t s, int i1 = 0, int i2 = 0);   // info = {ld, i1, i2, bad}
// token trees: packed int64 [Q][ld] (depth << 32 | token), lens [Q] node counts -> the node tables; bad[q] = 1 for a tree that
// breaks the depth rules (its rows, like the rows past a tree's nodes, become parentless roots).  max_depth <= 8192 (LDS).
hipError_t launch_tree_structure(const long long* packed, int ld, int Q, int Lp, const int* lens, int V, int max_depth,
                                 const TreeNodes& nd, int* bad, hipStream_t s);
// zt[node row] = z[parent row][token of the node]: a dot product of the head's 16-bit operands, or read from materialised fp32
// logits of head rows [row_off, row_off + rows)
hipError_t launch_tree_gather_dot(const void* A, int lda, const void* W, const float* bias, const TreeNodes& nd, int Lp, int M,
                                  int K, float* zt, hipStream_t s);
hipError_t launch_tree_gather_logits(const float* logits, int ldl, int row_off, int rows, const TreeNodes& nd, int Lp, int M,
                                     float* zt, hipStream_t s);
// out[q * ld + i] = (lp, mean_lp) of every node with a parent, from the parent row's tiles (launch_score_head / _rowstats) and zt
hipError_t launch_tree_combine(const float4* part, int ntiles, const float* zt, const TreeNodes& nd, int M, int Lp, int ld, int V,
                               float2* out, int* bad, hipStream_t s);

// GPU image transform (Pillow-exact bicubic resize + centre crop + CLIP normalisation)
hipError_t launch_preprocess(const unsigned char* rgb, int H, int W, int crop, unsigned char* tmp, float* out, hipStream_t s);
hipError_t launch_preprocess_batch(const unsigned char* rgb, const long long* desc, int n, int crop, unsigned char* tmp, float* out,
                                   hipStream_t s);
size_t preprocess_batch_workspace(const long long* desc, int n, int crop);
hipError_t launch_resize_crop_norm(const uint8_t* rgb, int H, int W, int nh, int nw, int top, int left, int ch, int cw,
                                   uint8_t* tmp, float* out, hipStream_t s);

}  // namespace gitmi
