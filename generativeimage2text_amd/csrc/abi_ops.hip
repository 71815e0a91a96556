// Unit entry points of the C ABI (include/gitmi.h: gitmi_op_*, gitmi_preprocess_*): ONE launch each on caller-supplied
// buffers -- what the GPU op tests and tools/ call -- plus the kernel-selection hooks of the measurement build.  No engine
// state: everything that needs a gitmi_engine lives in engine.hip / engine_weights.hip.
#include "../../include/gitmi.h"
#include "abi_common.h"
#include "gitmi_common.h"
#include "launchers.h"

#include <hip/hip_runtime.h>

using namespace gitmi;

#ifdef GITMI_EXPERIMENT
#include "../../include/gitmi_experiment.h"
#define GITMI_EXP_EXPORT extern "C"
#else
#define GITMI_EXPERIMENT_TYPES_ONLY          // the hooks are unused statics here: their argument types, not their declarations
#include "../../include/gitmi_experiment.h"
#define GITMI_EXP_EXPORT [[maybe_unused]] static
#endif

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

extern "C" int gitmi_operand_dtype(void);
static const char* dtype_name(int dtype) {
    return dtype == GITMI_DTYPE_F32 ? "fp32" : dtype == GITMI_DTYPE_BF16 ? "bf16" : dtype == GITMI_DTYPE_F16 ? "fp16" : "unknown";
}
// a dtype argument of a gitmi_op_* hook: fp32, or the 16-bit operand type of THIS build -- the other 16-bit code would make the
// kernels read every element with the wrong encoding
static int check_dtype(const char* op, const char* arg, int dtype) {
    if (dtype == GITMI_DTYPE_F32 || dtype == gitmi_operand_dtype()) return 0;
    return fail("%s: %s is %s (%d), but this library's 16-bit operands are %s (libgitmi%s.so)", op, arg, dtype_name(dtype), dtype,
                dtype_name(gitmi_operand_dtype()), gitmi_operand_dtype() == GITMI_DTYPE_F16 ? "_f16" : "");
}

// ---- single-kernel entry points ------------------------------------------------------------
extern "C" int gitmi_op_gemm(const void* A, const void* W, const float* bias, const float* residual, void* C, int M,
                             int N, int K, int lda, int ldc, int in_dtype, int out_dtype, int act, void* stream) {
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.res = residual; g.C = C;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc; g.ldr = ldc; g.act = act;
    RCK(check_dtype("op_gemm", "in_dtype", in_dtype));
    const bool in_f32 = in_dtype == GITMI_DTYPE_F32;
    if ((in_f32 && K % 16) || (!in_f32 && K % 64)) return fail("op_gemm: K must be a multiple of %d", in_f32 ? 16 : 64);
    if (out_dtype == GITMI_DTYPE_F16_STREAM) {      // fp16 residual-stream rows out, fp16 residual rows in (both builds)
        if (in_f32) return fail("op_gemm: fp16 stream rows need 16-bit operands");
        g.out_f16 = 1;
    } else {
        RCK(check_dtype("op_gemm", "out_dtype", out_dtype));
    }
    HIPCK(launch_gemm(g, in_f32, out_dtype == GITMI_DTYPE_F32, (hipStream_t)stream));
    return 0;
}
// the folded-LayerNorm forms of the large-M GEMM (kernels_gemm10.hip LNF; fp16-operand library, more than 512 rows), one launch
extern "C" int gitmi_op_gemm_ln(const void* A, const void* W, const float* bias, const float* colsum, const float* ln_part,
                                float ln_eps, const void* residual, const float* res_part, const float* res_gamma,
                                const float* res_beta, float res_eps, void* C, float* part_out, int M, int N, int K, int act,
                                void* stream) {
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.C = C;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N; g.act = act;
    if (K % 64) return fail("op_gemm_ln: K must be a multiple of 64");
    if (ln_part) {            // consumer: C = act(LayerNorm(A) W^T + b), A = raw fp16 rows, W / bias / colsum the folded set
        if (!colsum || residual || part_out || res_part) return fail("op_gemm_ln: consumer form takes colsum and no residual / partial output");
        g.ln_part = (const float2*)ln_part; g.ln_nparts = (K + 255) / 256; g.ln_colsum = colsum; g.ln_inv_d = 1.0f / (float)K; g.ln_eps = ln_eps;
    } else {                  // producer: fp16 stream rows + their row partials
        if (!part_out && !res_part) return fail("op_gemm_ln: neither a consumer (ln_part) nor a producer (part_out / res_part)");
        g.out_f16 = 1;
        g.res = (const float*)residual;
        g.part_out = (float2*)part_out;
        if (res_part) {
            g.res_part = (const float2*)res_part; g.res_nparts = (N + 255) / 256; g.res_gamma = res_gamma; g.res_beta = res_beta;
            g.res_inv_d = 1.0f / (float)N; g.res_eps = res_eps;
        }
    }
    if (!gemm_uses_p8(g, false, false))
        return fail("op_gemm_ln: the folded forms exist in gemm_p8_kernel only (more than 512 rows, N %% 256 == 0, K >= 128)");
    if (launch_gemm(g, false, false, (hipStream_t)stream) != hipSuccess)
        return fail("op_gemm_ln: launch refused (the folded forms are built into the fp16-operand library only)");
    return 0;
}
extern "C" int gitmi_op_layernorm(const float* x, const float* gamma, const float* beta, float eps, void* y_t,
                                  float* y_f32, int rows, int D, int out_dtype, void* stream) {
    if (y_t) RCK(check_dtype("op_layernorm", "out_dtype", out_dtype));
    HIPCK(launch_layernorm(x, D, gamma, beta, eps, nullptr, y_t, D, out_dtype == GITMI_DTYPE_F32, y_f32, D, rows, D, 0, 0,
                           0, (hipStream_t)stream));
    return 0;
}
extern "C" int gitmi_op_attention(const void* qkv, void* out, int B, int N, int H, int dtype, int impl, void* stream) {
    RCK(check_dtype("op_attention", "dtype", dtype));
    const size_t esz = dtype == GITMI_DTYPE_F32 ? 4 : 2;
    const int D = H * 64;
    AttnFullArgs a{};
    a.q = qkv;
    a.k = (const char*)qkv + (size_t)D * esz;
    a.v = (const char*)qkv + (size_t)2 * D * esz;
    a.out = out;
    a.ldq = a.ldk = a.ldv = 3 * D;
    a.ldo = D;
    a.N = N; a.H = H; a.scale = 0.125f;
    HIPCK(launch_attn_full(a, B, dtype == GITMI_DTYPE_F32, impl, (hipStream_t)stream));
    return 0;
}

// ---- decode-chain kernels (kernels_dgemm.hip), one launch each -----------------------------------------------
#ifdef GITMI_EXPERIMENT
static int g_dgemm_dbg = 0;
GITMI_EXP_EXPORT int gitmi_debug_set_dgemm(int dbg) { g_dgemm_dbg = dbg; return 0; }      // timing bits of kernels_dgemm.hip
#else
static const int g_dgemm_dbg = 0;
#endif
extern "C" int gitmi_op_dgemm(const void* A, const void* W, const float* bias, const float* colsum, const float* stats,
                              int strips, float eps, void* C, int c_frag, int M, int N, int K, int act, int strips_per_wg,
                              void* stream) {
    if (c_frag && N % 32) return fail("op_dgemm: a fragment-major output needs N %% 32 == 0");
    const DLn ln{(const float2*)stats, strips, 1.0f / (float)K, eps, nullptr, nullptr};
    DGemmArgs g = dgemm_ln(A, W, bias, colsum, stats ? &ln : nullptr, C, c_frag, act, M, N, K);
    g.dbg = g_dgemm_dbg;
    g.strips_per_wg = strips_per_wg;
    if (K % 32) return fail("op_dgemm: K must be a multiple of 32");
    HIPCK(launch_dgemm(g, (hipStream_t)stream));
    return 0;
}
extern "C" int gitmi_op_dgemm_res(const void* A, const void* W, const float* bias, const float* res_x, const float* res_stats,
                                  int res_strips, const float* res_gamma, const float* res_beta, float res_eps,
                                  float* x_out, void* xb_out, float* stats_out, int M, int N, int K, void* stream) {
    const DLn res_ln{(const float2*)res_stats, res_strips, 1.0f / (float)N, res_eps, res_gamma, res_beta};
    DGemmArgs g = dgemm_to_stream(A, W, bias, res_x, res_stats ? &res_ln : nullptr, x_out, xb_out, (float2*)stats_out, M, N, K);
    g.dbg = g_dgemm_dbg;
    if (K % 32 || N % 16) return fail("op_dgemm_res: need K %% 32 == 0 and N %% 16 == 0");
    HIPCK(launch_dgemm(g, (hipStream_t)stream));
    return 0;
}
// every launch form of the decode-chain GEMMs (tests/test_gpu_dgemm_forms.py): an argument check + the launcher the engine's
// dgemm() calls, with the three DGemmArgs fields the engine sets by policy and gitmi_op_dgemm / gitmi_op_dgemm_res leave at 0
// (rows_per_wg, strips_per_wg, no_row_walk) -- so launch_dgemm_t's choice of kernel is part of what runs.  One epilogue per
// call: C (the arguments of gitmi_op_dgemm) or x_out (those of gitmi_op_dgemm_res); the other's pointers are null.  a_rows:
// the rows allocated behind A; every form loads whole 16-row tiles up to the next multiple of 64 rows at most.  dbg stays 0.
GITMI_EXP_EXPORT int gitmi_debug_dgemm_form(const void* A, int a_rows, const void* W, const float* bias, const float* colsum,
                                            const float* stats, int strips, float eps, void* C, int c_frag, int act,
                                            const float* res_x, const float* res_stats, int res_strips, const float* res_gamma,
                                            const float* res_beta, float res_eps, float* x_out, void* xb_out, float* stats_out,
                                            int M, int N, int K, int rows_per_wg, int strips_per_wg, int no_row_walk,
                                            void* stream) {
    if (!A || !W || !bias) return fail("debug_dgemm_form: null argument (A, W, bias)");
    if (M < 0 || N < 0 || K < 0) return fail("debug_dgemm_form: M=%d N=%d K=%d", M, N, K);
    if ((C != nullptr) == (x_out != nullptr)) return fail("debug_dgemm_form: exactly one of C and x_out selects the epilogue");
    if (K % 32) return fail("debug_dgemm_form: K must be a multiple of 32 (K=%d)", K);
    if (a_rows < round_up(M, 64)) return fail("debug_dgemm_form: a_rows=%d, but M=%d rows are loaded as %d", a_rows, M, round_up(M, 64));
    if (rows_per_wg < 0 || strips_per_wg < 0) return fail("debug_dgemm_form: rows_per_wg=%d strips_per_wg=%d", rows_per_wg, strips_per_wg);
    DGemmArgs g;
    if (C) {
        if (res_x || res_stats || xb_out || stats_out) return fail("debug_dgemm_form: residual arguments with the C epilogue");
        if (c_frag && N % 32) return fail("debug_dgemm_form: c_frag needs N %% 32 == 0 (N=%d)", N);
        if (stats) {
            if (!colsum) return fail("debug_dgemm_form: stats without colsum");
            if (strips < 1 || strips > 64) return fail("debug_dgemm_form: strips=%d outside [1, 64]", strips);
        }
        const DLn ln{(const float2*)stats, strips, 1.0f / (float)K, eps, nullptr, nullptr};
        g = dgemm_ln(A, W, bias, colsum, stats ? &ln : nullptr, C, c_frag, act, M, N, K);
    } else {
        if (stats || colsum || c_frag || act) return fail("debug_dgemm_form: consumer arguments with the x_out epilogue");
        if (N % 16) return fail("debug_dgemm_form: the x_out epilogue needs N %% 16 == 0 (N=%d)", N);
        if (!xb_out || !stats_out || !res_x) return fail("debug_dgemm_form: the x_out epilogue needs xb_out, stats_out and res_x");
        if (res_stats) {
            if (!res_gamma || !res_beta) return fail("debug_dgemm_form: res_stats without res_gamma / res_beta");
            if (res_strips < 1 || res_strips > 64) return fail("debug_dgemm_form: res_strips=%d outside [1, 64]", res_strips);
        }
        const DLn res_ln{(const float2*)res_stats, res_strips, 1.0f / (float)N, res_eps, res_gamma, res_beta};
        g = dgemm_to_stream(A, W, bias, res_x, res_stats ? &res_ln : nullptr, x_out, xb_out, (float2*)stats_out, M, N, K);
    }
    g.rows_per_wg = rows_per_wg; g.strips_per_wg = strips_per_wg; g.no_row_walk = no_row_walk;
    HIPCK(launch_dgemm(g, (hipStream_t)stream));
    return 0;
}
// the VocabArgs fields gitmi_op_vocab_topm and gitmi_debug_vocab_topm_rules share (everything but the rule inputs)
static VocabArgs vocab_op_args(const void* A, const void* W, const float* bias, const float* colsum, const float* stats, int strips,
                               float eps, int M, int V, int K, int cols_per_wg, float* part_val, int* part_idx, float* part_lse,
                               float* logits_out, int max_wgs) {
    VocabArgs v{};
    v.max_wgs = max_wgs;
    v.A = (const unsigned short*)A; v.lda = K; v.W = (const unsigned short*)W; v.bias = bias;
    if (stats) { v.colsum = colsum; v.stats_in = (const float2*)stats; v.strips_in = strips; v.inv_d = 1.0f / (float)K; v.eps_in = eps; }
    v.M = M; v.N = V; v.K = K; v.cols_per_wg = cols_per_wg;
    v.part_val = part_val; v.part_idx = part_idx; v.part_lse = (float2*)part_lse;
    v.logits_out = logits_out; v.ld_logits = V;
    return v;
}
extern "C" int gitmi_op_vocab_topm(const void* A, const void* W, const float* bias, const float* colsum, const float* stats,
                                   int strips, float eps, int M, int V, int K, int cols_per_wg, int mtop,
                                   const int* suppress_tok, float* part_val, int* part_idx, float* part_lse,
                                   float* logits_out, int max_wgs, void* stream) {
    VocabArgs v = vocab_op_args(A, W, bias, colsum, stats, strips, eps, M, V, K, cols_per_wg, part_val, part_idx, part_lse, logits_out, max_wgs);
    if (cols_per_wg != 128) return fail("op_vocab_topm: cols_per_wg must be 128");
    // the rule is driven through the search tables in the engine; the unit entry point takes one token per row
    // (ids [M][1], cur_len 1, prefix length 0 => "past the first step")
    static int* zero_plen = nullptr;
    if (suppress_tok) {
        if (!zero_plen) { HIPCK(hipMalloc((void**)&zero_plen, 4096 * sizeof(int))); HIPCK(hipMemset(zero_plen, 0, 4096 * sizeof(int))); }
        if (M > 4096) return fail("op_vocab_topm: at most 4096 rows with suppress_tok");
        v.ids = suppress_tok; v.ld_ids = 1; v.cur_len = 1; v.plen = zero_plen; v.beams = 1; v.suppress_kind = 1;
    }
    HIPCK(launch_vocab_topm(v, mtop, (hipStream_t)stream));
    return 0;
}

// the decoding constraints of a hook call (include/gitmi_experiment.h: gitmi_debug_ban) -> the BanArgs the launchers take, after
// the checks gitmi_generate_constrained makes of a caller's tables -- on host copies, the stream synchronised first; rows / beams
// sentences.  Everything the kernels form an address from (set_of, W, the table lengths) is validated here.
[[maybe_unused]] static int fill_ban_tables(const char* op, const gitmi_debug_ban* ban, int rows, int beams, int V, hipStream_t s, BanArgs* out);
[[maybe_unused]] static int fill_ban(const char* op, const gitmi_debug_ban* ban, const int* ids, const int* plen, int rows, int beams, int V,
                    hipStream_t s, BanArgs* out) {
    if (!ids || !plen) return fail("%s: ban without ids or plen", op);
    return fill_ban_tables(op, ban, rows, beams, V, s, out);
}
// row_words (the rows' own sets, uint32 [rows][W]: the caller's to size) is taken as it is
static int fill_ban_tables(const char* op, const gitmi_debug_ban* ban, int rows, int beams, int V, hipStream_t s, BanArgs* out) {
    if (beams < 1 || rows % beams) return fail("%s: %d rows are not a multiple of beams=%d", op, rows, beams);
    if (ban->W != (V + 31) / 32) return fail("%s: ban W=%d, but (V + 31) / 32 = %d", op, ban->W, (V + 31) / 32);
    if (ban->n_sets < 0) return fail("%s: ban n_sets=%d", op, ban->n_sets);
    if (!ban->set_of || !ban->min_new || !ban->ngram) return fail("%s: ban with a null table", op);
    if (ban->eos < 0 || ban->eos >= V) return fail("%s: ban eos=%d outside [0, V=%d)", op, ban->eos, V);
    const int S = rows / beams;
    HIPCK(hipStreamSynchronize(s));
    std::vector<int> tab((size_t)3 * S);
    HIPCK(hipMemcpy(tab.data(), ban->set_of, (size_t)S * sizeof(int), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(tab.data() + S, ban->min_new, (size_t)S * sizeof(int), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(tab.data() + 2 * S, ban->ngram, (size_t)S * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < S; ++i) {
        const int so = tab[i], mn = tab[S + i], ng = tab[2 * S + i];
        if (so < -1 || so >= ban->n_sets) return fail("%s: ban set_of[%d]=%d outside [-1, n_sets=%d)", op, i, so, ban->n_sets);
        if (so >= 0 && !ban->words && !ban->row_words) return fail("%s: ban words are null, but set_of[%d]=%d", op, i, so);
        if (mn < 0) return fail("%s: ban min_new[%d]=%d is negative", op, i, mn);
        if (ng < 0 || ng > 8) return fail("%s: ban ngram[%d]=%d outside [0, 8]", op, i, ng);
    }
    out->words = ban->words; out->set_of = ban->set_of; out->min_new = ban->min_new; out->ngram = ban->ngram;
    out->W = ban->W; out->eos = ban->eos; out->row_words = ban->row_words;
    return 0;
}

// ban_rows_kernel alone (tests/test_gpu_ban_sequences_ops.py).  An entry point of its own in all but the export: the measurement
// builds' symbol list is pinned by a host test, so it is reached through gitmi_debug_row_topm with ban->row_words_out set, which
// does nothing else then.  When that list is next revised this becomes gitmi_debug_ban_rows and the three fields leave the struct:
// the per-row sets of one step under banned sequences.  ban: the
// static sets as for the other hooks (words / n_sets / W / set_of are read; min_new, ngram and eos are checked like theirs);
// pool_host int32 [n_pool] the HOST pool of GITMI_SEARCH_CONSTRAIN's extension for rows / beams sentences, validated by the
// engine's own check (abi_common.h ban_pool_check; max_lists = the sentence count); ids int32 [rows][ld_ids] DEVICE histories of
// cur_len tokens -> row_words_out uint32 [rows][W] DEVICE.  The pool travels to a device buffer of the hook's own.  Synchronises.
[[maybe_unused]] static int debug_ban_rows(const gitmi_debug_ban* ban, const int32_t* pool_host, int n_pool, const int* ids, int ld_ids,
                                           int cur_len, int rows, int beams, int V, uint32_t* row_words_out, void* stream) {
    if (!ban || !ids || !row_words_out) return fail("debug_ban_rows: null argument");
    if (ban->row_words) return fail("debug_ban_rows: ban->row_words together with row_words_out (the words are this form's output, not an input)");
    if (rows < 1 || beams < 1 || rows % beams) return fail("debug_ban_rows: %d rows are not a positive multiple of beams=%d", rows, beams);
    if (cur_len < 1 || cur_len > ld_ids) return fail("debug_ban_rows: cur_len=%d outside [1, ld_ids=%d]", cur_len, ld_ids);
    hipStream_t s = (hipStream_t)stream;
    BanArgs ba{};
    RCK(fill_ban_tables("debug_ban_rows", ban, rows, beams, V, s, &ba));
    ba.row_words = nullptr;
    if (ba.W > BAN_ROW_MAX_WORDS) return fail("debug_ban_rows: W=%d above the %d words the kernel holds in LDS", ba.W, BAN_ROW_MAX_WORDS);
    const int Q = rows / beams;
    BanPoolView pool;
    RCK(ban_pool_check("debug_ban_rows", pool_host, n_pool, Q, V, Q, BAN_SEQ_MAX_SEQS, BAN_SEQ_MAX_TOKS, BAN_SEQ_MAX_LEN, &pool));
    int* dev = nullptr;
    HIPCK(hipMalloc((void**)&dev, (size_t)n_pool * sizeof(int)));
    hipError_t err = hipMemcpyAsync(dev, pool_host, (size_t)n_pool * sizeof(int), hipMemcpyHostToDevice, s);
    const BanSeqArgs sq{dev + (pool.list_of - pool_host), dev + (pool.list_off - pool_host), dev + (pool.seq_off - pool_host),
                        dev + (pool.tok - pool_host)};
    if (err == hipSuccess) err = launch_ban_rows(ba, sq, ids, ld_ids, cur_len, rows, beams, row_words_out, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    hipFree(dev);
    HIPCK(err);
    return 0;
}

// the fused head with the REAL rule inputs of a search step (tests/test_gpu_search_ops.py): VocabArgs exactly as the engine's
// decode_head_impl fills them -- ids int32 [M][ld_ids] (DEVICE) the rows' histories, cur_len tokens each, plen int32 [M / beams]
// (DEVICE) the sentences' prefix lengths, suppress_kind 1 = the no-immediate-repeat rule on rows with cur_len > plen,
// rep_penalty the GENERATOR repetition penalty over ids[row][0..cur_len) (0 or 1: off).  ids == NULL: no rules.  A penalty over
// more than HIST_SLOTS / 2 tokens is refused HERE, as search_begin_impl refuses it for the engine (the row_topm / sample_rows
// launchers hold the history as a set of that capacity; launch_vocab_topm walks the ids and has no such check of its own).
// ban: the decoding constraints of the rows (VocabArgs::ban); the head walks the ids for the n-gram rule too, so a constrained
// call has no cap on cur_len.
GITMI_EXP_EXPORT int gitmi_debug_vocab_topm_rules(const void* A, const void* W, const float* bias, const float* colsum,
                                                  const float* stats, int strips, float eps, int M, int V, int K, int cols_per_wg,
                                                  int mtop, const int* ids, int ld_ids, int cur_len, const int* plen, int beams,
                                                  int suppress_kind, float rep_penalty, float* part_val, int* part_idx,
                                                  float* part_lse, float* logits_out, int max_wgs, void* stream,
                                                  const gitmi_debug_ban* ban) {
    if (!A || !W || !bias || !part_val || !part_idx || !part_lse) return fail("debug_vocab_topm_rules: null argument");
    if (cols_per_wg != 128) return fail("debug_vocab_topm_rules: cols_per_wg must be 128");
    VocabArgs v = vocab_op_args(A, W, bias, colsum, stats, strips, eps, M, V, K, cols_per_wg, part_val, part_idx, part_lse, logits_out, max_wgs);
    if (ids) {
        if (!plen) return fail("debug_vocab_topm_rules: ids without plen");
        if (beams < 1 || M % beams) return fail("debug_vocab_topm_rules: M=%d is not a multiple of beams=%d", M, beams);
        if (cur_len < 1 || cur_len > ld_ids) return fail("debug_vocab_topm_rules: cur_len=%d outside [1, ld_ids=%d]", cur_len, ld_ids);
        if (rep_penalty != 0.f && rep_penalty != 1.f && cur_len > HIST_SLOTS / 2)
            return fail("debug_vocab_topm_rules: the repetition penalty supports histories up to %d tokens (cur_len=%d)", HIST_SLOTS / 2, cur_len);
        v.ids = ids; v.ld_ids = ld_ids; v.cur_len = cur_len; v.plen = plen; v.beams = beams; v.suppress_kind = suppress_kind;
        v.rep_penalty = rep_penalty;
    }
    if (ban) RCK(fill_ban("debug_vocab_topm_rules", ban, ids, plen, M, beams, V, (hipStream_t)stream, &v.ban));
    HIPCK(launch_vocab_topm(v, mtop, (hipStream_t)stream));
    return 0;
}

// one step of the sampling branch on caller-supplied logits [R, V] (decoder.py:1146-1166): filtered logits (optional),
// ndraw draws per row in draw order and their log-probabilities under the filtered softmax
extern "C" int gitmi_op_sample_rows(const float* logits, int R, int V, float temperature, int top_k, float top_p, int ndraw,
                                    uint64_t seed, int step, float* draw_logprob, int* draw_token, float* filtered_out,
                                    void* stream) {
    float2* lse = nullptr;
    HIPCK(hipMalloc((void**)&lse, (size_t)R * sizeof(float2)));
    hipError_t err = launch_sample_rows(logits, V, V, R, temperature, top_k, top_p, ndraw, seed, step, draw_logprob, draw_token,
                                        lse, filtered_out, nullptr, 0, 0, 0.f, ndraw, (hipStream_t)stream);
    if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
    hipFree(lse);
    HIPCK(err);
    return 0;
}

// ---- op hooks of the whole-row selection kernels (kernels_search.hip; tests/test_gpu_select_ops.py): an argument check + the
// launcher the engine calls, so the launcher's own refusals and its choice of instantiation are part of what runs.
// the rule inputs the three hooks share: ids int32 [R][ld_ids] DEVICE histories of cur_len tokens (NULL: none)
[[maybe_unused]] static int check_history(const char* op, const int* ids, int ld_ids, int cur_len) {
    if (ids && (cur_len < 1 || cur_len > ld_ids)) return fail("%s: cur_len=%d outside [1, ld_ids=%d]", op, cur_len, ld_ids);
    return 0;
}
// row_topm_kernel: logits fp32 [R][ldl] -> part_val / part_idx [R][row_topm_slots(M)], part_lse [R] (max, sum exp)
GITMI_EXP_EXPORT int gitmi_debug_row_topm(const float* logits, int ldl, int V, int R, const int* ids, int ld_ids, int cur_len,
                                          const int* plen, int beams, int suppress_kind, float rep_penalty, int M, float* part_val,
                                          int* part_idx, float* part_lse, void* stream, const gitmi_debug_ban* ban) {
    if (ban && ban->row_words_out)
        return debug_ban_rows(ban, ban->pool_host, ban->n_pool, ids, ld_ids, cur_len, R, beams, V, ban->row_words_out, stream);
    if (!logits || !part_val || !part_idx || !part_lse) return fail("debug_row_topm: null argument");
    if (R < 1 || V < 1 || ldl < V) return fail("debug_row_topm: R=%d V=%d ldl=%d", R, V, ldl);
    if (ids) {
        if (!plen) return fail("debug_row_topm: ids without plen");
        if (beams < 1 || R % beams) return fail("debug_row_topm: R=%d is not a multiple of beams=%d", R, beams);
        RCK(check_history("debug_row_topm", ids, ld_ids, cur_len));
    } else {
        suppress_kind = 0;                                  // no histories: no rules (the kernel reads plen for the no-repeat rule)
    }
    BanArgs ba{};
    if (ban) RCK(fill_ban("debug_row_topm", ban, ids, plen, R, beams, V, (hipStream_t)stream, &ba));
    HIPCK(launch_row_topm(logits, ldl, V, ids, ld_ids, cur_len, plen, ids ? beams : 1, suppress_kind, rep_penalty, M, R, part_val,
                          part_idx, (float2*)part_lse, (hipStream_t)stream, ban ? &ba : nullptr));
    return 0;
}
// trie_select_kernel on a caller's CSR trie (all arrays DEVICE): child_off int32 [n_nodes + 1], child_tok / child_node int32
// [child_off[n_nodes]], cursor int32 [B] read and updated.  The arrays are checked as gitmi_set_trie checks them, and the
// cursors against n_nodes (host copies; synchronises the stream first).
GITMI_EXP_EXPORT int gitmi_debug_trie_select(const float* logits, int ldl, int V, int B, const int* ids, int ld_ids, int cur_len,
                                             const int* plen, int eos, const int* child_off, const int* child_tok,
                                             const int* child_node, int n_nodes, int* cursor, float* part_val, int* part_idx,
                                             float* part_lse, void* stream) {
    if (!logits || !ids || !plen || !part_val || !part_idx || !part_lse) return fail("debug_trie_select: null argument");
    if (!child_off || !child_tok || !child_node || !cursor) return fail("debug_trie_select: null trie arrays");
    if (V < 2) return fail("debug_trie_select: V=%d (at least 2 tokens)", V);
    if (B < 1 || ldl < V || n_nodes < 1) return fail("debug_trie_select: B=%d V=%d ldl=%d n_nodes=%d", B, V, ldl, n_nodes);
    RCK(check_history("debug_trie_select", ids, ld_ids, cur_len));
    hipStream_t s = (hipStream_t)stream;
    HIPCK(hipStreamSynchronize(s));
    std::vector<int> off((size_t)n_nodes + 1), cur((size_t)B);
    HIPCK(hipMemcpy(off.data(), child_off, off.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (off[0] != 0) return fail("debug_trie_select: child_off must start at 0");
    for (int n = 0; n < n_nodes; ++n)
        if (off[n + 1] < off[n]) return fail("debug_trie_select: child_off must be non-decreasing");
    const int n_edges = off[n_nodes];
    if (n_edges > 0) {
        std::vector<int> node((size_t)n_edges);
        HIPCK(hipMemcpy(node.data(), child_node, node.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < n_edges; ++i)
            if (node[i] < 0 || node[i] >= n_nodes) return fail("debug_trie_select: edge %d leads to node %d of %d", i, node[i], n_nodes);
    }
    HIPCK(hipMemcpy(cur.data(), cursor, cur.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
        if (cur[b] < -1 || cur[b] >= n_nodes) return fail("debug_trie_select: cursor %d of sentence %d outside [-1, %d)", cur[b], b, n_nodes);
    const TrieArgs tr{child_off, child_tok, child_node, cursor};
    HIPCK(launch_trie_select(logits, ldl, V, ids, ld_ids, cur_len, plen, eos, tr, B, part_val, part_idx, (float2*)part_lse, s));
    return 0;
}
// sample_rows_kernel with everything the engine's sampling step sets: gitmi_op_sample_rows' arguments + the row stride of the
// logits, the histories of the repetition penalty and the list stride (entries ndraw..stride are padding).  filtered_out [R][V].
// ban: the decoding constraints of the rows, with plen int32 [R / beams] (DEVICE) and beams -- read under a ban only.
GITMI_EXP_EXPORT int gitmi_debug_sample_rows(const float* logits, int R, int V, float temperature, int top_k, float top_p, int ndraw,
                                             uint64_t seed, int step, float* draw_logprob, int* draw_token, float* filtered_out,
                                             int ldl, const int* ids, int ld_ids, int cur_len, float rep_penalty, int stride,
                                             void* stream, const int* plen, int beams, const gitmi_debug_ban* ban) {
    if (!logits || !draw_logprob || !draw_token) return fail("debug_sample_rows: null argument");
    if (R < 1 || V < 1 || ldl < V) return fail("debug_sample_rows: R=%d V=%d ldl=%d", R, V, ldl);
    RCK(check_history("debug_sample_rows", ids, ld_ids, cur_len));
    BanArgs ba{};
    if (ban) RCK(fill_ban("debug_sample_rows", ban, ids, plen, R, beams, V, (hipStream_t)stream, &ba));
    float2* lse = nullptr;
    HIPCK(hipMalloc((void**)&lse, (size_t)R * sizeof(float2)));
    hipError_t err = launch_sample_rows(logits, ldl, V, R, temperature, top_k, top_p, ndraw, seed, step, draw_logprob, draw_token, lse,
                                        filtered_out, ids, ld_ids, cur_len, rep_penalty, stride, (hipStream_t)stream,
                                        ban ? &ba : nullptr, ban ? plen : nullptr, ban ? beams : 1);
    if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
    hipFree(lse);
    HIPCK(err);
    return 0;
}

GITMI_EXP_EXPORT int gitmi_debug_set_gemm_impl(int impl) {
    if (!set_gemm_impl(impl)) return fail("debug_set_gemm_impl: unknown selector %d (low byte: -1, 0 or 9)", impl);
    return 0;
}

// every launch form of the large-M / tile GEMM (tests/test_gpu_gemm_forms.py): an argument check + launch_gemm with everything
// the engine's gemm_args / gemm_run / ln_gemm / gemm_to_stream set -- leading dimensions of their own (a column slice of a wider
// buffer: ldc > N with C, W, bias and colsum offset by the caller), the serving policy's `shared`, and the folded-LayerNorm
// fields of the consumer (ln_part, colsum, ln_eps; K <= 1024) and of the producer (part_out; res_part / res_gamma / res_beta /
// res_eps: the post-norm residual; N <= 1024).  out_dtype: fp32, the operand type, or GITMI_DTYPE_F16_STREAM (fp16 rows, and
// `res` fp16 rows; the producer's only kind).  Row partials are [M][4] (sum, sumsq).  Tile heights and XCD partitions are forced
// through gitmi_debug_set_gemm_impl, so the launcher's own choice is what runs without it.
GITMI_EXP_EXPORT int gitmi_debug_gemm_form(const void* A, int lda, const void* W, const float* bias, const void* res, int ldr, void* C,
                                           int ldc, int M, int N, int K, int act, int in_dtype, int out_dtype, int shared,
                                           const float* ln_part, const float* colsum, float ln_eps, float* part_out,
                                           const float* res_part, const float* res_gamma, const float* res_beta, float res_eps,
                                           void* stream) {
    if (!A || !W || !C) return fail("debug_gemm_form: null argument (A, W, C)");
    if (M < 0 || N < 1 || K < 1) return fail("debug_gemm_form: M=%d N=%d K=%d", M, N, K);
    if (lda < K) return fail("debug_gemm_form: lda=%d < K=%d", lda, K);
    if (ldc < N) return fail("debug_gemm_form: ldc=%d < N=%d", ldc, N);
    if (res && ldr < N) return fail("debug_gemm_form: ldr=%d < N=%d", ldr, N);
    if (act < GITMI_ACT_NONE || act > GITMI_ACT_GELU_ERF) return fail("debug_gemm_form: act=%d", act);
    RCK(check_dtype("debug_gemm_form", "in_dtype", in_dtype));
    const bool in_f32 = in_dtype == GITMI_DTYPE_F32;
    if ((in_f32 && K % 16) || (!in_f32 && K % 64)) return fail("debug_gemm_form: K must be a multiple of %d (K=%d)", in_f32 ? 16 : 64, K);
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.res = (const float*)res; g.C = C;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc; g.ldr = res ? ldr : 0; g.act = act;
    g.shared = shared ? 1 : 0;
    if (out_dtype == GITMI_DTYPE_F16_STREAM) {
        if (in_f32) return fail("debug_gemm_form: fp16 stream rows need 16-bit operands");
        g.out_f16 = 1;
    } else {
        RCK(check_dtype("debug_gemm_form", "out_dtype", out_dtype));
    }
    const bool out_f32 = out_dtype == GITMI_DTYPE_F32;
    const bool consumer = ln_part != nullptr, producer = part_out != nullptr || res_part != nullptr;
    if (colsum && !consumer) return fail("debug_gemm_form: colsum without ln_part");
    if ((res_gamma || res_beta) && !res_part) return fail("debug_gemm_form: res_gamma / res_beta without res_part");
    if (consumer || producer) {
#ifndef GITMI_OPS_F16
        return fail("debug_gemm_form: the folded-LayerNorm forms are built into the fp16-operand library only");
#endif
        if (consumer && producer) return fail("debug_gemm_form: consumer (ln_part) and producer (part_out / res_part) arguments in one launch");
        if (consumer) {
            if (!colsum) return fail("debug_gemm_form: ln_part without colsum");
            if (res || in_f32 || out_f32 || g.out_f16) return fail("debug_gemm_form: the consumer writes operand-type rows and takes no residual");
            if (K > 1024) return fail("debug_gemm_form: row partials cover K <= 1024 (K=%d)", K);
            g.ln_part = (const float2*)ln_part; g.ln_nparts = (K + 255) / 256; g.ln_colsum = colsum; g.ln_inv_d = 1.0f / (float)K; g.ln_eps = ln_eps;
        } else {
            if (!g.out_f16 || act != GITMI_ACT_NONE) return fail("debug_gemm_form: the producer writes fp16 stream rows and has no activation");
            if (N > 1024) return fail("debug_gemm_form: row partials cover N <= 1024 (N=%d)", N);
            g.part_out = (float2*)part_out;
            if (res_part) {
                if (!res || !res_gamma || !res_beta) return fail("debug_gemm_form: res_part without res / res_gamma / res_beta");
                g.res_part = (const float2*)res_part; g.res_nparts = (N + 255) / 256; g.res_gamma = res_gamma; g.res_beta = res_beta;
                g.res_inv_d = 1.0f / (float)N; g.res_eps = res_eps;
            }
        }
        if (!gemm_uses_p8(g, false, false))
            return fail("debug_gemm_form: the folded forms exist in gemm_p8_kernel only (more than 512 rows, N %% 256 == 0, K >= 128, 16-byte aligned rows)");
    }
    HIPCK(launch_gemm(g, in_f32, out_f32, (hipStream_t)stream));
    return 0;
}

extern "C" int gitmi_op_attn_decode(const void* qkv, const void* img_k, const void* img_v, void* txt_k, void* txt_v,
                                    const int* kv_src, void* out, int B, int H, int N_img, int T_max, int pos, int beams,
                                    int dtype, int dbg, void* stream) {
    RCK(check_dtype("op_attn_decode", "dtype", dtype));
    AttnDecodeArgs a{};
    a.qkv = qkv; a.img_k = img_k; a.img_v = img_v; a.txt_k = txt_k; a.txt_v = txt_v; a.out = out;
    a.kv_src = kv_src; a.ld_src = T_max; a.d = H * 64; a.N_img = N_img; a.T_max = T_max; a.pos = pos; a.beams = beams;
    // dbg: bits 0..15 timing experiments of the kernels (measurement builds), bits 16..17 waves per pair (0 = by geometry,
    // 1, 2), bits 18.. workgroups of the streaming kernel (0 = register kernels)
    a.scale = 0.125f; a.dbg = dbg & 0xffff; a.waves_per_pair = (dbg >> 16) & 3; a.stream_wgs = dbg >> 18;
    if (dtype == GITMI_DTYPE_F32) {
        HIPCK(launch_attn_decode(a, B, H, (hipStream_t)stream));
        return 0;
    }
    // 16-bit: img_k / img_v are the MFMA operand layouts written by gitmi_op_kv_repack (keys padded to 32)
    a.N_pad = round_up(N_img, 32);
    HIPCK(launch_attn_decode_mfma(a, B, H, (hipStream_t)stream));
    return 0;
}
// image-row K/V of the prefill ([B*N, 3*H*64] packed q|k|v, 16-bit operands) -> the decode layouts of kernels_attn_decode.hip:
// kf, vt: [B][H][round_up(N, 32)][64] each
extern "C" int gitmi_op_kv_repack(const void* qkv_rows, void* kf, void* vt, int B, int N, int H, void* stream) {
    HIPCK(launch_kv_repack_frag(qkv_rows, kf, vt, B, N, round_up(N, 32), H, H * 64, (hipStream_t)stream));
    return 0;
}

// ---- ragged batches (measurement build; tests/test_gpu_ragged_ops.py): the attention kernels with per-image key counts.
// ntok: int32 [B] DEVICE, image b's rows (<= N; N stays the row stride of an image's block).  Same layouts as gitmi_op_attention /
// gitmi_op_attn_decode; impl of the full attention: 0 VALU (f32), 1 by geometry (short single-pass / flash), 2 flash forced.
GITMI_EXP_EXPORT int gitmi_debug_attention_ragged(const void* qkv, void* out, const int* ntok, int B, int N, int H, int dtype, int impl,
                                                  void* stream) {
    if (!ntok) return fail("debug_attention_ragged: ntok is required");
    const size_t esz = dtype == GITMI_DTYPE_F32 ? 4 : 2;
    const int D = H * 64;
    AttnFullArgs a{};
    a.q = qkv;
    a.k = (const char*)qkv + (size_t)D * esz;
    a.v = (const char*)qkv + (size_t)2 * D * esz;
    a.out = out;
    a.ldq = a.ldk = a.ldv = 3 * D;
    a.ldo = D;
    a.N = N; a.H = H; a.scale = 0.125f; a.ntok = ntok;
    HIPCK(launch_attn_full(a, B, dtype == GITMI_DTYPE_F32, impl, (hipStream_t)stream));
    return 0;
}
// every launch form of the decode attention (tests/test_gpu_attn_decode_forms.py): an argument check + the launcher the engine's
// decode step calls, with the AttnDecodeArgs fields that gitmi_op_attn_decode leaves at their defaults -- so the launcher's choice
// of kernel (packing, beam rows, one / two waves, streaming) is part of what runs.  dbg stays 0.
GITMI_EXP_EXPORT int gitmi_debug_attn_decode_form(const void* qkv, const void* img_k, const void* img_v, void* txt_k, void* txt_v,
                                                  const int* kv_src, void* out, const int* ntok, const int* img_of, int n_images,
                                                  int B, int H, int N_img, int T_max, int pos, int beams, int dtype, int out_frag,
                                                  int pairs_per_wg, int waves_per_pair, int stream_wgs, void* stream) {
    RCK(check_dtype("debug_attn_decode_form", "dtype", dtype));
    if (!qkv || !img_k || !img_v || !txt_k || !txt_v || !kv_src || !out) return fail("debug_attn_decode_form: null argument");
    if (beams < 1 || beams > 8) return fail("debug_attn_decode_form: beams=%d outside [1, 8]", beams);
    if (n_images < 1) return fail("debug_attn_decode_form: n_images=%d", n_images);
    if (B < 1 || H < 1 || N_img < 1 || pos < 0 || pos >= T_max)
        return fail("debug_attn_decode_form: B=%d H=%d N_img=%d pos=%d T_max=%d", B, H, N_img, pos, T_max);
    if (out_frag && dtype == GITMI_DTYPE_F32) return fail("debug_attn_decode_form: out_frag needs 16-bit rows");
    if (ntok && stream_wgs > 0) return fail("debug_attn_decode_form: the streaming kernel does not serve ragged batches (ntok)");
    AttnDecodeArgs a{};
    a.qkv = qkv; a.img_k = img_k; a.img_v = img_v; a.txt_k = txt_k; a.txt_v = txt_v; a.out = out;
    a.kv_src = kv_src; a.ld_src = T_max; a.d = H * 64; a.N_img = N_img; a.T_max = T_max; a.pos = pos; a.beams = beams;
    a.scale = 0.125f; a.ntok = ntok; a.img_of = img_of; a.out_frag = out_frag;
    a.pairs_per_wg = pairs_per_wg; a.waves_per_pair = waves_per_pair; a.stream_wgs = stream_wgs;
    if (dtype == GITMI_DTYPE_F32) {
        HIPCK(launch_attn_decode(a, B, H, (hipStream_t)stream));
        return 0;
    }
    a.N_pad = round_up(N_img, 32);
    HIPCK(launch_attn_decode_mfma(a, B, H, (hipStream_t)stream));
    return 0;
}
// the attention launch that computes its own q | k | v (tests/test_gpu_attn_decode_qkv.py): an argument check + the launcher the
// engine's decode step calls where its policy packs 8 one-wave pairs per workgroup.  The attention operands of
// gitmi_debug_attn_decode_form without qkv, and the QKV GEMM's operands as gitmi_debug_dgemm_form takes them (x fragment-major
// [x_rows][K = H * 64], w fragment-major [3 K][K], bias / colsum [3 K], stats [strips][B] strip partials or NULL).  The launch
// is of this one form whatever B is; a call outside it is refused by name, nothing launched.
GITMI_EXP_EXPORT int gitmi_debug_attn_decode_qkv(const void* x, int x_rows, const void* w, const float* bias, const float* colsum,
                                                 const float* stats, int strips, float eps, const void* img_k, const void* img_v,
                                                 void* txt_k, void* txt_v, const int* kv_src, void* out, const int* ntok,
                                                 const int* img_of, int n_images, int B, int H, int N_img, int T_max, int pos,
                                                 int beams, int dtype, int out_frag, int pairs_per_wg, int waves_per_pair,
                                                 int stream_wgs, void* stream) {
    RCK(check_dtype("debug_attn_decode_qkv", "dtype", dtype));
    if (dtype == GITMI_DTYPE_F32) return fail("debug_attn_decode_qkv: 16-bit operands only (the f32 mode keeps its QKV launch)");
    if (!x || !w || !bias || !img_k || !img_v || !txt_k || !txt_v || !kv_src || !out) return fail("debug_attn_decode_qkv: null argument");
    if (n_images < 1) return fail("debug_attn_decode_qkv: n_images=%d", n_images);
    if (B < 1 || H < 1 || N_img < 1 || pos < 0 || pos >= T_max)
        return fail("debug_attn_decode_qkv: B=%d H=%d N_img=%d pos=%d T_max=%d", B, H, N_img, pos, T_max);
    if (beams != 1) return fail("debug_attn_decode_qkv: beams=%d (beam batches keep the QKV launch)", beams);
    if (ntok) return fail("debug_attn_decode_qkv: ntok (ragged batches keep the QKV launch)");
    if (waves_per_pair == 2) return fail("debug_attn_decode_qkv: waves_per_pair=2 (two-wave pairs keep the QKV launch)");
    if (stream_wgs != 0) return fail("debug_attn_decode_qkv: stream_wgs=%d (the streaming form keeps the QKV launch)", stream_wgs);
    if (pairs_per_wg != 8) return fail("debug_attn_decode_qkv: pairs_per_wg=%d (the form packs 8 pairs)", pairs_per_wg);
    if (round_up(N_img, 32) > 256) return fail("debug_attn_decode_qkv: N_img=%d (more than 256 padded keys: the two-wave form)", N_img);
    if (H * 64 > 768) return fail("debug_attn_decode_qkv: hidden=%d > 768", H * 64);
    if (x_rows < round_up(B, 16)) return fail("debug_attn_decode_qkv: x_rows=%d, but B=%d rows are loaded as %d", x_rows, B, round_up(B, 16));
    if (stats) {
        if (!colsum) return fail("debug_attn_decode_qkv: stats without colsum");
        if (strips < 1 || strips > 64) return fail("debug_attn_decode_qkv: strips=%d outside [1, 64]", strips);
    }
    AttnDecodeArgs a{};
    a.img_k = img_k; a.img_v = img_v; a.txt_k = txt_k; a.txt_v = txt_v; a.out = out;
    a.kv_src = kv_src; a.ld_src = T_max; a.d = H * 64; a.N_img = N_img; a.T_max = T_max; a.pos = pos; a.beams = beams;
    a.scale = 0.125f; a.img_of = img_of; a.out_frag = out_frag; a.pairs_per_wg = pairs_per_wg; a.waves_per_pair = waves_per_pair;
    a.N_pad = round_up(N_img, 32);
    const DLn ln{(const float2*)stats, strips, 1.0f / (float)a.d, eps, nullptr, nullptr};
    const DGemmArgs g = dgemm_ln(x, w, bias, colsum, stats ? &ln : nullptr, nullptr, 0, 0, B, 3 * a.d, a.d);
    attn_decode_set_qkv(a, g);
    if (!attn_decode_qkv_form(a, B, H)) return fail("debug_attn_decode_qkv: not a launch of the form");
    HIPCK(launch_attn_decode_qkv(a, B, H, (hipStream_t)stream));
    return 0;
}
GITMI_EXP_EXPORT int gitmi_debug_attn_decode_ragged(const void* qkv, const void* img_k, const void* img_v, void* txt_k, void* txt_v,
                                                    const int* kv_src, void* out, const int* ntok, int B, int H, int N_img, int T_max,
                                                    int pos, int beams, int dtype, void* stream) {
    if (!ntok) return fail("debug_attn_decode_ragged: ntok is required");
    return gitmi_debug_attn_decode_form(qkv, img_k, img_v, txt_k, txt_v, kv_src, out, ntok, nullptr, B, B, H, N_img, T_max, pos, beams,
                                        dtype, 0, 0, 0, 0, stream);
}

// ---- GPU image transform -------------------------------------------------------
extern "C" int gitmi_preprocess_image(const uint8_t* rgb_hwc, int H, int W, int crop, uint8_t* tmp, size_t tmp_bytes,
                                      float* out_chw, void* stream) {
    if (!rgb_hwc || !out_chw || H < 1 || W < 1 || crop < 1) return fail("preprocess: bad argument");
    const int nw = W <= H ? crop : (int)((double)crop * W / H);
    if (nw != W && (!tmp || tmp_bytes < (size_t)H * nw * 3)) return fail("preprocess: workspace must hold H * %d * 3 bytes", nw);
    HIPCK(launch_preprocess(rgb_hwc, H, W, crop, tmp, out_chw, (hipStream_t)stream));
    return 0;
}

// a batch of decoded images in one staging buffer (include/gitmi.h)
extern "C" int gitmi_preprocess_batch(const uint8_t* rgb, size_t rgb_bytes, const int64_t* desc_host, int n, int crop, uint8_t* tmp,
                                      size_t tmp_bytes, float* out, void* stream) {
    if (!rgb || !desc_host || !out || n < 1 || crop < 1 || crop > 4096) return fail("preprocess_batch: bad argument");
    for (int i = 0; i < n; ++i) {
        const int64_t off = desc_host[3 * i], H = desc_host[3 * i + 1], W = desc_host[3 * i + 2];
        if (H < 1 || W < 1 || H > 65535 || W > 65535 || off < 0 || (uint64_t)off + (uint64_t)H * W * 3 > rgb_bytes ||
            (uint64_t)off + (uint64_t)H * W * 3 > 0xffffffffull)
            return fail("preprocess_batch: image %d (offset %lld, %lld x %lld) does not fit the staging buffer of %zu bytes", i,
                        (long long)off, (long long)H, (long long)W, rgb_bytes);
        const double r = W <= H ? (double)H / W : (double)W / H;
        if (r * crop > 65535.0) return fail("preprocess_batch: image %d: aspect ratio too extreme", i);
    }
    const size_t need = preprocess_batch_workspace((const long long*)desc_host, n, crop);
    if (need > 0 && (!tmp || tmp_bytes < need)) return fail("preprocess_batch: workspace must hold %zu bytes", need);
    if (need > 0xffffffffull) return fail("preprocess_batch: batch too large for one call");
    HIPCK(launch_preprocess_batch(rgb, (const long long*)desc_host, n, crop, tmp, out, (hipStream_t)stream));
    return 0;
}

// MinMaxResizeForTest (inference.py:29-64) output: a plain resize to out_h x out_w (no crop) + ToTensor + Normalize.
// The caller computes (out_h, out_w) with the reference's get_size() rule (generativeimage2text_amd/inference.py).
extern "C" int gitmi_preprocess_image_to(const uint8_t* rgb_hwc, int H, int W, int out_h, int out_w, uint8_t* tmp,
                                         size_t tmp_bytes, float* out_chw, void* stream) {
    if (!rgb_hwc || !out_chw || H < 1 || W < 1 || out_h < 1 || out_w < 1) return fail("preprocess: bad argument");
    if (out_w != W && (!tmp || tmp_bytes < (size_t)H * out_w * 3))
        return fail("preprocess: workspace must hold H * %d * 3 bytes", out_w);
    HIPCK(launch_resize_crop_norm(rgb_hwc, H, W, out_h, out_w, 0, 0, out_h, out_w, tmp, out_chw, (hipStream_t)stream));
    return 0;
}

// ---- op hooks of the caption-scoring kernels (kernels_score.hip; tests/test_gpu_score_ops.py) -----------------------
// attention: qkv [Q * Lp][3 H 64] text rows, img_kv [B * N_img][3 H 64] prefill rows, image_of int32 [Q] -> out [Q * Lp][H 64]
// (dtype GITMI_DTYPE_F32: the fp32 kernel of the parity mode; the build's 16-bit operand dtype: the MFMA kernel)
GITMI_EXP_EXPORT int gitmi_debug_score_attn(const void* qkv, const void* img_kv, const int* image_of, void* out, int Q, int H,
                                            int N_img, int Lp, int dtype, void* stream) {
    if (!qkv || !img_kv || !image_of || !out) return fail("debug_score_attn: null argument");
    if (dtype != GITMI_DTYPE_F32 && dtype != gitmi_operand_dtype()) return fail("debug_score_attn: dtype %d not served by this build", dtype);
    HIPCK(launch_score_attn(qkv, img_kv, image_of, out, Q, H, H * 64, N_img, Lp, 0.125f, dtype == GITMI_DTYPE_F32,
                            (hipStream_t)stream));
    return 0;
}
// attention map of one layer: the attention launch with its statistics, then the map kernel -> out fp32 [Q][Lp][N_img + Lp]
// (ntok: int32 [B] on the device, the image keys of every image, or NULL).  Synchronises the stream.
GITMI_EXP_EXPORT int gitmi_debug_score_attn_map(const void* qkv, const void* img_kv, const int* image_of, const int* ntok, float* out,
                                                int Q, int H, int N_img, int Lp, int dtype, void* stream) {
    if (!qkv || !img_kv || !image_of || !out || Q < 1 || H < 1 || N_img < 1 || Lp < 1) return fail("debug_score_attn_map: bad argument");
    if (dtype != GITMI_DTYPE_F32 && dtype != gitmi_operand_dtype()) return fail("debug_score_attn_map: dtype %d not served by this build", dtype);
    hipStream_t s = (hipStream_t)stream;
    const bool f32 = dtype == GITMI_DTYPE_F32;
    const int d = H * 64, Kc = N_img + Lp;
    void* ctx = nullptr; float2* stats = nullptr;
    auto body = [&]() -> int {
        HIPCK(hipMalloc(&ctx, (size_t)Q * Lp * d * (f32 ? 4 : 2)));
        HIPCK(hipMalloc(&stats, (size_t)Q * H * Lp * sizeof(float2)));
        HIPCK(launch_score_attn(qkv, img_kv, image_of, ctx, Q, H, d, N_img, Lp, 0.125f, f32, s, ntok, stats));
        HIPCK(launch_score_attn_map(qkv, img_kv, image_of, ntok, stats, nullptr, out, (size_t)Lp * Kc, (size_t)Kc, Lp, Q, H, N_img, Lp,
                                    0.125f, f32, nullptr, s));
        HIPCK(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    hipFree(ctx); hipFree(stats);
    return rc;
}
// tree attention of one layer (GITMI_SEARCH_TREE_SCORE): score_attn's operands with the rows of every "sentence" the nodes of a
// tree -- packed int64 [Q][Lp] DEVICE (depth << 32 | token), lens int32 [Q] DEVICE node counts, max_depth the depth bound -- and
// ntok as in score_attn_map: the structure launch, then the attention launch with its end[] table.  bad_out int32 [Q] DEVICE
// (or NULL) = the structure verdicts.  Synchronises the stream.
GITMI_EXP_EXPORT int gitmi_debug_score_attn_tree(const void* qkv, const void* img_kv, const int* image_of, const int* ntok,
                                                 const int64_t* packed, const int* lens, int max_depth, void* out, int* bad_out,
                                                 int Q, int H, int N_img, int Lp, int dtype, void* stream) {
    if (!qkv || !img_kv || !image_of || !packed || !lens || !out || Q < 1 || H < 1 || N_img < 1 || Lp < 1 || max_depth < 1)
        return fail("debug_score_attn_tree: bad argument");
    if (dtype != GITMI_DTYPE_F32 && dtype != gitmi_operand_dtype()) return fail("debug_score_attn_tree: dtype %d not served by this build", dtype);
    hipStream_t s = (hipStream_t)stream;
    const size_t M = (size_t)Q * Lp;
    int* tab = nullptr;
    auto body = [&]() -> int {
        HIPCK(hipMalloc(&tab, (4 * M + Q) * sizeof(int)));
        const TreeNodes nd{tab, tab + M, tab + 2 * M, tab + 3 * M};
        int* bad = tab + 4 * M;
        HIPCK(hipMemsetAsync(bad, 0, (size_t)Q * sizeof(int), s));
        HIPCK(launch_tree_structure((const long long*)packed, Lp, Q, Lp, lens, 1 << 30, max_depth, nd, bad, s));
        HIPCK(launch_score_attn(qkv, img_kv, image_of, out, Q, H, H * 64, N_img, Lp, 0.125f, dtype == GITMI_DTYPE_F32, s, ntok, nullptr,
                                nd.end));
        if (bad_out) HIPCK(hipMemcpyAsync(bad_out, bad, (size_t)Q * sizeof(int), hipMemcpyDefault, s));
        HIPCK(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    hipFree(tab);
    return rc;
}
// head + combine: logits z = A [M][K] W [V][K]^T + bias (never stored in the 16-bit form) -> out fp32 [M][2] =
// (log_softmax(z)[tgt[m]], mean_c log_softmax(z)[c]) for rows with tgt[m] >= 0, 0 elsewhere.  Synchronises the stream.
GITMI_EXP_EXPORT int gitmi_debug_score_head(const void* A, const void* W, const float* bias, const int* tgt, int M, int V, int K,
                                            int dtype, float* out, void* stream) {
    if (!A || !W || !bias || !tgt || !out || M < 1 || V < 2 || K < 32 || K % 32) return fail("debug_score_head: bad argument");
    if (dtype != GITMI_DTYPE_F32 && dtype != gitmi_operand_dtype()) return fail("debug_score_head: dtype %d not served by this build", dtype);
    hipStream_t s = (hipStream_t)stream;
    const bool f32 = dtype == GITMI_DTYPE_F32;
    const int ntiles = f32 ? 1 : score_head_tiles(V);
    const int ldl = round_up(V, 8);
    float4* part = nullptr; float* zt = nullptr; float2* o2 = nullptr; int* bad = nullptr; float* logits = nullptr;
    int rc = 0;
    auto body = [&]() -> int {
        HIPCK(hipMalloc(&part, (size_t)M * ntiles * sizeof(float4)));
        HIPCK(hipMalloc(&zt, (size_t)M * sizeof(float)));
        HIPCK(hipMalloc(&o2, (size_t)(M + 1) * sizeof(float2)));
        HIPCK(hipMalloc(&bad, (size_t)M * sizeof(int)));
        if (f32) {
            HIPCK(hipMalloc(&logits, (size_t)M * ldl * sizeof(float)));
            GemmArgs g{};
            g.A = A; g.W = W; g.bias = bias; g.C = logits; g.M = M; g.N = V; g.K = K; g.lda = K; g.ldc = ldl;
            HIPCK(launch_gemm(g, true, true, s));
            HIPCK(launch_score_rowstats(logits, ldl, V, tgt, 0, M, part, zt, s));
        } else {
            HIPCK(launch_score_head(A, K, W, bias, tgt, M, V, K, part, zt, s));
        }
        HIPCK(hipMemsetAsync(o2, 0, (size_t)(M + 1) * sizeof(float2), s));
        // one position per "sentence" (Lp = ld = 1): row m lands in o2[m + 1]
        HIPCK(launch_score_combine(part, ntiles, zt, tgt, M, 1, 1, V, o2, bad, s));
        HIPCK(hipMemcpyAsync(out, o2 + 1, (size_t)M * sizeof(float2), hipMemcpyDefault, s));
        HIPCK(hipStreamSynchronize(s));
        return 0;
    };
    rc = body();
    hipFree(part); hipFree(zt); hipFree(o2); hipFree(bad); hipFree(logits);
    return rc;
}

// ---- op hooks of the image front end of the encoder (kernels_norm.hip; tests/test_gpu_frontend_ops.py) -----------------------
// Each one is an argument check + the launcher encode_frames_impl calls, so the launcher's kernel selection is what runs.
#ifdef GITMI_EXPERIMENT
GITMI_EXP_EXPORT int gitmi_debug_im2col(const float* img, void* out, int out_dtype, int B, int H, int W, int p, int K, int Kpad,
                                        void* stream) {
    if (!img || !out) return fail("debug_im2col: null argument");
    RCK(check_dtype("debug_im2col", "out_dtype", out_dtype));
    if (B < 1 || p < 1 || H < p || W < p || K != 3 * p * p || Kpad < K) return fail("debug_im2col: bad shape");
    HIPCK(launch_im2col(img, out, out_dtype == GITMI_DTYPE_F32, B, H, W, p, K, Kpad, (hipStream_t)stream));
    return 0;
}
GITMI_EXP_EXPORT int gitmi_debug_pos_resize(const float* pos, float* out, int g, int gh, int gw, int D, void* stream) {
    if (!pos || !out || g < 1 || gh < 1 || gw < 1 || D < 1) return fail("debug_pos_resize: bad argument");
    HIPCK(launch_pos_bicubic(pos, out, g, gh, gw, D, (hipStream_t)stream));
    return 0;
}
GITMI_EXP_EXPORT int gitmi_debug_vit_assemble(const float* patch_out, const float* cls, const float* pos, const float* gamma,
                                              const float* beta, float eps, void* X, int x_f16, int B, int N, int D, float* part,
                                              void* stream) {
    if (!patch_out || !cls || !pos || !gamma || !beta || !X || B < 1 || N < 1 || D < 1) return fail("debug_vit_assemble: bad argument");
    HIPCK(launch_vit_assemble_ln(patch_out, cls, pos, gamma, beta, eps, X, x_f16 != 0, B, N, D, (float2*)part, (D + 255) / 256,
                                 (hipStream_t)stream));
    return 0;
}
GITMI_EXP_EXPORT int gitmi_debug_ragged_front(int stage, const float* src, float* slots, int* meta, int* ntok, void* patches,
                                              int patches_dtype, const float* patch_out, const float* cls, const float* pos, int g,
                                              const float* gamma, const float* beta, float eps, void* X, int x_f16, float* part,
                                              int B, int p, long long max_pixels, int Nmax, int K, int Kpad, int D, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B < 1 || p < 1 || max_pixels < 1 || Nmax < 2 || !meta) return fail("debug_ragged_front: bad argument");
    const size_t slot = (size_t)3 * (size_t)max_pixels;
    if (stage == 0) {
        if (!src || !slots || !ntok) return fail("debug_ragged_front: staging takes src, slots, meta and ntok");
        HIPCK(launch_ragged_stage(src, slots, slot, (int4*)meta, ntok, B, p, (size_t)max_pixels, Nmax, s));
    } else if (stage == 1) {
        if (!slots || !patches || K != 3 * p * p || Kpad < K) return fail("debug_ragged_front: im2col takes slots, meta and patches");
        RCK(check_dtype("debug_ragged_front", "patches_dtype", patches_dtype));
        HIPCK(launch_im2col_ragged(slots, slot, (const int4*)meta, patches, patches_dtype == GITMI_DTYPE_F32, B, Nmax, p, K, Kpad, s));
    } else if (stage == 2) {
        if (!patch_out || !cls || !pos || !gamma || !beta || !X || g < 1 || D < 1) return fail("debug_ragged_front: assembly argument missing");
        HIPCK(launch_vit_assemble_ragged(patch_out, cls, pos, g, (const int4*)meta, gamma, beta, eps, X, x_f16 != 0, B, Nmax, p, D,
                                         (float2*)part, s));
    } else {
        return fail("debug_ragged_front: stage %d (0 staging, 1 im2col, 2 assembly)", stage);
    }
    return 0;
}
GITMI_EXP_EXPORT int gitmi_debug_zero_pad_rows(void* x, int is_f32, int ld, const int* ntok, int B, int Nmax, void* stream) {
    if (!x || !ntok || B < 1 || Nmax < 1 || ld < 1) return fail("debug_zero_pad_rows: bad argument");
    HIPCK(launch_zero_pad_rows(x, is_f32 != 0, ld, ntok, B, Nmax, (hipStream_t)stream));
    return 0;
}
GITMI_EXP_EXPORT int gitmi_debug_layernorm_map(const void* x, int src_f16, const float* gamma, const float* beta, float eps,
                                               const float* add_after, void* y_t, int out_dtype, void* y_s, int rows, int D,
                                               int map_n_in, int map_n_out, int map_off, void* stream) {
    if (!x || !gamma || !beta || (!y_t && !y_s) || rows < 1 || D < 1) return fail("debug_layernorm_map: bad argument");
    if (y_t) RCK(check_dtype("debug_layernorm_map", "out_dtype", out_dtype));
    if (map_n_in > 0 && (map_off < 0 || map_off + map_n_in > map_n_out)) return fail("debug_layernorm_map: row map leaves its block");
    const bool t_is_f32 = out_dtype == GITMI_DTYPE_F32;
    if (src_f16)
        HIPCK(launch_layernorm_s16(x, D, gamma, beta, eps, add_after, y_t, D, t_is_f32, y_s, D, rows, D, map_n_in, map_n_out, map_off,
                                   (hipStream_t)stream));
    else
        HIPCK(launch_layernorm((const float*)x, D, gamma, beta, eps, add_after, y_t, D, t_is_f32, (float*)y_s, D, rows, D, map_n_in,
                               map_n_out, map_off, (hipStream_t)stream));
    return 0;
}
// the context kernel of GITMI_SEARCH_CONTEXT (tests/test_gpu_context_ops.py): the host table context_call builds + the launcher it calls
GITMI_EXP_EXPORT int gitmi_debug_context_embed(const int64_t* tokens, int ld, const int32_t* len_host, const int32_t* image_of_host,
                                               int Q, const float* words, int vocab, const float* positions, int max_pos,
                                               const float* gamma, const float* beta, float eps, void* feats, int dtype, float* feats_f32,
                                               int* ntok, int B, int n_img, int stride, int D, void* stream) {
    if (!tokens || !words || !positions || !gamma || !beta || !feats || !ntok) return fail("debug_context_embed: null argument");
    RCK(check_dtype("debug_context_embed", "dtype", dtype));
    if (ld < 1 || vocab < 1 || max_pos < 1 || n_img < 0 || stride < 1 || D < 8 || D > 1024 || D % 8)
        return fail("debug_context_embed: bad shape (D a multiple of 8 up to 1024)");
    if (((uintptr_t)words | (uintptr_t)positions | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)feats | (uintptr_t)feats_f32) & 15)
        return fail("debug_context_embed: tables and rows must be 16-byte aligned");
    ContextTable t;
    RCK(context_table("debug_context_embed", len_host, image_of_host, Q, B, std::min(ld, max_pos), n_img, stride, &t));
    hipStream_t s = (hipStream_t)stream;
    int* tab = nullptr;
    HIPCK(hipMalloc((void**)&tab, t.tab.size() * sizeof(int)));
    auto body = [&]() -> int {
        HIPCK(hipMemcpy(tab, t.tab.data(), t.tab.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCK(launch_context_embed((const long long*)tokens, ld, (const int4*)tab, Q, tab + 4 * (size_t)Q, words, positions, gamma, beta, eps,
                                   feats, dtype == GITMI_DTYPE_F32, feats_f32, ntok, B, n_img, stride, D, vocab, max_pos, s));
        HIPCK(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    hipFree(tab);
    return rc;
}

// ---- op hooks of the text pass around its attention (kernels_score.hip; tests/test_gpu_text_pass_ops.py) ---------------------
// Each one is an argument check + the launchers text_pass_impl calls, in its order.
GITMI_EXP_EXPORT int gitmi_debug_score_embed(const int64_t* tokens, int Q, int ld, int Lp, const float* words, int vocab,
                                             const float* positions, int max_pos, const float* gamma, const float* beta, float eps,
                                             int D, float* h_f, void* h_t, int dtype, const int* node_tok, const int* node_depth,
                                             void* stream) {
    if (!tokens || !words || !positions || !gamma || !beta || !h_f || !h_t) return fail("debug_score_embed: null argument");
    RCK(check_dtype("debug_score_embed", "dtype", dtype));
    if (Q < 1 || ld < 1 || Lp < 1 || vocab < 1 || max_pos < 1 || D < 4 || D > 1024 || D % 4)
        return fail("debug_score_embed: bad shape (D a multiple of 4 up to 1024)");
    if (!node_tok != !node_depth) return fail("debug_score_embed: the node tables come together");
    if (((uintptr_t)words | (uintptr_t)positions | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)h_f | (uintptr_t)h_t) & 15)
        return fail("debug_score_embed: tables and rows must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (node_tok) {       // the tree instantiation forms its addresses from the tables as they are (the structure kernel's output)
        const size_t M = (size_t)Q * Lp;
        std::vector<int> host(2 * M);
        HIPCK(hipMemcpyAsync(host.data(), node_tok, M * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCK(hipMemcpyAsync(host.data() + M, node_depth, M * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        for (size_t i = 0; i < M; ++i)
            if (host[i] < 0 || host[i] >= vocab || host[M + i] < 0 || host[M + i] >= max_pos)
                return fail("debug_score_embed: node row %zu (token %d, depth %d) outside the tables", i, host[i], host[M + i]);
    }
    const TreeNodes nd{const_cast<int*>(node_tok), const_cast<int*>(node_depth), nullptr, nullptr};
    HIPCK(launch_score_embed_ln((const long long*)tokens, ld, Q, Lp, words, positions, gamma, beta, eps, h_f, h_t, dtype == GITMI_DTYPE_F32,
                                D, vocab, max_pos, s, node_tok ? &nd : nullptr));
    return 0;
}
GITMI_EXP_EXPORT int gitmi_debug_tree_tables(const int64_t* packed, const int* lens, int Q, int ld, int Lp, int V, int max_depth,
                                             int* tok, int* depth, int* parent, int* end, int* bad, void* stream) {
    if (!packed || !lens || !tok || !depth || !parent || !end || !bad) return fail("debug_tree_tables: null argument");
    if (Q < 1 || ld < 1 || Lp < 1 || V < 1 || max_depth < 1 || max_depth > 8192) return fail("debug_tree_tables: bad shape");
    hipStream_t s = (hipStream_t)stream;
    HIPCK(hipMemsetAsync(bad, 0, (size_t)Q * sizeof(int), s));
    HIPCK(launch_tree_structure((const long long*)packed, ld, Q, Lp, lens, V, max_depth, TreeNodes{tok, depth, parent, end}, bad, s));
    return 0;
}
GITMI_EXP_EXPORT int gitmi_debug_score_tail(const void* A, const void* W, const float* bias, const int64_t* tokens, const int* lens,
                                            int Q, int ld, int Lp, int V, int K, int dtype, int chunk_rows, int tree_max_depth,
                                            float* out, int* bad, int* info, int* tgt_out, float* zt_out, void* stream) {
    if (!A || !W || !bias || !tokens || !lens || !out || !bad || !info) return fail("debug_score_tail: null argument");
    RCK(check_dtype("debug_score_tail", "dtype", dtype));
    const bool f32 = dtype == GITMI_DTYPE_F32, tree = tree_max_depth > 0;
    if (Q < 1 || ld < 1 || Lp < 1 || V < 2 || K < 32 || K % 32 || (size_t)Q * Lp > (1u << 20))
        return fail("debug_score_tail: bad shape (K a multiple of 32, at most 2^20 rows)");
    if (tree_max_depth < 0 || tree_max_depth > 8192) return fail("debug_score_tail: tree_max_depth=%d outside [0,8192]", tree_max_depth);
    if (f32 && (chunk_rows < 1 || chunk_rows > Q * Lp))
        return fail("debug_score_tail: the fp32 head needs chunk_rows in [1, Q * Lp = %d], got %d", Q * Lp, chunk_rows);
    if (((uintptr_t)A | (uintptr_t)W) & 15) return fail("debug_score_tail: A and W must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // sentences: the target and combine kernels index the caller's tables by the lengths, as the engine's calls do after
    // read_sentences has checked them.  (Trees: the structure kernel clamps the node count itself.)
    if (!tree) {
        std::vector<int> len_host(Q);
        HIPCK(hipMemcpyAsync(len_host.data(), lens, (size_t)Q * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        for (int q = 0; q < Q; ++q)
            if (len_host[q] < 1 || len_host[q] > ld) return fail("debug_score_tail: length %d of sentence %d outside [1,%d]", len_host[q], q, ld);
    }
    const int M = Q * Lp, ldl = round_up(V, 8);
    int* tab = nullptr; float4* part = nullptr; float* zt = nullptr; float* logits = nullptr;
    auto body = [&]() -> int {
        HIPCK(hipMalloc(&tab, (size_t)(tree ? 5 : 1) * M * sizeof(int)));
        HIPCK(hipMalloc(&part, (size_t)M * (f32 ? 1 : score_head_tiles(V)) * sizeof(float4)));
        HIPCK(hipMalloc(&zt, (size_t)M * sizeof(float)));
        if (f32) HIPCK(hipMalloc(&logits, (size_t)chunk_rows * ldl * sizeof(float)));
        int* tgt = tab;
        const TreeNodes nd{tab + M, tab + 2 * (size_t)M, tab + 3 * (size_t)M, tab + 4 * (size_t)M};
        const ScoreHeadArgs h{A, W, bias, tgt, part, zt, logits, ldl, chunk_rows};
        int ntiles = 1;
        HIPCK(hipMemsetAsync(bad, 0, (size_t)Q * sizeof(int), s));
        HIPCK(hipMemsetAsync(zt, 0xff, (size_t)M * sizeof(float), s));         // a logit nobody gathered is a NaN, not a stale value
        if (tree) {
            HIPCK(launch_tree_structure((const long long*)tokens, ld, Q, Lp, lens, V, tree_max_depth, nd, bad, s));
            HIPCK(hipMemsetAsync(tgt, 0xff, (size_t)M * sizeof(int), s));
            HIPCK(launch_score_head_rows(h, f32, M, V, K, &nd, Lp, &ntiles, s));
            HIPCK(launch_tree_combine(part, ntiles, zt, nd, M, Lp, ld, V, (float2*)out, bad, s));
        } else {
            HIPCK(launch_score_targets((const long long*)tokens, ld, Lp, lens, V, M, tgt, s));
            HIPCK(launch_score_head_rows(h, f32, M, V, K, nullptr, 0, &ntiles, s));
            HIPCK(launch_score_combine(part, ntiles, zt, tgt, M, Lp, ld, V, (float2*)out, bad, s));
        }
        HIPCK(launch_score_info(bad, Q, ld, info, s));
        if (tgt_out) HIPCK(hipMemcpyAsync(tgt_out, tgt, (size_t)M * sizeof(int), hipMemcpyDefault, s));
        if (zt_out) HIPCK(hipMemcpyAsync(zt_out, zt, (size_t)M * sizeof(float), hipMemcpyDefault, s));
        HIPCK(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    hipFree(tab); hipFree(part); hipFree(zt); hipFree(logits);
    return rc;
}
#endif
