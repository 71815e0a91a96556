// Host side of the GIT engine: the forward schedule (ViT encode -> decoder prefill over image tokens -> KV-cached
// decode steps -> device search), generate / graph, scoring, setters, profiling and the C ABI of include/gitmi.h.
// The state lives in engine_state.h; weight ingest/repack, clones and workspaces in engine_weights.hip.
//
// Schedule vs. the reference (SURVEY.md headline facts 2/3): the reference re-runs the visual
// projection and all decoder layers over [image | text] tokens at every decode step and for every
// beam copy.  Image rows never attend to text (mask top-right = -inf) and text is causal, so
// computing the image rows once per image and caching K/V is exact; this engine does that.
#include "../../include/gitmi.h"
#include "engine_state.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

using namespace gitmi;

// Entry points of the measurement build (include/gitmi_experiment.h): schedules that measured slower than the default and
// debug hooks.  The product libraries keep the code paths (they share the generate machinery) but do not export them.
#ifdef GITMI_EXPERIMENT
#include "../../include/gitmi_experiment.h"
#define GITMI_EXP_EXPORT extern "C"
#else
#define GITMI_EXP_EXPORT [[maybe_unused]] static
#endif

// ---------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
int gitmi::fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

static hipEvent_t get_event(gitmi_engine* e) {
    if (e->event_next == e->event_pool.size()) {
        hipEvent_t ev;
        hipEventCreate(&ev);
        e->event_pool.push_back(ev);
    }
    return e->event_pool[e->event_next++];
}
struct SpanGuard {
    gitmi_engine* e; hipStream_t s; size_t idx; bool on;
    SpanGuard(gitmi_engine* e_, hipStream_t s_, int tag, double flops) : e(e_), s(s_), idx(0), on(e_->profiling) {
        if (!on) return;
        TimedSpan sp{get_event(e), get_event(e), tag, flops};
        hipEventRecord(sp.a, s);
        idx = e->spans.size();
        e->spans.push_back(sp);
    }
    ~SpanGuard() { if (on) hipEventRecord(e->spans[idx].b, s); }
};

// serving policy of the encoder GEMM's tile height (kernels_gemm10.hip: launch_gemm_p8): 256-row tiles whatever the round
// fill, because other contexts' kernels fill the CUs a partial round leaves idle.  gemm_tall (measurement builds): 1 always,
// 0 never (the modelled height, as for a context alone), 2 only for the wide GEMMs (N >= 2048), 3 only for the N < 2048 ones
static bool gemm_tall_tiles(const gitmi_engine* e, int N) {
    if (!e->pol.shared_device) return false;
    return e->pol.gemm_tall == 1 || (e->pol.gemm_tall == 2 && N >= 2048) || (e->pol.gemm_tall == 3 && N < 2048);
}

static double gemm_flops(int M, int N, int K) { return 2.0 * (double)M * (double)N * (double)K; }
// ---- the schedule's large-M GEMMs: C = act(A W^T + bias) (+ res).  gemm_args fills what every form shares, gemm_run adds
// the tile policy and the profiling span and launches; the forms below differ in a few fields of the arguments
static GemmArgs gemm_args(const void* A, int lda, const void* W, const float* bias, const void* res, int ldr, void* C, int ldc,
                          int M, int N, int K, int act) {
    GemmArgs g{};
    g.A = A; g.W = W; g.bias = bias; g.res = (const float*)res; g.C = C;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc; g.ldr = ldr; g.act = act;
    return g;
}
static int gemm_run(gitmi_engine* e, hipStream_t s, GemmArgs g, bool in_f32, bool out_f32, int tag) {
    g.shared = gemm_tall_tiles(e, g.N) ? 1 : 0;
    SpanGuard sp(e, s, tag, gemm_flops(g.M, g.N, g.K));
    HIPCK(launch_gemm(g, in_f32, out_f32, s));
    return 0;
}
static int gemm(gitmi_engine* e, hipStream_t s, const void* A, int lda, const void* W, const float* bias,
                const float* res, int ldr, void* C, int ldc, bool out_f32, int M, int N, int K, int act, int tag) {
    return gemm_run(e, s, gemm_args(A, lda, W, bias, res, ldr, C, ldc, M, N, K, act), e->pol.f32, out_f32, tag);
}
// does a 16-bit GEMM of this shape run on gemm_p8_kernel (the only kernel with the folded epilogues)?
static bool on_p8(const void* A, int lda, const void* W, const void* C, int ldc, int M, int N, int K, bool stream_out) {
    GemmArgs g = gemm_args(A, lda, W, nullptr, nullptr, 0, const_cast<void*>(C), ldc, M, N, K, 0);
    g.out_f16 = stream_out ? 1 : 0;
    return gemm_uses_p8(g, false, false);
}
// ---- the residual stream of a pass (ViT blocks: v_x, prefill layers: p_y; fp32 rows, or fp16 with stream_f16) and the
// LayerNorm (gamma, beta, eps) that stands between its rows and their consumers right now.  A layer is written once, on
// ln_gemm / gemm_to_stream; its LayerNorms have two realisations.  Folded (the pass's gate; implies stream_f16): x keeps the raw
// sums, the consumer GEMMs read them as their A operand, and whoever writes the rows leaves their row partials `part`.
// Unfolded: a launch materialises LayerNorm(x) as the operand copy `t` (and as the stream rows `xn`).
struct Stream {
    void* x = nullptr; int M = 0, D = 0, tag = 0;
    bool fold = false;
    void* t = nullptr;
    // post-norm passes (BERT) keep the normalised rows: a producer's residual is LayerNorm(x) -- xn, or rebuilt from the
    // partials when folded -- where a pre-norm pass (ViT, xn == nullptr) adds x itself
    float* xn = nullptr;
    // partials buffers, attached by the gate when the pass folds.  Post-norm passes need two: a producer's tile reads the
    // previous partials of a row for the residual while another tile (another workgroup) writes the new ones
    float2* parts[2] = {nullptr, nullptr};
    const float2* part = nullptr; const float* gamma = nullptr; const float* beta = nullptr; float eps = 0.f;
};
// where the next writer of the rows leaves their partials: the buffer that is not being read (nullptr: the pass is not folded)
static float2* stream_part_out(const Stream& st) { return st.part == st.parts[0] ? st.parts[1] : st.parts[0]; }
// the rows were (re)written, with their partials in `part`: LayerNorm(gamma, beta, eps) stands in front of the consumers from here on
static void stream_written(Stream& st, const float2* part, const float* gamma, const float* beta, float eps) {
    st.part = part; st.gamma = gamma; st.beta = beta; st.eps = eps;
}
// consumer: columns [col0, col0 + N) of C = act(LayerNorm(stream) W^T + b); f: 16-bit(W . gamma), beta W^T + b, column sums
static int ln_gemm(gitmi_engine* e, hipStream_t s, const Stream& st, const Folded& f, const void* W, const float* bias, void* C,
                   int ldc, int col0, int N, int act) {
    const int D = st.D;
    const size_t woff = (size_t)col0 * D * e->pol.esz;
    C = (char*)C + (size_t)col0 * e->pol.esz;
    if (st.fold) {
        GemmArgs g = gemm_args(st.x, D, (const char*)f.w + woff, f.bias + col0, nullptr, 0, C, ldc, st.M, N, D, act);
        g.ln_part = st.part; g.ln_nparts = D / 256; g.ln_colsum = f.colsum + col0; g.ln_inv_d = 1.0f / (float)D; g.ln_eps = st.eps;
        return gemm_run(e, s, g, false, false, st.tag);
    }
    if (e->pol.stream_f16)
        HIPCK(launch_layernorm_s16(st.x, D, st.gamma, st.beta, st.eps, nullptr, st.t, D, false, st.xn, st.xn ? D : 0, st.M, D, 0, 0, 0, s));
    else
        HIPCK(launch_layernorm((const float*)st.x, D, st.gamma, st.beta, st.eps, nullptr, st.t, D, e->pol.f32, st.xn, st.xn ? D : 0, st.M,
                               D, 0, 0, 0, s));
    return gemm(e, s, st.t, D, (const char*)W + woff, bias + col0, nullptr, 0, C, ldc, e->pol.f32, st.M, N, D, act, st.tag);
}
// producer: stream rows = A W^T + b (+ the pass's residual), after which LayerNorm(gamma, beta, eps) stands on them
// (gamma == nullptr: none of the pass's own follows, nobody reads partials of these rows)
static int gemm_to_stream(gitmi_engine* e, hipStream_t s, Stream& st, const void* A, int lda, const void* W, const float* bias, int K,
                          bool residual, const float* gamma, const float* beta, float eps) {
    const int D = st.D;
    float2* part = gamma ? stream_part_out(st) : nullptr;
    const void* res = !residual ? nullptr : st.xn && !st.fold ? st.xn : st.x;
    GemmArgs g = gemm_args(A, lda, W, bias, res, residual ? D : 0, st.x, D, st.M, D, K, 0);
    g.out_f16 = e->pol.stream_f16 ? 1 : 0;
    if (st.fold) {
        g.part_out = part;
        if (residual && st.xn) {        // the residual added is LayerNorm(res), rebuilt from the partials of the raw rows
            g.res_part = st.part; g.res_nparts = D / 256; g.res_gamma = st.gamma; g.res_beta = st.beta;
            g.res_inv_d = 1.0f / (float)D; g.res_eps = st.eps;
        }
    }
    RCK(gemm_run(e, s, g, e->pol.f32, !e->pol.stream_f16, st.tag));
    stream_written(st, part, gamma, beta, eps);
    return 0;
}
// full attention over packed q|k|v rows [batch * N][3 * width] -> out [batch * N][width]
// ntok: keys (and query rows) per block, or nullptr: N each
static int attn_full_packed(gitmi_engine* e, const void* qkv, void* out, int width, int heads, int N, int batch, const int* ntok,
                            hipStream_t s) {
    AttnFullArgs a{};
    a.q = qkv;
    a.k = (const char*)qkv + (size_t)width * e->pol.esz;
    a.v = (const char*)qkv + (size_t)2 * width * e->pol.esz;
    a.out = out;
    a.ldq = a.ldk = a.ldv = 3 * width;
    a.ldo = width;
    a.N = N; a.H = heads; a.scale = 0.125f;
    a.ntok = ntok;
    HIPCK(launch_attn_full(a, batch, e->pol.f32, e->pol.attn_impl, s));
    return 0;
}
// generic post-norm tail of a decoder layer over M rows (decode steps outside the chain, caption scoring): out-proj + residual,
// LayerNorm, FFN1, FFN2 + residual, LayerNorm.  ctx: the attention output; hf / ht: the layer's input rows (fp32 / compute
// dtype), replaced by its output rows; y: the pre-LayerNorm sums; u: the FFN's inner rows
static int dec_layer_tail(gitmi_engine* e, hipStream_t s, const DecLayerW& L, const void* ctx, float* hf, void* ht, float* y, void* u,
                          int M) {
    const int d = e->cfg.dec_hidden, ffn = e->cfg.dec_ffn;
    RCK(gemm(e, s, ctx, d, L.wo, L.bo, hf, d, y, d, true, M, d, d, 0, TAG_GEMM_OTHER));
    HIPCK(launch_layernorm(y, d, L.lnag, L.lnab, 1e-12f, nullptr, ht, d, e->pol.f32, hf, d, M, d, 0, 0, 0, s));
    RCK(gemm(e, s, ht, d, L.w1, L.b1, nullptr, 0, u, ffn, e->pol.f32, M, ffn, d, 2, TAG_GEMM_OTHER));
    RCK(gemm(e, s, u, ffn, L.w2, L.b2, hf, d, y, d, true, M, d, ffn, 0, TAG_GEMM_OTHER));
    HIPCK(launch_layernorm(y, d, L.lnog, L.lnob, 1e-12f, nullptr, ht, d, e->pol.f32, hf, d, M, d, 0, 0, 0, s));
    return 0;
}

// ---------------------------------------------------------------------------------------
extern "C" int gitmi_abi_version(void) { return GITMI_ABI_VERSION; }
// 16-bit operand type this library was built for: GITMI_DTYPE_BF16 (libgitmi.so) or GITMI_DTYPE_F16 (libgitmi_f16.so)
extern "C" int gitmi_operand_dtype(void) {
#ifdef GITMI_OPS_F16
    return GITMI_DTYPE_F16;
#else
    return GITMI_DTYPE_BF16;
#endif
}
extern "C" const char* gitmi_last_error(void) { return g_err; }

extern "C" int gitmi_create(const gitmi_config* cfg, int device, gitmi_engine** out) {
    if (!cfg || !out) return fail("gitmi_create: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail("gitmi_create: no HIP device available (this engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail("gitmi_create: device %d out of range (%d devices)", device, ndev);
    HIPCK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("gitmi_create: device %d is %s; this library is built for gfx950 (MI355X) only", device,
                    prop.gcnArchName);
    const gitmi_config& c = *cfg;
    if (c.vit_width % c.vit_heads || c.vit_width / c.vit_heads != 64) return fail("ViT head_dim must be 64");
    if (c.dec_hidden % c.dec_heads || c.dec_hidden / c.dec_heads != 64) return fail("decoder head_dim must be 64");
    if (c.image_size % c.patch) return fail("image_size must be a multiple of patch");
    if (c.max_image_pixels < 0 || c.max_image_tokens < 0) return fail("negative image capacity");
    if (c.vit_width > 1024 || c.dec_hidden > 1024) return fail("hidden sizes above 1024 are not supported");
    if (c.vit_width % 64 || c.dec_hidden % 64 || c.dec_ffn % 64) return fail("hidden sizes must be multiples of 64");
    if (c.max_batch < 1 || c.max_beams < 1 || c.max_beams > 8 || c.max_frames < 1 || c.max_text_len < 2)
        return fail("bad capacity (max_batch>=1, 1<=max_beams<=8, max_frames>=1, max_text_len>=2)");
    if (c.max_text_len > c.max_pos) return fail("max_text_len exceeds max_pos");
    if (c.precision != GITMI_PREC_BF16 && c.precision != GITMI_PREC_F32) return fail("bad precision");

    gitmi_engine* e = new gitmi_engine();
    e->cfg = c;
    e->device = device;
    e->pol.f32 = c.precision == GITMI_PREC_F32;
    e->pol.esz = e->pol.f32 ? 4 : 2;
    e->pol.attn_impl = e->pol.f32 ? 0 : 1;
    init_geometry(e);
    e->pol.stream_f16 = !e->pol.f32;
#ifdef GITMI_OPS_F16
    e->pol.ln_fold = !e->pol.f32 && c.vit_width % 256 == 0 && c.dec_hidden % 256 == 0;
#endif
#ifdef GITMI_EXPERIMENT
    // measurement builds only (libgitmi_exp.so, `make exp`): kernel-shape overrides and work-skipping switches for A/B runs
    // and timing decompositions.  The product libraries read no environment.
    if (const char* env = getenv("GITMI_ATTN_IMPL")) e->pol.attn_impl = e->pol.f32 ? 0 : atoi(env);
    if (const char* env = getenv("GITMI_GRAPH")) e->pol.use_graph = atoi(env) != 0;
    if (const char* env = getenv("GITMI_ATTN_DBG")) e->pol.attn_dbg = atoi(env);
    if (const char* env = getenv("GITMI_ATTN_PW")) e->pol.attn_pw = atoi(env);
    if (const char* env = getenv("GITMI_ATTN_NH")) e->pol.attn_nh = atoi(env);
    if (const char* env = getenv("GITMI_ATTN_STREAM")) e->pol.attn_stream = atoi(env);
    if (const char* env = getenv("GITMI_DECODE_SKIP")) e->pol.decode_skip = atoi(env);
    if (const char* env = getenv("GITMI_GEMM_TALL")) e->pol.gemm_tall = atoi(env);
    if (const char* env = getenv("GITMI_DGEMM_ROWS")) e->pol.dgemm_rows = atoi(env);
    if (const char* env = getenv("GITMI_DGEMM_STRIPS")) e->pol.dgemm_strips = atoi(env);
    if (const char* env = getenv("GITMI_DGEMM_NO_ROW_WALK")) e->pol.dgemm_no_row_walk = atoi(env);
    if (const char* env = getenv("GITMI_DGEMM_DBG")) e->pol.dgemm_dbg = atoi(env);
    if (const char* env = getenv("GITMI_VOCAB_WGS")) e->pol.vocab_wgs = atoi(env);
    if (const char* env = getenv("GITMI_SKINNY")) e->pol.skinny = atoi(env) != 0;
    if (const char* env = getenv("GITMI_STREAM_F16")) e->pol.stream_f16 = !e->pol.f32 && atoi(env) != 0;
    if (const char* env = getenv("GITMI_GEMM_IMPL")) set_gemm_impl(atoi(env));
#endif
    e->pol.ln_fold = e->pol.ln_fold && e->pol.stream_f16;
    e->pol.ln_fold_ready = e->pol.ln_fold;
    *out = e;
    return 0;
}

int CapturedGraph::capture(hipStream_t s, const std::function<int()>& fn) {
    reset();
    HIPCK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = fn();            // 0, or the code of a gitmi::fail: nothing has run on the device either way
    const hipError_t ce = hipStreamEndCapture(s, &graph);
    if (rc != 0 || ce != hipSuccess) reset();
    RCK(rc);
    HIPCK(ce);
    HIPCK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    return 0;
}
// both hipGraph slots: full calls (one graph, or encode + prefill | decode) and follow-up calls (decode alone)
static void destroy_graph(gitmi_engine* e) {
    for (auto& gs : e->graphs) {
        for (CapturedGraph* g : {&gs.graph_full, &gs.graph_decode, &gs.graph_follow}) g->reset();
        gs.full_slot.valid = gs.follow_slot.valid = false;
    }
}
// ---- residency (include/gitmi.h: what a follow-up call runs over): the only writers of cur_* / have_* ----
// the engine's images stop being resident: an encode starts (or failed), or a setter changed what an encode would produce
static void drop_resident(gitmi_engine* e) { e->have_feats = e->have_prefill = false; }
// an encode of B images with F_eff frames each is enqueued (or replayed, or imported): they are resident, their K/V is not
// stride: the rows of an image's block when they are more than its F_eff * N image rows (a context call), else 0.  Key counts
// are in use from here on exactly when the front end is ragged; a context call turns them on itself (set_context)
static void set_resident(gitmi_engine* e, int B, int F_eff, int stride = 0) {
    e->cur_B = B; e->cur_F = F_eff; e->cur_Nimg = stride > 0 ? stride : F_eff * e->N;
    e->have_feats = true; e->have_prefill = false;
    e->keyed = e->ragged; e->has_context = false;
    e->res_desc.clear();
}
// the resident images carry context rows behind their image rows, rg_ntok holds every image's key count
static void set_context(gitmi_engine* e) { e->keyed = e->has_context = true; }
// per-image key counts of the resident batch (ragged images, context rows), or nullptr: cur_Nimg keys each
static const int* key_counts(const gitmi_engine* e) { return e->keyed ? e->rg_ntok : nullptr; }
static void set_prefilled(gitmi_engine* e) { e->have_prefill = true; }
// The failure rule, for every call that runs over images (rc: what its launches returned):
//   a call that was given frames and fails after its first launch or capture leaves NOTHING resident (the workspaces are
//     partly overwritten, or -- a failed capture -- the host side of the encode ran and nothing on the device);
//   a follow-up call (frames == NULL) that fails leaves what was resident: it writes text caches only;
//   an argument error is found before any launch and never gets here: it leaves everything as it was.
static int settle_residency(gitmi_engine* e, const Request& rq, int rc) {
    if (rc != 0 && rq.frames) drop_resident(e);
    return rc;
}

extern "C" void gitmi_destroy(gitmi_engine* e) {
    if (!e) return;
    hipSetDevice(e->device);
    hipDeviceSynchronize();
    // serving-schedule links: nobody keeps a pointer to a destroyed context
    if (e->enc_after) {
        auto& w = e->enc_after->enc_watchers;
        w.erase(std::remove(w.begin(), w.end(), e), w.end());
    }
    for (gitmi_engine* w : e->enc_watchers) w->enc_after = nullptr;
    destroy_graph(e);
    if (e->own_stream) hipStreamDestroy(e->own_stream);
    if (e->fence_in) hipEventDestroy(e->fence_in);
    if (e->fence_out) hipEventDestroy(e->fence_out);
    for (auto ev : e->gev)
        if (ev) hipEventDestroy(ev);
    if (e->enc_done) hipEventDestroy(e->enc_done);
    for (auto ev : e->event_pool) hipEventDestroy(ev);
    for (void* p : e->allocs) hipFree(p);
    for (void* p : e->sc_allocs) hipFree(p);
    hipFree(e->at_out); hipFree(e->at_stats); hipFree(e->ctx_tab); hipFree(e->mem_tab); hipFree(e->feat_tab); hipFree(e->ban_words);
    if (e->ban_stage) hipHostFree(e->ban_stage);
    if (e->ban_staged) hipEventDestroy(e->ban_staged);
    hipFree(e->ban_seq); hipFree(e->ban_row_words); hipFree(e->trace_buf);
    if (e->ban_seq_stage) hipHostFree(e->ban_seq_stage);
    if (e->trie_off) hipFree(e->trie_off);
    if (e->trie_tok) hipFree(e->trie_tok);
    if (e->trie_child) hipFree(e->trie_child);
    delete e;
}

// ---- input resolution (CLIP/model.py:243-251) ---------------------------------------------
extern "C" int gitmi_set_image_shape(gitmi_engine* e, int H, int W, void* stream) {
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("weights not finalized");
    const gitmi_config& c = e->cfg;
    if (H == 0 && W == 0) {         // ragged batches: the shapes travel with the input (include/gitmi.h)
        if (!e->ragged) {
            e->ragged = true;
            e->H = e->W = e->gh = e->gw = 0;
            e->N = e->Nmax;
            drop_resident(e);
        }
        return 0;
    }
    if (H < c.patch || W < c.patch) return fail("image %dx%d is smaller than one %d-pixel patch", H, W, c.patch);
    const int gh = H / c.patch, gw = W / c.patch;
    if ((size_t)H * W > e->max_pixels)
        return fail("image %dx%d exceeds the max_image_pixels capacity (%zu)", H, W, e->max_pixels);
    if (gh * gw + 1 > e->Nmax)
        return fail("a %dx%d token grid exceeds the max_image_tokens capacity (%d)", gh, gw, e->Nmax);
    if (H == e->H && W == e->W && !e->ragged) return 0;
    e->ragged = false;
    HIPCK(hipSetDevice(e->device));
    if (gh == e->g_nat && gw == e->g_nat) {
        e->pos_cur = e->w.pos;
    } else {
        HIPCK(launch_pos_bicubic(e->w.pos, e->pos_var, e->g_nat, gh, gw, c.vit_width, (hipStream_t)stream));
        e->pos_cur = e->pos_var;
    }
    e->H = H; e->W = W; e->gh = gh; e->gw = gw; e->N = gh * gw + 1;
    drop_resident(e);
    return 0;
}

// ---- the fold gates, one per pass: a pass folds its LayerNorms (pol.ln_fold, fp16-operand build) when every GEMM either side
// of them runs on gemm_p8_kernel, i.e. at more than 512 rows; otherwise every LayerNorm is a launch.  They return the pass's
// stream record with the decision and, when it folds, the partials buffers.
static Stream vit_stream(gitmi_engine* e, int M) {
    const int D = e->cfg.vit_width;
    const VitLayerW& L = e->w.vit[0];
    Stream st;
    st.x = e->v_x; st.M = M; st.D = D; st.tag = TAG_GEMM_VIT; st.t = e->v_h;
    st.fold = e->pol.ln_fold && on_p8(e->v_x, D, L.qkv_f.w, e->v_qkv, 3 * D, M, 3 * D, D, false) &&
              on_p8(e->v_x, D, L.ffn1_f.w, e->v_u, 4 * D, M, 4 * D, D, false) && on_p8(e->v_ctx, D, L.wo, e->v_x, D, M, D, D, true) &&
              on_p8(e->v_u, 4 * D, L.w2, e->v_x, D, M, D, 4 * D, true);
    if (st.fold) st.parts[0] = st.parts[1] = e->v_part;     // pre-norm: no producer reads partials, one buffer in place
    return st;
}
// prefill: the visual projection, Q|K|V and the last layer's K|V slice; FFN1, out-proj and FFN2 only where a layer runs them
static Stream prefill_stream(gitmi_engine* e, int M) {
    const int d = e->cfg.dec_hidden, ffn = e->cfg.dec_ffn, D = e->cfg.vit_width;
    const DecLayerW& L = e->w.dec[0];
    Stream st;
    st.x = e->p_y; st.M = M; st.D = d; st.tag = TAG_GEMM_OTHER; st.t = e->p_ht; st.xn = e->p_hf;
    st.fold = e->pol.ln_fold && on_p8(e->feats, D, e->w.vp_w, e->p_y, d, M, d, D, true) &&
              on_p8(e->p_y, d, L.qkv_pf.w, e->img_kv[0], 3 * d, M, 3 * d, d, false) &&
              on_p8(e->p_y, d, L.qkv_pf.w, e->img_kv[0], 3 * d, M, 2 * d, d, false) &&
              (e->cfg.dec_layers < 2 || (on_p8(e->p_y, d, L.ffn1_pf.w, e->p_u, ffn, M, ffn, d, false) &&
                                         on_p8(e->p_ctx, d, L.wo, e->p_y, d, M, d, d, true) && on_p8(e->p_u, ffn, L.w2, e->p_y, d, M, d, ffn, true)));
    if (st.fold) { st.parts[0] = e->p_part[0]; st.parts[1] = e->p_part[1]; }
    return st;
}

// ---------------------------------------------------------------------------------------
// stride > 0 (a context call, never ragged): the rows of an image's block in the feature tensor, more than its F_eff * N image
// rows; the rows behind them are the caller's to write
static int encode_frames_impl(gitmi_engine* e, const float* const* frames, int F, int B, float* feats_out,
                              hipStream_t s, int stride = 0) {
    const gitmi_config& c = e->cfg;
    const int D = c.vit_width, N = e->N;
    const int F_eff = c.num_frames > 0 ? std::min(F, c.num_frames) : F;   // zip() truncation, decoder.py:849
    const int Nimg = stride > 0 ? stride : F_eff * N;
    drop_resident(e);           // the workspaces are overwritten from here on: resident again once the whole pass is enqueued
    SpanGuard phase(e, s, TAG_VIT, 0);
    // all frames of the call go through the encoder as ONE batch of F*B images (the reference encodes frame by
    // frame, decoder.py:847; per-image results are identical, the GEMMs just see M = F*B*197 rows)
    const int BI = F_eff * B;                // images in the pass
    const int M = BI * N;
    const int g2 = N - 1;                    // patch rows per image (ragged: the capacity grid, zeros past each image's own)
    const size_t slot = (size_t)3 * e->max_pixels;
    if (e->ragged)      // F == 1; the images were staged by ragged_stage (the `frames` pointer is not read)
        HIPCK(launch_im2col_ragged(e->frame_stage[0], slot, e->rg_meta, e->patches, e->pol.f32, B, N, c.patch, e->Kp, e->Kp_pad, s));
    else
    for (int fr = 0; fr < F_eff; ++fr)
        HIPCK(launch_im2col(frames[fr], (char*)e->patches + (size_t)fr * B * g2 * e->Kp_pad * e->pol.esz, e->pol.f32, B,
                            e->H, e->W, c.patch, e->Kp, e->Kp_pad, s));
    RCK(gemm(e, s, e->patches, e->Kp_pad, e->w.conv_w, nullptr, nullptr, 0, e->patch_out, D, true, BI * g2, D, e->Kp_pad, 0,
             TAG_GEMM_VIT));
    Stream x = vit_stream(e, M);
    float2* part = stream_part_out(x);
    if (e->ragged)
        HIPCK(launch_vit_assemble_ragged(e->patch_out, e->w.cls, e->w.pos, e->g_nat, e->rg_meta, e->w.lnpre_g, e->w.lnpre_b, 1e-5f, e->v_x,
                                         e->pol.stream_f16, BI, N, c.patch, D, part, s));
    else
    HIPCK(launch_vit_assemble_ln(e->patch_out, e->w.cls, e->pos_cur, e->w.lnpre_g, e->w.lnpre_b, 1e-5f, e->v_x, e->pol.stream_f16, BI, N, D,
                                 part, D / 256, s));
    stream_written(x, part, e->w.vit[0].ln1g, e->w.vit[0].ln1b, 1e-5f);
    for (int l = 0; l < c.vit_layers; ++l) {        // pre-norm block: x += attn(ln_1(x)); x += mlp(ln_2(x))
        const VitLayerW& L = e->w.vit[l];
        const VitLayerW* Ln = l + 1 < c.vit_layers ? &e->w.vit[l + 1] : nullptr;   // ln_post after the last block is a launch of its own
        RCK(ln_gemm(e, s, x, L.qkv_f, L.wqkv, L.bqkv, e->v_qkv, 3 * D, 0, 3 * D, 0));
        RCK(attn_full_packed(e, e->v_qkv, e->v_ctx, D, c.vit_heads, N, BI, e->ragged ? e->rg_ntok : nullptr, s));
        RCK(gemm_to_stream(e, s, x, e->v_ctx, D, L.wo, L.bo, D, true, L.ln2g, L.ln2b, 1e-5f));
        RCK(ln_gemm(e, s, x, L.ffn1_f, L.w1, L.b1, e->v_u, 4 * D, 0, 4 * D, 1));
        RCK(gemm_to_stream(e, s, x, e->v_u, 4 * D, L.w2, L.b2, 4 * D, true, Ln ? Ln->ln1g : nullptr, Ln ? Ln->ln1b : nullptr, 1e-5f));
    }
    // ln_post (+ temporal embedding of the frame), scattered into the concatenated [B, F*N, D] feature tensor
    for (int fr = 0; fr < F_eff; ++fr) {
        const float* te = (c.num_frames > 0 && e->pol.use_temb) ? e->w.temb[fr] : nullptr;
        if (e->pol.stream_f16) {
            const char* xs = (const char*)e->v_x + (size_t)fr * B * N * D * 2;      // fp16 rows
            HIPCK(launch_layernorm_s16(xs, D, e->w.lnpost_g, e->w.lnpost_b, 1e-5f, te, e->feats, D, false, nullptr, 0, B * N, D, N,
                                       Nimg, fr * N, s));
            if (feats_out)      // parity hook: the fp32 copy of the features comes from a second pass over the same rows
                HIPCK(launch_layernorm_s16(xs, D, e->w.lnpost_g, e->w.lnpost_b, 1e-5f, te, feats_out, D, true, nullptr, 0, B * N, D,
                                           N, Nimg, fr * N, s));
        } else {
            HIPCK(launch_layernorm(e->v_x + (size_t)fr * B * N * D, D, e->w.lnpost_g, e->w.lnpost_b, 1e-5f, te, e->feats, D, e->pol.f32,
                                   feats_out, D, B * N, D, N, Nimg, fr * N, s));
        }
    }
    if (e->ragged) {    // padding rows of the features are zeros (prefill rows past an image stay finite and are never keys)
        HIPCK(launch_zero_pad_rows(e->feats, e->pol.f32, D, e->rg_ntok, B, N, s));
        if (feats_out) HIPCK(launch_zero_pad_rows(feats_out, true, D, e->rg_ntok, B, N, s));
    }

    set_resident(e, B, F_eff, stride);      // cur_Nimg == Nimg: N is e->N, ragged (Nmax) or not
    return 0;
}

// image K/V of layer l into the decode layout: head-major (fp32 VALU kernel) or the MFMA operand layouts (bf16)
static int kv_repack(gitmi_engine* e, int l, int B, int Nimg, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    void* kh = e->img_kh[l];
    void* vh = e->img_vh[l];
    if (e->pol.f32) HIPCK(launch_kv_repack(e->img_kv[l], kh, vh, B, Nimg, c.dec_heads, c.dec_hidden, s));
    else HIPCK(launch_kv_repack_frag(e->img_kv[l], kh, vh, B, Nimg, round_up(Nimg, 32), c.dec_heads, c.dec_hidden, s));
    return 0;
}

static int prefill_impl(gitmi_engine* e, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    const int d = c.dec_hidden, ffn = c.dec_ffn, D = c.vit_width;
    const int B = e->cur_B, Nimg = e->cur_Nimg, M = B * Nimg;
    e->have_prefill = false;
    SpanGuard phase(e, s, TAG_PREFILL, 0);
    // post-norm layers: y = LayerNorm(dense(..) + LayerNorm(previous y)), the first LayerNorm the visual projection's own
    Stream y = prefill_stream(e, M);
    RCK(gemm_to_stream(e, s, y, e->feats, D, e->w.vp_w, e->w.vp_b, D, false, e->w.vp_lng, e->w.vp_lnb, 1e-5f));
    for (int l = 0; l < c.dec_layers; ++l) {
        const DecLayerW& L = e->w.dec[l];
        // the last layer's image-row outputs are never consumed: only the K|V columns of its projection, and nothing after them
        const bool last = l + 1 == c.dec_layers;
        const int col0 = last ? d : 0;
        RCK(ln_gemm(e, s, y, L.qkv_pf, L.wqkv, L.bqkv, e->img_kv[l], 3 * d, col0, 3 * d - col0, 0));
        RCK(kv_repack(e, l, B, Nimg, s));
        if (last) break;
        RCK(attn_full_packed(e, e->img_kv[l], e->p_ctx, d, c.dec_heads, Nimg, B, key_counts(e), s));
        RCK(gemm_to_stream(e, s, y, e->p_ctx, d, L.wo, L.bo, d, true, L.lnag, L.lnab, 1e-12f));
        RCK(ln_gemm(e, s, y, L.ffn1_pf, L.w1, L.b1, e->p_u, ffn, 0, ffn, 2));
        RCK(gemm_to_stream(e, s, y, e->p_u, ffn, L.w2, L.b2, ffn, true, L.lnog, L.lnob, 1e-12f));
    }
    set_prefilled(e);
    return 0;
}

// work-skipping for timing decompositions exists in measurement builds only: the product libraries cannot be told to
// return wrong answers faster
#ifdef GITMI_EXPERIMENT
#define GITMI_SKIPPED(e, bit) (((e)->pol.decode_skip & (bit)) != 0)
#else
#define GITMI_SKIPPED(e, bit) false
#endif
// ---- decode step ---------------------------------------------------------------------------------------
// bf16: the folded-LayerNorm GEMM chain of kernels_dgemm.hip, 5 launches per layer
//   QKV (LayerNorm of the previous layer folded) -> attention -> out-proj (+ residual, strip partials)
//   -> FFN1 (attention-output LayerNorm folded, erf-GELU) -> FFN2 (+ residual, strip partials)
// and, when the step feeds the search, the vocabulary head with the running top-M / log-sum-exp fused.
// f32 (parity mode): generic GEMM + LayerNorm launches, materialised logits, row_topm.
// Input: the embedded token rows in d_hf (fp32) / d_ht (compute dtype), written by embed_ln or by the previous
// search step.  logits_out != nullptr additionally materialises the logits [R, ldl] (teacher-forced parity hook).
static int dgemm(gitmi_engine* e, hipStream_t s, const DGemmArgs& g_in) {
    DGemmArgs g = g_in;
    g.dbg = e->pol.dgemm_dbg;
    // N = 768 GEMMs of the chain: 64 rows per workgroup (one pass over the weight strip, a quarter of the workgroups) for
    // beam batches -- faster even alone (R = 256: 0.466 -> 0.461 ms per step) -- and whenever other contexts share the
    // device: the launch is 2.8 us longer on its own but closes far fewer CUs to the encoder's GEMM workgroups
    // (profiles/r03_t_bench_lines.txt: greedy 10.34k -> 10.49k, beam-4 6.70k -> 7.00k captions/s in the mixed schedule)
    // wide GEMMs over > 64 rows (beam batches, decode groups): one workgroup per strip walks the row blocks with its weight
    // fragments in registers when other contexts share the device (beam-4: 7.18k -> 7.30k captions/s in the mixed schedule,
    // profiles/r03_zzz_ab_bench_lines.txt); alone, one workgroup per (strip, row block) is 3.5 us faster per launch
    g.no_row_walk = e->pol.dgemm_no_row_walk >= 0 ? e->pol.dgemm_no_row_walk : e->pol.shared_device ? 0 : 1;
    g.strips_per_wg = e->pol.dgemm_strips >= 0 ? e->pol.dgemm_strips : e->pol.shared_device ? 2 : 1;
    // rows per workgroup of the N = 768 chain GEMMs: 16 alone (48 strips x R/16 workgroups, shortest launch); next to other
    // contexts 32 -- half the workgroups for +1 us per launch.  Round 3 took 64 there (a quarter of the workgroups, +5 us:
    // +1.5 % captions/s with the kernels of the time); with the walking vocabulary head and the two-strip wide GEMMs in place
    // 32 gives the same throughput and a 7 % shorter decode step (profiles/r04_k_policy_components_bench_lines.txt:
    // 16 / 32 / 64 rows = 11.18k / 11.24k / 11.20k captions/s at 0.297 / 0.310 / 0.333 ms per step).  > 64 rows (beam
    // batches): 64, faster alone too.
    g.rows_per_wg = e->pol.dgemm_rows > 0 ? e->pol.dgemm_rows : g.M > 64 ? 64 : e->pol.shared_device ? 32 : 16;
    SpanGuard sp(e, s, TAG_GEMM_OTHER, gemm_flops(g.M, g.N, g.K));
    HIPCK(launch_dgemm(g, s));
    return 0;
}

// the chain's consumer (launchers.h: dgemm_ln / dgemm_to_stream, the pair of ln_gemm / gemm_to_stream on strip partials) of a folded set
static DGemmArgs dgemm_ln(const void* A, const Folded& f, const DLn* ln, void* C, int c_frag, int act, int M, int N, int K) {
    return dgemm_ln(A, f.w, f.bias, f.colsum, ln, C, c_frag, act, M, N, K);
}

static int decode_layers_impl(gitmi_engine* e, const int* kv_src, int ld_ids, int pos, int R, int beams, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    const int d = c.dec_hidden, ffn = c.dec_ffn;
    const int B = R / beams;
    const bool chain = e->pol.skinny && !e->pol.f32;
    for (int l = 0; l < c.dec_layers; ++l) {
        const DecLayerW& L = e->w.dec[l];
        // chain: ln_o, the previous layer's output LayerNorm over xo (layer 0: none, the embedded rows are normalised already),
        // and ln_a, this layer's attention-output LayerNorm over xa
        const DecLayerW* Lp = l > 0 ? &e->w.dec[l - 1] : nullptr;
        const DLn ln_prev{e->stats_o, d / 16, 1.0f / (float)d, 1e-12f, Lp ? Lp->lnog : nullptr, Lp ? Lp->lnob : nullptr};
        const DLn ln_a{e->stats_a, d / 16, 1.0f / (float)d, 1e-12f, L.lnag, L.lnab};
        const DLn* ln_o = Lp ? &ln_prev : nullptr;
        AttnDecodeArgs a{};
        a.qkv = e->d_qkv; a.img_k = e->img_kh[l]; a.img_v = e->img_vh[l]; a.txt_k = e->txt_k[l]; a.txt_v = e->txt_v[l]; a.out = e->d_ctx;
        a.kv_src = kv_src; a.ld_src = ld_ids; a.d = d; a.N_img = e->cur_Nimg; a.T_max = c.max_text_len;
        a.img_of = e->img_identity ? nullptr : e->img_of_dev;
        a.pos = pos; a.beams = beams; a.scale = 0.125f;
        a.out_frag = chain ? 1 : 0;
        a.N_pad = round_up(e->cur_Nimg, 32);
        a.dbg = e->pol.attn_dbg;
        a.waves_per_pair = e->pol.attn_nh;
        a.pairs_per_wg = e->pol.attn_pw > 0 ? e->pol.attn_pw : e->pol.shared_device ? 8 : 4;
        // a context that has the device to itself streams the image K/V through LDS rings (kernels_attn_decode.hip: all of a
        // pair's first 36 KiB requested at once, no second memory round trip): 11.7 instead of 15.6 us per launch on 192
        // workgroups.  Same arithmetic as the one-wave register kernel, every fused multiply-add written out in both, so the
        // two agree bit for bit and gitmi_set_shared_device stays bitwise neutral.  Next to other contexts the register kernel
        // packed 8 pairs per workgroup stays: a CU streams ~24 GB/s from HBM whatever the kernel form, and fewer workgroups
        // of the streaming kernel only stretch the launch (profiles/r04_f_*)
        const bool stream_ok = !e->pol.shared_device && a.N_pad <= 8 * 32 && B * c.dec_heads >= 384 && e->pol.attn_nh != 2;
        a.stream_wgs = e->pol.attn_stream >= 0 ? e->pol.attn_stream : stream_ok ? 192 : 0;
        if (e->keyed) { a.ntok = e->rg_ntok; a.stream_wgs = 0; }       // per-image key counts: the register kernels
        // QKV projection.  Where the policy packs the one-wave register kernel 8 pairs to a workgroup (greedy batches next to other
        // contexts), the attention launch computes its pairs' q | k | v itself (launch_attn_decode_qkv: the same values bit for
        // bit, kernels_attn_decode.hip): 26 launches per step instead of 32.  Everything else -- beam batches, keyed batches,
        // two-wave pairs, the streaming form of a context alone, f32 -- keeps the QKV launch.  Measurement builds: with any
        // GITMI_DECODE_SKIP bit set the step runs unfused, so bit 16 (the QKV launch alone left out) prices the path it bounds.
        bool qkv_inside = false;
        if (chain) {
            const DGemmArgs g = dgemm_ln(l == 0 ? e->d_ht : e->xo_b, L.qkv_f, ln_o, e->d_qkv, 0, 0, R, 3 * d, d);
            attn_decode_set_qkv(a, g);
            qkv_inside = !GITMI_SKIPPED(e, ~0) && !e->pol.dgemm_dbg && attn_decode_qkv_form(a, B, c.dec_heads) && attn_decode_pairs_per_wg(a, B, c.dec_heads) == 8;
            if (!qkv_inside && !GITMI_SKIPPED(e, 2) && !GITMI_SKIPPED(e, 16)) RCK(dgemm(e, s, g));
        } else {
            RCK(gemm(e, s, e->d_ht, d, L.wqkv, L.bqkv, nullptr, 0, e->d_qkv, 3 * d, e->pol.f32, R, 3 * d, d, 0, TAG_GEMM_OTHER));
        }
        if (e->pol.f32) HIPCK(launch_attn_decode(a, B, c.dec_heads, s));
        else if (qkv_inside) HIPCK(launch_attn_decode_qkv(a, B, c.dec_heads, s));
        else if (!GITMI_SKIPPED(e, 1)) HIPCK(launch_attn_decode_mfma(a, B, c.dec_heads, s));
        if (chain) {
            if (!GITMI_SKIPPED(e, 4))
                RCK(dgemm(e, s, dgemm_to_stream(e->d_ctx, L.wo_p, L.bo, l == 0 ? e->d_hf : e->xo_f, ln_o, e->xa_f, e->xa_b, e->stats_a, R, d, d)));
            if (!GITMI_SKIPPED(e, 2)) RCK(dgemm(e, s, dgemm_ln(e->xa_b, L.ffn1_f, &ln_a, e->d_u, 1, 2, R, ffn, d)));
            if (!GITMI_SKIPPED(e, 4))
                RCK(dgemm(e, s, dgemm_to_stream(e->d_u, L.w2_p, L.b2, e->xa_f, &ln_a, e->xo_f, e->xo_b, e->stats_o, R, d, ffn)));
        } else {
            RCK(dec_layer_tail(e, s, L, e->d_ctx, e->d_hf, e->d_ht, e->d_y, e->d_u, R));
        }
    }
    return 0;
}

static int sample_candidates(gitmi_engine* e, const float* logits, int ldl, int R, int step, hipStream_t s, StepCands* cands,
                             const BanArgs* ban);
static int trie_candidates(gitmi_engine* e, const float* logits, int ldl, int cur_len, hipStream_t s, StepCands* cands);
// repetition penalty of the current search (GENERATOR only; 0 and 1 both mean "off")
static float rep_penalty_of(const gitmi_engine* e) {
    const double rp = e->sample.repetition_penalty;
    return (e->ss.kind == GITMI_SEARCH_GENERATOR && rp > 0 && rp != 1.0) ? (float)rp : 0.f;
}

// decoding constraints of the search in progress (GITMI_SEARCH_CONSTRAIN): the engine's tables, or all null when it runs plain
static BanArgs ban_args(const gitmi_engine* e) {
    BanArgs b{};
    if (!e->ban_live || !e->ban_words) return b;
    const int mb = e->cfg.max_batch;
    b.W = (e->cfg.vocab + 31) / 32; b.eos = e->cfg.eos;
    const int* tab = reinterpret_cast<const int*>(e->ban_words + (size_t)mb * b.W);
    b.words = e->ban_words; b.set_of = tab; b.min_new = tab + mb; b.ngram = tab + 2 * mb;
    if (e->ban_seq_live) b.row_words = e->ban_row_words;
    return b;
}
// the banned sequences of the search in progress: the fixed regions of the engine's device table (engine_state.h)
static BanSeqArgs ban_seq_args(const gitmi_engine* e) {
    const int mb = e->cfg.max_batch;
    const int* t = e->ban_seq;
    return {t, t + mb, t + 2 * mb + 1, t + 2 * mb + 1 + BAN_SEQ_MAX_SEQS + 1};
}
static size_t ban_seq_ints(const gitmi_engine* e) { return (size_t)2 * e->cfg.max_batch + 1 + BAN_SEQ_MAX_SEQS + 1 + BAN_SEQ_MAX_TOKS; }

// per-token trace (GITMI_SEARCH_TRACE): the carving of trace_buf for a call of Q sentences returning nout sequences each, T
// positions, n alternatives -- byte offsets of the log (rows = Q x max_beams, whatever the beam count of the call), the
// hypotheses' side of it, and the engine's output copies (the graph outputs, copied to the caller's buffers after the launch)
struct TraceLayout { int rows; size_t log_lp, log_tok, hyp_src, fin_lp, fin_tok, out_lp, out_tok, lse, total; };
static TraceLayout trace_layout(const gitmi_engine* e, int Q, int nout, int T, int n) {
    TraceLayout L{};
    L.rows = Q * e->cfg.max_beams;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t recs = (size_t)T * L.rows, seqs = (size_t)Q * nout;
    L.log_lp = take(recs * (1 + n) * sizeof(float)); L.log_tok = take(recs * n * sizeof(int));
    L.hyp_src = take(seqs * T * sizeof(int));
    L.fin_lp = take(seqs * (1 + n) * sizeof(float)); L.fin_tok = take(seqs * n * sizeof(int));
    L.out_lp = take(seqs * T * (1 + n) * sizeof(float)); L.out_tok = take(seqs * T * n * sizeof(long long));
    L.lse = take((size_t)L.rows * sizeof(float2));          // row_topm_traced's scratch
    L.total = at;
    return L;
}
static TraceLayout trace_layout_live(const gitmi_engine* e) { return trace_layout(e, e->trace_Q, e->trace_nout, e->trace_T, e->trace_n); }
// the log of the search in progress, or all null when it is not traced
static TraceArgs trace_args(const gitmi_engine* e) {
    TraceArgs t{};
    if (!e->trace_live || !e->trace_buf) return t;
    const TraceLayout L = trace_layout_live(e);
    char* p = e->trace_buf;
    t.n = e->trace_n; t.rows = L.rows;
    t.log_lp = (float*)(p + L.log_lp); t.log_tok = (int*)(p + L.log_tok); t.hyp_src = (int*)(p + L.hyp_src);
    t.fin_lp = (float*)(p + L.fin_lp); t.fin_tok = (int*)(p + L.fin_tok);
    return t;
}
// candidates per row the head of a step lists: what the search reads, and the n alternatives of a traced search
static int search_mtop(const SearchState& st);
static int head_mtop(const gitmi_engine* e) { return std::max(search_mtop(e->ss), e->trace_live ? e->trace_n : 0); }
// The whole-row top-M of a step (f32 mode, step seam) of a TRACED search.  The instantiation that holds max(M, n) candidates per
// row sums the row's exp in another order than the one the plain call launches, so the step's (max, sum exp) -- and with it every
// log-prob the search adds -- comes from the launch the plain call makes, and the longer lists from a second launch whose
// statistics go to a scratch: the list values are the logits themselves either way, and traced == plain bit for bit.
static int row_topm_traced(gitmi_engine* e, const float* logits, int ldl, int V, const int* ids, int ld_ids, int cur_len, int beams,
                           int suppress_kind, int R, hipStream_t s, const BanArgs* ban) {
    const int Mp = search_mtop(e->ss), M = head_mtop(e);
    HIPCK(launch_row_topm(logits, ldl, V, ids, ld_ids, cur_len, e->plen_dev, beams, suppress_kind, rep_penalty_of(e), Mp, R, e->part_val,
                          e->part_idx, e->part_lse, s, ban));
    if (row_topm_slots(M) != row_topm_slots(Mp))
        HIPCK(launch_row_topm(logits, ldl, V, ids, ld_ids, cur_len, e->plen_dev, beams, suppress_kind, rep_penalty_of(e), M, R,
                              e->part_val, e->part_idx, (float2*)(e->trace_buf + trace_layout_live(e).lse), s, ban));
    return 0;
}
// behind launch_search_finish: the trace of the returned sequences into the engine's output copies
static int trace_gather(gitmi_engine* e, hipStream_t s) {
    const TraceLayout L = trace_layout_live(e);
    HIPCK(launch_search_trace_gather(e->ss, e->ss_cur, e->ss_len, trace_args(e), (float*)(e->trace_buf + L.out_lp),
                                     e->trace_n > 0 ? (long long*)(e->trace_buf + L.out_tok) : nullptr, s));
    return 0;
}
// the engine's output copies to the buffers of the arming call (device or page-locked host memory), like the ids of a graphed call
static int trace_deliver(gitmi_engine* e, hipStream_t s) {
    const TraceLayout L = trace_layout_live(e);
    const size_t elems = (size_t)e->trace_Q * e->trace_nout * e->trace_T;
    HIPCK(hipMemcpyAsync(e->trace_user_lp, e->trace_buf + L.out_lp, elems * (1 + e->trace_n) * sizeof(float), hipMemcpyDefault, s));
    if (e->trace_n > 0)
        HIPCK(hipMemcpyAsync(e->trace_user_tok, e->trace_buf + L.out_tok, elems * e->trace_n * sizeof(long long), hipMemcpyDefault, s));
    return 0;
}

// vocabulary head of the step: candidate lists for the search (and optionally the logits themselves)
static int decode_head_impl(gitmi_engine* e, const int* ids, int ld_ids, int cur_len, int R, int beams, int suppress_kind,
                            int M, float* logits_out, int ldl, hipStream_t s, StepCands* cands) {
    const gitmi_config& c = e->cfg;
    const int d = c.dec_hidden;
    const bool chain = e->pol.skinny && !e->pol.f32;
    cands->part_val = e->part_val; cands->part_idx = e->part_idx; cands->part_lse = e->part_lse;
    const bool sampling = ids != nullptr && e->ss.sampled;
    const bool trie = ids != nullptr && e->trie_search;
    if ((sampling || trie) && !logits_out) { logits_out = e->logits; ldl = e->ldl; }     // the filter / the trie need the whole row
    // Decoding constraints: every logit is banned exactly ONCE.  Chain: by the fused head -- the logits it stores already carry
    // the -10000, so the sampling filter that reads them gets no tables.  Otherwise the GEMM stores raw logits and the one
    // whole-row kernel that consumes them (row_topm or sample_rows) applies the ban.
    const BanArgs ban = ids ? ban_args(e) : BanArgs{};
    // banned sequences: the rows' own sets of this step, behind the search step that wrote position cur_len - 1 and reordered the
    // beams (same stream) and before whichever kernel below applies the ban
    if (ban.row_words) HIPCK(launch_ban_rows(ban, ban_seq_args(e), ids, ld_ids, cur_len, R, beams, e->ban_row_words, s));
    if (chain) {
        VocabArgs v{};
        v.A = (const unsigned short*)e->xo_b; v.lda = d; v.W = (const unsigned short*)e->w.out_f.w; v.bias = e->w.out_f.bias; v.colsum = e->w.out_f.colsum;
        v.stats_in = e->stats_o; v.strips_in = d / 16; v.inv_d = 1.0f / (float)d; v.eps_in = 1e-12f;
        v.M = R; v.N = c.vocab; v.K = d; v.cols_per_wg = e->vocab_cols;
        // workgroups of the head: by default one per column block (one HBM round trip; fastest alone); when other contexts
        // share the device, ~60 workgroups that each WALK four column blocks with a rolling weight refill -- the launch is
        // bound by the chip's HBM rate either way, and every CU that holds one of its waves is closed to the image encoder's
        // GEMM workgroups for the whole launch
        // (beam batches, R > 64 rows: one column block per workgroup in either policy -- the walking form re-reads the rows of
        // four row blocks per column block and takes 186 instead of 56 us, and the mix measures the same captions/s with either:
        // profiles/r05_m_beam_head_wgs_ab_bench_lines.txt; the shorter launch takes 0.17 ms off every beam step)
        v.max_wgs = e->pol.vocab_wgs >= 0 ? e->pol.vocab_wgs : (e->pol.shared_device && R <= 64) ? 60 : 0;
        v.ids = ids; v.ld_ids = ld_ids; v.cur_len = cur_len; v.plen = e->plen_dev; v.beams = beams; v.suppress_kind = suppress_kind;
        v.rep_penalty = ids ? rep_penalty_of(e) : 0.f;
        v.ban = ban;
        v.part_val = e->part_val; v.part_idx = e->part_idx; v.part_lse = e->part_lse;
        v.logits_out = logits_out; v.ld_logits = ldl;
        {
            SpanGuard sp(e, s, TAG_GEMM_OTHER, gemm_flops(R, c.vocab, d));
            if (!GITMI_SKIPPED(e, 8)) HIPCK(launch_vocab_topm(v, M, s, ids != nullptr && e->trace_live));
        }
        cands->nparts = e->vocab_nparts; cands->slots = vocab_mtop_slots(M);
        if (sampling) RCK(sample_candidates(e, logits_out, ldl, R, cur_len, s, cands, nullptr));
        if (trie) RCK(trie_candidates(e, logits_out, ldl, cur_len, s, cands));
    } else {
        RCK(gemm(e, s, e->d_ht, d, e->w.out_w, e->w.out_b, nullptr, 0, e->logits, e->ldl, true, R, c.vocab, d, 0, TAG_GEMM_OTHER));
        cands->nparts = 1; cands->slots = row_topm_slots(M);
        if (sampling) RCK(sample_candidates(e, e->logits, e->ldl, R, cur_len, s, cands, &ban));
        else if (trie) RCK(trie_candidates(e, e->logits, e->ldl, cur_len, s, cands));
        else if (ids && e->trace_live)
            RCK(row_topm_traced(e, e->logits, e->ldl, c.vocab, ids, ld_ids, cur_len, beams, suppress_kind, R, s, &ban));
        else if (ids)
            HIPCK(launch_row_topm(e->logits, e->ldl, c.vocab, ids, ld_ids, cur_len, e->plen_dev, beams, suppress_kind,
                                  rep_penalty_of(e), M, R,
                                  e->part_val, e->part_idx, e->part_lse, s, &ban));
        if (logits_out && logits_out != e->logits) HIPCK(launch_copy_f32(e->logits, e->ldl, logits_out, ldl, R, c.vocab, s));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
static int check_ready(gitmi_engine* e) {
    if (!e) return fail("null engine");
    if (!e->finalized) return fail("weights not finalized (call gitmi_finalize_weights)");
    HIPCK(hipSetDevice(e->device));
    return 0;
}

// ragged batches: frames[0] is the caller's descriptor + planes buffer (include/gitmi.h).  One launch validates every entry
// on the device and copies the valid images into fixed slots of frame_stage[0], outside any captured graph: the encoder
// then reads the slots and the per-image meta, so one graph (keyed on the capacity) serves every mix of shapes.
static int ragged_prepare(gitmi_engine* e, const float* const* frames, int F, int B, hipStream_t s) {
    if (!e->ragged) return 0;
    if (F != 1 || !frames[0]) return fail("ragged input (gitmi_set_image_shape(e, 0, 0)): F must be 1, frames[0] the descriptor buffer");
    drop_resident(e);           // rg_meta / rg_ntok of the resident batch are overwritten
    HIPCK(launch_ragged_stage(frames[0], e->frame_stage[0], (size_t)3 * e->max_pixels, e->rg_meta, e->rg_ntok, B, e->cfg.patch,
                              e->max_pixels, e->Nmax, s));
    return 0;
}

// the input checks every entry point that encodes images shares; `who` names it in the error text
static int check_frames(const gitmi_engine* e, const char* who, const float* const* frames, int F, int B) {
    if (!frames || F < 1 || F > e->cfg.max_frames) return fail("%s: F=%d outside [1,%d]", who, F, e->cfg.max_frames);
    if (B < 1 || B > e->cfg.max_batch) return fail("%s: B=%d outside [1,%d]", who, B, e->cfg.max_batch);
    return 0;
}

// follow-up calls (frames == NULL, include/gitmi.h): the images of the engine's last encode, `B` of them
static int check_resident(const gitmi_engine* e, const char* who, int B) {
    if (!e->have_feats)
        return fail("%s: frames == NULL is a follow-up call, but the engine holds no resident images (encode some with a call "
                    "that takes frames; a change of the image shape or mode, of the temporal embedding or of the LayerNorm "
                    "folding, and a failed call, drop them)", who);
    if (B != e->cur_B) return fail("%s: follow-up call with B=%d, but %d images are resident (B must equal that count)", who, B, e->cur_B);
    return 0;
}

extern "C" int gitmi_encode_frames(gitmi_engine* e, const float* const* frames, int F, int B, float* feats_out,
                                   void* stream) {
    RCK(check_ready(e));
    RCK(check_frames(e, "encode_frames", frames, F, B));
    RCK(ragged_prepare(e, frames, F, B, (hipStream_t)stream));
    return encode_frames_impl(e, frames, F, B, feats_out, (hipStream_t)stream);
}

static EmbedArgs embed_args(gitmi_engine* e, bool on) {
    EmbedArgs em{};
    if (!on) return em;
    em.words = e->w.words_f; em.positions = e->w.positions_f; em.gamma = e->w.emb_lng; em.beta = e->w.emb_lnb; em.eps = 1e-8f;
    em.h_f = e->d_hf; em.h_t = e->d_ht; em.D = e->cfg.dec_hidden; em.vocab = e->cfg.vocab;
    em.frag = (e->pol.skinny && !e->pol.f32) ? 1 : 0;
    return em;
}
// embeds position `pos` of the R token rows ids [R][ld_ids] into d_hf / d_ht (every later position: the search step's fused embedding)
static int embed_position(gitmi_engine* e, const int* ids, int ld_ids, int pos, int R, hipStream_t s) {
    const EmbedArgs em = embed_args(e, true);
    HIPCK(launch_embed_ln(ids, ld_ids, pos, em.words, em.positions, em.gamma, em.beta, em.eps, em.h_f, em.h_t, e->pol.f32, R, em.D,
                          em.vocab, em.frag != 0, s));
    return 0;
}

extern "C" int gitmi_prefill(gitmi_engine* e, void* stream) {
    RCK(check_ready(e));
    if (!e->have_feats) return fail("prefill: no encoded frames");
    return prefill_impl(e, (hipStream_t)stream);
}

extern "C" int gitmi_step_logits(gitmi_engine* e, const int64_t* tokens, int R, int t, float* logits_out, void* stream) {
    RCK(check_ready(e));
    if (!e->have_feats) return fail("step_logits: no encoded frames");
    hipStream_t s = (hipStream_t)stream;
    if (!e->have_prefill) RCK(prefill_impl(e, s));
    const int B = e->cur_B;
    if (R < B || R % B) return fail("step_logits: R=%d is not a multiple of the encoded batch %d", R, B);
    const int beams = R / B;
    if (beams > e->cfg.max_beams) return fail("step_logits: %d beams exceed max_beams", beams);
    if (t < 1 || t > e->cfg.max_text_len) return fail("step_logits: t=%d outside [1,%d]", t, e->cfg.max_text_len);
    const gitmi_config& c = e->cfg;
    const int T = c.max_text_len;
    e->img_identity = true;
    HIPCK(launch_load_ids((const long long*)tokens, R, t, e->ss.ids[0], e->ss.kv_src[0], T, s));
    // note: load_ids writes rows of length ld = T_max
    StepCands cands{};
    for (int pos = 0; pos < t; ++pos) {
        SpanGuard step(e, s, TAG_STEP, 0);
        RCK(embed_position(e, e->ss.ids[0], T, pos, R, s));
        RCK(decode_layers_impl(e, e->ss.kv_src[0], T, pos, R, beams, s));
        if (pos == t - 1) RCK(decode_head_impl(e, nullptr, T, t, R, beams, 0, 1, logits_out, c.vocab, s, &cands));
    }
    return 0;
}

// ---- search seam -----------------------------------------------------------------------
// `start_dev` / `plen_dev` (/ `img_of_dev`) must already describe the rq.Q sentences of the call (of rq, the search and
// the sentence counts are read; V: the vocabulary the search ranks)
static int search_begin_impl(gitmi_engine* e, const Request& rq, int V, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    const gitmi_search* sp = rq.sp;
    const int B = rq.Q, minP = rq.minP, maxP = rq.maxP;
    if (!sp) return fail("search: null config");
    if (sp->kind != GITMI_SEARCH_AUTOREGRESSIVE && sp->kind != GITMI_SEARCH_GENERATOR && sp->kind != GITMI_SEARCH_TRIE)
        return fail("search: bad kind");
    if (sp->kind == GITMI_SEARCH_TRIE) {
        if (sp->beam_size != 1) return fail("search: TrieAutoRegressiveBeamSearch asserts beam_size == 1 (trie_decoder.py:37)");
        if (!e->trie_off) return fail("search: no trie loaded (gitmi_set_trie)");
        if (sp->do_sample) return fail("search: the trie search has no sampling branch");
    }
    if (B < 1 || B > c.max_batch) return fail("search: B=%d outside [1,%d]", B, c.max_batch);
    if (sp->beam_size < 1 || sp->beam_size > c.max_beams) return fail("search: beam_size %d outside [1,%d]", sp->beam_size, c.max_beams);
    if (sp->per_node_beam_size < 1 && sp->kind != GITMI_SEARCH_TRIE) return fail("search: per_node_beam_size must be >= 1");
    if (sp->kind == GITMI_SEARCH_GENERATOR && sp->per_node_beam_size < 2)
        return fail("search: GeneratorWithBeamSearch requires per_node_beam_size > 1 (decoder.py:1078)");
    if (sp->beam_size * sp->per_node_beam_size > 16) return fail("search: beam_size*per_node_beam_size > 16 unsupported");
    if (sp->max_steps > c.max_text_len) return fail("search: max_steps %d exceeds max_text_len %d", sp->max_steps, c.max_text_len);
    if (minP < 1 || maxP > sp->max_steps) return fail("search: prefix lengths [%d,%d] outside [1,max_steps]", minP, maxP);
    if (sp->kind == GITMI_SEARCH_GENERATOR && !(sp->length_penalty > 0)) return fail("search: length_penalty must be > 0");
    if (sp->repetition_penalty != 0 && sp->repetition_penalty != 1.0) {
        if (sp->kind != GITMI_SEARCH_GENERATOR) return fail("search: repetition_penalty belongs to GeneratorWithBeamSearch (decoder.py:1064)");
        if (!(sp->repetition_penalty >= 1.0)) return fail("search: `repetition_penalty` should be >= 1 (decoder.py:1080)");
        if (sp->max_steps > 1024) return fail("search: repetition_penalty supports histories up to 1024 tokens");
    }
    if (sp->num_keep_best < 0 || sp->num_keep_best > SS_NHMAX) return fail("search: num_keep_best %d outside [1,%d]", sp->num_keep_best, SS_NHMAX);
    if (sp->num_keep_best > 1 && sp->kind != GITMI_SEARCH_GENERATOR)
        return fail("search: num_keep_best belongs to GeneratorWithBeamSearch.search (decoder.py:1087)");
    if (sp->do_sample) {
        if (sp->kind != GITMI_SEARCH_GENERATOR) return fail("search: do_sample is implemented for GeneratorWithBeamSearch (decoder.py:1146-1166) only");
        if (sp->temperature < 0) return fail("search: temperature must be > 0");
        if (V > 32768) return fail("search: sampling supports vocabularies up to 32768 tokens");
    }
    SearchState& st = e->ss;
    e->trie_search = sp->kind == GITMI_SEARCH_TRIE;
    st.B = B; st.k = sp->beam_size; st.pn = e->trie_search ? 1 : sp->per_node_beam_size;
    st.T = sp->max_steps;           // max_length of the search AND the row stride of ids/kv_src/hyp_tok
    // the trie search shares AutoRegressiveBeamSearch's bookkeeping (beam 1): only the candidate selection differs
    st.V = V; st.eos = c.eos; st.kind = e->trie_search ? GITMI_SEARCH_AUTOREGRESSIVE : sp->kind; st.length_penalty = sp->length_penalty;
    st.prefixed = rq.prefixed ? 1 : 0;
    st.nh = keep_best(*sp);
    st.sampled = sp->do_sample ? 1 : 0;
    e->sample = *sp;
    st.start = e->start_dev; st.ld_start = c.max_text_len; st.plen = e->plen_dev;
    e->ss_cur = 0; e->ss_len = minP;
    HIPCK(launch_search_init(st, s));
    if (e->trie_search) HIPCK(launch_fill_i32(e->trie_cursor, 0, B, s));      // TokenTrie.reset(): every cursor at the root
    return 0;
}

static int trace_check(const gitmi_engine* e, const char* who, const gitmi_search* sp, int Q, bool* traced);
static int search_mtop(const SearchState& st) {
    if (st.sampled) return st.pn;
    return st.kind == GITMI_SEARCH_AUTOREGRESSIVE ? std::max(st.k, st.pn) : st.pn * st.k;
}
// sampling branch: filter + draws from the materialised logits of the step (decoder.py:1146-1166)
static int sample_candidates(gitmi_engine* e, const float* logits, int ldl, int R, int step, hipStream_t s, StepCands* cands,
                             const BanArgs* ban) {
    const gitmi_search& sp = e->sample;
    const float temp = sp.temperature > 0 ? (float)sp.temperature : 1.0f;
    HIPCK(launch_sample_rows(logits, ldl, e->ss.V, R, temp, sp.top_k, (float)sp.top_p, e->ss.pn, sp.seed, step,
                             e->part_val, e->part_idx, e->part_lse, nullptr, e->ss.ids[e->ss_cur], e->ss.T, step,
                             rep_penalty_of(e), row_topm_slots(e->ss.pn), s, ban, e->plen_dev, e->ss.k));
    cands->part_val = e->part_val; cands->part_idx = e->part_idx; cands->part_lse = e->part_lse;
    cands->nparts = 1; cands->slots = row_topm_slots(e->ss.pn);
    return 0;
}

// trie-constrained selection on the materialised logits of the step (trie_decoder.py:57-71, 115-158)
static int trie_candidates(gitmi_engine* e, const float* logits, int ldl, int cur_len, hipStream_t s, StepCands* cands) {
    const SearchState& st = e->ss;
    TrieArgs tr{e->trie_off, e->trie_tok, e->trie_child, e->trie_cursor};
    HIPCK(launch_trie_select(logits, ldl, st.V, st.ids[e->ss_cur], st.T, cur_len, e->plen_dev, st.eos, tr, st.B, e->part_val,
                             e->part_idx, e->part_lse, s));
    cands->part_val = e->part_val; cands->part_idx = e->part_idx; cands->part_lse = e->part_lse;
    cands->nparts = 1; cands->slots = 1;
    return 0;
}

// one search step on the candidate lists of the current step (+ the embedding of the appended tokens)
static int search_step_impl(gitmi_engine* e, const StepCands& cands, bool embed, hipStream_t s) {
    const SearchState& st = e->ss;
    const int cur_len = e->ss_len;
    if (cur_len >= st.T) return fail("search_advance: sequence already at max_steps");
    const TraceArgs tr = trace_args(e);
    HIPCK(launch_search_step(st, e->ss_cur, cur_len, cands, embed_args(e, embed), e->pol.f32, s, tr.log_lp ? &tr : nullptr));
    e->ss_cur ^= 1;
    e->ss_len = cur_len + 1;
    return 0;
}

static int fill_uniform_sentences(gitmi_engine* e, int B, const long long* prefix_dev, int P, hipStream_t s) {
    HIPCK(launch_fill_start(e->start_dev, e->cfg.max_text_len, prefix_dev, 0, 1, e->cfg.sos, B, P, s));
    HIPCK(launch_fill_i32(e->plen_dev, P, B, s));
    e->img_identity = true;
    return 0;
}

// Token trie for GITMI_SEARCH_TRIE (trie_decoder.py:224-257 TokenTrie as CSR): node 0 is the root, the children of node n
// are the edges child_off[n] .. child_off[n + 1] - 1 (token child_tok[e] leads to node child_node[e]).  Host arrays, copied.
// n_nodes == 0 removes the trie.
extern "C" int gitmi_set_trie(gitmi_engine* e, int n_nodes, const int32_t* child_off, const int32_t* child_tok,
                              const int32_t* child_node) {
    RCK(check_ready(e));
    HIPCK(hipDeviceSynchronize());
    destroy_graph(e);                                       // captured launches hold the old pointers
    // the new arrays are built completely before the old ones go: a failed allocation or copy leaves the engine with the
    // trie it had (all three arrays or none), never with offsets that point into freed edge arrays
    int *n_off = nullptr, *n_tok = nullptr, *n_child = nullptr;
    if (n_nodes > 0) {
        if (!child_off || child_off[0] != 0) return fail("set_trie: child_off must start at 0");
        const int n_edges = child_off[n_nodes];
        for (int n = 0; n < n_nodes; ++n)
            if (child_off[n + 1] < child_off[n]) return fail("set_trie: child_off must be non-decreasing");
        if (n_edges > 0 && (!child_tok || !child_node)) return fail("set_trie: null edge arrays");
        for (int i = 0; i < n_edges; ++i)
            if (child_node[i] < 0 || child_node[i] >= n_nodes) return fail("set_trie: edge %d leads to node %d of %d", i, child_node[i], n_nodes);
        hipError_t err = hipMalloc((void**)&n_off, (size_t)(n_nodes + 1) * sizeof(int));
        if (err == hipSuccess) err = hipMalloc((void**)&n_tok, (size_t)std::max(n_edges, 1) * sizeof(int));
        if (err == hipSuccess) err = hipMalloc((void**)&n_child, (size_t)std::max(n_edges, 1) * sizeof(int));
        if (err == hipSuccess) err = hipMemcpy(n_off, child_off, (size_t)(n_nodes + 1) * sizeof(int), hipMemcpyHostToDevice);
        if (err == hipSuccess && n_edges > 0) err = hipMemcpy(n_tok, child_tok, (size_t)n_edges * sizeof(int), hipMemcpyHostToDevice);
        if (err == hipSuccess && n_edges > 0) err = hipMemcpy(n_child, child_node, (size_t)n_edges * sizeof(int), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            if (n_off) hipFree(n_off);
            if (n_tok) hipFree(n_tok);
            if (n_child) hipFree(n_child);
            return fail("set_trie: %s (the previous trie is kept)", hipGetErrorString(err));
        }
    }
    if (e->trie_off) { hipFree(e->trie_off); hipFree(e->trie_tok); hipFree(e->trie_child); }
    e->trie_off = n_off; e->trie_tok = n_tok; e->trie_child = n_child;
    return 0;
}

// start_host int64 [B][ld] and the prefix lengths (plen_host int32 [B], or NULL: all `ld`) -> the engine's start / plen tables,
// then search_begin_impl.  `who` names the entry point in the error text.
static int search_begin_host(gitmi_engine* e, const char* who, const gitmi_search* sp, int B, const int64_t* start_host, int ld,
                             const int32_t* plen_host, int vocab, void* stream) {
    RCK(check_ready(e));
    if (!start_host) return fail("%s: null start", who);
    if (B < 1 || B > e->cfg.max_batch || ld < 1 || ld > e->cfg.max_text_len) return fail("%s: bad B/P", who);
    if (vocab < 2) return fail("%s: bad vocab", who);
    if (sp && sp->kind == GITMI_SEARCH_SCORE) return fail("%s: GITMI_SEARCH_SCORE is not a search (gitmi_generate_prefixed scores sentences)", who);
    if (sp && sp->kind == GITMI_SEARCH_ATTEND) return fail("%s: GITMI_SEARCH_ATTEND is not a search (gitmi_generate_prefixed returns the attention maps of sentences)", who);
    if (sp && sp->kind == GITMI_SEARCH_CONTEXT) return fail("%s: GITMI_SEARCH_CONTEXT is not a search (gitmi_generate_prefixed puts context tokens into the decoder memory)", who);
    if (sp && sp->kind == GITMI_SEARCH_TREE_SCORE) return fail("%s: GITMI_SEARCH_TREE_SCORE is not a search (gitmi_generate_prefixed scores token trees)", who);
    if (sp && sp->kind == GITMI_SEARCH_KEEP) return fail("%s: GITMI_SEARCH_KEEP is not a search (gitmi_generate_prefixed keeps the memory of resident images)", who);
    if (sp && sp->kind == GITMI_SEARCH_RECALL) return fail("%s: GITMI_SEARCH_RECALL is not a search (gitmi_generate_prefixed recalls kept images)", who);
    if (sp && sp->kind == GITMI_SEARCH_FEATURES) return fail("%s: GITMI_SEARCH_FEATURES is not a search (gitmi_generate_prefixed installs given feature rows)", who);
    if (sp && sp->kind == GITMI_SEARCH_CONSTRAIN) return fail("%s: GITMI_SEARCH_CONSTRAIN is not a search (gitmi_generate_prefixed arms the constraints of the next search call)", who);
    if (sp && sp->kind == GITMI_SEARCH_TRACE) return fail("%s: search->kind GITMI_SEARCH_TRACE is not a search (gitmi_generate_prefixed arms the per-token trace of the next search call)", who);
    if (e->ban_armed)
        return fail("%s: decoding constraints are armed for %d sentences (GITMI_SEARCH_CONSTRAIN): the seam's caller owns its logits and "
                    "applies its own -- disarm first (a GITMI_SEARCH_CONSTRAIN call with Q == 0)", who, e->ban_armed);
    e->ban_live = e->ban_seq_live = false;
    bool traced = false;
    if (sp) RCK(trace_check(e, who, sp, B, &traced));
    e->trace_live = false;
    int minP = ld, maxP = ld;
    if (plen_host) {
        maxP = 1;
        for (int b = 0; b < B; ++b) {
            if (plen_host[b] < 1 || plen_host[b] > ld) return fail("%s: prefix length %d of sentence %d outside [1,%d]", who, plen_host[b], b, ld);
            minP = std::min(minP, (int)plen_host[b]); maxP = std::max(maxP, (int)plen_host[b]);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    // one row per sentence, written into the engine's [B, max_text_len] start table
    HIPCK(hipMemcpy2DAsync(e->start_dev, (size_t)e->cfg.max_text_len * sizeof(long long), start_host,
                           (size_t)ld * sizeof(long long), (size_t)ld * sizeof(long long), (size_t)B, hipMemcpyHostToDevice, s));
    if (plen_host) HIPCK(hipMemcpyAsync(e->plen_dev, plen_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCK(hipStreamSynchronize(s));
    if (!plen_host) HIPCK(launch_fill_i32(e->plen_dev, ld, B, s));
    e->img_identity = true;
    Request rq{};
    rq.Q = B; rq.minP = minP; rq.maxP = maxP; rq.prefixed = plen_host != nullptr; rq.sp = sp;
    RCK(search_begin_impl(e, rq, vocab, s));
    // the seam search consumes an armed trace under the kind of the search it starts; gitmi_search_finish fills the buffers
    if (traced) { e->trace_armed = 0; e->trace_live = true; }
    return 0;
}

extern "C" int gitmi_search_begin(gitmi_engine* e, const gitmi_search* sp, int B, const int64_t* start_host, int P,
                                  int vocab, void* stream) {
    return search_begin_host(e, "search_begin", sp, B, start_host, P, nullptr, vocab, stream);
}

extern "C" int gitmi_search_rows(gitmi_engine* e, int64_t* tokens_out, int* R, int* t, void* stream) {
    RCK(check_ready(e));
    const SearchState& st = e->ss;
    if (R) *R = st.B * st.k;
    if (t) *t = e->ss_len;
    if (tokens_out) HIPCK(launch_search_rows(st, e->ss_cur, e->ss_len, (long long*)tokens_out, (hipStream_t)stream));
    return 0;
}

extern "C" int gitmi_search_advance(gitmi_engine* e, const float* logits, void* stream) {
    RCK(check_ready(e));
    if (!logits) return fail("search_advance: null logits");
    const SearchState& st = e->ss;
    hipStream_t s = (hipStream_t)stream;
    const int M = head_mtop(e), R = st.B * st.k;
    StepCands cands{e->part_val, e->part_idx, e->part_lse, 1, row_topm_slots(M)};
    if (st.sampled) RCK(sample_candidates(e, logits, st.V, R, e->ss_len, s, &cands, nullptr));
    else if (e->trie_search) RCK(trie_candidates(e, logits, st.V, e->ss_len, s, &cands));
    else if (e->trace_live)
        RCK(row_topm_traced(e, logits, st.V, st.V, st.ids[e->ss_cur], st.T, e->ss_len, st.k,
                            st.kind == GITMI_SEARCH_AUTOREGRESSIVE ? 1 : 0, R, s, nullptr));
    else
        HIPCK(launch_row_topm(logits, st.V, st.V, st.ids[e->ss_cur], st.T, e->ss_len, e->plen_dev, st.k,
                              st.kind == GITMI_SEARCH_AUTOREGRESSIVE ? 1 : 0, rep_penalty_of(e), M, R, e->part_val,
                              e->part_idx, e->part_lse, s));
    return search_step_impl(e, cands, false, s);
}

extern "C" int gitmi_search_done_count(gitmi_engine* e, int* done_out, void* stream) {
    RCK(check_ready(e));
    if (!done_out) return fail("search_done_count: null argument");
    int h = 0;
    HIPCK(hipMemcpyAsync(&h, e->ss.info, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCK(hipStreamSynchronize((hipStream_t)stream));
    *done_out = h;
    return 0;
}

extern "C" int gitmi_search_finish(gitmi_engine* e, int64_t* tokens_out, float* logprob_out, int32_t* info_out,
                                   void* stream) {
    RCK(check_ready(e));
    const SearchState& st = e->ss;
    HIPCK(launch_search_finish(st, e->ss_cur, e->ss_len, (long long*)tokens_out, logprob_out, info_out, nullptr,
                               (hipStream_t)stream));
    if (e->trace_live) {
        RCK(trace_gather(e, (hipStream_t)stream));
        RCK(trace_deliver(e, (hipStream_t)stream));
        e->trace_live = false;          // delivered: a second finish returns the ids alone, and the context may be armed again
    }
    return 0;
}

// ---- op hooks of the search step (measurement build; tests/test_gpu_search_ops.py) -------------------------------------------
// gitmi_search_begin with a prefix of its own length per sentence: start_host int64 [B][ld], plen_host int32 [B] (1 .. ld).
// Every sentence then stands for its own batch-1 reference call, as in gitmi_generate_prefixed; the search starts at the
// shortest prefix length and appends the given tokens to the longer ones until their prefix ends.
GITMI_EXP_EXPORT int gitmi_debug_search_begin_prefixed(gitmi_engine* e, const gitmi_search* sp, int B, const int64_t* start_host,
                                                       int ld, const int32_t* plen_host, int vocab, void* stream) {
    if (!plen_host) return fail("debug_search_begin_prefixed: null prefix lengths");
    return search_begin_host(e, "debug_search_begin_prefixed", sp, B, start_host, ld, plen_host, vocab, stream);
}
// gitmi_search_advance on caller-supplied candidate lists (DEVICE; the format of the fused vocabulary head: part_val / part_idx
// [R][nparts][slots] sorted, unused entries (-inf, 0x7fffffff); part_lse [R][nparts] (max, sum exp)) in place of the row_topm
// launch: the multi-part merge of search_step_kernel.  embed != 0: the step also embeds the appended tokens (engine weights).
GITMI_EXP_EXPORT int gitmi_debug_search_advance_lists(gitmi_engine* e, const float* part_val, const int* part_idx,
                                                      const float* part_lse, int nparts, int slots, int embed, void* stream) {
    RCK(check_ready(e));
    if (!part_val || !part_idx || !part_lse) return fail("debug_search_advance_lists: null argument");
    const SearchState& st = e->ss;
    if (st.B < 1 || st.T < 1) return fail("debug_search_advance_lists: no search has begun");
    if (st.sampled || e->trie_search) return fail("debug_search_advance_lists: the sampling and trie searches select from whole logit rows");
    if (nparts < 1 || nparts > 256) return fail("debug_search_advance_lists: nparts=%d outside [1,256]", nparts);
    if (slots != 1 && slots != 2 && slots != 4 && slots != 8 && slots != 16)
        return fail("debug_search_advance_lists: slots=%d is not one of 1, 2, 4, 8, 16", slots);
    if (slots < head_mtop(e))
        return fail("debug_search_advance_lists: slots=%d, but the step reads %d candidates per row (the search's, or the n alternatives "
                    "of its trace)", slots, head_mtop(e));
    const StepCands cands{part_val, part_idx, (const float2*)part_lse, nparts, slots};
    return search_step_impl(e, cands, embed != 0, (hipStream_t)stream);
}
// the embedded rows of the most recent step (embed_ln / the search step's fused embedding): hf_out fp32 [R][D]; ht_out
// round_up(R, 16) * D elements of the engine's compute type exactly as stored, *ht_frag = 1 when that is the fragment-major
// operand layout (gitmi_common.h frag_offset; the caller undoes it), *ht_dtype its GITMI_DTYPE_* code.  Synchronises.
GITMI_EXP_EXPORT int gitmi_debug_read_hidden(gitmi_engine* e, int R, float* hf_out, void* ht_out, int* ht_frag, int* ht_dtype,
                                             void* stream) {
    RCK(check_ready(e));
    const gitmi_config& c = e->cfg;
    if (R < 1 || R > c.max_batch * c.max_beams) return fail("debug_read_hidden: R=%d outside the capacity", R);
    if (!hf_out || !ht_out || !ht_frag || !ht_dtype) return fail("debug_read_hidden: null argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t D = (size_t)c.dec_hidden, Rp = (size_t)(R + 15) / 16 * 16;
    HIPCK(hipMemcpyAsync(hf_out, e->d_hf, (size_t)R * D * sizeof(float), hipMemcpyDefault, s));
    HIPCK(hipMemcpyAsync(ht_out, e->d_ht, Rp * D * e->pol.esz, hipMemcpyDefault, s));
    HIPCK(hipStreamSynchronize(s));
    *ht_frag = (e->pol.skinny && !e->pol.f32) ? 1 : 0;
    *ht_dtype = e->pol.f32 ? GITMI_DTYPE_F32 : gitmi_operand_dtype();
    return 0;
}

// ---- the whole hot path ------------------------------------------------------------------
// image encoder + decoder prefill over the image tokens
static int generate_encode(gitmi_engine* e, const Request& rq, hipStream_t s) {
    RCK(encode_frames_impl(e, rq.frames, rq.F, rq.B, nullptr, s));
    return prefill_impl(e, s);
}
// the image K/V a call runs over: encode + prefill of its frames; a follow-up call: the resident images' prefill if it is not current
static int images_ready(gitmi_engine* e, const Request& rq, hipStream_t s) {
    if (rq.frames) return generate_encode(e, rq, s);
    return e->have_prefill ? 0 : prefill_impl(e, s);
}

// search over the text positions (teacher-forced prefix positions, then searched ones) + result formatting.
// rq.Q sentences (start_dev / plen_dev / img_of_dev describe them), prefix lengths in [minP, maxP].
static int generate_decode(gitmi_engine* e, const Request& rq, hipStream_t s, bool allow_poll) {
    const gitmi_config& c = e->cfg;
    const gitmi_search* sp = rq.sp;
    RCK(search_begin_impl(e, rq, c.vocab, s));
    const int Q = rq.Q, minP = rq.minP, maxP = rq.maxP, T = sp->max_steps, k = sp->beam_size, R = Q * k;
    const SearchState& st = e->ss;
    const int M = head_mtop(e);
    const int suppress = sp->kind != GITMI_SEARCH_GENERATOR ? 1 : 0;
    {
        SpanGuard phase(e, s, TAG_DECODE, 0);
        // position 0 is embedded here; every later position by the search step that appends its token
        RCK(embed_position(e, st.ids[0], T, 0, R, s));
        e->ss_len = 1;
        // Steps below minP only append given tokens and read no list.  A traced step still checks that its lists hold n
        // alternatives, so the shape the head will give them stands from the first step on.
        const bool chain = e->pol.skinny && !e->pol.f32;
        StepCands cands{e->part_val, e->part_idx, e->part_lse, 1, e->trace_live ? (chain ? vocab_mtop_slots(M) : row_topm_slots(M)) : 1};
        while (e->ss_len < T) {
            const int cur_len = e->ss_len;
            SpanGuard step(e, s, TAG_STEP, 0);
            RCK(decode_layers_impl(e, st.kv_src[e->ss_cur], T, cur_len - 1, R, k, s));
            // steps that only append given prefix tokens to every sentence (VQA question tokens) need no logits
            if (cur_len >= minP)
                RCK(decode_head_impl(e, st.ids[e->ss_cur], T, cur_len, R, k, suppress, M, nullptr, 0, s, &cands));
            RCK(search_step_impl(e, cands, true, s));
            // long step budgets (the shipped default is max_steps=1024, model.py:37): every 8 steps read
            // the device-side count of finished sentences so the loop ends like decoder.py:319 / :1251.
            // Extra steps past that point are idempotent, so polling sparsely is exact.
            if (allow_poll && e->ss_len > maxP && (e->ss_len - maxP) % 8 == 0 && e->ss_len < T) {
                int h[4];
                HIPCK(hipMemcpyAsync(h, st.info, sizeof(h), hipMemcpyDeviceToHost, s));
                HIPCK(hipStreamSynchronize(s));
                if (h[0] >= Q) break;
            }
        }
    }
    HIPCK(launch_search_finish(st, e->ss_cur, e->ss_len, rq.tokens, rq.logprob, rq.info, rq.sent, s));
    if (e->trace_live) RCK(trace_gather(e, s));
    if (e->ragged)      // sentences over a rejected image: NaN log-probs, counted with the non-finite ones (info[3])
        HIPCK(launch_ragged_report(e->rg_meta, e->img_identity ? nullptr : e->img_of_dev, Q, keep_best(*sp), rq.logprob, rq.info,
                                   nullptr, s));
    // algorithmic bytes of one decode step: all decoder weights once +
    // per sentence the K/V of every layer (image part shared by beams, text part per beam)
    const double kv = (double)Q * c.dec_layers * 2.0 * ((double)e->cur_Nimg + k * 0.5 * (minP + T)) * c.dec_hidden * e->pol.esz;
    e->last_decode_step_bytes = e->w.dec_weight_bytes + kv;
    return 0;
}

// the whole call: the image K/V, then the search
static int generate_body(gitmi_engine* e, const Request& rq, hipStream_t s, bool allow_poll) {
    SpanGuard total(e, s, 99, 0);
    RCK(images_ready(e, rq, s));
    return generate_decode(e, rq, s, allow_poll);
}

// hipGraph cache key of a call: everything the captured launch sequence depends on
static GraphKey graph_key_of(const gitmi_engine* e, const Request& rq, int F_eff) {
    const gitmi_search& sp = *rq.sp;
    // a follow-up call runs over the memory as it stands: the row stride of an image's block is an argument of every attention
    // launch, and so is whether key counts are read (their values live in rg_ntok, whose pointer never changes)
    const bool resident = rq.frames == nullptr;
    return {rq.B, rq.Q, F_eff, rq.minP, sp.kind, sp.beam_size, sp.per_node_beam_size, sp.max_steps, e->H, e->W,
            rq.prefixed ? 1 : 0, e->img_identity ? 1 : 0, e->pol.use_temb ? 1 : 0, resident ? 1 : 0,
            resident ? e->cur_Nimg : 0, resident && e->keyed ? 1 : 0, sp.length_penalty,
            sp.do_sample, sp.top_k, keep_best(sp), sp.top_p, sp.temperature, sp.repetition_penalty, sp.seed, e->ban_live ? (e->ban_seq_live ? 2 : 1) : 0,
            e->trace_live ? 1 + e->trace_n : 0};
}

// Launches the graphs of one call on `x`: `enc` (the whole call, or encode + prefill; nullptr in a follow-up), then `dec`
// (the decode part; nullptr when `enc` is the whole call).  Between the two graphs of a split full call the serving schedule
// has its say: the call waits for enc_after's encoder before `enc` and records enc_done after it for its watchers.  A
// follow-up runs no encoder, so it neither waits nor records (watchers keep waiting for the most recent real encoder).
// profile_mode 2 takes the place of the schedule: events around each graph, a synchronisation, the split_* sums; a
// follow-up's graph is timed as the decode graph of a full call and adds nothing to the encode side.
static int replay(gitmi_engine* e, const Request& rq, hipStream_t x, const CapturedGraph* enc, const CapturedGraph* dec) {
    const bool timed = e->profile_mode == 2;
    if (timed) {
        for (auto& ev : e->gev)
            if (!ev) HIPCK(hipEventCreate(&ev));
        HIPCK(hipEventRecord(e->gev[enc ? 0 : 1], x));
    } else if (enc && e->enc_after && e->enc_after->enc_done) {
        HIPCK(hipStreamWaitEvent(x, e->enc_after->enc_done, 0));
    }
    if (enc) {
        HIPCK(enc->launch(x));
        if (timed) HIPCK(hipEventRecord(e->gev[1], x));
        else if (e->enc_done && !e->enc_watchers.empty()) HIPCK(hipEventRecord(e->enc_done, x));
    }
    if (dec) HIPCK(dec->launch(x));
    if (!timed) return 0;
    HIPCK(hipEventRecord(e->gev[2], x));
    HIPCK(hipStreamSynchronize(x));
    float a = 0, b = 0;
    if (enc) HIPCK(hipEventElapsedTime(&a, e->gev[0], e->gev[1]));
    HIPCK(hipEventElapsedTime(&b, e->gev[1], e->gev[2]));
    e->split_encode_ms += a; e->split_decode_ms += b; e->split_calls += 1; e->split_steps += rq.sp->max_steps - 1;
    return 0;
}

// hipGraph path: the launch sequence only depends on (B,Q,F,minP,search); inputs and outputs are staged through
// engine-owned buffers so the captured pointers stay valid across calls.
static int generate_graphed(gitmi_engine* e, const Request& rq, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    const bool resident = rq.frames == nullptr;     // follow-up call: the decode part alone (+ the prefill if it is not current)
    // the legacy null stream cannot be captured: run on the engine's own stream, fenced by events
    hipStream_t x = s ? s : e->own_stream;
    if (x != s) {
        HIPCK(hipEventRecord(e->fence_in, s));
        HIPCK(hipStreamWaitEvent(x, e->fence_in, 0));
    }
    // ---- stage the inputs (ragged: ragged_prepare staged the images already; follow-up: no frames)
    const size_t frame_bytes = (size_t)rq.B * 3 * e->H * e->W * sizeof(float);
    const int F_eff = resident ? e->cur_F : c.num_frames > 0 ? std::min(rq.F, c.num_frames) : rq.F;
    if (!e->ragged && !resident)
    for (int f = 0; f < F_eff; ++f)
        HIPCK(hipMemcpyAsync(e->frame_stage[f], rq.frames[f], frame_bytes, hipMemcpyDeviceToDevice, x));
    // ---- look the graphs up, or capture them: the same call on the engine's own frames and output buffers
    Request own = rq;
    if (!resident) { own.frames = e->frame_stage.data(); own.F = F_eff; }
    own.tokens = e->out_tokens; own.logprob = e->out_lp; own.info = e->out_info; own.sent = e->out_sent;
    const GraphKey key = graph_key_of(e, rq, F_eff);
    const CapturedGraph *enc = nullptr, *dec = nullptr;
    gitmi_engine::GraphSet& gs = e->graphs[e->trace_live ? 1 : 0];
    if (resident) {
        RCK(images_ready(e, rq, x));        // the prefill, after gitmi_encode_frames alone: outside the graph
        if (!gs.follow_slot.valid || !(key == gs.follow_slot.key)) {
            gs.follow_slot.valid = false;
            RCK(gs.graph_follow.capture(x, [&] { return generate_decode(e, own, x, false); }));
            gs.follow_slot = {key, true};
        }
        dec = &gs.graph_follow;
    } else {
        // two graphs (encode + prefill | decode) whenever something has to happen between them: profiling events or the
        // enc_done record other contexts wait for
        const bool split = e->profile_mode == 2 || e->enc_after != nullptr || !e->enc_watchers.empty();
        if (!gs.full_slot.valid || !(key == gs.full_slot.key) || split != gs.graph_is_split) {
            gs.full_slot.valid = false;
            gs.graph_decode.reset();
            if (!split) {
                RCK(gs.graph_full.capture(x, [&] { return generate_body(e, own, x, false); }));
            } else {
                RCK(gs.graph_full.capture(x, [&] { return generate_encode(e, own, x); }));
                RCK(gs.graph_decode.capture(x, [&] { return generate_decode(e, own, x, false); }));
            }
            gs.full_slot = {key, true}; gs.graph_is_split = split;
        } else {
            // a replay: the host-side state that enqueueing the encode and the prefill leaves behind
            set_resident(e, rq.B, F_eff);
            set_prefilled(e);
        }
        enc = &gs.graph_full;
        if (split) dec = &gs.graph_decode;
    }
    RCK(replay(e, rq, x, enc, dec));
    // ---- results to the caller's buffers: device memory or PAGE-LOCKED host memory (hipMemcpyDefault: the results then arrive on
    // the host as part of the request itself -- a server reads them after the stream's event without enqueueing anything more, which
    // matters when its other streams keep the device's queues full: a separate small read-back waits milliseconds for a queue slot)
    const size_t nout = (size_t)rq.Q * (size_t)keep_best(*rq.sp);      // sequences returned
    HIPCK(hipMemcpyAsync(rq.tokens, e->out_tokens, nout * rq.sp->max_steps * sizeof(long long), hipMemcpyDefault, x));
    HIPCK(hipMemcpyAsync(rq.logprob, e->out_lp, nout * sizeof(float), hipMemcpyDefault, x));
    HIPCK(hipMemcpyAsync(rq.info, e->out_info, 4 * sizeof(int), hipMemcpyDefault, x));
    if (rq.sent != e->out_sent) HIPCK(hipMemcpyAsync(rq.sent, e->out_sent, (size_t)rq.Q * 2 * sizeof(int), hipMemcpyDefault, x));
    if (x != s) {
        HIPCK(hipEventRecord(e->fence_out, x));
        HIPCK(hipStreamWaitEvent(s, e->fence_out, 0));
    }
    return 0;
}

// common tail of gitmi_generate / gitmi_generate_prefixed: start_dev / plen_dev / img_of_dev are already enqueued on `s`.
// Eager launches for profiling spans and for long step budgets (which poll the finished count), else captured graphs.
// constrained (constrain_check): the call consumes the armed decoding constraints -- here, behind the last step of the entry point
// that can refuse the call, so that a refused call stays armed; the tables are live for exactly this call
// traced (trace_check): likewise the armed per-token trace; its output copies go to the caller's buffers behind the call
static int generate_run(gitmi_engine* e, const Request& rq, hipStream_t s, bool constrained, bool traced) {
    const bool long_budget = rq.sp->max_steps - rq.minP > 32;
    const bool graph = e->pol.use_graph && !e->profiling && !long_budget;
    if (constrained) e->ban_armed = 0;
    e->ban_live = constrained;
    e->ban_seq_live = constrained && e->ban_seq_armed;
    if (traced) e->trace_armed = 0;
    e->trace_live = traced;
    int rc = settle_residency(e, rq, graph ? generate_graphed(e, rq, s) : generate_body(e, rq, s, long_budget && !e->profiling));
    if (rc == 0 && traced) rc = trace_deliver(e, s);
    e->ban_live = e->ban_seq_live = e->trace_live = false;
    return rc;
}

static int constrain_check(const gitmi_engine* e, const char* who, const gitmi_search* sp, int Q, bool* constrained);

extern "C" int gitmi_generate(gitmi_engine* e, const float* const* frames, int F, int B, const int64_t* prefix, int P,
                              const gitmi_search* sp, int64_t* tokens_out, float* logprob_out, int32_t* info_out,
                              void* stream) {
    RCK(check_ready(e));
    const gitmi_config& c = e->cfg;
    if (sp && sp->kind == GITMI_SEARCH_SCORE) return fail("generate: GITMI_SEARCH_SCORE scores given sentences: call gitmi_generate_prefixed");
    if (sp && sp->kind == GITMI_SEARCH_ATTEND) return fail("generate: GITMI_SEARCH_ATTEND maps given sentences: call gitmi_generate_prefixed");
    if (sp && sp->kind == GITMI_SEARCH_CONTEXT) return fail("generate: GITMI_SEARCH_CONTEXT takes context segments: call gitmi_generate_prefixed");
    if (sp && sp->kind == GITMI_SEARCH_TREE_SCORE) return fail("generate: GITMI_SEARCH_TREE_SCORE scores given token trees: call gitmi_generate_prefixed");
    if (sp && sp->kind == GITMI_SEARCH_KEEP) return fail("generate: GITMI_SEARCH_KEEP keeps the memory of resident images: call gitmi_generate_prefixed");
    if (sp && sp->kind == GITMI_SEARCH_RECALL) return fail("generate: GITMI_SEARCH_RECALL recalls kept images: call gitmi_generate_prefixed");
    if (sp && sp->kind == GITMI_SEARCH_FEATURES) return fail("generate: GITMI_SEARCH_FEATURES installs given feature rows: call gitmi_generate_prefixed");
    if (sp && sp->kind == GITMI_SEARCH_CONSTRAIN) return fail("generate: GITMI_SEARCH_CONSTRAIN arms decoding constraints: call gitmi_generate_prefixed");
    if (sp && sp->kind == GITMI_SEARCH_TRACE) return fail("generate: GITMI_SEARCH_TRACE arms the per-token trace: call gitmi_generate_prefixed");
    // follow-up call over the resident images (F is ignored); asked first: without images there is nothing to size buffers by
    if (!frames) RCK(check_resident(e, "generate", B));
    if (!sp || !tokens_out || !logprob_out || !info_out) return fail("generate: null argument");
    if (frames) RCK(check_frames(e, "generate", frames, F, B));
    if (!prefix) P = 1;
    if (P < 1 || P > c.max_text_len) return fail("generate: prefix length %d outside [1,%d]", P, c.max_text_len);
    if (sp->max_steps < P || sp->max_steps > c.max_text_len) return fail("generate: max_steps %d outside [P,%d]", sp->max_steps, c.max_text_len);
    bool constrained = false;
    RCK(constrain_check(e, "generate", sp, B, &constrained));
    bool traced = false;
    RCK(trace_check(e, "generate", sp, B, &traced));
    hipStream_t s = (hipStream_t)stream;
    if (frames) RCK(ragged_prepare(e, frames, F, B, s));
    // start tokens [B, P] on device (shared prefix, or [CLS]) -- filled by a kernel, no host copy
    RCK(fill_uniform_sentences(e, B, (const long long*)prefix, P, s));
    const Request rq{frames, F, B, B, P, P, false, sp, (long long*)tokens_out, logprob_out, info_out, e->out_sent};
    return generate_run(e, rq, s, constrained, traced);
}

// ---- caption scoring (GITMI_SEARCH_SCORE) -------------------------------------------------------------------------
// Token trees (GITMI_SEARCH_TREE_SCORE, include/gitmi.h): depths are embedding positions and index the root path of the structure walk
static int tree_max_depth(const gitmi_config& c) { return std::min((int)c.max_text_len, (int)c.max_pos); }
// Rows (trees x padded nodes) of one tree call.  Every row count, row index and launch grid of the pass is an int and byte offsets
// are size_t, so the binding widths are grid dimensions: the attention's grid.z = padded nodes of a tree / 64 <= 65535 and the
// head's grid.y = rows / 128 <= 65535.  The former, for one tree that has all the rows, is the smaller and is the cap.
constexpr int TREE_MAX_ROWS = 65535 * 64;
static void score_free(gitmi_engine* e) {
    for (void* p : e->sc_allocs) hipFree(p);
    e->sc_allocs.clear();
    e->sc_rows = 0;
    e->tr_out_n = 0;
}
// Workspaces of a score call with `rows` text rows (Q x Lp): allocated by the first score call and grown when a later call
// needs more rows, so an engine that never scores keeps its footprint and one that scores short sentences pays for those.
// Per-sentence buffers are sized for the capacity (max_batch x max_beams sentences x max_text_len; a few hundred KiB).
// tree_out > 0 (GITMI_SEARCH_TREE_SCORE): also the node tables of the rows and an output of tree_out (tree, node) elements,
// kept by later growth; engines that never score trees never hold them.
static int score_alloc(gitmi_engine* e, size_t rows_needed, size_t tree_out = 0) {
    size_t rows = (size_t)round_up((int)rows_needed, 128);          // the head's 128-row tiles (its loads clamp to M - 1)
    if (e->sc_rows >= rows && e->tr_out_n >= tree_out) return 0;
    rows = std::max(rows, e->sc_rows);
    tree_out = std::max(tree_out, e->tr_out_n);
    score_free(e);
    const gitmi_config& c = e->cfg;
    const int d = c.dec_hidden;
    const size_t Qmax = (size_t)c.max_batch * c.max_beams;
    const size_t esz = e->pol.esz;
    auto alloc = [&](auto** p, size_t bytes) -> bool {
        void* q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) return false;
        e->sc_allocs.push_back(q);
        *reinterpret_cast<void**>(p) = q;
        return true;
    };
    const bool ok = alloc(&e->sc_hf, rows * d * 4) && alloc(&e->sc_y, rows * d * 4) && alloc(&e->sc_ht, rows * d * esz) &&
                    alloc(&e->sc_qkv, rows * 3 * d * esz) && alloc(&e->sc_ctx, rows * d * esz) &&
                    alloc(&e->sc_u, rows * c.dec_ffn * esz) &&
                    alloc(&e->sc_part, rows * (size_t)(e->pol.f32 ? 1 : score_head_tiles(c.vocab)) * sizeof(float4)) &&
                    alloc(&e->sc_zt, rows * 4) && alloc(&e->sc_tgt, rows * 4) && alloc(&e->sc_lens, Qmax * 4) &&
                    alloc(&e->sc_img, Qmax * 4) && alloc(&e->sc_bad, Qmax * 4) && alloc(&e->sc_info, 16) &&
                    alloc(&e->sc_out, Qmax * (size_t)c.max_text_len * sizeof(float2)) &&
                    (!tree_out || (alloc(&e->tr_nodes, rows * 4 * sizeof(int)) && alloc(&e->tr_out, tree_out * sizeof(float2))));
    if (!ok) {
        score_free(e);
        (void)hipGetLastError();
        return fail("score: out of device memory for the workspaces of %zu text rows", rows);
    }
    e->sc_rows = rows;
    e->tr_out_n = tree_out;
    return 0;
}

// ---- attention maps (GITMI_SEARCH_ATTEND) --------------------------------------------------------------------------------
// The output [Q, ld, layers, Kc] and one layer's statistics [Q, heads, Lp]: allocated by the first attend call, grown when a
// later call needs more (engines that never attend keep their footprint).  The text pass itself runs in score_alloc's workspaces.
static int attend_alloc(gitmi_engine* e, size_t floats, size_t stat_rows) {
    if (e->at_floats < floats) {
        hipFree(e->at_out);
        e->at_out = nullptr; e->at_floats = 0;
        if (hipMalloc(&e->at_out, floats * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return fail("attend: out of device memory for the %zu floats of the maps", floats);
        }
        e->at_floats = floats;
    }
    if (e->at_stat_rows < stat_rows) {
        hipFree(e->at_stats);
        e->at_stats = nullptr; e->at_stat_rows = 0;
        if (hipMalloc(&e->at_stats, stat_rows * sizeof(float2)) != hipSuccess) {
            (void)hipGetLastError();
            return fail("attend: out of device memory for the softmax statistics of %zu rows", stat_rows);
        }
        e->at_stat_rows = stat_rows;
    }
    return 0;
}
// image key rows of one image in a call: what an encode of these frames makes resident, or what is
static int call_Nimg(const gitmi_engine* e, const float* const* frames, int F) {
    if (!frames) return e->cur_Nimg;
    return (e->cfg.num_frames > 0 ? std::min(F, (int)e->cfg.num_frames) : F) * e->N;
}

// vocabulary head of the score pass over the M text rows in sc_ht, reduced to per-row statistics: sc_part [M][*ntiles], sc_zt
// tree (token trees; sc_tgt holds no target): sc_zt[node row] = the logit of the node's token at its parent's row instead
static int score_head_impl(gitmi_engine* e, int M, hipStream_t s, int* ntiles, const TreeNodes* tree = nullptr, int Lp = 0) {
    const gitmi_config& c = e->cfg;
    const int d = c.dec_hidden, V = c.vocab;
    // launch_score_head_rows (gitmi_debug_score_tail runs it on a caller's buffers): 16-bit modes the fused head; the parity mode
    // materialises the logits in e->logits, the decode workspace's rows at a time (the last three fields, unused otherwise).
    // One span over the whole head: in parity mode it times the row statistics and the tree gather with the GEMM chunks.
    const ScoreHeadArgs h{e->sc_ht, e->w.out_w, e->w.out_b, e->sc_tgt, e->sc_part, e->sc_zt, e->logits, e->ldl,
                          round_up(c.max_batch * c.max_beams, 64)};
    SpanGuard sp(e, s, TAG_GEMM_OTHER, gemm_flops(M, V, d));
    HIPCK(launch_score_head_rows(h, e->pol.f32, M, V, d, tree, Lp, ntiles, s));
    return 0;
}
// The text pass of GITMI_SEARCH_SCORE / _ATTEND: the textual head over whole sentences (CaptioningModel.forward_one_ce,
// decoder.py:916-972) after the usual encode + prefill: embedding of every position, then the decoder layers over all text rows
// at once (generic GEMM + LayerNorm launches, the attention of kernels_score.hip against the prefill's image K/V).  tokens [Q][ld]
// device int64; lens / image_of already on the device.  score: then the vocabulary head, reduced to (lp, mean_lp) per position
// in sc_out [Q][ld].  attend: every layer's attention launch also writes its softmax statistics and the map kernel turns them
// into the head-mean probabilities of the layer's slice of at_out [Q, ld, layers, Kc] (zero-filled first: rows past a sentence's
// length, text columns past a row, image columns past a ragged image's own rows stay 0); the last layer stops after its
// attention (nothing reads its output) and there is no head.
static int text_pass_impl(gitmi_engine* e, const Request& rq, const long long* tokens, int ld, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    const int d = c.dec_hidden, V = c.vocab, Q = rq.Q, L = c.dec_layers;
    const bool attend = rq.sp->kind == GITMI_SEARCH_ATTEND, tree = rq.sp->kind == GITMI_SEARCH_TREE_SCORE;
    RCK(images_ready(e, rq, s));
    const int Lp = round_up(rq.maxP, 16), M = Q * Lp;
    const int Nk = e->cur_Nimg, Kc = Nk + ld;
    void* const out = attend ? (void*)e->at_out : tree ? (void*)e->tr_out : (void*)e->sc_out;
    const size_t out_bytes = attend ? (size_t)Q * ld * L * Kc * sizeof(float) : (size_t)Q * ld * sizeof(float2);
    auto zero_outputs = [&]() -> int {
        HIPCK(hipMemsetAsync(out, 0, out_bytes, s));
        HIPCK(hipMemsetAsync(e->sc_bad, 0, (size_t)Q * sizeof(int), s));
        return 0;
    };
    SpanGuard phase(e, s, TAG_DECODE, 0);
    if (attend || tree) RCK(zero_outputs());       // the map kernels of every layer write into it; the tree verdicts flag sc_bad
    // token trees: `tokens` is the packed (depth, token) table.  The structure launch is the only reader of its depths; a tree
    // that fails its rules leaves it as parentless rows, so no later kernel forms an address from what the caller sent.
    const size_t R = tree ? e->sc_rows : 0;
    const TreeNodes nodes = tree ? TreeNodes{e->tr_nodes, e->tr_nodes + R, e->tr_nodes + 2 * R, e->tr_nodes + 3 * R} : TreeNodes{};
    if (tree) HIPCK(launch_tree_structure(tokens, ld, Q, Lp, e->sc_lens, V, tree_max_depth(c), nodes, e->sc_bad, s));
    HIPCK(launch_score_embed_ln(tokens, ld, Q, Lp, e->w.words_f, e->w.positions_f, e->w.emb_lng, e->w.emb_lnb, 1e-8f, e->sc_hf, e->sc_ht,
                                e->pol.f32, d, V, c.max_pos, s, tree ? &nodes : nullptr));
    const int* ntok = key_counts(e);
    for (int l = 0; l < L; ++l) {
        const DecLayerW& W = e->w.dec[l];
        RCK(gemm(e, s, e->sc_ht, d, W.wqkv, W.bqkv, nullptr, 0, e->sc_qkv, 3 * d, e->pol.f32, M, 3 * d, d, 0, TAG_GEMM_OTHER));
        HIPCK(launch_score_attn(e->sc_qkv, e->img_kv[l], e->sc_img, e->sc_ctx, Q, c.dec_heads, d, Nk, Lp, 0.125f, e->pol.f32, s, ntok,
                                attend ? e->at_stats : nullptr, tree ? nodes.end : nullptr));
        if (attend)
            HIPCK(launch_score_attn_map(e->sc_qkv, e->img_kv[l], e->sc_img, ntok, e->at_stats, e->sc_lens, e->at_out + (size_t)l * Kc,
                                        (size_t)ld * L * Kc, (size_t)L * Kc, ld, Q, c.dec_heads, Nk, Lp, 0.125f, e->pol.f32, e->sc_bad, s));
        if (!attend || l + 1 < L) RCK(dec_layer_tail(e, s, W, e->sc_ctx, e->sc_hf, e->sc_ht, e->sc_y, e->sc_u, M));
    }
    if (int ntiles = 1; tree) {
        HIPCK(hipMemsetAsync(e->sc_tgt, 0xff, (size_t)M * sizeof(int), s));      // no row has a single target: -1 everywhere
        RCK(score_head_impl(e, M, s, &ntiles, &nodes, Lp));
        HIPCK(launch_tree_combine(e->sc_part, ntiles, e->sc_zt, nodes, M, Lp, ld, V, e->tr_out, e->sc_bad, s));
    } else if (!attend) {
        HIPCK(launch_score_targets(tokens, ld, Lp, e->sc_lens, V, M, e->sc_tgt, s));
        RCK(score_head_impl(e, M, s, &ntiles));
        RCK(zero_outputs());
        HIPCK(launch_score_combine(e->sc_part, ntiles, e->sc_zt, e->sc_tgt, M, Lp, ld, V, e->sc_out, e->sc_bad, s));
    }
    if (e->ragged) HIPCK(launch_ragged_report(e->rg_meta, e->sc_img, Q, 0, nullptr, nullptr, e->sc_bad, s));
    HIPCK(launch_score_info(e->sc_bad, Q, ld, e->sc_info, s, attend ? Kc : 0, attend ? L : 0));
    HIPCK(hipMemcpyAsync(rq.logprob, out, out_bytes, hipMemcpyDefault, s));
    HIPCK(hipMemcpyAsync(rq.info, e->sc_info, 4 * sizeof(int), hipMemcpyDefault, s));
    return 0;
}

// Sentence tables of gitmi_generate_prefixed (every kind): read_sentences checks Q <= Qmax (`cap` names it), lengths in
// [1, ld] and images in [0, B) into plen_host / img_of_host; upload_sentences copies them to the caller's device tables.
struct SentenceSpan { int minP, maxP; bool ident; };
static int read_sentences(gitmi_engine* e, const char* who, const int32_t* plen, const int32_t* image_of, int ld, int B, int Q,
                          int Qmax, const char* cap, SentenceSpan* span) {
    if (Q < 1 || Q > Qmax) return fail("%s: Q=%d sentences outside [1,%d] (%s)", who, Q, Qmax, cap);
    if (!image_of && Q != B) return fail("%s: without image_of, Q must equal B", who);
    *span = {1 << 30, 0, true};
    e->plen_host.assign(plen, plen + Q);
    e->img_of_host.resize(Q);
    for (int q = 0; q < Q; ++q) {
        const int p = plen[q];
        if (p < 1 || p > ld) return fail("%s: length %d of sentence %d outside [1,%d]", who, p, q, ld);
        span->minP = std::min(span->minP, p); span->maxP = std::max(span->maxP, p);
        const int im = image_of ? image_of[q] : q;
        if (im < 0 || im >= B) return fail("%s: sentence %d names image %d of %d", who, q, im, B);
        e->img_of_host[q] = im;
        span->ident = span->ident && im == q;
    }
    return 0;
}
// staged synchronously (the previous call's work on `s` may still read them): this serves the VQA loop, not the benchmark
static int upload_sentences(gitmi_engine* e, int* plen_dst, int* img_dst, hipStream_t s) {
    const size_t bytes = e->plen_host.size() * sizeof(int);
    HIPCK(hipStreamSynchronize(s));
    HIPCK(hipMemcpy(plen_dst, e->plen_host.data(), bytes, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(img_dst, e->img_of_host.data(), bytes, hipMemcpyHostToDevice));
    return 0;
}

// ---- context tokens in the decoder memory (GITMI_SEARCH_CONTEXT, include/gitmi.h; decoder.py:861-871) ----------------------------
// The segment table of a call lives in ctx_tab, allocated by the first context call and grown on demand.
static int context_alloc(gitmi_engine* e, size_t ints) {
    if (e->ctx_tab_ints >= ints) return 0;
    hipFree(e->ctx_tab);
    e->ctx_tab = nullptr; e->ctx_tab_ints = 0;
    if (hipMalloc((void**)&e->ctx_tab, ints * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        return fail("context: out of device memory for the table of the segments");
    }
    e->ctx_tab_ints = ints;
    return 0;
}
// Encode + context rows + prefill, eagerly: the images and their context are resident afterwards, in key-count mode.
// Every check comes before the first launch (an argument error leaves the resident set as it was).
static int context_call(gitmi_engine* e, const float* const* frames, int F, int B, const long long* tokens, int ld,
                        const int32_t* len_host, const int32_t* image_of_host, int Q, int32_t* info_out, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    if (!frames)
        return fail("context: frames == NULL: context segments come with the call that encodes their images (appending context "
                    "to resident images is not implemented)");
    if (!tokens || !len_host || !info_out) return fail("context: null argument");
    RCK(check_frames(e, "context", frames, F, B));
    if (e->ragged)
        return fail("context: ragged image mode (gitmi_set_image_shape(e, 0, 0)): context on images of mixed shapes is not implemented");
    if (c.vit_width != c.dec_hidden)
        return fail("context: visual_feature_size %d != hidden_size %d: the reference cannot concatenate the embedded tokens to "
                    "the visual features of this model (decoder.py:866)", c.vit_width, c.dec_hidden);
    if (ld < 1) return fail("context: ld=%d", ld);
    const int n_img = call_Nimg(e, frames, F), cap = c.max_frames * e->Nmax;
    ContextTable t;
    RCK(context_table("context", len_host, image_of_host, Q, B, std::min(ld, (int)c.max_pos), n_img, cap, &t));
    RCK(context_alloc(e, t.tab.size()));
    // staged synchronously, as upload_sentences does: the previous call's work on `s` may still read the table
    HIPCK(hipStreamSynchronize(s));
    HIPCK(hipMemcpy(e->ctx_tab, t.tab.data(), t.tab.size() * sizeof(int), hipMemcpyHostToDevice));
    const int* tab = e->ctx_tab;
    auto body = [&]() -> int {
        RCK(encode_frames_impl(e, frames, F, B, nullptr, s, t.stride));
        HIPCK(launch_context_embed(tokens, ld, (const int4*)tab, Q, tab + 4 * (size_t)Q, e->w.words_f, e->w.positions_f, e->w.emb_lng,
                                   e->w.emb_lnb, 1e-8f, e->feats, e->pol.f32, nullptr, e->rg_ntok, B, n_img, t.stride, c.vit_width,
                                   c.vocab, c.max_pos, s));
        set_context(e);
        for (int b = 0; b < B; ++b) e->res_desc.push_back(int4{n_img, t.cnt()[b], e->H, e->W});
        RCK(prefill_impl(e, s));
        HIPCK(hipMemcpyAsync(info_out, tab + 4 * (size_t)Q + B, 4 * sizeof(int), hipMemcpyDefault, s));
        return 0;
    };
    const int rc = body();
    if (rc != 0) drop_resident(e);
    return rc;
}

// ---- image memory snapshots (GITMI_SEARCH_KEEP / GITMI_SEARCH_RECALL, include/gitmi.h) ------------------------------------------
// What a follow-up call reads of an image is its feature rows (a later prefill), the K | V columns of its prefill rows
// (text pass) and their decode layouts (decode attention; rebuilt by kv_repack), plus its key count.  KEEP copies the first two
// into a slot of the caller's store, RECALL copies any selection of slots back and rebuilds the third.
static int memory_cap_rows(const gitmi_engine* e) { return e->cfg.max_frames * e->Nmax; }
static int memory_elem_dtype(const gitmi_engine* e) { return e->pol.f32 ? GITMI_DTYPE_F32 : gitmi_operand_dtype(); }
// the geometry of a slot and of the engine's buffers (stride: the rows of an image's block there); fails by message where
// the configuration does not fit the kernels
static int memory_args(const gitmi_engine* e, const char* who, int stride, MemoryArgs* out) {
    const gitmi_config& c = e->cfg;
    const size_t esz = e->pol.esz, cap = (size_t)memory_cap_rows(e);
    if (c.dec_layers > MEMORY_MAX_LAYERS) return fail("%s: %d decoder layers, the layer table holds %d", who, c.dec_layers, MEMORY_MAX_LAYERS);
    if ((c.vit_width * esz) % 16 || (2 * c.dec_hidden * esz) % 16 || (c.dec_hidden * esz) % 16)
        return fail("%s: rows of %zu and %zu bytes are not multiples of the 16 bytes a lane moves", who, c.vit_width * esz, 2 * c.dec_hidden * esz);
    MemoryArgs a{};
    a.feats = e->feats;
    for (int l = 0; l < c.dec_layers; ++l) a.kv[l] = e->img_kv[l];
    a.layers = c.dec_layers; a.stride = stride;
    a.feat_row = (int)(c.vit_width * esz); a.kv_row = (int)(2 * c.dec_hidden * esz);
    a.kv_ld = (int)(3 * c.dec_hidden * esz); a.kv_col = (int)(c.dec_hidden * esz);
    a.feat_plane = cap * a.feat_row; a.kv_plane = cap * a.kv_row;
    a.slot_bytes = (MEMORY_HEADER_BYTES + a.feat_plane + c.dec_layers * a.kv_plane + 255) / 256 * 256;
    a.ntok = e->rg_ntok; a.meta = nullptr;
    *out = a;
    return 0;
}
static void memory_fingerprint(const gitmi_engine* e, int* hdr) {
    const gitmi_config& c = e->cfg;
    const int fp[MEMW_FP_END - MEMW_FP0] = {c.vit_width, c.dec_hidden, c.dec_layers, c.dec_heads, (int)e->pol.esz, memory_elem_dtype(e),
                                            memory_cap_rows(e)};
    for (int i = 0; i < MEMW_FP_END - MEMW_FP0; ++i) hdr[MEMW_FP0 + i] = fp[i];
}
static const char* const MEMORY_FP_NAMES[MEMW_FP_END - MEMW_FP0] = {"vit_width", "dec_hidden", "dec_layers", "dec_heads", "element size",
                                                                     "element dtype", "row capacity"};
static int memory_table_alloc(gitmi_engine* e, const char* who) {
    const size_t n = (size_t)e->cfg.max_batch;
    if (e->mem_tab_n >= n) return 0;
    hipFree(e->mem_tab);
    e->mem_tab = nullptr; e->mem_tab_n = 0;
    // the entries, and behind them room for the first 64 bytes of every slot header of a RECALL (memory_headers)
    if (hipMalloc((void**)&e->mem_tab, n * (sizeof(MemoryEntry) + MEMORY_HEADER_WORDS * sizeof(int))) != hipSuccess) {
        (void)hipGetLastError();
        return fail("%s: out of device memory for the table of the call", who);
    }
    e->mem_tab_n = n;
    return 0;
}
static int* memory_headers(gitmi_engine* e) { return reinterpret_cast<int*>(e->mem_tab + e->mem_tab_n); }
// info_out (device or page-locked host) <- four host values; the stream is synchronised so that they may live on the stack
static int memory_info(const int (&v)[4], int32_t* info_out, hipStream_t s) {
    HIPCK(hipMemcpyAsync(info_out, v, sizeof(v), hipMemcpyDefault, s));
    HIPCK(hipStreamSynchronize(s));
    return 0;
}
// the checks KEEP and RECALL share on the store and the slot list
static int memory_check_store(const char* who, const void* store, int slots, const int32_t* slot_of, int Q) {
    if (!store) return fail("%s: null store", who);
    if ((uintptr_t)store & 255) return fail("%s: the store's base address %p is not 256-byte aligned", who, store);
    if (slots < 1) return fail("%s: a store of %d slots", who, slots);
    if (!slot_of) return fail("%s: null slot list (prefix_len_host)", who);
    for (int q = 0; q < Q; ++q)
        if (slot_of[q] < 0 || slot_of[q] >= slots) return fail("%s: entry %d names slot %d of a store of %d slots", who, q, slot_of[q], slots);
    return 0;
}

static int memory_keep(gitmi_engine* e, const float* const* frames, int B, void* store, int slots, const int32_t* slot_of,
                       const int32_t* image_of, int Q, int32_t* info_out, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    if (!info_out) return fail("keep: null info_out");
    MemoryArgs a;
    RCK(memory_args(e, "keep", 1, &a));
    const int units = (int)(a.slot_bytes / 256);
    if (Q == 0) return memory_info({units, 0, 0, 0}, info_out, s);         // the size query
    if (frames) return fail("keep: frames != NULL: KEEP runs over the resident images (encode them with a call of their own)");
    RCK(check_resident(e, "keep", B));
    if (Q < 1 || Q > c.max_batch) return fail("keep: Q=%d images outside [1,%d] (max_batch)", Q, c.max_batch);
    if (!image_of && Q != B) return fail("keep: without image_of, Q must equal B");
    RCK(memory_check_store("keep", store, slots, slot_of, Q));
    for (int q = 0; q < Q; ++q) {
        const int im = image_of ? image_of[q] : q;
        if (im < 0 || im >= B) return fail("keep: entry %d names image %d of %d", q, im, B);
        for (int p = 0; p < q; ++p)
            if (slot_of[p] == slot_of[q]) return fail("keep: entries %d and %d both write slot %d", p, q, slot_of[q]);
    }
    RCK(memory_table_alloc(e, "keep"));
    RCK(images_ready(e, Request{}, s));             // after gitmi_encode_frames alone: the prefill first, as a follow-up does
    // what the host has to know of every image: a ragged batch keeps it on the device
    HIPCK(hipStreamSynchronize(s));
    std::vector<int4> meta;
    if (e->res_desc.empty() && e->ragged) {
        meta.resize(B);
        HIPCK(hipMemcpy(meta.data(), e->rg_meta, (size_t)B * sizeof(int4), hipMemcpyDeviceToHost));
    }
    std::vector<MemoryEntry> tab(Q);
    int max_n = 0, sum_n = 0;
    for (int q = 0; q < Q; ++q) {
        const int im = image_of ? image_of[q] : q;
        MemoryEntry& en = tab[q];
        memset(&en, 0, sizeof(en));
        int* h = en.hdr;
        h[MEMW_MAGIC] = MEMORY_MAGIC; h[MEMW_VERSION] = 1;
        memory_fingerprint(e, h);
        h[MEMW_F] = e->cur_F;
        if (!e->res_desc.empty()) {
            const int4 d = e->res_desc[im];
            h[MEMW_IMG_ROWS] = d.x; h[MEMW_CTX_ROWS] = d.y; h[MEMW_H] = d.z; h[MEMW_W] = d.w;
        } else if (e->ragged) {
            h[MEMW_IMG_ROWS] = meta[im].z; h[MEMW_H] = meta[im].x; h[MEMW_W] = meta[im].y; h[MEMW_REJECTED] = meta[im].w != 0;
        } else {
            h[MEMW_IMG_ROWS] = e->cur_Nimg; h[MEMW_H] = e->H; h[MEMW_W] = e->W;
        }
        h[MEMW_N] = h[MEMW_IMG_ROWS] + h[MEMW_CTX_ROWS];
        if (h[MEMW_N] < 0 || h[MEMW_N] > e->cur_Nimg || h[MEMW_N] > memory_cap_rows(e))
            return fail("keep: image %d has %d rows, its block holds %d", im, h[MEMW_N], e->cur_Nimg);
        en.image = im; en.slot = slot_of[q]; en.n = h[MEMW_N];
        max_n = std::max(max_n, en.n); sum_n += en.n;
    }
    HIPCK(hipMemcpy(e->mem_tab, tab.data(), (size_t)Q * sizeof(MemoryEntry), hipMemcpyHostToDevice));
    a.stride = e->cur_Nimg;
    HIPCK(launch_memory_pack(a, store, e->mem_tab, Q, max_n, s));
    return memory_info({units, max_n, sum_n, 0}, info_out, s);
}

static int memory_recall(gitmi_engine* e, const float* const* frames, int B, const void* store, int slots, const int32_t* slot_of,
                         const int32_t* image_of, int Q, int32_t* info_out, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    if (frames) return fail("recall: frames != NULL: RECALL forms its images from kept slots");
    if (!info_out) return fail("recall: null info_out");
    if (image_of) return fail("recall: image_of_host must be NULL (slot q becomes image q)");
    if (Q < 1 || Q > c.max_batch) return fail("recall: Q=%d images outside [1,%d] (max_batch)", Q, c.max_batch);
    if (B != Q) return fail("recall: B=%d must equal Q=%d, the number of images to form", B, Q);
    RCK(memory_check_store("recall", store, slots, slot_of, Q));
    const int cap = memory_cap_rows(e);
    MemoryArgs a;
    RCK(memory_args(e, "recall", 1, &a));
    RCK(memory_table_alloc(e, "recall"));
    // the headers, validated on the host before anything is launched: gathered on the device (one small copy per slot,
    // enqueued), then one copy to the host and one synchronisation -- not a blocking read per slot
    const size_t hbytes = MEMORY_HEADER_WORDS * sizeof(int);
    for (int q = 0; q < Q; ++q)
        HIPCK(hipMemcpyAsync(memory_headers(e) + (size_t)q * MEMORY_HEADER_WORDS, (const char*)store + (size_t)slot_of[q] * a.slot_bytes,
                             hbytes, hipMemcpyDefault, s));
    std::vector<int> headers((size_t)Q * MEMORY_HEADER_WORDS);
    HIPCK(hipMemcpyAsync(headers.data(), memory_headers(e), (size_t)Q * hbytes, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    std::vector<MemoryEntry> tab(Q);
    int want[MEMORY_HEADER_WORDS] = {};
    memory_fingerprint(e, want);
    int max_n = 0, sum_n = 0, F = 0;
    bool uniform = !e->ragged, context = false;
    for (int q = 0; q < Q; ++q) {
        MemoryEntry& en = tab[q];
        memset(&en, 0, sizeof(en));
        const int slot = slot_of[q];
        int* h = en.hdr;
        memcpy(h, headers.data() + (size_t)q * MEMORY_HEADER_WORDS, hbytes);
        if (h[MEMW_MAGIC] != MEMORY_MAGIC || h[MEMW_VERSION] != 1)
            return fail("recall: slot %d: bad magic 0x%08x / version %d (nothing was kept there)", slot, (unsigned)h[MEMW_MAGIC], h[MEMW_VERSION]);
        for (int i = MEMW_FP0; i < MEMW_FP_END; ++i)
            if (h[i] != want[i])
                return fail("recall: slot %d: fingerprint mismatch: %s is %d in the slot, %d in this engine (kept by another model, "
                            "precision or capacity)", slot, MEMORY_FP_NAMES[i - MEMW_FP0], h[i], want[i]);
        const int n = h[MEMW_N];
        if (n < 1 || n > cap) return fail("recall: slot %d: n=%d rows outside [1,%d], the per-image capacity", slot, n, cap);
        if (h[MEMW_IMG_ROWS] < 1 || h[MEMW_CTX_ROWS] < 0 || h[MEMW_IMG_ROWS] + h[MEMW_CTX_ROWS] != n)
            return fail("recall: slot %d: %d image rows + %d context rows do not make n=%d", slot, h[MEMW_IMG_ROWS], h[MEMW_CTX_ROWS], n);
        if (h[MEMW_REJECTED]) return fail("recall: slot %d: the rejected flag is set (a ragged entry the device refused was kept)", slot);
        if (h[MEMW_F] < 1 || h[MEMW_F] > c.max_frames) return fail("recall: slot %d: F=%d frames outside [1,%d]", slot, h[MEMW_F], c.max_frames);
        if (q == 0) F = h[MEMW_F];
        if (h[MEMW_F] != F) return fail("recall: slot %d: F=%d frames, slot %d has F=%d (one batch, one F)", slot, h[MEMW_F], slot_of[0], F);
        uniform = uniform && h[MEMW_CTX_ROWS] == 0 && n == F * e->N;
        context = context || h[MEMW_CTX_ROWS] > 0;
        en.image = q; en.slot = slot; en.n = n;
        max_n = std::max(max_n, n); sum_n += n;
    }
    // the mode: exactly the state the original call left where that is a uniform batch of the current shape, else key counts
    const int stride = uniform ? F * e->N : round_up(max_n, 16) <= cap ? round_up(max_n, 16) : max_n;
    HIPCK(hipMemcpy(e->mem_tab, tab.data(), (size_t)Q * sizeof(MemoryEntry), hipMemcpyHostToDevice));
    a.stride = stride;
    a.meta = e->ragged ? e->rg_meta : nullptr;
    auto body = [&]() -> int {
        drop_resident(e);               // the workspaces are overwritten from here on
        HIPCK(launch_memory_unpack(a, store, e->mem_tab, Q, s));
        for (int l = 0; l < c.dec_layers; ++l) RCK(kv_repack(e, l, Q, stride, s));
        set_resident(e, Q, F, stride);
        if (!uniform) {
            e->keyed = true; e->has_context = context;
            for (int q = 0; q < Q; ++q)
                e->res_desc.push_back(int4{tab[q].hdr[MEMW_IMG_ROWS], tab[q].hdr[MEMW_CTX_ROWS], tab[q].hdr[MEMW_H], tab[q].hdr[MEMW_W]});
        }
        set_prefilled(e);
        return memory_info({stride, max_n, sum_n, 0}, info_out, s);
    };
    const int rc = body();
    if (rc != 0) drop_resident(e);
    return rc;
}

// ---- features in (GITMI_SEARCH_FEATURES, include/gitmi.h) -------------------------------------------------------------------------
// The other side of gitmi_encode_frames' feats_out: rows the caller holds -- cached, composed from per-frame rows, averaged, of
// another tower of the same width -- become the resident feature tensor, and the prefill runs over them.  Every check comes
// before the first launch (an argument error leaves the resident set as it was).
static int features_call(gitmi_engine* e, const float* const* frames, int F, int B, const void* rows, int dtype, int ld,
                         const int32_t* pieces_host, const int32_t* image_of_host, int Q, int32_t* info_out, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    if (frames) return fail("features: frames != NULL: the images of this call are formed from the given feature rows");
    if (!rows || !pieces_host || !info_out) return fail("features: null argument");
    if ((uintptr_t)rows & 15) return fail("features: the base address %p of the rows is not 16-byte aligned", rows);
    if (c.vit_width % 8) return fail("features: vit_width %d is not a multiple of the 8 elements a lane moves", c.vit_width);
    if (dtype != GITMI_DTYPE_F32 && (e->pol.f32 || dtype != gitmi_operand_dtype()))
        return fail("features: rows of element type %d: this engine takes GITMI_DTYPE_F32 (0)%s", dtype,
                    e->pol.f32 ? " only (fp32 precision)"
                               : gitmi_operand_dtype() == GITMI_DTYPE_F16 ? " or GITMI_DTYPE_F16 (2), this library's 16-bit operand type"
                                                                          : " or GITMI_DTYPE_BF16 (1), this library's 16-bit operand type");
    if (B < 1 || B > c.max_batch) return fail("features: B=%d outside [1,%d]", B, c.max_batch);
    if (F < 1 || F > c.max_frames) return fail("features: F=%d outside [1,%d] (max_frames)", F, c.max_frames);
    if (c.num_frames > 0 && F > c.num_frames) return fail("features: F=%d above the %d frames of the model (num_frames)", F, c.num_frames);
    const int Qmax = c.max_batch * c.max_frames;
    if (Q < 1 || Q > Qmax) return fail("features: Q=%d pieces outside [1,%d] (max_batch x max_frames)", Q, Qmax);
    if (!image_of_host && Q != B) return fail("features: without image_of, Q must equal B");
    if (ld < 1) return fail("features: a buffer of %d rows (ld_prefix)", ld);
    const int cap = c.max_frames * e->Nmax;
    std::vector<FeaturePiece> tab((size_t)Q);
    std::vector<int> count((size_t)B, 0);
    for (int q = 0; q < Q; ++q) {
        const int im = image_of_host ? image_of_host[q] : q;
        const int src0 = pieces_host[3 * q], n = pieces_host[3 * q + 1], t = pieces_host[3 * q + 2];
        if (im < 0 || im >= B) return fail("features: piece %d names image %d of %d", q, im, B);
        if (n < 1) return fail("features: piece %d has %d rows (at least 1)", q, n);
        if (src0 < 0 || (long long)src0 + n > ld)
            return fail("features: piece %d reads rows [%d,%lld) of a buffer of %d rows", q, src0, (long long)src0 + n, ld);
        if (t < -1) return fail("features: piece %d has temporal index %d (-1: none)", q, t);
        if (t >= 0 && c.num_frames <= 0) return fail("features: piece %d has temporal index %d, but the model has no temporal embeddings", q, t);
        if (t >= c.num_frames && t >= 0) return fail("features: piece %d has temporal index %d outside [0,%d) (num_frames)", q, t, c.num_frames);
        if ((long long)count[im] + n > cap)
            return fail("features: image %d asks for %lld rows, the workspaces hold %d per image (max_frames x max(N, max_image_tokens))",
                        im, (long long)count[im] + n, cap);
        tab[q] = FeaturePiece{im, count[im], src0, n, t >= 0 ? e->w.temb[t] : nullptr};
        count[im] += n;
    }
    int max_n = 0, sum_n = 0;
    bool uniform = !e->ragged;
    for (int b = 0; b < B; ++b) {
        if (count[b] < 1) return fail("features: image %d has no piece", b);
        max_n = std::max(max_n, count[b]); sum_n += count[b];
        uniform = uniform && count[b] == F * e->N;
    }
    // the mode, by RECALL's rule: a uniform batch of the current shape is exactly what gitmi_encode_frames leaves, else key counts
    const int stride = uniform ? F * e->N : round_up(max_n, 16) <= cap ? round_up(max_n, 16) : max_n;
    const size_t tab_bytes = (size_t)Qmax * sizeof(FeaturePiece) + (size_t)c.max_batch * sizeof(int);
    if (!e->feat_tab && hipMalloc((void**)&e->feat_tab, tab_bytes) != hipSuccess) {
        (void)hipGetLastError();
        e->feat_tab = nullptr;
        return fail("features: out of device memory for the table of the call");
    }
    int* count_dev = reinterpret_cast<int*>(e->feat_tab + Qmax);
    // staged synchronously, as upload_sentences does: the previous call's work on `s` may still read the table
    HIPCK(hipStreamSynchronize(s));
    HIPCK(hipMemcpy(e->feat_tab, tab.data(), (size_t)Q * sizeof(FeaturePiece), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(count_dev, count.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
    FeatureArgs a{};
    a.feats = e->feats; a.src = rows; a.pieces = e->feat_tab; a.pieces_n = Q; a.count = count_dev;
    a.stride = stride; a.D = c.vit_width;
    a.ntok = e->rg_ntok; a.meta = e->ragged ? e->rg_meta : nullptr;
    auto body = [&]() -> int {
        drop_resident(e);               // the workspaces are overwritten from here on
        HIPCK(launch_feature_install(a, B, dtype != GITMI_DTYPE_F32, !e->pol.f32, s));
        set_resident(e, B, F, uniform ? 0 : stride);
        if (!uniform) {
            e->keyed = true;
            for (int b = 0; b < B; ++b) e->res_desc.push_back(int4{count[b], 0, 0, 0});
        }
        RCK(prefill_impl(e, s));
        return memory_info({stride, max_n, sum_n, 0}, info_out, s);
    };
    const int rc = body();
    if (rc != 0) drop_resident(e);
    return rc;
}

// ---- per-sentence decoding constraints (GITMI_SEARCH_CONSTRAIN, include/gitmi.h; the rule: ban_rules.h) -----------------------
// Arms the constraints of the NEXT search call of this context: the ban sets (DEVICE words) and the per-sentence table (host) are
// copied into the engine's own tables.  Every check comes before any launch; a refused call leaves what was armed, and what is
// resident, as it was.  Q == 0 disarms.
// info_out of an arming call, enqueued on `s` like the tables (through the staging buffer where there is one: no host wait)
static int constrain_info(gitmi_engine* e, const int (&v)[4], int32_t* info_out, hipStream_t s) {
    if (!e->ban_stage) return memory_info(v, info_out, s);          // a disarming call on a context that was never armed
    HIPCK(hipEventSynchronize(e->ban_staged));
    int* dst = e->ban_stage + 3 * (size_t)e->cfg.max_batch;
    for (int i = 0; i < 4; ++i) dst[i] = v[i];
    HIPCK(hipMemcpyAsync(info_out, dst, 4 * sizeof(int), hipMemcpyDefault, s));
    HIPCK(hipEventRecord(e->ban_staged, s));
    return 0;
}
// n_pool > 0 (search->reserved_): pool_host is the HOST pool of banned token sequences, int32 [n_pool] (abi_common.h ban_pool_check)
static int constrain_call(gitmi_engine* e, const float* const* frames, const unsigned int* sets, int n_sets, const int32_t* table_host,
                          const int32_t* image_of_host, int Q, int32_t* info_out, const int32_t* pool_host, int n_pool, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    const int W = (c.vocab + 31) / 32;
    if (Q == 0) {                   // disarms and reads nothing else
        e->ban_armed = 0;
        e->ban_seq_armed = false;
        return info_out ? constrain_info(e, {0, 0, W, 0}, info_out, s) : 0;
    }
    if (frames) return fail("constrain: frames != NULL: constraints belong to the next search call, which brings its own images");
    if (image_of_host) return fail("constrain: image_of != NULL: row q of the table is sentence q of the call to be constrained");
    if (Q < 1 || Q > c.max_batch) return fail("constrain: Q=%d sentences outside [0,%d] (max_batch)", Q, c.max_batch);
    if (n_sets < 0 || n_sets > c.max_batch) return fail("constrain: %d ban sets (ld_prefix) outside [0,%d] (max_batch)", n_sets, c.max_batch);
    if (n_sets > 0 && !sets) return fail("constrain: %d ban sets, but a null pointer to their words (prefixes)", n_sets);
    if (!table_host || !info_out) return fail("constrain: null argument");
    if (c.max_text_len > 1024)      // the whole-row kernels keep the n-gram hits of a row in an LDS set of HIST_SLOTS / 2 tokens
        return fail("constrain: max_text_len %d: constrained searches support histories up to 1024 tokens", c.max_text_len);
    for (int q = 0; q < Q; ++q) {
        const int set = table_host[3 * q], min_new = table_host[3 * q + 1], ngram = table_host[3 * q + 2];
        if (set < -1 || set >= n_sets) return fail("constrain: sentence %d: set index %d outside [-1,%d)", q, set, n_sets);
        if (min_new < 0 || min_new > c.max_text_len) return fail("constrain: sentence %d: min_new %d outside [0,%d] (max_text_len)", q, min_new, c.max_text_len);
        if (ngram < 0 || ngram > 8) return fail("constrain: sentence %d: ngram %d outside [0,8]", q, ngram);
    }
    const size_t mb = (size_t)c.max_batch;
    BanPoolView pool;
    if (n_pool < 0) return fail("constrain: search->reserved_ = %d: 0, or the word count of the sequence pool in sent_out", n_pool);
    if (n_pool > 0) {
        if (!pool_host) return fail("constrain: search->reserved_ = %d words of banned sequences, but sent_out is NULL", n_pool);
        RCK(ban_pool_check("constrain", pool_host, n_pool, Q, c.vocab, c.max_batch, BAN_SEQ_MAX_SEQS, BAN_SEQ_MAX_TOKS, BAN_SEQ_MAX_LEN, &pool));
        if (W > BAN_ROW_MAX_WORDS)
            return fail("constrain: banned sequences need the %d words of a ban set in LDS, the kernel holds %d (vocabularies up to %d)",
                        W, BAN_ROW_MAX_WORDS, BAN_ROW_MAX_WORDS * 32);
    }
    if (!e->ban_words && hipMalloc((void**)&e->ban_words, (mb * W + 3 * mb) * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        e->ban_words = nullptr;
        return fail("constrain: out of device memory for the tables of the constraints");
    }
    if (!e->ban_stage) {
        hipError_t err = hipHostMalloc((void**)&e->ban_stage, (3 * mb + 4) * sizeof(int), hipHostMallocDefault);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&e->ban_staged, hipEventDisableTiming);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            if (e->ban_stage) hipHostFree(e->ban_stage);
            e->ban_stage = nullptr;
            return fail("constrain: out of page-locked memory for the staging buffer of the constraints");
        }
    }
    // the three buffers of the sequence rule: all of them or none
    if (n_pool > 0 && !e->ban_seq) {
        int *seq_tab = nullptr, *stage = nullptr; unsigned int* rows = nullptr;
        hipError_t err = hipMalloc((void**)&seq_tab, ban_seq_ints(e) * sizeof(int));
        if (err == hipSuccess) err = hipMalloc((void**)&rows, mb * c.max_beams * W * sizeof(int));
        if (err == hipSuccess) err = hipHostMalloc((void**)&stage, ban_seq_ints(e) * sizeof(int), hipHostMallocDefault);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            hipFree(seq_tab); hipFree(rows);
            return fail("constrain: out of memory for the tables of the banned sequences");
        }
        e->ban_seq = seq_tab; e->ban_row_words = rows; e->ban_seq_stage = stage;
    }
    // No synchronisation with the work in flight: the table travels through a page-locked staging buffer as a copy ON `s`, behind
    // whatever on `s` still reads the tables.  The host waits only for the previous arming call's own copy to have left the buffer.
    HIPCK(hipEventSynchronize(e->ban_staged));
    e->ban_armed = 0;               // from here on the tables are being overwritten: a copy that fails leaves the context disarmed
    int* tab = e->ban_stage;
    for (size_t q = 0; q < mb; ++q) {
        const bool in = q < (size_t)Q;
        tab[q] = in ? table_host[3 * q] : -1; tab[mb + q] = in ? table_host[3 * q + 1] : 0; tab[2 * mb + q] = in ? table_host[3 * q + 2] : 0;
    }
    HIPCK(hipMemcpyAsync(e->ban_words + mb * W, tab, 3 * mb * sizeof(int), hipMemcpyHostToDevice, s));
    if (n_sets > 0) HIPCK(hipMemcpyAsync(e->ban_words, sets, (size_t)n_sets * W * sizeof(int), hipMemcpyDeviceToDevice, s));
    e->ban_seq_armed = false;
    if (n_pool > 0) {               // the pool's four arrays, each into its fixed region of the staging twin and from there on `s`
        const BanSeqArgs at = ban_seq_args(e);
        const int* src[4] = {pool.list_of, pool.list_off, pool.seq_off, pool.tok};
        const int* dst[4] = {at.list_of, at.list_off, at.seq_off, at.tok};
        const size_t cnt[4] = {(size_t)Q, (size_t)pool.L + 1, (size_t)pool.S + 1, (size_t)pool.T};
        for (int i = 0; i < 4; ++i) {
            if (!cnt[i]) continue;
            int* st = e->ban_seq_stage + (dst[i] - e->ban_seq);
            memcpy(st, src[i], cnt[i] * sizeof(int));
            HIPCK(hipMemcpyAsync(const_cast<int*>(dst[i]), st, cnt[i] * sizeof(int), hipMemcpyHostToDevice, s));
        }
    }
    RCK(constrain_info(e, {Q, n_sets, W, 0}, info_out, s));
    e->ban_armed = Q;
    e->ban_seq_armed = n_pool > 0;
    return 0;
}
// A search call of Q sentences meets the arming: disarmed -> it runs plain; armed for Q -> it will run constrained (generate_run
// consumes the arming); anything else is refused and stays armed.  Changes nothing: the last argument check of a search call.
static int constrain_check(const gitmi_engine* e, const char* who, const gitmi_search* sp, int Q, bool* constrained) {
    *constrained = false;
    if (!e->ban_armed) return 0;
    if (sp->kind == GITMI_SEARCH_TRIE)
        return fail("%s: GITMI_SEARCH_TRIE while decoding constraints are armed (GITMI_SEARCH_CONSTRAIN): constraints on the trie search "
                    "are not implemented -- disarm first (a GITMI_SEARCH_CONSTRAIN call with Q == 0)", who);
    if (Q != e->ban_armed)
        return fail("%s: decoding constraints are armed for %d sentences, this call has %d (they stay armed: run the call they were "
                    "armed for, arm again, or disarm with Q == 0)", who, e->ban_armed, Q);
    *constrained = true;
    return 0;
}

// ---- per-token trace (GITMI_SEARCH_TRACE, include/gitmi.h) -------------------------------------------------------------------
// Arms the trace of the NEXT search call of this context: its shape (Q sentences x nout sequences, T positions, n alternatives)
// and the caller's output buffers.  Every check comes before the first change, so a refused call leaves the arming as it was.
static int trace_call(gitmi_engine* e, const float* const* frames, const int64_t* prefixes, const int32_t* prefix_len_host,
                      const int32_t* image_of_host, int Q, const gitmi_search* sp, int64_t* tokens_out, float* logprob_out,
                      int32_t* info_out, hipStream_t s) {
    const gitmi_config& c = e->cfg;
    if (Q == 0) {
        e->trace_armed = 0;
        return info_out ? memory_info({0, 0, 0, 0}, info_out, s) : 0;
    }
    if (e->trace_live)
        return fail("trace: a traced seam search is in progress (gitmi_search_begin without gitmi_search_finish): its log is carved by "
                    "the arming it consumed -- finish it, or begin another search, before arming again");
    if (frames) return fail("trace: frames != NULL: the trace belongs to the next search call, which brings its own images");
    if (prefixes) return fail("trace: prefixes != NULL: the call to be traced brings its own");
    if (prefix_len_host) return fail("trace: prefix_len_host != NULL: the call to be traced brings its own");
    if (image_of_host) return fail("trace: image_of != NULL: the call to be traced brings its own");
    if (Q < 1 || Q > c.max_batch) return fail("trace: Q=%d sentences outside [0,%d] (max_batch)", Q, c.max_batch);
    if (sp->num_keep_best < 0 || sp->num_keep_best > SS_NHMAX)
        return fail("trace: search->num_keep_best %d outside [0,%d]", sp->num_keep_best, SS_NHMAX);
    if (sp->max_steps < 1 || sp->max_steps > c.max_text_len)
        return fail("trace: search->max_steps %d outside [1,%d] (max_text_len)", sp->max_steps, c.max_text_len);
    const int n = sp->reserved_, nout = keep_best(*sp), T = sp->max_steps;
    if (n < 0 || n > TRACE_NMAX) return fail("trace: search->reserved_ = %d alternatives outside [0,%d]", n, TRACE_NMAX);
    if (n >= c.vocab) return fail("trace: search->reserved_ = %d alternatives, the vocabulary has %d tokens", n, c.vocab);
    if (!logprob_out) return fail("trace: logprob_out is NULL (fp32 [Q * nout][T][1 + n])");
    if (n > 0 && !tokens_out) return fail("trace: tokens_out is NULL with search->reserved_ = %d alternatives (int64 [Q * nout][T][n])", n);
    const TraceLayout L = trace_layout(e, Q, nout, T, n);
    if (L.total > e->trace_bytes) {
        // captured traced graphs hold pointers into the old allocation, a traced search in flight writes it
        HIPCK(hipDeviceSynchronize());
        char* buf = nullptr;
        if (hipMalloc((void**)&buf, L.total) != hipSuccess) {
            (void)hipGetLastError();
            return fail("trace: out of device memory for the log of the trace (%zu bytes)", L.total);
        }
        for (CapturedGraph* g : {&e->graphs[1].graph_full, &e->graphs[1].graph_decode, &e->graphs[1].graph_follow}) g->reset();
        e->graphs[1].full_slot.valid = e->graphs[1].follow_slot.valid = false;
        hipFree(e->trace_buf);
        e->trace_buf = buf; e->trace_bytes = L.total;
    }
    if (info_out) RCK(memory_info({Q, nout, T, n}, info_out, s));       // (waits for the stream; NULL: the host does not wait)
    e->trace_armed = e->trace_Q = Q; e->trace_nout = nout; e->trace_T = T; e->trace_n = n;
    e->trace_user_lp = logprob_out; e->trace_user_tok = (long long*)tokens_out;
    return 0;
}
// A search call of Q sentences meets the arming: disarmed -> it runs plain; armed for its shape -> it will run traced (generate_run
// or the seam's begin consumes the arming); anything else is refused and stays armed.  Changes nothing.
static int trace_check(const gitmi_engine* e, const char* who, const gitmi_search* sp, int Q, bool* traced) {
    *traced = false;
    if (!e->trace_armed) return 0;
    if (sp->kind == GITMI_SEARCH_TRIE)
        return fail("%s: GITMI_SEARCH_TRIE while the per-token trace is armed (GITMI_SEARCH_TRACE): traces of the trie search are not "
                    "implemented -- disarm first (a GITMI_SEARCH_TRACE call with Q == 0)", who);
    if (sp->do_sample && e->trace_n > 0)
        return fail("%s: do_sample while the per-token trace is armed with %d alternatives (GITMI_SEARCH_TRACE): alternatives under "
                    "sampling are not implemented -- arm with search->reserved_ = 0, or disarm with Q == 0", who, e->trace_n);
    if (Q != e->trace_armed)
        return fail("%s: the per-token trace is armed for %d sentences, this call has %d (it stays armed: run the call it was armed "
                    "for, arm again, or disarm with Q == 0)", who, e->trace_armed, Q);
    const int nout = sp->kind == GITMI_SEARCH_GENERATOR ? keep_best(*sp) : 1;
    if (nout != e->trace_nout)
        return fail("%s: the per-token trace is armed for %d sequences per sentence (num_keep_best), this call returns %d (it stays "
                    "armed)", who, e->trace_nout, nout);
    if (sp->max_steps != e->trace_T)
        return fail("%s: the per-token trace is armed for max_steps %d, this call has %d (it stays armed)", who, e->trace_T, sp->max_steps);
    *traced = true;
    return 0;
}

// Q sentences with their own prefixes over B encoded images (batched VQA: the questions of one image share its K/V)
extern "C" int gitmi_generate_prefixed(gitmi_engine* e, const float* const* frames, int F, int B, const int64_t* prefixes,
                                       int ld_prefix, const int32_t* prefix_len_host, const int32_t* image_of_host, int Q,
                                       const gitmi_search* sp, int64_t* tokens_out, float* logprob_out,
                                       int32_t* sent_out, int32_t* info_out, void* stream) {
    RCK(check_ready(e));
    const gitmi_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    SentenceSpan span;
    if (sp && sp->kind == GITMI_SEARCH_CONTEXT)
        return context_call(e, frames, F, B, (const long long*)prefixes, ld_prefix, prefix_len_host, image_of_host, Q, info_out, s);
    if (sp && sp->kind == GITMI_SEARCH_KEEP)
        return memory_keep(e, frames, B, logprob_out, ld_prefix, prefix_len_host, image_of_host, Q, info_out, s);
    if (sp && sp->kind == GITMI_SEARCH_RECALL)
        return memory_recall(e, frames, B, prefixes, ld_prefix, prefix_len_host, image_of_host, Q, info_out, s);
    if (sp && sp->kind == GITMI_SEARCH_CONSTRAIN)
        return constrain_call(e, frames, (const unsigned int*)prefixes, ld_prefix, prefix_len_host, image_of_host, Q, info_out, sent_out,
                              sp->reserved_, s);
    if (sp && sp->kind == GITMI_SEARCH_TRACE)
        return trace_call(e, frames, prefixes, prefix_len_host, image_of_host, Q, sp, tokens_out, logprob_out, info_out, s);
    if (sp && sp->kind == GITMI_SEARCH_FEATURES)
        return features_call(e, frames, F, B, prefixes, sp->reserved_, ld_prefix, prefix_len_host, image_of_host, Q, info_out, s);
    if (sp && (sp->kind == GITMI_SEARCH_SCORE || sp->kind == GITMI_SEARCH_ATTEND || sp->kind == GITMI_SEARCH_TREE_SCORE)) {
        const bool attend = sp->kind == GITMI_SEARCH_ATTEND, tree = sp->kind == GITMI_SEARCH_TREE_SCORE;
        const char* who = attend ? "attend" : tree ? "tree_score" : "score";
        if (!frames) RCK(check_resident(e, who, B));
        if (attend && !frames && e->has_context)
            return fail("attend: the resident images carry context rows; the attention map over [image | context | text] columns "
                        "is not implemented (run the attend call with frames, or encode without context)");
        if (!logprob_out || !info_out || !prefixes || !prefix_len_host) return fail("%s: null argument", who);
        if (frames) RCK(check_frames(e, who, frames, F, B));
        // sentences are bounded by max_text_len positions; a tree by its depths (checked on the device) and the row cap
        if (tree && tree_max_depth(c) > 8192)
            return fail("tree_score: the depth bound min(max_text_len, max_pos) = %d exceeds the 8192 entries of the structure walk's "
                        "root path", tree_max_depth(c));
        const int ld_max = tree ? TREE_MAX_ROWS : c.max_text_len;
        if (ld_prefix < 1 || ld_prefix > ld_max)
            return fail("%s: ld=%d outside [1,%d] (%s)", who, ld_prefix, ld_max, tree ? "the row cap of a tree call" : "max_text_len");
        RCK(read_sentences(e, who, prefix_len_host, image_of_host, ld_prefix, B, Q, c.max_batch * c.max_beams,
                           "max_batch x max_beams", &span));
        const int Lp = round_up(span.maxP, 16);
        if (tree && (size_t)Q * Lp > (size_t)TREE_MAX_ROWS)
            return fail("tree_score: %d trees x %d padded nodes = %zu rows above the cap of %d rows per call", Q, Lp, (size_t)Q * Lp,
                        TREE_MAX_ROWS);
        RCK(score_alloc(e, (size_t)Q * Lp, tree ? (size_t)Q * ld_prefix : 0));
        if (attend)
            RCK(attend_alloc(e, (size_t)Q * ld_prefix * c.dec_layers * (call_Nimg(e, frames, F) + ld_prefix),
                             (size_t)Q * c.dec_heads * Lp));
        RCK(upload_sentences(e, e->sc_lens, e->sc_img, s));
        if (frames) RCK(ragged_prepare(e, frames, F, B, s));
        // the sentences are whole captions of lengths [minP, maxP]; logprob_out receives (lp, mean_lp) per position, or the maps
        const Request rq{frames, F, B, Q, span.minP, span.maxP, true, sp, nullptr, logprob_out, info_out, e->out_sent};
        const long long* tokens = (const long long*)prefixes;
        return settle_residency(e, rq, text_pass_impl(e, rq, tokens, ld_prefix, s));
    }
    if (!frames) RCK(check_resident(e, "generate_prefixed", B));
    if (!sp || !tokens_out || !logprob_out || !info_out || !prefixes || !prefix_len_host)
        return fail("generate_prefixed: null argument");
    if (frames) RCK(check_frames(e, "generate_prefixed", frames, F, B));
    RCK(read_sentences(e, "generate_prefixed", prefix_len_host, image_of_host, ld_prefix, B, Q, c.max_batch, "max_batch", &span));
    if (sp->max_steps < span.maxP || sp->max_steps > c.max_text_len)
        return fail("generate_prefixed: max_steps %d outside [%d,%d]", sp->max_steps, span.maxP, c.max_text_len);
    bool constrained = false;
    RCK(constrain_check(e, "generate_prefixed", sp, Q, &constrained));
    bool traced = false;
    RCK(trace_check(e, "generate_prefixed", sp, Q, &traced));
    RCK(upload_sentences(e, e->plen_dev, e->img_of_dev, s));
    HIPCK(hipMemcpy2D(e->start_dev, (size_t)c.max_text_len * sizeof(long long), prefixes, (size_t)ld_prefix * sizeof(long long),
                      (size_t)span.maxP * sizeof(long long), (size_t)Q, hipMemcpyDeviceToDevice));
    e->img_identity = span.ident;
    if (frames) RCK(ragged_prepare(e, frames, F, B, s));
    const Request rq{frames, F, B, Q, span.minP, span.maxP, true, sp, (long long*)tokens_out, logprob_out, info_out,
                     sent_out ? sent_out : e->out_sent};
    return generate_run(e, rq, s, constrained, traced);
}

// ---- profiling --------------------------------------------------------------------------
extern "C" int gitmi_profile_enable(gitmi_engine* e, int on) {
    if (!e) return fail("null engine");
    e->profile_mode = on;
    e->profiling = on == 1;
    e->split_encode_ms = e->split_decode_ms = 0; e->split_calls = e->split_steps = 0;
    e->spans.clear();
    e->event_next = 0;
    return 0;
}
// Serving schedule for several contexts on one device: `e`'s image encoder (+ decoder prefill) of a gitmi_generate call
// starts only after the encoder of `after`'s most recently submitted call has finished; the decode steps are not
// ordered.  Chain the contexts in a ring in submission order: at most one MFMA-bound encoder runs at a time and the
// latency-bound decode chains of the other contexts fill in beside it.  after == NULL removes the dependency.
static void unlink_encode_after(gitmi_engine* e) {
    if (!e->enc_after) return;
    auto& w = e->enc_after->enc_watchers;
    w.erase(std::remove(w.begin(), w.end(), e), w.end());
    e->enc_after = nullptr;
}
extern "C" int gitmi_set_encode_after(gitmi_engine* e, gitmi_engine* after) {
    if (!e) return fail("null engine");
    if (after == e) return fail("set_encode_after: a context cannot wait for its own encoder");
    HIPCK(hipSetDevice(e->device));
    unlink_encode_after(e);
    if (after) {
        if (!after->enc_done) HIPCK(hipEventCreateWithFlags(&after->enc_done, hipEventDisableTiming));
        after->enc_watchers.push_back(e);
        e->enc_after = after;
    }
    return 0;
}

// CaptioningModel.forward_one adds img_temperal_embedding[i] only when batch['image'] is a LIST of frames
// (decoder.py:845-857); a bare tensor goes through image_encoder alone, also on a video model.
extern "C" int gitmi_set_temporal_embedding(gitmi_engine* e, int on) {
    if (!e) return fail("null engine");
    if ((on != 0) != e->pol.use_temb) { e->pol.use_temb = on != 0; drop_resident(e); }
    return 0;
}
// Serving policy: other contexts keep the device busy beside this one.  Kernel shapes are then chosen for what they cost
// the device as a whole rather than for their own duration: the encoder GEMMs take the 256-row tile even where it leaves
// a partial round (the idle CUs are filled by the other contexts), the N = 768 GEMMs of the decode chain take 64 rows per
// workgroup, the decode attention packs 8 (sentence, head) pairs per workgroup.  Results are bit-identical either way.
extern "C" int gitmi_set_shared_device(gitmi_engine* e, int on) {
    if (!e) return fail("null engine");
    if ((on != 0) != e->pol.shared_device) {
        HIPCK(hipSetDevice(e->device));
        HIPCK(hipDeviceSynchronize());
        e->pol.shared_device = on != 0;
        destroy_graph(e);
    }
    return 0;
}
// LayerNorm folding of the encoder / prefill passes (fp16-operand build, on by default there): off = every LayerNorm is a launch
// that materialises its output, as in the bf16 build.  Results differ by rounding only (one rounding of the normalised
// rows less with the fold); the switch exists for A/B timing and for the parity tests that hold both forms to the same bound.
extern "C" int gitmi_set_ln_fold(gitmi_engine* e, int on) {
    if (!e) return fail("null engine");
    if (on && !e->pol.ln_fold_ready)
        return fail("gitmi_set_ln_fold: not available (needs the fp16-operand library, the 16-bit engine mode and hidden sizes that are multiples of 256)");
    if ((on != 0) != e->pol.ln_fold) {
        HIPCK(hipSetDevice(e->device));
        HIPCK(hipDeviceSynchronize());
        e->pol.ln_fold = on != 0;
        drop_resident(e);
        destroy_graph(e);
    }
    return 0;
}
extern "C" int gitmi_set_graph(gitmi_engine* e, int on) {
    if (!e) return fail("null engine");
    e->pol.use_graph = on != 0;
    return 0;
}
extern "C" int gitmi_profile_read(gitmi_engine* e, gitmi_profile* out) {
    if (!e || !out) return fail("null argument");
    HIPCK(hipSetDevice(e->device));
    HIPCK(hipDeviceSynchronize());
    memset(out, 0, sizeof(*out));
    if (e->profile_mode == 2) {
        // graph-replay timing: (encode + prefill) graph and decode graph of every call since enable, averaged per call
        const double n = e->split_calls ? (double)e->split_calls : 1.0;
        out->vit_ms = (float)(e->split_encode_ms / n);            // encode + prefill together (one graph)
        out->decode_ms = (float)(e->split_decode_ms / n);
        out->total_ms = out->vit_ms + out->decode_ms;
        out->decode_steps = e->split_calls ? e->split_steps / e->split_calls : 0;
        out->decode_step_ms = e->split_steps ? (float)(e->split_decode_ms / e->split_steps) : 0.f;
        out->decode_step_bytes = e->last_decode_step_bytes;
        e->split_encode_ms = e->split_decode_ms = 0; e->split_calls = e->split_steps = 0;
        return 0;
    }
    double step_ms = 0;
    for (const TimedSpan& sp : e->spans) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, sp.a, sp.b) != hipSuccess) continue;
        switch (sp.tag) {
            case TAG_VIT: out->vit_ms += ms; break;
            case TAG_PREFILL: out->prefill_ms += ms; break;
            case TAG_DECODE: out->decode_ms += ms; break;
            case 99: out->total_ms += ms; break;
            case TAG_STEP: step_ms += ms; out->decode_steps += 1; break;
            case TAG_GEMM_VIT:
                out->vit_gemm_ms += ms; out->vit_gemm_launches += 1; out->vit_gemm_flops += sp.flops;
                // fallthrough
            case TAG_GEMM_OTHER:
                out->gemm_ms += ms; out->gemm_launches += 1; out->gemm_flops += sp.flops;
                break;
            default: break;
        }
    }
    out->decode_step_ms = out->decode_steps ? (float)(step_ms / out->decode_steps) : 0.f;
    out->decode_step_bytes = e->last_decode_step_bytes;
    e->spans.clear();
    e->event_next = 0;
    return 0;
}

// ---- error attribution hooks (tools/error_attribution.py): hand the products of a stage from one context to another
// of the SAME model in the other precision, so that a stage can be switched between bf16 and fp32 on its own.
//   stage 1: visual features (image encoder output)        -> dst runs prefill + decode itself
//   stage 2: + the image K/V of every decoder layer (prefill) -> dst runs only the decode steps itself
GITMI_EXP_EXPORT int gitmi_debug_import_stage(gitmi_engine* dst, gitmi_engine* src, int stage, void* stream) {
    RCK(check_ready(dst));
    if (!src || !src->finalized) return fail("debug_import_stage: bad source");
    if (stage != 1 && stage != 2) return fail("debug_import_stage: stage must be 1 or 2");
    const gitmi_config &a = dst->cfg, &b = src->cfg;
    if (a.vit_width != b.vit_width || a.dec_hidden != b.dec_hidden || a.dec_layers != b.dec_layers || a.dec_heads != b.dec_heads)
        return fail("debug_import_stage: the two contexts are different models");
    if (!src->have_feats || (stage == 2 && !src->have_prefill)) return fail("debug_import_stage: the source has not run that stage");
    if (src->has_context) return fail("debug_import_stage: the source's resident images carry context rows");
    if (src->cur_B > a.max_batch || src->cur_F > a.max_frames || src->N != dst->N) return fail("debug_import_stage: capacity / resolution mismatch");
    hipStream_t s = (hipStream_t)stream;
    const size_t M = (size_t)src->cur_B * src->cur_Nimg;
    HIPCK(launch_convert(src->feats, src->pol.f32, dst->feats, dst->pol.f32, M * a.vit_width, s));
    set_resident(dst, src->cur_B, src->cur_F);      // src->N == dst->N: the same cur_Nimg
    if (stage == 2) {
        for (int l = 0; l < a.dec_layers; ++l) {
            HIPCK(launch_convert(src->img_kv[l], src->pol.f32, dst->img_kv[l], dst->pol.f32, M * 3 * a.dec_hidden, s));
            RCK(kv_repack(dst, l, dst->cur_B, dst->cur_Nimg, s));
        }
        set_prefilled(dst);
    }
    return 0;
}
// the vocabulary head of `dst` (bf16: the fused, LayerNorm-folded head) applied to the last hidden state that `src`
// (an fp32 context) computed in its most recent gitmi_step_logits over R rows: logits_out fp32 [R, vocab] (device)
GITMI_EXP_EXPORT int gitmi_debug_head_from(gitmi_engine* dst, gitmi_engine* src, int R, float* logits_out, void* stream) {
    RCK(check_ready(dst));
    if (!src || !src->pol.f32 || !logits_out) return fail("debug_head_from: the source must be an fp32 context");
    if (dst->pol.f32 || !dst->pol.skinny) return fail("debug_head_from: the destination must run the bf16 decode chain");
    const gitmi_config& c = dst->cfg;
    if (c.dec_hidden != src->cfg.dec_hidden || c.vocab != src->cfg.vocab) return fail("debug_head_from: different models");
    if (R < 1 || R > c.max_batch * c.max_beams) return fail("debug_head_from: R outside the capacity");
    hipStream_t s = (hipStream_t)stream;
    HIPCK(launch_chain_input(src->d_y, dst->xo_b, dst->stats_o, R, c.dec_hidden, s));   // d_y: pre-LayerNorm sum of the last layer
    StepCands cands{};
    return decode_head_impl(dst, nullptr, c.max_text_len, 1, R, 1, 0, 1, logits_out, c.vocab, s, &cands);
}