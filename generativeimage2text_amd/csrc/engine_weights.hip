// Weight side of the GIT engine: ingest of the checkpoint's tensors, upload / repack, the LayerNorm folds, clones that
// borrow the packed weights, and the workspaces every context owns.
#include "engine_state.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace gitmi;

// ---------------------------------------------------------------------------------------
static int dev_alloc(gitmi_engine* e, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    HIPCK(hipMalloc(p, bytes));
    e->allocs.push_back(*p);
    return 0;
}
template <typename T> static int dev_alloc_t(gitmi_engine* e, T** p, size_t count) {
    return dev_alloc(e, reinterpret_cast<void**>(p), count * sizeof(T));
}

// ---------------------------------------------------------------------------------------
static float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000) << 16;
    uint32_t exp = (h >> 10) & 0x1f, man = h & 0x3ff, out;
    if (exp == 0) {
        if (man == 0) out = sign;
        else {
            exp = 127 - 15 + 1;
            while (!(man & 0x400)) { man <<= 1; --exp; }
            man &= 0x3ff;
            out = sign | (exp << 23) | (man << 13);
        }
    } else if (exp == 31) out = sign | 0x7f800000u | (man << 13);
    else out = sign | ((exp + 127 - 15) << 23) | (man << 13);
    float f;
    memcpy(&f, &out, 4);
    return f;
}

extern "C" int gitmi_load_tensor(gitmi_engine* e, const char* key, const void* data_host, const int64_t* shape,
                                 int ndim, int dtype) {
    if (!e || !key || !data_host || (ndim > 0 && !shape)) return fail("gitmi_load_tensor: null argument");
    if (e->finalized) return fail("gitmi_load_tensor: weights already finalized");
    std::string k(key);
    if (k.rfind("module.", 0) == 0) k = k.substr(7);          // torch_common.py:95-99 strips DataParallel prefixes
    if (k == "image_encoder.proj") return 0;                   // unused with output_grid=True
    const bool known = k.rfind("image_encoder.", 0) == 0 || k.rfind("textual.", 0) == 0 ||
                       k.rfind("img_temperal_embedding.", 0) == 0;
    if (!known) return fail("gitmi_load_tensor: unknown key '%s'", key);
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    const size_t n = t.numel();
    t.data.resize(n);
    if (dtype == GITMI_DTYPE_F32) memcpy(t.data.data(), data_host, n * 4);
    else if (dtype == GITMI_DTYPE_BF16) {
        const uint16_t* p = (const uint16_t*)data_host;
        for (size_t i = 0; i < n; ++i) { uint32_t u = (uint32_t)p[i] << 16; memcpy(&t.data[i], &u, 4); }
    } else if (dtype == GITMI_DTYPE_F16) {
        const uint16_t* p = (const uint16_t*)data_host;
        for (size_t i = 0; i < n; ++i) t.data[i] = half_to_float(p[i]);
    } else return fail("gitmi_load_tensor: bad dtype %d", dtype);
    // a checkpoint with inf / NaN in it fails here, by name, not as garbage ids later
    float amax = 0.f;
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(t.data[i])) return fail("gitmi_load_tensor: '%s' holds a non-finite value at element %zu", key, i);
        amax = std::max(amax, std::fabs(t.data[i]));
    }
    t.amax = amax;
    e->host_w[k] = std::move(t);
    return 0;
}

static int get_w(gitmi_engine* e, const std::string& key, std::initializer_list<int64_t> shape, const HostTensor** out) {
    auto it = e->host_w.find(key);
    if (it == e->host_w.end()) return fail("missing weight '%s'", key.c_str());
    size_t want = 1;
    for (auto s : shape) want *= (size_t)s;
    if (it->second.numel() != want) return fail("weight '%s' has %zu elements, expected %zu", key.c_str(), it->second.numel(), want);
    *out = &it->second;
    return 0;
}
// fp32 vector / table on device
static int up_f32(gitmi_engine* e, const std::string& key, std::initializer_list<int64_t> shape, float** dst) {
    const HostTensor* t;
    RCK(get_w(e, key, shape, &t));
    RCK(dev_alloc_t(e, dst, t->numel()));
    HIPCK(hipMemcpy(*dst, t->data.data(), t->numel() * 4, hipMemcpyHostToDevice));
    return 0;
}
// a MATRIX that becomes an MFMA operand must fit the operand format: fp16 tops out at 65504 (bf16 and f32 share fp32's exponent)
static int operand_range_check(gitmi_engine* e, const char* what, float amax) {
#ifdef GITMI_OPS_F16
    if (!e->pol.f32 && amax > 65504.f)
        return fail("'%s': max |w| = %g is outside the fp16 operand range (65504): load this checkpoint with precision "
                    "\"bf16\" or \"f32\"", what, (double)amax);
#endif
    (void)e; (void)what; (void)amax;
    return 0;
}
// matrix [rows, K] -> compute dtype [rows, Kpad]
static int up_mat(gitmi_engine* e, const std::string& key, int64_t rows, int K, int Kpad, void** dst) {
    const HostTensor* t;
    RCK(get_w(e, key, {rows, (int64_t)K}, &t));
    RCK(operand_range_check(e, key.c_str(), t->amax));
    RCK(dev_alloc(e, dst, (size_t)rows * Kpad * e->pol.esz));
    float* tmp = nullptr;
    HIPCK(hipMalloc((void**)&tmp, t->numel() * 4));
    hipError_t err = hipMemcpy(tmp, t->data.data(), t->numel() * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_convert_pad(tmp, *dst, e->pol.f32, (size_t)rows, K, Kpad, 0);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    hipFree(tmp);
    HIPCK(err);
    return 0;
}

void gitmi::init_geometry(gitmi_engine* e) {
    const gitmi_config& c = e->cfg;
    e->g_nat = e->gh = e->gw = c.image_size / c.patch;
    e->N_nat = e->N = e->g_nat * e->g_nat + 1;
    e->H = e->W = c.image_size;
    e->Nmax = std::max(e->N_nat, c.max_image_tokens);
    e->max_pixels = std::max((size_t)c.image_size * c.image_size, (size_t)c.max_image_pixels);
    e->Kp = 3 * c.patch * c.patch;
    e->Kp_pad = round_up(e->Kp, 64);
    e->pos_cur = e->w.pos;
}

static int alloc_workspaces(gitmi_engine* e) {
    const gitmi_config& c = e->cfg;
    const size_t esz = e->pol.esz;
    const int D = c.vit_width, d = c.dec_hidden;
    const size_t Mv = (size_t)c.max_batch * c.max_frames * e->Nmax;  // ViT rows: all frames of a call in one pass
    const size_t Mp = (size_t)c.max_batch * c.max_frames * e->Nmax;  // prefill rows
    // fragment-major operand buffers hold whole 16-row tiles, and the wide chain GEMMs / the vocabulary head load their
    // activations four tiles (64 rows) at a time whatever M is: every row-sized buffer is padded to 64 rows
    const size_t R = (size_t)round_up(c.max_batch * c.max_beams, 64);
    const int T = c.max_text_len;
    RCK(dev_alloc(e, &e->patches, (size_t)c.max_batch * c.max_frames * (e->Nmax - 1) * e->Kp_pad * esz));
    RCK(dev_alloc_t(e, &e->patch_out, (size_t)c.max_batch * c.max_frames * (e->Nmax - 1) * D));
    RCK(dev_alloc_t(e, &e->pos_var, (size_t)e->Nmax * D));
    RCK(dev_alloc_t(e, &e->v_x, Mv * D));
    RCK(dev_alloc(e, &e->v_h, Mv * D * esz));
    RCK(dev_alloc(e, &e->v_qkv, Mv * 3 * D * esz));
    RCK(dev_alloc(e, &e->v_ctx, Mv * D * esz));
    RCK(dev_alloc(e, &e->v_u, Mv * 4 * D * esz));
    RCK(dev_alloc(e, &e->feats, Mp * D * esz));
    if (e->pol.ln_fold_ready) {
        // [row][4] (sum, sumsq) per 256-column tile; slots past the row width stay zero for ever
        RCK(dev_alloc_t(e, &e->v_part, Mv * 4));
        RCK(dev_alloc_t(e, &e->p_part[0], Mp * 4));
        RCK(dev_alloc_t(e, &e->p_part[1], Mp * 4));
        HIPCK(hipMemset(e->v_part, 0, Mv * 4 * sizeof(float2)));
        HIPCK(hipMemset(e->p_part[0], 0, Mp * 4 * sizeof(float2)));
        HIPCK(hipMemset(e->p_part[1], 0, Mp * 4 * sizeof(float2)));
    }
    RCK(dev_alloc_t(e, &e->p_y, Mp * d));
    RCK(dev_alloc_t(e, &e->p_hf, Mp * d));
    RCK(dev_alloc(e, &e->p_ht, Mp * d * esz));
    RCK(dev_alloc(e, &e->p_ctx, Mp * d * esz));
    RCK(dev_alloc(e, &e->p_u, Mp * c.dec_ffn * esz));
    e->img_kv.resize(c.dec_layers);
    e->img_kh.resize(c.dec_layers);
    e->img_vh.resize(c.dec_layers);
    e->txt_k.resize(c.dec_layers);
    e->txt_v.resize(c.dec_layers);
    for (int l = 0; l < c.dec_layers; ++l) {
        RCK(dev_alloc(e, &e->img_kv[l], Mp * 3 * d * esz));
        // decode layout; bf16: per (image, head) keys padded to a multiple of 32 (kernels_attn_decode.hip)
        const size_t Mkv = (size_t)c.max_batch * round_up(c.max_frames * e->Nmax, 32);
        RCK(dev_alloc(e, &e->img_kh[l], Mkv * d * esz));
        RCK(dev_alloc(e, &e->img_vh[l], Mkv * d * esz));
        RCK(dev_alloc(e, &e->txt_k[l], R * T * d * esz));
        RCK(dev_alloc(e, &e->txt_v[l], R * T * d * esz));
    }
    RCK(dev_alloc_t(e, &e->d_y, R * d));
    RCK(dev_alloc_t(e, &e->d_hf, R * d));
    RCK(dev_alloc(e, &e->d_ht, R * d * esz));
    RCK(dev_alloc(e, &e->d_qkv, R * 3 * d * esz));
    RCK(dev_alloc(e, &e->d_ctx, R * d * esz));
    RCK(dev_alloc(e, &e->d_u, R * c.dec_ffn * esz));
    RCK(dev_alloc_t(e, &e->xa_f, R * d));
    RCK(dev_alloc_t(e, &e->xo_f, R * d));
    RCK(dev_alloc(e, &e->xa_b, R * d * 2));
    RCK(dev_alloc(e, &e->xo_b, R * d * 2));
    RCK(dev_alloc_t(e, &e->stats_a, R * (size_t)(d / 16)));
    RCK(dev_alloc_t(e, &e->stats_o, R * (size_t)(d / 16)));
    e->ldl = round_up(c.vocab, 8);
    RCK(dev_alloc_t(e, &e->logits, R * e->ldl));
    // candidate lists of a step: the fused vocabulary head writes one list per (row, 128-column workgroup)
    e->vocab_cols = 128;                  // columns per workgroup of the fused head (239 workgroups for the 30522-token vocabulary)
    // only the bf16 decode chain uses the fused head (finalize_weights turns the chain off for vocabularies above 32768
    // tokens); f32 engines and search-only contexts get ONE list per row from row_topm / sample_rows
    e->vocab_nparts = (e->pol.skinny && !e->pol.f32) ? vocab_parts(c.vocab, e->vocab_cols) : 1;
    RCK(dev_alloc_t(e, &e->part_val, R * (size_t)e->vocab_nparts * 16));
    RCK(dev_alloc_t(e, &e->part_idx, R * (size_t)e->vocab_nparts * 16));
    RCK(dev_alloc_t(e, &e->part_lse, R * (size_t)e->vocab_nparts));
    // search state
    SearchState& s = e->ss;
    for (int i = 0; i < 2; ++i) {
        RCK(dev_alloc_t(e, &s.ids[i], R * T));
        RCK(dev_alloc_t(e, &s.kv_src[i], R * T));
        RCK(dev_alloc_t(e, &s.score[i], R));
    }
    RCK(dev_alloc_t(e, &s.done, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &s.hyp_n, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &s.hyp_cnt, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &s.hyp_worst, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &s.hyp_score, (size_t)c.max_batch * SS_NHMAX));
    RCK(dev_alloc_t(e, &s.hyp_len, (size_t)c.max_batch * SS_NHMAX));
    RCK(dev_alloc_t(e, &s.hyp_seq, (size_t)c.max_batch * SS_NHMAX));
    RCK(dev_alloc_t(e, &s.hyp_tok, (size_t)c.max_batch * SS_NHMAX * T));
    RCK(dev_alloc_t(e, &s.stop, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &s.early, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &s.info, 4));
    RCK(dev_alloc_t(e, &s.len_norm, (size_t)T + 1));
    RCK(dev_alloc_t(e, &e->start_dev, (size_t)c.max_batch * T));
    RCK(dev_alloc_t(e, &e->plen_dev, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &e->img_of_dev, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &e->trie_cursor, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &e->out_tokens, (size_t)c.max_batch * SS_NHMAX * T));
    RCK(dev_alloc_t(e, &e->out_lp, (size_t)c.max_batch * SS_NHMAX));
    RCK(dev_alloc_t(e, &e->out_info, 4));
    RCK(dev_alloc_t(e, &e->out_sent, (size_t)c.max_batch * 2));
    HIPCK(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
    HIPCK(hipEventCreateWithFlags(&e->fence_in, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&e->fence_out, hipEventDisableTiming));
    e->frame_stage.resize(c.max_frames);
    for (int f = 0; f < c.max_frames; ++f)
        RCK(dev_alloc_t(e, &e->frame_stage[f], (size_t)c.max_batch * 3 * e->max_pixels));
    RCK(dev_alloc_t(e, &e->rg_meta, (size_t)c.max_batch));
    RCK(dev_alloc_t(e, &e->rg_ntok, (size_t)c.max_batch));
    return 0;
}

// ---- LayerNorm folding for the decode chain (kernels_dgemm.hip) ------------------------------------------------
// An fp32 value rounded to the 16-bit operand type of this build (round-to-nearest-even, as the device conversions do
// it): the column sums of a folded LayerNorm must be taken over exactly the values the MFMA will see.
#ifdef GITMI_OPS_F16
static inline float bf16_round(float f) { return (float)(_Float16)f; }
#else
static inline float bf16_round(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return f;
    u += 0x7fffu + ((u >> 16) & 1u);
    u &= 0xffff0000u;
    memcpy(&f, &u, 4);
    return f;
}
#endif
// W [rows, K], bias [rows], LayerNorm (gamma, beta) [K] in front of it  ->  device W' (bf16), folded bias, column sums
// frag: fragment-major packing for the decode chain; else row-major for gemm_p8_kernel
static int fold_layernorm(gitmi_engine* e, const std::vector<float>& W, const std::vector<float>& bias,
                          const std::vector<float>& gamma, const std::vector<float>& beta, int64_t rows, int K, bool frag,
                          Folded* out) {
    std::vector<float> wf((size_t)rows * K), b2((size_t)rows), c2((size_t)rows);
    float amax = 0.f;
    for (int64_t n = 0; n < rows; ++n) {
        double sum = 0.0, cst = bias[n];
        const float* w = &W[(size_t)n * K];
        float* o = &wf[(size_t)n * K];
        for (int k = 0; k < K; ++k) {
            amax = std::max(amax, std::fabs(w[k] * gamma[k]));
            o[k] = bf16_round(w[k] * gamma[k]);
            sum += (double)o[k];
            cst += (double)beta[k] * (double)w[k];
        }
        c2[n] = (float)sum;
        b2[n] = (float)cst;
    }
    RCK(operand_range_check(e, "a matrix with the LayerNorm gain in front of it folded in (W . gamma)", amax));
    const int64_t rows_pad = (rows + 127) / 128 * 128;       // the vocabulary head reads bias / colsum a workgroup (128 columns) at a time
    RCK(dev_alloc(e, &out->w, (size_t)rows_pad * K * 2));
    float* tmp = nullptr;
    void* tmp_b = nullptr;
    HIPCK(hipMalloc((void**)&tmp, wf.size() * 4));
    hipError_t err = hipSuccess;
    if (frag) err = hipMalloc(&tmp_b, wf.size() * 2);
    if (err == hipSuccess) err = hipMemcpy(tmp, wf.data(), wf.size() * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = launch_convert_pad(tmp, frag ? tmp_b : out->w, false, (size_t)rows, K, K, 0);
    if (err == hipSuccess && frag) err = launch_frag_pack(tmp_b, out->w, (int)rows, (int)rows_pad, K, 0);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    hipFree(tmp);
    if (tmp_b) hipFree(tmp_b);
    HIPCK(err);
    b2.resize((size_t)rows_pad, 0.f);
    c2.resize((size_t)rows_pad, 0.f);
    RCK(dev_alloc_t(e, &out->bias, (size_t)rows_pad));
    RCK(dev_alloc_t(e, &out->colsum, (size_t)rows_pad));
    HIPCK(hipMemcpy(out->bias, b2.data(), (size_t)rows_pad * 4, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(out->colsum, c2.data(), (size_t)rows_pad * 4, hipMemcpyHostToDevice));
    return 0;
}
// fragment-major copy of an already packed row-major bf16 matrix [rows, K]
static int pack_frag(gitmi_engine* e, const void* src, int64_t rows, int K, void** dst) {
    const int64_t rows_pad = (rows + 15) / 16 * 16;
    RCK(dev_alloc(e, dst, (size_t)rows_pad * K * 2));
    HIPCK(launch_frag_pack(src, *dst, (int)rows, (int)rows_pad, K, 0));
    HIPCK(hipDeviceSynchronize());
    return 0;
}
// the LayerNorm `ln` in front of the dense layer `dense` (key prefixes; "weight" [K] / [rows, K] and "bias" [K] / [rows]
// complete them) folded into it
static int fold_named(gitmi_engine* e, const std::string& ln, const std::string& dense, int64_t rows, int K, bool frag, Folded* out) {
    const HostTensor *g, *b, *w, *bi;
    RCK(get_w(e, ln + "weight", {K}, &g));
    RCK(get_w(e, ln + "bias", {K}, &b));
    RCK(get_w(e, dense + "weight", {rows, K}, &w));
    RCK(get_w(e, dense + "bias", {rows}, &bi));
    return fold_layernorm(e, w->data, bi->data, g->data, b->data, rows, K, frag, out);
}
static std::string vit_layer_key(int i) { return "image_encoder.transformer.resblocks." + std::to_string(i) + "."; }
static std::string dec_layer_key(int i) { return "textual.transformer.encoder.layer." + std::to_string(i) + "."; }
// [Wq; Wk; Wv] and [bq; bk; bv] of a decoder layer as host tensors "attention.self.qkv.weight" / ".bias": one GEMM produces
// the packed q|k|v rows the attention kernels read.  The plain upload, the decode-chain fold and the prefill fold read them.
static int concat_qkv(gitmi_engine* e, const std::string& pre, int d) {
    HostTensor w, b;
    w.shape = {3 * d, d};
    b.shape = {3 * d};
    for (const char* name : {"query", "key", "value"}) {
        const HostTensor *tw, *tb;
        RCK(get_w(e, pre + "attention.self." + name + ".weight", {d, d}, &tw));
        RCK(operand_range_check(e, (pre + "attention.self." + name + ".weight").c_str(), tw->amax));
        RCK(get_w(e, pre + "attention.self." + name + ".bias", {d}, &tb));
        w.data.insert(w.data.end(), tw->data.begin(), tw->data.end());
        b.data.insert(b.data.end(), tb->data.begin(), tb->data.end());
        w.amax = std::max(w.amax, tw->amax);
    }
    e->host_w[pre + "attention.self.qkv.weight"] = std::move(w);
    e->host_w[pre + "attention.self.qkv.bias"] = std::move(b);
    return 0;
}

// decode chain: which LayerNorm stands in front of which matrix (fragment-major)
static int fold_decoder(gitmi_engine* e) {
    const gitmi_config& c = e->cfg;
    const int d = c.dec_hidden, f = c.dec_ffn;
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string pre = dec_layer_key(i);
        DecLayerW& L = e->w.dec[i];
        if (i > 0) {      // QKV behind the previous layer's output LayerNorm
            RCK(fold_named(e, dec_layer_key(i - 1) + "output.LayerNorm.", pre + "attention.self.qkv.", 3 * d, d, true, &L.qkv_f));
        } else {          // layer 0 consumes the embedding LayerNorm's output directly: plain weights, packed
            RCK(pack_frag(e, L.wqkv, 3 * d, d, &L.qkv_f.w));
            L.qkv_f.bias = L.bqkv;
        }
        RCK(pack_frag(e, L.wo, d, d, &L.wo_p));
        RCK(pack_frag(e, L.w2, d, f, &L.w2_p));
        RCK(fold_named(e, pre + "attention.output.LayerNorm.", pre + "intermediate.dense.", f, d, true, &L.ffn1_f));
    }
    return fold_named(e, dec_layer_key(c.dec_layers - 1) + "output.LayerNorm.", "textual.output.", c.vocab, d, true, &e->w.out_f);
}

// encoder and prefill GEMMs behind a LayerNorm (e->pol.ln_fold): row-major folded copies next to the plain ones (small batches and
// shapes outside gemm_p8_kernel's rules keep the LayerNorm launches and the plain matrices)
static int fold_encoder_prefill(gitmi_engine* e) {
    const gitmi_config& c = e->cfg;
    const int D = c.vit_width, d = c.dec_hidden, f = c.dec_ffn;
    for (int i = 0; i < c.vit_layers; ++i) {
        const std::string pre = vit_layer_key(i);
        RCK(fold_named(e, pre + "ln_1.", pre + "attn.in_proj_", 3 * D, D, false, &e->w.vit[i].qkv_f));
        RCK(fold_named(e, pre + "ln_2.", pre + "mlp.c_fc.", 4 * D, D, false, &e->w.vit[i].ffn1_f));
    }
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string pre = dec_layer_key(i);
        DecLayerW& L = e->w.dec[i];
        // layer 0 stands behind the visual projection's LayerNorm, the others behind the previous layer's output LayerNorm
        const std::string ln = i == 0 ? "textual.visual_projection.1." : dec_layer_key(i - 1) + "output.LayerNorm.";
        RCK(fold_named(e, ln, pre + "attention.self.qkv.", 3 * d, d, false, &L.qkv_pf));
        if (i + 1 == c.dec_layers) break;            // the last layer's image rows stop at K / V
        RCK(fold_named(e, pre + "attention.output.LayerNorm.", pre + "intermediate.dense.", f, d, false, &L.ffn1_pf));
    }
    return 0;
}

extern "C" int gitmi_finalize_weights(gitmi_engine* e) {
    if (!e) return fail("null engine");
    if (e->finalized) return 0;
    HIPCK(hipSetDevice(e->device));
    const gitmi_config& c = e->cfg;
    const int D = c.vit_width, F4 = 4 * D, d = c.dec_hidden, f = c.dec_ffn, V = c.vocab;
    const int64_t p = c.patch;
    // ---- image encoder -----------------------------------------------------------------
    {
        const HostTensor* t;
        RCK(get_w(e, "image_encoder.conv1.weight", {D, 3, p, p}, &t));
        e->host_w["image_encoder.conv1.weight"].shape = {D, (int64_t)e->Kp};
        RCK(up_mat(e, "image_encoder.conv1.weight", D, e->Kp, e->Kp_pad, &e->w.conv_w));
    }
    RCK(up_f32(e, "image_encoder.class_embedding", {D}, &e->w.cls));
    RCK(up_f32(e, "image_encoder.positional_embedding", {e->N_nat, D}, &e->w.pos));
    e->pos_cur = e->w.pos;
    RCK(up_f32(e, "image_encoder.ln_pre.weight", {D}, &e->w.lnpre_g));
    RCK(up_f32(e, "image_encoder.ln_pre.bias", {D}, &e->w.lnpre_b));
    RCK(up_f32(e, "image_encoder.ln_post.weight", {D}, &e->w.lnpost_g));
    RCK(up_f32(e, "image_encoder.ln_post.bias", {D}, &e->w.lnpost_b));
    e->w.vit.resize(c.vit_layers);
    for (int i = 0; i < c.vit_layers; ++i) {
        const std::string pre = vit_layer_key(i);
        VitLayerW& L = e->w.vit[i];
        RCK(up_mat(e, pre + "attn.in_proj_weight", 3 * D, D, D, &L.wqkv));
        RCK(up_f32(e, pre + "attn.in_proj_bias", {3 * D}, &L.bqkv));
        RCK(up_mat(e, pre + "attn.out_proj.weight", D, D, D, &L.wo));
        RCK(up_f32(e, pre + "attn.out_proj.bias", {D}, &L.bo));
        RCK(up_f32(e, pre + "ln_1.weight", {D}, &L.ln1g));
        RCK(up_f32(e, pre + "ln_1.bias", {D}, &L.ln1b));
        RCK(up_mat(e, pre + "mlp.c_fc.weight", F4, D, D, &L.w1));
        RCK(up_f32(e, pre + "mlp.c_fc.bias", {F4}, &L.b1));
        RCK(up_mat(e, pre + "mlp.c_proj.weight", D, F4, F4, &L.w2));
        RCK(up_f32(e, pre + "mlp.c_proj.bias", {D}, &L.b2));
        RCK(up_f32(e, pre + "ln_2.weight", {D}, &L.ln2g));
        RCK(up_f32(e, pre + "ln_2.bias", {D}, &L.ln2b));
    }
    e->w.temb.resize(c.num_frames);
    for (int i = 0; i < c.num_frames; ++i)
        RCK(up_f32(e, "img_temperal_embedding." + std::to_string(i), {1, 1, D}, &e->w.temb[i]));
    // ---- text decoder ------------------------------------------------------------------
    RCK(up_mat(e, "textual.visual_projection.0.weight", d, D, D, &e->w.vp_w));
    RCK(up_f32(e, "textual.visual_projection.0.bias", {d}, &e->w.vp_b));
    RCK(up_f32(e, "textual.visual_projection.1.weight", {d}, &e->w.vp_lng));
    RCK(up_f32(e, "textual.visual_projection.1.bias", {d}, &e->w.vp_lnb));
    RCK(up_f32(e, "textual.embedding.words.weight", {V, d}, &e->w.words_f));
    RCK(up_f32(e, "textual.embedding.positions.weight", {c.max_pos, d}, &e->w.positions_f));
    RCK(up_f32(e, "textual.embedding.layer_norm.weight", {d}, &e->w.emb_lng));
    RCK(up_f32(e, "textual.embedding.layer_norm.bias", {d}, &e->w.emb_lnb));
    e->w.dec.resize(c.dec_layers);
    double wbytes = 0;
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string pre = dec_layer_key(i);
        DecLayerW& L = e->w.dec[i];
        RCK(concat_qkv(e, pre, d));
        RCK(up_mat(e, pre + "attention.self.qkv.weight", 3 * d, d, d, &L.wqkv));
        RCK(up_f32(e, pre + "attention.self.qkv.bias", {3 * d}, &L.bqkv));
        RCK(up_mat(e, pre + "attention.output.dense.weight", d, d, d, &L.wo));
        RCK(up_f32(e, pre + "attention.output.dense.bias", {d}, &L.bo));
        RCK(up_f32(e, pre + "attention.output.LayerNorm.weight", {d}, &L.lnag));
        RCK(up_f32(e, pre + "attention.output.LayerNorm.bias", {d}, &L.lnab));
        RCK(up_mat(e, pre + "intermediate.dense.weight", f, d, d, &L.w1));
        RCK(up_f32(e, pre + "intermediate.dense.bias", {f}, &L.b1));
        RCK(up_mat(e, pre + "output.dense.weight", d, f, f, &L.w2));
        RCK(up_f32(e, pre + "output.dense.bias", {d}, &L.b2));
        RCK(up_f32(e, pre + "output.LayerNorm.weight", {d}, &L.lnog));
        RCK(up_f32(e, pre + "output.LayerNorm.bias", {d}, &L.lnob));
        wbytes += ((double)4 * d * d + (double)2 * d * f) * e->pol.esz;
    }
    if (e->host_w.find("textual.output.weight") == e->host_w.end())   // tied (decoder.py:503-505)
        e->host_w["textual.output.weight"] = e->host_w["textual.embedding.words.weight"];
    RCK(up_mat(e, "textual.output.weight", V, d, d, &e->w.out_w));
    RCK(up_f32(e, "textual.output.bias", {V}, &e->w.out_b));
    wbytes += (double)V * d * e->pol.esz;
    e->w.dec_weight_bytes = wbytes;
    if (!e->pol.f32 && d % 32 == 0 && f % 32 == 0 && d <= 768 && V <= 32768) RCK(fold_decoder(e));      // the bf16 decode chain (else: generic GEMM + LayerNorm launches)
    else e->pol.skinny = false;
    if (e->pol.ln_fold_ready) RCK(fold_encoder_prefill(e));
    e->host_w.clear();
    RCK(alloc_workspaces(e));
    HIPCK(hipDeviceSynchronize());
    e->finalized = true;
    return 0;
}

// A second execution context on the same device that BORROWS the packed weights of `src` (its own
// workspaces, KV caches, search state, streams and graph).  Lets a server keep several batches in
// flight on different HIP streams: the latency-bound decode steps of one batch overlap the
// MFMA-bound encoder of the next.  `src` must outlive the clone.
extern "C" int gitmi_clone(gitmi_engine* src, gitmi_engine** out) {
    if (!src || !out) return fail("gitmi_clone: null argument");
    if (!src->finalized) return fail("gitmi_clone: source weights not finalized");
    HIPCK(hipSetDevice(src->device));
    gitmi_engine* e = new gitmi_engine();
    e->cfg = src->cfg;
    e->device = src->device;
    e->w = src->w;              // the same device pointers: borrowed
    e->pol = src->pol;          // as it stands now (gitmi_set_ln_fold / _shared_device / _temporal_embedding / _graph included)
    // a clone starts at the native resolution (its own gitmi_set_image_shape state and resized table), non-ragged,
    // without a trie, without profiling and without encoder-ordering links
    init_geometry(e);
    e->parent = src->parent ? src->parent : src;
    int rc = alloc_workspaces(e);
    if (rc != 0) { gitmi_destroy(e); return rc; }
    HIPCK(hipDeviceSynchronize());
    e->finalized = true;
    *out = e;
    return 0;
}