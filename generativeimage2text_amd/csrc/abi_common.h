// Error reporting shared by the translation units that implement the C ABI (engine.hip, engine_weights.hip, abi_ops.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <vector>

namespace gitmi {
// formats the thread's message for gitmi_last_error() and returns 1 (the ABI's failure code)
int fail(const char* fmt, ...);

// Host side of launch_context_embed (GITMI_SEARCH_CONTEXT and its op hook): Q context segments of lengths len[q] in
// [1, max_len], segment q of image image_of[q] (nullptr: Q == B, segment q <-> image q); the segments of one image follow each
// other in increasing q.  -> tab = seg [Q][4] {image, first context row within the image, length, 0} | cnt [B] context rows
// per image | {stride, max_b cnt[b], sum_b cnt[b], 0}, one upload.  The stride is the engine's choice for the call: n_img plus
// the longest context, up to the next multiple of 16 where the capacity `cap` (rows per image) allows.  Fails by message,
// naming `who`, on a bad count, length or image and when an image's rows exceed cap.
struct ContextTable {
    std::vector<int32_t> tab;
    int Q = 0, B = 0, stride = 0, max_rows = 0, total = 0;
    const int32_t* seg() const { return tab.data(); }
    const int32_t* cnt() const { return tab.data() + (size_t)4 * Q; }
    const int32_t* info() const { return tab.data() + (size_t)4 * Q + B; }
};
inline int context_table(const char* who, const int32_t* len, const int32_t* image_of, int Q, int B, int max_len, int n_img, int cap,
                         ContextTable* out) {
    if (Q < 1 || B < 1 || !len) return fail("%s: Q=%d context segments over B=%d images", who, Q, B);
    if (!image_of && Q != B) return fail("%s: without image_of, Q must equal B", who);
    ContextTable& t = *out;
    t.Q = Q; t.B = B; t.max_rows = t.total = 0;
    t.tab.assign((size_t)4 * Q + B + 4, 0);
    int32_t* cnt = t.tab.data() + (size_t)4 * Q;
    for (int q = 0; q < Q; ++q) {
        const int n = len[q], im = image_of ? image_of[q] : q;
        if (n < 1 || n > max_len) return fail("%s: length %d of context segment %d outside [1,%d]", who, n, q, max_len);
        if (im < 0 || im >= B) return fail("%s: context segment %d names image %d of %d", who, q, im, B);
        if (cnt[im] > cap - n_img - n)
            return fail("%s: image %d needs %d rows (%d image rows + %d context rows), the capacity is %d rows per image "
                        "(max_frames x max_image_tokens)", who, im, n_img + cnt[im] + n, n_img, cnt[im] + n, cap);
        int32_t* sg = t.tab.data() + (size_t)4 * q;
        sg[0] = im; sg[1] = cnt[im]; sg[2] = n;
        cnt[im] += n;
        t.total += n;
        if (cnt[im] > t.max_rows) t.max_rows = cnt[im];
    }
    if (n_img > cap) return fail("%s: %d image rows exceed the capacity of %d rows per image", who, n_img, cap);
    const int need = n_img + t.max_rows;
    t.stride = (need + 15) / 16 * 16 <= cap ? (need + 15) / 16 * 16 : need;
    int32_t* info = t.tab.data() + (size_t)4 * Q + B;
    info[0] = t.stride; info[1] = t.max_rows; info[2] = t.total; info[3] = 0;
    return 0;
}

// Host side of the banned-sequence pool (GITMI_SEARCH_CONSTRAIN's extension, include/gitmi.h, and its op hook): pool int32 [n] =
// { L, S, T, 0, list_of[Q], list_off[L + 1], seq_off[S + 1], tok[T] }.  Everything ban_rows_kernel forms an address from is
// checked here, before any launch: the sizes add up to n, L <= max_lists, S and T within the caps (launchers.h BAN_SEQ_MAX_*),
// list_of in [-1, L), both offset arrays start at 0, never decrease and end at S / T, every sequence has 2 .. max_len tokens,
// every token lies in [0, vocab).  Fails by message naming `who` and the sentence, list and sequence.
struct BanPoolView {
    int L = 0, S = 0, T = 0;
    const int32_t *list_of = nullptr, *list_off = nullptr, *seq_off = nullptr, *tok = nullptr;
};
inline int ban_pool_check(const char* who, const int32_t* pool, int n, int Q, int vocab, int max_lists, int max_seqs, int max_toks,
                          int max_len, BanPoolView* out) {
    if (!pool || n < 4) return fail("%s: a sequence pool of %d words (at least the 4 of its header)", who, n);
    const int L = pool[0], S = pool[1], T = pool[2];
    if (L < 0 || L > max_lists) return fail("%s: %d sequence lists outside [0,%d] (max_batch)", who, L, max_lists);
    if (S < 0 || S > max_seqs) return fail("%s: %d sequences above the cap of %d per call", who, S, max_seqs);
    if (T < 0 || T > max_toks) return fail("%s: %d sequence tokens above the cap of %d per call", who, T, max_toks);
    const long long need = 4LL + Q + (L + 1) + (S + 1) + T;
    if (pool[3] != 0 || need != (long long)n)
        return fail("%s: the sequence pool has %d words, but { L=%d, S=%d, T=%d, 0 } with %d sentences needs %lld", who, n, L, S, T, Q, need);
    BanPoolView v;
    v.L = L; v.S = S; v.T = T;
    v.list_of = pool + 4; v.list_off = v.list_of + Q; v.seq_off = v.list_off + L + 1; v.tok = v.seq_off + S + 1;
    for (int q = 0; q < Q; ++q)
        if (v.list_of[q] < -1 || v.list_of[q] >= L) return fail("%s: sentence %d: sequence list %d outside [-1,%d)", who, q, v.list_of[q], L);
    if (v.list_off[0] != 0 || v.list_off[L] != S) return fail("%s: list offsets run from %d to %d, not from 0 to S=%d", who, v.list_off[0], v.list_off[L], S);
    for (int l = 0; l < L; ++l)
        if (v.list_off[l + 1] < v.list_off[l]) return fail("%s: list %d: offsets decrease (%d after %d)", who, l, v.list_off[l + 1], v.list_off[l]);
    if (v.seq_off[0] != 0 || v.seq_off[S] != T) return fail("%s: sequence offsets run from %d to %d, not from 0 to T=%d", who, v.seq_off[0], v.seq_off[S], T);
    for (int l = 0; l < L; ++l)
        for (int j = v.list_off[l]; j < v.list_off[l + 1]; ++j) {
            const long long m = (long long)v.seq_off[j + 1] - v.seq_off[j];
            if (m < 2 || m > max_len) return fail("%s: list %d: sequence %d has %lld tokens, outside [2,%d]", who, l, j, m, max_len);
        }
    // with list_off ending at S and every length >= 2, seq_off is strictly increasing from 0 to T: every token index is in [0, T)
    for (int l = 0; l < L; ++l)
        for (int j = v.list_off[l]; j < v.list_off[l + 1]; ++j)
            for (int i = v.seq_off[j]; i < v.seq_off[j + 1]; ++i)
                if (v.tok[i] < 0 || v.tok[i] >= vocab)
                    return fail("%s: list %d: sequence %d holds token %d outside [0,%d)", who, l, j, v.tok[i], vocab);
    *out = v;
    return 0;
}
}  // namespace gitmi

#define HIPCK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e__ = (expr);                                                                      \
        if (e__ != hipSuccess) return gitmi::fail("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
    } while (0)
#define RCK(expr)                 \
    do {                          \
        int r__ = (expr);         \
        if (r__ != 0) return r__; \
    } while (0)
