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
