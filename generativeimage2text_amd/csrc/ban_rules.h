// Per-sentence decoding constraints (GITMI_SEARCH_CONSTRAIN, include/gitmi.h): THE definition of "token c is banned for row r at
// this step", shared by every kernel that sees logits together with the row's history (vocab_topm_kernel<., VOC_GENERIC>,
// row_topm_kernel, sample_rows_kernel).  A banned logit becomes -10000.f before anything else happens to it.
//
// Row r belongs to sentence s = r / beams and holds tokens x[0 .. t), start tokens and prefix (plen tokens) included.  c is banned if
//   set     bit c % 32 of word c / 32 of ban set set_of[s] is set (set_of[s] == -1: no set), or
//   length  c == eos and t - plen < min_new[s], or
//   n-gram  n = ngram[s] > 0, t >= n, and for some i in [0, t - n]:  x[i .. i + n - 1) == x[t - n + 1 .. t)  and  x[i + n - 1] == c
//           (n == 1: every token of the history), or
//   sequence  some sequence a = (a_0 .. a_{m-1}), 2 <= m <= 16, of the sentence's list has a_{m-1} == c, t >= m - 1 and
//           x[t - m + 1 .. t) == a[0 .. m - 1).  Many sequences per sentence: no consumer scans them.  ban_rows_kernel
//           (kernels_search.hip) ORs the hits into a per-row copy of the sentence's set once per step, and the consumers read
//           that copy (BanArgs::row_words) through the set rule.
// In code:  banned(c) = ban_static(row, c) || exists i in [0, ban_ngram_last(row, t)] with ban_ngram_hit(row, x, t, i) and
// x[i + n - 1] == c.  The n-gram rule bans at most t tokens, each of them a history token: every consumer walks i once per
// row, folds the hits into the lookup it already keeps for the repetition penalty (a bit mask over the lane's columns, a
// token set in LDS), and then asks once per logit.  Addresses are formed from the host-validated set_of, the column index
// and history positions in [0, t) only; history tokens are compared, never used as indices.
#pragma once
#include "launchers.h"

namespace gitmi {

struct BanRow {
    const unsigned int* set;    // the W words of the sentence's ban set, or nullptr
    int W;
    int eos;                    // the token the length rule bans at this step, or -1
    int n;                      // n-gram size, 0 when the rule is off or the history is shorter than n
};

__device__ __forceinline__ BanRow ban_row(const BanArgs& b, int row, int sent, int plen, int t) {
    BanRow r;
    const int si = b.set_of[sent];
    r.set = b.row_words ? b.row_words + (size_t)row * b.W : si >= 0 ? b.words + (size_t)si * b.W : nullptr;
    r.W = b.W;
    r.eos = t - plen < b.min_new[sent] ? b.eos : -1;
    const int n = b.ngram[sent];
    r.n = (n > 0 && t >= n) ? n : 0;
    return r;
}
// word w of the row's ban set (token 32 w + j <-> bit j); 0 without a set and past its last word
__device__ __forceinline__ unsigned int ban_set_word(const BanRow& r, int w) { return (r.set && w < r.W) ? r.set[w] : 0u; }
// the set and length rules
__device__ __forceinline__ bool ban_static(const BanRow& r, int c) { return c == r.eos || ((ban_set_word(r, c >> 5) >> (c & 31)) & 1u); }
// the n-gram rule: the last start position to test (-1: none), and whether the n - 1 tokens at i equal the last n - 1 of the
// history -- then x[i + n - 1] is banned
__device__ __forceinline__ int ban_ngram_last(const BanRow& r, int t) { return r.n > 0 ? t - r.n : -1; }
__device__ __forceinline__ bool ban_ngram_hit(const BanRow& r, const int* x, int t, int i) {
    bool same = true;
    for (int j = 0; j + 1 < r.n; ++j) same = same && x[i + j] == x[t - r.n + 1 + j];
    return same;
}
// the sequence rule: whether the history x[0 .. t) ends with the m - 1 tokens a[0 .. m - 1) -- then a[m - 1] is banned
__device__ __forceinline__ bool ban_seq_hit(const int* x, int t, const int* a, int m) {
    if (t < m - 1) return false;
    bool same = true;
    for (int j = 0; j + 1 < m; ++j) same = same && x[t - m + 1 + j] == a[j];
    return same;
}

}  // namespace gitmi
