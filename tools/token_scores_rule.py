"""The per-token trace rule (include/gitmi.h GITMI_SEARCH_TRACE) restated on the CPU in fp64.

Two forms of the same rule:

  simulate(...)        runs AutoRegressiveBeamSearch / GeneratorWithBeamSearch over SCRIPTED logits (logits[cur_len][row]) and lets
                       every beam carry its own records -- (log-prob of the pick, the n best of the row it was picked from) per
                       position -- so that beam reordering copies them with the history.  No log, no row indirection: what the
                       engine's log must reproduce.  tests/test_gpu_token_scores_ops.py drives the engine's step seam with the
                       same script.
  records_of(...)      derives the records of a RETURNED sequence from the (rows, logits) calls a search class made to its `step`:
                       for position s, the first recorded row whose history equals seq[:s], the class's rules before its
                       log-softmax, the token's log-prob and the n best.  This is what a recording wrapper around the unmodified
                       search classes gives (oracle.git_oracle's, or the reference's).

Both order alternatives by (log-prob descending, token id ascending), report an alternative whose log-prob is -inf as token -1,
and apply the rules in fp32 (as both the engine and the reference do) before the fp64 log-softmax.
"""
import math
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

NEG = -10000.0


def ruled_logprobs(kind: str, logits: torch.Tensor, history: Sequence[int], P: int, eos: int,
                   repetition_penalty: float = 1.0) -> torch.Tensor:
    """class_logprobs of one row in fp64: `logits` fp32 [V] as `step` returned them (constraint bans included), `history` the
    row's tokens (start tokens and prefix, P of them, included).
      autoregressive (decoder.py:330-358): past the first search step -10000 on the previous token, and the one-hot [SEP] of an
                     ended beam;  generator (decoder.py:1135-1144): the repetition penalty over the history's tokens."""
    x = logits.detach().to(torch.float32).clone()
    if kind == "autoregressive":
        if len(history) > P:
            last = int(history[-1])
            x[last] = NEG
            if last == eos:
                x[:] = float("-inf")
                x[eos] = 0.0
    elif repetition_penalty not in (0.0, 1.0):
        rp = torch.tensor(repetition_penalty, dtype=torch.float32)
        for tok in set(int(t) for t in history):
            x[tok] = x[tok] * rp if x[tok] < 0 else x[tok] / rp
    return torch.log_softmax(x.double(), dim=0)


def top_alternatives(lp: torch.Tensor, n: int):
    """the n likeliest (token, log-prob) of a distribution, ties to the lower token id; -inf entries are token -1"""
    if n == 0:
        return [], []
    order = torch.sort(lp, descending=True, stable=True)            # stable: equal values keep ascending token order
    vals = order.values[:n].tolist()
    toks = [int(t) if v != float("-inf") else -1 for t, v in zip(order.indices[:n].tolist(), vals)]
    return toks, vals


def blank(n: int):
    """the record of a position that was not chosen (prefix, past the end): lp 0, no alternatives"""
    return 0.0, [-1] * n, [0.0] * n


def length_norm(length: int, alpha: float) -> float:
    return (5.0 + length) ** alpha / 6.0 ** alpha


def _f32(x: float) -> float:
    return float(np.float32(x))


def _sum32(a: float, b: float) -> float:
    return float(np.float32(a) + np.float32(b))


class Trace:
    """Result of simulate(): per returned sequence o (sentence-major, best first) tokens [T], logprob, and per position
    lp [T], alt_tok [T][n], alt_lp [T][n]; `margin` = the smallest gap between a kept and the next candidate sum over all
    decisions that were not exact ties (how much logit noise the ids tolerate)."""

    def __init__(self):
        self.tokens, self.logprob, self.lp, self.alt_tok, self.alt_lp, self.length = [], [], [], [], [], []
        self.margin = math.inf


def _emit(tr: Trace, tokens, logprob, recs, first, T, n, eos, length):
    """recs: the records of positions [first, first + len(recs))"""
    lp, at, al = [], [], []
    for s in range(T):
        r = recs[s - first] if first <= s < first + len(recs) else blank(n)
        lp.append(r[0]); at.append(list(r[1])); al.append(list(r[2]))
    tr.tokens.append(list(tokens) + [eos] * (T - len(tokens)))
    tr.logprob.append(logprob); tr.lp.append(lp); tr.alt_tok.append(at); tr.alt_lp.append(al); tr.length.append(length)


def simulate(kind: str, logits: Callable[[int], torch.Tensor], prefixes: List[List[int]], k: int, pn: int, T: int, eos: int, n: int,
             num_keep_best: int = 1, length_penalty: float = 1.0, repetition_penalty: float = 1.0, prefixed: bool = True) -> Trace:
    """The search of `kind` ("autoregressive" | "generator") over scripted logits: logits(cur_len) -> fp32 [B * k, V], row b * k + j
    = beam j of sentence b at the step that appends position cur_len.  Every sentence has its own prefix (the search starts at the
    shortest and appends the given tokens of the longer ones).  Running sums are fp32, as in the engine; everything else fp64."""
    B = len(prefixes)
    plen = [len(p) for p in prefixes]
    minP = min(plen)
    tr = Trace()
    # a beam: (ids, score, recs) with recs the records of positions [plen, len(ids))
    beams = [[(list(prefixes[b][:minP]), 0.0 if (kind == "autoregressive" or j == 0) else -1e9, []) for j in range(k)] for b in range(B)]
    stop = [0] * B
    done = [False] * B
    hyps = [[] for _ in range(B)]            # generator: dicts(score, seq, ids, recs) in slot order
    hyp_cnt = [0] * B
    worst = [1e9] * B

    def note_margin(sums_sorted, kept):
        for i in range(min(kept, len(sums_sorted) - 1)):          # the order of the kept ones decides their rows, so it counts too
            gap = sums_sorted[i] - sums_sorted[i + 1]
            if gap > 0:
                tr.margin = min(tr.margin, gap)

    for cur_len in range(minP, T):
        x = logits(cur_len)
        old = beams
        new = []
        for b in range(B):
            P = plen[b]
            if cur_len < P:
                new.append([(ids + [prefixes[b][cur_len]], sc, recs) for ids, sc, recs in old[b]])
                continue
            first = cur_len == P
            dist = [ruled_logprobs(kind, x[b * k + j], old[b][j][0], P, eos, repetition_penalty) for j in range(k)]
            alts = [top_alternatives(d, n) for d in dist]
            if kind == "autoregressive":
                if not first and stop[b] == 0 and all(bm[0][-1] == eos for bm in old[b]):
                    stop[b] = cur_len
                if first:
                    o = torch.sort(dist[0], descending=True, stable=True)       # decoder.py:257-298: beam 0 alone is expanded
                    vals = o.values[:k + 1].tolist()
                    note_margin(vals, k)
                    ids0 = old[b][0][0]
                    new.append([(ids0 + [int(o.indices[j])], _f32(vals[j]), [(vals[j], *alts[0])]) for j in range(k)])
                else:
                    cands = []
                    for j in range(k):
                        o = torch.sort(dist[j], descending=True, stable=True)
                        for d in range(pn):
                            cands.append((_sum32(float(o.values[d]), old[b][j][1]), j * pn + d, j, int(o.indices[d]), float(o.values[d])))
                    cands.sort(key=lambda c: (-c[0], c[1]))
                    note_margin([c[0] for c in cands], k)
                    new.append([(old[b][j][0] + [tok], s, old[b][j][2] + [(lp, *alts[j])]) for s, _, j, tok, lp in cands[:k]])
                continue
            # ---- generator
            V = dist[0].numel()
            ncand = pn * k
            cands = []
            for j in range(k):
                o = torch.sort(dist[j], descending=True, stable=True)
                for d in range(min(ncand, V)):
                    cands.append((_sum32(float(o.values[d]), old[b][j][1]), j * V + int(o.indices[d]), j, int(o.indices[d]), float(o.values[d])))
            cands.sort(key=lambda c: (-c[0], c[1]))
            note_margin([c[0] for c in cands], ncand)
            cands = cands[:ncand]
            if not done[b] and len(hyps[b]) >= num_keep_best:
                done[b] = worst[b] >= cands[0][0] / length_norm(T - 1, length_penalty)
            nxt = []
            if not done[b]:
                for s, _, j, tok, lp in cands:
                    if len(nxt) == k:
                        break
                    if tok == eos or cur_len + 1 == T:
                        sc = s / length_norm(cur_len, length_penalty)
                        h = dict(score=sc, seq=hyp_cnt[b], ids=list(old[b][j][0]), recs=old[b][j][2] + [(lp, *alts[j])])
                        if len(hyps[b]) < num_keep_best:
                            hyps[b].append(h)
                            hyp_cnt[b] += 1
                            worst[b] = min(worst[b], sc)
                        elif sc > worst[b]:
                            slot = min(range(len(hyps[b])), key=lambda i: (hyps[b][i]["score"], hyps[b][i]["seq"]))
                            hyps[b][slot] = h
                            hyp_cnt[b] += 1
                            worst[b] = min(hh["score"] for hh in hyps[b])
                    else:
                        nxt.append((old[b][j][0] + [tok], s, old[b][j][2] + [(lp, *alts[j])]))
            if len(nxt) < k:
                pad = old[b][0] if prefixed else old[0][0]
                nxt = [(pad[0] + [eos], 0.0, pad[2] + [blank(n)]) for _ in range(k)]
            new.append(nxt)
        beams = new
    for b in range(B):
        P = plen[b]
        if kind == "autoregressive":
            L = stop[b] if stop[b] > 0 else T
            ids, score, recs = beams[b][0]
            seq = ids[:L]
            nv = max(1, sum(t != eos for t in seq) + (1 if eos in seq else 0) - P)
            _emit(tr, seq, score / nv, recs[:L - P], P, T, n, eos, L)
        else:
            order = sorted(hyps[b], key=lambda h: (-h["score"], h["seq"]))
            for i in range(num_keep_best):
                if i < len(order):
                    h = order[i]
                    _emit(tr, h["ids"], h["score"], h["recs"], P, T, n, eos, len(h["ids"]))
                else:
                    _emit(tr, [], -1e5, [], P, T, n, eos, 0)
    return tr


def records_of(kind: str, calls, seq: Sequence[int], P: int, end: int, n: int, eos: int, repetition_penalty: float = 1.0,
               sentence: int = 0, sentences: int = 1):
    """The records of positions [P, end) of a returned sequence from the search class's recorded step calls: calls = [(rows int64
    [R, t], logits fp32 [R, V])], the rows of a call being `sentences` equal blocks (sentence-major).  Position s takes the FIRST
    recorded row of the sequence's own sentence whose history equals seq[:s] (other sentences may hold the same tokens over
    another image).  -> [(lp, alt_tok, alt_lp)] for s in [P, end)"""
    out = []
    for s in range(P, end):
        want = [int(t) for t in seq[:s]]
        row = None
        for rows, lg in calls:
            if rows.shape[1] != s:
                continue
            per = rows.shape[0] // sentences
            lo = sentence * per
            hit = (rows[lo:lo + per] == torch.tensor(want, dtype=rows.dtype)).all(dim=1).nonzero()
            if hit.numel():
                row = lg[lo + int(hit[0])]
                break
        if row is None:
            raise LookupError(f"no recorded row has the history of position {s}")
        lp = ruled_logprobs(kind, row, want, P, eos, repetition_penalty)
        out.append((float(lp[int(seq[s])]), *top_alternatives(lp, n)))
    return out


def check_sum(lp_row: Sequence[float], logprob: float, divisor: float, T: int) -> Optional[str]:
    """The sum invariant: sum_s lp[s] / divisor reproduces logprob within T * 2^-23 * max(1, |sum|) (the engine sums sequentially
    in fp32, this sums in fp64).  -> None, or what is wrong"""
    total = math.fsum(float(v) for v in lp_row)
    bound = T * 2.0 ** -23 * max(1.0, abs(total))
    if abs(total - float(logprob) * divisor) > bound:
        return f"sum {total!r} vs logprob x divisor {float(logprob) * divisor!r}: off by more than {bound:.3e}"
    return None
