"""The per-sentence decoding constraints (include/gitmi.h GITMI_SEARCH_CONSTRAIN) as a wrapper of the reference's `step` callable.

wrap_step(step, ...) returns a step that calls the given one and sets z[c] = -10000 for every token c banned for (row, t); the
search class then does whatever it does after `step`.  This is the definition the engine's kernels implement
(csrc/ban_rules.h), written with torch on full logits: tools/make_constraints_golden.py hands it to the unmodified reference
search classes, tests/test_constraints_host.py checks it against a brute-force restatement.
"""
from __future__ import annotations

import numpy as np
import torch

BANNED = -10000.0


def set_mask(words, vocab: int) -> torch.Tensor:
    """uint32 words [W] of a ban set -> bool [vocab]: token c <-> bit c % 32 of word c // 32 (bits past vocab are ignored)"""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return torch.from_numpy(bits[:vocab].astype(bool))


def ngram_banned(history, n: int):
    """The tokens that would complete, at the end of `history`, an n-gram the history already holds"""
    t = len(history)
    if n <= 0 or t < n:
        return set()
    tail = list(history[t - n + 1:])
    return {history[i + n - 1] for i in range(t - n + 1) if list(history[i:i + n - 1]) == tail}


def sequence_banned(history, seqs):
    """The last tokens of the sequences of `seqs` (2 or more tokens each) whose other tokens the `history` ends with"""
    t = len(history)
    return {int(a[-1]) for a in seqs if t >= len(a) - 1 and list(history[t - len(a) + 1:]) == [int(v) for v in a[:-1]]}


def wrap_step(step, sets, table, eos: int, plen, sequences=None, list_of=None):
    """step: [rows, t] token ids -> [rows, vocab] logits, rows = sentences x beams with the rows of a sentence contiguous.
    sets: uint32 [n_sets, W]; table: one [set index or -1, min_new, ngram] per sentence; plen: the prefix length of every
    sentence (start tokens included).  sequences: lists of banned token sequences, list_of: the list of every sentence or -1
    (None with sequences: sentence s <-> list s)."""
    table = [[int(v) for v in row] for row in table]
    plen = [int(p) for p in plen]
    S = len(table)
    if sequences is not None and list_of is None:
        list_of = list(range(S))

    def constrained(tokens: torch.Tensor) -> torch.Tensor:
        z = step(tokens).clone()
        rows, t = tokens.shape
        assert rows % S == 0, (rows, S)
        beams, vocab = rows // S, z.shape[1]
        for r in range(rows):
            s = r // beams
            set_index, min_new, n = table[s]
            if set_index >= 0:
                z[r, set_mask(sets[set_index], vocab)] = BANNED
            if t - plen[s] < min_new:
                z[r, eos] = BANNED
            for c in ngram_banned(tokens[r].tolist(), n):
                z[r, c] = BANNED
            if sequences is not None and list_of[s] >= 0:
                for c in sequence_banned(tokens[r].tolist(), sequences[list_of[s]]):
                    z[r, c] = BANNED
        return z

    return constrained
