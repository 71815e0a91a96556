"""Host side of token-tree scoring (GITMI_SEARCH_TREE_SCORE, include/gitmi.h): TokenTrie.preorder, the packed (depth, token)
table and its checks, CaptioningModel.rank's tree construction and path sums against a stub engine, and the interface constants."""
import os
import types

import pytest
import torch

from generativeimage2text_amd import engine as E
from generativeimage2text_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- TokenTrie.preorder ---------------------------------------------------------------------------------------------------------
# the sequences of test_host.py::test_token_trie_mirror_matches_the_oracle_restatement, then a duplicate and a prefix of another
SEQS = [[5, 6, 102], [5, 7, 102], [9, 102], [5, 6, 8, 102]]


def test_preorder_lists_children_in_insertion_order():
    tokens, depths, terminal = M.TokenTrie.construct(SEQS).preorder()
    #  5 -+- 6 -+- 102          9 - 102
    #     |     +- 8 - 102
    #     +- 7 - 102
    assert tokens == [5, 6, 102, 8, 102, 7, 102, 9, 102]
    assert depths == [1, 2, 3, 3, 4, 2, 3, 1, 2]
    assert terminal == [2, 6, 8, 4]
    for seq, t in zip(SEQS, terminal):                       # the path from the root to terminal[s] spells sequence s
        assert _path_tokens(tokens, depths, t) == seq


def test_preorder_duplicates_share_a_node_and_a_prefix_ends_inside():
    seqs = SEQS + [[5, 7, 102], [5, 6], []]
    trie = M.TokenTrie.construct(seqs)
    tokens, depths, terminal = trie.preorder()
    assert tokens == [5, 6, 102, 8, 102, 7, 102, 9, 102]     # no new node
    assert terminal == [2, 6, 8, 4, 6, 1, -1]                # the duplicate's node; an inner node; the root
    assert trie.get_valid([5, 6]) == [102, 8]                # the reference interface is what it was
    assert trie.csr()[0][:2] == [0, 2]


def _parents(depths):
    path, out = {}, []
    for i, d in enumerate(depths):
        out.append(path.get(d - 1, -1))
        path[d] = i
    return out


def _path_tokens(tokens, depths, node):
    par, out = _parents(depths), []
    while node >= 0:
        out.append(tokens[node])
        node = par[node]
    return out[::-1]


# ---- the packed table and every ValueError ------------------------------------------------------------------------------------
def test_pack_trees_layout():
    tokens = torch.tensor([[101, 7, 8, 9, 0], [101, 5, 6, 7, 999]])
    depths = torch.tensor([[0, 1, 1, 2, 0], [0, 1, 2, 3, 1]])
    table, lens = E.pack_trees(tokens, depths, [4, 5], vocab=1000, max_depth=4)
    assert table.dtype == torch.int64 and table.shape == (2, 5) and lens == [4, 5]
    assert torch.equal(table & 0xFFFFFFFF, torch.tensor([[101, 7, 8, 9, 0], [101, 5, 6, 7, 999]]))
    assert torch.equal(table >> 32, torch.tensor([[0, 1, 1, 2, 0], [0, 1, 2, 3, 1]]))
    assert int(table[0, 4]) == 0                             # past the length: zero, whatever was there
    table, lens = E.pack_trees([[101, 3]], [[0, 1]], None, vocab=1000, max_depth=2)
    assert lens == [2] and table.tolist() == [[101, (1 << 32) | 3]]


@pytest.mark.parametrize("depths, lengths, match", [
    ([[0, 1, 2], [1, 1, 2]], None, r"tree 1, node 0: the root must have depth 0, got 1"),
    ([[0, 1, 2], [0, 2, 3]], None, r"tree 1, node 1: depth 2 must lie in \[1, depth of the node before it \+ 1\]"),   # a jump of 2
    ([[0, 1, 3], [0, 1, 2]], None, r"tree 0, node 2: depth 3 must lie in"),
    ([[0, 1, 0], [0, 1, 2]], None, r"tree 0, node 2: depth 0 must lie in .*one root"),                               # a second root
    ([[0, 1, 2], [0, 1, 2]], None, None),
    ([[0, 1, 2, 3, 4]], None, r"tree 0, node 4: depth 4 must be below 4"),                                            # at the bound
    ([[0, 1, 2], [0, 1, 2]], [3, 0], r"tree 1: length 0 outside \[1, 3\]"),
    ([[0, 1, 2], [0, 1, 2]], [4, 1], r"tree 0: length 4 outside \[1, 3\]"),
    ([[0, 1, 2], [0, 1, 9]], [3, 2], None),                                                                          # past the length
])
def test_pack_trees_rules(depths, lengths, match):
    tokens = torch.full((len(depths), len(depths[0])), 7)
    if match is None:
        E.pack_trees(tokens, depths, lengths, vocab=1000, max_depth=4)
        return
    with pytest.raises(ValueError, match=match):
        E.pack_trees(tokens, depths, lengths, vocab=1000, max_depth=4)


def test_pack_trees_ids_and_shapes():
    with pytest.raises(ValueError, match=r"token ids outside \[0, 1000\)"):
        E.pack_trees([[101, 1000]], [[0, 1]], None, vocab=1000, max_depth=4)
    with pytest.raises(ValueError, match="must both be"):
        E.pack_trees([[101, 5]], [[0, 1, 2]], None, vocab=1000, max_depth=4)


# ---- rank: tree construction, path sums, argmax --------------------------------------------------------------------------------
class _TreeEngine:
    """score_tree of a stub: lp of node i of tree q is -(1000 q + i) / 8 (exact in fp32), mean_lp its double"""

    def __init__(self):
        self.calls = []
        self.c = types.SimpleNamespace(max_batch=8, max_frames=1)
        self.resident, self.generation = 0, 0

    def set_temporal_embedding(self, on):
        pass

    def score_tree(self, frames, tokens, depths=None, lengths=None, image_of=None):
        E.pack_trees(tokens, depths, lengths, vocab=30522, max_depth=64)            # the trees rank builds obey the rules
        self.calls.append(dict(frames=frames, tokens=tokens.clone(), depths=depths.clone(), lengths=list(lengths), image_of=image_of))
        Q, L = tokens.shape
        lp = -(1000.0 * torch.arange(Q)[:, None] + torch.arange(L)[None, :]) / 8
        return torch.stack([lp, 2 * lp], -1).float()


def _model():
    m = object.__new__(M.CaptioningModel)
    m.cfg = types.SimpleNamespace(num_frames=0, sos=101, eos=102, vocab=30522)
    m.engine, m._loaded, m.training = _TreeEngine(), True, False
    return m


def test_rank_builds_one_tree_per_prefix_and_sums_the_candidates_own_nodes():
    m = _model()
    cands = [[5, 6], [5, 7], [9], [5, 6, 8], [5, 6]]                           # shared prefixes, a duplicate
    out = m.rank(torch.zeros(2, 3, 8, 8), cands, prefixes=[[11, 12], [101, 13]], image_of=[1, 0])
    call = m.engine.calls[-1]
    trie_tok = [5, 6, 102, 8, 102, 7, 102, 9, 102]
    assert call["tokens"].tolist() == [[101, 11, 12] + trie_tok, [101, 13] + trie_tok + [0]]        # [CLS] is not doubled
    assert call["depths"].tolist() == [[0, 1, 2, 3, 4, 5, 5, 6, 4, 5, 3, 4], [0, 1, 2, 3, 4, 4, 5, 3, 4, 2, 3, 0]]
    assert call["lengths"] == [12, 11] and call["image_of"] == [1, 0]
    assert out["tree"]["terminal"].tolist() == [[5, 9, 11, 7, 5], [4, 8, 10, 6, 4]]
    # candidate 0 of tree 0 = nodes 3, 4, 5 (5, 6, [SEP]); the prefix nodes 1, 2 do not count
    own = [[3 + 4 + 5, 3 + 8 + 9, 10 + 11, 3 + 4 + 6 + 7, 3 + 4 + 5], [2 + 3 + 4, 2 + 7 + 8, 9 + 10, 2 + 3 + 5 + 6, 2 + 3 + 4]]
    counts = [3, 3, 2, 4, 3]                                                   # nodes of every candidate, [SEP] included
    want = torch.tensor([[-(1000.0 * q * n + s) / 8 for s, n in zip(row, counts)] for q, row in enumerate(own)])
    assert torch.equal(out["scores"], want)
    # tree 0: candidates 0 and 4 tie at the top, the first wins; tree 1 (every node costs 125 more): the two-node candidate
    assert out["best"].tolist() == [0, 2]
    assert out["node_logprobs"].shape == (2, 12, 2)


def test_rank_argmax_ties_and_plain_candidates():
    m = _model()
    out = m.rank(torch.zeros(3, 3, 8, 8), [[9, 9, 9], [7], [7]], append_eos=False)     # no prefix: one tree per image
    call = m.engine.calls[-1]
    assert call["tokens"].tolist() == [[101, 9, 9, 9, 7]] * 3 and call["depths"].tolist() == [[0, 1, 2, 3, 1]] * 3
    assert call["image_of"] is None and call["lengths"] == [5, 5, 5]
    assert out["scores"][0].tolist() == [-(1 + 2 + 3) / 8, -4 / 8, -4 / 8]
    assert out["best"].tolist() == [1, 1, 1]                                    # 1 and 2 tie: the first wins
    with pytest.raises(ValueError, match="at least one candidate"):
        m.rank(torch.zeros(1, 3, 8, 8), [])
    with pytest.raises(ValueError, match="image_of"):
        m.rank(None, [[7]])


# ---- interface constants -----------------------------------------------------------------------------------------------------
def test_interface_constants():
    assert E.SEARCH_TREE_SCORE == 6
    with open(os.path.join(ROOT, "include", "gitmi.h")) as f:
        header = f.read()
    assert "#define GITMI_SEARCH_TREE_SCORE 6" in header
    assert "#define GITMI_ABI_VERSION 10\n" in header
    assert len(E.EXPORTED_SYMBOLS) == 40
    assert "gitmi_debug_score_attn_tree" in E.EXPERIMENT_SYMBOLS
    with open(os.path.join(ROOT, "include", "gitmi_experiment.h")) as f:
        assert "gitmi_debug_score_attn_tree(" in f.read()
