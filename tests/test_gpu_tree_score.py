"""Token-tree scoring on the MI355X (GITMI_SEARCH_TREE_SCORE, csrc/kernels_score.hip): Engine.score_tree / CaptioningModel.rank
against the CPU oracle's full recompute of every root-to-node path, against Engine.score on the paths as sentences, and against
the fixtures frozen from the reference.  The bound is test_gpu_score.py's: 2 logit_bound(precision, span of the logits)."""
import functools
import glob
import os

import pytest
import torch

from conftest import GOLDEN, golden_case
from tools.parity import logit_bound

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16", "bf16")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "score_*.npz")))


def _engine(cfg, w, precision, B, Q, L, F=1, hw=None):
    from generativeimage2text_amd.engine import Engine
    eng = Engine(cfg, precision=precision, max_batch=B, max_beams=max(1, -(-Q // B)), max_frames=F, max_text_len=max(L, 2),
                 max_image_hw=hw)
    eng.load_state_dict(w)
    return eng


def _parents(depths):
    path, out = {}, []
    for i, d in enumerate(depths):
        out.append(path.get(d - 1, -1))
        path[d] = i
    return out


def _path(par, node):
    out = []
    while node >= 0:
        out.append(node)
        node = par[node]
    return out[::-1]


def _random_tree(n, seed, max_depth, vocab, sos):
    """n nodes in pre-order: every depth in [1, depth of the node before + 1], below max_depth"""
    gen = torch.Generator().manual_seed(seed)
    depths = [0]
    for _ in range(n - 1):
        depths.append(int(torch.randint(1, min(depths[-1] + 1, max_depth - 1) + 1, (1,), generator=gen)))
    tokens = [sos] + torch.randint(1, vocab, (n - 1,), generator=gen).tolist()
    return tokens, depths


def _bushy_tree(vocab, sos):
    """A root chain of 3; 70 single-token leaves under its last node (siblings across two 64-query tiles and three 32-key
    blocks); under the same node one branch down to depth 39; two-level forks under the chain's upper nodes."""
    depths = [0, 1, 2] + [3] * 70 + list(range(3, 40)) + [2, 3, 4, 4, 3, 4, 4] + [1, 2, 3, 3, 2, 2] + [1, 2, 2]
    gen = torch.Generator().manual_seed(81)
    tokens = [sos] + torch.randint(1, vocab, (len(depths) - 1,), generator=gen).tolist()
    return tokens, depths


def _pad(trees):
    L = max(len(t) for t, _ in trees)
    tok, dep = torch.zeros(len(trees), L, dtype=torch.int64), torch.zeros(len(trees), L, dtype=torch.int64)
    for q, (t, d) in enumerate(trees):
        tok[q, :len(t)], dep[q, :len(d)] = torch.tensor(t), torch.tensor(d)
    return tok, dep, [len(t) for t, _ in trees]


def _oracle_nodes(cfg, w, feats, tokens, depths):
    """(lp, mean_lp) float64 [n, 2] of every node from the oracle's logits of its root-to-parent path, and their span.  One
    oracle call per node that has a leaf child or is a leaf's deepest inner ancestor: its rows serve every node on the path."""
    from oracle import git_oracle as O
    n, par = len(tokens), _parents(depths)
    rows, span = {}, 0.0
    for i in range(n - 1, 0, -1):                                 # deepest paths first: a later node's parent is usually covered
        if par[i] in rows:
            continue
        path = _path(par, par[i])
        with torch.no_grad():
            z = O.textual_logits_full(cfg, w, feats, torch.tensor([[tokens[k] for k in path]])).double()[0]
        for pos, k in enumerate(path):
            rows[k] = z[pos]
    out = torch.zeros(n, 2, dtype=torch.float64)
    for i in range(1, n):
        z = rows[par[i]]
        ls = torch.log_softmax(z, -1)
        out[i, 0], out[i, 1] = ls[tokens[i]], ls.mean()
        span = max(span, float(z.max() - z.min()))
    return out, span


@functools.lru_cache(maxsize=None)
def _tiny(seed):
    from oracle import git_oracle as O
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=seed, tie_output=False, successor=2.0)
    frames = O.make_images(cfg, 3, 1, seed=seed + 1)
    with torch.no_grad():
        feats = O.visual_features(cfg, w, frames)
    return cfg, w, frames, feats


@functools.lru_cache(maxsize=None)
def _ragged_trees():
    """Trees of 1, 18, 65 and 130 nodes over images 0, 0, 2, 1 with the oracle's values: computed once, shared, never changed"""
    cfg, w, frames, feats = _tiny(83)
    image_of = [0, 0, 2, 1]
    trees = [_random_tree(n, 90 + n, 40, cfg.vocab, cfg.sos) for n in (1, 18, 65, 130)]
    ref = [_oracle_nodes(cfg, w, feats[im:im + 1], t, d) for (t, d), im in zip(trees, image_of)]
    return trees, image_of, [r[0] for r in ref], max(r[1] for r in ref)


def _tol(precision, span):
    return 2.0 * logit_bound(precision, span)


# ---- 1. a chain is a sentence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_chain_equals_score(precision):
    from oracle import git_oracle as O
    cfg, w, frames, feats = _tiny(83)
    B, L = 3, 17
    tokens = torch.randint(1, cfg.vocab, (B, L), generator=torch.Generator().manual_seed(84))
    tokens[:, 0] = cfg.sos
    with torch.no_grad():
        z = O.textual_logits_full(cfg, w, feats, tokens)
    eng = _engine(cfg, w, precision, B, B, L)
    dev = [f.cuda() for f in frames]
    want = eng.score(dev, tokens).cpu()
    got = eng.score_tree(dev, tokens, torch.arange(L).expand(B, L)).cpu()
    eng.close()
    err = (got - want).abs().max().item()
    tol = _tol(precision, float(z.max() - z.min()))
    print(f"chain {precision}: max |score_tree - score| {err:.3e} bound {tol:.3e}")
    assert want[:, 1:, 0].abs().min() > 0 and torch.all(got[:, 0] == 0)
    assert err <= tol
    if precision == "f32":
        assert torch.equal(got, want)                            # the same launches in the same order, the gather reads score's logits


# ---- 2. a bushy tree against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_bushy_tree_against_the_oracle(precision):
    cfg, w, frames, feats = _tiny(83)
    tokens, depths = _bushy_tree(cfg.vocab, cfg.sos)
    assert len(tokens) == 126 and max(depths) == 39 and depths.count(3) >= 70
    ref, span = _oracle_nodes(cfg, w, feats[1:2], tokens, depths)
    eng = _engine(cfg, w, precision, 1, 1, 40)
    got = eng.score_tree([f[1:2].cuda() for f in frames], [tokens], [depths]).cpu().double()[0]
    eng.close()
    err = (got - ref).abs().max(0).values.tolist()
    print(f"bushy {precision}: lp error {err[0]:.3e} mean-lp error {err[1]:.3e} bound {_tol(precision, span):.3e}")
    assert torch.all(got[0] == 0)
    assert max(err) <= _tol(precision, span), (precision, err)


# ---- 3. the values frozen from the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", CASES)
def test_tree_of_the_golden_sentences_matches_reference(name, precision):
    """The sentences of every image merged into one trie below their shared [CLS]: lp / mean_lp of (sentence, position) are the
    node's on the sentence's path."""
    from generativeimage2text_amd.model import TokenTrie
    g, cfg, w, frames, _, _ = golden_case(name)
    hw = tuple(int(v) for v in g["hw"]) if g["hw"].size else None
    tokens, lengths, image_of = torch.as_tensor(g["tokens"]), g["lengths"].tolist(), g["image_of"].tolist()
    B, F = int(g["batch"]), int(g["frames"])
    trees, where = [], []                                        # where: (sentence, tree, node of every position >= 1)
    for b in range(B):
        mine = [q for q, im in enumerate(image_of) if im == b]
        tok, dep, terminal = TokenTrie.construct([tokens[q, 1:lengths[q]].tolist() for q in mine]).preorder()
        trees.append(([int(tokens[mine[0], 0])] + tok, [0] + dep))
        par = _parents([0] + dep)
        where += [(q, b, _path(par, t + 1)[1:]) for q, t in zip(mine, terminal)]
    tok, dep, lens = _pad(trees)
    eng = _engine(cfg, w, precision, B, B, tokens.shape[1], F, hw)
    out = eng.score_tree([f.cuda() for f in frames], tok, dep, lengths=lens).cpu().double()
    eng.close()
    bound = 2.0 * logit_bound(precision, float(g["logit_max"]) - float(g["logit_min"]))
    lp_ref, mean_ref = torch.as_tensor(g["lp"]), torch.as_tensor(g["mean_lp"])
    err = 0.0
    for q, b, nodes in where:
        assert len(nodes) == lengths[q] - 1
        for j, node in enumerate(nodes, start=1):
            err = max(err, abs(float(out[b, node, 0] - lp_ref[q, j])), abs(float(out[b, node, 1] - mean_ref[q, j])))
    print(f"{name} {precision}: error {err:.3e} bound {bound:.3e}")
    assert err <= bound, (name, precision, err, bound)


# ---- 4. batch independence and ragged sizes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_batch_independence_and_ragged_sizes(precision):
    cfg, w, frames, feats = _tiny(83)
    trees, image_of, ref, span = _ragged_trees()
    tok, dep, lens = _pad(trees)
    dev = [f.cuda() for f in frames]
    eng = _engine(cfg, w, precision, 3, 4, 40)
    together = eng.score_tree(dev, tok, dep, lengths=lens, image_of=image_of).cpu()
    tol = 1e-6 if precision == "f32" else _tol(precision, span)
    for q, (n, im) in enumerate(zip(lens, image_of)):
        alone = eng.score_tree([f[im:im + 1] for f in dev], tok[q:q + 1, :n], dep[q:q + 1, :n]).cpu()
        assert (together[q, :n] - alone[0]).abs().max().item() <= tol, (q, precision)
        assert (together[q, :n].double() - ref[q]).abs().max().item() <= _tol(precision, span), (q, precision)
        assert torch.all(together[q, n:] == 0) and torch.all(together[q, 0] == 0)
        assert n == 1 or together[q, 1:n, 0].abs().min() > 0
    eng.close()


# ---- 5. residency -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_followup_over_resident_images_is_bit_equal(precision):
    from generativeimage2text_amd.engine import Engine
    cfg, w, frames, feats = _tiny(83)
    trees, image_of, _, _ = _ragged_trees()
    tok, dep, lens = _pad(trees[1:3])
    dev = [f.cuda() for f in frames]
    eng = _engine(cfg, w, precision, 3, 3, 40)
    with_frames = eng.score_tree(dev, tok, dep, lengths=lens, image_of=[0, 2]).cpu()
    eng.generate(dev, Engine.make_search("greedy", 12, 1, 1))
    gen = eng.generation
    resident = eng.score_tree(None, tok, dep, lengths=lens, image_of=[0, 2]).cpu()
    assert eng.generation == gen                                 # nothing was encoded
    eng.close()
    assert torch.equal(resident, with_frames)


@pytest.mark.parametrize("precision", PRECS)
def test_tree_over_image_and_context_equals_score_on_the_paths(precision):
    from generativeimage2text_amd.engine import context_segments
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel
    g, cfg, w, frames, gsearch, _ = golden_case("context_tiny_greedy")
    B, T = int(g["batch"]), gsearch.max_steps
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=T, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision=precision, max_batch=B, max_frames=1, max_text_len=T,
                            max_context=max(g["context_counts"].tolist()))
    model.load_state_dict(w)
    eng = model.engine
    context = [{"tokens": torch.as_tensor(g[f"ctx_tokens_{i}"]), "length": torch.as_tensor(g[f"ctx_lengths_{i}"])}
               for i in range(int(g["n_context"]))]
    segs, seg_image = context_segments(context, B, cfg.vocab, cfg.max_pos)
    eng.encode_context([frames[0].cuda()], segs, image_of=seg_image)
    trees = [_random_tree(14, 70 + b, T, cfg.vocab, cfg.sos) for b in range(B)]
    tok, dep, lens = _pad(trees)
    got = eng.score_tree(None, tok, dep, lengths=lens).cpu()
    err, checked = 0.0, 0
    for b, (t, d) in enumerate(trees):
        par = _parents(d)
        leaves = [i for i in range(len(t)) if i + 1 == len(t) or d[i + 1] <= d[i]]
        for c0 in range(0, len(leaves), B):                     # the engine holds max_batch x 1 sentences per call
            paths = [_path(par, leaf) for leaf in leaves[c0:c0 + B]]
            sent = torch.zeros(len(paths), max(len(p) for p in paths), dtype=torch.int64)
            for r, p in enumerate(paths):
                sent[r, :len(p)] = torch.tensor([t[k] for k in p])
            want = eng.score(None, sent, lengths=[len(p) for p in paths], image_of=[b] * len(paths)).cpu()
            for r, p in enumerate(paths):
                err = max(err, (got[b, p] - want[r, :len(p)]).abs().max().item())
                checked += len(p) - 1
    # the context is part of what was scored: over the images alone the numbers leave the bound
    plain = eng.score_tree([frames[0].cuda()], tok, dep, lengths=lens).cpu()
    model.close()
    bound = 2.0 * logit_bound(precision, float(g["logit_max"]) - float(g["logit_min"]))
    moved = (plain - got).abs().max().item()
    print(f"context {precision}: max |tree - score on paths| {err:.3e} bound {bound:.3e}; without the context {moved:.3e}")
    assert checked >= 13 * B and err <= bound
    if precision == "f32":
        assert moved > bound


@pytest.mark.parametrize("precision", PRECS)
def test_ragged_image_batch_equals_per_image_trees(precision):
    """Images of different shapes in one call (key counts 2, 31 and 33 either side of the 32-key block): every tree gets what a
    call with its image alone gets, as score does in ragged mode."""
    from generativeimage2text_amd.engine import Engine
    cfg, w, _, _ = _tiny(83)
    gen = torch.Generator().manual_seed(86)
    imgs = [torch.randn(3, h, wd, generator=gen).cuda() for h, wd in ((16, 16), (80, 96), (64, 128))]
    trees = [_random_tree(n, 40 + n, 12, cfg.vocab, cfg.sos) for n in (20, 9, 70)]
    tok, dep, lens = _pad(trees)
    eng = Engine(cfg, precision=precision, max_batch=3, max_beams=1, max_frames=1, max_text_len=12, max_image_hw=(96, 128))
    eng.load_state_dict(w)
    out = eng.score_tree(eng.ragged(imgs), tok, dep, lengths=lens).cpu()
    for b, im in enumerate(imgs):
        n = lens[b]
        ref = eng.score_tree([im[None]], tok[b:b + 1, :n], dep[b:b + 1, :n]).cpu()[0]
        err = (out[b, :n] - ref).abs().max().item()
        assert err <= (1e-6 if precision == "f32" else _tol(precision, 8.0)), (b, precision, err)
        assert out[b, 1:n, 0].abs().min() > 0 and torch.all(out[b, n:] == 0)
    eng.close()


# ---- 6. refusals and rejection ------------------------------------------------------------------------------------------------------
def test_refusals_by_message():
    from generativeimage2text_amd import engine as E
    cfg, w, frames, feats = _tiny(83)
    trees, image_of, _, _ = _ragged_trees()
    dev = [f.cuda() for f in frames]
    eng = _engine(cfg, w, "f32", 3, 3, 40)
    s = E.Engine.make_search("greedy", 12, 1, 1)
    s.kind = E.SEARCH_TREE_SCORE
    with pytest.raises(E.GitmiError, match="GITMI_SEARCH_TREE_SCORE scores given token trees: call gitmi_generate_prefixed"):
        eng.generate(dev, s)
    with pytest.raises(E.GitmiError, match="GITMI_SEARCH_TREE_SCORE is not a search"):
        eng.search_begin(s, torch.full((3, 1), cfg.sos), cfg.vocab)
    with pytest.raises(ValueError, match=r"tree 0, node 40: depth 40 must be below 40"):
        eng.score_tree(dev, [[cfg.sos] + [5] * 40] * 3, [list(range(41))] * 3)
    with pytest.raises(E.GitmiError, match="max_batch x max_beams"):
        eng.score_tree(dev, [[cfg.sos, 5]] * 4, [[0, 1]] * 4, image_of=[0, 1, 2, 0])
    tok, dep, lens = _pad(trees[1:4])
    good = eng.score_tree(dev, tok, dep, lengths=lens, image_of=image_of[1:4]).cpu()
    # above the row cap: refused before any launch (nothing reads the table), the message carries the numbers
    arr, keep, B = eng._frames_arg(dev)
    big = torch.empty(3, 1 << 21, dtype=torch.int64, device="cuda")
    with pytest.raises(E.GitmiError, match=r"3 trees x 2097152 padded nodes = 6291456 rows above the cap of 4194240 rows per call"):
        eng._sentence_call(E.SEARCH_TREE_SCORE, dev, arr, keep, B, big, [1 << 21] * 3, image_of[1:4], torch.empty(2, device="cuda"))
    del big
    again = eng.score_tree(dev, tok, dep, lengths=lens, image_of=image_of[1:4]).cpu()
    eng.close()
    assert torch.equal(again, good)


@pytest.mark.parametrize("precision", PRECS)
def test_rejected_trees_stay_zero_and_leave_the_others(precision):
    """Invalid DATA the engine is specified to reject on the device, before any kernel reads the structure: through the raw call
    path, with none of the host checks.  No kernel is altered and nothing is made to fault."""
    from generativeimage2text_amd import engine as E
    cfg, w, frames, feats = _tiny(83)
    trees, image_of, _, span = _ragged_trees()
    dev = [f.cuda() for f in frames]
    eng = _engine(cfg, w, precision, 3, 3, 40)
    tok, dep, lens = _pad(trees[1:4])
    good = eng.score_tree(dev, tok, dep, lengths=lens, image_of=image_of[1:4]).cpu()
    tol = 1e-6 if precision == "f32" else _tol(precision, span)          # test 4's tolerance

    def raw(depths):
        """the packed table as a caller of the C interface writes it: none of the host checks"""
        table = ((depths << 32) | tok).cuda()
        out = torch.full((3, tok.shape[1], 2), 7.0, device="cuda")
        arr, keep, B = eng._frames_arg(dev)
        info = eng._sentence_call(E.SEARCH_TREE_SCORE, dev, arr, keep, B, table, lens, image_of[1:4], out, check=False)
        return out.cpu(), info.tolist()

    out, info = raw(dep)
    assert info == [tok.shape[1], 0, 0, 0] and torch.equal(out, good)
    # a depth jump of 2 in the middle tree, a depth at the bound (max_text_len = 40) in the first, a second root in the last, a
    # root that is not at depth 0
    for q, node, value in ((1, 30, int(dep[1, 29]) + 2), (0, 9, 40), (2, 100, 0), (1, 0, 1)):
        wrong = dep.clone()
        wrong[q, node] = value
        out, info = raw(wrong)
        assert info == [tok.shape[1], 0, 0, 1], (q, node, info)
        assert torch.all(out[q] == 0), (q, node)
        for other in set(range(3)) - {q}:
            assert (out[other] - good[other]).abs().max().item() <= tol, (q, node, other, precision)
    again = eng.score_tree(dev, tok, dep, lengths=lens, image_of=image_of[1:4]).cpu()
    eng.close()
    assert torch.equal(again, good)


# ---- 7. rank end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_rank_end_to_end(precision):
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel
    cfg, w, frames, feats = _tiny(83)
    gen = torch.Generator().manual_seed(85)
    stems = [torch.randint(1, cfg.vocab, (2,), generator=gen).tolist() for _ in range(3)]
    cands = [stems[k % 3][:1 + k % 2] + torch.randint(1, cfg.vocab, (1 + k % 3,), generator=gen).tolist() for k in range(12)]
    prefixes = [[7, 8, 9], [11, 12, 13, 14, 15]]
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=20, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision=precision, max_batch=2, max_frames=1, max_text_len=20)
    model.load_state_dict(w)
    images = frames[0][:2].cuda()
    out = model.rank(images, cands, prefixes=prefixes)
    assert out["scores"].shape == (2, 12) and len(out["tree"]["lengths"]) == 2
    assert out["tree"]["lengths"][0] < sum(len(c) + 1 for c in cands) + 4          # shared prefixes share nodes
    longest = max(len(c) for c in cands) + 1
    span, err = 0.0, 0.0
    for q, p in enumerate(prefixes):
        for k in range(0, 12, 2):                                # two sentences per call: the engine's capacity
            sents = [[cfg.sos] + p + c + [cfg.eos] for c in cands[k:k + 2]]
            L = max(len(s) for s in sents)
            tok = torch.tensor([s + [0] * (L - len(s)) for s in sents])
            need = (tok != 0).long()
            need[:, :1 + len(p)] = 0
            want = model.score(images[q:q + 1], tok, image_of=[0, 0], need_predict=need)["sum"]
            err = max(err, (out["scores"][q, k:k + 2] - want).abs().max().item())
    from oracle import git_oracle as O
    with torch.no_grad():
        for q, p in enumerate(prefixes):
            z = O.textual_logits_full(cfg, w, feats[q:q + 1], torch.tensor([[cfg.sos] + p + max(cands, key=len) + [cfg.eos]]))
            span = max(span, float(z.max() - z.min()))
    model.close()
    bound = _tol(precision, span) * longest
    print(f"rank {precision}: max |scores - sums of score| {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(out["best"], out["scores"].argmax(1))
