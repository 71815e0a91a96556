"""Context tokens in the decoder memory on the MI355X (GITMI_SEARCH_CONTEXT; the reference's batch['context'], decoder.py:861-871)
against fixtures frozen from the reference (tools/make_context_golden.py): ids, teacher-forced log-probs and the training-mode
loss, the padding that is never read, residency and captured graphs, and the calls that are refused."""

import numpy as np
import pytest
import torch

from conftest import golden_case
from tools.parity import F32_LOGIT_ABS, ids_parity, logit_bound

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16", "bf16")
ID_CASES = ("context_tiny_greedy", "context_tiny_beam4", "context_tiny_prefix_beam4", "context_video_greedy")


def _context(g):
    return [{"tokens": torch.as_tensor(g[f"ctx_tokens_{i}"]), "length": torch.as_tensor(g[f"ctx_lengths_{i}"])}
            for i in range(int(g["n_context"]))]


def _decoder(cfg, search):
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, GeneratorWithBeamSearch
    if search.kind == "greedy":
        return AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=search.max_steps, beam_size=search.beam_size,
                                        per_node_beam_size=search.per_node_beam_size, fix_missing_prefix=True)
    return GeneratorWithBeamSearch(eos_index=cfg.eos, max_steps=search.max_steps, beam_size=search.beam_size,
                                   per_node_beam_size=search.per_node_beam_size, length_penalty=search.length_penalty)


def _case(name, precision="f32", search=None, max_context=None):
    """-> (fixture, cfg, model, batch with the context, batch without it)"""
    from generativeimage2text_amd.model import CaptioningModel
    g, cfg, w, frames, gsearch, prefix = golden_case(name)
    B, F = int(g["batch"]), int(g["frames"])
    counts = g["context_counts"].tolist()
    model = CaptioningModel(cfg, _decoder(cfg, search or gsearch), precision=precision, max_batch=B, max_frames=F,
                            max_text_len=gsearch.max_steps, max_context=max(counts) if max_context is None else max_context)
    model.load_state_dict(w)
    frames = [f.cuda() for f in frames]
    plain = {"image": frames if F > 1 else frames[0]}
    if prefix is not None:
        plain["prefix"] = prefix.cuda()
    return g, cfg, model, dict(plain, context=_context(g)), plain


def _same(a, b):
    return a["predictions"].shape == b["predictions"].shape and torch.equal(a["predictions"].cpu(), b["predictions"].cpu()) and \
        torch.equal(a["logprobs"].cpu(), b["logprobs"].cpu())


def _until_eos(row, eos):
    return row[:row.index(eos) + 1] if eos in row else row


# ---- 1. ids, f32 mode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ID_CASES)
def test_f32_ids_equal_the_reference(name):
    """Greedy B = 4 with key counts 17 / 18 / 32 / 33 (they straddle the 32-key tile of the decode attention; one image has two
    segments), beam 4 over the same batch against the per-image reference calls, B = 1 with prefix + context under beam 4, a
    video model (F = 3).  Every margin of the fixtures is >= 10 x F32_LOGIT_ABS (asserted when they were frozen), so every row
    must equal the reference's ids; and every row with context must differ from the ids the reference returns WITHOUT the
    context -- which is what an engine that drops the context returns."""
    g, cfg, model, batch, plain = _case(name)
    out = model(batch)
    preds, lps = out["predictions"].cpu().numpy(), out["logprobs"].cpu().numpy()
    model.close()
    ref = g["predictions"]
    import ast
    kind, _, k, _, _ = ast.literal_eval(str(g["search"]))
    assert float(g["step_margin"].min()) >= 10 * F32_LOGIT_ABS
    assert preds.shape == ref.shape, (preds.shape, ref.shape)
    stats = ids_parity(preds, ref, g["step_margin"], 10 * F32_LOGIT_ABS, chained=not (kind == "greedy" and k == 1),
                       first_decision_pos=0 if g["prefix"].size else 1)
    print(name, stats)
    assert stats["identical"] == stats["rows"] == ref.shape[0]
    assert np.allclose(lps.reshape(-1), g["logprobs"].reshape(-1), atol=1e-4), (lps, g["logprobs"])
    without = g["predictions_plain"]
    L = max(preds.shape[1], without.shape[1])
    pad = lambda x: np.concatenate([x, np.zeros((x.shape[0], L - x.shape[1]), dtype=x.dtype)], 1)
    for b, c in enumerate(g["context_counts"].tolist()):
        if c > 0:
            assert bool((pad(preds)[b] != pad(without)[b]).any()), (b, c, preds[b], without[b])
        else:           # an image without context is not touched by its neighbours' (up to its own end: the batch ends later or sooner)
            assert _until_eos(preds[b].tolist(), cfg.eos) == _until_eos(without[b].tolist(), cfg.eos), (b, preds[b], without[b])


# ---- 2. teacher-forced log-probs and the training-mode loss --------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", ("context_tiny_greedy", "context_video_greedy"))
def test_score_and_training_loss_with_context(name, precision):
    g, cfg, model, batch, plain = _case(name, precision)
    tokens, need = torch.as_tensor(g["tf_tokens"]), torch.as_tensor(g["tf_need_predict"])
    bound = 2.0 * logit_bound(precision, float(g["logit_max"]) - float(g["logit_min"]))
    out = model.score(batch["image"], tokens, need_predict=need, context=batch["context"])
    valid = torch.arange(tokens.shape[1])[None, :] < torch.as_tensor(g["tf_lengths"]).long()[:, None]
    err_lp = ((out["logprobs"].double() - torch.as_tensor(g["tf_lp"])).abs() * valid).max().item()
    err_mean = ((out["mean_logprobs"].double() - torch.as_tensor(g["tf_mean_lp"])).abs() * valid).max().item()
    # the context is part of what was scored: without it the numbers leave the bound
    off = model.score(batch["image"], tokens, need_predict=need)
    moved = ((off["logprobs"].double() - torch.as_tensor(g["tf_lp"])).abs() * valid).max().item()
    hint = str(g["tf_hint"])
    loss = model.train()(dict(batch, caption_tokens=tokens, need_predict=need, context_target_type=[hint]))
    model.eval()
    model.close()
    print(f"{name} {precision}: lp error {err_lp:.2e} mean-lp error {err_mean:.2e} bound {bound:.2e}; without the context {moved:.2e}")
    assert err_lp <= bound and err_mean <= bound, (err_lp, err_mean, bound)
    if precision == "f32":
        assert moved > bound, (moved, bound)
    assert set(loss) == {f"vl_{hint}_loss"}
    assert abs(float(loss[f"vl_{hint}_loss"]) - float(g["tf_loss"])) <= bound, (float(loss[f"vl_{hint}_loss"]), float(g["tf_loss"]))


# ---- 3. the padding is never read ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_ids_past_every_length_change_nothing(precision):
    g, cfg, model, batch, plain = _case("context_tiny_greedy", precision)
    tokens = torch.as_tensor(g["tf_tokens"])
    a = model(batch)
    sa = model.score(batch["image"], tokens, context=batch["context"])
    other = []
    for c in batch["context"]:
        t = c["tokens"].clone()
        pad = torch.arange(t.shape[1])[None, :] >= c["length"][:, None]
        t[pad] = (t[pad] * 7 + 13) % cfg.vocab
        assert not torch.equal(t, c["tokens"])
        other.append({"tokens": t, "length": c["length"]})
    b = model(dict(batch, context=other))
    sb = model.score(batch["image"], tokens, context=other)
    model.close()
    assert _same(a, b)
    assert torch.equal(sa["logprobs"], sb["logprobs"]) and torch.equal(sa["mean_logprobs"], sb["mean_logprobs"])


# ---- 4. residency and graphs ------------------------------------------------------------------------------------------------------
def test_model_call_equals_context_call_plus_followups():
    """model(batch with context) == Engine.encode_context, then explicit follow-ups on the one resident batch: greedy, beam 4, score."""
    from generativeimage2text_amd.engine import Engine, context_segments
    from generativeimage2text_amd.model import format_predictions
    from oracle import git_oracle as O
    g, cfg, m_greedy, batch, plain = _case("context_tiny_greedy", "f16")
    want_greedy = m_greedy(batch)
    tokens = torch.as_tensor(g["tf_tokens"])
    want_score = m_greedy.score(batch["image"], tokens, context=batch["context"])
    m_greedy.close()
    _, _, m_beam, _, _ = _case("context_tiny_greedy", "f16", search=O.BEAM4)
    want_beam = m_beam(batch)
    eng = m_beam.engine
    B = int(g["batch"])
    segs, image_of = context_segments(batch["context"], B, cfg.vocab, cfg.max_pos)
    info = eng.encode_context([batch["image"]], segs, image_of=image_of)
    geo = eng.resident_geometry
    # 17 image rows + 16: the engine's 33 rows per image (max_context = 16) leave no room to round the stride up
    assert info == {"stride": 33, "max_context": 16, "context_rows": 32}
    assert geo == (33, 1, [(4, 4)] * B) and geo.image_rows == 17 and geo.context == g["context_counts"].tolist() and eng.resident == B
    t, lp, inf = eng.generate(None, Engine.make_search("greedy", 20, 1, 1))
    preds, lps = format_predictions(t, lp, inf.tolist()[:2], None, "autoregressive")
    assert torch.equal(preds.cpu(), want_greedy["predictions"].cpu()) and torch.equal(lps.cpu(), want_greedy["logprobs"].cpu())
    t, lp, inf = eng.generate(None, Engine.make_search("beam", 20, 4, 2, 0.6))
    preds, lps = format_predictions(t, lp, inf.tolist()[:2], None, "generator")
    assert torch.equal(preds.cpu(), want_beam["predictions"].cpu()) and torch.equal(lps.cpu(), want_beam["logprobs"].cpu())
    sc = eng.score(None, tokens).cpu()
    assert torch.equal(sc[..., 0], want_score["logprobs"]) and torch.equal(sc[..., 1], want_score["mean_logprobs"])
    # per-sentence prefixes over the same memory: every question's answer is the shared-prefix call's
    pfx = [cfg.sos, 300, 2]
    t1, lp1, _ = eng.generate(None, Engine.make_search("greedy", 20, 1, 1), prefix=torch.tensor(pfx))
    t2, lp2, _, _ = eng.generate_prefixed(None, Engine.make_search("greedy", 20, 1, 1), [pfx] * B)
    for b in range(B):
        assert _until_eos(t1[b].tolist(), cfg.eos) == _until_eos(t2[b].tolist(), cfg.eos), (b, t1[b], t2[b])
    assert eng.resident == B and eng.resident_geometry.context == g["context_counts"].tolist()
    m_beam.close()


@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_graph_on_off_stale_counts_and_plain_call_afterwards(precision):
    g, cfg, model, batch, plain = _case("context_tiny_greedy", precision)
    B = int(g["batch"])
    # a second context for the same images: equal stride (17 + 16 rows), other counts
    gen = torch.Generator().manual_seed(5)
    lengths2 = [16, 3, 0, 9]
    batch2 = dict(plain, context=[{"tokens": torch.randint(1, cfg.vocab, (B, 16), generator=gen), "length": torch.tensor(lengths2)}])
    _, _, fresh, _, _ = _case("context_tiny_greedy", precision)
    fresh.engine.set_graph(False)
    want1, want2, want_plain = fresh(batch), fresh(batch2), fresh(plain)
    assert fresh.engine.resident_geometry == (17, 1, [(4, 4)] * B)
    fresh.close()
    _, _, fresh2, _, _ = _case("context_tiny_greedy", precision)
    assert _same(fresh2(plain), want_plain)                    # a plain call on an engine that never saw a context
    fresh2.close()
    got1 = model(batch)                                         # captures the follow-up graph
    assert model.engine.resident_geometry.context == g["context_counts"].tolist()
    got2 = model(batch2)                                        # replays it: same stride, other counts
    assert model.engine.resident_geometry.stride == 33 and model.engine.resident_geometry.context == lengths2
    got1b = model(batch)
    got_plain = model(plain)                                    # leaves key-count mode
    got1c = model(batch)
    model.close()
    assert _same(got1, want1) and _same(got1b, want1) and _same(got1c, want1)
    assert _same(got2, want2) and not _same(got2, got1)
    assert _same(got_plain, want_plain)
    if precision == "f32":
        assert np.array_equal(got1["predictions"].cpu().numpy(), g["predictions"])
        assert np.array_equal(got_plain["predictions"].cpu().numpy(), g["predictions_plain"])


# ---- 5. refusals: by message, before any launch, the resident set as it was --------------------------------------------------------
def _resident_answer(eng, steps=20):
    from generativeimage2text_amd.engine import Engine
    t, lp, _ = eng.generate(None, Engine.make_search("greedy", steps, 1, 1))
    return t.cpu(), lp.cpu()


def test_refusals_leave_the_resident_images():
    from generativeimage2text_amd import engine as E
    from generativeimage2text_amd.model import CaptioningModel
    g, cfg, model, batch, plain = _case("context_tiny_greedy", "f32", max_context=4)
    eng, B = model.engine, int(g["batch"])
    frames = [batch["image"]]
    greedy = E.Engine.make_search("greedy", 20, 1, 1)
    model(plain)                # (the model's calls set the temporal-embedding switch; flipping it would drop the images)
    before = _resident_answer(eng)
    gen0 = eng.generation

    def intact():
        after = _resident_answer(eng)
        return eng.resident == B and torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])

    # over capacity: the engine holds 17 + 4 rows per image; the message names the rows asked for and the capacity
    with pytest.raises(E.GitmiError, match=r"image 2 needs 22 rows \(17 image rows \+ 5 context rows\), the capacity is 21 rows per image"):
        eng.encode_context(frames, [[5, 6], [7, 8, 9], [1, 2]], image_of=[2, 2, 0])
    assert intact()
    with pytest.raises(ValueError, match=r"max_context=16\).*now max_context=4"):
        model(batch)
    assert intact()
    # a length outside its range
    with pytest.raises(E.GitmiError, match=r"length 0 of context segment 1 outside \[1,3\]"):
        eng.encode_context(frames, torch.ones(2, 3).long(), lengths=[2, 0], image_of=[0, 1])
    assert intact()
    # frames == NULL: the context comes with the call that encodes its images
    with pytest.raises(E.GitmiError, match=r"context: frames == NULL"):
        eng.encode_context(None, [[5, 6]] * B)
    assert intact()
    # gitmi_generate / gitmi_search_begin with the new kind
    s = E.Engine.make_search("greedy", 20, 1, 1)
    s.kind = E.SEARCH_CONTEXT
    with pytest.raises(E.GitmiError, match="GITMI_SEARCH_CONTEXT takes context segments: call gitmi_generate_prefixed"):
        eng.generate(frames, s)
    assert intact()
    with pytest.raises(E.GitmiError, match="GITMI_SEARCH_CONTEXT is not a search"):
        eng.search_begin(s, torch.full((B, 1), cfg.sos), cfg.vocab)
    assert intact()
    # ATTEND over a context-carrying resident batch
    eng.encode_context(frames, [[5, 6, 7]], image_of=[1])
    with_ctx = _resident_answer(eng)
    with pytest.raises(E.GitmiError, match="attend: the resident images carry context rows"):
        eng.attend(None, torch.tensor([[cfg.sos, 5, 6]] * B))
    again = _resident_answer(eng)
    assert eng.resident == B and torch.equal(with_ctx[0], again[0]) and torch.equal(with_ctx[1], again[1])
    assert eng.attend(frames, torch.tensor([[cfg.sos, 5, 6]] * B)).shape == (B, 3, cfg.dec_layers, 17 + 3)     # with frames: a plain call
    # ragged mode: mixed shapes plus context is not implemented
    images = [torch.rand(3, 64, 64), torch.rand(3, 48, 64)]
    eng.generate(eng.ragged(images), greedy)
    rag = _resident_answer(eng)
    with pytest.raises(E.GitmiError, match=r"context: ragged image mode \(gitmi_set_image_shape\(e, 0, 0\)\)"):
        eng.encode_context(eng.ragged(images), [[5, 6]] * 2)
    again = _resident_answer(eng)
    assert eng.resident == 2 and torch.equal(rag[0], again[0]) and torch.equal(rag[1], again[1])
    assert eng.generation > gen0
    model.close()


def test_models_whose_widths_differ_are_refused():
    """TINY_L: visual features 192 wide, hidden states 128: the reference's torch.cat fails, the engine says why."""
    from generativeimage2text_amd import engine as E
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel
    from oracle import git_oracle as O
    cfg = O.CONFIGS["TINY_L"]
    w = O.make_weights(cfg, seed=21, eos_bias=1.0)
    frames = [f.cuda() for f in O.make_images(cfg, 2, 1, seed=3)]
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=12, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision="f32", max_batch=2, max_text_len=12, max_context=8)
    model.load_state_dict(w)
    want = model({"image": frames[0]})
    before = _resident_answer(model.engine, 12)
    with pytest.raises(E.GitmiError, match=r"context: visual_feature_size 192 != hidden_size 128"):
        model.engine.encode_context(frames, [[5, 6], [7]])
    after = _resident_answer(model.engine, 12)
    assert model.engine.resident == 2 and torch.equal(before[0], after[0])
    ctx = [{"tokens": torch.tensor([[5, 6], [7, 8]]), "length": torch.tensor([2, 1])}]
    with pytest.raises(ValueError, match="visual_feature_size == hidden_size"):
        model({"image": frames[0], "context": ctx})
    # no image has a non-empty segment: a plain call
    empty = [{"tokens": torch.tensor([[5, 6], [7, 8]]), "length": torch.tensor([0, 0])}]
    assert _same(model({"image": frames[0], "context": empty}), want)
    model.close()
