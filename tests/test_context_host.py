"""Context tokens in the decoder memory (GITMI_SEARCH_CONTEXT), host side: the conversion of the reference's batch['context']
into segments, the max_context capacity arithmetic, the header's description of the new kind and the inputs that are refused.
No GPU."""
import os

import pytest
import torch

from generativeimage2text_amd import engine
from generativeimage2text_amd.engine import GitmiConfig, context_capacity, context_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx(tokens, length):
    return {"tokens": torch.tensor(tokens), "length": torch.tensor(length)}


def test_zero_lengths_are_dropped_and_rows_truncated_to_their_length():
    segs, image_of = context_segments([_ctx([[5, 6, 7, 8], [1, 2, 3, 4], [9, 9, 9, 9]], [2, 0, 4])], 3, 100, 64)
    assert segs == [[5, 6], [9, 9, 9, 9]] and image_of == [0, 2]
    # the ids past a length are padding: whatever they are, even outside the vocabulary, they are never looked at
    segs2, _ = context_segments([_ctx([[5, 6, 999, -4], [777, 2, 3, 4], [9, 9, 9, 9]], [2, 0, 4])], 3, 100, 64)
    assert segs2 == segs
    assert context_segments([_ctx([[1, 2]], [0])], 1, 100, 64) == ([], [])
    assert context_segments([], 2, 100, 64) == ([], []) and context_segments(None, 2, 100, 64) == ([], [])


def test_two_segments_of_one_image_keep_the_order_of_the_list_and_restart_their_positions():
    ctx = [_ctx([[11, 12, 13], [21, 22, 23]], [3, 1]), _ctx([[14, 15], [24, 25]], [2, 2])]
    segs, image_of = context_segments(ctx, 2, 100, 64)
    # list entry by list entry; within the engine the segments of one image are appended in increasing q
    assert segs == [[11, 12, 13], [21], [14, 15], [24, 25]] and image_of == [0, 1, 0, 1]
    assert [s for s, b in zip(segs, image_of) if b == 0] == [[11, 12, 13], [14, 15]]
    # every segment is a row of its own in the table the engine gets: its tokens sit at positions 0 .. len - 1 of that row,
    # so the second segment of image 0 starts at position 0 again (the engine embeds row q at positions 0 .. len_q - 1)
    table = engine.id_table(segs)
    assert table.tolist() == [[11, 12, 13], [21, 0, 0], [14, 15, 0], [24, 25, 0]]
    # a segment may be as long as the textual embedding has positions, and no longer
    assert context_segments([_ctx([list(range(1, 65))], [64])], 1, 100, 64)[0] == [list(range(1, 65))]


def test_bad_ids_lengths_and_shapes_raise():
    with pytest.raises(ValueError, match=r"outside \[0, 100\)"):
        context_segments([_ctx([[5, 100, 7]], [2])], 1, 100, 64)
    with pytest.raises(ValueError, match=r"outside \[0, 100\)"):
        context_segments([_ctx([[-1, 3, 7]], [1])], 1, 100, 64)
    with pytest.raises(ValueError, match="exceeds the 8 positions"):
        context_segments([_ctx([list(range(1, 10))], [9])], 1, 100, 8)
    with pytest.raises(ValueError, match=r"length 4 of image 0 outside \[0, 3\]"):
        context_segments([_ctx([[1, 2, 3]], [4])], 1, 100, 64)
    with pytest.raises(ValueError, match=r"length -1 of image 0"):
        context_segments([_ctx([[1, 2, 3]], [-1])], 1, 100, 64)
    with pytest.raises(ValueError, match=r"must be \[B, Lc\]"):
        context_segments([_ctx([[1, 2, 3]], [1])], 2, 100, 64)


def test_max_context_arithmetic_and_default_footprint():
    # the default leaves gitmi_config as it is: max_image_tokens untouched, whatever it was
    assert context_capacity(224, 16, 0, 1, 0) == 0 and context_capacity(224, 16, 1201, 1, 0) == 1201
    # N = 197 rows per frame; the workspaces hold max_frames x max(N, max_image_tokens) rows per image
    for frames, want in ((1, 32), (1, 1), (6, 32), (6, 5), (3, 100)):
        tokens = context_capacity(224, 16, 0, frames, want)
        assert frames * tokens >= frames * 197 + want > frames * (tokens - 1)
    # on top of a capacity for larger images
    assert context_capacity(224, 16, 1201, 1, 64) == 1265
    # TINY: 17 rows per frame
    assert context_capacity(64, 16, 0, 1, 16) == 33 and context_capacity(64, 16, 0, 3, 8) == 20
    c = GitmiConfig()
    assert engine.C.sizeof(c) == 84 and engine.SEARCH_CONTEXT == 5
    import inspect
    from generativeimage2text_amd.model import CaptioningModel
    assert inspect.signature(engine.Engine.__init__).parameters["max_context"].default == 0
    assert inspect.signature(CaptioningModel.__init__).parameters["max_context"].default == 0


def test_geometry_reports_stride_and_context_counts_and_stays_a_plain_triple():
    g = engine.Geometry(48, 1, [(4, 4)] * 3, image_rows=17, context=[0, 1, 16])
    assert g == (48, 1, [(4, 4)] * 3) and g.stride == 48 and g.image_rows == 17 and g.context == [0, 1, 16]
    Nk, F, grids = g
    assert (Nk, F, len(grids)) == (48, 1, 3)
    plain = engine.Geometry(17, 1, [(4, 4)] * 2)
    assert plain.image_rows == 17 and plain.context == [0, 0]


def test_header_documents_the_context_kind():
    hdr = open(os.path.join(ROOT, "include", "gitmi.h")).read()
    flat = " ".join(hdr.split())
    assert "#define GITMI_SEARCH_CONTEXT 5" in flat
    assert "#define GITMI_ABI_VERSION 10" in " ".join(hdr.split())
    for phrase in ("search->kind == GITMI_SEARCH_CONTEXT", "positions restarting at 0 in every segment",
                   "ntok[b] = F N + C_b", "must be non-NULL", "increasing q", "key-count mode",
                   "{ row stride of an image's block, max_b C_b, sum_b C_b, 0 }",
                   "GITMI_SEARCH_ATTEND over a context-carrying resident batch is refused",
                   "fails before any launch", "ragged image mode", "vit_width != dec_hidden",
                   "gitmi_generate and gitmi_search_begin refuse this kind", "A clone starts with nothing resident",
                   "keyed on the row stride"):
        assert phrase in flat.replace("* ", ""), phrase
    exp = open(os.path.join(ROOT, "include", "gitmi_experiment.h")).read()
    assert "gitmi_debug_context_embed(" in exp and "gitmi_debug_context_embed" in engine.EXPERIMENT_SYMBOLS
    assert "gitmi_debug_context_embed" not in engine.EXPORTED_SYMBOLS and len(engine.EXPORTED_SYMBOLS) == 40


class _NoEngine:
    """Stands in for Engine where a CaptioningModel is built without a GPU: records the keyword arguments."""

    def __init__(self, cfg, **kw):
        self.kw = kw


def _model(monkeypatch, **kw):
    from generativeimage2text_amd import model as M
    from generativeimage2text_amd.configs import config_for_model
    monkeypatch.setattr(M, "Engine", _NoEngine)
    cfg = config_for_model("GIT_BASE")
    dec = M.AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=20, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    return M.CaptioningModel(cfg, dec, **kw)


def test_context_not_share_embedding_raises(monkeypatch):
    with pytest.raises(NotImplementedError, match=r"decoder\.py:825"):
        _model(monkeypatch, context_not_share_embedding=True)
    assert _model(monkeypatch).engine.kw["max_context"] == 0
    assert _model(monkeypatch, max_context=32).engine.kw["max_context"] == 32


def test_bi_valid_mask_caption_raises_in_both_modes(monkeypatch):
    m = _model(monkeypatch)
    m._loaded = True
    batch = {"image": torch.zeros(1, 3, 224, 224), "bi_valid_mask_caption": torch.ones(1, 4, 4)}
    with pytest.raises(NotImplementedError, match="bi_valid_mask_caption"):
        m.submit(batch)
    with pytest.raises(NotImplementedError, match="bi_valid_mask_caption"):
        m(batch)
    with pytest.raises(NotImplementedError, match="bi_valid_mask_caption"):
        m.train()(dict(batch, caption_tokens=torch.ones(1, 4).long(), need_predict=torch.ones(1, 4).long()))
