"""Attention maps (GITMI_SEARCH_ATTEND), host side (no GPU): the header defines the kind and documents the output layout, the
Python constant matches it, and the front end routes CaptioningModel.attend like score -- images to a full call, None to a
follow-up on the handle's context, a stale handle refused -- and splits / reshapes what the engine returns."""
import os
import re
import types

import pytest
import torch

from generativeimage2text_amd import engine
from generativeimage2text_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = 2


def test_header_defines_the_kind_and_documents_the_layout():
    hdr = open(os.path.join(ROOT, "include", "gitmi.h")).read()
    assert re.search(r"#define\s+GITMI_SEARCH_ATTEND\s+4\b", hdr)
    assert engine.SEARCH_ATTEND == 4 and engine.SEARCH_SCORE == 3
    doc = hdr[hdr.index("---- attention maps"):]
    doc = doc[:doc.index("int  gitmi_generate_prefixed(")]
    text = " ".join(doc.replace("*", " ").split())
    for phrase in ("GITMI_SEARCH_ATTEND", "[Q, ld, dec_layers, Kc]", "Kc = Nk + ld", "F N for uniform input", "Nmax in ragged mode",
                   "att[q, j, l, k] = (1/H) sum_h softmax_k'", "frame-major", "class token first", "column Nk + t is text position t",
                   "rows j >= len_q", "text columns t > j", "image columns >= n_b", "exactly 0",
                   "info_out = { ld, Kc, dec_layers, sentences with a non-finite value }", "the vocabulary head does not run",
                   "gitmi_generate and gitmi_search_begin refuse this kind", "no hipGraph", "engines that never attend keep their footprint"):
        assert phrase in text, phrase
    exp = open(os.path.join(ROOT, "include", "gitmi_experiment.h")).read()
    assert "gitmi_debug_score_attn_map(" in exp and "gitmi_debug_score_attn_map" in engine.EXPERIMENT_SYMBOLS


class _FakeEngine:
    """An engine context as the front end sees it.  attend answers with a map that names its own indices:
    att[q, j, l, k] = 1000 q + 100 j + 10 l + k / 1000, so every reshape can be checked by value."""

    def __init__(self, name, patch=4, max_tokens=40):
        self.name, self.calls = name, []
        self.resident, self.generation, self.resident_geometry = None, 0, None
        self.c = types.SimpleNamespace(max_batch=8, max_frames=3, patch=patch)
        self.max_tokens = max_tokens

    def set_temporal_embedding(self, on):
        pass

    def check_finite(self, info):
        pass

    def ragged(self, images):
        return types.SimpleNamespace(shapes=[tuple(im.shape[1:]) for im in images])

    def _encode(self, frames):
        if frames is None:
            return
        p = self.c.patch
        if hasattr(frames, "shapes"):
            self.resident = len(frames.shapes)
            self.resident_geometry = (self.max_tokens, 1, [(h // p, w // p) for h, w in frames.shapes])
        else:
            B, _, H, W = frames[0].shape
            self.resident = int(B)
            self.resident_geometry = (len(frames) * ((H // p) * (W // p) + 1), len(frames), [(H // p, W // p)] * B)
        self.generation += 1

    def generate(self, frames, search, prefix=None, sync=True, host_out=False):
        self.calls.append(("generate", frames is None))
        self._encode(frames)
        B = self.resident
        return torch.full((B, search.max_steps), 102), torch.zeros(B), torch.tensor([search.max_steps, 0, 0, 0])

    def attend(self, frames, tokens, lengths=None, image_of=None):
        self.calls.append(("attend", frames is None, list(lengths), None if image_of is None else list(image_of)))
        self._encode(frames)
        Q, L = tokens.shape
        Kc = self.resident_geometry[0] + L
        idx = torch.meshgrid(torch.arange(Q), torch.arange(L), torch.arange(LAYERS), torch.arange(Kc), indexing="ij")
        return (1000 * idx[0] + 100 * idx[1] + 10 * idx[2]).double() + idx[3].double() / 1000


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: types.SimpleNamespace(synchronize=lambda: None))


def _model(contexts=1, num_frames=0):
    cfg = types.SimpleNamespace(num_frames=num_frames, sos=101, eos=102, vocab=30522)
    m = object.__new__(M.CaptioningModel)
    m.cfg = cfg
    m.decoder = M.AutoRegressiveBeamSearch(eos_index=102, max_steps=10, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    m.engine, m._loaded, m.training = _FakeEngine("ctx0"), True, False
    if contexts > 1:
        m._ctxs = [m.engine] + [_FakeEngine(f"ctx{i}") for i in range(1, contexts)]
        m._streams = [None] * contexts
        m._next = 0
    return m


def _value(q, j, l, k):
    return 1000 * q + 100 * j + 10 * l + k / 1000


def test_attend_routes_images_to_a_full_call_and_none_to_a_followup(no_device):
    m = _model()
    with pytest.raises(M.StaleImagesError, match="no resident images"):
        m.attend(None, [[101, 5]], image_of=[0])
    maps = m.attend(torch.zeros(2, 3, 8, 12), [[101, 5, 6], [101]])          # grid 2 x 3: 7 tokens per image
    assert m.engine.calls == [("attend", False, [3, 1], None)] and m.engine.resident == 2
    assert maps.image.shape == (2, 3, LAYERS, 7) and maps.text.shape == (2, 3, LAYERS, 3)
    assert maps.image[1, 2, 1, 6] == _value(1, 2, 1, 6) and maps.text[1, 2, 1, 2] == _value(1, 2, 1, 7 + 2)
    # captions as a zero-padded tensor: a caption ends at its last id
    m.attend(None, torch.tensor([[101, 5, 0, 0], [101, 7, 8, 9]]), image_of=[1, 1])
    assert m.engine.calls[-1] == ("attend", True, [2, 4], [1, 1])
    assert m.engine.generation == 1                                         # the follow-up touched no image
    m({"image": torch.zeros(3, 3, 8, 8)})
    maps = m.attend(None, [[101, 5, 102]], image_of=[2])                     # generate, then attend: no re-encode
    assert m.engine.calls[-2:] == [("generate", False), ("attend", True, [3], [2])]
    assert maps.image.shape == (1, 3, LAYERS, 5)


def test_attend_runs_on_the_context_of_its_handle_and_refuses_a_stale_one(no_device):
    m = _model(contexts=2)
    pa = m.submit({"image": torch.zeros(2, 3, 8, 8)})
    pb = m.submit({"image": torch.zeros(3, 3, 8, 8)})
    m.attend(None, [[101, 5]], image_of=[2])                                 # without on=: the most recent call's context
    assert pb.engine.calls[-1][:2] == ("attend", True) and len(pa.engine.calls) == 1
    m.attend(None, [[101, 5]], image_of=[1], on=pa)
    assert pa.engine.calls[-1][:2] == ("attend", True)
    m.attend(None, [[101, 5]], image_of=[0], on=pb.result())                 # the result object is a handle too
    assert len(pb.engine.calls) == 3 and m._next == 2
    pc = m.submit({"image": torch.zeros(2, 3, 8, 8)})                        # back on ctx0: pa's images are replaced
    assert pc.engine is pa.engine
    with pytest.raises(M.StaleImagesError, match="no longer resident"):
        m.attend(None, [[101, 5]], image_of=[0], on=pa)
    with pytest.raises(TypeError):
        m.attend(None, [[101, 5]], image_of=[0], on={"predictions": []})


def test_patch_grid_uniform_frames_and_ragged(no_device):
    # uniform, one frame: 8 x 12 at patch 4 -> grid 2 x 3, column 0 the class token
    m = _model()
    maps = m.attend(torch.zeros(2, 3, 8, 12), [[101, 5, 6], [101, 7]], image_of=[1, 0])
    g = maps.patch_grid(0)
    assert g.shape == (3, LAYERS, 1, 2, 3)
    for j, l, r, c in ((0, 0, 0, 0), (2, 1, 1, 2), (1, 0, 1, 0)):
        assert g[j, l, 0, r, c] == _value(0, j, l, 1 + 3 * r + c)
    assert maps.patch_grid(1).shape == (2, LAYERS, 1, 2, 3)                  # the caption's own rows only
    # F = 3 frames: frame-major, a class column in front of every frame's patches
    m = _model(num_frames=3)
    maps = m.attend([torch.zeros(1, 3, 8, 8)] * 3, [[101, 5]])
    assert maps.image.shape == (1, 2, LAYERS, 15)
    g = maps.patch_grid(0)
    assert g.shape == (2, LAYERS, 3, 2, 2)
    for f in range(3):
        assert g[1, 1, f, 1, 0] == _value(0, 1, 1, 5 * f + 1 + 2)
    # ragged: every image its own grid inside the capacity rows
    m = _model()
    maps = m.attend([torch.zeros(3, 8, 16), torch.zeros(3, 12, 4)], [[101, 5], [101, 6, 7]])
    assert m.engine.calls[-1][:2] == ("attend", False)
    assert maps.image.shape == (2, 3, LAYERS, 40) and maps.text.shape == (2, 3, LAYERS, 3)
    g0, g1 = maps.patch_grid(0), maps.patch_grid(1)
    assert g0.shape == (2, LAYERS, 1, 2, 4) and g1.shape == (3, LAYERS, 1, 3, 1)
    assert g0[1, 0, 0, 1, 3] == _value(0, 1, 0, 1 + 4 + 3) and g1[2, 1, 0, 2, 0] == _value(1, 2, 1, 1 + 2)
