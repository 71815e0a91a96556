"""GPU: the kernel-shape policy of gitmi_set_shared_device never changes results (include/gitmi.h); a clone inherits the
current policy of its source."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", ["bf16", "f16", "f32"])
def test_shared_device_policy_is_bitwise_neutral(precision):
    """gitmi_set_shared_device changes kernel SHAPES (256-row GEMM tiles everywhere, two (sentence, head) pairs per
    attention workgroup), never results: features, ids and log-probs of the benchmark geometry are bit-identical, for
    a context and for a clone that inherits the setting.  This is the guard of include/gitmi.h's promise for
    gitmi_set_shared_device -- in particular that the streaming decode attention (solo policy) and the register form (serving
    policy) agree bit for bit (`fp contract(off)` + explicit fmaf in both, kernels_attn_decode.hip) -- in every operand build."""
    from generativeimage2text_amd.configs import config_for_model
    from generativeimage2text_amd.engine import Engine
    from generativeimage2text_amd.synthetic import random_frames, random_state_dict
    cfg = config_for_model("GIT_BASE")
    B = 8 if precision == "f32" else 64
    eng = Engine(cfg, precision=precision, max_batch=B, max_beams=4, max_frames=1, max_text_len=20)
    eng.load_state_dict(random_state_dict(cfg, seed=1234))
    frames = random_frames(cfg, B, 1, seed=0)
    out = {}
    for search in (Engine.make_search("greedy", 20, 1, 1), Engine.make_search("beam", 20, 4, 2, 0.6)):
        for on in (False, True):
            eng.set_shared_device(on)
            feats = eng.encode(frames, return_features=True)
            tok, lp, _ = eng.generate(frames, search)
            out[on] = (feats.clone(), tok.clone(), lp.clone())
        clone = eng.clone()                                  # inherits "on"
        tok_c, lp_c, _ = clone.generate(frames, search)
        clone.close()
        assert torch.equal(out[False][0], out[True][0])
        assert torch.equal(out[False][1], out[True][1]) and torch.equal(out[False][2], out[True][2])
        assert torch.equal(tok_c, out[True][1]) and torch.equal(lp_c, out[True][2])
    eng.close()


def test_clone_inherits_the_current_switches_of_its_source():
    """A clone takes the CURRENT gitmi_set_ln_fold / gitmi_set_shared_device / gitmi_set_temporal_embedding state of its
    source, not the defaults of a fresh context: after the three setters, features, ids and log-probs of the clone are
    bit-identical to the source's.  The folded and the unfolded encoder differ by rounding (B x 197 > 512 rows, so the fold is
    live), and a video model's features differ with and without the temporal embedding, so equality holds only if the clone
    really took the switches; both discriminations are asserted."""
    from generativeimage2text_amd.configs import config_for_model
    from generativeimage2text_amd.engine import Engine
    from generativeimage2text_amd.synthetic import random_frames, random_state_dict
    search = Engine.make_search("greedy", 20, 1, 1)
    for model, B, F in (("GIT_BASE", 4, 1), ("GIT_BASE_VATEX", 3, 2)):
        cfg = config_for_model(model)
        eng = Engine(cfg, precision="f16", max_batch=B, max_beams=1, max_frames=F, max_text_len=20)
        eng.load_state_dict(random_state_dict(cfg, seed=1234))
        frames = random_frames(cfg, B, F, seed=0)
        feats = {}
        for fold, temb in ((False, False), (True, False), (True, True)):
            eng.set_ln_fold(fold)
            eng.set_shared_device(True)
            eng.set_temporal_embedding(temb)
            f = eng.encode(frames, return_features=True).clone()
            tok, lp, _ = eng.generate(frames, search)
            clone = eng.clone()
            f_c = clone.encode(frames, return_features=True).clone()
            tok_c, lp_c, _ = clone.generate(frames, search)
            clone.close()
            assert torch.equal(f_c, f), (model, fold, temb)
            assert torch.equal(tok_c, tok) and torch.equal(lp_c, lp), (model, fold, temb)
            feats[fold, temb] = f
        assert not torch.equal(feats[False, False], feats[True, False]), model        # the fold switch changes the rounding
        if cfg.num_frames:
            assert not torch.equal(feats[True, False], feats[True, True]), model      # the embedding switch changes the features
        eng.close()
