#!/usr/bin/env python
"""SHA-256 digests of what the forward schedule (engine.hip: encode, prefill, decode chain, text pass) computes on the paths
bench.py never takes.  A change to the host side of the schedule must leave every digest as it was: run this once per build
and compare the two JSONs key for key.  A difference in "features" points at the encoder; one only in the later outputs at the
prefill, the decode chain or the text pass.

Model: GIT_BASE widths (768: the LayerNorm fold exists) with 2 ViT blocks and 3 decoder layers (first, middle and last prefill
layer all occur), seeded oracle weights and images.  The fold needs more than 512 rows: 3 images at 224 px are 591.

    a  f16, fold on, B = 3                      e  f32, B = 3
    h  a's engine, set_shared_device(True)      f  f16 ragged: three sizes, capacity 224 x 256 (3 x 225 = 675 rows)
    b  a's engine, set_ln_fold(False)           g  f16, num_frames = 2: two frames, B = 2 (788 rows)
    c  a's engine, B = 2: 394 rows, the gate picks the unfolded launches
    d  bf16, B = 3

Per case: encode() features; step_logits of a 3-token history at R = B and R = 2B; generate greedy and beam_size = 2
(max_steps 6), graph on and off: tokens and log-probs; score and attend of B + 1 sentences of unequal lengths whose image_of
reuses image 0; the same score as a follow-up call (frames=None).

    python tools/schedule_digest.py [--out FILE]          # one JSON line: {case: {output: sha256}}"""
from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 6                   # max_steps of the searches, and the longest sentence


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(eng, frames, B: int, vocab: int, sos: int) -> dict:
    """every output of the list above for one engine state; frames: what encode / generate / score take"""
    import torch
    from generativeimage2text_amd.engine import Engine
    g = torch.Generator().manual_seed(77)
    out = {"features": sha(eng.encode(frames))}
    for R in (B, 2 * B):
        hist = torch.randint(1000, vocab, (R, 3), generator=g)
        hist[:, 0] = sos
        out["step_logits_R%d" % R] = sha(eng.step_logits(hist))
    for name, search in (("greedy", Engine.make_search("greedy", T, 1, 1)), ("beam2", Engine.make_search("beam", T, 2, 2, 0.6))):
        for graph in (True, False):
            eng.set_graph(graph)
            tok, lp, _ = eng.generate(frames, search)
            key = "generate_%s_%s" % (name, "graph" if graph else "eager")
            out[key + "_tokens"], out[key + "_logprobs"] = sha(tok), sha(lp)
    eng.set_graph(True)
    Q = B + 1
    lens = [T - (q % 3) for q in range(Q)]
    sent = torch.randint(1000, vocab, (Q, T), generator=g)
    sent[:, 0] = sos
    image_of = list(range(B)) + [0]
    out["score"] = sha(eng.score(frames, sent, lengths=lens, image_of=image_of))
    out["attend"] = sha(eng.attend(frames, sent, lengths=lens, image_of=image_of))
    out["score_followup"] = sha(eng.score(None, sent, lengths=lens, image_of=image_of))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the JSON to this file")
    args = ap.parse_args()
    import torch
    from generativeimage2text_amd.engine import Engine
    from oracle import git_oracle as O
    cfg = dataclasses.replace(O.CONFIGS["GIT_BASE"], name="GIT_BASE_2x3", vit_layers=2, dec_layers=3)
    cfg2 = dataclasses.replace(cfg, name="GIT_BASE_2x3_F2", num_frames=2)

    def engine(c, precision, frames=1, hw=None):
        eng = Engine(c, precision=precision, max_batch=3, max_beams=2, max_frames=frames, max_text_len=8, max_image_hw=hw)
        eng.load_state_dict(O.make_weights(c, seed=91, tie_output=False, eos_bias=-2.0))
        return eng

    def images(c, B, frames=1):
        return [f.cuda() for f in O.make_images(c, B, frames, seed=92)]

    res = {}
    eng = engine(cfg, "f16")
    res["a_f16_fold"] = run_case(eng, images(cfg, 3), 3, cfg.vocab, cfg.sos)
    eng.set_shared_device(True)
    res["h_f16_fold_shared_device"] = run_case(eng, images(cfg, 3), 3, cfg.vocab, cfg.sos)
    eng.set_shared_device(False)
    eng.set_ln_fold(False)
    res["b_f16_unfolded"] = run_case(eng, images(cfg, 3), 3, cfg.vocab, cfg.sos)
    eng.set_ln_fold(True)
    res["c_f16_fold_394_rows"] = run_case(eng, images(cfg, 2), 2, cfg.vocab, cfg.sos)
    eng.close()
    for key, precision in (("d_bf16", "bf16"), ("e_f32", "f32")):
        eng = engine(cfg, precision)
        res[key] = run_case(eng, images(cfg, 3), 3, cfg.vocab, cfg.sos)
        eng.close()
    eng = engine(cfg, "f16", hw=(224, 256))
    gen = torch.Generator().manual_seed(93)
    ragged = [torch.randn(3, h, w, generator=gen).cuda() for h, w in ((224, 256), (160, 192), (96, 240))]
    res["f_f16_ragged"] = run_case(eng, eng.ragged(ragged), 3, cfg.vocab, cfg.sos)
    eng.close()
    eng = engine(cfg2, "f16", frames=2)
    res["g_f16_two_frames"] = run_case(eng, images(cfg2, 2, 2), 2, cfg.vocab, cfg.sos)
    eng.close()
    torch.cuda.synchronize()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, sort_keys=True, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
