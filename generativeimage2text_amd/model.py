"""Host-side mirror of the reference's model interface for the hot path.

Same names, argument meaning and return conventions as
  generativeimage2text/model.py:9-61              get_git_model
  generativeimage2text/layers/decoder.py:774-1054 CaptioningModel (forward / infer)
  generativeimage2text/layers/decoder.py:208-222  AutoRegressiveBeamSearch  (constructor arguments)
  generativeimage2text/layers/decoder.py:1056-1081 GeneratorWithBeamSearch (constructor arguments)
but all arithmetic happens in libgitmi.so (HIP, gfx950).  The two search classes hold the reference's constructor
arguments; the search itself runs on the device (csrc/kernels_search.hip), inside gitmi_generate for model(batch) and
behind `decoder.search(start_predictions, step)` for callers that bring their own `step` (decoder.py:224-231, 1083-1092).
"""
from __future__ import annotations

import logging
import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import torch

from .configs import GitModelConfig, config_from_param
from .engine import CONSTRAINT_KEYS, TRACE_MAX_ALTERNATIVES, Engine, banned_sequence_tables, constraint_tables, context_segments, id_table

# search_param keys of the per-sentence decoding constraints (CaptioningModel._constraints)
CONSTRAINT_PARAMS = CONSTRAINT_KEYS + ("bad_words", "bad_sequences", "bad_phrases")


# search_param keys of the per-token trace (CaptioningModel._trace)
TRACE_PARAMS = ("output_scores", "top_logprobs")


def trace_param(search_param: Optional[dict], kind: str) -> Optional[int]:
    """The per-token trace a request asks for (include/gitmi.h GITMI_SEARCH_TRACE) from its search_param: output_scores (bool)
    asks for the log-prob of every returned token, top_logprobs (0 .. 8; above 0 implies output_scores) for that many
    alternatives per position as well.  `kind`: the decoder's search.  -> the number of alternatives n, or None: no trace, the
    request builds nothing and arms nothing."""
    sp = search_param or {}
    n = sp.get("top_logprobs", 0)
    n = 0 if n is None else n
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= TRACE_MAX_ALTERNATIVES:
        raise ValueError(f"top_logprobs {n!r} outside [0, {TRACE_MAX_ALTERNATIVES}]")
    if not sp.get("output_scores", False) and n == 0:
        return None
    if kind == "trie":
        raise NotImplementedError("output_scores / top_logprobs on the trie search are not implemented")
    if n > 0 and sp.get("do_sample", False):
        raise NotImplementedError("top_logprobs with do_sample: alternatives under sampling are not implemented (output_scores alone works)")
    return n


def _arm_trace(eng, n: Optional[int], Q: int, search, host: bool):
    """Arm the trace of a request (trace_param) of Q sentences on `eng`, right before the call that consumes it -> its buffers, or None"""
    if n is None:
        return None
    return eng.trace(Q, max(1, int(search.num_keep_best)), int(search.max_steps), n, host_out=host)


def format_trace(trace, spans):
    """The trace of a finished call (Engine.trace's buffers: lp [S, T, 1 + n], tokens [S, T, n] or None) cut like its predictions:
    spans[o] = (first, end) positions of returned sequence o.  -> {'token_logprobs': per sequence the log-prob of every token,
    'top_tokens' / 'top_logprobs': per sequence [len, n] lists (n > 0 only)}"""
    lp, tok = trace
    lp = lp.cpu()
    out = {"token_logprobs": [lp[o, a:b, 0].tolist() for o, (a, b) in enumerate(spans)]}
    if tok is not None:
        tok = tok.cpu()
        out["top_tokens"] = [tok[o, a:b].tolist() for o, (a, b) in enumerate(spans)]
        out["top_logprobs"] = [lp[o, a:b, 1:].tolist() for o, (a, b) in enumerate(spans)]
    return out


def trace_spans(n_seq: int, nout: int, T: int, sent, prefix, kind: str):
    """The positions format_predictions keeps of every returned sequence (n_seq sentences x nout sequences, T positions): the
    same arguments, the same rule -> [(first, end)] per returned sequence"""
    autoregressive = kind in ("autoregressive", "trie")
    spans = []
    for q in range(n_seq):
        if isinstance(prefix, (list, tuple)):
            P, L, early = int(prefix[q]), int(sent[q][0]), int(sent[q][1])
            first = P
        else:
            P, L, early = (1 if prefix is None else int(prefix)), int(sent[0]), int(sent[1])
            first = 0 if prefix is None else P
        if autoregressive:
            # the early-[SEP] return keeps position P alone, and a given prefix is then removed from THAT one-token row
            # (format_predictions, as decoder.py:1004-1006 does): nothing is left of it
            span = ((P, P + 1) if first == 0 else (P + 1, P + 1)) if early else (first, L)
        else:
            span = (first, T)
        spans.extend([span] * nout)
    return spans


def _arm(eng, ban) -> None:
    """Arm the constraints of a request (CaptioningModel._constraints) on `eng`: (words, table), or with banned sequences
    (words, table, pool) -- only then does the call carry the `sequences` keyword."""
    if len(ban) == 2:
        eng.constrain(ban[0], ban[1])
    else:
        eng.constrain(ban[0], ban[1], sequences=ban[2])


# ---- decoder.search(start_predictions, step): the reference's search seam as a method ----------------------------
# The search itself runs on the device (csrc/kernels_search.hip) behind gitmi_search_begin / rows / advance / finish.
# Those entry points live on an engine context, so a search with a caller-supplied `step` gets a SMALL context of its own
# (a minimal model geometry with placeholder weights that are never used: only the search state and kernels are).
_SEARCH_ENGINES: Dict[tuple, Engine] = {}


def _search_engine(eos: int, sos: int, B: int, beams: int, T: int, factory=None) -> Engine:
    """A context that only hosts searches: capacity (B sentences, `beams` beams, T positions).  `factory` (tests) builds
    the context instead of Engine."""
    key = (int(eos), int(B), int(beams), int(T))
    eng = _SEARCH_ENGINES.get(key)
    if eng is None:
        if factory is not None:
            eng = factory(eos, B, beams, T)
        else:
            from .synthetic import random_state_dict
            cfg = GitModelConfig(name="search-only", image_size=64, patch=16, vit_width=128, vit_layers=2, vit_heads=2,
                                 dec_hidden=128, dec_layers=2, dec_heads=2, dec_ffn=512, vocab=1000, max_pos=max(64, int(T)),
                                 sos=int(sos), eos=int(eos))
            eng = Engine(cfg, precision="f32", max_batch=int(B), max_beams=int(beams), max_frames=1, max_text_len=int(T))
            eng.load_state_dict(random_state_dict(cfg, seed=0))
        if len(_SEARCH_ENGINES) >= 4:                        # a few capacities at most stay alive
            _SEARCH_ENGINES.pop(next(iter(_SEARCH_ENGINES))).close()
        _SEARCH_ENGINES[key] = eng
    return eng


def _begin_and_run(decoder, start_predictions, step, search_struct, first_step_rows_per_sentence, stop_when_all_eos, fmt,
                   engine_factory=None):
    start = start_predictions.detach().to("cpu", torch.int64)
    assert start.dim() == 2, "start_predictions is [batch, prefix_length]"
    B, P = start.shape
    T, k = int(decoder.max_steps), int(decoder.beam_size)
    if P > T:
        raise ValueError(f"prefix of {P} tokens exceeds max_steps={T}")
    dev = start_predictions.device
    eng = _search_engine(decoder._eos_index, int(start[0, 0]), B, k, T, engine_factory)
    if getattr(decoder, "kind", "") == "trie":
        eng.set_trie(*decoder.trie.csr())
    # the vocabulary size is only known from the first logits: the first `step` call is made on the start rows as the
    # reference makes it (one row per sentence for AutoRegressiveBeamSearch, decoder.py:259; B*k rows for the generator,
    # decoder.py:1101-1102), then the device search begins and receives those logits as its first advance
    if P < T:
        first_rows = start if (first_step_rows_per_sentence or k == 1) else start.repeat_interleave(k, dim=0)
        logits = step(first_rows.to(dev))
        if logits.shape[0] != B * k:
            logits = logits.repeat_interleave(k, dim=0)
        eng.search_begin(search_struct, start, int(logits.shape[-1]))
        eng.search_advance(logits)
    else:
        eng.search_begin(search_struct, start, 2)
    while True:
        rows = eng.search_rows()                                        # int64 [B*k, t], rows of a sentence contiguous
        t = int(rows.shape[1])
        if t >= T:
            break
        if stop_when_all_eos and bool((rows[:, -1] == decoder._eos_index).all()):
            break                                                       # decoder.py:319-320
        eng.search_advance(step(rows.to(dev)))
        if not stop_when_all_eos and eng.search_done_count() >= B:
            break                                                       # decoder.py:1251: every sentence is done
    tokens, logprobs, info = eng.search_finish()
    seq_len, early = int(info[0]), int(info[1])
    tokens, logprobs = tokens.to(dev), logprobs.to(dev)
    if fmt == "autoregressive":
        if early:                                                       # decoder.py:279-291
            return tokens[:, P:P + 1], logprobs[:, None]
        return tokens[:, :seq_len], logprobs
    return tokens, (logprobs[:, None] if logprobs.dim() == 1 else logprobs)      # [B, num_keep_best]


class AutoRegressiveBeamSearch:
    """Constructor-compatible with the reference class (decoder.py:209-222)."""

    def __init__(self, eos_index: int, max_steps: int = 50, beam_size: int = 5,
                 per_node_beam_size: int = 2, fix_missing_prefix: bool = False) -> None:
        assert fix_missing_prefix, "should always true"          # decoder.py:222
        self._eos_index = eos_index
        self.max_steps = max_steps
        self.beam_size = beam_size
        self.per_node_beam_size = per_node_beam_size or beam_size
        self.kind = "autoregressive"
        self.length_penalty = 1.0

    def search(self, start_predictions: torch.Tensor, step, only_return_best: bool = True, do_sample: bool = False,
               top_k: int = 0, top_p=None, num_return_sequences: int = 1, temperature: float = 1, _engine_factory=None):
        """decoder.py:224-440 with a caller-supplied `step(rows int64 [R, t]) -> logits fp32 [R, V]`:
        -> (predictions int64 [B, length <= max_steps] incl. the start tokens, logprobs fp32 [B]); when every sentence
        ends at its first step with beam_size == 1: ([B, 1], [B, 1]) (decoder.py:279-291).  The sampling branch and
        only_return_best=False are used by SCST training only and are not implemented."""
        if do_sample or not only_return_best or num_return_sequences != 1 or temperature != 1:
            raise NotImplementedError("AutoRegressiveBeamSearch.search: only the inference form "
                                      "(only_return_best=True, do_sample=False) is implemented")
        s = Engine.make_search("autoregressive", self.max_steps, self.beam_size, self.per_node_beam_size)
        return _begin_and_run(self, start_predictions, step, s, first_step_rows_per_sentence=True, stop_when_all_eos=True,
                              fmt="autoregressive", engine_factory=_engine_factory)


class TokenTrie:
    """Same interface as the reference's TokenTrie (trie_decoder.py:224-257): construct / insert / get_valid / reset /
    get_curr_valid / move.  The search itself walks a CSR copy of it on the device (`csr()` -> gitmi_set_trie)."""

    def __init__(self):
        self._children = [{}]                  # node -> {token: child node}; node 0 is the root
        self._ends = []                        # the node every inserted sequence ends in, in insertion order
        self.curr = 0

    @classmethod
    def construct(cls, all_tokens):
        ret = cls()
        for ts in all_tokens:
            ret.insert(ts)
        return ret

    def insert(self, tokens):
        cur = 0
        for t in tokens:
            nxt = self._children[cur].get(int(t))
            if nxt is None:
                nxt = len(self._children)
                self._children.append({})
                self._children[cur][int(t)] = nxt
            cur = nxt
        self._ends.append(cur)

    def get_valid(self, tokens):
        cur = 0
        for t in tokens:
            cur = self._children[cur].get(int(t))
            if cur is None:
                return []
        return list(self._children[cur].keys())

    def reset(self):
        self.curr = 0

    def get_curr_valid(self):
        return list(self._children[self.curr].keys())

    def move(self, t):
        assert int(t) in self._children[self.curr]
        self.curr = self._children[self.curr][int(t)]

    def preorder(self):
        """The trie below its (token-less) root in DFS pre-order, children in insertion order -- the node order of
        Engine.score_tree.  -> (tokens, depths, terminal): token id and depth (1 for the first token of a sequence) of every
        node, and terminal[s] = the index of the node inserted sequence s ends in (duplicates share a node, a sequence that is
        a prefix of another ends in an inner node; -1 for an empty sequence, which ends in the root)."""
        tokens, depths, index = [], [], {0: -1}
        stack = [(0, iter(self._children[0].items()))]
        while stack:
            step = next(stack[-1][1], None)
            if step is None:
                stack.pop()
                continue
            tok, node = step
            index[node] = len(tokens)
            tokens.append(tok)
            depths.append(len(stack))
            stack.append((node, iter(self._children[node].items())))
        return tokens, depths, [index[n] for n in self._ends]

    def csr(self):
        off, tok, node = [0], [], []
        for ch in self._children:
            tok.extend(ch.keys())
            node.extend(ch.values())
            off.append(len(tok))
        return off, tok, node


def get_output_vocab_tokens(tokenizer, texts):
    """trie_decoder.py:18-25: every allowed answer as its token ids + [SEP]."""
    return [tokenizer(a, padding="do_not_pad", add_special_tokens=False)["input_ids"] + [tokenizer.sep_token_id] for a in texts]


def get_trie(tokenizer, texts=None, fname="./aux_data/imagenet/imagenet_unique_readable_names.txt"):
    """trie_decoder.py:6-16: the trie over the allowed output texts (default: the ImageNet names file of the reference)."""
    if texts is None:
        with open(fname, "r") as fp:
            texts = list(fp)
    return TokenTrie.construct(get_output_vocab_tokens(tokenizer, texts))


class TrieAutoRegressiveBeamSearch:
    """Constructor-compatible with the reference class (trie_decoder.py:27-39): greedy decoding (beam_size == 1) restricted
    to the token sequences of `trie`.  Every sentence of a batch walks its own trie cursor, i.e. gets what its own batch-1
    reference call returns (the reference's single cursor follows row 0)."""

    def __init__(self, eos_index: int, max_steps: int = 50, beam_size: int = 5, trie=None) -> None:
        self._eos_index = eos_index
        self.max_steps = max_steps
        assert beam_size == 1                                       # trie_decoder.py:37
        self.beam_size = beam_size
        self.per_node_beam_size = 1
        self.trie = trie
        self.kind = "trie"
        self.length_penalty = 1.0

    def search(self, start_predictions: torch.Tensor, step, only_return_best: bool = True, do_sample: bool = False,
               top_k: int = 0, top_p=None, num_return_sequences: int = 1, temperature: float = 1, _engine_factory=None):
        """trie_decoder.py:41-218 with a caller-supplied `step`: -> (predictions [B, length <= max_steps] incl. the start
        tokens, logprobs [B]); ([B, 1], [B, 1]) when every first prediction is EOS."""
        if do_sample or not only_return_best or num_return_sequences != 1 or temperature != 1:
            raise NotImplementedError("TrieAutoRegressiveBeamSearch.search: only the inference form is implemented")
        s = Engine.make_search("trie", self.max_steps, 1, 1)
        return _begin_and_run(self, start_predictions, step, s, first_step_rows_per_sentence=True, stop_when_all_eos=True,
                              fmt="autoregressive", engine_factory=_engine_factory)


class GeneratorWithBeamSearch:
    """Constructor-compatible with the reference class (decoder.py:1057-1081)."""

    def __init__(self, eos_index: int, max_steps: int, beam_size: int, per_node_beam_size: int = 2,
                 length_penalty: float = 1, repetition_penalty: float = 1, temperature: float = 1) -> None:
        self._eos_index = eos_index
        self.max_steps = max_steps
        self.beam_size = beam_size
        self.per_node_beam_size = per_node_beam_size or beam_size
        self.length_penalty = length_penalty
        assert self.per_node_beam_size > 1
        assert self.length_penalty > 0, "`length_penalty` should be strictely positive."
        assert repetition_penalty >= 1.0, "`repetition_penalty` should be >= 1."        # decoder.py:1080
        self.repetition_penalty = repetition_penalty
        assert temperature > 0, "`temperature` should be strictely positive."        # decoder.py:1081
        self.temperature = temperature
        self.kind = "generator"

    def search(self, input_ids: torch.Tensor, step, num_keep_best: int = 1, do_sample: bool = False, top_k=None,
               top_p=None, num_return_sequences: int = 1, seed: int = 0, _engine_factory=None):
        """decoder.py:1083-1290 with a caller-supplied `step`: -> (decoded int64 [B, max_steps] = best hypothesis + EOS,
        right-padded with EOS, logprobs fp32 [B, 1]); with num_keep_best = n > 1 the n best hypotheses of every sentence,
        best first: ([B, n, max_steps], [B, n]), missing ones all EOS at -1e5 (decoder.py:1262-1290); B counts every
        sentence num_return_sequences times (decoder.py:1093-1097).  Like the reference, the loop stops calling `step` once
        every sentence is done (decoder.py:1251)."""
        if num_return_sequences != 1:                   # decoder.py:1093-1097: every sentence num_return_sequences times
            input_ids = input_ids[:, None, :].expand(input_ids.shape[0], num_return_sequences, input_ids.shape[1])
            input_ids = input_ids.reshape(-1, input_ids.shape[-1])
        s = Engine.make_search("generator", self.max_steps, self.beam_size, self.per_node_beam_size, self.length_penalty,
                               do_sample=do_sample, top_k=top_k or 0, top_p=top_p, temperature=self.temperature, seed=seed,
                               repetition_penalty=self.repetition_penalty, num_keep_best=num_keep_best)
        return _begin_and_run(self, input_ids, step, s, first_step_rows_per_sentence=False, stop_when_all_eos=False,
                              fmt="generator", engine_factory=_engine_factory)


def load_state_dict_by_suffix(model_keys: Sequence[str], loaded: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Key alignment of torch_common.py:45-54, 93-145: strip EVERY leading 'module.' (DataParallel wrapped any number
    of times), then give every model key the loaded key that is its LONGEST (purely textual) suffix; model keys that
    nothing matches are left out.  Pinned against the reference's align_and_update_state_dicts by
    tests/golden/state_dict_align.json (oracle/make_host_golden.py)."""
    stripped = {}
    for k, v in loaded.items():
        while k.startswith("module."):
            k = k[len("module."):]
        stripped[k] = v
    out: Dict[str, torch.Tensor] = {}
    for key in model_keys:
        best = None
        for cand in stripped:
            if key.endswith(cand) and (best is None or len(cand) > len(best)):
                best = cand
        if best is not None:
            out[key] = stripped[best]
    return out


def expected_state_dict_keys(cfg: GitModelConfig, tied_output: bool = False) -> Sequence[str]:
    """Keys the engine ingests."""
    keys = ["image_encoder.class_embedding", "image_encoder.positional_embedding", "image_encoder.conv1.weight",
            "image_encoder.ln_pre.weight", "image_encoder.ln_pre.bias", "image_encoder.ln_post.weight",
            "image_encoder.ln_post.bias"]
    for i in range(cfg.vit_layers):
        p = f"image_encoder.transformer.resblocks.{i}."
        keys += [p + s for s in ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                                 "attn.out_proj.bias", "ln_1.weight", "ln_1.bias", "mlp.c_fc.weight",
                                 "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias")]
    keys += ["textual.visual_projection.0.weight", "textual.visual_projection.0.bias",
             "textual.visual_projection.1.weight", "textual.visual_projection.1.bias",
             "textual.embedding.words.weight", "textual.embedding.positions.weight",
             "textual.embedding.layer_norm.weight", "textual.embedding.layer_norm.bias"]
    for i in range(cfg.dec_layers):
        p = f"textual.transformer.encoder.layer.{i}."
        for nm in ("query", "key", "value"):
            keys += [p + f"attention.self.{nm}.weight", p + f"attention.self.{nm}.bias"]
        keys += [p + s for s in ("attention.output.dense.weight", "attention.output.dense.bias",
                                 "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias",
                                 "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight",
                                 "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias")]
    if not tied_output:
        keys.append("textual.output.weight")
    keys.append("textual.output.bias")
    keys += [f"img_temperal_embedding.{i}" for i in range(cfg.num_frames)]
    return keys


def caption_loss(lp, mean_lp, tokens, need_predict, loss_type: Optional[str] = "smooth", eps: float = 0.1,
                 vocab: int = 30522, padding_idx: int = 0) -> float:
    """The reference's caption loss (CaptioningModel.forward_one_ce, decoder.py:938-966) from per-position scores, in fp64.

    lp, mean_lp: [Q, L] as Engine.score returns them (position j = the prediction of tokens[:, j]); tokens, need_predict
    [Q, L].  The positions counted are j >= 1 with need_predict[:, j] == 1 and tokens[:, j] != padding_idx (the reference
    sets the target of need_predict == 0 to padding_idx and both losses ignore it).
      loss_type None    : nn.CrossEntropyLoss (decoder.py:814-815): mean of -lp (nan when nothing is counted, as torch)
      loss_type 'smooth': SmoothLabelCrossEntropyLoss(eps) (decoder.py:620-671): mean over the positions of
                          KL(one-hot smoothed to eps / (V - 1) || softmax) =
                          (1-eps) log(1-eps) + eps log(eps/(V-1)) - [(1-eps) lp + eps/(V-1) (V mean_lp - lp)]
                          (asserts that something is counted, like the reference)."""
    lp = torch.as_tensor(lp).detach().double().cpu()
    mean_lp = torch.as_tensor(mean_lp).detach().double().cpu()
    tokens = torch.as_tensor(tokens).cpu()
    need_predict = torch.as_tensor(need_predict).cpu()
    sel = (need_predict[:, 1:] == 1) & (tokens[:, 1:] != padding_idx)
    a = lp[:, 1:][sel]
    if loss_type is None:
        return float((-a).mean()) if a.numel() else float("nan")
    if loss_type != "smooth":
        raise NotImplementedError(loss_type)
    assert a.numel() > 0, "no position to predict (SmoothLabelCrossEntropyLoss asserts target.numel() > 0)"
    m = mean_lp[:, 1:][sel]
    V = float(vocab)
    off = eps / (V - 1.0)
    const = (1.0 - eps) * math.log(1.0 - eps) + eps * math.log(off)
    per = const - ((1.0 - eps) * a + off * (V * m - a))
    return float(per.mean())


def format_predictions(tokens, logprobs, sent, prefix, kind: str):
    """What the caller of a search gets from its raw output (tokens incl. the start tokens, logprobs): the early-EOS rule
    of the autoregressive searches (decoder.py:279-291 / trie_decoder.py:76-83), then the prefix removed (decoder.py:1004-1006,
    along dim 1 whatever it is).  Pure: launches no device work.
      prefix None or an int P (one prefix for the whole batch; None: [CLS] alone, nothing removed): sent = (seq_len, early) of
        the call (info[:2]) -> (predictions tensor, logprobs [B] / [B, 1] / [B, num_keep_best]) as model(batch) returns them;
      prefix a list of per-sentence lengths: sent [Q, 2] = (length, early) of every sentence -> ([ids of each sentence],
        logprobs [Q, 1] / [Q, num_keep_best])."""
    autoregressive = kind in ("autoregressive", "trie")
    if isinstance(prefix, (list, tuple)):
        preds = []
        for q, P in enumerate(prefix):
            L, early = int(sent[q][0]), int(sent[q][1])
            row = tokens[q]
            if autoregressive:
                row = row[P:P + 1] if early else row[:L]
            preds.append(row[P:].tolist())
        return preds, logprobs.reshape(len(prefix), -1)
    P = 1 if prefix is None else int(prefix)
    seq_len, early = int(sent[0]), int(sent[1])
    if autoregressive:
        if early:
            tokens, logprobs = tokens[:, P:P + 1], logprobs[:, None]
        else:
            tokens = tokens[:, :seq_len]
    elif logprobs.dim() == 1:
        logprobs = logprobs[:, None]                                    # [B, num_keep_best]
    return (tokens if prefix is None else tokens[:, P:]), logprobs


def _finish_batch(eng, out, prefix, kind: str):
    """Pending.finish of a batch-uniform request (model(batch), captioning ragged batches); a traced request's `out` carries
    Engine.trace's buffers as a fourth entry."""
    tokens, logprobs, info = out[:3]
    info_h = info.tolist()                                              # ONE small read-back for the four fields
    eng.check_finite(info_h)
    predictions, logprobs = format_predictions(tokens, logprobs, info_h[:2], prefix, kind)
    res = {"predictions": predictions, "logprobs": logprobs}
    if len(out) > 3:
        nout = 1 if tokens.dim() == 2 else int(tokens.shape[1])
        res.update(format_trace(out[3], trace_spans(int(tokens.shape[0]), nout, int(tokens.shape[-1]), info_h[:2], prefix, kind)))
    return res


def _is_image_list(images) -> bool:
    """A list of [3, h, w] images of their own sizes (one ragged engine call); a list of [B, 3, H, W] tensors means frames."""
    return isinstance(images, (list, tuple)) and len(images) > 0 and \
        all(isinstance(t, torch.Tensor) and t.dim() == 3 for t in images)


class AttentionMaps:
    """What CaptioningModel.attend returns, fp32 on the CPU.
      image [Q, L, layers, Nk]: the attention of text row (q, j) of every decoder layer to the Nk image key rows of its image,
                                head mean; frame-major, the class token first within each frame (ragged input: the image's own
                                tokens, then zeros up to the capacity);
      text  [Q, L, layers, L] : the same row's attention to the text positions (0 past j).
    image and text of a row j < lengths[q] sum to 1 together; rows past a caption's length are 0."""

    def __init__(self, att: torch.Tensor, Nk: int, lengths: Sequence[int], image_of: Sequence[int], F: int,
                 grids: Sequence[Tuple[int, int]]):
        self.image, self.text = att[..., :Nk], att[..., Nk:]
        self.lengths, self.image_of, self.frames, self.grids = list(lengths), list(image_of), int(F), list(grids)

    def patch_grid(self, q: int) -> torch.Tensor:
        """[L_q, layers, F, H/p, W/p]: the image columns of caption q's own rows laid out on the patch grid of its image,
        class columns dropped (ragged input: that image's own grid)."""
        grid = self.grids[self.image_of[q]]
        if grid is None:
            raise ValueError(f"image {self.image_of[q]} has no patch grid: its features came without a shape (installed feature "
                             f"rows of another count than the current image shape's, or a recall without geometry)")
        gh, gw = grid
        n = gh * gw + 1
        rows = self.image[q, :self.lengths[q], :, :self.frames * n]
        Lq, layers = rows.shape[:2]
        return rows.reshape(Lq, layers, self.frames, n)[..., 1:].reshape(Lq, layers, self.frames, gh, gw)


class CaptioningModel:
    """Callable like the reference model: ``model(batch) -> {'predictions', 'logprobs'}``.

    batch['image']  : FloatTensor [B,3,H,W] or a list of such (video frames)   (decoder.py:845-857)
    batch['prefix'] : LongTensor [1,P] starting with [CLS] (VQA question)       (decoder.py:984-989)

    A batch WITHOUT 'image' (the reference requires the key) is a follow-up request over the images the engine context
    still holds from its last call -- no image encoder, no prefill: {'prefix' [1,P] or 'prefixes' [id lists], 'image_of' [Q]};
    see submit_followup.
    """

    # precision: "f32" (reference-identical ids), "f16" (default 16-bit mode: fp16 operands, same MFMA rate as bf16 on gfx950,
    # 8 x smaller logit error: the build that meets the specification and the benchmarked one since round 6) or "bf16" (BASELINE.json's named precision)
    def __init__(self, cfg: GitModelConfig, decoder, precision: str = "f16", max_batch: int = 64,
                 max_frames: Optional[int] = None, max_text_len: Optional[int] = None,
                 device: Optional[int] = None, max_context: int = 0, context_not_share_embedding: bool = False):
        """max_context: the most context tokens (batch['context'], all segments of one image together) a request may carry;
        the engine's per-image rows are sized for max_frames frames plus that many.  0 (default): today's footprint, and any
        non-empty context raises ValueError naming this argument."""
        if context_not_share_embedding:
            raise NotImplementedError("context_not_share_embedding=True: the reference cannot construct this model either "
                                      "(decoder.py:825 calls .clone() on an nn.Module); only the shared textual embedding exists")
        self.cfg = cfg
        self.decoder = decoder
        self.sos_index = cfg.sos
        self.eos_index = cfg.eos
        if max_frames is None:
            max_frames = max(1, cfg.num_frames)
        if max_text_len is None:
            max_text_len = min(cfg.max_pos, max(int(decoder.max_steps), 2))
        self.engine = Engine(cfg, precision=precision, max_batch=max_batch,
                             max_beams=max(1, int(decoder.beam_size)), max_frames=max_frames,
                             max_text_len=max_text_len, device=device, max_context=max_context)
        self._loaded = False
        # loss of the training-mode forward (model.py:55 builds the reference with loss_type='smooth'; None = cross entropy)
        self.loss_type: Optional[str] = "smooth"
        self.label_smoothing = 0.1
        # training: model(batch) returns the caption loss {'vl_l_loss'} (decoder.py:938-966) instead of searching
        self.training = False

    # nn.Module look-alikes so that reference call sites (`model.cuda(); model.eval()`) keep working
    def cuda(self, *a, **k):
        return self

    def eval(self):
        return self.train(False)

    def train(self, mode: bool = True):
        """training = True: model(batch) evaluates the caption loss of batch['caption_tokens'] (decoder.py:938-966).  There is
        no dropout and no backward pass: the value is the reference's with dropout inactive (CaptioningModel.training set,
        its submodules in eval mode); the reference in .train() applies dropout 0.1 (decoder.py:198-199) and is stochastic."""
        self.training = bool(mode)
        return self

    def load_state_dict(self, state_dict: Mapping[str, torch.Tensor], strict: bool = False):
        tied = not any(k.endswith("textual.output.weight") for k in state_dict)   # keys may carry 'module.' prefixes
        keys = expected_state_dict_keys(self.cfg, tied_output=tied)
        aligned = load_state_dict_by_suffix(keys, state_dict)
        missing = [k for k in keys if k not in aligned]
        if missing:
            raise KeyError(f"checkpoint is missing {len(missing)} tensors, e.g. {missing[:4]}")
        self.engine.load_state_dict(aligned)
        self._loaded = True
        return self

    def _search_struct(self, search_param: Optional[dict] = None):
        """search_param: the keyword arguments CaptioningModel.infer forwards to decoder.search (decoder.py:1001-1003):
        do_sample / top_k / top_p for GeneratorWithBeamSearch (decoder.py:1088-1090); `seed` selects the random stream.  The
        per-sentence decoding constraints (min_new_tokens, no_repeat_ngram_size, bad_tokens, allowed_tokens, bad_words) are not
        part of the struct: _constraints turns them into the tables the front end arms before the call."""
        d = self.decoder
        sp = dict(search_param or {})
        unknown = set(sp) - {"do_sample", "top_k", "top_p", "seed", "num_keep_best", "num_return_sequences"} - set(CONSTRAINT_PARAMS) \
            - set(TRACE_PARAMS)
        if unknown:
            raise NotImplementedError(f"search parameters {sorted(unknown)} are not implemented")
        if d.kind != "generator" and (int(sp.get("num_keep_best", 1)) != 1 or int(sp.get("num_return_sequences", 1)) != 1):
            raise NotImplementedError("num_keep_best / num_return_sequences: GeneratorWithBeamSearch.search only "
                                      "(the other classes use them in SCST training only)")
        return Engine.make_search(d.kind, d.max_steps, d.beam_size, d.per_node_beam_size, d.length_penalty,
                                  do_sample=bool(sp.get("do_sample", False)), top_k=sp.get("top_k") or 0,
                                  top_p=sp.get("top_p"), temperature=getattr(d, "temperature", 1.0),
                                  seed=int(sp.get("seed", 0)),
                                  repetition_penalty=getattr(d, "repetition_penalty", 1.0),
                                  num_keep_best=int(sp.get("num_keep_best", 1)))

    def _constraints(self, search_param: Optional[dict], n: int, repeat: int = 1):
        """The decoding constraints of a request of `n` sentences (include/gitmi.h GITMI_SEARCH_CONSTRAIN) from its search_param:
        min_new_tokens, no_repeat_ngram_size, bad_tokens, allowed_tokens -- each one value for all sentences or one per sentence
        (engine.constraint_tables) -- and bad_words, words that are one WordPiece each (one list for all, or one per sentence),
        banned like bad_tokens.  bad_sequences (id sequences) and bad_phrases (strings of any number of WordPieces, through the
        tokenizer) ban token sequences: one list for all sentences or one per sentence (engine.banned_sequence_tables); their
        one-token entries join the sentence's bad tokens.  repeat: every sentence stands for `repeat` consecutive ones
        (num_return_sequences).
        -> (words, table) for Engine.constrain -- (words, table, pool) when some sentence bans a sequence of two or more tokens --
        or None: the request is not constrained and nothing is armed."""
        sp = {k: v for k, v in (search_param or {}).items() if k in CONSTRAINT_PARAMS and v is not None}
        if not sp:
            return None
        if self.decoder.kind == "trie":
            raise NotImplementedError("decoding constraints on the trie search are not implemented")
        bad = sp.get("bad_tokens")
        pool = None
        if "bad_sequences" in sp or "bad_phrases" in sp:
            singles, pool = banned_sequence_tables(n, int(self.cfg.vocab), self._sequences(sp, n))
            if any(one is not None for one in singles):
                bad = self._merge_ids("bad_tokens", bad, singles, n)
        if "bad_words" in sp:
            words = sp["bad_words"]
            flat = all(isinstance(w, str) for w in words)
            ids = [self._word_ids(words)] * n if flat else [None if ws is None else self._word_ids(ws) for ws in words]
            if len(ids) != n:
                raise ValueError(f"bad_words has {len(ids)} entries for {n} sentences (one list for all, or one per sentence)")
            bad = ids if bad is None else self._merge_ids("bad_tokens", bad, ids, n)
        out = constraint_tables(n, int(self.cfg.vocab), int(self.cfg.eos), sp.get("min_new_tokens", 0), sp.get("no_repeat_ngram_size", 0),
                                bad, sp.get("allowed_tokens"), max_new=int(self.engine.c.max_text_len))
        if pool is None:
            if out is None or repeat == 1:
                return out
            return out[0], [row for row in out[1] for _ in range(repeat)]
        import numpy as np
        if out is None:             # sequences alone: no set, no length rule, no n-gram rule
            out = np.zeros((0, (int(self.cfg.vocab) + 31) // 32), dtype=np.uint32), [[-1, 0, 0] for _ in range(n)]
        if repeat != 1:             # list_of is the pool's only per-sentence array
            pool = np.concatenate([pool[:4], np.repeat(pool[4:4 + n], repeat), pool[4 + n:]]).astype(np.int32)
        return out[0], [row for row in out[1] for _ in range(repeat)], pool

    @staticmethod
    def _merge_ids(name: str, given, more, n: int):
        """given: a search_param id list for all sentences or one (or None) per sentence; more: n entries, None or ids -> n entries"""
        flat_ids = all(isinstance(t, int) and not isinstance(t, bool) for t in given or [])       # one id list for every sentence
        per = [None if given is None else list(given)] * n if flat_ids else list(given)
        if len(per) != n:
            raise ValueError(f"{name} has {len(per)} entries for {n} sentences (one value for all, or one per sentence)")
        return [None if a is None and b is None else list(a or []) + list(b or []) for a, b in zip(more, per)]

    def _sequences(self, sp: dict, n: int):
        """bad_sequences and bad_phrases of a request -> one entry per sentence: None or its list of id sequences"""
        def per_sentence(name, value, is_leaf):
            if not isinstance(value, (list, tuple)):
                raise ValueError(f"{name} must be a list (one for all sentences, or one list or None per sentence)")
            if all(is_leaf(v) for v in value):
                return [list(value)] * n
            if len(value) != n:
                raise ValueError(f"{name} has {len(value)} entries for {n} sentences (one list for all, or one per sentence)")
            return list(value)

        import numpy as np
        is_int = lambda t: isinstance(t, (int, np.integer)) and not isinstance(t, bool)
        is_ids = lambda v: isinstance(v, (list, tuple)) and len(v) > 0 and all(is_int(t) for t in v)
        per = [None] * n
        if sp.get("bad_sequences") is not None:
            per = per_sentence("bad_sequences", sp["bad_sequences"], is_ids)
        if sp.get("bad_phrases") is not None:
            tok = getattr(self, "tokenizer", None)
            if tok is None:
                raise ValueError("bad_phrases needs the model's tokenizer (get_git_model keeps it; or set model.tokenizer)")
            phrases = per_sentence("bad_phrases", sp["bad_phrases"], lambda v: isinstance(v, str))
            for q, lst in enumerate(phrases):
                if lst is None:
                    continue
                seqs = []
                for ph in lst:
                    if not isinstance(ph, str):
                        raise ValueError(f"sentence {q}: bad_phrases holds {ph!r}, not a string")
                    ids = [int(t) for t in tok(ph, add_special_tokens=False)["input_ids"]]
                    if not ids:
                        raise ValueError(f"sentence {q}: bad_phrases: {ph!r} has no WordPiece")
                    seqs.append(ids)
                per[q] = seqs if per[q] is None else list(per[q]) + seqs
        return per

    def _word_ids(self, words) -> List[int]:
        tok = getattr(self, "tokenizer", None)
        if tok is None:
            raise ValueError("bad_words needs the model's tokenizer (get_git_model keeps it; or set model.tokenizer)")
        ids = []
        for w in words:
            pieces = tok(w, add_special_tokens=False)["input_ids"]
            if len(pieces) != 1:
                raise ValueError(f"bad_words: {w!r} is {len(pieces)} WordPieces; only words that are one WordPiece can be banned "
                                 f"(multi-token banned sequences are not implemented for bad_words: use bad_phrases)")
            ids.append(int(pieces[0]))
        return ids

    def close(self) -> None:
        """Free the engine contexts (workspaces, KV caches, packed weights) now rather than at garbage collection."""
        for c in (getattr(self, "_ctxs", None) or [])[1:]:
            c.close()
        self._ctxs = None
        self.engine.close()
        self._loaded = False

    # ---- several requests in flight (serving / the TSV task) -----------------------------------------------------------------
    def set_pipeline(self, contexts: int = 4, encoder_chains: int = 2) -> None:
        """Keep up to `contexts` requests in flight: context i (a clone that borrows the packed weights, gitmi_clone) runs on a
        HIP stream of its own, so the latency-bound decode steps of one request overlap the MFMA-bound image encoder of the
        next; at most `encoder_chains` encoders run at a time (gitmi_set_encode_after) -- the schedule bench.py measures.
        submit() then rotates over the contexts; model(batch) keeps using context 0 synchronously."""
        if not self._loaded:
            raise RuntimeError("weights not loaded (call load_state_dict first)")
        contexts = max(1, int(contexts))
        if getattr(self, "_ctxs", None) and len(self._ctxs) == contexts:
            return
        for c in getattr(self, "_ctxs", [])[1:]:
            c.close()
        if contexts > 1:
            self.engine.set_shared_device(True)          # kernel shapes by whole-device cost (bit-identical results)
        self._ctxs = [self.engine] + [self.engine.clone() for _ in range(contexts - 1)]
        self._streams = [torch.cuda.Stream() for _ in self._ctxs]
        chains = max(1, int(encoder_chains))
        if len(self._ctxs) > chains:
            for i, c in enumerate(self._ctxs):
                c.set_encode_after(self._ctxs[i - chains])
        self._next = 0

    def _context(self):
        """-> (engine context, its stream or None) of the next submission"""
        if not getattr(self, "_ctxs", None):
            self._last = self.engine
            return self.engine, None
        i = self._next % len(self._ctxs)
        self._next += 1
        self._last = self._ctxs[i]
        return self._ctxs[i], self._streams[i]

    def _followup_context(self, on=None):
        """-> (engine context, its stream or None) of a follow-up request: the context that ran `on` (a Pending, or the result
        it returned), else the context of the most recent call.  Raises when that context's images are no longer the ones
        `on` was issued for: a follow-up must never answer about other images."""
        on = getattr(on, "pending", on)
        if on is not None and not isinstance(on, Pending):
            raise TypeError("on= takes the Pending of the call that encoded the images, or the result it returned")
        eng = on.engine if on is not None else getattr(self, "_last", None) or self.engine
        if on is not None and eng.generation != on.generation:
            raise StaleImagesError("the images of this handle are no longer resident on its context: another call has "
                                   "replaced them (or a setter dropped them) since it was issued")
        if eng.resident is None:
            raise StaleImagesError("no resident images on this context: run a call with images first")
        ctxs = getattr(self, "_ctxs", None)
        if ctxs:        # every context of a pipeline owns a stream: the follow-up is ordered behind the context's own work
            for c, st in zip(ctxs, self._streams):
                if c is eng:
                    return eng, st
        return eng, None

    def _prepare(self, eng, frames_is_list: Optional[bool]):
        """frames_is_list None: a follow-up request (the temporal-embedding switch stays: flipping it drops the images)"""
        if frames_is_list is not None:
            eng.set_temporal_embedding(frames_is_list)                      # decoder.py:845-857: list branch only
        if self.decoder.kind == "trie" and getattr(eng, "_trie_loaded", None) is not self.decoder.trie:
            eng.set_trie(*self.decoder.trie.csr())
            eng._trie_loaded = self.decoder.trie

    def _context_segments(self, eng, frames, context):
        """batch['context'] of a call over `frames` -> (segments, image_of) for Engine.encode_context, or None when no image has
        a non-empty segment (a plain call).  Checks the ids, the lengths and the engine's per-image row capacity on the host."""
        if not context:
            return None
        B, _, H, W = frames[0].shape
        segments, image_of = context_segments(context, int(B), int(self.cfg.vocab), int(self.cfg.max_pos))
        if not segments:
            return None
        if self.cfg.vit_width != self.cfg.dec_hidden:
            raise ValueError(f"'context' needs visual_feature_size == hidden_size (the reference concatenates the embedded tokens "
                             f"to the visual features, decoder.py:866); this model has {self.cfg.vit_width} and {self.cfg.dec_hidden}")
        counts = [0] * int(B)
        for ids, b in zip(segments, image_of):
            counts[b] += len(ids)
        F_eff = min(len(frames), self.cfg.num_frames) if self.cfg.num_frames > 0 else len(frames)
        rows = F_eff * ((int(H) // eng.c.patch) * (int(W) // eng.c.patch) + 1)
        cap = int(eng.c.max_frames) * eng.max_tokens
        if rows + max(counts) > cap:
            raise ValueError(f"{max(counts)} context tokens behind {rows} image rows exceed the {cap} rows per image of this model: "
                             f"construct CaptioningModel(..., max_context={max(counts)}) (workspaces are sized at construction; "
                             f"now max_context={eng.max_context})")
        return segments, image_of

    def submit(self, batch: Mapping[str, Union[torch.Tensor, Sequence[torch.Tensor]]],
               search_param: Optional[dict] = None, on=None) -> "Pending":
        """Asynchronous model(batch): enqueue the request on the next context's stream and return at once; `.result()` waits
        for it and returns what model(batch) returns.  The batch's tensors must have been produced on the CURRENT stream (the
        context's stream waits for it).  A batch without 'image' is a follow-up request (submit_followup; `on` names the call
        whose images it is about)."""
        if not self._loaded:
            raise RuntimeError("weights not loaded (call load_state_dict first)")
        if "image" not in batch:
            return self.submit_followup(batch, search_param, on=on)
        if on is not None:
            raise ValueError("on= belongs to follow-up requests (a batch without 'image')")
        if batch.get("bi_valid_mask_caption") is not None:
            raise NotImplementedError("'bi_valid_mask_caption' (image rows attending to the text, decoder.py:139-146) is not implemented")
        image = batch["image"]
        is_list = isinstance(image, (list, tuple))
        frames = list(image) if is_list else [image]
        eng, stream = self._context()
        if self.cfg.num_frames == 0 and len(frames) > eng.c.max_frames:
            # the reference concatenates the features of every frame of a list, also on an image model
            raise ValueError(f"{len(frames)} frames on an image model: construct CaptioningModel(..., max_frames="
                             f"{len(frames)}) (workspaces are sized at construction; now max_frames={eng.c.max_frames})")
        self._prepare(eng, is_list)
        prefix = batch.get("prefix")
        if prefix is not None:
            assert len(prefix) == 1, "not supported"                       # decoder.py:988
        # batch['context'] (decoder.py:861-871): the context call encodes images + context, the search is a follow-up over them
        ctx = self._context_segments(eng, frames, batch.get("context"))
        search = self._search_struct(search_param)
        P = None if prefix is None else int(prefix.numel())
        nret = int((search_param or {}).get("num_return_sequences", 1))
        kind = self.decoder.kind
        ban = self._constraints(search_param, int(frames[0].shape[0]), repeat=nret)
        trace_n = trace_param(search_param, kind)

        def launch():
            frames_arg = frames
            if ctx is not None:
                eng.encode_context(frames, ctx[0], image_of=ctx[1])
                frames_arg = None
            if ban is not None:         # armed on this context and stream, immediately before the call that consumes it
                _arm(eng, ban)
            trace = _arm_trace(eng, trace_n, int(frames[0].shape[0]) * nret, search, stream is not None)
            if nret != 1:
                # decoder.py:1093-1097: every image's start tokens num_return_sequences times -- r sentences per image, each
                # with its own beams (they differ only when sampling); rows b * r + j, as the reference returns them
                B = int(frames[0].shape[0])
                start = [int(self.cfg.sos)] if prefix is None else [int(t) for t in prefix.reshape(-1).tolist()]
                if B * nret > eng.c.max_batch:
                    raise ValueError(f"{B} images x num_return_sequences={nret} exceed max_batch={eng.c.max_batch}")
                tokens, logprobs, _, info = eng.generate_prefixed(
                    frames_arg, search, [start] * (B * nret), image_of=[b for b in range(B) for _ in range(nret)], sync=False,
                    host_out=stream is not None)
            else:
                # requests in flight on other streams: results straight into page-locked host memory (no read-back to enqueue)
                tokens, logprobs, info = eng.generate(frames_arg, search, prefix=prefix, sync=False, host_out=stream is not None)
            return (tokens, logprobs, info) if trace is None else (tokens, logprobs, info, trace)

        return Pending(stream, launch, lambda out: _finish_batch(eng, out, P, kind), keep=(frames, prefix), engine=eng)

    def submit_followup(self, batch: Mapping, search_param: Optional[dict] = None, on=None) -> "Pending":
        """A request over RESIDENT images: the ones the context of `on` (default: of the most recent call) encoded in its
        last call.  Only the decode steps run.  batch: {'prefix': [1, P] (one question for every sentence) or 'prefixes': [id
        lists starting with [CLS]], 'image_of': [Q] image index of every sentence}; search_param as for submit (the search
        may differ from the first call's: a beam pass after a greedy one, sampling, num_keep_best).
        `.result()`: {'predictions': [ids of each sentence, the prefix removed], 'logprobs': fp32 [Q, 1 or num_keep_best]}."""
        if not self._loaded:
            raise RuntimeError("weights not loaded (call load_state_dict first)")
        if "image_of" not in batch or ("prefix" not in batch and "prefixes" not in batch):
            raise ValueError("a batch without 'image' is a follow-up request: it needs 'image_of' and 'prefix' or 'prefixes'")
        image_of = [int(i) for i in batch["image_of"]]
        if "prefixes" in batch:
            prefixes = [[int(t) for t in p] for p in batch["prefixes"]]
        else:
            prefix = torch.as_tensor(batch["prefix"])
            assert len(prefix) == 1, "not supported"                       # decoder.py:988
            prefixes = [[int(t) for t in prefix.reshape(-1).tolist()]] * len(image_of)
        if int((search_param or {}).get("num_return_sequences", 1)) != 1:
            raise NotImplementedError("num_return_sequences in a follow-up request: repeat the sentence in 'image_of'")
        eng, stream = self._followup_context(on)
        return self._submit_prefixed(eng, stream, None, prefixes, image_of, self._search_struct(search_param), as_dict=True,
                                     ban=self._constraints(search_param, len(prefixes)),
                                     trace_n=trace_param(search_param, self.decoder.kind))

    def forward(self, batch: Mapping[str, Union[torch.Tensor, Sequence[torch.Tensor]]],
                search_param: Optional[dict] = None, on=None) -> Dict[str, torch.Tensor]:
        if self.training:
            return self._loss_forward(batch)
        if "image" not in batch:
            return self.submit(batch, search_param, on=on).result()
        return self._on_context0(lambda: self.submit(batch, search_param))

    __call__ = forward

    def _loss_forward(self, batch) -> Dict[str, torch.Tensor]:
        """forward_one_ce with self.training (decoder.py:938-966): {'vl_<hint>_loss': loss} over batch['caption_tokens'] /
        batch['need_predict'] of the images in batch['image'] (a tensor or a list of frames) and, when given, the context tokens
        of batch['context']; hint = batch['context_target_type'][0], default 'l'."""
        if "image" not in batch:
            raise NotImplementedError("the text-only branch ('l_*_loss') is not implemented")
        if batch.get("bi_valid_mask_caption") is not None:
            raise NotImplementedError("'bi_valid_mask_caption' (image rows attending to the text, decoder.py:139-146) is not implemented")
        tokens = torch.as_tensor(batch["caption_tokens"]).cpu()
        need_predict = torch.as_tensor(batch["need_predict"]).cpu()
        out = self.score(batch["image"], tokens, need_predict=need_predict, context=batch.get("context"))
        loss = caption_loss(out["logprobs"], out["mean_logprobs"], tokens, need_predict, self.loss_type,
                            self.label_smoothing, self.cfg.vocab)
        hint = batch["context_target_type"][0] if "context_target_type" in batch else "l"        # decoder.py:963
        return {f"vl_{hint}_loss": torch.tensor(loss, dtype=torch.float32)}

    def score(self, images: Union[None, torch.Tensor, Sequence[torch.Tensor]], captions,
              image_of: Optional[Sequence[int]] = None, need_predict=None, on=None, context=None) -> Dict[str, torch.Tensor]:
        """Log-likelihood of given captions (validation loss / perplexity, reranking, retrieval, closed-set VQA).
        captions: int [Q, L] padded with 0 (or a list of id lists), each starting with [CLS]; caption q belongs to image
        image_of[q] of `images` (default: caption q <-> image q).  need_predict [Q, L] (default: the non-padding positions
        after [CLS]) selects the positions that count, e.g. 0 on a VQA question prefix.
        images None: the captions are scored over the RESIDENT images of `on`'s context (default: of the most recent call),
        e.g. the captions that call just generated; nothing is encoded (their context, if that call had one, is part of them).
        context: the reference's batch['context'] for `images` (a list of {'tokens' [B, Lc], 'length' [B]}): the captions are
        scored over [image | context].
        -> {'logprobs' [Q, L] (lp of tokens[:, j], 0 at position 0), 'mean_logprobs' [Q, L] (mean log-prob over the
            vocabulary at that position), 'sum' [Q], 'mean' [Q] (over the counted positions)}, all fp32 on the CPU."""
        if not isinstance(captions, torch.Tensor):
            captions = id_table(captions)
        tokens = captions.detach().cpu().long()
        out, _ = self._sentence_pass("score", images, tokens, image_of, on, context=context)
        lp, mean_lp = out[..., 0], out[..., 1]
        if need_predict is None:
            need_predict = (tokens != 0).long()
            need_predict[:, 0] = 0
        need_predict = torch.as_tensor(need_predict).cpu()
        sel = torch.zeros_like(tokens, dtype=torch.bool)
        sel[:, 1:] = (need_predict[:, 1:] == 1) & (tokens[:, 1:] != 0)
        total = torch.where(sel, lp, torch.zeros_like(lp)).sum(1)
        n = sel.sum(1)
        return {"logprobs": lp, "mean_logprobs": mean_lp, "sum": total,
                "mean": total / n.clamp(min=1).to(total.dtype)}

    def rank(self, images: Union[None, torch.Tensor, Sequence[torch.Tensor]], candidates, prefixes=None,
             image_of: Optional[Sequence[int]] = None, on=None, context=None, append_eos: bool = True) -> Dict[str, object]:
        """Exact log-probability of every candidate of a closed set (VQA answer list, class names, captions to rerank) in ONE
        engine call: the candidates are merged into a token trie and every trie node is scored once (Engine.score_tree), so
        a shared question prefix and shared answer prefixes pass through the decoder and the vocabulary head once, and the
        call is not chunked by max_batch x max_beams candidates.
        candidates: K id lists (without [CLS]); append_eos adds [SEP] to each, so that the probability of stopping counts, as in
        the reference's class tries (get_output_vocab_tokens).  prefixes: Q id lists, the question of tree q ([CLS] is put in
        front unless it is there already; default: none, one tree per image); tree q belongs to image image_of[q] (default:
        q <-> image q).  images, on and context as for score: images None ranks over the RESIDENT images.
        -> {'scores' fp32 [Q, K]: the sum of lp over candidate k's own nodes (the prefix does not count); 'best' int64 [Q]: its
            argmax, ties to the first candidate; 'node_logprobs' fp32 [Q, L, 2]: (lp, mean_lp) of every node; 'tree':
            {'tokens', 'depths' int64 [Q, L], 'lengths' [Q], 'terminal' int64 [Q, K] the node candidate k ends in}}, on the CPU."""
        eos = [int(self.cfg.eos)] if append_eos else []
        cands = [[int(t) for t in c] + eos for c in candidates]
        if not cands or any(not c for c in cands):
            raise ValueError("rank needs at least one candidate, each of at least one token")
        if prefixes is None:
            n = len(image_of) if image_of is not None else None if images is None else \
                len(images) if _is_image_list(images) else int((images[0] if isinstance(images, (list, tuple)) else images).shape[0])
            if n is None:
                raise ValueError("rank over resident images needs image_of (or prefixes)")
            prefixes = [[]] * n
        sos = int(self.cfg.sos)
        chains = [[int(t) for t in p] for p in prefixes]
        chains = [c if c[:1] == [sos] else [sos] + c for c in chains]
        trie_tok, trie_dep, terminal = TokenTrie.construct(cands).preorder()
        Q, L = len(chains), max(len(c) for c in chains) + len(trie_tok)
        tokens, depths = torch.zeros(Q, L, dtype=torch.int64), torch.zeros(Q, L, dtype=torch.int64)
        lengths = []
        for q, c in enumerate(chains):
            n = len(c) + len(trie_tok)
            tokens[q, :n] = torch.tensor(c + trie_tok)
            depths[q, :n] = torch.tensor(list(range(len(c))) + [len(c) - 1 + d for d in trie_dep])
            lengths.append(n)
        out, _ = self._sentence_pass("score_tree", images, tokens, image_of, on, context=context, depths=depths, lengths=lengths)
        out = out.float()
        # path sums below the chain, one trie level at a time: own[i] = own[parent(i)] + lp[i]; slot 0 is the chain's last node
        first = torch.tensor([len(c) for c in chains])
        own = torch.zeros(Q, len(trie_tok) + 1, dtype=torch.float32)
        own[:, 1:] = torch.gather(out[..., 0], 1, first[:, None] + torch.arange(len(trie_tok))[None, :])
        path, parent = [0], []                                                        # slot of the node at every trie depth
        for i, d in enumerate(trie_dep):
            del path[d:]
            parent.append(path[d - 1])
            path.append(i + 1)
        dep, parent = torch.tensor(trie_dep), torch.tensor(parent)
        for d in range(2, max(trie_dep) + 1):
            level = (dep == d).nonzero()[:, 0]
            own[:, level + 1] += own[:, parent[level]]
        scores = own[:, [t + 1 for t in terminal]]
        term = torch.tensor([[len(c) + t for t in terminal] for c in chains], dtype=torch.int64)
        return {"scores": scores, "best": torch.from_numpy(scores.numpy().argmax(1)), "node_logprobs": out,
                "tree": {"tokens": tokens, "depths": depths, "lengths": lengths, "terminal": term}}

    def _sentence_pass(self, method: str, images, tokens: torch.Tensor, image_of, on, context=None, **kw):
        """One engine pass over given sentences (Engine.score / Engine.attend) routed like every request: images None -> the
        follow-up context of `on` on its stream, a list of [3, h, w] images -> one ragged call, else frames; the calls that
        encode run on context 0.  -> (the result on the CPU, the engine context that ran it)"""
        if not self._loaded:
            raise RuntimeError("weights not loaded (call load_state_dict first)")
        is_list = isinstance(images, (list, tuple))
        if context and (images is None or _is_image_list(images)):
            raise NotImplementedError("context comes with the call that encodes its images, all of one shape")
        if images is None:
            eng, stream = self._followup_context(on)
            if stream is None:
                return getattr(eng, method)(None, tokens, image_of=image_of, **kw).cpu(), eng
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                return getattr(eng, method)(None, tokens, image_of=image_of, **kw).cpu(), eng
        eng = self.engine
        if _is_image_list(images):
            self._check_ragged()
            eng.set_temporal_embedding(False)
            frames = eng.ragged(images)
        else:
            frames = list(images) if is_list else [images]
            eng.set_temporal_embedding(is_list)                              # decoder.py:845-857: list branch only
            ctx = self._context_segments(eng, frames, context)
            if ctx is not None:          # the context call encodes images + context; the sentences run as a follow-up over them
                eng.encode_context(frames, ctx[0], image_of=ctx[1])
                frames = None
        out = getattr(eng, method)(frames, tokens, image_of=image_of, **kw).cpu()
        self._last = eng
        return out, eng

    def attend(self, images: Union[None, torch.Tensor, Sequence[torch.Tensor]], captions,
               image_of: Optional[Sequence[int]] = None, on=None) -> "AttentionMaps":
        """Where every token of given captions looked: the attention of the decoder's text rows to the image tokens and to
        their own text, per layer, averaged over the heads (the reference's BertSelfAttention.output_attentions).  captions,
        image_of, images and on as for score: images None runs over the RESIDENT images -- `generate`, then
        `attend(None, captions)` locates what the caption just generated was read from, with no re-encode.
        -> AttentionMaps: .image [Q, L, layers, Nk], .text [Q, L, layers, L], .patch_grid(q) [L_q, layers, F, H/p, W/p]."""
        if isinstance(captions, torch.Tensor):
            tokens = captions.detach().cpu().long()
            pos = torch.arange(1, tokens.shape[1] + 1)
            lengths = ((tokens != 0).long() * pos).amax(1).clamp(min=1).tolist()      # 0 pads: a caption ends at its last id
        else:
            lengths = [len(c) for c in captions]
            tokens = id_table(captions)
        out, eng = self._sentence_pass("attend", images, tokens, image_of, on, lengths=lengths)
        Nk, F, grids = eng.resident_geometry
        return AttentionMaps(out, Nk, lengths, list(range(len(lengths))) if image_of is None else [int(i) for i in image_of],
                             F, grids)

    # ---- features out and in: the encoder / head seam of the reference (image_encoder(x) -> visual_features -> textual) --------
    def features(self, images: torch.Tensor) -> torch.Tensor:
        """The visual features of `images` [B, 3, H, W]: fp32 [B, N, vit_width] on the device, what the reference's
        image_encoder(x) returns for a bare tensor (no temporal embedding: install_features / FeatureStore.recall add the one
        of a frame's position in its window).  Runs on context 0 and the caller's stream; the images are resident there
        afterwards, as after any encode."""
        if not self._loaded:
            raise RuntimeError("weights not loaded (call load_state_dict first)")
        if not isinstance(images, torch.Tensor) or images.dim() != 4:
            raise ValueError("features takes one [B, 3, H, W] tensor (the frames of a video: one call per frame, or stack them)")

        def run():
            self.engine.set_temporal_embedding(False)
            feats = self.engine.encode([images])
            self._last = self.engine
            return Pending(None, lambda: feats, lambda out: out, engine=self.engine)

        return self._on_context0(run)

    def submit_features(self, rows: torch.Tensor, pieces=None, image_of: Optional[Sequence[int]] = None, F: int = 1,
                        context=None) -> "Pending":
        """Make visual feature rows the resident images of an engine context (Engine.install_features: rows [R, D] with pieces, or
        [B, n, D]) -- `context`, default the next one in the model's rotation -- and return the handle follow-up requests take
        as on= (submit_followup, submit_answers(None, ...), score / rank / attend(None, ...)).
        `.result()`: {'stride', 'max_rows', 'total_rows'}."""
        if not self._loaded:
            raise RuntimeError("weights not loaded (call load_state_dict first)")
        if context is None:
            eng, _ = self._context()
        else:
            eng = context
            self._last = eng
        info = _on_context_stream(self, eng, lambda: eng.install_features(rows, pieces, image_of, F))
        return Pending(None, lambda: info, lambda out: dict(out), engine=eng)

    def _check_ragged(self) -> None:
        if not self._loaded:
            raise RuntimeError("weights not loaded (call load_state_dict first)")
        if self.cfg.num_frames != 0:
            raise ValueError("images of different sizes in one call: only models without temporal image embeddings "
                             "(num_image_with_embedding = 0) take a list of [3, h, w] images")

    def submit_ragged(self, images: Optional[Sequence[torch.Tensor]], prefixes: Optional[Sequence[Sequence[int]]] = None,
                      image_of: Optional[Sequence[int]] = None, search_param: Optional[dict] = None, on=None) -> "Pending":
        """Images of DIFFERENT sizes in one engine call (the aspect-preserving VQA models: MinMaxResizeForTest gives every
        image its own shape).  images: list of fp32 [3, h, w]; every image gets exactly what a call with that image alone
        gets.  prefixes None: captioning, `.result()` is submit({'image': image}).result()'s dict over the B images.
        prefixes given: question q (token ids starting with [CLS]) about image image_of[q] (default: q <-> image q);
        `.result()` is {'predictions': [ids of each answer, the prefix removed], 'logprobs': fp32 [Q, 1]}.
        images None: a follow-up request over the resident images (submit_followup)."""
        if images is None:
            if prefixes is None or image_of is None:
                raise ValueError("a follow-up request (images=None) needs prefixes and image_of")
            return self.submit_followup({"prefixes": prefixes, "image_of": image_of}, search_param, on=on)
        self._check_ragged()
        images = list(images)
        if not _is_image_list(images):
            raise ValueError("submit_ragged takes a non-empty list of [3, h, w] images")
        eng, stream = self._context()
        self._prepare(eng, False)
        packed = eng.ragged(images)                                        # host-side shape checks, then one upload
        search = self._search_struct(search_param)
        if int((search_param or {}).get("num_return_sequences", 1)) != 1:
            raise NotImplementedError("num_return_sequences with images of different sizes")
        ban = self._constraints(search_param, len(images) if prefixes is None else len(prefixes))
        trace_n = trace_param(search_param, self.decoder.kind)
        if prefixes is None:
            def launch():
                if ban is not None:
                    _arm(eng, ban)
                trace = _arm_trace(eng, trace_n, len(images), search, stream is not None)
                out = eng.generate(packed, search, sync=False, host_out=stream is not None)
                return out if trace is None else (*out, trace)

            return Pending(stream, launch,
                           lambda out: _finish_batch(eng, out, None, self.decoder.kind), keep=(packed,), engine=eng)
        Q = len(prefixes)
        image_of = list(range(Q)) if image_of is None else [int(i) for i in image_of]
        if Q > eng.c.max_batch:
            raise ValueError(f"{Q} questions exceed max_batch={eng.c.max_batch}")
        if len(image_of) != Q or any(i < 0 or i >= len(images) for i in image_of):
            raise ValueError(f"image_of must name one of the {len(images)} images for each of the {Q} questions")
        return self._submit_prefixed(eng, stream, packed, prefixes, image_of, search, as_dict=True, ban=ban, trace_n=trace_n)

    def generate_ragged(self, images: Sequence[torch.Tensor], prefixes: Optional[Sequence[Sequence[int]]] = None,
                        image_of: Optional[Sequence[int]] = None, search_param: Optional[dict] = None):
        """submit_ragged(...).result() on context 0 and the caller's stream."""
        return self._on_context0(lambda: self.submit_ragged(images, prefixes, image_of, search_param))

    def submit_answers(self, images: Union[None, torch.Tensor, Sequence[torch.Tensor]], prefixes: Sequence[Sequence[int]],
                       image_of: Optional[Sequence[int]] = None, on=None, search_param: Optional[dict] = None) -> "Pending":
        """Questions about SEVERAL images of one resolution in one engine call (batched ragged prefixes): `images` [B,3,H,W]
        (or a list of frames of that shape), question q = token ids starting with [CLS], about image image_of[q] (default: all
        about image 0).  `.result()` returns, per question, the list of predicted token ids exactly as
        ``model({'image': image, 'prefix': [prefix]})['predictions'][0]`` gives them for that image alone -- the reference loop
        of inference.py:172-199 without re-encoding an image per question and without one call per image.
        images None: further questions about the RESIDENT images of `on`'s context (default: of the most recent call).
        search_param: as for submit (sampling, decoding constraints per question)."""
        if not self._loaded:
            raise RuntimeError("weights not loaded (call load_state_dict first)")
        if images is None:
            image_of = [0] * len(prefixes) if image_of is None else [int(i) for i in image_of]
            eng, stream = self._followup_context(on)
            self._prepare(eng, None)
            return self._submit_prefixed(eng, stream, None, prefixes, image_of, self._search_struct(search_param), as_dict=False,
                                         ban=self._constraints(search_param, len(prefixes)),
                                         trace_n=trace_param(search_param, self.decoder.kind))
        is_list = isinstance(images, (list, tuple))
        frames = list(images) if is_list else [images]
        Q = len(prefixes)
        image_of = [0] * Q if image_of is None else [int(i) for i in image_of]
        eng, stream = self._context()
        if Q > eng.c.max_batch or int(frames[0].shape[0]) > eng.c.max_batch:
            raise ValueError(f"{Q} questions / {int(frames[0].shape[0])} images exceed max_batch={eng.c.max_batch}")
        self._prepare(eng, is_list)
        return self._submit_prefixed(eng, stream, frames, prefixes, image_of, self._search_struct(search_param), as_dict=False,
                                     ban=self._constraints(search_param, Q), trace_n=trace_param(search_param, self.decoder.kind))

    def _submit_prefixed(self, eng, stream, frames, prefixes, image_of, search, as_dict: bool, ban=None, trace_n=None) -> "Pending":
        """submit_answers / submit_ragged with questions: one generate_prefixed call on `eng` (frames: a stacked batch or
        RaggedImages).  .result(): the answers' id lists, and with as_dict {'predictions': them, 'logprobs' [Q, 1]}.
        ban: the decoding constraints of the sentences (_constraints), armed on the context's stream right before the call.
        trace_n (trace_param): the request is traced -- the result is then the dict whatever as_dict says, with the trace's keys."""
        kind = self.decoder.kind
        if frames is None:
            self._prepare(eng, None)
            if len(prefixes) > eng.c.max_batch:
                raise ValueError(f"{len(prefixes)} questions exceed max_batch={eng.c.max_batch}")
            if any(i < 0 or i >= eng.resident for i in image_of) or len(image_of) != len(prefixes):
                raise ValueError(f"image_of must name one of the {eng.resident} resident images for each of the "
                                 f"{len(prefixes)} sentences")

        def launch():
            if ban is not None:
                _arm(eng, ban)
            trace = _arm_trace(eng, trace_n, len(prefixes), search, stream is not None)
            out = eng.generate_prefixed(frames, search, prefixes, image_of=image_of, sync=False, host_out=stream is not None)
            return out if trace is None else (*out, trace)

        def finish(out):
            tokens, logprobs, sent, info = out[:4]
            eng.check_finite(info.tolist())
            plens = [len(p) for p in prefixes]
            preds, logprobs = format_predictions(tokens.cpu(), logprobs, sent.cpu(), plens, kind)
            if len(out) > 4:
                nout = 1 if tokens.dim() == 2 else int(tokens.shape[1])
                res = {"predictions": preds, "logprobs": logprobs.cpu()}
                res.update(format_trace(out[4], trace_spans(len(prefixes), nout, int(tokens.shape[-1]), sent.cpu(), plens, kind)))
                return res
            return {"predictions": preds, "logprobs": logprobs.cpu()} if as_dict else preds

        return Pending(stream, launch, finish, keep=(frames,), engine=eng)

    def answer(self, image: Union[torch.Tensor, Sequence[torch.Tensor]], prefixes: Sequence[Sequence[int]]):
        """Several questions about ONE image in one engine call: submit_answers(...).result() on context 0."""
        frames = list(image) if isinstance(image, (list, tuple)) else [image]
        assert frames[0].shape[0] == 1, "answer() takes one image (or one clip)"
        return self._on_context0(lambda: self.submit_answers(image, prefixes))

    def _on_context0(self, submit):
        """submit().result() on context 0 and the caller's stream (model(batch), answer, generate_ragged).  With set_pipeline
        active, context 0 may still have a submission in flight on its own stream: the caller's stream waits for it, and
        context 0's stream then waits for this call, so the context's workspaces are never in use on two streams at once."""
        ctxs = getattr(self, "_ctxs", None)
        if not ctxs:
            return submit().result()
        cur, own = torch.cuda.current_stream(), self._streams[0]
        cur.wait_stream(own)
        self._ctxs = None                                               # _context() -> (self.engine, None)
        try:
            pending = submit()
        finally:
            self._ctxs = ctxs
            own.wait_stream(cur)
        return pending.result()


class StaleImagesError(RuntimeError):
    """A follow-up request names images that its context no longer holds."""


class _ResultDict(dict):
    """What Pending.result() returns for dict results: the dict, plus `.pending` so that it can be passed as on=."""
    pending = None


class _ResultList(list):
    pending = None


class Pending:
    """A request enqueued on a context's stream (CaptioningModel.submit / submit_answers).  It records the engine context
    that ran it and that context's image generation after the launch (Engine.generation): a follow-up request issued with
    on=<this> (or with the result it returned) runs on the same context and stream, and is refused once another call has
    replaced the images there."""

    def __init__(self, stream, launch, finish, keep=(), engine=None):
        self._finish, self._keep, self._done, self._value, self._stream = finish, keep, False, None, stream
        self.engine = engine
        if stream is None:
            self._out = launch()
            self._event = None
        else:
            stream.wait_stream(torch.cuda.current_stream())          # the inputs were produced on the caller's stream
            with torch.cuda.stream(stream):
                self._out = launch()
                self._event = torch.cuda.Event()
                self._event.record()
        self.generation = engine.generation if engine is not None else None

    wait_s = 0.0            # class-wide: seconds spent waiting for the device in result() (diagnostics of the TSV task)

    def result(self):
        if not self._done:
            import time
            t0 = time.perf_counter()
            if self._event is not None:
                self._event.synchronize()
            else:
                torch.cuda.current_stream().synchronize()
            Pending.wait_s += time.perf_counter() - t0
            value = self._finish(self._out)
            if type(value) is dict:
                value = _ResultDict(value)
            elif type(value) is list:
                value = _ResultList(value)
            if isinstance(value, (_ResultDict, _ResultList)):
                value.pending = self
            self._value = value
            self._done, self._out, self._keep = True, None, ()
        return self._value


def _on_context_stream(model, eng, fn):
    """fn() on the stream of the pipeline context `eng` (ordered behind its own work), or on the caller's stream"""
    for c, st in zip(getattr(model, "_ctxs", None) or [], getattr(model, "_streams", None) or []):
        if c is eng and st is not None:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                return fn()
    return fn()


class ImageStore:
    """Encoded images kept beyond the call that encoded them (include/gitmi.h GITMI_SEARCH_KEEP / GITMI_SEARCH_RECALL): one device
    tensor of `capacity` slots, caller keys mapped to slots, the least recently used key evicted when a new one needs a slot.

        first = model.submit({'image': images}); first.result()
        store.put(first, keys=['a', 'b', 'c'])                  # after any number of other requests, on any context:
        h = store.recall(['c', 'a', 'c'])                       # image 0 = 'c', image 1 = 'a', image 2 = 'c' again
        model.submit_followup({'prefixes': qs, 'image_of': [0, 1, 2]}, on=h).result()

    The handle recall returns is accepted as on= wherever a Pending is (submit_followup, submit_answers(None, ...), score(None, ...),
    rank(None, ...), attend(None, ...)); StaleImagesError is raised once another call has replaced the images on its context.
    With a pipelined model (set_pipeline) put reads from the context that produced the result and recall binds its handle to
    the context that performed it.  The slots are plain bytes of this model's weights: `tensor` may be saved and loaded."""

    def __init__(self, model: "CaptioningModel", capacity: int):
        if int(capacity) < 1:
            raise ValueError("an image store needs at least one slot")
        eng = model.engine
        self.model, self.capacity = model, int(capacity)
        self.tensor = eng.memory_store(self.capacity)
        self._entries: Dict[object, tuple] = {}          # key -> (slot, geometry of the kept image); insertion order = LRU order
        self._free = list(range(self.capacity - 1, -1, -1))

    def __contains__(self, key) -> bool:
        return key in self._entries

    def __len__(self) -> int:
        return len(self._entries)

    def keys(self):
        """The keys held, least recently used first."""
        return list(self._entries)

    def evict(self, key) -> None:
        slot, _ = self._entries.pop(key)
        self._free.append(slot)

    def _touch(self, key) -> None:
        self._entries[key] = self._entries.pop(key)

    def _slot_for(self, key, pinned) -> int:
        """The slot `key` is (over)written in: its own, a free one, or the least recently used key's that is not in `pinned`."""
        if key in self._entries:
            return self._entries[key][0]
        if not self._free:
            victim = next((k for k in self._entries if k not in pinned), None)
            if victim is None:
                raise ValueError(f"{len(pinned)} keys in one call exceed the {self.capacity} slots of the store")
            self.evict(victim)
        return self._free.pop()

    def _on(self, eng, fn):
        return _on_context_stream(self.model, eng, fn)

    def put(self, source, keys: Sequence, images: Optional[Sequence[int]] = None) -> None:
        """Keep images of a finished call: `source` is the Pending of the call that encoded them (or a recall handle), or the
        result it returned; key keys[q] names resident image images[q] (default: image q).  A key already held is overwritten
        in its slot.  Raises StaleImagesError if the context no longer holds the images of `source`."""
        pending = getattr(source, "pending", source)
        if not isinstance(pending, Pending) or pending.engine is None:
            raise TypeError("put takes the Pending of the call that encoded the images, or the result it returned")
        eng = pending.engine
        if eng.generation != pending.generation or eng.resident is None:
            raise StaleImagesError("the images of this handle are no longer resident on its context: another call has replaced "
                                   "them (or a setter dropped them) since it was issued")
        keys = list(keys)
        images = list(range(len(keys))) if images is None else [int(i) for i in images]
        if len(images) != len(keys) or len(set(keys)) != len(keys):
            raise ValueError("put needs one image index per key, every key once")
        if any(i < 0 or i >= eng.resident for i in images):
            raise ValueError(f"images must name some of the {eng.resident} resident images")
        if len(keys) > self.capacity:
            raise ValueError(f"{len(keys)} keys in one call exceed the {self.capacity} slots of the store")
        slots = [self._slot_for(k, keys) for k in keys]
        try:
            kept = self._on(eng, lambda: eng.keep(self.tensor, slots, images))
        except Exception:
            for k, s in zip(keys, slots):       # nothing is known about what the slots hold now
                if k in self._entries:
                    self.evict(k)
                else:
                    self._free.append(s)
            raise
        for k, s, g in zip(keys, slots, kept["geometry"]):
            self._entries.pop(k, None)
            self._entries[k] = (s, g)

    def recall(self, keys: Sequence, context=None) -> "Pending":
        """Make the images of `keys` (any order, repeats) the resident batch of an engine context -- `context`, default the next
        one in the model's rotation -- and return the handle follow-up requests take as on=: image q of the batch is keys[q].
        `.result()`: {'stride', 'max_rows', 'total_rows'}.  KeyError for a key that is not held (never kept, or evicted)."""
        keys = list(keys)
        missing = [k for k in keys if k not in self._entries]
        if missing:
            raise KeyError(f"not in the image store (never kept, or evicted): {missing[:4]}")
        if context is None:
            eng, _ = self.model._context()
        else:
            eng = context
            self.model._last = eng
        slots = [self._entries[k][0] for k in keys]
        geometry = [self._entries[k][1] for k in keys]
        for k in keys:
            self._touch(k)
        info = self._on(eng, lambda: eng.recall(self.tensor, slots, geometry))
        return Pending(None, lambda: info, lambda out: dict(out), engine=eng)


class FeatureStore:
    """Visual features kept beyond the call that encoded them (include/gitmi.h GITMI_SEARCH_FEATURES): the sibling of ImageStore
    that holds the feature rows alone -- [capacity, N, vit_width] for the model's current uniform image shape, 13 x smaller per
    image than an ImageStore slot in 16-bit -- and pays one prefill at recall.  Caller keys map to slots, the least recently
    used key is evicted when a new one needs a slot.  A video model slides a window over per-frame features:

        store.put(frame_t, keys=[('video', t)])                                   # one encoder pass per NEW frame
        h = store.recall([[('video', t - 5 + i) for i in range(6)]])              # image 0 = the window, embedding i on key i
        model.submit_followup({'prefixes': [[cls]], 'image_of': [0]}, on=h).result()

    dtype: torch.float32 (exact: what the encoder's own store rounds) or the engine's 16-bit operand type (half the bytes; the
    rows are rounded by torch, which is the same round-to-nearest-even).  The handle recall returns is accepted as on= wherever
    a Pending is; StaleImagesError is raised once another call has replaced the images on its context."""

    def __init__(self, model: "CaptioningModel", capacity: int, dtype: torch.dtype = torch.float32):
        if int(capacity) < 1:
            raise ValueError("a feature store needs at least one slot")
        eng = model.engine
        self.model, self.capacity, self.dtype = model, int(capacity), dtype
        self.rows, self.width = int(eng.n_tok), int(eng.c.vit_width)
        self.tensor = eng.feature_store(self.capacity, dtype)
        self._entries: Dict[object, int] = {}            # key -> slot; insertion order = LRU order
        self._free = list(range(self.capacity - 1, -1, -1))

    def __contains__(self, key) -> bool:
        return key in self._entries

    def __len__(self) -> int:
        return len(self._entries)

    def keys(self):
        """The keys held, least recently used first."""
        return list(self._entries)

    @property
    def bytes_per_image(self) -> int:
        return self.rows * self.width * self.tensor.element_size()

    def evict(self, key) -> None:
        self._free.append(self._entries.pop(key))

    def _touch(self, key) -> None:
        self._entries[key] = self._entries.pop(key)

    def _slot_for(self, key, pinned) -> int:
        if key in self._entries:
            return self._entries[key]
        if not self._free:
            victim = next((k for k in self._entries if k not in pinned), None)
            if victim is None:
                raise ValueError(f"{len(pinned)} keys in one call exceed the {self.capacity} slots of the store")
            self.evict(victim)
        return self._free.pop()

    def put(self, frames: torch.Tensor, keys: Sequence) -> None:
        """Encode `frames` [B, 3, H, W] as a bare tensor (no temporal embedding) and keep image b's feature rows under keys[b]."""
        if int(frames.shape[0]) != len(list(keys)):
            raise ValueError(f"{len(list(keys))} keys for {int(frames.shape[0])} frames")
        self.put_features(self.model.features(frames), keys)

    def put_features(self, rows: torch.Tensor, keys: Sequence) -> None:
        """Keep feature rows [B, N, vit_width] (fp32, or the store's dtype) under keys[b]; a key already held is overwritten."""
        keys = list(keys)
        if tuple(rows.shape) != (len(keys), self.rows, self.width):
            raise ValueError(f"feature rows must be [{len(keys)}, {self.rows}, {self.width}] for {len(keys)} keys, got {tuple(rows.shape)}")
        if len(set(keys)) != len(keys):
            raise ValueError("put needs every key once")
        if len(keys) > self.capacity:
            raise ValueError(f"{len(keys)} keys in one call exceed the {self.capacity} slots of the store")
        slots = [self._slot_for(k, keys) for k in keys]
        self.tensor[torch.as_tensor(slots, device=self.tensor.device)] = rows.to(device=self.tensor.device, dtype=self.dtype)
        for k, s in zip(keys, slots):
            self._entries.pop(k, None)
            self._entries[k] = s

    def pieces(self, windows: Sequence[Sequence], temporal=None):
        """(pieces, image_of, F) of recall: image q is the concatenation of the rows of windows[q]'s keys.  temporal: per window
        the temporal index of every key (None: none); default: index i for the i-th key of a window of more than one key on a
        model with temporal embeddings, else none.  KeyError for a key that is not held."""
        windows = [list(w) for w in windows]
        missing = [k for w in windows for k in w if k not in self._entries]
        if missing:
            raise KeyError(f"not in the feature store (never put, or evicted): {missing[:4]}")
        if not windows or any(len(w) == 0 for w in windows):
            raise ValueError("recall needs at least one window, every window at least one key")
        if temporal is not None and ([len(t) for t in temporal] != [len(w) for w in windows]):
            raise ValueError("temporal needs one index (or None) per key of every window")
        nf = int(self.model.cfg.num_frames)
        pieces, image_of = [], []
        for q, w in enumerate(windows):
            for i, k in enumerate(w):
                t = temporal[q][i] if temporal is not None else (i if nf > 0 and len(w) > 1 else None)
                pieces.append((self._entries[k] * self.rows, self.rows, t))
                image_of.append(q)
        return pieces, image_of, max(len(w) for w in windows)

    def recall(self, windows: Sequence[Sequence], temporal=None, context=None) -> "Pending":
        """Make the windows the resident batch of an engine context -- `context`, default the next one in the model's rotation --
        and run the prefill over them; returns the handle follow-up requests take as on=.  `.result()`: {'stride', 'max_rows',
        'total_rows'}."""
        pieces, image_of, F = self.pieces(windows, temporal)
        for w in windows:
            for k in w:
                self._touch(k)
        return self.model.submit_features(self.tensor.view(-1, self.width), pieces, image_of, F, context=context)


def get_git_model(tokenizer, param: Optional[dict], precision: str = "f16", max_batch: int = 64,
                  decoder=None, device: Optional[int] = None, max_context: int = 0) -> CaptioningModel:
    """Same role as the reference's get_git_model (model.py:9-61): GIT decoder hyper-parameters are
    fixed, the encoder follows param['image_encoder_type'].  The default search is the shipped one:
    GeneratorWithBeamSearch(beam_size=4, length_penalty=0.6, max_steps=1024) (model.py:34-40)."""
    cfg = config_from_param(param)
    sos = getattr(tokenizer, "cls_token_id", None)
    eos = getattr(tokenizer, "sep_token_id", None)
    if sos is not None and eos is not None and (sos != cfg.sos or eos != cfg.eos):
        import dataclasses
        cfg = dataclasses.replace(cfg, sos=int(sos), eos=int(eos))
    if decoder is None:
        decoder = GeneratorWithBeamSearch(eos_index=cfg.eos, max_steps=1024, beam_size=4, length_penalty=0.6)
    logging.info("building GIT engine: %s, search %s", cfg, type(decoder).__name__)
    model = CaptioningModel(cfg, decoder, precision=precision, max_batch=max_batch, device=device, max_context=max_context,
                            context_not_share_embedding=bool((param or {}).get("context_not_share_embedding", False)))
    model.tokenizer = tokenizer        # search_param['bad_words'] goes through it
    return model
