"""Ragged image batches on the MI355X (gitmi_set_image_shape(e, 0, 0)): one engine call over images of different sizes.
Every image must get exactly what a call with that image alone gets: per-image calls at its own shape (bit for bit in
f32), the CPU oracle (f32 ids), and the same result whatever its batch companions or its place in the batch."""
import pytest
import torch

from oracle import git_oracle as O

pytestmark = pytest.mark.gpu

CFG = O.CONFIGS["TINY"]
MAX_HW = (480, 640)                   # capacity grid 30 x 40: Nmax = 1201 rows per image
# token rows n = (h/16)(w/16) + 1 of the shapes below: 2, 17, 31, 32, 33, 881, 901, 1201 and a few between
SHAPES = [(16, 16), (64, 64), (80, 96), (16, 496), (64, 128), (352, 640), (480, 480), (480, 640), (96, 64), (72, 100)]
PRECS = ("f32", "f16", "bf16")
FEAT_TOL = {"f32": 0.0, "bf16": 0.15, "f16": 0.05}
T = 12


def _weights():
    return O.make_weights(CFG, seed=21, tie_output=False, eos_bias=-2.0)


def _images(shapes, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, h, w, generator=g) for h, w in shapes]


def _engine(precision, B, beams=1):
    from generativeimage2text_amd.engine import Engine
    eng = Engine(CFG, precision=precision, max_batch=B, max_beams=beams, max_frames=1, max_text_len=T, max_image_hw=MAX_HW)
    eng.load_state_dict(_weights())
    return eng


def _greedy():
    from generativeimage2text_amd.engine import Engine
    return Engine.make_search("greedy", T, 1, 1)


def _ntok(h, w):
    return (h // 16) * (w // 16) + 1


def _ragged_generate(eng, imgs):
    tok, lp, info = eng.generate(eng.ragged([i.cuda() for i in imgs]), _greedy())
    return tok.cpu(), lp.cpu(), info.cpu()


def _single_generate(eng, img):
    tok, lp, info = eng.generate([img[None].cuda()], _greedy())
    return tok.cpu()[0], lp.cpu()[0], info.cpu()


def _row_ids(tok_row, L):
    """the ids a batch-1 call returns (info[0] of the call = its sequence length); EOS-padded rows compared up to EOS"""
    row = tok_row.tolist()
    if CFG.eos in row[1:]:
        row = row[:row.index(CFG.eos, 1) + 1]
    return row[:L]


@pytest.mark.parametrize("precision", PRECS)
def test_ragged_features_equal_per_image_calls(precision):
    imgs = _images(SHAPES[:8])
    eng = _engine(precision, len(imgs))
    feats = eng.encode(eng.ragged([i.cuda() for i in imgs])).cpu()
    Nmax = eng.max_tokens
    assert feats.shape == (len(imgs), Nmax, CFG.vit_width)
    for b, im in enumerate(imgs):
        n = _ntok(*im.shape[1:])
        ref = eng.encode([im[None].cuda()]).cpu()[0]
        assert ref.shape[0] == n
        if precision == "f32":
            assert torch.equal(feats[b, :n], ref), (b, (feats[b, :n] - ref).abs().max())
        else:
            err = (feats[b, :n] - ref).abs().max().item()
            assert err < FEAT_TOL[precision], (b, err)
        assert torch.count_nonzero(feats[b, n:]) == 0, f"image {b}: padding rows of the features are not zero"
    eng.close()


def test_ragged_f32_ids_equal_oracle_and_per_image_calls():
    imgs = _images(SHAPES[:8])
    eng = _engine("f32", len(imgs))
    tok, lp, info = _ragged_generate(eng, imgs)
    assert int(info[3]) == 0
    w = _weights()
    for b, im in enumerate(imgs):
        t1, l1, i1 = _single_generate(eng, im)
        L = int(i1[0])
        assert _row_ids(tok[b], L) == _row_ids(t1, L), b
        assert lp[b].item() == l1.item(), (b, lp[b].item(), l1.item())       # bit for bit
        with torch.no_grad():
            ref = O.caption(CFG, w, [im[None]], O.SearchConfig("greedy", T, 1, 1))
        pred = ref["predictions"][0].tolist()
        assert _row_ids(tok[b], len(pred)) == pred, (b, tok[b].tolist(), pred)
    eng.close()


@pytest.mark.parametrize("precision", ("f16", "bf16"))
def test_ragged_16bit_logprobs_close_to_per_image_calls(precision):
    imgs = _images(SHAPES[:6], seed=8)
    eng = _engine(precision, len(imgs))
    tok, lp, info = _ragged_generate(eng, imgs)
    from tools.parity import logit_bound
    for b, im in enumerate(imgs):
        t1, l1, i1 = _single_generate(eng, im)
        L = int(i1[0])
        assert _row_ids(tok[b], L) == _row_ids(t1, L), b
        # a mean log-prob over the row: within the parity.py logit bound of this precision (span of TINY's logits < 8)
        assert abs(lp[b].item() - l1.item()) < 2 * logit_bound(precision, 8.0), (b, lp[b].item(), l1.item())
    eng.close()


@pytest.mark.parametrize("precision", PRECS)
def test_ragged_batch_independence(precision):
    """image 0 and image 2 keep bit-identical ids / log-probs when their companions change shape and when the batch is
    permuted: padding never leaks into another image"""
    a, c = _images([(64, 128), (352, 640)], seed=11)
    comp1 = _images([(16, 16), (480, 640), (80, 96)], seed=12)
    comp2 = _images([(480, 480), (64, 64), (16, 496)], seed=13)
    eng = _engine(precision, 5)
    t1, l1, _ = _ragged_generate(eng, [a, comp1[0], c, comp1[1], comp1[2]])
    t2, l2, _ = _ragged_generate(eng, [a, comp2[0], c, comp2[1], comp2[2]])
    t3, l3, _ = _ragged_generate(eng, [comp2[2], c, comp2[0], a, comp2[1]])          # permuted
    for (i, j, k) in ((0, 0, 3), (2, 2, 1)):
        assert torch.equal(t1[i], t2[j]) and torch.equal(t1[i], t3[k]), (precision, i)
        assert l1[i].item() == l2[j].item() == l3[k].item(), (precision, i)
    eng.close()


def test_ragged_prefixed_questions_equal_per_image_calls():
    """batched VQA over images of different sizes: two questions per image, each equal to its own batch-1 call (f32)"""
    imgs = _images([(64, 64), (480, 640), (96, 64), (16, 496)], seed=3)
    qs = [[CFG.sos, 11, 12], [CFG.sos, 13], [CFG.sos, 14, 15, 16], [CFG.sos, 17], [CFG.sos, 18, 19],
          [CFG.sos, 20], [CFG.sos, 21, 22], [CFG.sos, 23, 24, 25]]
    image_of = [0, 0, 1, 1, 2, 2, 3, 3]
    eng = _engine("f32", len(qs))
    tok, lp, sent, info = eng.generate_prefixed(eng.ragged([i.cuda() for i in imgs]), _greedy(), qs, image_of=image_of)
    tok, lp, sent = tok.cpu(), lp.cpu(), sent.cpu()
    for q, (p, b) in enumerate(zip(qs, image_of)):
        t1, l1, s1, _ = eng.generate_prefixed([imgs[b][None].cuda()], _greedy(), [p], image_of=[0])
        L = int(s1[0, 0])
        assert int(sent[q, 0]) == L and tok[q, :L].tolist() == t1.cpu()[0, :L].tolist(), q
        assert lp[q].item() == l1.cpu()[0].item(), q
    eng.close()


@pytest.mark.parametrize("precision", PRECS)
def test_ragged_score_equals_per_image_scoring(precision):
    imgs = _images([(16, 16), (80, 96), (480, 640), (64, 128)], seed=4)
    caps = torch.tensor([[CFG.sos, 5, 6, 7, CFG.eos], [CFG.sos, 8, 9, CFG.eos, 0], [CFG.sos, 10, 11, 12, 13],
                         [CFG.sos, 14, CFG.eos, 0, 0]])
    lens = [5, 4, 5, 3]
    eng = _engine(precision, len(imgs))
    out = eng.score(eng.ragged([i.cuda() for i in imgs]), caps, lengths=lens).cpu()
    for b, im in enumerate(imgs):
        ref = eng.score([im[None].cuda()], caps[b:b + 1], lengths=[lens[b]]).cpu()[0]
        if precision == "f32":
            assert torch.equal(out[b], ref), (b, (out[b] - ref).abs().max())
        else:
            assert (out[b] - ref).abs().max().item() < 0.1, b
    eng.close()


def test_ragged_rejected_image_is_reported_and_isolated():
    """an oversize descriptor entry is caught on the device: its sentence comes back NaN and counted in info[3]; the other
    images' results are unchanged (their planes are staged as before, the bad entry's are never read)"""
    from generativeimage2text_amd.engine import RaggedImages
    imgs = _images([(64, 64), (80, 96), (64, 128)], seed=9)
    eng = _engine("f32", 3)
    good = eng.ragged([i.cuda() for i in imgs])
    t0, l0, _ = _ragged_generate(eng, imgs)
    buf = good.buffer.clone()
    buf[4:8].view(torch.int32).copy_(torch.tensor([4000, 4000, int(buf[6:7].view(torch.int32).item()), 0], dtype=torch.int32))
    tok, lp, info = eng.generate(RaggedImages(buf, good.shapes), _greedy(), sync=False)
    torch.cuda.synchronize()
    tok, lp, info = tok.cpu(), lp.cpu(), info.cpu()
    assert int(info[3]) == 1
    assert torch.isnan(lp[1])
    for b in (0, 2):
        assert torch.equal(tok[b], t0[b]) and lp[b].item() == l0[b].item(), b
    with pytest.raises(Exception):
        eng.check_finite(info)
    eng.close()


def test_ragged_graphs_follow_the_shapes_of_every_call():
    """graphs on (the default): the captured graph is keyed on the capacity, the shapes are read on the device -- a second
    call with another shape mix must not replay the first one's shapes"""
    mix1 = _images([(64, 64), (480, 640), (80, 96)], seed=21)
    mix2 = _images([(352, 640), (16, 16), (96, 64)], seed=22)
    eng = _engine("f32", 3)
    eng.lib.gitmi_set_graph(eng._h, 0)
    ref1, _, _ = _ragged_generate(eng, mix1)
    ref2, _, _ = _ragged_generate(eng, mix2)
    eng.lib.gitmi_set_graph(eng._h, 1)
    g1, _, _ = _ragged_generate(eng, mix1)
    g2, _, _ = _ragged_generate(eng, mix2)
    g1b, _, _ = _ragged_generate(eng, mix1)
    assert torch.equal(g1, ref1) and torch.equal(g2, ref2) and torch.equal(g1b, ref1)
    # back to a uniform shape: the uniform path as before
    u = _images([(64, 64)] * 3, seed=23)
    tu, _, _ = eng.generate([torch.stack(u).cuda()], _greedy())
    for b in range(3):
        t1, _, i1 = _single_generate(eng, u[b])
        L = int(i1[0])
        assert _row_ids(tu.cpu()[b], L) == _row_ids(t1, L)
    eng.close()


def test_captioning_model_generate_ragged_and_score_list():
    from generativeimage2text_amd.model import CaptioningModel, AutoRegressiveBeamSearch
    dec = AutoRegressiveBeamSearch(CFG.eos, max_steps=T, beam_size=1, fix_missing_prefix=True)
    m = CaptioningModel(CFG, dec, precision="f32", max_batch=4)
    m.engine.close()
    m.engine = _engine("f32", 4)
    m._loaded = True
    imgs = [i.cuda() for i in _images([(64, 64), (80, 96), (480, 640)], seed=31)]
    out = m.generate_ragged(imgs)
    for b, im in enumerate(imgs):
        one = m({"image": im[None]})["predictions"][0].tolist()
        assert out["predictions"][b].tolist()[:len(one)] == one, b
    ans = m.generate_ragged(imgs, prefixes=[[CFG.sos, 7], [CFG.sos, 8, 9]], image_of=[2, 0])
    for q, (p, b) in enumerate(zip([[CFG.sos, 7], [CFG.sos, 8, 9]], [2, 0])):
        assert ans["predictions"][q] == m.answer(imgs[b][None], [p])[0], q
    caps = [[CFG.sos, 5, 6], [CFG.sos, 7], [CFG.sos, 8, 9, 10]]
    s = m.score(imgs, caps)
    for b in range(3):
        s1 = m.score(imgs[b][None], [caps[b]])
        assert torch.equal(s["logprobs"][b, :len(caps[b])], s1["logprobs"][0]), b
    m.close()


@pytest.mark.parametrize("cap", [224, 256])
@pytest.mark.parametrize("precision", PRECS)
def test_ragged_at_captioning_capacities(cap, precision):
    """capacity grids of 197 / 257 rows (a captioning model's own 224 / 256 square): the ragged short single-pass encoder
    kernels (13 / 17 sub-tiles) and, at N_pad <= 256, the two-wave decode with an empty second wave for images of <= 32 keys.
    Features equal per-image calls (bit for bit in f32), ids / log-probs independent of companions and order."""
    from generativeimage2text_amd.engine import Engine
    eng = Engine(CFG, precision=precision, max_batch=5, max_beams=1, max_frames=1, max_text_len=T, max_image_hw=(cap, cap))
    eng.load_state_dict(_weights())
    assert eng.max_tokens == (cap // 16) ** 2 + 1
    a, c = _images([(16, 16), (cap, cap)], seed=41)
    comp1 = _images([(64, 64), (112, 160), (32, cap)], seed=42)
    comp2 = _images([(cap - 16, 48), (16, 64), (96, 96)], seed=43)
    batch = [a, comp1[0], c, comp1[1], comp1[2]]
    feats = eng.encode(eng.ragged([i.cuda() for i in batch])).cpu()
    for b, im in enumerate(batch):
        n = _ntok(*im.shape[1:])
        ref = eng.encode([im[None].cuda()]).cpu()[0]
        if precision == "f32":
            assert torch.equal(feats[b, :n], ref), b
        else:
            assert (feats[b, :n] - ref).abs().max().item() < FEAT_TOL[precision], b
        assert torch.count_nonzero(feats[b, n:]) == 0, b
    t1, l1, _ = _ragged_generate(eng, batch)
    t2, l2, _ = _ragged_generate(eng, [a, comp2[0], c, comp2[1], comp2[2]])
    t3, l3, _ = _ragged_generate(eng, [comp2[2], c, comp2[0], a, comp2[1]])
    for (i, j, k) in ((0, 0, 3), (2, 2, 1)):
        assert torch.equal(t1[i], t2[j]) and torch.equal(t1[i], t3[k]), (precision, i)
        assert l1[i].item() == l2[j].item() == l3[k].item(), (precision, i)
    if precision == "f32":
        for b, im in enumerate(batch):
            ts, ls, i1 = _single_generate(eng, im)
            L = int(i1[0])
            assert _row_ids(t1[b], L) == _row_ids(ts, L) and l1[b].item() == ls.item(), b
    eng.close()


def test_tsv_mixed_shapes_answers_equal_per_shape_answers(tmp_path):
    """the TSV task's two VQA paths on a real engine (f32): run_tsv_inference with the model's submit_answers (images bucketed
    by shape) and with submit_ragged (mixed_shapes=True: one call across shapes) write the same answer rows"""
    from generativeimage2text_amd import inference, tsv_io
    from generativeimage2text_amd.model import CaptioningModel, AutoRegressiveBeamSearch
    import base64
    import json
    shapes = [(64, 64), (96, 64), (64, 64), (64, 128), (96, 64), (48, 80), (64, 128)]
    imgs = _images(shapes, seed=51)
    dec = AutoRegressiveBeamSearch(CFG.eos, max_steps=T, beam_size=1, fix_missing_prefix=True)
    m = CaptioningModel(CFG, dec, precision="f32", max_batch=12)
    m.engine.close()
    m.engine = _engine("f32", 12)
    m._loaded = True
    rows = [["key%d" % i, base64.b64encode(b"%02d" % i).decode()] for i in range(len(shapes))]
    tsv_io.tsv_writer(rows, str(tmp_path / "img.tsv"))
    q = [["key%d" % i, json.dumps([{"question": "%d %d" % (i, j), "question_id": 10 * i + j} for j in range(1 + i % 2)])]
         for i in range(len(shapes))]
    tsv_io.tsv_writer(q, str(tmp_path / "q.tsv"))

    def prefix(text):
        i, j = map(int, text.split())
        return [CFG.sos, 200 + i, 300 + j]

    def submit(imgs_, qss, mixed):
        prefixes = [prefix(t) for qs in qss for t in qs]
        image_of = [b for b, qs in enumerate(qss) for _ in qs]
        counts = [len(qs) for qs in qss]
        if mixed:
            h = m.submit_ragged([im.cuda() for im in imgs_], prefixes=prefixes, image_of=image_of)
            get = lambda: h.result()["predictions"]                                  # noqa: E731
        else:
            h = m.submit_answers(torch.stack(list(imgs_)).cuda(), prefixes, image_of)
            get = h.result

        class Done:
            def result(self):
                preds, out, lo = [str(p) for p in get()], [], 0
                for n in counts:
                    out.append(preds[lo:lo + n])
                    lo += n
                return out
        return Done()

    outs = {}
    for mixed in (False, True):
        out = str(tmp_path / ("out_%d.tsv" % mixed))
        inference.run_tsv_inference(
            str(tmp_path / "img.tsv"), str(tmp_path / "q.tsv"), out, transform=lambda b: imgs[int(b.decode())],
            caption_batch=None, answer_questions=None, batch_size=4, rank=0, world=1,
            submit_answers=lambda a, b, mixed=mixed: submit(a, b, mixed), max_questions=12, mixed_shapes=mixed)
        outs[mixed] = open(out, "rb").read()
    assert outs[True] == outs[False]
    assert outs[True].count(b"\n") == sum(1 + i % 2 for i in range(len(shapes)))
    m.close()


def test_context0_calls_while_pipelined_requests_are_in_flight():
    """model(batch) and answer() run on context 0 and the caller's stream while set_pipeline submissions are still in
    flight, one of them on context 0's own stream: every result equals the same call made with no pipeline."""
    from generativeimage2text_amd.model import CaptioningModel, AutoRegressiveBeamSearch
    dec = AutoRegressiveBeamSearch(CFG.eos, max_steps=T, beam_size=1, fix_missing_prefix=True)
    m = CaptioningModel(CFG, dec, precision="f32", max_batch=4)
    m.engine.close()
    m.engine = _engine("f32", 4)
    m._loaded = True
    g = torch.Generator().manual_seed(43)
    batches = [torch.randn(3, 3, CFG.image_size, CFG.image_size, generator=g).cuda() for _ in range(5)]
    qs = [[CFG.sos, 7], [CFG.sos, 8, 9], [CFG.sos, 5]]

    def cpu(out):
        return {k: v.cpu() for k, v in out.items()}
    ref = [cpu(m({"image": b})) for b in batches]
    ref_ans = m.answer(batches[1][:1], qs)
    m.set_pipeline(4)
    pending = [m.submit({"image": b}) for b in batches]              # the fifth goes to context 0 behind the first
    fwd = cpu(m({"image": batches[2]}))
    ans = m.answer(batches[1][:1], qs)
    got = [cpu(p.result()) for p in pending]
    for want, have in zip(ref + [ref[2]], got + [fwd]):
        assert torch.equal(want["predictions"], have["predictions"]) and torch.equal(want["logprobs"], have["logprobs"])
    assert ans == ref_ans
    m.close()
