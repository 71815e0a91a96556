"""The paths of gitmi_generate / gitmi_generate_prefixed that differ from the plain one only in HOW the launches reach the
device: two graphs instead of one (gitmi_set_encode_after, gitmi_profile_enable(e, 2)), eager launches (profile_enable(1),
a step budget above 32), the engine's own stream for a caller on the null stream.  Each must return what the plain path
returns, bit for bit, and fail by the residency rules tests/test_gpu_followup.py::test_residency_rules states for it.

TINY, 3 images, max_steps 8, a greedy and a 2-beam generator search, f32 and f16.  The plain path's results are computed
once per precision by a lone engine (graphs on, checked against graphs off) and shared."""
import functools

import pytest
import torch

from oracle import git_oracle as O
from test_gpu_followup import _Raw, _cpu, _engine, _same, _search, _tiny

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16")
T, B = 8, 3
T_LONG = 40                             # max_steps - minP > 32: the eager path with the finished-count poll
IMAGE_OF = [2, 0]


def _searches(steps=T):
    return {"greedy": _search("greedy", steps), "beam2": _search("beam", steps, 2, 2, 0.6)}


def _questions(cfg):
    return [[cfg.sos, 7, 44], [cfg.sos, 5]]


@functools.lru_cache(maxsize=None)
def _model():
    cfg, w, fa = _tiny()
    return cfg, w, (fa, [f.cuda() for f in O.make_images(cfg, B, 1, seed=93)])


def _new(precision, steps=T, graph=True):
    cfg, w, _ = _model()
    return _engine(cfg, w, precision, B, 2, steps, graph=graph)


def _three_calls(eng, frames, s):
    """a full call, a follow-up with the same sentences, a prefixed call with two questions of different lengths"""
    cfg = _model()[0]
    return [_cpu(eng.generate(frames, s)), _cpu(eng.generate(None, s)),
            _cpu(eng.generate_prefixed(frames, s, _questions(cfg), image_of=IMAGE_OF))]


@functools.lru_cache(maxsize=None)
def _plain(precision):
    """what a lone engine returns on the plain path, graphs on (and, checked here, graphs off); never modified afterwards"""
    cfg, _, sets = _model()
    ref = {}
    for graph in (True, False):
        eng = _new(precision, graph=graph)
        got = {}
        for name, s in _searches().items():
            got["full", name, 0], got["follow", name], got["prefixed", name] = _three_calls(eng, sets[0], s)
            got["full", name, 1] = _cpu(eng.generate(sets[1], s))
        # follow-ups over set 0: the same sentences after a greedy full call, then another search, then new questions
        eng.generate(sets[0], _searches()["greedy"])
        for name, s in _searches().items():
            got["follow_after_greedy", name] = _cpu(eng.generate(None, s))
            got["follow_prefixed", name] = _cpu(eng.generate_prefixed(None, s, _questions(cfg), image_of=IMAGE_OF))
        eng.close()
        if not ref:
            ref = got
        assert ref.keys() == got.keys()
        for key in ref:
            _same(ref[key], got[key])
    assert not torch.equal(ref["full", "greedy", 0][0], ref["full", "greedy", 1][0])     # the two image sets differ in their ids
    return ref


def _chained(precision):
    a = _new(precision)
    b = a.clone()
    b.set_encode_after(a)               # a has a watcher, b waits: both split their full calls into two graphs
    return a, b


@pytest.mark.parametrize("precision", PRECS)
def test_split_graphs_equal_the_single_graph(precision):
    ref, sets = _plain(precision), _model()[2]
    a, b = _chained(precision)
    for name, s in _searches().items():
        for _ in range(2):                                              # the second round replays both graphs of both contexts
            for i, frames in enumerate(sets):
                _same(ref["full", name, i], _cpu(a.generate(frames, s)))
                _same(ref["full", name, i], _cpu(b.generate(frames, s)))
        b.set_encode_after(None)                                        # `split` flips for both: captured again as one graph
        for i, frames in enumerate(sets):
            _same(ref["full", name, i], _cpu(a.generate(frames, s)))
            _same(ref["full", name, i], _cpu(b.generate(frames, s)))
        b.set_encode_after(a)
    b.close()
    a.close()


@pytest.mark.parametrize("precision", PRECS)
def test_followup_under_split(precision):
    ref, sets, cfg = _plain(precision), _model()[2], _model()[0]
    a, b = _chained(precision)
    s = _searches()
    for eng in (a, b):
        _same(ref["full", "greedy", 0], _cpu(eng.generate(sets[0], s["greedy"])))
        for _ in range(2):
            _same(ref["follow_after_greedy", "greedy"], _cpu(eng.generate(None, s["greedy"])))
        _same(ref["follow_after_greedy", "beam2"], _cpu(eng.generate(None, s["beam2"])))
        for name in s:
            _same(ref["follow_prefixed", name], _cpu(eng.generate_prefixed(None, s[name], _questions(cfg), image_of=IMAGE_OF)))
        _same(ref["full", "greedy", 1], _cpu(eng.generate(sets[1], s["greedy"])))        # and the full graphs are still there
    b.close()
    a.close()


@pytest.mark.parametrize("precision", PRECS)
def test_profile_mode_2_returns_the_same_and_times_both_graphs(precision):
    ref, sets = _plain(precision), _model()[2]
    eng = _new(precision)
    eng.profile_enable(2)
    for name, s in _searches().items():
        for _ in range(2):
            got = _three_calls(eng, sets[0], s)
            for key, out in zip((("full", name, 0), ("follow", name), ("prefixed", name)), got):
                _same(ref[key], out)
    p = eng.profile_read()
    assert p["vit_ms"] > 0 and p["decode_ms"] > 0 and p["decode_steps"] == T - 1, p
    p = eng.profile_read()                                              # the read reset the accumulators
    assert p["vit_ms"] == 0 and p["decode_ms"] == 0 and p["decode_steps"] == 0 and p["decode_step_ms"] == 0, p
    eng.profile_enable(0)                                               # captured again, unsplit
    for name, s in _searches().items():
        got = _three_calls(eng, sets[0], s)
        for key, out in zip((("full", name, 0), ("follow", name), ("prefixed", name)), got):
            _same(ref[key], out)
    eng.close()


@pytest.mark.parametrize("precision", PRECS)
def test_eager_paths_profile_mode_1_and_long_budget(precision):
    """profile_enable(1) launches eagerly with events around everything; a budget of more than 32 steps launches eagerly
    and polls the count of finished sentences.  The first must equal the plain path; the second has no graph counterpart
    (the budget decides the path), so it must equal itself under profile_enable(1) -- the same launches without the poll,
    all 39 steps -- and its follow-up must equal its full call."""
    ref, sets, cfg = _plain(precision), _model()[2], _model()[0]
    eng = _new(precision, T_LONG)
    eng.profile_enable(1)
    for name, s in _searches().items():
        got = _three_calls(eng, sets[0], s)
        for key, out in zip((("full", name, 0), ("follow", name), ("prefixed", name)), got):
            _same(ref[key], out)
    p = eng.profile_read()
    assert p["vit_ms"] > 0 and p["decode_ms"] > 0, p
    unpolled = {name: _three_calls(eng, sets[0], s) for name, s in _searches(T_LONG).items()}
    eng.profile_enable(0)
    for name, s in _searches(T_LONG).items():
        got = _three_calls(eng, sets[0], s)
        _same(got[0], got[1])
        for x, y in zip(unpolled[name], got):
            _same(x, y)
    for name, s in _searches().items():                                 # and the short budget is back on its graphs
        _same(ref["full", name, 0], _cpu(eng.generate(sets[0], s)))
    eng.close()


@pytest.mark.parametrize("precision", PRECS)
def test_null_stream_runs_on_the_engines_own_stream(precision):
    """the null stream cannot be captured: the call runs on the engine's own stream between two fences.  The same calls on
    a stream of the caller's are captured on that stream itself; both return the plain path's results."""
    ref, sets = _plain(precision), _model()[2]
    eng = _new(precision)
    torch.cuda.synchronize()
    for stream in (torch.cuda.default_stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            for name, s in _searches().items():
                for _ in range(2):
                    _same(ref["full", name, 0], _cpu(eng.generate(sets[0], s)))
                    _same(ref["follow", name], _cpu(eng.generate(None, s)))
        torch.cuda.synchronize()
    eng.close()


@pytest.mark.parametrize("path", ("split", "profile2"))
@pytest.mark.parametrize("precision", PRECS)
def test_failure_rules_under_split_and_profile_2(precision, path):
    """an argument error found before any launch leaves the resident images as they were, in a follow-up and in a full
    call; a follow-up with a wrong B fails by name and leaves them too"""
    ref, sets = _plain(precision), _model()[2]
    eng = _new(precision)
    other = None
    if path == "split":
        other = eng.clone()
        eng.set_encode_after(other)
    else:
        eng.profile_enable(2)
    raw = _Raw(eng, T)
    want = ref["full", "greedy", 0]
    assert raw(sets[0], B)[0] == 0
    _same(want, raw.result(B))
    for frames in (None, sets[0]):
        rc, msg = raw(frames, B, max_steps=T + 1)
        assert rc != 0 and "max_steps" in msg
        assert raw(None, B)[0] == 0
        _same(want, raw.result(B))
    rc, msg = raw(None, 1)
    assert rc != 0 and "B=1" in msg and f"{B} images" in msg
    assert raw(None, B)[0] == 0
    _same(want, raw.result(B))
    assert raw(sets[1], B)[0] == 0                                      # and the engine is as usable as before
    _same(ref["full", "greedy", 1], raw.result(B))
    eng.close()
    if other is not None:
        other.close()
