#!/usr/bin/env python
"""When does the generate path capture, and what does each call replay?  A fixed call sequence for
`rocprofv3 --kernel-trace --stats`, and the comparison of two such traces: a change to the host side of the path
(engine.hip: generate_run, the hipGraph slots) must leave kernel names and call counts exactly as they were.

The sequence, on one f16 engine `a` and its clone `b` with b.set_encode_after(a) (both split their full calls into an
encode + prefill graph and a decode graph), each call on `a` then on `b`:
    full, full again (a replay), follow-up, follow-up again (a replay); b.set_encode_after(None); one more full call
    (`split` flips: captured again as one graph).
TINY model, 3 images, greedy, max_steps 8: the launches are what counts, not their durations.

    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/graph_paths_trace.py
    python tools/rocprof_summary.py DIR/trace_results.db TABLE
    python tools/graph_paths_trace.py --compare TABLE_A TABLE_B        # exit code 1 and the differing rows if they differ"""
from __future__ import annotations

import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sequence() -> None:
    import torch
    from generativeimage2text_amd.engine import Engine
    from oracle import git_oracle as O
    cfg = O.CONFIGS["TINY"]
    frames = [f.cuda() for f in O.make_images(cfg, 3, 1, seed=82)]
    a = Engine(cfg, precision="f16", max_batch=3, max_beams=1, max_frames=1, max_text_len=8)
    a.load_state_dict(O.make_weights(cfg, seed=81, tie_output=False, successor=2.0, eos_bias=1.0))
    b = a.clone()
    b.set_encode_after(a)
    s = Engine.make_search("greedy", 8, 1, 1)
    for fr in (frames, frames, None, None):
        for eng in (a, b):
            eng.generate(fr, s)
    b.set_encode_after(None)
    for eng in (a, b):
        eng.generate(frames, s)
    torch.cuda.synchronize()
    b.close()
    a.close()


def launches(table: str) -> collections.Counter:
    """(kernel <<<workgroups>>>) -> calls of a tools/rocprof_summary.py table"""
    out = collections.Counter()
    for line in open(table):
        f = line.split(None, 9)
        if len(f) == 10 and f[0].endswith("%"):
            out[f[9].strip()] += int(f[1])
    return out


def main() -> int:
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        x, y = launches(sys.argv[2]), launches(sys.argv[3])
        for k in sorted(set(x) | set(y)):
            if x[k] != y[k]:
                print("%6d %6d  %s" % (x[k], y[k], k))
        print("%d kernels, %d / %d launches: %s" % (len(set(x) | set(y)), sum(x.values()), sum(y.values()),
                                                   "equal" if x == y else "DIFFERENT"))
        return 0 if x == y and x else 1
    sequence()
    return 0


if __name__ == "__main__":
    sys.exit(main())
