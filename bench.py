#!/usr/bin/env python
"""Headline benchmark: captions/s for the GIT hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one pass of the whole hot path (ViT encode -> decoder prefill -> 19 KV-cached greedy
decode steps with on-device search) over one batch of B=64 synthetic 224x224 images per GPU that are
already resident in HBM (BASELINE.json configs[1]: GIT_BASE bs=64 greedy max_len=20; 16-bit operands: fp16 since round 6,
the build that meets the logit clause of north_star -- bf16 runs beside it as `alt_precision`), plus -- for
N > 1 -- the RCCL gather of the token ids to rank 0.  Images shard data-parallel across ranks with no
collective on the data path ("scaling": "weak").

Rank 0 prints ONE JSON line.  `value` is whole-job captions/s, `ms_per_step` the wall time of one timed step.  A plain
run does only what that figure needs: set-up, warm-up, the timed steps, `--dump-outputs DIR` if given (the ids, log-probs
and info of the last timed step as .npy files), the line.  Everything below runs with `--full` only.

With `--full`: `roofline` describes the dominant
kernel (the 16-bit MFMA GEMM inside the image encoder, MFMA-bound; fp16 and bf16 MFMAs share one peak on gfx950) from a separate HIP-event-instrumented
pass of the same workload; `roofline_decode` the HBM-bound decode step (hipGraph replays, events around the
decode graph); `parity` compares the generated ids with the reference's ids for this very workload
(tests/golden/full_*.npz, PARITY_GOLDENS); `cpu_baseline` times the CPU oracle (a port of the reference
algorithm, full recompute like the reference) on a bounded sample; for N > 1 `gather` reports the cost of the one
collective.

Without a launcher, `python bench.py --gpus N` starts the N ranks itself (torch.distributed.run, one process per GPU)
and refuses to print a line whose n_gpus differs from --gpus.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0     # dense bf16 MFMA peak, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0         # HBM3E spec peak


def gather_results(tokens: torch.Tensor, logprobs: torch.Tensor):
    """The only collective of the path: token ids + log-probs of every rank to rank 0 in ONE gather
    (replaces the shared-filesystem poll/concat of reference inference.py:214-225).  The fp32 log-probs
    ride along bit-cast into an extra int64 column, so a batch costs a single ~10 KB RCCL call."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return tokens, logprobs
    world, rank = dist.get_world_size(), dist.get_rank()
    lp_bits = logprobs.float().contiguous().view(torch.int32).to(torch.int64)
    packed = torch.cat([tokens, lp_bits[:, None]], dim=1).contiguous()
    out = [torch.empty_like(packed) for _ in range(world)] if rank == 0 else None
    dist.gather(packed, out, dst=0)
    if rank != 0:
        return None, None
    allp = torch.cat(out, 0)
    return allp[:, :-1].contiguous(), allp[:, -1].to(torch.int32).view(torch.float32)


def dump_outputs(out_dir: str, tokens: torch.Tensor, logprobs: torch.Tensor, info: torch.Tensor) -> None:
    """--dump-outputs: what the caller of the timed path received from its last step (N > 1: the rows of every rank, as
    gathered to rank 0), so that two builds can be compared output for output.  Ids and info are exact in float64; the
    whole set is a few KB per 64 images."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "tokens.npy"), tokens.cpu().numpy().astype(np.float64))
    np.save(os.path.join(out_dir, "logprobs.npy"), logprobs.float().cpu().numpy())
    np.save(os.path.join(out_dir, "info.npy"), info.cpu().numpy().astype(np.float64))


def _cpu_run(sample_batch: int, max_steps: int, threads: int):
    """One timed pass of the CPU port: GIT_BASE fp32, greedy, full recompute per step (the reference's semantics)."""
    from oracle import git_oracle as O
    torch.set_num_threads(threads)
    cfg = O.CONFIGS["GIT_BASE"]
    w = O.make_weights(cfg, seed=1234)
    frames = O.make_images(cfg, sample_batch, 1, seed=0)
    search = O.SearchConfig("greedy", max_steps, 1, 1)
    t0 = time.time()
    with torch.no_grad():
        feats = O.visual_features(cfg, w, frames)
        t1 = time.time()
        out = O.caption(cfg, w, frames, search, cached=False, feats=feats)
    dt = time.time() - t0
    return {"captions_per_s": sample_batch / dt, "wall_s": dt, "vit_s": t1 - t0, "decode_s": dt - (t1 - t0),
            "steps": int(out["predictions"].shape[1] - 1)}


def cpu_baseline(sample_batch: int, max_steps: int, threads: int = 0, repeats: int = 3, big_batch: int = 0):
    """Reference algorithm on the host cores (SURVEY.md 8d protocol): the oracle (a PORT of the reference: fp32, full
    recompute per step exactly like CaptioningModel.infer as shipped), greedy, GIT_BASE; one warm-up pass, then the
    MEDIAN of `repeats` passes at bs = sample_batch (default 8: ~15 s of CPU work in all), thread count pinned and
    reported; `--cpu-big-batch 64` adds ONE pass at bs = 64 (75 s on the GPU box's host: 0.85 captions/s,
    profiles/r03_a_bench.json).  torch's CPU kernels oversubscribe badly on a 256-thread host (measured 85x slower than 16 threads), so
    the thread count is capped; `python bench.py --cpu-sweep` measures other counts (profiles/r02_d_cpu_sweep.json).
    /root/reference does not exist on the GPU box, so the reference modules themselves cannot be timed there:
    kind = "port"."""
    cores = os.cpu_count() or 1
    try:
        from generativeimage2text_amd.inference import effective_cpus
        usable = effective_cpus()                        # affinity mask capped by the cgroup CPU quota
    except Exception:
        usable = cores
    threads = threads or min(cores, 16)
    _cpu_run(min(2, sample_batch), max_steps, threads)                    # warm-up (thread pool, allocator, first-touch)
    runs = [_cpu_run(sample_batch, max_steps, threads) for _ in range(max(1, repeats))]
    med = sorted(runs, key=lambda r: r["captions_per_s"])[len(runs) // 2]
    out = {"value": round(med["captions_per_s"], 4), "unit": "captions/s", "cores": threads, "kind": "port",
           "threads_note": "16 threads is the FASTEST setting of the sweep on the GPU box's 256-thread host (profiles/r02_d_cpu_sweep.json: "
                           "16 / 32 / 64 / 128 threads) -- the box's container has a cgroup CPU quota of 16 cores (host_cpus_usable; "
                           "cpu.max = 1600000 100000, found in round 6), so 16 threads is every core this process may use",
           "host_cpus": cores, "host_cpus_usable": usable, "vit_s": round(med["vit_s"], 2), "decode_s": round(med["decode_s"], 2),
           "runs": [round(r["captions_per_s"], 4) for r in runs],
           "sample": f"GIT_BASE fp32 bs={sample_batch} greedy {med['steps']} decode steps, full recompute per step "
                     f"(reference semantics): median of {len(runs)} passes after one warm-up, {med['wall_s']:.1f}s each on "
                     f"{threads} threads (the fastest thread count of the sweep in profiles/r02_d_cpu_sweep.json)"}
    # how representative the port is: measured once where /root/reference is importable (oracle/time_port_vs_reference.py,
    # same weights / images / threads / batch: the unmodified reference modules against the port, ids equal)
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle", "port_vs_reference.json")) as f:
            pr = json.load(f)
        out["port_vs_reference_ratio"] = pr["port_vs_reference_ratio"]
        # EXTRAPOLATED: this host's port figure / a ratio stored in oracle/port_vs_reference.json (measured on another host)
        out["reference_estimate"] = {"value": round(out["value"] / pr["port_vs_reference_ratio"], 4),
                                     "how": "this run's port value / the stored ratio (not a measurement of this host)",
                                     "ratio_measured_on": {"host_cpus": pr.get("host_cpus"), "threads": pr.get("threads"),
                                                           "batch": pr.get("batch")}}
        out["sample"] += (f"; the port runs at {pr['port_vs_reference_ratio']:.2f} x the speed of the reference's own modules "
                          f"(bs={pr['batch']}, {pr['threads']} threads, measured where /root/reference exists: "
                          f"{pr['port_s']} s vs {pr['reference_s']} s)")
    except (OSError, KeyError, ValueError):
        pass
    out["bs64_note_historical"] = ("NOT measured in this run: the GPU workload's own batch (bs = 64) is behind --cpu-big-batch 64 (one "
                                   "pass = 75 s); round 3 measured 0.85 captions/s on a GPU-box host (profiles/r03_a_bench.json), and "
                                   "in the build container the reference's modules took 59.4 s against the port's 61.8 s at bs = 64")
    if big_batch and big_batch != sample_batch:
        big = _cpu_run(big_batch, max_steps, threads)
        out["bs%d" % big_batch] = {"value": round(big["captions_per_s"], 4), "vit_s": round(big["vit_s"], 2),
                                   "decode_s": round(big["decode_s"], 2), "wall_s": round(big["wall_s"], 1)}
    return out


def csrc_sha() -> str:
    import glob, hashlib
    h = hashlib.sha1()
    for f in sorted(glob.glob(os.path.join(ROOT, "generativeimage2text_amd", "csrc", "*.hip")) +
                    glob.glob(os.path.join(ROOT, "generativeimage2text_amd", "csrc", "*.h"))):
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def pmc_profile(kernel_substrs):
    """Counter figures of the named kernels from the newest committed rocprofv3 --pmc summary
    (profiles/*pmc_summary.tsv, tools/gpu_pmc.sh + tools/pmc_summary.py: FETCH_SIZE / WRITE_SIZE / SQ / GRBM groups in
    separate passes; HBM bytes = 2*FETCH_SIZE + WRITE_SIZE as MI355X_MICROARCH.md prescribes for gfx950).
    PMC counters cannot be collected from inside this process, so the figures are the profiled ones; `stale` says
    whether the kernels' sources changed since that profile (hash of csrc/ recorded in its header)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_summary.tsv")))
    if not files:
        return None

    def sha_of(f):
        with open(f) as fh:
            return next((l.split("=", 1)[1].strip() for l in fh if l.startswith("# csrc_sha=")), None)
    # the summary taken for THIS csrc/ if there is one, else the last by name (reported as stale)
    cur = csrc_sha()
    files = [f for f in files if sha_of(f) == cur][-1:] or files
    lines = open(files[-1]).read().splitlines()
    sha = next((l.split("=", 1)[1].strip() for l in lines if l.startswith("# csrc_sha=")), None)
    rows = [l.split("\t") for l in lines if not l.startswith("#")]
    hdr = rows[0]
    out = {"source": os.path.relpath(files[-1], ROOT), "stale": sha != csrc_sha()}
    for key, sub in kernel_substrs.items():
        acc, n = {}, 0.0
        for r in rows[1:]:
            if sub not in r[0]:
                continue
            d = {h: float(v) for h, v in zip(hdr[1:], r[1:]) if v != "-"}
            wgt = d.get("DISPATCHES", 1.0)
            n += wgt
            for h in ("HBM_BYTES", "MFMA_UTIL_PCT", "L2_HIT_PCT"):
                if h in d:
                    acc[h] = acc.get(h, 0.0) + wgt * d[h]
        if n:
            out[key] = {h.lower(): round(v / n, 2) for h, v in acc.items()}
    return out


# workloads whose reference ids are frozen under tests/golden/ (oracle/make_golden.py FULL_CASES, generated from the
# unmodified reference modules): (model family, batch, search, max_steps, frames) -> (golden, weight seed of
# synthetic.random_state_dict; the frames are synthetic.random_frames(seed=0) in every case)
PARITY_GOLDENS = {
    ("GIT_BASE", 64, "greedy", 20, 1): ("full_bench_b64_greedy", 1234),
    ("GIT_BASE", 64, "beam", 20, 1): ("full_bench_b64_beam4", 1234),
    ("GIT_LARGE", 32, "greedy", 20, 1): ("full_large_b32_greedy", 1242),
    ("GIT_BASE_VATEX", 16, "greedy", 20, 6): ("full_vatex_b16_greedy", 1243),
}


def model_family(name: str) -> str:
    for fam in ("GIT_BASE_VATEX", "GIT_LARGE", "GIT_BASE"):
        if name.startswith(fam):
            return fam
    return name


def parity_golden(args):
    """(golden name, weight seed) of the workload, or (None, 1234) when no reference ids are frozen for it."""
    key = (model_family(args.model), args.batch, args.search, args.max_steps, args.frames)
    name, seed = PARITY_GOLDENS.get(key, (None, 1234))
    if name and not os.path.isfile(os.path.join(ROOT, "tests", "golden", name + ".npz")):
        name = None
    return name, seed


def bench_parity(eng, tokens, info, args):
    """Ids of the timed workload against the REFERENCE's ids for exactly this workload (tests/golden/full_*.npz:
    synthetic.random_state_dict(seed) weights, random_frames(seed=0), frozen from the unmodified reference modules by
    oracle/make_golden.py).  The tolerance is the specification's (tools/parity.py: logits within SPEC_LOGIT_FRAC = 1e-3 of the
    reference's logit span for the headline fp16 build, 2^3 x that for bf16; a row may leave the reference only at a decision
    whose fp32 margin is below 2 x the bound); the floor on identical rows is a regression guard; the counts go into the line."""
    import numpy as np
    name, _ = parity_golden(args)
    if name is None:
        return None
    from tools.parity import IDENTICAL_FLOORS, IDENTICAL_FLOORS_F16, ids_parity, logit_bound, margin_threshold
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    chained = args.search != "greedy"
    seq_len = int(info.tolist()[0])
    got = (tokens if chained else tokens[:, :seq_len]).cpu().numpy()
    lg = eng.step_logits(torch.from_numpy(g["tf_tokens"]))[:4, ::3].float().cpu().numpy()
    lerr = float(np.abs(lg - g["tf_logits"]).max())
    span = float(g["tf_logits"].max() - g["tf_logits"].min())
    f32, f16 = args.precision == "f32", args.precision == "f16"
    floor = got.shape[0] if f32 else (IDENTICAL_FLOORS_F16 if f16 else IDENTICAL_FLOORS).get(name)
    lbound = logit_bound(args.precision, span)
    # a one-beam row sees the reference's own tokens until its first divergence: within the logit bound, only a decision
    # whose fp32 margin is below 2 x bound can flip (parity.margin_threshold)
    thr = 1e-6 if f32 else margin_threshold(args.precision, lbound, chained)
    try:
        st = ids_parity(got, g["predictions"], g["step_margin"], thr, chained=chained, min_identical=floor)
        st["ok"] = bool(lerr < lbound)
        if not st["ok"]:
            st["violation"] = f"logit error {lerr:.5f} above the bound {lbound:.5f}"
    except AssertionError as exc:
        st = {"ok": False, "violation": str(exc)[:200]}
    st["logit_err"] = round(lerr, 5)
    st["logit_span"] = round(span, 3)
    st["logit_err_frac_of_span"] = round(lerr / span, 6)       # north_star's "logits within 1e-3", read relative to the span
    st["logit_err_bound"] = round(lbound, 5)
    st["identical_floor"] = floor                               # regression guard, not a tolerance (tools/parity.py)
    st["reference"] = f"tests/golden/{name}.npz"
    if not chained and not getattr(args, "no_teacher_forced", False):
        from generativeimage2text_amd.configs import config_for_model
        from generativeimage2text_amd.synthetic import random_frames, random_state_dict
        cfg = config_for_model(args.model)
        st["teacher_forced"] = bench_teacher_forced(
            eng, name, g, args, cfg, lambda: random_state_dict(cfg, seed=parity_golden(args)[1]),
            random_frames(cfg, args.batch, args.frames, seed=0))
        if st.get("teacher_forced") is not None and not st["teacher_forced"]["ok"]:
            st["ok"] = False
            st.setdefault("violation", "teacher_forced: " + st["teacher_forced"].get("violation", ""))
    return st


def bench_teacher_forced(eng, name, g, args, cfg, weights, frames):
    """EVERY decision of every row against the reference (tools/parity.teacher_forced_parity): the engine is fed the
    reference's own ids[:, :t], t = 1 .. L-1, through gitmi_step_logits; the argmax after the no-repeat rule must be the
    reference's id wherever its fp32 margin is >= 2 x the specification's logit bound, and the logit error is taken over every
    row x every vocabulary column x every decision (against an f32-mode engine built here on the same weights and images,
    itself held to 1e-4 of the frozen reference logits of tests/golden/<case>_tf.npz).  weights: callable -> state dict."""
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", name + "_tf.npz")
    if not os.path.isfile(path):
        return None
    from generativeimage2text_amd.engine import Engine
    from tools.parity import teacher_forced_parity, tf_bounds
    gt = np.load(path)
    span = float(gt["logit_max"]) - float(gt["logit_min"])
    b = tf_bounds(args.precision, span)
    B, F = int(frames[0].shape[0]), len(frames)
    f32_logits = None
    e32 = None
    if args.precision != "f32":
        e32 = Engine(cfg, precision="f32", max_batch=B, max_beams=1, max_frames=max(1, F), max_text_len=args.max_steps)
        e32.load_state_dict(weights())
        e32.encode(frames, return_features=False)
        f32_logits = e32.step_logits
    try:
        eng.encode(frames, return_features=False)
        st = teacher_forced_parity(eng.step_logits, g["predictions"], gt, cfg.eos, b["thr"], b["lerr"], f32_step_logits=f32_logits)
    finally:
        if e32 is not None:
            e32.close()
    st["reference"] = f"tests/golden/{name}_tf.npz"
    st["spec_logit_frac"] = b["lerr"] / span
    return st


def bench_trained_statistics(args, cfg, device):
    """Second parity leg of the line: the SAME geometry with the statistics of a trained checkpoint --
    synthetic.random_state_dict(stats="trained"): LayerNorm gains over [0.2, 5], biases of order 1, three residual channels of
    the image encoder 100x / 300x / 1000x above the rest -- on 64 images whose every fp32 decision margin is >= 0.03 = 2 x the
    specification's logit tolerance (tests/golden/full_trained_b64_greedy.npz + _tf.npz, frozen from the unmodified reference by
    oracle/make_golden.py).  In this run's precision: free-running ids (every row REQUIRED when 2 x the build's logit bound is
    below the margins: f32 and the fp16 headline build) and the teacher-forced logit error over every logit."""
    import ast
    import numpy as np
    name = "full_trained_b64_greedy"
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    if (model_family(args.model), args.batch, max(1, args.frames), args.search, args.max_steps) != ("GIT_BASE", 64, 1, "greedy", 20) \
            or not os.path.exists(path):
        return None
    from generativeimage2text_amd.engine import Engine
    from generativeimage2text_amd.synthetic import random_state_dict, seeded_images
    from tools.parity import identity_required, logit_bound
    g = np.load(path)
    wsrc = ast.literal_eval(str(g["weights"]))              # ("trained", seed, eos_bias, successor)
    weights = lambda: random_state_dict(cfg, seed=wsrc[1], eos_bias=wsrc[2], successor=wsrc[3], stats="trained")
    frames = seeded_images(cfg, g["image_seeds"].tolist(), device=device)
    eng = Engine(cfg, precision=args.precision, max_batch=args.batch, max_beams=1, max_frames=1, max_text_len=20)
    try:
        eng.load_state_dict(weights())
        tokens, lps, info = eng.generate(frames, Engine.make_search("greedy", 20, 1, 1), sync=True)
        got = tokens[:, :int(info.tolist()[0])].cpu().numpy()
        ref = g["predictions"]
        same = int(sum(1 for r in range(ref.shape[0]) if got.shape == ref.shape and (got[r] == ref[r]).all()))
        tf = bench_teacher_forced(eng, name, g, args, cfg, weights, frames)
    finally:
        eng.close()
    span = tf["logit_span"] if tf else float(g["tf_logits"].max() - g["tf_logits"].min())
    min_margin = float(g["step_margin"].min())
    must = identity_required(args.precision, span, min_margin)
    out = {"reference": f"tests/golden/{name}.npz", "rows": int(ref.shape[0]), "identical": same,
           "required": int(ref.shape[0]) if must else None, "min_reference_margin": round(min_margin, 4),
           "finite": bool(torch.isfinite(lps).all().item()), "logit_err_bound": round(logit_bound(args.precision, span), 5),
           "teacher_forced": tf}
    out["ok"] = bool(out["finite"] and (not must or same == ref.shape[0]) and (tf is None or tf["ok"]))
    return out


def child_line(argv_child, timeout_s=150):
    """One `python bench.py ... --full --brief` child on this (now idle) GPU -> its parsed JSON line, or {"error": ...}.  Short
    timeout: the headline line must not die with a side measurement."""
    cmd = [sys.executable, os.path.abspath(__file__)] + argv_child
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        return json.loads(line)
    except Exception as exc:
        return {"error": f"{type(exc).__name__}: {exc}"[:300]}


def alt_precision_line(argv_child):
    """The OTHER 16-bit operand build (headline fp16 -> libgitmi.so with bf16 operands, BASELINE.json's named precision; the
    same kernels at the same MFMA rate, 3 fewer mantissa bits per operand) on the SAME workload and schedule, run as a child
    `python bench.py --precision bf16 --full --brief` after this process has gone idle: captions/s of a short timed loop and the same
    `parity` object, so the default line carries both builds."""
    c = child_line(argv_child)
    if "error" in c:
        return c
    return {"precision": c["dtype"], "library": c["config"]["library"], "captions_per_s": c["value"],
            "ms_per_step": c["ms_per_step"], "steps": c["steps"], "parity": c.get("parity"),
            "timed_ids_equal_solo": c.get("timed_ids_equal_solo")}


# the other BASELINE.json configurations that fit one GPU (configs[2], [3] per GPU, [4]); the default line runs each as a
# short --full --brief child after its own timed region so that the driver's record carries all four workloads
OTHER_CONFIGS = {
    "cfg3_base_b64_beam4": ["--model", "GIT_BASE", "--batch", "64", "--search", "beam"],
    "cfg4_large_b32_greedy": ["--model", "GIT_LARGE", "--batch", "32"],
    "cfg5_vatex_b16_6frames": ["--model", "GIT_BASE_VATEX", "--batch", "16", "--frames", "6"],
}


def other_configs_lines(args):
    out = {}
    for key, wl in OTHER_CONFIGS.items():
        c = child_line(wl + ["--precision", args.precision, "--brief", "--full", "--no-cpu-baseline", "--no-teacher-forced",
                             "--steps", str(args.steps), "--warmup", str(args.warmup)])
        if "error" in c:
            out[key] = c
            continue
        par = c.get("parity") or {}
        out[key] = {"workload": c["config"]["workload"], "captions_per_s": c["value"], "ms_per_step": c["ms_per_step"],
                    "steps": c["steps"], "decode_step_ms": (c.get("roofline_decode") or {}).get("avg_step_ms"),
                    "parity": {k: par.get(k) for k in ("ok", "rows", "identical", "identical_floor", "logit_err_frac_of_span",
                                                       "logit_err_bound", "reference") if k in par},
                    "wide_margin": {k: (par.get("wide_margin") or {}).get(k) for k in ("identical", "required", "ok")}
                    if par.get("wide_margin") else None}
    return out


def bench_wide_margin(args, cfg, device):
    """north_star: "greedy outputs bit-identical to reference token IDs".  On the benchmark's own random-init weights every
    row has a top-1 / top-2 near-tie somewhere in its 19 steps, so that clause is undecidable for a 16-bit pipeline (`parity`
    above reports the count and the floor).  tests/golden/full_wide_b64_*.npz is the same geometry in the regime where it IS
    decidable (the benchmark's weight family + a successor structure, 64 images on which every greedy decision of the fp32
    reference has a margin >= 0.2; frozen from the unmodified reference by oracle/make_golden.py): the engine must return
    the reference's ids on EVERY row.  One solo pass in this run's precision and search, outside the timed region."""
    import numpy as np
    name = {("GIT_BASE", 64, 1, "greedy"): "full_wide_b64_greedy", ("GIT_BASE", 64, 1, "beam"): "full_wide_b64_beam4",
            ("GIT_LARGE", 32, 1, "greedy"): "full_wide_large_b32_greedy",
            ("GIT_BASE_VATEX", 16, 6, "greedy"): "full_wide_vatex_b16_greedy"}.get(
        (model_family(args.model), args.batch, max(1, args.frames), args.search))
    if name is None or args.max_steps != 20:
        return None
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    if not os.path.exists(path):
        return None
    from generativeimage2text_amd.engine import Engine
    from generativeimage2text_amd.synthetic import random_state_dict, seeded_images
    g = np.load(path)
    import ast
    wsrc = ast.literal_eval(str(g["weights"]))              # ("wide", seed, eos_bias, successor[, images of])
    beams = 1 if args.search == "greedy" else 4
    F = max(1, args.frames)
    eng = Engine(cfg, precision=args.precision, max_batch=args.batch, max_beams=beams, max_frames=F, max_text_len=20)
    try:
        eng.load_state_dict(random_state_dict(cfg, seed=wsrc[1], eos_bias=wsrc[2], successor=wsrc[3]))
        search = Engine.make_search("greedy", 20, 1, 1) if beams == 1 else Engine.make_search("beam", 20, 4, 2, 0.6)
        tokens, _, info = eng.generate(seeded_images(cfg, g["image_seeds"].tolist(), device=device, frames=F), search, sync=True)
    finally:
        eng.close()
    got = (tokens if beams > 1 else tokens[:, :int(info.tolist()[0])]).cpu().numpy()
    ref = g["predictions"]
    same = int(sum(1 for r in range(ref.shape[0]) if got.shape == ref.shape and (got[r] == ref[r]).all()))
    from tools.parity import WIDE_BEAM_FLOOR
    need = int(ref.shape[0]) if (beams == 1 or args.precision == "f32") else WIDE_BEAM_FLOOR      # beam search: no margin certificate
    return {"reference": f"tests/golden/{name}.npz", "rows": int(ref.shape[0]), "identical": same,
            "required": need, "ok": same >= need,
            "min_reference_margin": round(float(g["step_margin"].min()), 4) if beams == 1 else None}


class _HostDev:
    """Stand-in for the torch.cuda stream / event calls of main(): lets the rank logic of this file (environment, process
    group, sharding, gather, MAX-over-ranks timing, the JSON line) run under gloo on the CPU with a stand-in engine
    (tests/test_dist_cpu.py).  Never used on a GPU box."""

    class Stream:
        def wait_event(self, ev):
            pass

    class Event:
        def __init__(self, enable_timing=False):
            self.t = None

        def record(self):
            self.t = time.perf_counter()

        def synchronize(self):
            pass

        def elapsed_time(self, other):
            return (other.t - self.t) * 1e3

    @staticmethod
    def stream(s):
        return contextlib.nullcontext()

    @staticmethod
    def synchronize():
        pass


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(gpus: int, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks here (one process per GPU, RCCL over xGMI) through
    torch.distributed.run, exactly as the driver would, and hand its exit code back."""
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < gpus:
        raise SystemExit(f"bench.py --gpus {gpus}: only {have} GPU(s) visible on this node; refusing to print a line for "
                         f"fewer GPUs than asked for")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


def main(argv=None, engine_factory=None):
    """engine_factory (tests only): callable(args, rank) -> (engine, frames) standing in for the HIP engine, which makes
    the rank logic below run on the CPU under gloo (tests/test_dist_cpu.py); everything device-specific then goes through
    _HostDev instead of torch.cuda."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--model", default="GIT_BASE")
    ap.add_argument("--search", default="greedy", choices=["greedy", "beam"])
    ap.add_argument("--max-steps", type=int, default=20)
    ap.add_argument("--precision", default="f16", choices=["bf16", "f16", "f32"],
                    help="f16 (headline since round 6): the kernels built for fp16 operands (libgitmi_f16.so) -- the 16-bit build "
                         "that meets north_star's logit clause (1e-3 of the logit span) on every weight family; bf16: the same kernels "
                         "with BASELINE.json's named operand format (same MFMA rate, 3 fewer mantissa bits: 5e-3 of the span on "
                         "trained-like weights), reported beside the headline as alt_precision; f32: parity mode")
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=8,
                    help="batch size of the CPU baseline's median-of-3 passes (one bs=64 pass is timed besides)")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--cpu-big-batch", type=int, default=0, help="also time ONE CPU pass at this batch size (64: ~75 s)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-ln-fold", action="store_true",
                    help="A/B (f16 build): one LayerNorm launch per module in the encoder / prefill instead of the folded GEMM epilogues")
    ap.add_argument("--contexts", type=int, default=4,
                    help="engine contexts (shared weights) kept in flight on separate HIP streams")
    ap.add_argument("--free-run", action="store_true", help="do not chain the contexts' image encoders at all")
    ap.add_argument("--solo-policy", action="store_true",
                    help="A/B: keep the kernel shapes of a context that has the device to itself (no gitmi_set_shared_device)")
    ap.add_argument("--encoder-chains", type=int, default=2,
                    help="image encoders of the contexts in flight are chained (context i starts its encoder after "
                         "context i - chains has finished its own): at most this many encoders run at a time")
    ap.add_argument("--coalesce", type=int, default=1,
                    help="N > 1: N requests of --batch images are served by ONE engine pass over N x batch rows "
                         "(Engine.generate_coalesced; the concatenation is inside the timed region).  A step is still one "
                         "request of --batch images; the default 1 is the BASELINE configuration (one pass per request)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, everything besides the headline figure: roofline passes, parity legs, the "
                         "alt_precision and other_configs children, the CPU baseline, the gather figures for N > 1")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the ids, log-probs and info of the last timed step to DIR/{tokens,logprobs,info}.npy")
    ap.add_argument("--brief", action="store_true",
                    help="with --full: timed loop + parity only, no roofline passes, no CPU baseline (what the alt_precision "
                         "and other_configs children run)")
    ap.add_argument("--no-teacher-forced", action="store_true",
                    help="skip parity.teacher_forced (its f32-mode engine adds ~2 300 fp32 launches to a kernel trace of the run)")
    ap.add_argument("--no-alt-precision", action="store_true",
                    help="skip the child run of the bf16-operand build that the default line reports as alt_precision")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short child runs of BASELINE.json configs[2..4] that the default line reports as other_configs")
    ap.add_argument("--e2e-tsv", type=int, default=0, metavar="N",
                    help="instead of the benchmark: N synthetic 640x480 JPEG rows -> test_git_inference_single_tsv -> TSV, one JSON "
                         "line with end-to-end captions/s, host threads and GPU-busy fraction (tools/e2e_tsv.py)")
    ap.add_argument("--experiment", action="store_true",
                    help="A/B harness only: load libgitmi_exp.so (the bf16 build with -DGITMI_EXPERIMENT), whose engine reads "
                         "kernel-shape overrides from GITMI_* environment variables; the line says so in config.library")
    ap.add_argument("--cpu-sweep", action="store_true",
                    help="only time the CPU port at several thread counts (median of 3, bs=8) and print JSON")
    args = ap.parse_args(argv)
    if args.brief and not args.full:
        ap.error("--brief narrows what --full adds: give both")
    if args.e2e_tsv:
        from tools.e2e_tsv import main as e2e_main
        e2e_main(["--rows", str(args.e2e_tsv), "--precision", args.precision, "--batch", str(args.batch),
                  "--contexts", str(args.contexts)])
        return
    if args.cpu_sweep:
        res = []
        for th in (16, 32, 64, 128):
            res.append(cpu_baseline(8, args.max_steps, th, repeats=3, big_batch=0))
        print(json.dumps({"cpu_sweep": res, "host_cpus": os.cpu_count()}), flush=True)
        return

    standin = engine_factory is not None
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        if standin:
            raise SystemExit("bench.main: the stand-in run takes RANK / WORLD_SIZE from the environment")
        self_launch(args.gpus, sys.argv[1:] if argv is None else argv)          # does not return
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report n_gpus != --gpus")
    if not standin:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X; there is no CPU path to benchmark")
        if torch.cuda.device_count() <= local_rank:
            raise SystemExit(f"rank {rank}: LOCAL_RANK={local_rank} but only {torch.cuda.device_count()} GPU(s) visible")
        torch.cuda.set_device(local_rank)
    dev = _HostDev if standin else torch.cuda
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if standin else "nccl")     # "nccl" is RCCL on ROCm
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"process group has {dist.get_world_size()} ranks, --gpus {args.gpus}")

    from generativeimage2text_amd.configs import config_for_model
    from generativeimage2text_amd.engine import Engine
    from generativeimage2text_amd.synthetic import random_state_dict, random_frames

    if os.environ.get("BENCH_GEMM_IMPL") and not args.experiment and not standin:
        raise SystemExit("BENCH_GEMM_IMPL is a switch of the measurement build: add --experiment")
    if args.experiment:
        from generativeimage2text_amd.engine import use_experiment_build
        use_experiment_build(True)
    cfg = config_for_model(args.model)
    beams = 1 if args.search == "greedy" else 4
    coalesce = max(1, args.coalesce)
    if args.steps % coalesce:
        raise SystemExit(f"--steps {args.steps} is not a multiple of --coalesce {coalesce} (a partial pass would re-capture "
                         f"the context's hipGraph inside the timed region)")
    args.warmup = (args.warmup + coalesce - 1) // coalesce * coalesce        # whole passes only, for the same reason
    golden_name, weight_seed = parity_golden(args)
    if standin:
        eng, frames = engine_factory(args, rank)
    else:
        eng = Engine(cfg, precision=args.precision, max_batch=args.batch * coalesce, max_beams=beams,
                     max_frames=max(1, args.frames), max_text_len=args.max_steps)
        # the weight seed is the one the workload's reference ids were frozen with (PARITY_GOLDENS), 1234 otherwise
        eng.load_state_dict(random_state_dict(cfg, seed=weight_seed))
        # rank r captions its own images (seed r): resident in HBM before timing
        frames = random_frames(cfg, args.batch, args.frames, seed=rank)
    if args.no_graph:
        eng.set_graph(False)
    if args.no_ln_fold and not standin:
        eng.set_ln_fold(False)                  # before cloning: the clones inherit it
    if os.environ.get("BENCH_GEMM_IMPL"):       # measurement build: A/B of GEMM variants in situ (tools/gpu_ab.sh)
        from generativeimage2text_amd.engine import set_gemm_impl
        set_gemm_impl(int(os.environ["BENCH_GEMM_IMPL"]))
    # several batches in flight: context i%C runs on its own stream, so the latency-bound decode steps of
    # one batch overlap the MFMA-bound encoder of the next (weights are shared, workspaces are not)
    if args.contexts > 1 and not args.solo_policy and not standin:
        eng.set_shared_device(True)             # before cloning: the clones inherit it
    ctxs = [eng] + [eng.clone() for _ in range(max(1, args.contexts) - 1)]
    for c in ctxs[1:]:
        if args.no_graph:
            c.set_graph(False)
    chains = max(1, args.encoder_chains)
    if len(ctxs) > chains and not args.free_run:
        # serving schedule: at most `chains` encoders of consecutive submissions in flight, decode chains float
        for i, c in enumerate(ctxs):
            c.set_encode_after(ctxs[i - chains])
    # one HIP stream per context.  (BENCH_STREAM_STRIDE: experiment knob -- take every n-th stream of a larger pool, to see
    # how the runtime's stream -> hardware-queue assignment affects the overlap of contexts)
    stride = int(os.environ.get("BENCH_STREAM_STRIDE", "1"))
    pool = [dev.Stream() for _ in range(len(ctxs) * stride)]
    streams = pool[::stride][:len(ctxs)]
    counter = [0]
    if args.search == "greedy":
        search = Engine.make_search("greedy", args.max_steps, 1, 1)
    else:
        search = Engine.make_search("beam", args.max_steps, 4, 2, 0.6)

    lat_events = []
    gather_events = []          # N > 1: events around the batch's ONE collective on its stream
    last_lp = [None]
    last_out = [None]           # (ids, log-probs, info) as the caller of the last step receives them (--dump-outputs)

    def step(record_latency=False):
        i = counter[0] % len(ctxs)
        counter[0] += 1
        with dev.stream(streams[i]):
            if record_latency:
                e0, e1 = dev.Event(enable_timing=True), dev.Event(enable_timing=True)
                e0.record()
            tokens, logprobs, info = ctxs[i].generate(frames, search, sync=False)
            last_lp[0] = logprobs
            last_out[0] = (tokens, logprobs, info)
            if world > 1:
                if record_latency:
                    g0, g1 = dev.Event(enable_timing=True), dev.Event(enable_timing=True)
                    g0.record()
                last_out[0] = gather_results(tokens, logprobs) + (info,)
                if record_latency:
                    g1.record()
                    gather_events.append((g0, g1))
            if record_latency:
                e1.record()
                lat_events.append((e0, e1))
        return tokens, info

    def fence():
        if world > 1:
            dist.barrier()
        dev.synchronize()

    def coalesced_pass(n, record_latency=False):
        """n requests of --batch images -> one engine pass on the next context"""
        i = counter[0] % len(ctxs)
        counter[0] += 1
        with dev.stream(streams[i]):
            if record_latency:
                e0, e1 = dev.Event(enable_timing=True), dev.Event(enable_timing=True)
                e0.record()
            outs, info = ctxs[i].generate_coalesced([frames] * n, search, sync=False)
            last_out[0] = outs[-1] + (info,)
            if world > 1:
                for tk, lp in outs:
                    last_out[0] = gather_results(tk, lp) + (info,)
            if record_latency:
                e1.record()
                lat_events.extend([(e0, e1)] * n)
        return outs[-1][0], info

    def run_steps(k, record_latency=False):
        out = None
        if coalesce > 1:
            done = 0
            while done < k:
                n = min(coalesce, k - done)
                out = coalesced_pass(n, record_latency)
                done += n
        else:
            for _ in range(k):
                out = step(record_latency)
        return out

    # every context captures its hipGraph before anything is timed (a context's first call captures and instantiates)
    run_steps(len(ctxs) * coalesce)
    fence()
    run_steps(args.warmup)
    fence()
    t0 = time.perf_counter()
    tokens, info = run_steps(args.steps, record_latency=True)
    fence()
    elapsed = time.perf_counter() - t0
    lat = sorted(a.elapsed_time(b) for a, b in lat_events)
    if world > 1:
        t = torch.tensor([elapsed], device="cpu" if standin else "cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, *last_out[0])

    # N > 1: what the one collective of the path costs ("report the gather latency separately") -- in the timed
    # schedule (device time between the events around it on the batch's stream: it queues behind the batch's decode chain
    # and waits for the slowest rank) and alone (one gather + stream synchronisation at a time, after the timed region)
    gather_stats = None
    if world > 1 and tokens is not None and args.full:
        g_in = sorted(a.elapsed_time(b) for a, b in gather_events)
        alone = []
        lp_probe = last_lp[0] if last_lp[0] is not None and last_lp[0].shape[0] == tokens.shape[0] else \
            torch.zeros(tokens.shape[0], device=tokens.device)
        for _ in range(20):
            t_g = time.perf_counter()
            gather_results(tokens, lp_probe)
            dev.synchronize()
            alone.append(1e3 * (time.perf_counter() - t_g))
        alone.sort()
        gather_stats = {"in_schedule_ms": {"median": round(g_in[len(g_in) // 2], 4), "max": round(g_in[-1], 4)} if g_in else None,
                        "alone_ms": {"median": round(alone[len(alone) // 2], 4), "max": round(alone[-1], 4)},
                        "bytes_per_rank": int(tokens.shape[0] * (tokens.shape[1] + 1) * 8),
                        "what": "ONE gather of int64 [B, max_len + 1] (ids + bit-cast log-probs) to rank 0 per batch"}

    # fixed-work check: no caption ended early (every caption ran max_steps-1 decode steps)
    info_h = info.tolist()
    steps_run = info_h[2]

    result = None
    if rank == 0:
        value = world * args.batch * args.steps / elapsed
        result = {
            "metric": "captions/sec whole-node (GIT_BASE 224px bs=64/GPU greedy len=20)",
            "value": round(value, 2), "unit": "captions/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.precision, "data": "synthetic (random-init weights, N(0,1) images resident in HBM)",
            "config": {"workload": f"{args.model} {cfg.image_size}px bs={args.batch}/GPU {args.search} "
                                   f"max_len={args.max_steps} frames={args.frames}",
                       "global_batch": world * args.batch, "parallelism": f"dp{world}",
                       "decode_steps_per_caption": steps_run, "seq_len_returned": info_h[0],
                       "hip_graph": not args.no_graph, "contexts_in_flight": len(ctxs),
                       "layernorm_folded": bool(args.precision == "f16" and not args.no_ln_fold and not args.experiment),
                       "library": ("libgitmi_exp.so (measurement build: " + " ".join(
                           f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("GITMI_")) + ")") if args.experiment
                       else {"bf16": "libgitmi.so", "f16": "libgitmi_f16.so"}.get(args.precision, "libgitmi.so"),
                       "shared_device_policy": bool(args.contexts > 1 and not args.solo_policy),
                       "encoder_chains": 0 if (args.free_run or len(ctxs) <= chains) else chains,
                       "schedule": (f"mixed, {coalesce} requests of {args.batch} images coalesced per engine pass" if coalesce > 1
                                    else "mixed")},
            # a batch's own latency (submit -> ids ready) while `contexts_in_flight` batches share the GPU
            "batch_latency_ms": {"median": round(lat[len(lat) // 2], 3), "max": round(lat[-1], 3)},
        }
        if gather_stats is not None:
            result["gather"] = gather_stats

    # ---- roofline passes: one context alone on rank 0's GPU after the timed region (N > 1: the other ranks wait at the final
    #      barrier, so every line -- 1, 2, 4, 8 GPUs -- carries `roofline` / `roofline_decode`) -----------------------------
    if rank == 0 and not standin and args.full and args.brief:
        # one context alone: the ids the parity legs compare, and the decode step of the production launch path
        eng.profile_enable(2)
        for it in range(4):
            tokens_solo, _, info_solo = eng.generate(frames, search, sync=True)
            if it == 0:
                eng.profile_read()
        bprof = eng.profile_read()
        eng.profile_enable(0)
        result["roofline_decode"] = {"avg_step_ms": round(bprof["decode_step_ms"], 4), "steps": bprof["decode_steps"],
                                     "bytes_per_step": bprof["decode_step_bytes"]}
    if rank == 0 and not standin and args.full and not args.brief:
        pmc = pmc_profile({"gemm": "gemm_p8", "attn_decode": "attn_decode", "dgemm": "dgemm_kernel", "vocab": "vocab_topm"})
        # (1) eager launches, HIP events around every GEMM launch on the launch stream: per-kernel durations
        eng.profile_enable(1)
        for _ in range(2):
            eng.generate(frames, search, sync=True)
            prof = eng.profile_read()
        # (2) the production launch path: hipGraph replays of one context alone, split into an (encode + prefill)
        #     graph and a decode graph with HIP events between them
        eng.profile_enable(2)
        for it in range(6):
            tokens_solo, _, info_solo = eng.generate(frames, search, sync=True)
            if it == 0:
                eng.profile_read()          # drop the capture + first replay
        gprof = eng.profile_read()
        eng.profile_enable(0)
        n = max(1, prof["vit_gemm_launches"])
        flops_per_launch = prof["vit_gemm_flops"] / n
        avg_ms_raw = prof["vit_gemm_ms"] / n
        # what an event pair costs by itself on this stream (nothing between the two records): the eager pass brackets every
        # launch with such a pair, so a launch's raw figure = that overhead + dispatch latency + the kernel
        ev_over = []
        for _ in range(64):
            a_, b_ = dev.Event(enable_timing=True), dev.Event(enable_timing=True)
            a_.record()
            b_.record()
            b_.synchronize()
            ev_over.append(a_.elapsed_time(b_))
        ev_over_ms = sorted(ev_over)[len(ev_over) // 2]
        # net of that overhead: with it removed the figure agrees with the kernel's own duration in a rocprofv3 kernel trace
        # (profiles/r05_e_*: 49.8 us net against 49.6 us traced; raw 54.2 us)
        avg_ms = max(avg_ms_raw - ev_over_ms, 1e-6)
        achieved_raw = flops_per_launch / (avg_ms_raw * 1e-3) / 1e12 if avg_ms_raw > 0 else 0.0
        achieved = flops_per_launch / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
        result["roofline"] = {
            "kernel": f"gitmi::gemm_p8_kernel <{args.precision} operands> (the 49 image-encoder GEMM launches)"
                      if args.precision != "f32" else "gitmi::gemm_kernel<f32>",
            "bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": None,
            "launches_per_step": prof["vit_gemm_launches"], "avg_launch_ms": round(avg_ms, 4),
            "avg_launch_ms_raw": round(avg_ms_raw, 4), "empty_event_pair_ms": round(ev_over_ms, 5),
            "frac_raw": round(achieved_raw / PEAK_BF16_TFLOPS, 4),
            "flops_per_launch": flops_per_launch,
            "method": "HIP events around each launch on the launch stream, eager (no graph) pass after the timed region; "
                      "avg_launch_ms = the raw event-to-event time (avg_launch_ms_raw) minus what an event pair with nothing "
                      "between its records measures on the same stream (empty_event_pair_ms, median of 64); frac_raw = without "
                      "that correction",
        }
        # (no figures here: a pointer.  The kernel's K loop is power-limited on N(0,1) operands -- identical cycle counts, lower clock --
        # so `frac` is priced against a peak this instruction mix cannot draw the power for; the measurement is a standalone probe)
        result["roofline"]["ceiling_evidence"] = "tools/probe/gemm_probe.hip -> profiles/r05_b_*, r05_h_gemm_power_ab.txt, r05_t_bench_socket_power.txt"
        if pmc and "gemm" in pmc:
            result["roofline"]["traffic"] = round(pmc["gemm"].get("hbm_bytes", 0)) or None
            result["roofline"]["mfma_busy_pct"] = pmc["gemm"].get("mfma_util_pct")
            result["roofline"]["l2_hit_pct"] = pmc["gemm"].get("l2_hit_pct")
            result["roofline"]["traffic_source"] = pmc["source"]
            result["roofline"]["traffic_stale"] = pmc["stale"]
        step_ms = gprof["decode_step_ms"]
        step_gbs = gprof["decode_step_bytes"] / (step_ms * 1e-3) / 1e9 if step_ms > 0 else 0.0
        result["roofline_decode"] = {
            "bound": "hbm", "achieved": round(step_gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(step_gbs / PEAK_HBM_GBS, 4), "traffic": None,
            "bytes_per_step": gprof["decode_step_bytes"], "avg_step_ms": round(step_ms, 4),
            "steps": gprof["decode_steps"], "eager_step_ms": round(prof["decode_step_ms"], 4),
            "method": "HIP events around the decode hipGraph of one context (production launch path), averaged over "
                      "5 replays; eager_step_ms = the same step with one host launch per kernel",
        }
        if result["config"].get("shared_device_policy"):
            # the same two measurements with the kernel shapes a context picks when it has the device to itself
            # (gitmi_set_shared_device off): what the serving policy trades away per launch for the whole-device rate
            solo = eng.clone()
            solo.set_shared_device(False)
            solo.profile_enable(1)
            for _ in range(2):
                solo.generate(frames, search, sync=True)
                sprof = solo.profile_read()
            solo.profile_enable(2)
            for it in range(6):
                solo.generate(frames, search, sync=True)
                if it == 0:
                    solo.profile_read()
            sgprof = solo.profile_read()
            solo.profile_enable(0)
            solo.close()
            s_raw = sprof["vit_gemm_ms"] / max(1, sprof["vit_gemm_launches"])
            s_ms = max(s_raw - ev_over_ms, 1e-6)
            s_tf = flops_per_launch / (s_ms * 1e-3) / 1e12 if s_ms > 0 else 0.0
            result["roofline"]["solo_policy"] = {"avg_launch_ms": round(s_ms, 4), "avg_launch_ms_raw": round(s_raw, 4),
                                                 "achieved": round(s_tf, 2), "frac": round(s_tf / PEAK_BF16_TFLOPS, 4)}
            ss_ms = sgprof["decode_step_ms"]
            ss_gbs = sgprof["decode_step_bytes"] / (ss_ms * 1e-3) / 1e9 if ss_ms > 0 else 0.0
            result["roofline_decode"]["solo_policy"] = {"avg_step_ms": round(ss_ms, 4), "achieved": round(ss_gbs, 1),
                                                        "frac": round(ss_gbs / PEAK_HBM_GBS, 4)}
        if pmc:
            per_step = 0.0
            for key, launches in (("dgemm", 4 * cfg.dec_layers), ("attn_decode", cfg.dec_layers), ("vocab", 1)):
                if key in pmc and "hbm_bytes" in pmc[key]:
                    per_step += launches * pmc[key]["hbm_bytes"]
            if per_step > 0:
                result["roofline_decode"]["traffic"] = round(per_step)
                result["roofline_decode"]["traffic_source"] = pmc["source"]
                result["roofline_decode"]["traffic_stale"] = pmc["stale"]
        result["phases_ms"] = {k: round(prof[k], 3) for k in ("vit_ms", "prefill_ms", "decode_ms", "total_ms", "gemm_ms")}
        result["phases_ms"]["graph_encode_prefill_ms"] = round(gprof["vit_ms"], 3)
        result["phases_ms"]["graph_decode_ms"] = round(gprof["decode_ms"], 3)
    if rank == 0 and not standin and args.full:
        # the ids of the timed schedule's last batch are the ids of the solo pass (same images, same weights)
        result["timed_ids_equal_solo"] = bool(torch.equal(tokens.cpu(), tokens_solo.cpu()))
        result["nonfinite_sequences"] = int(info.tolist()[3]) + int(info_solo.tolist()[3])
        result["parity"] = bench_parity(eng, tokens_solo, info_solo, args)
        if result["parity"] is not None:
            result["parity"]["wide_margin"] = bench_wide_margin(args, cfg, frames[0].device)
            if not args.no_teacher_forced:
                result["parity"]["trained_statistics"] = bench_trained_statistics(args, cfg, frames[0].device)
            for leg in ("wide_margin", "trained_statistics"):
                if result["parity"].get(leg) is not None and not result["parity"][leg]["ok"]:
                    result["parity"]["ok"] = False
                    result["parity"].setdefault("violation", leg + " leg failed")
            if result["nonfinite_sequences"]:
                result["parity"]["ok"] = False
                result["parity"].setdefault("violation", "non-finite log-probabilities in the timed run")
    if rank == 0 and world == 1 and not standin and args.full and not args.brief:
        if (args.precision in ("f16", "bf16") and not args.no_alt_precision and not args.experiment and coalesce == 1
                and golden_name is not None):
            # the other 16-bit operand build on the same workload and schedule, in a child process, with this process idle
            dev.synchronize()
            other = "bf16" if args.precision == "f16" else "f16"
            child = ["--precision", other, "--brief", "--full", "--no-cpu-baseline", "--steps", str(args.steps), "--warmup", str(args.warmup),
                     "--batch", str(args.batch), "--model", args.model, "--search", args.search, "--max-steps", str(args.max_steps),
                     "--frames", str(args.frames), "--contexts", str(args.contexts), "--encoder-chains", str(args.encoder_chains)]
            child += ["--solo-policy"] if args.solo_policy else []
            child += ["--free-run"] if args.free_run else []
            child += ["--no-graph"] if args.no_graph else []
            result["alt_precision"] = alt_precision_line(child)
        if (not args.no_other_configs and not args.experiment and coalesce == 1 and golden_name == "full_bench_b64_greedy"
                and args.contexts == 4 and args.encoder_chains == 2 and not (args.solo_policy or args.free_run or args.no_graph)):
            dev.synchronize()
            result["other_configs"] = other_configs_lines(args)
        if not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(args.cpu_sample, args.max_steps, args.cpu_threads,
                                                  big_batch=args.cpu_big_batch)

    if rank == 0:
        assert result["n_gpus"] == args.gpus
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
