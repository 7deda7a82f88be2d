#!/usr/bin/env python
"""Collision steering against plain generation, through the public entry point, in one process (bench.py is not touched).

    python tools/bench_steer.py [--reps 2] [--step-reps 7]        -> one JSON line on stdout, the same record in profiles/steer_bench.json

* the calls: generate_layout_batched(128, collision_scale=0.02) against generate_layout_batched(128) of the same model configuration
  (bench.py's ``bedroom21`` at N = 12 and ``living80`` at N = 80, synthetic weights) for the T-step loop (T = 1000) and for S = 50, in
  alternation in the same process -- the yardstick is the unsteered call beside it, not an earlier run;
* the captured step: the steered step (one more launch, dsc_steer_boxes_f32 with every step active) against the unsteered step, each
  replayed ``--launches`` times, microseconds per step, in alternation; and the steering launch alone, issued eagerly ``--launches`` times
  on an idle stream (what one launch costs when nothing hides it: launch latency included).
The expectation this tool confirms or refutes: the launch costs under 1 % of a step.  The weights are synthetic: nothing here says
anything about the quality of steered scenes.  Every variant is warmed up first (capture included), a device synchronise brackets every
timed call, medians are reported.  Reads nothing outside the repository."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, WEIGHT = 128, 0.02
SHAPES = {12: "bedroom21", 80: "living80"}


def _model(device, n):
    import bench
    spec = dict(bench.CONFIGS[SHAPES[n]], batch=B, objects=n)
    model, cfg = bench.build_model(spec, device)
    return model.eval(), cfg


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def call_compare(device, n, reps, strided):
    import torch
    ms, cfg = _model(device, n)                  # one model per variant: each keeps its own live graph
    mu, _ = _model(device, n)
    C = cfg["point_dim"]
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    kw = dict(sampling_timesteps=strided) if strided else {}
    calls = {"steered": lambda: ms.generate_layout_batched(rooms, n, C, B, clip_denoised=True, collision_scale=WEIGHT, **kw),
             "unsteered": lambda: mu.generate_layout_batched(rooms, n, C, B, clip_denoised=True, **kw)}
    first = {k: _wall(f) for k, f in calls.items()}
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ts[k].append(_wall(f))
    out = {"shape": [B, n, C], "steps": strided or 1000, "collision_scale": WEIGHT}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"seconds": round(med, 4), "scenes_per_s": round(B / med, 1), "calls": [round(v, 4) for v in ts[k]],
                  "first_call_s": round(first[k], 3)}
    out["steered_over_unsteered"] = round(statistics.median(ts["steered"]) / statistics.median(ts["unsteered"]), 4)
    return out


def step_compare(device, n, step_reps, launches):
    """Microseconds per captured step, steered and unsteered, and per eager steering launch on an idle stream."""
    import torch
    from diffuscene_amd import ops
    from diffuscene_amd.sampler import _StepGraph
    m, cfg = _model(device, n)
    C = cfg["point_dim"]
    gd, net = m.diffusion.diffusion, m.diffusion.model
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        cond, cross = m._sampling_conditions(rooms, n, device)
        weight, k, bounds, bbox_dim, class_dim = gd._steer_inputs((B, n, C), device, WEIGHT, None, "bench_steer")
        graphs = {"steered": _StepGraph(gd, net, (B, n, C), device, cond, cross, True, steer=(bounds, bbox_dim, class_dim)),
                  "unsteered": _StepGraph(gd, net, (B, n, C), device, cond, cross, True)}
    graphs["steered"].steer.load(weight, k)

    def run(name):
        g = graphs[name]
        g.x.normal_()
        g.t.fill_(launches)                      # counts down in the graph: stays inside the schedule for the whole timed region
        return _wall(lambda: g.replay_steps(launches)) / launches * 1e6

    g = graphs["steered"]
    rec = ops.steer_rec(g.x, torch.randn((B, n, C), device=device), g.mean_type, steer=g.steer.spec, **g.sched)

    def alone():
        g.t.fill_(0)

        def many():
            for _ in range(launches):
                ops.issue(rec)
        return _wall(many) / launches * 1e6

    for name in graphs:
        run(name)
    alone()
    ts = {name: [] for name in list(graphs) + ["launch_alone"]}
    for _ in range(step_reps):
        for name in graphs:
            ts[name].append(run(name))
        ts["launch_alone"].append(alone())
    med = {k_: statistics.median(v) for k_, v in ts.items()}
    out = {"shape": [B, n, C], "launches": launches}
    for k_ in ts:
        out[k_ + "_us"] = round(med[k_], 2)
        out[k_ + "_all"] = [round(v, 2) for v in ts[k_]]
    out["steered_minus_unsteered_us"] = round(med["steered"] - med["unsteered"], 2)
    out["unsteered_spread_us"] = round(max(ts["unsteered"]) - min(ts["unsteered"]), 2)
    out["launch_share_of_step"] = round((med["steered"] - med["unsteered"]) / med["unsteered"], 5)
    out["launch_alone_share_of_step"] = round(med["launch_alone"] / med["unsteered"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--only", default=None, help="comma list of: steps, tstep, strided")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steer_bench.json"))
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_steer.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else {"steps", "tstep", "strided"}
    out = {"tool": "tools/bench_steer.py", "T": 1000, "git_head": __import__("bench").git_head(), "weights": "synthetic"}
    for n in SHAPES:
        if "steps" in only:
            out["step_b%d_n%d" % (B, n)] = step_compare(device, n, a.step_reps, a.launches)
            torch.cuda.empty_cache()
        if "strided" in only:
            out["s50_b%d_n%d" % (B, n)] = call_compare(device, n, a.reps, 50)
            torch.cuda.empty_cache()
        if "tstep" in only:
            out["tstep_b%d_n%d" % (B, n)] = call_compare(device, n, a.reps, None)
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
