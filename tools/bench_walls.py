#!/usr/bin/env python
"""Floor-plan steering against plain and collision-steered generation, in one process (bench.py is not touched).

    python tools/bench_walls.py [--reps 2] [--step-reps 7]        -> one JSON line on stdout, the same record in profiles/walls_bench.json

* the captured step at B = 128, N = 12 (``bedroom21``) and N = 80 (``living80``), a 64 x 64 room mask: the step with the wall launch
  (dsc_steer_walls_f32, every step active) against the unsteered step of the same tree and against the collision-steered one, each
  replayed ``--launches`` times, microseconds per step, the arms in alternation;
* the launch alone, issued eagerly ``--launches`` times on an idle stream (launch latency included), and ops.floor_field alone -- the
  work per call -- at 128 x 64 x 64;
* the calls: generate_layout_batched(128, wall_scale=0.05, room_side=3.1) against generate_layout_batched(128) for the T-step loop
  (T = 1000) and for S = 50, in alternation.
The expectation this tool confirms or refutes: the launch does O(9 N) work against collision steering's O(N^2), so it costs no more than
that launch and under 1 % of a step.  The weights are synthetic: nothing here says anything about the quality of steered scenes.  Every
variant is warmed up first (capture included), a device synchronise brackets every timed call, medians are reported, the driver's
shader clock level is read after the measurements.  Reads nothing outside the repository."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_steer import B, SHAPES, _model, _wall  # noqa: E402

WEIGHT, COLLISION, SIDE, HW = 0.05, 0.02, 3.1, 64


def room_masks(device):
    """(B, 1, 64, 64): an L-shaped room, |x|, |z| < 2 m without the quadrant x, z > 0, the same for every scene but its own copy."""
    import torch
    c = -SIDE + (torch.arange(HW, dtype=torch.float64) + 0.5) * (2 * SIDE / HW)
    X, Z = c[None, :].expand(HW, HW), c[:, None].expand(HW, HW)
    m = ((X.abs() < 2) & (Z.abs() < 2) & ~((X > 0) & (Z > 0))).float()
    return m[None, None].expand(B, 1, HW, HW).contiguous().to(device)


def call_compare(device, n, reps, strided):
    import torch
    mw, cfg = _model(device, n)                  # one model per variant: each keeps its own live graph
    mu, _ = _model(device, n)
    C = cfg["point_dim"]
    rooms = room_masks(device)
    kw = dict(sampling_timesteps=strided) if strided else {}
    calls = {"walls": lambda: mw.generate_layout_batched(rooms, n, C, B, clip_denoised=True, wall_scale=WEIGHT, room_side=SIDE, **kw),
             "unsteered": lambda: mu.generate_layout_batched(rooms, n, C, B, clip_denoised=True, **kw)}
    first = {k: _wall(f) for k, f in calls.items()}
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ts[k].append(_wall(f))
    out = {"shape": [B, n, C], "steps": strided or 1000, "wall_scale": WEIGHT, "room_side": SIDE, "mask": [HW, HW]}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"seconds": round(med, 4), "scenes_per_s": round(B / med, 1), "calls": [round(v, 4) for v in ts[k]],
                  "first_call_s": round(first[k], 3)}
    out["walls_over_unsteered"] = round(statistics.median(ts["walls"]) / statistics.median(ts["unsteered"]), 4)
    torch.cuda.empty_cache()
    return out


def step_compare(device, n, step_reps, launches):
    """Microseconds per captured step -- with the wall launch, with the collision launch, with neither --, per eager wall launch on an
    idle stream and per floor_field call."""
    import torch
    from diffuscene_amd import ops
    from diffuscene_amd.sampler import _StepGraph
    m, cfg = _model(device, n)
    C = cfg["point_dim"]
    gd, net = m.diffusion.diffusion, m.diffusion.model
    rooms = room_masks(device)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        cond, cross = m._sampling_conditions(rooms, n, device)
        weight, k, bounds, bbox_dim, class_dim, field, side = gd._wall_inputs((B, n, C), device, WEIGHT, None, SIDE, rooms, "bench_walls")
        cweight = gd._steer_inputs((B, n, C), device, COLLISION, None, "bench_walls")[0]
        layout = (bounds, bbox_dim, class_dim)
        graphs = {"walls": _StepGraph(gd, net, (B, n, C), device, cond, cross, True, walls=layout + (HW, HW)),
                  "collision": _StepGraph(gd, net, (B, n, C), device, cond, cross, True, steer=layout),
                  "unsteered": _StepGraph(gd, net, (B, n, C), device, cond, cross, True)}
    graphs["walls"].walls.load(weight, k, field, side)
    graphs["collision"].steer.load(cweight, k)

    def run(name):
        g = graphs[name]
        g.x.normal_()
        g.t.fill_(launches)                      # counts down in the graph: stays inside the schedule for the whole timed region
        return _wall(lambda: g.replay_steps(launches)) / launches * 1e6

    g = graphs["walls"]
    rec = ops.walls_rec(g.x, torch.randn((B, n, C), device=device), g.mean_type, walls=g.walls.spec, **g.sched)

    def alone():
        g.t.fill_(0)

        def many():
            for _ in range(launches):
                ops.issue(rec)
        return _wall(many) / launches * 1e6

    fmask = rooms.reshape(B, HW, HW)
    fout = torch.empty_like(fmask)
    frec = ops.floor_field_rec(fmask, fout, SIDE)

    def field_alone():
        def many():
            for _ in range(launches):
                ops.issue(frec)
        return _wall(many) / launches * 1e6

    extra = {"launch_alone": alone, "floor_field": field_alone}
    for name in graphs:
        run(name)
    for f in extra.values():
        f()
    ts = {name: [] for name in list(graphs) + list(extra)}
    for _ in range(step_reps):
        for name in graphs:
            ts[name].append(run(name))
        for name, f in extra.items():
            ts[name].append(f())
    med = {k_: statistics.median(v) for k_, v in ts.items()}
    out = {"shape": [B, n, C], "launches": launches, "mask": [B, HW, HW]}
    for k_ in ts:
        out[k_ + "_us"] = round(med[k_], 2)
        out[k_ + "_all"] = [round(v, 2) for v in ts[k_]]
    out["walls_minus_unsteered_us"] = round(med["walls"] - med["unsteered"], 2)
    out["collision_minus_unsteered_us"] = round(med["collision"] - med["unsteered"], 2)
    out["unsteered_spread_us"] = round(max(ts["unsteered"]) - min(ts["unsteered"]), 2)
    out["launch_share_of_step"] = round((med["walls"] - med["unsteered"]) / med["unsteered"], 5)
    out["launch_alone_share_of_step"] = round(med["launch_alone"] / med["unsteered"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--only", default=None, help="comma list of: steps, tstep, strided")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walls_bench.json"))
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_walls.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    from bench_ddim_complete import shader_clock
    only = set(a.only.split(",")) if a.only else {"steps", "tstep", "strided"}
    out = {"tool": "tools/bench_walls.py", "T": 1000, "git_head": __import__("bench").git_head(), "weights": "synthetic"}
    for n in SHAPES:
        if "steps" in only:
            out["step_b%d_n%d" % (B, n)] = step_compare(device, n, a.step_reps, a.launches)
            torch.cuda.empty_cache()
        if "strided" in only:
            out["s50_b%d_n%d" % (B, n)] = call_compare(device, n, a.reps, 50)
        if "tstep" in only:
            out["tstep_b%d_n%d" % (B, n)] = call_compare(device, n, a.reps, None)
    out["shader_clock"] = shader_clock()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
