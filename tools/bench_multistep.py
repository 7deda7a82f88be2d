#!/usr/bin/env python
"""The multistep DPM-Solver++(2M) solver against the DDIM loops it rides on, in one process (bench.py is not touched).

    python tools/bench_multistep.py [--reps 3] [--step-reps 7]     -> one JSON line on stdout, the same record in profiles/multistep_bench.json

* the captured strided step: the step with the solver's launch (dsc_multistep_x0_f32 after the model call) against the step without it,
  each replayed ``--launches`` times on a schedule of ``--launches`` + 1 pairs, microseconds per step, in alternation; and the launch
  alone, issued eagerly ``--launches`` times on an idle stream (launch latency included: what one launch costs when nothing hides it);
* the calls: generate_layout_batched(128, sampling_timesteps=20, sampling_solver="dpmpp_2m") against S = 50 DDIM and S = 20 DDIM of the
  same model configuration (bench.py's ``bedroom21`` at N = 12 and ``living80`` at N = 80, synthetic weights), in alternation in the
  same process -- the yardstick is the call beside it, not an earlier run.
The expectations this tool confirms or refutes: the launch adds under 1 % of a step, and the S = 20 call costs 20 / 50 of the S = 50 one.
The weights are synthetic: nothing here says anything about sample quality.  Every variant is warmed up first (capture included), a
device synchronise brackets every timed call, medians are reported, the driver's shader clock level is read after the measurements.
Reads nothing outside the repository."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

B = 128
SHAPES = {12: "bedroom21", 80: "living80"}
SOLVER = "dpmpp_2m"


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


def call_compare(device, n, reps):
    import torch
    variants = {"dpmpp_2m_s20": dict(sampling_timesteps=20, sampling_solver=SOLVER), "ddim_s50": dict(sampling_timesteps=50),
                "ddim_s20": dict(sampling_timesteps=20)}
    models = {k: _model(device, n) for k in variants}        # one model per variant: each keeps its own live graph
    C = models["ddim_s50"][1]["point_dim"]
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    calls = {k: (lambda k=k: models[k][0].generate_layout_batched(rooms, n, C, B, clip_denoised=True, **variants[k])) for k in variants}
    first = {k: _wall(f) for k, f in calls.items()}
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ts[k].append(_wall(f))
    out = {"shape": [B, n, C]}
    med = {k: statistics.median(v) for k, v in ts.items()}
    for k in calls:
        out[k] = {"seconds": round(med[k], 4), "scenes_per_s": round(B / med[k], 1), "calls": [round(v, 4) for v in ts[k]],
                  "first_call_s": round(first[k], 3)}
    out["solver_s20_over_ddim_s50"] = round(med["dpmpp_2m_s20"] / med["ddim_s50"], 4)
    out["solver_s20_over_ddim_s20"] = round(med["dpmpp_2m_s20"] / med["ddim_s20"], 4)
    return out


def step_compare(device, n, step_reps, launches):
    """Microseconds per captured strided step, with and without the solver's launch, and per eager launch on an idle stream."""
    import torch
    from diffuscene_amd import ops
    from diffuscene_amd.sampler import _DDIMGraph
    m, cfg = _model(device, n)
    C = cfg["point_dim"]
    gd, net = m.diffusion.diffusion, m.diffusion.model
    S = launches + 1                             # the replayed step advances the pair: every replay stays inside the schedule
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        cond, cross = m._sampling_conditions(rooms, n, device)
        graphs = {"solver": _DDIMGraph(gd, net, (B, n, C), device, cond, cross, S, multistep=True),
                  "ddim": _DDIMGraph(gd, net, (B, n, C), device, cond, cross, S)}
    dtab = gd.ddim_tables(S, 0.0, device)
    t0 = {"solver": graphs["solver"]._begin(dtab, gd.multistep_table(S, device))[0], "ddim": graphs["ddim"]._begin(dtab)[0]}

    def run(name):
        g = graphs[name]
        g.x.normal_()
        g.step.zero_()
        g.t.fill_(t0[name])
        return _wall(lambda: g.replay_steps(launches)) / launches * 1e6

    g = graphs["solver"]
    rec = ops.multistep_rec(g.x, torch.randn((B, n, C), device=device), g.multistep.hist, g.multistep.weights, g.mean_type, **g.sched)

    def alone():
        g.step.fill_(1)                          # an active pair: the history is read, both outputs are written

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
    for gr in graphs.values():
        gr._park()
    med = {k: statistics.median(v) for k, v in ts.items()}
    out = {"shape": [B, n, C], "launches": launches}
    for k in ts:
        out[k + "_us"] = round(med[k], 2)
        out[k + "_all"] = [round(v, 2) for v in ts[k]]
    out["solver_minus_ddim_us"] = round(med["solver"] - med["ddim"], 2)
    out["ddim_spread_us"] = round(max(ts["ddim"]) - min(ts["ddim"]), 2)
    out["launch_share_of_step"] = round((med["solver"] - med["ddim"]) / med["ddim"], 5)
    out["launch_alone_share_of_step"] = round(med["launch_alone"] / med["ddim"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--only", default=None, help="comma list of: steps, calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistep_bench.json"))
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_multistep.py measures on a HIP device; none is visible")
    from bench_ddim_complete import shader_clock
    device = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else {"steps", "calls"}
    out = {"tool": "tools/bench_multistep.py", "T": 1000, "solver": SOLVER, "git_head": __import__("bench").git_head(), "weights": "synthetic"}
    for n in SHAPES:
        if "steps" in only:
            out["step_b%d_n%d" % (B, n)] = step_compare(device, n, a.step_reps, a.launches)
            torch.cuda.empty_cache()
        if "calls" in only:
            out["calls_b%d_n%d" % (B, n)] = call_compare(device, n, a.reps)
            torch.cuda.empty_cache()
    out["shader_clock"] = shader_clock()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
