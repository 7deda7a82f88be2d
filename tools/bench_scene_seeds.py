#!/usr/bin/env python
"""Per-scene seeds against the device generator, in one process (bench.py is not touched).

    python tools/bench_scene_seeds.py [--step-reps 7] [--launches 200]     -> one JSON line on stdout, the same record in
                                                                              profiles/scene_seeds_bench.json

* the captured step of p_sample_loop, seeded (dsc_scene_randn_f32 + the draw-counter increment) against unseeded (the torch.randn node),
  each replayed ``--launches`` times, microseconds per step, in alternation: B = 256, N = 80, C = 65 (bench.py's ``living80``) and
  B = 1, N = 12 (``bedroom21`` at N = 12, C = 62);
* the kernel alone at 256 x 80 x 65: microseconds per launch over ``--launches`` launches, beside torch.randn of the same shape.
The question is whether the seeded step stays inside the run-to-run spread of the unseeded repetitions (the draw is 5.3 MB of stores in a
step of several milliseconds); the record holds every repetition, nothing is asserted.  Every variant is warmed up first (capture
included), a device synchronise brackets every timed region, medians are reported.  Reads nothing outside the repository."""
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


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def step_compare(device, config, B, N, step_reps, launches):
    """Microseconds per captured p_sample_loop step at (B, N): the seeded graph against the unseeded one of the same model."""
    import bench
    import torch
    from diffuscene_amd.sampler import SEEDED, _StepGraph
    spec = dict(bench.CONFIGS[config], batch=B, objects=N, kind="uncond")
    m, cfg = bench.build_model(spec, device)
    m.eval()
    C = cfg["point_dim"]
    gd, net = m.diffusion.diffusion, m.diffusion.model
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        cond, cross = m._sampling_conditions(rooms, N, device)
        graphs = {"unseeded": _StepGraph(gd, net, (B, N, C), device, cond, cross, True),
                  "seeded": _StepGraph(gd, net, (B, N, C), device, cond, cross, True, replay=SEEDED)}
    graphs["seeded"].seeds.copy_(torch.arange(B, device=device))

    def run(name):
        g = graphs[name]
        g.x.normal_()
        g.t.fill_(launches)                      # counts down in the graph: stays inside the schedule for the whole timed region
        g.noise.counter.fill_(1)
        return _wall(lambda: g.replay_steps(launches)) / launches * 1e6

    for name in graphs:
        run(name)
    ts = {name: [] for name in graphs}
    for _ in range(step_reps):
        for name in ts:
            ts[name].append(run(name))
    med = {k: statistics.median(v) for k, v in ts.items()}
    out = {"shape": [B, N, C], "launches": launches}
    for k in ts:
        out[k + "_us_per_step"] = round(med[k], 2)
        out[k + "_all"] = [round(v, 2) for v in ts[k]]
    out["seeded_minus_unseeded_us"] = round(med["seeded"] - med["unseeded"], 2)
    out["unseeded_spread_us"] = round(max(ts["unseeded"]) - min(ts["unseeded"]), 2)
    out["inside_unseeded_spread"] = bool(min(ts["unseeded"]) <= med["seeded"] <= max(ts["unseeded"]))
    return out


def kernel_alone(device, B, N, C, reps, launches):
    import torch
    from diffuscene_amd import ops
    seeds = torch.arange(B, dtype=torch.int64, device=device)
    draw = torch.zeros((1,), dtype=torch.int64, device=device)
    out = torch.empty((B, N, C), device=device)
    calls = {"scene_randn": lambda: ops.scene_randn(seeds, draw, 0, (B, N, C), out=out), "torch_randn": lambda: out.normal_()}

    def run(f):
        def many():
            for _ in range(launches):
                f()
        return _wall(many) / launches * 1e6

    for f in calls.values():
        run(f)
    ts = {k: [run(f) for _ in range(reps)] for k, f in calls.items()}
    rec = {"shape": [B, N, C], "launches": launches, "bytes_stored": B * N * C * 4}
    for k, v in ts.items():
        rec[k + "_us"] = round(statistics.median(v), 2)
        rec[k + "_all"] = [round(x, 2) for x in v]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_seeds_bench.json"))
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_scene_seeds.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    out = {"tool": "tools/bench_scene_seeds.py", "T": 1000, "git_head": __import__("bench").git_head()}
    out["step_b256_n80"] = step_compare(device, "living80", 256, 80, a.step_reps, a.launches)
    torch.cuda.empty_cache()
    out["step_b1_n12"] = step_compare(device, "bedroom21", 1, 12, a.step_reps, a.launches)
    torch.cuda.empty_cache()
    out["kernel_b256_n80_c65"] = kernel_alone(device, 256, 80, 65, a.step_reps, a.launches)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
