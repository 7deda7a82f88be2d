#!/usr/bin/env python
"""Resampling jumps (RePaint) against the loops they ride on, in one process (bench.py is not touched).

    python tools/bench_resample.py [--reps 3] [--launches 200]     -> one JSON line on stdout, the same record in profiles/resample_bench.json

* the jump graph of the captured masked loop replayed ``--launches`` times against one captured step replayed as often, microseconds each,
  in alternation, at B = 128, N = 12 and N = 80; and the jump launch alone (dsc_resample_jump_f32 with a mask), issued eagerly
  ``--launches`` times on an idle stream (launch latency included: what one launch costs when nothing hides it);
* the calls: inpaint_scene_batched at T = 1000 with resample=(10, 3), resample_steps=250 and at S = 250 with resample=(10, 10) against the
  same calls without ``resample`` (bench.py's ``bedroom21`` at N = 12, synthetic weights), in alternation in the same process.
The expectation this tool confirms or refutes: a call costs its model-call count times the plain step, and a jump is launch latency -- a few
microseconds, under 1 % of a step.  Every variant is warmed up first (capture included), a device synchronise brackets every timed call,
medians and spreads are reported, the driver's shader clock level is read after the measurements.  Reads nothing outside the repository."""
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


def _stats(xs, scale=1.0):
    return dict(median=statistics.median(xs) * scale, min=min(xs) * scale, max=max(xs) * scale)


def _inputs(device, n, c):
    import torch
    g = torch.Generator().manual_seed(1)
    boxes = (torch.rand((B, n, c), generator=g) * 2 - 1).to(device)
    mask = torch.zeros((B, n, c), dtype=torch.bool)
    mask[:, :min(3, n)] = True                        # three objects given, the rest of the room asked for
    return boxes, mask


def step_compare(device, n, reps, launches):
    """Microseconds per replay: the jump graph against one captured step of the T-step masked loop; the jump launch alone."""
    import torch
    from diffuscene_amd import ops
    model, cfg = _model(device, n)
    c = cfg["point_dim"]
    boxes, mask = _inputs(device, n, c)
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    gd = model.diffusion.diffusion
    with contextlib.redirect_stdout(io.StringIO()):      # builds the graph set (step, prejump, jump, final) and leaves it cached
        model.inpaint_scene_batched(rooms, n, c, boxes, mask, clip_denoised=True, resample=(10, 2), resample_steps=10)
    (g,) = gd._graphs.values()
    T = gd.num_timesteps

    def replay(graph, start):
        def run():
            g.t.fill_(start)
            for _ in range(launches):
                graph.replay()
                g.t.fill_(start)                         # the same rows every time: the tables stay in range
        return run
    arms = {"step": replay(g.graph, T // 2), "jump_graph": replay(g.jump, T // 2)}
    x, noise = g.x.clone(), torch.randn_like(g.x)
    t = torch.full((B,), T // 2, dtype=torch.int64, device=device)

    def alone():
        for _ in range(launches):
            ops.resample_jump(x, noise, g.resample.ja, g.resample.jb, 10, t=t, mask=(g.known, noise, g.mask), q=g.q)
    arms["jump_launch_alone"] = alone
    for f in arms.values():
        _wall(f)
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            times[k].append(_wall(f) / launches)
    fill = _wall(lambda: [g.t.fill_(0) for _ in range(launches)]) / launches      # the fill between replays, to subtract
    out = {k: _stats(v, 1e6) for k, v in times.items()}
    out["fill_us"] = fill * 1e6
    out["jump_graph_over_step"] = (out["jump_graph"]["median"] - out["fill_us"]) / (out["step"]["median"] - out["fill_us"])
    g._park()
    return out


def call_compare(device, reps):
    import torch
    n = 12
    variants = {"t1000_plain": dict(), "t1000_resample_10_3_k250": dict(resample=(10, 3), resample_steps=250),
                "s250_plain": dict(sampling_timesteps=250), "s250_resample_10_10": dict(sampling_timesteps=250, resample=(10, 10))}
    models = {k: _model(device, n) for k in variants}        # one model per variant: each keeps its own live graph
    c = models["t1000_plain"][1]["point_dim"]
    boxes, mask = _inputs(device, n, c)
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    calls = {k: (lambda k=k: models[k][0].inpaint_scene_batched(rooms, n, c, boxes, mask, clip_denoised=True, **variants[k])) for k in variants}
    first = {k: _wall(f) for k, f in calls.items()}
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            times[k].append(_wall(f))
    gd = models["t1000_plain"][0].diffusion.diffusion
    counts = {"t1000_plain": 1000, "t1000_resample_10_3_k250": gd.resample_schedule(10, 3, 250).calls, "s250_plain": 250,
              "s250_resample_10_10": gd.resample_schedule(10, 10, sampling_timesteps=250).calls}
    out = {k: dict(_stats(v), first_call=first[k], model_calls=counts[k]) for k, v in times.items()}
    for res, plain in (("t1000_resample_10_3_k250", "t1000_plain"), ("s250_resample_10_10", "s250_plain")):
        out[res]["time_over_plain"] = out[res]["median"] / out[plain]["median"]
        out[res]["calls_over_plain"] = counts[res] / counts[plain]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-calls", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    device = torch.device("cuda:0")
    from bench_ddim_complete import shader_clock
    rec = dict(tool="bench_resample", batch=B, reps=args.reps, launches=args.launches, git_head=bench.git_head())
    rec["step"] = {"N%d" % n: step_compare(device, n, args.reps + 2, args.launches) for n in SHAPES}
    rec["calls"] = "not measured" if args.skip_calls else call_compare(device, args.reps)
    rec["shader_clock"] = shader_clock()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "resample_bench.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
