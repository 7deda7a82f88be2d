#!/usr/bin/env python
"""Batched scene completion against the per-scene call, through the public entry points, in one process (bench.py is not touched).

    python tools/bench_complete.py [--reps 3] [--scenes 64] [--step-reps 7]        -> one JSON line on stdout

* per-scene baseline: complete_scene(batch_size=1) over ``--scenes`` scenes, N = 12 and N = 21, T = 1000, seconds per scene.  In the
  ``cycling`` sweep the number of given objects P cycles through four values from scene to scene, as a sweep over a test set does; the
  graph cache of the uniform loop keys on P and keeps one live graph, so every change of P re-captures -- that is part of what the call
  costs and stays in.  The ``constant`` sweep holds P fixed (no re-capture after the first call), so the capture cost shows as the
  difference.  The two sweeps have a model each (identical weights) and are timed in alternation, scene by scene.
* batched: complete_scene_batched on the same scenes in ONE call (seconds per scene), and at the ``complete`` benchmark shape (B = 128,
  N = 80, counts 16..24) scenes per second, beside generate_layout_batched at the same B and N -- no overwrite, the natural ceiling.
* fused against unfused step: the captured ragged step with dsc_p_sample_inpaint_f32 against the same step captured from ragged
  overwrite + p_sample, microseconds per replayed step at (128, 80) and (1, 12); ``unfused_spread_us`` is max - min over the unfused
  measurement's own repetitions, the yardstick for "not slower".
Every variant is warmed up first (capture included), a device synchronise brackets every timed call, medians are reported."""
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

P_CYCLE = {12: (1, 3, 5, 8), 21: (2, 5, 9, 14)}
P_CONST = {12: 3, 21: 5}


def _model(spec, device):
    import bench
    model, cfg = bench.build_model(spec, device)
    model.eval()
    return model, cfg


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _scenes(spec, count, device, seed=7):
    from diffuscene_amd import workloads as W
    return W.synth_scene_batch(count, spec["objects"], spec["class_dim"], 32, seed).to(device)


def sweep(device, N, scenes, reps):
    """complete_scene(batch_size=1) per scene (P cycling / P constant) against one complete_scene_batched call over the same scenes."""
    import bench
    import torch
    spec = dict(bench.CONFIGS["bedroom21"], batch=1, objects=N)
    x = _scenes(spec, scenes, device)
    room = torch.zeros(1, 1, 64, 64, device=device)
    cyc = [P_CYCLE[N][i % len(P_CYCLE[N])] for i in range(scenes)]
    models = {k: _model(spec, device) for k in ("cycling", "constant", "batched")}
    C = models["batched"][1]["point_dim"]

    def one(kind, i, p):
        m = models[kind][0]
        return _wall(lambda: m.complete_scene(room, N, C, x[i:i + 1, :p].contiguous(), batch_size=1, clip_denoised=True))

    first = {"cycling": one("cycling", 0, cyc[-1]), "constant": one("constant", 0, P_CONST[N])}      # warm-up: code objects, first capture
    ts = {"cycling": [], "constant": []}
    for i in range(scenes):                                       # alternation, scene by scene
        ts["cycling"].append(one("cycling", i, cyc[i]))
        ts["constant"].append(one("constant", i, P_CONST[N]))
    mb = models["batched"][0]
    rooms = torch.zeros(scenes, 1, 64, 64, device=device)
    given = [x[i, :cyc[i]].contiguous() for i in range(scenes)]
    call = lambda: mb.complete_scene_batched(rooms, N, C, given, clip_denoised=True)      # noqa: E731
    first["batched"] = _wall(call)
    tb = [_wall(call) for _ in range(reps)]
    row = {"scenes": scenes, "given_objects_cycle": list(P_CYCLE[N]), "given_objects_constant": P_CONST[N]}
    for k in ("cycling", "constant"):
        row["complete_scene_b1_" + k] = {"seconds_per_scene_mean": round(sum(ts[k]) / scenes, 4),
                                         "seconds_per_scene_median": round(statistics.median(ts[k]), 4),
                                         "min": round(min(ts[k]), 4), "max": round(max(ts[k]), 4), "first_call_s": round(first[k], 3)}
    med = statistics.median(tb)
    row["complete_scene_batched"] = {"seconds_per_call_median": round(med, 4), "seconds_per_scene": round(med / scenes, 5),
                                     "calls": [round(v, 4) for v in tb], "first_call_s": round(first["batched"], 3)}
    row["capture_cost_s_per_scene"] = round((sum(ts["cycling"]) - sum(ts["constant"])) / scenes, 4)
    row["speedup_over_cycling_sweep"] = round(sum(ts["cycling"]) / scenes / (med / scenes), 1)
    row["speedup_over_constant_sweep"] = round(sum(ts["constant"]) / scenes / (med / scenes), 1)
    return row


def _counts_around_20(B):
    return [20 + (b * 7) % 9 - 4 for b in range(B)]                # 16 .. 24


def benchmark_shape(device, reps):
    import bench
    import torch
    spec = dict(bench.CONFIGS["complete"])
    B, N = spec["batch"], spec["objects"]
    x = _scenes(spec, B, device)
    counts = _counts_around_20(B)
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    mc, cfg = _model(spec, device)
    mg, _ = _model(spec, device)
    C = cfg["point_dim"]
    calls = {"complete_scene_batched": lambda: mc.complete_scene_batched(rooms, N, C, x, num_partial=counts, clip_denoised=True),
             "generate_layout_batched": lambda: mg.generate_layout_batched(rooms, N, C, B, clip_denoised=True)}
    first = {k: _wall(f) for k, f in calls.items()}
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ts[k].append(_wall(f))
    out = {"workload": "uncond living rooms, B=%d, N=%d, T=1000, given objects per scene %d..%d" % (B, N, min(counts), max(counts))}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"seconds": round(med, 3), "scenes_per_s": round(B / med, 1), "calls": [round(v, 3) for v in ts[k]],
                  "first_call_s": round(first[k], 3)}
    out["completion_over_generation"] = round(statistics.median(ts["complete_scene_batched"]) / statistics.median(ts["generate_layout_batched"]), 4)
    return out


def step_compare(device, B, N, step_reps, steps=200):
    """Microseconds per replayed captured step: fused (dsc_p_sample_inpaint_f32) against unfused (ragged overwrite + p_sample)."""
    import bench
    import torch
    from diffuscene_amd.sampler import graph_complete_ragged_loop
    spec = dict(bench.CONFIGS["complete" if N == 80 else "bedroom21"], batch=B, objects=N)
    x = _scenes(spec, B, device)
    counts = torch.tensor([min(N, c) for c in (_counts_around_20(B) if N == 80 else [3 + b % 5 for b in range(B)])], dtype=torch.int64, device=device)
    graphs = {}
    for fused in (True, False):
        m, cfg = _model(spec, device)
        diff = m.diffusion
        cond = m._base_condition(None, B, N, device).contiguous()
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            graph_complete_ragged_loop(diff.diffusion, diff._denoise, (B, N, cfg["point_dim"]), device, cond, None, True, 2, torch.randn,
                                       x.contiguous(), counts, fused=fused)
        g, = diff.diffusion._graphs.values()
        assert g.fused is fused
        graphs[fused] = (m, g)

    def run(fused):
        g = graphs[fused][1]
        g.check_current()
        g.t.fill_(999)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            g.graph.replay()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        g.t.fill_(0)
        return dt / steps * 1e6

    for fused in graphs:
        run(fused)
    ts = {True: [], False: []}
    for _ in range(step_reps):
        for fused in (True, False):
            ts[fused].append(run(fused))
    fm, um = statistics.median(ts[True]), statistics.median(ts[False])
    spread = max(ts[False]) - min(ts[False])
    return {"shape": [B, N], "replayed_steps_per_repetition": steps, "repetitions": step_reps,
            "fused_us_per_step": round(fm, 2), "unfused_us_per_step": round(um, 2),
            "fused_all": [round(v, 2) for v in ts[True]], "unfused_all": [round(v, 2) for v in ts[False]],
            "unfused_spread_us": round(spread, 2), "fused_minus_unfused_us": round(fm - um, 2),
            "fused_not_slower_within_spread": bool(fm - um <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma list of: sweep12, sweep21, shape, steps")
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_complete.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else {"sweep12", "sweep21", "shape", "steps"}
    out = {"tool": "tools/bench_complete.py", "T": 1000, "git_head": __import__("bench").git_head()}
    if "steps" in only:
        out["captured_step_b128_n80"] = step_compare(device, 128, 80, a.step_reps)
        out["captured_step_b1_n12"] = step_compare(device, 1, 12, a.step_reps)
        torch.cuda.empty_cache()
    if "shape" in only:
        out["benchmark_shape_b128_n80"] = benchmark_shape(device, a.reps)
        torch.cuda.empty_cache()
    for N in (12, 21):
        if "sweep%d" % N in only:
            out["sweep_n%d" % N] = sweep(device, N, a.scenes, a.reps)
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
