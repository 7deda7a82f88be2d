#!/usr/bin/env python
"""Strided (DDIM) batched completion and re-arrangement against the T = 1000 batched calls, through the public entry points, in one process
(bench.py is not touched).

    python tools/bench_ddim_complete.py [--reps 3] [--scenes 64] [--step-reps 7] [--out profiles/ddim_complete_bench.json]
                                                                                          -> one JSON line on stdout, the same in --out

* complete_scene_batched at S in {50, 100, 250} against the unchanged T = 1000 call and against generate_layout_batched at the same S
  (no overwrite: the natural ceiling).  Shapes of tools/bench_complete.py: ``--scenes`` scenes at N = 12 and N = 21 with the given objects
  cycling through four counts, and the ``complete`` benchmark shape (B = 128, N = 80, counts 16..24).
* arrange_scene_batched at the same S against its T = 1000 call, at the ``arrange`` benchmark shape (B = 128, N = 80).
* fused against unfused step: the captured strided step with dsc_ddim_inpaint_step_f32 against the same step captured from ragged
  overwrite + ddim_step, microseconds per replayed step at (128, 80) and (1, 12); ``unfused_spread_us`` is max - min over the unfused
  measurement's own repetitions.
Every variant has its own model (identical seeded weights: one live graph per model) and is warmed up first (capture included); the variants
are then timed in alternation with a device synchronise around every call, medians reported.  The shader clock is read from the driver's
read-only sysfs listing when there is one (nothing is set); in-kernel clocks can sit below that figure."""
import argparse
import contextlib
import glob
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = (50, 100, 250)
P_CYCLE = {12: (1, 3, 5, 8), 21: (2, 5, 9, 14)}


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


def _counts_around_20(B):
    return [20 + (b * 7) % 9 - 4 for b in range(B)]                # 16 .. 24


def _alternate(calls, reps, scenes):
    """Warm every variant up (capture), time them in alternation; per variant: median seconds per call and per scene."""
    first = {k: _wall(f) for k, f in calls.items()}
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ts[k].append(_wall(f))
    out = {}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"seconds_per_call_median": round(med, 4), "seconds_per_scene": round(med / scenes, 5), "scenes_per_s": round(scenes / med, 1),
                  "calls": [round(v, 4) for v in ts[k]], "first_call_s": round(first[k], 3)}
    return out


def _name(kind, S):
    return "%s_%s" % (kind, "T1000" if S is None else "S%d" % S)


def _ddim(S):
    return {} if S is None else dict(sampling_timesteps=S, ddim_sampling_eta=0.0)


def completion(device, spec, x, counts, reps):
    """complete_scene_batched (T = 1000 and every S) and generate_layout_batched (every S) on one shape."""
    import torch
    B, N = len(counts), spec["objects"]
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    calls = {}
    for S in (None,) + STEPS:
        m, cfg = _model(spec, device)
        calls[_name("complete_scene_batched", S)] = (lambda m=m, C=cfg["point_dim"], S=S: m.complete_scene_batched(
            rooms, N, C, x, num_partial=counts, clip_denoised=True, **_ddim(S)))
    for S in STEPS:
        m, cfg = _model(spec, device)
        calls[_name("generate_layout_batched", S)] = (lambda m=m, C=cfg["point_dim"], S=S: m.generate_layout_batched(
            rooms, N, C, B, clip_denoised=True, **_ddim(S)))
    out = _alternate(calls, reps, B)
    full = out[_name("complete_scene_batched", None)]["seconds_per_call_median"]
    for S in STEPS:
        c, g = out[_name("complete_scene_batched", S)], out[_name("generate_layout_batched", S)]
        c["speedup_over_T1000"] = round(full / c["seconds_per_call_median"], 1)
        c["completion_over_generation"] = round(c["seconds_per_call_median"] / g["seconds_per_call_median"], 4)
    return out


def sweep(device, N, scenes, reps):
    import bench
    spec = dict(bench.CONFIGS["bedroom21"], batch=scenes, objects=N)
    x = _scenes(spec, scenes, device)
    counts = [P_CYCLE[N][i % len(P_CYCLE[N])] for i in range(scenes)]
    row = {"scenes": scenes, "objects": N, "given_objects_cycle": list(P_CYCLE[N])}
    row.update(completion(device, spec, x, counts, reps))
    return row


def benchmark_shape(device, reps):
    import bench
    spec = dict(bench.CONFIGS["complete"])
    B = spec["batch"]
    counts = _counts_around_20(B)
    row = {"workload": "uncond living rooms, B=%d, N=%d, given objects per scene %d..%d" % (B, spec["objects"], min(counts), max(counts))}
    row.update(completion(device, spec, _scenes(spec, B, device), counts, reps))
    return row


def arrangement(device, reps):
    import bench
    import torch
    spec = dict(bench.CONFIGS["arrange"])
    B, N = spec["batch"], spec["objects"]
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    x = None
    calls = {}
    for S in (None,) + STEPS:
        m, cfg = _model(spec, device)
        if x is None:
            from diffuscene_amd import workloads as W
            x = W.synth_scene_batch(B, N, spec["class_dim"], 32, 7)[:, :, :cfg["point_dim"]].contiguous().to(device)
        calls[_name("arrange_scene_batched", S)] = (lambda m=m, C=cfg["point_dim"], S=S: m.arrange_scene_batched(
            rooms, N, C, x, clip_denoised=True, **_ddim(S)))
    out = _alternate(calls, reps, B)
    full = out[_name("arrange_scene_batched", None)]["seconds_per_call_median"]
    for S in STEPS:
        out[_name("arrange_scene_batched", S)]["speedup_over_T1000"] = round(full / out[_name("arrange_scene_batched", S)]["seconds_per_call_median"], 1)
    out["workload"] = "re-arrangement, living rooms, B=%d, N=%d" % (B, N)
    return out


def step_compare(device, B, N, step_reps, S=250, steps=200):
    """Microseconds per replayed captured step: fused (dsc_ddim_inpaint_step_f32) against unfused (ragged overwrite + ddim_step)."""
    import bench
    import torch
    from diffuscene_amd.sampler import graph_ddim_complete_ragged_loop
    spec = dict(bench.CONFIGS["complete" if N == 80 else "bedroom21"], batch=B, objects=N)
    x = _scenes(spec, B, device)
    counts = torch.tensor([min(N, c) for c in (_counts_around_20(B) if N == 80 else [3 + b % 5 for b in range(B)])], dtype=torch.int64, device=device)
    graphs = {}
    for fused in (True, False):
        m, cfg = _model(spec, device)
        diff = m.diffusion
        cond = m._base_condition(None, B, N, device).contiguous()
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            graph_ddim_complete_ragged_loop(diff.diffusion, diff._denoise, (B, N, cfg["point_dim"]), device, cond, None, S, 0.0, torch.randn,
                                            x.contiguous(), counts, fused=fused)
        g, = diff.diffusion._graphs.values()
        assert g.fused is fused and g.S == S and steps < S
        graphs[fused] = (m, g)

    def run(fused):
        g = graphs[fused][1]
        g.check_current()
        g.step.zero_()                                             # `steps` < S - 1 replays: the counter stays inside the tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            g.graph.replay()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        g.step.zero_()
        return dt / steps * 1e6

    for fused in graphs:
        run(fused)
    ts = {True: [], False: []}
    for _ in range(step_reps):
        for fused in (True, False):
            ts[fused].append(run(fused))
    fm, um = statistics.median(ts[True]), statistics.median(ts[False])
    spread = max(ts[False]) - min(ts[False])
    return {"shape": [B, N], "S": S, "replayed_steps_per_repetition": steps, "repetitions": step_reps,
            "fused_us_per_step": round(fm, 2), "unfused_us_per_step": round(um, 2),
            "fused_all": [round(v, 2) for v in ts[True]], "unfused_all": [round(v, 2) for v in ts[False]],
            "unfused_spread_us": round(spread, 2), "fused_minus_unfused_us": round(fm - um, 2),
            "fused_not_slower_within_spread": bool(fm - um <= spread)}


def shader_clock():
    """The driver's current shader clock level ('*' line of pp_dpm_sclk), read only; None when the listing is not there."""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            with open(path) as f:
                cur = [ln.strip() for ln in f if ln.strip().endswith("*")]
            if cur:
                return {"source": "pp_dpm_sclk (first card, after the measurements)", "current": cur[0]}
        except OSError:
            continue
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--only", default=None, help="comma list of: sweep12, sweep21, shape, arrange, steps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddim_complete_bench.json"))
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ddim_complete.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else {"sweep12", "sweep21", "shape", "arrange", "steps"}
    out = {"tool": "tools/bench_ddim_complete.py", "T": 1000, "S": list(STEPS), "eta": 0.0, "git_head": __import__("bench").git_head()}
    if "steps" in only:
        out["captured_step_b128_n80"] = step_compare(device, 128, 80, a.step_reps)
        out["captured_step_b1_n12"] = step_compare(device, 1, 12, a.step_reps)
        torch.cuda.empty_cache()
    for N in (12, 21):
        if "sweep%d" % N in only:
            out["sweep_n%d" % N] = sweep(device, N, a.scenes, a.reps)
            torch.cuda.empty_cache()
    if "shape" in only:
        out["benchmark_shape_b128_n80"] = benchmark_shape(device, a.reps)
        torch.cuda.empty_cache()
    if "arrange" in only:
        out["arrange_b128_n80"] = arrangement(device, a.reps)
        torch.cuda.empty_cache()
    out["shader_clock"] = shader_clock()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
