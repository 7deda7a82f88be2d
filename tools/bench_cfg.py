#!/usr/bin/env python
"""Classifier-free guidance against plain text-conditioned generation, through the public entry points, in one process (bench.py is not
touched).

    python tools/bench_cfg.py [--reps 3] [--step-reps 7]        -> one JSON line on stdout, the same record in profiles/cfg_bench.json

* the calls: generate_layout_batched(128, text, guidance_scale=2) against generate_layout_batched(128, text) of the same model
  configuration (bench.py's ``text``: B = 128, N = 12, L = 32 cached BERT rows per scene) for the T-step loop (T = 1000) and for S = 50,
  in alternation in the same process -- the yardstick is the unguided call beside it, not an earlier run; and the guided
  generate_layout(batch_size=1, text);
* the captured step: the guided step (a plan at 2 B, fused dsc_p_sample_cfg_f32) against the same step from the unfused kernels
  (dsc_cfg_combine_f32, dsc_p_sample_f32 and a copy into the null half) and against the unguided step at B, each replayed ``--launches``
  times, microseconds per step, in alternation.
Every variant is warmed up first (capture included), a device synchronise brackets every timed call, medians are reported.  Reads
nothing outside the repository."""
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

B, N, SCALE = 128, 12, 2.0


class _SyntheticBertCache:
    """text_cache.BertFeatureCache protocol over fixed synthetic features: (len(texts), L, 768) on the device."""

    def __init__(self, n, L, device):
        import torch
        self.feats = torch.randn((n, L, 768), generator=torch.Generator().manual_seed(5)).to(device)

    def batch(self, texts, device):
        return self.feats[:len(texts)]


def _model(device):
    import bench
    spec = dict(bench.CONFIGS["text"], batch=B, objects=N)
    model, cfg = bench.build_model(spec, device)
    model.eval()
    model.attach_bert_cache(_SyntheticBertCache(B, spec["text_len"], device))
    return model, cfg, spec


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternate(calls, reps):
    first = {k: _wall(f) for k, f in calls.items()}
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ts[k].append(_wall(f))
    return first, ts


def call_compare(device, reps, strided):
    import torch
    mg, cfg, _ = _model(device)                  # one model per variant: each keeps its own live graph
    mu, _, _ = _model(device)
    C = cfg["point_dim"]
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    text = ["synthetic"] * B
    kw = dict(sampling_timesteps=strided) if strided else {}
    calls = {"guided": lambda: mg.generate_layout_batched(rooms, N, C, B, text=text, clip_denoised=True, guidance_scale=SCALE, **kw),
             "unguided": lambda: mu.generate_layout_batched(rooms, N, C, B, text=text, clip_denoised=True, **kw)}
    first, ts = _alternate(calls, reps)
    out = {"shape": [B, N, C], "steps": strided or 1000, "guidance_scale": SCALE}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"seconds": round(med, 4), "scenes_per_s": round(B / med, 1), "calls": [round(v, 4) for v in ts[k]],
                  "first_call_s": round(first[k], 3)}
    out["guided_over_unguided"] = round(statistics.median(ts["guided"]) / statistics.median(ts["unguided"]), 4)
    return out


def single_scene(device, reps):
    import torch
    m, cfg, _ = _model(device)
    C = cfg["point_dim"]
    room = torch.zeros(1, 1, 64, 64, device=device)
    calls = {"guided": lambda: m.generate_layout(room, N, C, batch_size=1, text=["synthetic"], clip_denoised=True, guidance_scale=SCALE)}
    first, ts = _alternate(calls, reps)
    med = statistics.median(ts["guided"])
    return {"shape": [1, N, C], "steps": 1000, "seconds": round(med, 4), "calls": [round(v, 4) for v in ts["guided"]],
            "first_call_s": round(first["guided"], 3)}


def step_compare(device, step_reps, launches):
    """Microseconds per captured step: guided fused, guided unfused, unguided at B."""
    import torch
    from diffuscene_amd.sampler import _GuidedStepGraph, _StepGraph
    m, cfg, spec = _model(device)
    C = cfg["point_dim"]
    gd, net = m.diffusion.diffusion, m.diffusion.model
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        cond, cross = m._sampling_conditions(rooms, N, device, text=["synthetic"] * B)
        cond2, cross2, scale = gd._guided_inputs((B, N, C), device, cond, cross, SCALE, "bench_cfg")
        graphs = {"guided_fused": _GuidedStepGraph(gd, net, (B, N, C), device, cond2, cross2, True, fused=True),
                  "guided_unfused": _GuidedStepGraph(gd, net, (B, N, C), device, cond2, cross2, True, fused=False),
                  "unguided": _StepGraph(gd, net, (B, N, C), device, cond, cross, True)}
    for name, g in graphs.items():
        if name != "unguided":
            g.scale.copy_(scale)

    def run(name):
        g = graphs[name]
        g.x2.normal_() if name != "unguided" else g.x.normal_()
        g.t.fill_(launches)                      # counts down in the graph: stays inside the schedule for the whole timed region
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
    out["fused_minus_unfused_us"] = round(med["guided_fused"] - med["guided_unfused"], 2)
    out["unfused_spread_us"] = round(max(ts["guided_unfused"]) - min(ts["guided_unfused"]), 2)
    out["guided_over_unguided_step"] = round(med["guided_fused"] / med["unguided"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--only", default=None, help="comma list of: steps, tstep, strided, single")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfg_bench.json"))
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_cfg.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else {"steps", "tstep", "strided", "single"}
    out = {"tool": "tools/bench_cfg.py", "T": 1000, "git_head": __import__("bench").git_head()}
    if "steps" in only:
        out["step_b%d_n%d" % (B, N)] = step_compare(device, a.step_reps, a.launches)
        torch.cuda.empty_cache()
    if "tstep" in only:
        out["tstep_b%d_n%d" % (B, N)] = call_compare(device, a.reps, None)
        torch.cuda.empty_cache()
    if "strided" in only:
        out["s50_b%d_n%d" % (B, N)] = call_compare(device, a.reps, 50)
        torch.cuda.empty_cache()
    if "single" in only:
        out["tstep_b1_n%d" % N] = single_scene(device, a.reps)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
