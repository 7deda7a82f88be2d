#!/usr/bin/env python
"""Text-guided in-painting against its two neighbours, through the public entry points, in one process (bench.py is not touched).

    python tools/bench_guided_inpaint.py [--reps 3] [--step-reps 7]     -> one JSON line on stdout, the same record in
                                                                           profiles/guided_inpaint_bench.json

At bench.py's ``text`` configuration (B = 128, N = 12, L = 32 cached BERT rows per scene), every pair in alternation in the same process,
so the yardstick is the variant beside it, not an earlier run:
* the captured step, microseconds per replayed step: the guided masked step (a plan at 2 B, fused dsc_p_sample_masked_cfg_f32, the main
  draw and the known-draw) against the same step from the unfused kernels (dsc_cfg_combine_f32, dsc_p_sample_masked_f32 and a copy into the
  null half), and against the guided generation step (_GuidedStepGraph: fused dsc_p_sample_cfg_f32, the main draw only);
* the calls: inpaint_scene_batched(guidance_scale=2) against generate_layout_batched(guidance_scale=2) for the T-step loop (T = 1000) and
  for S = 50.  About 30 % of the elements are given.
Every variant is warmed up first (capture included), a device synchronise brackets every timed call; medians and the spread (max - min
over the repetitions) are reported.  No threshold is set here: the numbers are recorded in DESIGN.md.  Reads nothing outside the
repository."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_cfg import B, N, SCALE, _alternate, _model, _wall  # noqa: E402

GIVEN = 0.3


def _given(C, device):
    """(known (B, N, C) in [-1, 1], mask (B, N, C) bool with about GIVEN of the elements set), seeded."""
    import torch
    g = torch.Generator().manual_seed(9)
    known = (torch.rand((B, N, C), generator=g) * 2 - 1).to(device)
    return known, (torch.rand((B, N, C), generator=g) < GIVEN).to(device)


def _spread(v):
    return max(v) - min(v)


def call_compare(device, reps, strided):
    import torch
    mi, cfg, _ = _model(device)                  # one model per variant: each keeps its own live graph
    mg, _, _ = _model(device)
    C = cfg["point_dim"]
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    text = ["synthetic"] * B
    known, mask = _given(C, device)
    kw = dict(sampling_timesteps=strided) if strided else {}
    calls = {"guided_inpaint": lambda: mi.inpaint_scene_batched(rooms, N, C, known, mask, text=text, clip_denoised=True,
                                                                guidance_scale=SCALE, **kw),
             "guided_generate": lambda: mg.generate_layout_batched(rooms, N, C, B, text=text, clip_denoised=True, guidance_scale=SCALE, **kw)}
    first, ts = _alternate(calls, reps)
    out = {"shape": [B, N, C], "steps": strided or 1000, "guidance_scale": SCALE, "given_fraction": round(float(mask.float().mean()), 3)}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"seconds": round(med, 4), "scenes_per_s": round(B / med, 1), "calls": [round(v, 4) for v in ts[k]],
                  "spread_s": round(_spread(ts[k]), 4), "first_call_s": round(first[k], 3)}
    out["inpaint_over_generate"] = round(statistics.median(ts["guided_inpaint"]) / statistics.median(ts["guided_generate"]), 4)
    return out


def step_compare(device, step_reps, launches):
    """Microseconds per captured step: guided masked fused, guided masked unfused, guided generation."""
    import torch
    from diffuscene_amd import ops
    from diffuscene_amd.sampler import _GuidedStepGraph, _MaskedGuidedGraph
    m, cfg, spec = _model(device)
    C = cfg["point_dim"]
    gd, net = m.diffusion.diffusion, m.diffusion.model
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    known, mask = _given(C, device)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        cond, cross = m._sampling_conditions(rooms, N, device, text=["synthetic"] * B)
        cond2, cross2, scale = gd._guided_inputs((B, N, C), device, cond, cross, SCALE, "bench_guided_inpaint")
        graphs = {"masked_fused": _MaskedGuidedGraph(gd, net, (B, N, C), device, cond2, cross2, True, fused=True),
                  "masked_unfused": _MaskedGuidedGraph(gd, net, (B, N, C), device, cond2, cross2, True, fused=False),
                  "generation": _GuidedStepGraph(gd, net, (B, N, C), device, cond2, cross2, True, fused=True)}
    for name, g in graphs.items():
        g.scale.copy_(scale)
        if name != "generation":
            g.known.copy_(known)
            g.mask.copy_(ops.known_mask(mask, (B, N, C), device))

    def run(name):
        g = graphs[name]
        g.x2.normal_()
        g.t.fill_(launches)                      # counts down in the graph: stays inside the schedule for the whole timed region
        return _wall(lambda: g.replay_steps(launches)) / launches * 1e6

    for name in graphs:
        run(name)
    ts = {name: [] for name in graphs}
    for _ in range(step_reps):
        for name in ts:
            ts[name].append(run(name))
    med = {k: statistics.median(v) for k, v in ts.items()}
    out = {"shape": [B, N, C], "launches": launches, "given_fraction": round(float(mask.float().mean()), 3)}
    for k in ts:
        out[k + "_us_per_step"] = round(med[k], 2)
        out[k + "_all"] = [round(v, 2) for v in ts[k]]
        out[k + "_spread_us"] = round(_spread(ts[k]), 2)
    out["fused_minus_unfused_us"] = round(med["masked_fused"] - med["masked_unfused"], 2)
    out["masked_minus_generation_us"] = round(med["masked_fused"] - med["generation"], 2)
    out["masked_over_generation_step"] = round(med["masked_fused"] / med["generation"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--only", default=None, help="comma list of: steps, tstep, strided")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_inpaint_bench.json"))
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_guided_inpaint.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else {"steps", "tstep", "strided"}
    out = {"tool": "tools/bench_guided_inpaint.py", "T": 1000, "git_head": __import__("bench").git_head()}
    if "steps" in only:
        out["step_b%d_n%d" % (B, N)] = step_compare(device, a.step_reps, a.launches)
        torch.cuda.empty_cache()
    if "tstep" in only:
        out["tstep_b%d_n%d" % (B, N)] = call_compare(device, a.reps, None)
        torch.cuda.empty_cache()
    if "strided" in only:
        out["s50_b%d_n%d" % (B, N)] = call_compare(device, a.reps, 50)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
