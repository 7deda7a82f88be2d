#!/usr/bin/env python
"""Attribute-level in-painting against plain generation, through the public entry points, in one process (bench.py is not touched).

    python tools/bench_edit.py [--reps 3] [--step-reps 7]        -> one JSON line on stdout

* fused against unfused step: dsc_p_sample_masked_f32 against dsc_p_sample_f32 + dsc_masked_overwrite_f32 (what the eager loop launches),
  each captured ``--launches`` times into a hipGraph and replayed, microseconds per step at (128, 80, C) and (64, 12, C), for an
  all-free mask (the traffic of p_sample plus one byte per element) and for the 'sizes | classes | objfeats' mask; the two variants are
  timed in alternation, ``unfused_spread_us`` is max - min over the unfused repetitions;
* the calls: inpaint_scene_batched ('sizes | class_labels | objfeats' of every row given) against generate_layout_batched of the same
  model configuration at B = 128, N = 80 and at B = 64, N = 12, for the T-step loop (T = 1000) and S = 50, in alternation in the same
  process -- the yardstick is the generation call beside it, not an earlier run.
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

SHAPES = ((128, 80, "complete"), (64, 12, "bedroom21"))
KNOWN = ("sizes", "class_labels", "objfeats")


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


def step_compare(device, B, N, C, mask, step_reps, launches):
    """Microseconds per step: one fused launch against p_sample + masked_overwrite, both replayed from a graph of ``launches`` steps."""
    import torch
    from diffuscene_amd import ops
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    gd = GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, 1000),
                           "mse", "v", "fixedsmall", False, False, None)
    tb = gd.tables(device)
    ca, cb = gd._coeffs(tb)
    sa, sb, k1, k2, sg = (tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"], tb["posterior_mean_coef1"],
                          tb["posterior_mean_coef2"], gd._sigma(tb))
    g = torch.Generator(device=device).manual_seed(3)
    x, mo, noise, known, nk = (torch.randn((B, N, C), device=device, generator=g) for _ in range(5))
    t = torch.full((B,), 500, dtype=torch.int64, device=device)
    tm1 = t - 1
    out = torch.empty_like(x)

    def fused():
        ops.p_sample_masked(x, mo, noise, known, nk, mask, t, ca, cb, k1, k2, sg, sa, sb, ops.MEAN_V, True, out=out)

    def unfused():
        ops.p_sample(x, mo, noise, t, ca, cb, k1, k2, sg, ops.MEAN_V, True, out=out)
        ops.masked_overwrite(out, known, nk, mask, tm1, sa, sb)

    graphs = {}
    for name, fn in (("fused", fused), ("unfused", unfused)):
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream(device).wait_stream(side)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(launches):
                fn()

    def run(name):
        return _wall(graphs[name].replay) / launches * 1e6

    for name in graphs:
        run(name)
    ts = {"fused": [], "unfused": []}
    for _ in range(step_reps):
        for name in ts:
            ts[name].append(run(name))
    fm, um = statistics.median(ts["fused"]), statistics.median(ts["unfused"])
    spread = max(ts["unfused"]) - min(ts["unfused"])
    return {"fused_us_per_step": round(fm, 2), "unfused_us_per_step": round(um, 2), "fused_all": [round(v, 2) for v in ts["fused"]],
            "unfused_all": [round(v, 2) for v in ts["unfused"]], "unfused_spread_us": round(spread, 2),
            "fused_minus_unfused_us": round(fm - um, 2), "given_share": round(float((mask != 0).float().mean()), 4)}


def call_compare(device, B, N, config, reps, strided):
    import bench
    import torch
    from diffuscene_amd import workloads as W
    spec = dict(bench.CONFIGS[config], batch=B, objects=N)
    mi, cfg = _model(spec, device)
    mg, _ = _model(spec, device)
    C = cfg["point_dim"]
    x = W.synth_scene_batch(B, N, spec["class_dim"], 32, 7).to(device)
    rooms = torch.zeros(B, 1, 64, 64, device=device)
    mask = mi.attribute_mask(N, KNOWN, B, N)
    kw = dict(sampling_timesteps=strided) if strided else {}
    calls = {"inpaint_scene_batched": lambda: mi.inpaint_scene_batched(rooms, N, C, x, mask, clip_denoised=True, **kw),
             "generate_layout_batched": lambda: mg.generate_layout_batched(rooms, N, C, B, clip_denoised=True, **kw)}
    first = {k: _wall(f) for k, f in calls.items()}
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ts[k].append(_wall(f))
    out = {"shape": [B, N, C], "steps": strided or 1000, "known": "|".join(KNOWN)}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"seconds": round(med, 4), "scenes_per_s": round(B / med, 1), "calls": [round(v, 4) for v in ts[k]],
                  "first_call_s": round(first[k], 3)}
    out["inpaint_over_generation"] = round(statistics.median(ts["inpaint_scene_batched"]) / statistics.median(ts["generate_layout_batched"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--only", default=None, help="comma list of: steps, tstep, strided")
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_edit.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    only = set(a.only.split(",")) if a.only else {"steps", "tstep", "strided"}
    out = {"tool": "tools/bench_edit.py", "T": 1000, "git_head": __import__("bench").git_head()}
    for B, N, config in SHAPES:
        tag = "b%d_n%d" % (B, N)
        if "steps" in only:
            C = 62 if N == 12 else 65
            zero = torch.zeros((B, N, C), dtype=torch.uint8, device=device)
            attr = zero.clone()
            attr[:, :, 3:6] = 1
            attr[:, :, 8:] = 1
            out["step_all_free_" + tag] = step_compare(device, B, N, C, zero, a.step_reps, a.launches)
            out["step_sizes_classes_objfeats_" + tag] = step_compare(device, B, N, C, attr, a.step_reps, a.launches)
        if "tstep" in only:
            out["tstep_" + tag] = call_compare(device, B, N, config, a.reps, None)
            torch.cuda.empty_cache()
        if "strided" in only:
            out["s50_" + tag] = call_compare(device, B, N, config, a.reps, 50)
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
