#!/usr/bin/env python
"""The floor-plan encoder (networks/feature_extractors.py) beside the work it conditions, in one process (bench.py is not touched).

    python tools/bench_floorplan.py [--reps 5]        -> one JSON line on stdout, the same record in profiles/floorplan_bench.json

* the encoder alone at B = 128 and 256 on 64 x 64 masks: forward (no grad, as sampling runs it) and forward plus backward, milliseconds;
* the five new kernel families at the shapes they take inside that encoder, microseconds per launch and achieved bandwidth (bytes the
  launch must read and write / time; launch latency included, issued ``--launches`` times back to back);
* generate_layout_batched(128) at N = 12 with and without the conditioning, T = 1000 and S = 50, in alternation;
* one training step (train_on_batch, Adam) on the autograd path at B = 256, N = 80 with and without the encoder, in alternation, and the
  same unconditioned model on the static plan for scale.
Expectations this tool confirms or refutes (none is a pass / fail number): the encoder costs a few percent of a training step and is
invisible beside a sampling loop.  The weights are synthetic and the masks are rectangles: nothing here says anything about the quality
of conditioned scenes.  Every variant is warmed up first, a device synchronise brackets every timed call, medians are reported, the
driver's shader clock level is read after the measurements.  Reads nothing outside the repository."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_steer import _wall  # noqa: E402

SIDE, FEATURE, LATENT = 64, 64, 64


def room_masks(b, device):
    import torch
    m = torch.zeros(b, 1, SIDE, SIDE)
    for i in range(b):
        m[i, 0, 4 + i % 9:SIDE - 6 - i % 7, 5 + i % 5:SIDE - 4 - i % 11] = 1.0
    return m.to(device)


def build(device, n, kw_name, class_dim, room):
    """The benchmark's model (bench.build_model) with or without ``room_mask_condition``."""
    import torch
    from diffuscene_amd import workloads as W
    from diffuscene_amd.flat import ensure_flat
    from diffuscene_amd.networks import build_network
    stats = os.path.join(tempfile.mkdtemp(), "dataset_stats.txt")
    with open(stats, "w") as f:
        json.dump(W.DATASET_STATS, f)
    kw = dict(getattr(W, kw_name))
    kw["instanclass_dim"] = 128 + (LATENT if room else 0)
    net = {"type": "diffusion_scene_layout_ddpm", "net_type": "unet1d", "point_dim": 8 + class_dim + 32, "latent_dim": LATENT if room else 0,
           "room_mask_condition": room, "sample_num_points": n, "objectness_dim": 0, "objfeat_dim": 32, "class_dim": class_dim,
           "angle_dim": 2, "learnable_embedding": True, "instance_condition": True, "instance_emb_dim": 128,
           "diffusion_kwargs": dict(schedule_type="linear", beta_start=1e-4, beta_end=0.02, time_num=1000, loss_type="mse",
                                    model_mean_type="v", model_var_type="fixedsmall", loss_separate=True, loss_iou=True,
                                    train_stats_file=stats),
           "net_kwargs": kw}
    cfg = {"network": net, "feature_extractor": dict(name="resnet18", freeze_bn=True, input_channels=1, feature_size=FEATURE)}
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model, train, _ = build_network(net["point_dim"], class_dim + 1, cfg, device=device)
    ensure_flat(model)
    return model, net, train


def _alternate(calls, reps):
    first = {k: _wall(f) for k, f in calls.items()}
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            ts[k].append(_wall(f))
    return first, ts


def encoder_alone(device, reps):
    import torch
    from diffuscene_amd.networks.feature_extractors import get_feature_extractor
    torch.manual_seed(0)
    enc = get_feature_extractor("resnet18", freeze_bn=True, input_channels=1, feature_size=FEATURE).to(device)
    out = {}
    for b in (128, 256):
        x = room_masks(b, device)
        g = torch.randn(b, FEATURE, device=device)

        def fwd():
            with torch.no_grad():
                enc(x)

        def fwd_bwd():
            for p in enc.parameters():
                p.grad = None
            enc(x).backward(g)

        _, ts = _alternate({"forward": fwd, "forward_backward": fwd_bwd}, reps)
        out["b%d" % b] = {k: {"ms": round(statistics.median(v) * 1e3, 3), "all_ms": [round(t * 1e3, 3) for t in v]} for k, v in ts.items()}
        out["b%d" % b]["gflop_forward"] = round(0.15 * b, 1)
        torch.cuda.empty_cache()
    return out


def kernels(device, launches, reps):
    """Each kernel family at a shape it takes inside the 64 x 64 encoder: (name, bytes moved, launcher)."""
    import torch
    from diffuscene_amd import ops
    out = {}
    for b in (128, 256):
        f = lambda *s: torch.rand(*s, device=device) + 0.5                   # noqa: E731
        x1, x64 = f(b * 64 * 64, 1), f(b * 16 * 16, 64)
        p1 = torch.empty(b * 32 * 32, ops.conv_kpad(1, 7), device=device)
        p64 = torch.empty(b * 16 * 16, ops.conv_kpad(64, 3), device=device)
        dx64 = torch.empty_like(x64)
        s32 = f(b * 32 * 32, 64)
        y32 = torch.empty_like(s32)
        py, pa = torch.empty(b * 16 * 16, 64, device=device), torch.empty(b * 16 * 16, 64, device=device, dtype=torch.uint8)
        pdx = torch.empty_like(s32)
        w = [f(64) for _ in range(4)]
        bouts = (torch.empty_like(s32), torch.empty_like(s32), torch.empty(64, device=device), torch.empty(64, device=device))
        a512, am, adx = f(b * 4, 512), torch.empty(b, 512, device=device), torch.empty(b * 4, 512, device=device)
        cases = {
            "conv_patches_7x7s2_c1": (4 * (x1.numel() + p1.numel()), lambda: ops.conv_patches(x1, (b, 64, 64), 7, 2, 3, out=p1)),
            "conv_patches_3x3s1_c64": (4 * (x64.numel() + p64.numel()), lambda: ops.conv_patches(x64, (b, 16, 16), 3, 1, 1, out=p64)),
            "conv_patches_bwd_3x3s1_c64": (4 * (p64.numel() + dx64.numel()), lambda: ops.conv_patches_bwd(p64, (b, 16, 16), 64, 3, 1, 1, out=dx64)),
            "maxpool2d_c64": (4 * s32.numel() + 5 * py.numel(), lambda: ops.maxpool2d(s32, (b, 32, 32), out=py, arg=pa)),
            "maxpool2d_bwd_c64": (5 * py.numel() + 4 * pdx.numel(), lambda: ops.maxpool2d_bwd(py, pa, (b, 32, 32), out=pdx)),
            "frozen_bn_act_res_relu_c64": (4 * 3 * s32.numel(), lambda: ops.frozen_bn_act(s32, *w, residual=s32, relu=True, out=y32)),
            "frozen_bn_act_bwd_res_relu_c64": (4 * 5 * s32.numel(), lambda: ops.frozen_bn_act_bwd(s32, y32, s32, w[0], w[2], w[3], relu=True,
                                                                                                    want_residual=True, outs=bouts)),
            "avgpool_rows_c512": (4 * (a512.numel() + am.numel()), lambda: ops.avgpool_rows(a512, b, out=am)),
            "avgpool_rows_bwd_c512": (4 * (am.numel() + adx.numel()), lambda: ops.avgpool_rows_bwd(am, 4, out=adx)),
        }
        rec = {}
        for name, (nbytes, fn) in cases.items():
            def many(fn=fn):
                for _ in range(launches):
                    fn()
            many()
            us = statistics.median([_wall(many) for _ in range(reps)]) / launches * 1e6
            rec[name] = {"us": round(us, 2), "mbytes": round(nbytes / 1e6, 2), "gb_per_s": round(nbytes / us / 1e3, 1)}
        out["b%d" % b] = rec
        del cases
        torch.cuda.empty_cache()
    return out


def sampling(device, reps, strided):
    import torch
    b, n = 128, 12
    mr, cfg, _ = build(device, n, "UNCOND_BEDROOM", 22, True)
    mu, _, _ = build(device, n, "UNCOND_BEDROOM", 22, False)
    mr.eval(), mu.eval()
    rooms = room_masks(b, device)
    kw = dict(sampling_timesteps=strided) if strided else {}
    calls = {"conditioned": lambda: mr.generate_layout_batched(rooms, n, cfg["point_dim"], b, clip_denoised=True, **kw),
             "unconditioned": lambda: mu.generate_layout_batched(rooms, n, cfg["point_dim"], b, clip_denoised=True, **kw)}
    first, ts = _alternate(calls, reps)
    out = {"shape": [b, n, cfg["point_dim"]], "steps": strided or 1000, "mask": [SIDE, SIDE]}
    for k in calls:
        med = statistics.median(ts[k])
        out[k] = {"seconds": round(med, 4), "scenes_per_s": round(b / med, 1), "calls": [round(v, 4) for v in ts[k]],
                  "first_call_s": round(first[k], 3)}
    out["conditioned_over_unconditioned"] = round(statistics.median(ts["conditioned"]) / statistics.median(ts["unconditioned"]), 4)
    torch.cuda.empty_cache()
    return out


def training(device, reps):
    import torch
    from diffuscene_amd import workloads as W
    from diffuscene_amd.networks import optimizer_factory
    b, n, nc = 256, 80, 25
    x = W.synth_scene_batch(b, n, nc, 32, seed=1).to(device)
    batch = {"translations": x[:, :, 0:3].contiguous(), "sizes": x[:, :, 3:6].contiguous(), "angles": x[:, :, 6:8].contiguous(),
             "class_labels": x[:, :, 8:8 + nc].contiguous(), "objfeats_32": x[:, :, 8 + nc:].contiguous(),
             "room_layout": room_masks(b, device)}
    tcfg = {"training": {"max_grad_norm": 10}}
    arms = {}
    for name, room, plan in (("autograd_with_encoder", True, "0"), ("autograd_without_encoder", False, "0"), ("plan_without_encoder", False, "1")):
        model, _, train = build(device, n, "UNCOND_LIVING", nc, room)
        opt = optimizer_factory({"optimizer": "Adam", "lr": 2e-4}, filter(lambda p: p.requires_grad, model.parameters()))

        def step(model=model, opt=opt, train=train, plan=plan):
            os.environ["DSC_TRAIN_PLAN"] = plan
            try:
                train(model, opt, batch, tcfg)
            finally:
                os.environ.pop("DSC_TRAIN_PLAN", None)
        arms[name] = step
    for f in arms.values():
        _wall(f)                                   # warm-up beyond the first call _alternate takes: plans, graphs, optimizer state
    _, ts = _alternate(arms, reps)
    med = {k: statistics.median(v) for k, v in ts.items()}
    out = {"shape": [b, n, 8 + nc + 32], "mask": [SIDE, SIDE]}
    for k, v in ts.items():
        out[k] = {"ms": round(med[k] * 1e3, 2), "all_ms": [round(t * 1e3, 2) for t in v]}
    out["encoder_share_of_autograd_step"] = round((med["autograd_with_encoder"] - med["autograd_without_encoder"]) / med["autograd_with_encoder"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--only", default=None, help="comma list of: encoder, kernels, tstep, strided, train")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floorplan_bench.json"))
    a = ap.parse_args()
    import torch
    from diffuscene_amd import _lib
    try:
        _lib.load()
    except _lib.HipLibraryMissing:          # a fresh checkout: compile first
        import __graft_entry__
        __graft_entry__.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_floorplan.py measures on a HIP device; none is visible")
    device = torch.device("cuda:0")
    from bench_ddim_complete import shader_clock
    only = set(a.only.split(",")) if a.only else {"encoder", "kernels", "tstep", "strided", "train"}
    out = {"tool": "tools/bench_floorplan.py", "git_head": __import__("bench").git_head(), "weights": "synthetic"}
    if "encoder" in only:
        out["encoder_64x64"] = encoder_alone(device, a.reps)
    if "kernels" in only:
        out["kernels"] = kernels(device, a.launches, a.reps)
    if "strided" in only:
        out["s50_b128_n12"] = sampling(device, max(2, a.reps // 2), 50)
    if "tstep" in only:
        out["tstep_b128_n12"] = sampling(device, 2, None)
    if "train" in only:
        out["train_b256_n80"] = training(device, a.reps)
    out["shader_clock"] = shader_clock()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
