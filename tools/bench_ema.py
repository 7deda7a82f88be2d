#!/usr/bin/env python
"""What the weight EMA costs, on the work list of the 77.7 M-parameter denoiser, in one process (bench.py is not touched).

    python tools/bench_ema.py [--reps 7] [--calls 10] [--out profiles/ema_bench.json]        -> one JSON line on stdout

Four ways to take an optimizer step, on the same parameters and gradients, timed in alternation:
* ``adam``:        ``FusedAdam.step()`` with ``ema_decay=None`` -- dsc_adam_step_f32, the code path without this feature (28 B/parameter);
* ``adam_ema``:    ``FusedAdam(ema_decay=0.9999).step()`` -- dsc_adam_ema_step_f32, the average kept in the same sweep (36 B/parameter);
* ``adam+update``: ``FusedAdam.step()`` then ``ParamEMA.update()`` -- dsc_adam_step_f32 + dsc_ema_update_f32 (28 + 12 B/parameter);
* ``adam+lerp``:   ``FusedAdam.step()`` then ``torch._foreach_lerp_`` on a copy of the parameters, what a user had to write before.
``graph_us``: ``--calls`` steps captured into one hipGraph and replayed between device events, per step (the kernels back to back);
``eager_us``: the same calls from Python between two synchronisations on the host clock, per step (what a training loop that does
nothing else would see; bounded below by the host cost of ``step()``).  Medians over ``--reps`` rounds, with min and max.
``gb_per_s`` is bytes from the parameter count over the graph time.  ``swap``: ``ema_swap()`` + ``DenoiserEngine.refresh()`` (standardised
weights, packed time MLPs, bf16 planes re-derived), the price of entering or leaving ``ema_weights()``, host clock around a synchronise.
Every variant is warmed up first; there is no fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tools")):
    if path not in sys.path:
        sys.path.insert(0, path)

DECAY = 0.9999
BYTES = {"adam": 28, "adam_ema": 36, "adam+update": 40}        # per parameter, from the kernels' reads and writes


def _stats(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--config", default="living80")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ema.py needs a GPU")
    import bench
    from bench_ddim_complete import shader_clock
    from diffuscene_amd.optim import FusedAdam, ParamEMA
    device = torch.device("cuda:0")
    spec = bench.CONFIGS[args.config]
    model, _ = bench.build_model(spec, device)
    params = [p for p in model.parameters() if p.requires_grad]
    n_param = sum(p.numel() for p in params)
    g = torch.Generator(device=device).manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, device=device, generator=g) * 1e-3

    plain = FusedAdam(params, lr=1e-5)
    fused = FusedAdam(params, lr=1e-5, ema_decay=DECAY)
    with_update, ema = FusedAdam(params, lr=1e-5), ParamEMA(params, DECAY)
    with_lerp = FusedAdam(params, lr=1e-5)
    copies = [p.detach().clone() for p in params]
    raw = [p.detach() for p in params]

    def step_update():
        with_update.step()
        ema.update()

    def step_lerp():
        with_lerp.step()
        torch._foreach_lerp_(copies, raw, 1.0 - DECAY)

    variants = {"adam": plain.step, "adam_ema": fused.step, "adam+update": step_update, "adam+lerp": step_lerp}
    graphs = {}
    for name, fn in variants.items():
        for _ in range(3):                                      # warm-up: state, work lists and their upload
            fn()
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream(device).wait_stream(side)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(args.calls):
                fn()
        graphs[name].replay()
    torch.cuda.synchronize()

    def graph_us(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graphs[name].replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.calls

    def eager_us(name):
        fn = variants[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.calls

    times = {name: {"graph_us": [], "eager_us": []} for name in variants}
    for _ in range(args.reps):                                  # in alternation: drift and neighbours hit every variant alike
        for name in variants:
            times[name]["graph_us"].append(graph_us(name))
        for name in variants:
            times[name]["eager_us"].append(eager_us(name))
    res = {}
    for name in variants:
        res[name] = {k: _stats(v) for k, v in times[name].items()}
        if name in BYTES:
            res[name]["bytes_per_param"] = BYTES[name]
            res[name]["gb_per_s"] = round(BYTES[name] * n_param / (res[name]["graph_us"]["median"] * 1e-6) / 1e9, 1)
    base = res["adam"]["graph_us"]["median"]
    ratios = {name: round(res[name]["graph_us"]["median"] / base, 4) for name in variants}

    # one swap + the re-derivation the next model call pays
    B, N, C = 2, spec["objects"], 8 + spec["class_dim"] + 32
    net = model.diffusion.model
    with torch.no_grad():
        net(torch.zeros(B, N, C, device=device), torch.zeros(B, dtype=torch.int64, device=device), model._instance_condition(B, device), None)
    engine = net.engine(device)
    swaps, refreshes = [], []
    for _ in range(2 * max(2, args.reps // 2)):                 # an even number: the weights end where they were
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fused.ema_swap()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        engine.refresh()
        torch.cuda.synchronize()
        swaps.append((t1 - t0) * 1e6)
        refreshes.append((time.perf_counter() - t1) * 1e6)
    assert not fused.ema_swapped

    out = {"tool": "tools/bench_ema.py", "git_head": bench.git_head(), "device": torch.cuda.get_device_name(0), "config": args.config,
           "parameters": n_param, "tensors": len(params), "ema_decay": DECAY, "calls_per_measurement": args.calls, "reps": args.reps,
           "step": res, "graph_time_over_adam": ratios, "expected_fused_over_adam_from_bytes": round(36 / 28, 4),
           "swap": {"ema_swap_us": _stats(swaps[1:]), "engine_refresh_us": _stats(refreshes[1:]), "bytes_per_param": 16},
           "shader_clock": shader_clock()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
