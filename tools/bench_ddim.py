#!/usr/bin/env python
"""DDIM against DDPM through the public sampling entry points, in one process (bench.py is not touched).

    python tools/bench_ddim.py [--reps 3] [--kernel-db trace/x_results.db]        -> one JSON line on stdout
    rocprofv3 --kernel-trace --stats -d trace -o x -- python tools/bench_ddim.py --trace-only    (the separate kernel-trace run)

* generate_layout(batch_size=1) -- the call shape of scripts/generate_diffusion.py -- seconds per scene at N = 12 and N = 21, for the
  T = 1000 DDPM loop and DDIM with S in {250, 100, 50} (eta = 0);
* generate_layout_batched(256) at N = 80 (the metric shape), scenes per second, DDIM S = 50 against DDPM.
Every variant has its own model (identical seeded weights): the graph cache keeps one live graph per model, so alternating variants
on one model would time a capture per call.  Each variant is warmed up (capture) first, then the variants are timed in alternation,
with a device synchronise around every call; the median is reported.  ``--kernel-db`` adds the DDIM step kernel's line of a rocprofv3
trace of ``--trace-only`` (warm-up, then one batched S = 50 call): achieved HBM bytes/s of the step (3 fp32 reads + 1 write per element)
against the 8.0 TB/s peak of the MI355X."""
import argparse
import contextlib
import io
import json
import os
import sqlite3
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec (about 6.3e12 achievable with a streaming copy)
VARIANTS = (None, 250, 100, 50)


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


def per_scene(device, N, reps):
    import bench
    import torch
    spec = dict(bench.CONFIGS["bedroom21"], batch=1, objects=N)
    room = torch.zeros(1, 1, 64, 64, device=device)
    calls = {}
    for S in VARIANTS:
        model, cfg = _model(spec, device)
        calls[S] = (lambda m=model, c=cfg, S=S: m.generate_layout(room_mask=room, num_points=N, point_dim=c["point_dim"], batch_size=1,
                                                                  device="cpu", clip_denoised=True, sampling_timesteps=S))
    first = {S: _wall(calls[S]) for S in VARIANTS}
    ts = {S: [] for S in VARIANTS}
    for _ in range(reps):
        for S in VARIANTS:
            ts[S].append(_wall(calls[S]))
    row = {}
    ddpm = statistics.median(ts[None])
    for S in VARIANTS:
        med = statistics.median(ts[S])
        row["ddpm_T1000" if S is None else "ddim_S%d" % S] = {"seconds_per_scene": round(med, 4), "first_call_s": round(first[S], 3),
                                                               "network_evaluations": 1000 if S is None else S,
                                                               "speedup_over_ddpm": round(ddpm / med, 2)}
    return row


def batched(device, reps, S=50):
    import bench
    import torch
    spec = dict(bench.CONFIGS["living80"])
    B, N = spec["batch"], spec["objects"]
    room = torch.zeros(B, 1, 64, 64, device=device)
    calls = {}
    for s in (None, S):
        model, cfg = _model(spec, device)
        calls[s] = (lambda m=model, c=cfg, s=s: m.generate_layout_batched(room_mask=room, num_points=N, point_dim=c["point_dim"],
                                                                          batch_size=B, clip_denoised=True, sampling_timesteps=s))
    for s in calls:
        _wall(calls[s])
    ts = {s: [] for s in calls}
    for _ in range(reps):
        for s in calls:
            ts[s].append(_wall(calls[s]))
    med = {s: statistics.median(v) for s, v in ts.items()}
    return {"workload": "uncond living rooms, generate_layout_batched(batch_size=%d), N=%d" % (B, N),
            "ddpm_T1000": {"seconds": round(med[None], 3), "scenes_per_s": round(B / med[None], 1)},
            "ddim_S%d" % S: {"seconds": round(med[S], 4), "scenes_per_s": round(B / med[S], 1)},
            "speedup": round(med[None] / med[S], 2)}


# dsc_ddim_step_f32 launches step_kernel<STRIDED = true, GIVEN = none, GUIDED = false> (csrc/diffusion.hip); demangled or mangled name
DDIM_STEP_KERNEL = "(name like '%step_kernel<true, 0, false>%' or name like '%step_kernelILb1ELi0ELb0E%')"


def kernel_line(db, B=256, N=80, C=65):
    con = sqlite3.connect(db)
    cur = con.cursor()
    r = cur.execute("select count(*), avg(end-start), min(end-start), max(end-start) from kernels where " + DDIM_STEP_KERNEL).fetchone()
    if not r or not r[0]:
        return {"error": "no step_kernel<true, 0, false> dispatch in %s" % db}
    n, avg_ns, mn, mx = r
    full = cur.execute("select count(*), avg(end-start) from kernels where " + DDIM_STEP_KERNEL + " and end-start > ?",
                       (0.5 * avg_ns,)).fetchone()
    elems = B * N * C
    bytes_step = 4 * elems * 4            # x_t, model output, noise read; x written
    tl = cur.execute("select min(start), max(end), sum(end-start), count(*) from kernels").fetchone()
    return {"kernel": "step_kernel<true, 0, false>", "dispatches": n, "avg_us": round(avg_ns / 1e3, 2), "min_us": round(mn / 1e3, 2),
            "max_us": round(mx / 1e3, 2), "shape": [B, N, C], "bytes_per_step": bytes_step,
            "achieved_TBps": round(bytes_step / (mn * 1e-9) / 1e12, 2), "achieved_TBps_avg": round(bytes_step / (avg_ns * 1e-9) / 1e12, 2),
            "hbm_peak_TBps": HBM_PEAK / 1e12, "fraction_of_peak_best": round(bytes_step / (mn * 1e-9) / HBM_PEAK, 3),
            "traced_span_ms": round((tl[1] - tl[0]) / 1e6, 2), "kernel_busy_ms": round(tl[2] / 1e6, 2), "traced_dispatches": tl[3],
            "note": "%d dispatches above half the mean" % full[0]}


def trace_only(device):
    """What the kernel trace records: one warm-up (capture) and one timed batched S = 50 call."""
    import bench
    import torch
    spec = dict(bench.CONFIGS["living80"])
    model, cfg = _model(spec, device)
    room = torch.zeros(spec["batch"], 1, 64, 64, device=device)
    for _ in range(2):
        _wall(lambda: model.generate_layout_batched(room_mask=room, num_points=spec["objects"], point_dim=cfg["point_dim"],
                                                    batch_size=spec["batch"], clip_denoised=True, sampling_timesteps=50))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-db", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch
    import __graft_entry__
    __graft_entry__.build()
    device = torch.device("cuda:0")
    if a.trace_only:
        trace_only(device)
        return
    out = {"tool": "tools/bench_ddim.py", "eta": 0.0, "git_head": __import__("bench").git_head()}
    for N in (12, 21):
        out["generate_b1_n%d" % N] = per_scene(device, N, a.reps)
        torch.cuda.empty_cache()
    out["generate_batched_b256"] = batched(device, max(2, a.reps - 1))
    if a.kernel_db:
        out["rocprofv3_ddim_step_kernel"] = kernel_line(a.kernel_db)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
