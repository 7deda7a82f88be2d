#!/usr/bin/env python
"""Measurement for the scene-statistics row: box_bounds + scene_stats on the GPU vs a numpy port on the host, same scenes.
Prints one JSON line: scenes/s at (B = 4096, N = 21) and (B = 1024, N = 80)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from diffuscene_amd import scene_stats as S
from tools.make_golden_scene_stats import draw_scene, numpy_box_bounds


def numpy_port(tr, sz, an, sc):
    """One scene on the host, vectorised over the pairs (the reference loops over them in Python): bounds, IoU matrix, symmetry."""
    b = numpy_box_bounds(tr, sz, an)
    n = len(b)
    vol = (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])
    wh = np.maximum(np.minimum(b[:, None, 3:], b[None, :, 3:]) - np.maximum(b[:, None, :3], b[None, :, :3]), np.float32(0))
    ov = wh[..., 0] * wh[..., 1] * wh[..., 2]
    iou = ov / np.maximum((vol[:, None] + vol[None, :]) - ov, np.float32(1e-6))
    up = np.triu(np.ones((n, n), bool), 1)
    d, cls = b.astype(np.float64), sc.argmax(-1)
    half, cen = (d[:, 3:] - d[:, :3]) / 2, (d[:, 3:] + d[:, :3]) / 2
    dc = np.abs(cen[:, None] - cen[None, :])
    sym = (np.abs(half[:, None] - half[None, :]).max(-1) < 0.1) & ((dc[..., 0] < 0.1) | (dc[..., 2] < 0.1)) & (cls[:, None] == cls[None, :])
    return int(((iou > 0) & up).sum()), int((sym & up).sum()), float(iou[up].astype(np.float64).sum())


def case(B, N, distinct=32, host_scenes=16):
    scenes = [draw_scene(np.random.default_rng([7, N, k]), N) for k in range(distinct)]
    pick = [scenes[k % distinct] for k in range(B)]
    tr, sz, an, sc = (torch.from_numpy(np.stack([p[i] for p in pick])).cuda() for i in range(4))

    def both():
        return S.scene_stats(S.box_bounds(tr, sz, an), sc)
    st = both(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        both()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    t0 = time.perf_counter()
    host = [numpy_port(*scenes[k][:4]) for k in range(host_scenes)]
    cpu = host_scenes / (time.perf_counter() - t0)
    ni, ns = st.num_intersecting.cpu().numpy(), st.num_symmetry.cpu().numpy()
    # integers may differ from the host's only where a bound differs by one ulp at a threshold; report it instead of hiding it
    agree = sum(int((ni[k], ns[k]) == host[k][:2]) for k in range(host_scenes))
    return {"B": B, "N": N, "scenes_per_s": round(B / (ms * 1e-3)), "ms_per_batch": round(ms, 4), "cpu_numpy_port_scenes_per_s": round(cpu, 1),
            "host_scenes_with_equal_integers": "%d/%d" % (agree, host_scenes)}


print(json.dumps({"metric": "scene statistics scenes/s (box_bounds + scene_stats, two launches)", "cases": [case(4096, 21), case(1024, 80)],
                  "note": "GPU time includes the host checks and allocations of the Python wrappers; host port is vectorised numpy, one scene at a time"}))
