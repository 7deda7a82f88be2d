"""tests/golden/complete_ragged.npz: the REAL reference's scene completion (p_sample_loop_complete, diffusion_ddpm.py:447-476), run
ONE SCENE AT A TIME with a different number of given objects per scene (build machine only).

Usage:  python tools/make_golden_complete_ragged.py        (a few minutes on CPU)

The batched completion of this project (p_sample_loop_complete_ragged) defines scene b as the reference loop run on that scene alone, at
B = 1, with partial_boxes[b, :counts[b]].  That is what is recorded here: for every scene of a case, one call of the reference's
``DiffusionPoint.complete_samples`` at B = 1.  The noise of the B calls is sliced from COMMON seeded buffers
(oracle.make_golden.noise_list) laid out as the batched loop draws them -- x_T (B, N, C), then per step a partial draw (B, N, C) (the
given rows are padded to N; scene b reads rows [0, counts[b])) and a main draw (B, N, C) -- so the test replays the same buffers through
one batched call.  Weights, conditions and scenes are re-derived from seeds by the tests (oracle/weights.py); only outputs are stored.
All cases: T = 50, linear schedule.

Cases (name: network, mean type, B, N, counts, clip_denoised):
  living80   uncond living room, v, B = 8, N = 80, counts (0, 1, 7, 20, 20, 33, 79, 80), clipped
  bedroom    the reference WRAPPER of the shipped uncond bedroom config (oracle.make_golden_wrapper 'uncond': v, N = 12, condition = its
             positional embedding), B = 6, counts (0, 1, 3, 5, 11, 12), clipped; also the dict its delete_empty_from_network_samples
             makes of each B = 1 output
  eps        the bedroom network of the meantypes fixture with model_mean_type 'eps', B = 4, N = 12, counts (0, 2, 6, 12), unclipped
  partial    the 'partial' wrapper configuration (room_partial_condition): the reference's own ``sample`` per scene, which builds the
             cat([partial, zeros]) condition, B = 4, counts (1, 2, 3, 0), clipped; raw outputs and the post-filtered dicts
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from oracle.make_golden import GOLDEN, Replay, build_ref, noise_list  # noqa: E402

T = 50

# name: (kind, net kwargs | wrapper case, mean type, N, counts, clip_denoised, seed)
CASES = {
    "living80": ("net", W.UNCOND_LIVING, "v", 80, (0, 1, 7, 20, 20, 33, 79, 80), True, 70),
    "bedroom": ("wrapper", "uncond", "v", 12, (0, 1, 3, 5, 11, 12), True, 71),
    "eps": ("net", W.UNCOND_BEDROOM, "eps", 12, (0, 2, 6, 12), False, 72),
    "partial": ("wrapper", "partial", "v", 12, (1, 2, 3, 0), True, 73),
}


def ragged_inputs(name):
    """(kind, net kwargs | wrapper case, mean type, shape, counts, clip, scenes (B, N, C), main noise (T+1, B, N, C), partial noise (T, B, N, C),
    condition (B, N, 128) or None for the wrapper cases, which build their own)."""
    kind, kw, mt, N, counts, clip, seed = CASES[name]
    B = len(counts)
    C = 62 if kind == "wrapper" else kw["channels"]
    nc = 22 if kind == "wrapper" else kw["class_dim"]
    x = W.synth_scene_batch(B, N, nc, 32, seed)
    main = torch.stack(noise_list([(B, N, C)] * (T + 1), seed, "ragged_%s_main_" % name))
    part = torch.stack(noise_list([(B, N, C)] * T, seed, "ragged_%s_part_" % name))
    cond = W.synth_condition(B, N, 128, seed, shared=True).contiguous() if kind == "net" else None
    return kind, kw, mt, (B, N, C), counts, clip, x, main, part, cond


def scene_noise(main, part, b, p):
    """The draws of the reference loop on scene b alone: x_T, then per step the partial draw (1, p, C) and the main draw (1, N, C)."""
    seq = [main[0, b:b + 1]]
    for i in range(T):
        seq += [part[i, b:b + 1, :p].contiguous(), main[i + 1, b:b + 1]]
    return seq


def _dict_arrays(prefix, d):
    return {"%s.%s" % (prefix, k): v.numpy() for k, v in d.items()}


def run_reference(name, stats_file):
    kind, kw, mt, shape, counts, clip, x, main, part, cond = ragged_inputs(name)
    B, N, C = shape
    out = {}
    quiet = contextlib.redirect_stdout(io.StringIO())
    if kind == "net":
        net, diff = build_ref(kw, time_num=T, model_mean_type=mt)
        rows = []
        for b, p in enumerate(counts):
            with torch.no_grad(), quiet:
                rows.append(diff.complete_samples((1, N, C), "cpu", condition=cond[b:b + 1], condition_cross=None,
                                                  noise_fn=Replay(scene_noise(main, part, b, p)), clip_denoised=clip,
                                                  partial_boxes=x[b:b + 1, :p].contiguous()))
        out[name] = torch.cat(rows).numpy()
        return out
    from oracle.make_golden_wrapper import build_reference_wrapper
    mod, m, cfg = build_reference_wrapper(kw, stats_file, time_num=T)
    room = torch.zeros(1, 1, 64, 64)
    rows = []
    for b, p in enumerate(counts):
        given = x[b:b + 1, :p].contiguous()
        replay = Replay(scene_noise(main, part, b, p))
        with torch.no_grad(), quiet:
            if kw == "uncond":
                y = m.diffusion.complete_samples((1, N, C), "cpu", condition=m.positional_embedding[None].detach(), condition_cross=None,
                                                 noise_fn=replay, clip_denoised=clip, partial_boxes=given)
            else:
                # the reference's own sample(): it assembles the partial condition and calls complete_samples with the default
                # noise_fn; the replayed noise goes in on the instance, the call itself is the reference's
                inner = m.diffusion.complete_samples
                m.diffusion.complete_samples = lambda *a, _inner=inner, _r=replay, **k: _inner(*a, noise_fn=_r, **k)
                y = m.sample(room, N, C, batch_size=1, partial_boxes=given, clip_denoised=clip)
                m.diffusion.complete_samples = inner
            assert replay.i == 2 * T + 1
            d = m.delete_empty_from_network_samples(y)
        rows.append(y)
        out.update(_dict_arrays("%s.dict.%d" % (name, b), d))
    out[name] = torch.cat(rows).numpy()
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    stats_file = os.path.join(tempfile.mkdtemp(), "dataset_stats.txt")
    with open(stats_file, "w") as f:
        json.dump(W.DATASET_STATS, f)
    out = {}
    for name in CASES:
        res = run_reference(name, stats_file)
        y, counts = res[name], CASES[name][4]
        x = ragged_inputs(name)[6].numpy()
        for b, p in enumerate(counts):
            assert np.array_equal(y[b, :p], x[b, :p]), (name, b)           # the given objects come back untouched
        kept = [res["%s.dict.%d.translations" % (name, b)].shape[1] for b in range(len(counts))] if name + ".dict.0.translations" in res else None
        print("%-9s shape %-14s mean|x| %.5f finite %s kept %s" % (name, y.shape, float(np.abs(y).mean()), bool(np.isfinite(y).all()), kept))
        out.update({k: np.asarray(v, dtype=np.float32) for k, v in res.items()})
    path = os.path.join(GOLDEN, "complete_ragged.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
