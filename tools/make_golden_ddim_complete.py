"""tests/golden/ddim_complete.npz: strided (DDIM) scene completion and re-arrangement, from the REAL reference's ddim_sample_loop
(diffusion_ddpm.py:402-444) run ONE SCENE AT A TIME at B = 1 (build machine only).

Usage:  python tools/make_golden_ddim_complete.py        (a few minutes on CPU)

The reference defines no strided completion; this project defines scene b of ``ddim_complete_ragged_loop`` as the reference's own
ddim_sample_loop on that scene alone with one addition taken from p_sample_loop_complete (:461-466): before every model call at pair
(t, t_next) the first counts[b] rows of ``img`` are overwritten in place with q_sample(partial, t, fresh noise).  The loop body runs
exactly as written: its two call-site slips are bridged on the INSTANCE as in tools/make_golden_ddim.py (``self_condition = False``, a
``model_predictions`` bound to ``DiffusionPoint._denoise``), and that same instance-level bridge does
``img[:, :p] = gd.q_sample(partial, t_, noise=replayed partial draw)`` before it calls the reference method.  The DDIM update reads x_t
only through x_start and pred_noise, so nothing else changes.  The restore of the given rows after the last pair is done here.

The noise of the B calls is sliced from COMMON seeded buffers (oracle.make_golden.noise_list) laid out as the batched loop draws them:
main (S, B, N, C) -- x_T, then the main draw of every pair but the last -- and partial (S, B, N, C), one draw per pair (the given rows are
padded to N; scene b reads rows [0, counts[b])).  So every chain here has Pmax == N, the layout the scene-level entry points always
use; a partial buffer narrower than N (Pmax < N) is not pinned to the reference by this file and is covered by the kernel composition
and draw-order tests of tests/test_gpu_ddim_complete.py alone.  Weights, conditions and scenes are re-derived from seeds by the tests; only outputs are
stored.  All cases: T = 1000, linear schedule.

Cases (name: network, mean type, B, N, counts or mode, S, eta):
  living80.eta0     uncond living room, v, B = 8, N = 80, counts (0, 1, 7, 20, 20, 33, 79, 80), S = 50, eta 0
  living80.eta0.5   the same case at eta 0.5
  eps               the bedroom network of the meantypes fixture, eps, B = 4, N = 12, counts (0, 2, 6, 12), S = 20, eta 0.3
  partial           the 'partial' wrapper configuration (room_partial_condition): the reference's own ``sample`` per scene builds the
                    cat([partial, zeros]) condition, B = 4, counts (1, 2, 3, 0), S = 7 (non-uniform gaps), eta 0; raw outputs and the
                    post-filtered dicts
  arrange           the 'arrange' wrapper configuration on the wrapper fixture's batch: the bridged loop on the sub-shape (1, N, 5) under
                    the condition the reference's own ``sample`` builds, then the re-assembly expression of p_sample_loop_arrange
                    (:496-503), S = 10, eta 0; re-assembled outputs and their dicts
"""
import contextlib
import functools
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

T = 1000
ARRANGE_CHANNELS = 5            # translation_dim + angle_dim of the shipped re-arrangement config

# name: (kind, net kwargs | wrapper case, mean type, N, counts (None: re-arrangement), S, eta, seed)
CASES = {
    "living80.eta0": ("net", W.UNCOND_LIVING, "v", 80, (0, 1, 7, 20, 20, 33, 79, 80), 50, 0.0, 80),
    "living80.eta0.5": ("net", W.UNCOND_LIVING, "v", 80, (0, 1, 7, 20, 20, 33, 79, 80), 50, 0.5, 80),
    "eps": ("net", W.UNCOND_BEDROOM, "eps", 12, (0, 2, 6, 12), 20, 0.3, 82),
    "partial": ("wrapper", "partial", "v", 12, (1, 2, 3, 0), 7, 0.0, 83),
    "arrange": ("wrapper", "arrange", "v", 12, None, 10, 0.0, 84),
}


def ddim_complete_inputs(name):
    """(kind, net kwargs | wrapper case, mean type, shape, counts, S, eta, scenes (B, N, C), main noise (S, B, N, C') -- x_T then S - 1
    main draws --, partial noise (S, B, N, C) or None, condition (B, N, 128) or None for the wrapper cases, which build their own).
    C' is C, or 5 for re-arrangement (the diffused sub-shape)."""
    kind, kw, mt, N, counts, S, eta, seed = CASES[name]
    if counts is None:
        from oracle.make_golden_wrapper import B, wrapper_batch
        x = wrapper_batch("arrange")[1]
        C = x.shape[-1]
        main = torch.stack(noise_list([(B, N, ARRANGE_CHANNELS)] * S, seed, "ddimc_%s_main_" % name))
        return kind, kw, mt, (B, N, C), None, S, eta, x, main, None, None
    B = len(counts)
    C = 62 if kind == "wrapper" else kw["channels"]
    nc = 22 if kind == "wrapper" else kw["class_dim"]
    x = W.synth_scene_batch(B, N, nc, 32, seed)
    tag = name.split(".eta")[0]                     # the two eta cases are one case: the same scenes and the same noise
    main = torch.stack(noise_list([(B, N, C)] * S, seed, "ddimc_%s_main_" % tag))
    part = torch.stack(noise_list([(B, N, C)] * S, seed, "ddimc_%s_part_" % tag))
    cond = W.synth_condition(B, N, 128, seed, shared=True).contiguous() if kind == "net" else None
    return kind, kw, mt, (B, N, C), counts, S, eta, x, main, part, cond


def reference_ddim_scene(dp, shape, cond, cross, S, eta, mains, given=None, part_draws=None, clamped=None):
    """The reference's ddim_sample_loop on one scene (``dp``: the reference DiffusionPoint), bridged on the instance.  ``mains``: the S
    draws of the loop (x_T first); ``given`` (1, p, C) with its S partial draws: the in-place overwrite before every model call."""
    gd = dp.diffusion
    bound = functools.partial(type(gd).model_predictions, gd, dp._denoise)
    p = 0 if given is None else given.shape[1]
    calls = [0]

    def model_predictions(img, t_, *args, **kwargs):          # the reference's own method, with denoise_fn bound
        if p:
            img[:, :p] = gd.q_sample(given, t_, noise=part_draws[calls[0]])
        calls[0] += 1
        pred = bound(img, t_, *args, **kwargs)
        if clamped is not None:
            raw = bound(img, t_, *args, **dict(kwargs, clip_x_start=False)).pred_x_start
            clamped.append(float((raw != pred.pred_x_start).double().mean()))
        return pred

    gd.self_condition = False
    gd.model_predictions = model_predictions
    replay = Replay(mains)
    try:
        with torch.no_grad(), contextlib.redirect_stderr(io.StringIO()):
            out = gd.ddim_sample_loop(dp._denoise, shape, "cpu", cond, cross, noise_fn=replay, clip_denoised=True,
                                      sampling_timesteps=S, ddim_sampling_eta=eta)
    finally:
        del gd.model_predictions
    assert replay.i == S and calls[0] == S
    out = out.clone()
    if p:
        out[:, :p] = given                                   # the clean objects restored after the last pair
    return out


def _dict_arrays(prefix, d):
    return {"%s.%s" % (prefix, k): v.numpy() for k, v in d.items()}


def run_reference(name, stats_file):
    """(arrays of the case, mean share of x_start elements the clamp changed)."""
    kind, kw, mt, shape, counts, S, eta, x, main, part, cond = ddim_complete_inputs(name)
    B, N, C = shape
    out, clamped, rows = {}, [], []
    quiet = contextlib.redirect_stdout(io.StringIO())
    if kind == "net":
        net, dp = build_ref(kw, time_num=T, model_mean_type=mt)
        for b, p in enumerate(counts):
            rows.append(reference_ddim_scene(dp, (1, N, C), cond[b:b + 1], None, S, eta, [main[k, b:b + 1] for k in range(S)],
                                             x[b:b + 1, :p].contiguous(), [part[k, b:b + 1, :p].contiguous() for k in range(S)], clamped))
        out[name] = torch.cat(rows).numpy()
        return out, float(np.mean(clamped))
    from oracle.make_golden_wrapper import build_reference_wrapper
    mod, m, cfg = build_reference_wrapper(kw, stats_file, time_num=T)
    gd = m.diffusion.diffusion
    room = torch.zeros(1, 1, 64, 64)
    for b in range(B):
        mains = [main[k, b:b + 1] for k in range(S)]
        # the reference's own sample() assembles the condition and hands it to complete_samples / arrange_samples: those two are
        # pointed at the bridged strided loop on the instance, everything in front of them is the reference's
        if counts is not None:
            p = counts[b]
            given = x[b:b + 1, :p].contiguous()
            draws = [part[k, b:b + 1, :p].contiguous() for k in range(S)]
            m.diffusion.complete_samples = lambda shp, device, condition=None, condition_cross=None, clip_denoised=True, partial_boxes=None: \
                reference_ddim_scene(m.diffusion, tuple(shp), condition, condition_cross, S, eta, mains, partial_boxes, draws, clamped)
            with torch.no_grad(), quiet:
                y = m.sample(room, N, C, batch_size=1, partial_boxes=given, clip_denoised=True)
            del m.diffusion.complete_samples
        else:
            def arrange(shp, device, condition=None, condition_cross=None, clip_denoised=True, input_boxes=None):
                sub = (shp[0], shp[1], gd.translation_dim + gd.angle_dim)
                img = reference_ddim_scene(m.diffusion, sub, condition, condition_cross, S, eta, mains, clamped=clamped)
                tr, sz, bb = gd.translation_dim, gd.size_dim, gd.bbox_dim
                return torch.cat([img[:, :, 0:tr], input_boxes[:, :, tr:tr + sz], img[:, :, tr:], input_boxes[:, :, bb:]], dim=-1).contiguous()
            m.diffusion.arrange_samples = arrange
            with torch.no_grad(), quiet:
                y = m.sample(room, N, C, batch_size=1, input_boxes=x[b:b + 1], clip_denoised=True)
            del m.diffusion.arrange_samples
        with quiet:
            d = m.delete_empty_from_network_samples(y)
        rows.append(y)
        out.update(_dict_arrays("%s.dict.%d" % (name, b), d))
    out[name] = torch.cat(rows).numpy()
    return out, float(np.mean(clamped))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    stats_file = os.path.join(tempfile.mkdtemp(), "dataset_stats.txt")
    with open(stats_file, "w") as f:
        json.dump(W.DATASET_STATS, f)
    out, shares = {}, []
    for name in CASES:
        res, frac = run_reference(name, stats_file)
        shares.append(frac)
        y, counts = res[name], CASES[name][4]
        x = ddim_complete_inputs(name)[7].numpy()
        if counts is not None:
            for b, p in enumerate(counts):
                assert np.array_equal(y[b, :p], x[b, :p]), (name, b)           # the given objects come back bit-equal
        else:
            assert np.array_equal(y[:, :, 3:6], x[:, :, 3:6]) and np.array_equal(y[:, :, 8:], x[:, :, 8:]), name
        kept = [res["%s.dict.%d.translations" % (name, b)].shape[1] for b in range(y.shape[0])] if name + ".dict.0.translations" in res else None
        print("%-16s shape %-14s mean|x| %.5f finite %s clamp changed %.2f%% of x_start  kept %s"
              % (name, y.shape, float(np.abs(y).mean()), bool(np.isfinite(y).all()), 100 * frac, kept))
        out.update({k: np.asarray(v, dtype=np.float32) for k, v in res.items()})
    assert max(shares) > 0, "no case exercises the clamp"
    path = os.path.join(GOLDEN, "ddim_complete.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
