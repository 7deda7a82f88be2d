"""tests/golden/masked.npz: element-wise scene in-painting (p_sample_loop_masked / ddim_masked_loop), from the REAL reference's q_sample,
p_sample and ddim_sample_loop run ONE SCENE AT A TIME at B = 1 (build machine only).

Usage:  python tools/make_golden_masked.py        (several minutes on CPU: two of the cases are T = 1000 chains)

The reference has no masked loop; this project defines scene b of ``p_sample_loop_masked`` as the reference's p_sample_loop_complete
(diffusion_ddpm.py:447-476) on that scene alone with its two torch.cat's replaced by a select, and scene b of ``ddim_masked_loop`` as the
reference's ddim_sample_loop (:402-444) on that scene alone with the same select in front of every model call.  Only the select is
written here:
  T-step   x = where(mask, gd.q_sample(known, t, known-draw), x); x = gd.p_sample(...) -- the reference's own methods -- per step, and
           x = where(mask, known, x) after t == 0;
  strided  the reference's ddim_sample_loop runs as written, bridged on the INSTANCE as in tools/make_golden_ddim_complete.py
           (``self_condition = False``, a ``model_predictions`` bound to ``DiffusionPoint._denoise``); that bridge does the select on
           ``img`` in place before it calls the reference method.  The final select is done here.
The noise of the B calls is sliced from COMMON seeded buffers (oracle.make_golden.noise_list) laid out as the batched loop draws them:
main -- x_T, then the p_sample / DDIM draw of every step -- and known (one full-shape (B, N, C) draw per step), so the tests replay the
same buffers through one batched call.  Weights, conditions and scenes are re-derived from seeds by the tests; only outputs are stored.

The network is the reference WRAPPER of the shipped unconditional bedroom config (oracle.make_golden_wrapper 'uncond': v, N = 12,
condition = its positional embedding); the text case is the 'text' wrapper configuration (cross-attention over the stand-in BERT
features, condition and condition_cross as the reference's own ``sample`` assembles them at batch_size 1).

Scenes of the batch (``scene_masks``; channels [translation 0:3 | size 3:6 | angle 6:8 | class 8:30 | objfeat 30:62]):
  0 empty mask            1 whole rows {0, 1, 2}       2 whole rows {1, 5, 11}      3 the class channels of all rows
  4 size + class + objfeat of all rows      5 everything known      6 translations of rows 0-3 plus classes of rows 6-11
Cases (name: mean type, T, loop):
  v.T1000         v, T = 1000, T-step loop, clip_denoised on
  eps.T50         eps, T = 50, T-step loop, unclipped
  ddim.S20.eta0   v, T = 1000, S = 20, eta 0
  ddim.S7.eta0.3  v, T = 1000, S = 7 (non-uniform gaps), eta 0.3
  text.T50        the text model, v, T = 50, T-step loop, clip on, B = 2: scenes 2 and 6 of the list above
The text-free cases also store the dict the reference's delete_empty_from_network_samples makes of each B = 1 output."""
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
from oracle.make_golden import GOLDEN, Replay, noise_list  # noqa: E402

N, C = 12, 62
TR, SZ, BB, NC = 3, 3, 8, 22              # translation_dim, size_dim, bbox_dim, class_dim of the bedroom configs

# name: (wrapper case, mean type, T, S (None: the T-step loop), eta, clip_denoised, scenes of scene_masks(), seed)
CASES = {
    "v.T1000": ("uncond", "v", 1000, None, 0.0, True, tuple(range(7)), 100),
    "eps.T50": ("uncond", "eps", 50, None, 0.0, False, tuple(range(7)), 101),
    "ddim.S20.eta0": ("uncond", "v", 1000, 20, 0.0, True, tuple(range(7)), 102),
    "ddim.S7.eta0.3": ("uncond", "v", 1000, 7, 0.3, True, tuple(range(7)), 103),
    "text.T50": ("text", "v", 50, None, 0.0, True, (2, 6), 104),
}
TEXT_FREE = tuple(n for n in CASES if CASES[n][0] == "uncond")


def scene_masks():
    """(7, N, C) bool: the masks of the module docstring."""
    m = torch.zeros((7, N, C), dtype=torch.bool)
    m[1, [0, 1, 2]] = True
    m[2, [1, 5, 11]] = True
    m[3, :, BB:BB + NC] = True
    m[4, :, TR:TR + SZ] = True
    m[4, :, BB:] = True
    m[5] = True
    m[6, 0:4, 0:TR] = True
    m[6, 6:12, BB:BB + NC] = True
    return m


@functools.lru_cache(maxsize=None)
def masked_inputs(name):
    """(wrapper case, mean type, T, S, eta, clip, known (B, N, C), mask (B, N, C) bool, main noise, known noise).  T-step: main
    (T + 1, B, N, C) -- x_T, then the p_sample draw of every step --, known noise (T, B, N, C); strided: both (S, B, N, C).  Cached: callers share the tensors and leave them unchanged."""
    case, mt, T, S, eta, clip, scenes, seed = CASES[name]
    B = len(scenes)
    known = W.synth_scene_batch(B, N, NC, 32, seed)
    mask = scene_masks()[list(scenes)].contiguous()
    n_main, n_known = (T + 1, T) if S is None else (S, S)
    main = torch.stack(noise_list([(B, N, C)] * n_main, seed, "masked_%s_main_" % name))
    kn = torch.stack(noise_list([(B, N, C)] * n_known, seed, "masked_%s_known_" % name))
    return case, mt, T, S, eta, clip, known, mask, main, kn


def case_texts(name):
    from oracle.make_golden_wrapper import texts
    return texts()[:len(CASES[name][6])] if CASES[name][0] == "text" else None


def reference_tstep_scene(dp, cond, cross, T, clip, known, mask, mains, kdraws):
    """The reference's q_sample and p_sample on one scene, the select in between."""
    gd = dp.diffusion
    x = mains[0].clone()
    for i, t in enumerate(reversed(range(T))):
        t_ = torch.full((1,), t, dtype=torch.int64)
        x = torch.where(mask, gd.q_sample(known, t_, noise=kdraws[i]), x)
        x = gd.p_sample(dp._denoise, data=x, t=t_, condition=cond, condition_cross=cross, noise_fn=Replay([mains[i + 1]]),
                        clip_denoised=clip, return_pred_xstart=False)
    return torch.where(mask, known, x)


def reference_ddim_scene(dp, cond, cross, S, eta, known, mask, mains, kdraws, clamped):
    """The reference's ddim_sample_loop on one scene, bridged on the instance; the select happens on ``img`` in place in front of the
    reference's own model_predictions."""
    gd = dp.diffusion
    bound = functools.partial(type(gd).model_predictions, gd, dp._denoise)
    calls = [0]

    def model_predictions(img, t_, *args, **kwargs):
        img.copy_(torch.where(mask, gd.q_sample(known, t_, noise=kdraws[calls[0]]), img))
        calls[0] += 1
        pred = bound(img, t_, *args, **kwargs)
        raw = bound(img, t_, *args, **dict(kwargs, clip_x_start=False)).pred_x_start
        clamped.append(float((raw != pred.pred_x_start)[~mask].double().mean()) if (~mask).any() else 0.0)
        return pred

    gd.self_condition = False
    gd.model_predictions = model_predictions
    replay = Replay([m.clone() for m in mains])
    try:
        with torch.no_grad(), contextlib.redirect_stderr(io.StringIO()):
            out = gd.ddim_sample_loop(dp._denoise, (1, N, C), "cpu", cond, cross, noise_fn=replay, clip_denoised=True,
                                      sampling_timesteps=S, ddim_sampling_eta=eta)
    finally:
        del gd.model_predictions
    assert replay.i == S and calls[0] == S
    return torch.where(mask, known, out)


def run_reference(name, stats_file):
    """(arrays of the case, mean share of the free x_start elements the clamp changed or None)."""
    from oracle.make_golden_wrapper import build_reference_wrapper
    case, mt, T, S, eta, clip, known, mask, main, kn = masked_inputs(name)
    mod, m, cfg = build_reference_wrapper(case, stats_file, time_num=T)
    if mt != cfg["diffusion_kwargs"]["model_mean_type"]:
        with contextlib.redirect_stdout(io.StringIO()):
            m.diffusion = type(m.diffusion)(m.diffusion.model, cfg, **dict(cfg["diffusion_kwargs"], model_mean_type=mt))
    dp = m.diffusion
    quiet = contextlib.redirect_stdout(io.StringIO())
    room = torch.zeros(1, 1, 64, 64)
    text = case_texts(name)
    out, rows, clamped = {}, [], []
    for b in range(known.shape[0]):
        if text is None:
            cond, cross = m.positional_embedding[None].detach(), None
        else:
            # the reference's own sample() assembles both conditions and hands them to gen_samples: that call is caught on the instance
            got = {}
            dp.gen_samples = lambda shp, device, condition=None, condition_cross=None, clip_denoised=True: \
                got.update(cond=condition, cross=condition_cross) or torch.zeros(shp)
            with torch.no_grad(), quiet:
                m.sample(room, N, C, batch_size=1, text=[text[b]], clip_denoised=clip)
            del dp.gen_samples
            cond, cross = got["cond"], got["cross"]
        kb, mb = known[b:b + 1], mask[b:b + 1]
        mains = [main[k, b:b + 1] for k in range(main.shape[0])]
        kdraws = [kn[k, b:b + 1] for k in range(kn.shape[0])]
        with torch.no_grad():
            if S is None:
                y = reference_tstep_scene(dp, cond, cross, T, clip, kb, mb, mains, kdraws)
            else:
                y = reference_ddim_scene(dp, cond, cross, S, eta, kb, mb, mains, kdraws, clamped)
        rows.append(y)
        if text is None:
            with torch.no_grad(), quiet:
                d = m.delete_empty_from_network_samples(y)
            out.update({"%s.dict.%d.%s" % (name, b, k): v.numpy() for k, v in d.items()})
    out[name] = torch.cat(rows).numpy()
    return out, (float(np.mean(clamped)) if clamped else None)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    only = sys.argv[1:]
    stats_file = os.path.join(tempfile.mkdtemp(), "dataset_stats.txt")
    with open(stats_file, "w") as f:
        json.dump(W.DATASET_STATS, f)
    path = os.path.join(GOLDEN, "masked.npz")
    out = dict(np.load(path)) if only and os.path.exists(path) else {}
    shares = []
    for name in CASES:
        if only and name not in only:
            continue
        res, frac = run_reference(name, stats_file)
        if frac is not None:
            shares.append(frac)
        y = res[name]
        known, mask = masked_inputs(name)[6].numpy(), masked_inputs(name)[7].numpy()
        assert np.array_equal(y[mask], known[mask]), name                  # the given elements come back bit-equal
        assert np.isfinite(y).all(), name
        kept = [res["%s.dict.%d.translations" % (name, b)].shape[1] for b in range(y.shape[0])] if name in TEXT_FREE else None
        print("%-15s shape %-12s mean|x| %.5f%s  kept %s" % (name, y.shape, float(np.abs(y).mean()),
              "" if frac is None else "  clamp changed %.2f%% of the free x_start" % (100 * frac), kept), flush=True)
        out = {k: v for k, v in out.items() if k != name and not k.startswith(name + ".dict.")}
        out.update({k: np.asarray(v, dtype=np.float32) for k, v in res.items()})
    if not only:
        assert max(shares) > 0, "no strided case exercises the clamp"
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
