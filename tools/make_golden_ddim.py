"""tests/golden/ddim.npz: the REAL reference's DDIM loop (diffusion_ddpm.py:402-444), unmodified (build machine only).

Usage:  python tools/make_golden_ddim.py        (about a minute on CPU)

The reference's ddim_sample_loop cannot run as shipped: it calls ``self.model_predictions(img, t_, ...)`` without the
``denoise_fn`` argument and reads ``self.self_condition``, which GaussianDiffusion never sets.  Both are call-site slips, bridged
here on the INSTANCE only -- ``self_condition = False`` and a ``model_predictions`` bound to ``DiffusionPoint._denoise`` -- so the
loop body itself runs exactly as written.  Weights, conditions and noise are re-derived from seeds (oracle/weights.py,
oracle.make_golden.noise_list) by the tests; only the outputs are stored.  The noise is replayed (draw 0 = x_T, then one draw per
pair except the last: S draws), all on the linear schedule with T = 1000 of the shipped configs.

Cases (name: network, mean type, B, N, S, eta):
  living80.S50.eta0 / living80.S50.eta0.5   uncond living room, v, B = 2, N = 80
  text32.S7                                 text bedroom, v, B = 4, N = 12, L = 32 (non-uniform gaps from the truncation)
  eps.S20 / x0.S20                          the bedroom network of the meantypes fixture, B = 2, N = 12.  The clamp triggers on
                                            eps as is; the x0 network predicts |x0| < 0.3 on its seeded weights, so for x0 the last
                                            Linear of each output head is scaled by 16 (exact in fp32) on both sides
  one.S50                                   one scene, B = 1, N = 12 (the K-parallel GEMM dispatch)
  traj.S10                                  return_all_timesteps=True, B = 2, N = 12: the S + 1 states
"""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from oracle.make_golden import GOLDEN, Replay, build_ref, noise_list  # noqa: E402

T = 1000

# name: (net kwargs, mean type, B, N, ctx dim, text L, S, eta, return_all_timesteps, seed, output-head scale)
CASES = {
    "living80.S50.eta0": (W.UNCOND_LIVING, "v", 2, 80, 128, 0, 50, 0.0, False, 60, 1),
    "living80.S50.eta0.5": (W.UNCOND_LIVING, "v", 2, 80, 128, 0, 50, 0.5, False, 61, 1),
    "text32.S7": (W.TEXT_BEDROOM, "v", 4, 12, 128, 32, 7, 0.0, False, 62, 1),
    "eps.S20": (W.UNCOND_BEDROOM, "eps", 2, 12, 128, 0, 20, 0.3, False, 63, 1),
    "x0.S20": (W.UNCOND_BEDROOM, "x0", 2, 12, 128, 0, 20, 0.0, False, 64, 16),
    "one.S50": (W.UNCOND_BEDROOM, "v", 1, 12, 128, 0, 50, 0.0, False, 65, 1),
    "traj.S10": (W.UNCOND_BEDROOM, "v", 2, 12, 128, 0, 10, 0.5, True, 66, 1),
}


def scale_heads(net, scale):
    """Multiply the last Linear of every output head (``*_hidden2output.4``) by ``scale`` (a power of two: exact)."""
    if scale != 1:
        with torch.no_grad():
            for n, p in net.named_parameters():
                if "hidden2output.4." in n:
                    p.mul_(scale)


def ddim_inputs(name):
    """(net kwargs, mean type, shape, condition, condition_cross, S, eta, return_all_timesteps, noise list of S draws)."""
    kw, mt, B, N, ctx_dim, L, S, eta, all_steps, seed, _ = CASES[name]
    shape = (B, N, kw["channels"])
    cond = W.synth_condition(B, N, ctx_dim, seed, shared=True).contiguous()
    cross = W.synth_text_condition(B, L, kw.get("text_dim", 512), seed) if L else None
    noise = noise_list([shape] * S, seed, "ddim_%s_" % name)
    return kw, mt, shape, cond, cross, S, eta, all_steps, noise


def run_reference(name):
    """The reference's ddim_sample_loop on CPU; returns (result, fraction of x_start elements the clamp changed)."""
    kw, mt, shape, cond, cross, S, eta, all_steps, noise = ddim_inputs(name)
    net, diff = build_ref(kw, time_num=T, model_mean_type=mt)
    scale_heads(net, CASES[name][-1])
    gd = diff.diffusion
    bound = functools.partial(type(gd).model_predictions, gd, diff._denoise)
    clamped = []

    def model_predictions(*args, **kwargs):          # the reference's own method, with denoise_fn bound
        pred = bound(*args, **kwargs)
        raw = bound(*args, **dict(kwargs, clip_x_start=False)).pred_x_start
        clamped.append(float((raw != pred.pred_x_start).double().mean()))
        return pred

    gd.self_condition = False
    gd.model_predictions = model_predictions
    with torch.no_grad(), contextlib.redirect_stderr(io.StringIO()):
        out = gd.ddim_sample_loop(diff._denoise, shape, "cpu", cond, cross, noise_fn=Replay(noise), clip_denoised=True,
                                  sampling_timesteps=S, ddim_sampling_eta=eta, return_all_timesteps=all_steps)
    out = torch.stack(out) if all_steps else out
    return out.numpy(), float(np.mean(clamped))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    for name in CASES:
        res, frac = run_reference(name)
        out[name] = res
        print("%-20s shape %-18s mean|x| %.5f  clamp changed %.2f%% of x_start" % (name, res.shape, float(np.abs(res).mean()),
                                                                                    100 * frac))
    path = os.path.join(GOLDEN, "ddim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
