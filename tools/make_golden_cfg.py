"""tests/golden/cfg.npz: classifier-free guidance on the text path (p_sample_loop_guided / ddim_guided_loop) and the gated training
loss (text_drop_prob), from the REAL reference (build machine only).

Usage:  python tools/make_golden_cfg.py [case ...]        (about ten minutes on CPU: three of the chains run the T = 1000 model)

The reference has no guidance.  This project defines scene b of the guided loops as the reference's p_sample_loop
(diffusion_ddpm.py:355-371) resp. ddim_sample_loop (:402-444) with  m = u + w[b] * (c - u)  in place of the model output, c the
denoiser on (x, t, condition, condition_cross) and u the denoiser on (x, t, condition, 0).  Only that bridge is written here: the
reference's ``DiffusionPoint._denoise`` is replaced ON THE INSTANCE by a function that makes the two reference model calls and mixes
them (difference, product and sum as three float32 torch ops); the reference's own loops run as written around it.  ddim_sample_loop
additionally needs the two instance-level bridges of tools/make_golden_ddim_complete.py (``self_condition = False``, a
``model_predictions`` bound to the denoiser).

The network is the reference WRAPPER of the shipped text config (oracle.make_golden_wrapper 'text': v, N = 12, cross-attention over the
stand-in BERT features); condition and condition_cross are what the reference's own ``sample`` assembles at batch_size 3 for the first
three texts.  Scales (0, 1.5, 3).  Noise comes from seeded buffers (oracle.make_golden.noise_list) in the loop's draw order; the tests
re-derive weights, conditions and noise from the seeds, only outputs are stored.

Chains (name: mean type, T, loop):
  v.T1000          v, T = 1000, p_sample_loop, clip_denoised on
  eps.T50          eps, T = 50, p_sample_loop, unclipped
  ddim.S20.eta0    v, T = 1000, S = 20, eta 0
  ddim.S7.eta0.5   v, T = 1000, S = 7 (non-uniform gaps), eta 0.5
Per chain: ``<name>`` the reference's float32 final state (3, 12, 62) and ``<name>.sens`` = [norm-relative, element-wise] distance
between that state and a FLOAT64 run of the same chain on the same draws, under the metric of tests/test_gpu_wide.py (max|a-b| / max|b|
and max(|a-b| / max(|b|, 5 % of max|b|)), b the float64 run).  The GPU test bounds each chain by the larger of the project's chain
criterion and 4 x this sensitivity.

Which float64 run: the reference network resists the cast -- WeightStandardizedConv2d and LayerNorm switch their eps from 1e-5 to
1e-3 for any dtype other than float32 (denoise_net.py:84,99), and ``_denoise`` asserts float32 (:750) -- so a .double() of the
reference wrapper computes a different function.  The float64 run is therefore the pinned port oracle.ref_torch (eps stays 1e-5) on
the float32 weights, tables, conditions and draws cast to double, the sinusoidal time embedding evaluated in double; the guided
loops around it are restated below from its p_sample_step and the reference's DDIM expressions (as tests/test_cfg_host.py does in
float32).

Pinability (tests/test_cfg_host.py asserts it): every chain's sensitivity is at most a quarter of the bound the GPU test uses.  Measured
when the file was written (norm-relative / element-wise): v.T1000 1.9e-6 / 2.2e-5, eps.T50 5.1e-7 / 3.1e-6, ddim.S20.eta0 8.2e-7 /
2.8e-6, ddim.S7.eta0.5 5.5e-7 / 1.1e-5 -- no scale was lowered and no chain shortened.

Training case (``train.*``): the reference's ``get_loss`` at B = 4 on oracle.make_golden_wrapper's text batch, with
``keep = (1, 0, 1, 0)`` applied as a select to fc_text_f(desc_bert) in front of the reference's ``diffusion.get_loss_iter``
(torch.manual_seed(SEED_TRAIN) right before: t, then the noise).  Stored: the loss, the logged loss parts, the gradient of
fc_text_f.bias and rows GRAD_ROWS of the gradient of fc_text_f.weight."""
import contextlib
import functools
import io
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_torch as R  # noqa: E402
from oracle import weights as W  # noqa: E402
from oracle.make_golden import GOLDEN, Replay, noise_list  # noqa: E402

B, N, C = 3, 12, 62
SCALES = (0.0, 1.5, 3.0)
# name: (mean type, T, S (None: the T-step loop), eta, clip_denoised, seed)
CASES = {
    "v.T1000": ("v", 1000, None, 0.0, True, 110),
    "eps.T50": ("eps", 50, None, 0.0, False, 111),
    "ddim.S20.eta0": ("v", 1000, 20, 0.0, True, 112),
    "ddim.S7.eta0.5": ("v", 1000, 7, 0.5, True, 113),
}
TRAIN_B, TRAIN_KEEP, SEED_TRAIN = 4, (True, False, True, False), 1240
GRAD_ROWS = (0, 73, 146, 219, 292, 365, 438, 511)


def case_texts():
    from oracle.make_golden_wrapper import texts
    return texts()[:B]


@functools.lru_cache(maxsize=None)
def chain_noise(name):
    """(T + 1, B, N, C) -- x_T, then the draw of every step -- resp. (S, B, N, C).  Cached: callers share it and leave it unchanged."""
    mt, T, S, eta, clip, seed = CASES[name]
    return torch.stack(noise_list([(B, N, C)] * (T + 1 if S is None else S), seed, "cfg_%s_" % name))


def distance(a, b):
    """(norm-relative, element-wise with the 5 % range floor) of tests/test_gpu_wide.check, b the reference side."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    bmax = float(b.abs().max())
    return float((a - b).abs().max() / bmax), float(((a - b).abs() / torch.clamp(b.abs(), min=5e-2 * bmax)).max())


# ------------------------------------------------------------------------------------------------ the float64 run (oracle.ref_torch)
def guided(denoise, x, t, cross, w):
    """m = u + w (c - u) from two calls of ``denoise(x, t, cross)``, each op on its own."""
    c = denoise(x, t, cross)
    u = denoise(x, t, torch.zeros_like(cross))
    return u + w * (c - u)


def restated_tstep(tb, denoise, T, clip, mt, cross, w, noise):
    x = noise[0]
    for i, step in enumerate(reversed(range(T))):
        t = torch.full((x.shape[0],), step, dtype=torch.int64)
        x = R.p_sample_step(tb, x, t, guided(denoise, x, t, cross, w), noise[i + 1], clip, mt)
    return x


def restated_ddim(tb, denoise, T, S, eta, mt, cross, w, noise):
    """ddim_sample_loop (reference :402-444) with model_predictions(clip_x_start=True) (:242-264) on the guided output."""
    times = list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))
    ac = tb["alphas_cumprod"]
    x = noise[0]
    k = 1
    for time, time_next in zip(times[:-1], times[1:]):
        t = torch.full((x.shape[0],), time, dtype=torch.int64)
        out = guided(denoise, x, t, cross, w)
        if mt == "v":
            x0 = R.predict_start_from_v(tb, x, t, out).clamp(-1.0, 1.0)
        elif mt == "eps":
            x0 = R.predict_start_from_eps(tb, x, t, out).clamp(-1.0, 1.0)
        else:
            x0 = out.clamp(-1.0, 1.0)
        if mt == "eps":
            pred_noise = out
        else:
            pred_noise = (R._ex(tb["sqrt_recip_alphas_cumprod"], t, x.dim()) * x - x0) / R._ex(tb["sqrt_recipm1_alphas_cumprod"], t, x.dim())
        if time_next < 0:
            x = x0
            continue
        alpha, alpha_next = ac[time], ac[time_next]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        c = (1 - alpha_next - sigma ** 2).sqrt()
        x = x0 * alpha_next.sqrt() + c * pred_noise + sigma * noise[k]
        k += 1
    return x


def _sinusoid64(t, dim):
    half = dim // 2
    freq = torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000) / (half - 1)))
    arg = t[:, None].double() * freq[None, :]
    return torch.cat((arg.sin(), arg.cos()), dim=-1)


def run_float64(name, sd, kw, cond, cross):
    mt, T, S, eta, clip, seed = CASES[name]
    tb = {k: v.double() for k, v in R.schedule_tables(1e-4, 0.02, T, mt).items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    cond64, cross64 = cond.double(), cross.double()
    w = torch.tensor(SCALES, dtype=torch.float64)[:, None, None]
    noise = chain_noise(name).double()

    def denoise(x, t, cr):
        return R.unet1d_forward(sd64, kw, x, t, cond64, cr)

    keep = R.sinusoidal_embedding
    R.sinusoidal_embedding = _sinusoid64          # the port builds the embedding in float32; this run wants it in double
    try:
        with torch.no_grad():
            if S is None:
                return restated_tstep(tb, denoise, T, clip, mt, cross64, w, noise)
            return restated_ddim(tb, denoise, T, S, eta, mt, cross64, w, noise)
    finally:
        R.sinusoidal_embedding = keep


# ------------------------------------------------------------------------------------------------ the reference run
def reference_conditions(m, clip):
    """(condition, condition_cross) as the reference's own sample() hands them to gen_samples at batch_size B."""
    dp = m.diffusion
    got = {}
    dp.gen_samples = lambda shp, device, condition=None, condition_cross=None, clip_denoised=True: \
        got.update(cond=condition, cross=condition_cross) or torch.zeros(shp)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        m.sample(torch.zeros(B, 1, 64, 64), N, C, batch_size=B, text=case_texts(), clip_denoised=clip)
    del dp.gen_samples
    return got["cond"], got["cross"]


def run_reference(name, stats_file):
    """(float32 final state of the reference's loop around the guided bridge, denoiser state dict, net kwargs, cond, cross)."""
    from oracle.make_golden_wrapper import build_reference_wrapper
    mt, T, S, eta, clip, seed = CASES[name]
    mod, m, cfg = build_reference_wrapper("text", stats_file, time_num=T)
    if mt != cfg["diffusion_kwargs"]["model_mean_type"]:
        with contextlib.redirect_stdout(io.StringIO()):
            m.diffusion = type(m.diffusion)(m.diffusion.model, cfg, **dict(cfg["diffusion_kwargs"], model_mean_type=mt))
    dp = m.diffusion
    gd = dp.diffusion
    cond, cross = reference_conditions(m, clip)
    assert cross.dim() == 3 and cross.shape[0] == B
    w = torch.tensor(SCALES, dtype=torch.float32)[:, None, None]
    null = torch.zeros_like(cross)
    calls = [0]

    def bridged(data, t, condition, condition_cross):                        # the reference's _denoise, bridged on the instance
        calls[0] += 1
        c = dp.model(data, t, condition, condition_cross)
        u = dp.model(data, t, condition, null)
        return u + w * (c - u)

    dp._denoise = bridged
    noise = chain_noise(name)
    replay = Replay([noise[i].clone() for i in range(noise.shape[0])])
    try:
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            if S is None:
                y = gd.p_sample_loop(dp._denoise, (B, N, C), "cpu", cond, cross, noise_fn=replay, clip_denoised=clip)
            else:
                gd.self_condition = False
                gd.model_predictions = functools.partial(type(gd).model_predictions, gd, dp._denoise)
                try:
                    y = gd.ddim_sample_loop(dp._denoise, (B, N, C), "cpu", cond, cross, noise_fn=replay, clip_denoised=True,
                                            sampling_timesteps=S, ddim_sampling_eta=eta)
                finally:
                    del gd.model_predictions
    finally:
        del dp._denoise
    assert replay.i == noise.shape[0] and calls[0] == (T if S is None else S), (replay.i, calls[0])
    sd = {k[len("diffusion.model."):]: v.detach() for k, v in m.state_dict().items() if k.startswith("diffusion.model.")}
    return y, sd, cfg["net_kwargs"], cond.detach(), cross.detach()


def run_training(stats_file):
    from oracle.make_golden_wrapper import build_reference_wrapper, wrapper_batch
    mod, m, cfg = build_reference_wrapper("text", stats_file)
    s, _ = wrapper_batch("text")
    keep = torch.tensor(TRAIN_KEEP)[:, None, None]
    inner = m.diffusion.get_loss_iter

    def gated(data, noises=None, condition=None, condition_cross=None):
        return inner(data, noises=noises, condition=condition,
                     condition_cross=torch.where(keep, condition_cross, torch.zeros_like(condition_cross)))

    m.diffusion.get_loss_iter = gated
    torch.manual_seed(SEED_TRAIN)
    loss, parts = m.get_loss(s)
    loss.backward()
    del m.diffusion.get_loss_iter
    gw = m.fc_text_f.weight.grad
    dropped = [b for b, k in enumerate(TRAIN_KEEP) if not k]
    assert gw is not None and float(gw.abs().max()) > 0 and dropped
    out = {"train.loss": np.float32(loss.item()), "train.keep": np.array(TRAIN_KEEP),
           "train.grad.fc_text_f.bias": m.fc_text_f.bias.grad.numpy().astype(np.float32),
           "train.grad.fc_text_f.weight": gw[list(GRAD_ROWS)].numpy().astype(np.float32)}
    for k, v in parts.items():
        out["train.part." + k] = np.float32(v.item())
    print("train: loss %.6f, |d fc_text_f.weight| %.4g, |d fc_text_f.bias| %.4g" % (loss.item(), float(gw.norm()),
                                                                                     float(m.fc_text_f.bias.grad.norm())), flush=True)
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    only = sys.argv[1:]
    stats_file = os.path.join(tempfile.mkdtemp(), "dataset_stats.txt")
    with open(stats_file, "w") as f:
        json.dump(W.DATASET_STATS, f)
    path = os.path.join(GOLDEN, "cfg.npz")
    out = dict(np.load(path)) if only and os.path.exists(path) else {}
    for name in CASES:
        if only and name not in only:
            continue
        y, sd, kw, cond, cross = run_reference(name, stats_file)
        y64 = run_float64(name, sd, kw, cond, cross)
        r, ew = distance(y, y64)
        assert torch.isfinite(y).all(), name
        spread = float((y[1] - y[0]).abs().max())
        print("%-15s mean|x| %.5f  reference f32 vs f64: norm-relative %.3g, element-wise %.3g  (bound / 4: %.3g, %.3g)"
              % (name, float(y.abs().mean()), r, ew, max(5e-6, 4 * r) / 4, max(1e-4, 4 * ew) / 4), flush=True)
        assert spread > 0
        out[name] = y.numpy().astype(np.float32)
        out[name + ".sens"] = np.array([r, ew], dtype=np.float64)
    if not only or "train" in only:
        out.update(run_training(stats_file))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
