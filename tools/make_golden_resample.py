"""tests/golden/resample.npz: the completion and in-painting loops under resampling jumps (RePaint), from the REAL reference's q_sample,
p_sample and ddim_sample_loop run ONE SCENE AT A TIME at B = 1 (build machine only).

Usage:  python tools/make_golden_resample.py [case ...]        (some minutes on CPU: one chain makes 1200 calls of the T = 1000 model)

The reference has no resampling.  This project defines scene b of a resampled loop as the masked loop of tools/make_golden_masked.py --
the reference's p_sample (diffusion_ddpm.py:339-352) resp. one pair of its ddim_sample_loop (:402-444) on that scene alone, with the
select  x = where(mask, q_sample(known, t, given-draw), x)  in front of every model call and  x = where(mask, known, x)  after the last
one -- walked along RePaint's schedule instead of straight down, with one forward diffusion of the whole state at every jump.  Only the
schedule (``schedule``) and the forward jump (``jump_coefficients``, ``x = ja * x + jb * eps`` in three float32 torch
ops) are written here; the jump coefficients come from the reference instance's own float64 betas (``np_betas``), rounded once.
  T-step   gd.q_sample and gd.p_sample, the reference's own methods, per model call;
  strided  the reference's ddim_sample_loop runs as written, ONE PAIR per call: bridged on the instance as in tools/make_golden_masked.py
           (``self_condition = False``, a ``model_predictions`` bound to ``DiffusionPoint._denoise`` that does the select on ``img`` in
           place), with torch.linspace answering the loop's own request (-1 .. T' - 1 in 2 points) by the pair (t_next, t) that the
           schedule has reached -- the pairs themselves are the reference's ``linspace(-1, T - 1, S + 1).int()``;
  guided   the reference's ``DiffusionPoint._denoise`` replaced on the instance by the two-call function of tools/make_golden_cfg.py.
The noise of the B calls is sliced from COMMON seeded buffers (oracle.make_golden.noise_list) laid out as the batched loop draws them:
main -- x_T, then one row per step draw and per jump draw in order of occurrence --, given -- one row per model call, (B, N, C), or
(B, Pmax, C) for the ragged-rows case --, so the tests replay the same buffers through one batched call.

B = 3, N = 12, C = 62.  Masks (tools/make_golden_guided_inpaint.scene_masks): scene 0 whole rows [0, 4), scene 1 sizes + classes of all
rows, scene 2 scattered single elements.  Cases (name: wrapper, mean type, T / S, (j, r), K):
  eps.T50          uncond, eps, T = 50, (5, 3), unclipped                       140 calls
  v.T1000.K100     uncond, v, T = 1000, (10, 3), K = 100, clip on              1200 calls
  ddim.S20.eta0    uncond, v, T = 1000, S = 20, (4, 2), eta 0
  ddim.S7.eta0.3   uncond, v, T = 1000, S = 7, (2, 3), eta 0.3
  ragged.T50       uncond, v, T = 50, (5, 3), rows [0, counts[b]) given, counts (0, 3, 5), Pmax = 5
  text.T50         text, v, T = 50, (5, 3), guidance scales (0, 1.5, 3)
Per chain: ``<name>`` the reference's float32 final state (3, 12, 62) and ``<name>.sens`` = [norm-relative, element-wise] distance
(``distance`` of tools/make_golden_cfg.py) between that state and a FLOAT64 run of the same chain on the same draws: the pinned port
oracle.ref_torch on the float32 weights, tables, jump coefficients, conditions and draws cast to double (``restated``), as in
tools/make_golden_cfg.py.  The GPU test bounds each chain by the larger of the project's chain criterion and 4 x this sensitivity."""
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

from oracle import ref_torch as R  # noqa: E402
from oracle import weights as W  # noqa: E402
from oracle.make_golden import GOLDEN, Replay, noise_list  # noqa: E402
from tools.make_golden_cfg import _sinusoid64, distance  # noqa: E402
from tools.make_golden_guided_inpaint import scene_masks  # noqa: E402

B, N, C = 3, 12, 62
NC = 22
SCALES = (0.0, 1.5, 3.0)
COUNTS, PMAX = (0, 3, 5), 5
# name: (wrapper case, mean type, T, S (None: the T-step loop), eta, clip_denoised, (j, r), K, given kind, seed)
CASES = {
    "eps.T50": ("uncond", "eps", 50, None, 0.0, False, (5, 3), None, "mask", 140),
    "v.T1000.K100": ("uncond", "v", 1000, None, 0.0, True, (10, 3), 100, "mask", 141),
    "ddim.S20.eta0": ("uncond", "v", 1000, 20, 0.0, True, (4, 2), None, "mask", 142),
    "ddim.S7.eta0.3": ("uncond", "v", 1000, 7, 0.3, True, (2, 3), None, "mask", 143),
    "ragged.T50": ("uncond", "v", 50, None, 0.0, True, (5, 3), None, "rows", 144),
    "text.T50": ("text", "v", 50, None, 0.0, True, (5, 3), None, "mask", 145),
}


def pair_times(T, S):
    """The times of the S pairs, the reference's own expression (:409-410)."""
    return list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))[:-1]


def schedule(U, j, r, time_of, K=None):
    """RePaint's get_schedule_jump on remaining indices -> [("call", u) | ("jump", s)]."""
    budget = {s: r - 1 for s in range(0, U - j, j) if K is None or time_of(s) < K}
    out, u = [], U
    while u >= 1:
        u -= 1
        out.append(("call", u))
        s = u - 1
        if budget.get(s, 0) > 0:
            budget[s] -= 1
            out.append(("jump", s))
            u = s + j + 1
    return out


def case_schedule(name):
    """(op list, time(u)) of a case."""
    case, mt, T, S, eta, clip, (j, r), K, kind, seed = CASES[name]
    if S is None:
        time_of = lambda u: u  # noqa: E731
        return schedule(T, j, r, time_of, K), time_of
    times = pair_times(T, S)
    time_of = lambda u: times[S - 1 - u]  # noqa: E731
    return schedule(S, j, r, time_of, K), time_of


def jump_coefficients(np_betas, t_from, t_to):
    """(ja, jb) float32 of one jump from noise level t_from up to t_to, from float64 betas, rounded once."""
    ac = np.cumprod(1.0 - np.asarray(np_betas, dtype=np.float64))
    ratio = ac[t_to] / ac[t_from]
    return torch.tensor(np.float32(np.sqrt(ratio))), torch.tensor(np.float32(np.sqrt(1.0 - ratio)))


def case_texts():
    from oracle.make_golden_wrapper import texts
    return texts()[:B]


@functools.lru_cache(maxsize=None)
def chain_inputs(name):
    """(known (B, N, C), mask (B, N, C) bool, main noise (rows, B, N, C), given noise (calls, B, N or Pmax, C)).  Cached: callers share
    the tensors and leave them unchanged."""
    case, mt, T, S, eta, clip, jr, K, kind, seed = CASES[name]
    ops_, _ = case_schedule(name)
    calls = sum(1 for op, _ in ops_ if op == "call")
    jumps = len(ops_) - calls
    known = W.synth_scene_batch(B, N, NC, 32, seed)
    if kind == "rows":
        mask = (torch.arange(N)[None, :] < torch.tensor(COUNTS)[:, None])[:, :, None].expand(B, N, C).contiguous()
    else:
        mask = scene_masks()
    n_main = calls + jumps + (1 if S is None else 0)
    main = torch.stack(noise_list([(B, N, C)] * n_main, seed, "resample_%s_main_" % name))
    gn = torch.stack(noise_list([(B, PMAX if kind == "rows" else N, C)] * calls, seed, "resample_%s_given_" % name))
    return known, mask, main, gn


def full_rows(draw):
    """A given draw of (b, Pmax, C) padded with zeros to (b, N, C): rows at or beyond the count are never selected."""
    if draw.shape[1] == N:
        return draw
    return torch.cat([draw, torch.zeros((draw.shape[0], N - draw.shape[1], C), dtype=draw.dtype)], dim=1)


# ------------------------------------------------------------------------------------------------ the restatement (oracle.ref_torch)
def restated(name, tb, denoise, np_betas, known, mask, main, gn, cross=None, w=None):
    """The batched resampled loop of a case from oracle.ref_torch parts, in the dtype of its operands: the float64 run of this tool and
    the CPU restatement of tests/test_resample_host.py.  ``denoise(x, t, cross)``; ``w`` (B, 1, 1): the guidance scales of the text case."""
    case, mt, T, S, eta, clip, (j, r), K, kind, seed = CASES[name]
    ops_, time_of = case_schedule(name)
    ac = tb["alphas_cumprod"]
    x = main[0]
    mi, ci = 1, 0
    for op, u in ops_:
        if op == "jump":
            ja, jb = (v.to(x.dtype) for v in jump_coefficients(np_betas, time_of(u), time_of(u + j)))
            x = ja * x + jb * main[mi]
            mi += 1
            continue
        time = time_of(u)
        t = torch.full((x.shape[0],), time, dtype=torch.int64)
        x = torch.where(mask, R.q_sample(tb, known, t, full_rows(gn[ci])), x)
        ci += 1
        out = denoise(x, t, cross)
        if w is not None:
            un = denoise(x, t, torch.zeros_like(cross))
            out = un + w * (out - un)
        if S is None:
            x = R.p_sample_step(tb, x, t, out, main[mi], clip, mt)
            mi += 1
            continue
        x0 = (R.predict_start_from_v(tb, x, t, out) if mt == "v" else R.predict_start_from_eps(tb, x, t, out) if mt == "eps" else out).clamp(-1.0, 1.0)
        pred_noise = out if mt == "eps" else \
            (R._ex(tb["sqrt_recip_alphas_cumprod"], t, x.dim()) * x - x0) / R._ex(tb["sqrt_recipm1_alphas_cumprod"], t, x.dim())
        if u == 0:
            x = x0
            continue
        alpha, alpha_next = ac[time], ac[time_of(u - 1)]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        c = (1 - alpha_next - sigma ** 2).sqrt()
        x = x0 * alpha_next.sqrt() + c * pred_noise + sigma * main[mi]
        mi += 1
    assert mi == main.shape[0] and ci == gn.shape[0], (mi, ci)
    return torch.where(mask, known, x)


def run_float64(name, sd, kw, cond, cross, np_betas):
    case, mt, T = CASES[name][:3]
    known, mask, main, gn = chain_inputs(name)
    tb = {k: v.double() for k, v in R.schedule_tables(1e-4, 0.02, T, mt).items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    cond64 = cond.double()
    keep = R.sinusoidal_embedding
    R.sinusoidal_embedding = _sinusoid64          # the port builds the embedding in float32; this run wants it in double
    try:
        with torch.no_grad():
            return restated(name, tb, lambda x, t, cr: R.unet1d_forward(sd64, kw, x, t, cond64, cr), np_betas, known.double(), mask,
                            main.double(), gn.double(), None if cross is None else cross.double(),
                            torch.tensor(SCALES, dtype=torch.float64)[:, None, None] if case == "text" else None)
    finally:
        R.sinusoidal_embedding = keep


# ------------------------------------------------------------------------------------------------ the reference run
def reference_ddim_pair(dp, cond, cross, eta, time, time_next, x, known, mask, kdraw, noise):
    """One pair of the reference's ddim_sample_loop on one scene, entered through the loop itself: x is its x_T, the select is done on
    ``img`` in place in front of its own model_predictions, torch.linspace answers its request with the pair."""
    gd = dp.diffusion
    bound = functools.partial(type(gd).model_predictions, gd, dp._denoise)

    def model_predictions(img, t_, *args, **kwargs):
        assert int(t_[0]) == time
        img.copy_(torch.where(mask, gd.q_sample(known, t_, noise=kdraw), img))
        return bound(img, t_, *args, **kwargs)

    linspace = torch.linspace

    def one_pair(start, end, steps=None, **kwargs):
        if start == -1 and steps == 2 and not kwargs:
            return torch.tensor([float(time_next), float(time)])
        return linspace(start, end, steps=steps, **kwargs)

    gd.self_condition = False
    gd.model_predictions = model_predictions
    torch.linspace = one_pair
    replay = Replay([x] + ([noise] if time_next >= 0 else []))
    try:
        with torch.no_grad(), contextlib.redirect_stderr(io.StringIO()):
            out = gd.ddim_sample_loop(dp._denoise, (1, N, C), "cpu", cond, cross, noise_fn=replay, clip_denoised=True, sampling_timesteps=1,
                                      ddim_sampling_eta=eta)
    finally:
        torch.linspace = linspace
        del gd.model_predictions
    assert replay.i == len(replay.seq)
    return out


def reference_scene(name, dp, cond, cross, kb, mb, mains, gdraws):
    """The resampled loop of a case on one scene: the reference's own steps along the schedule, the jump in three float32 torch ops."""
    case, mt, T, S, eta, clip, (j, r), K, kind, seed = CASES[name]
    gd = dp.diffusion
    ops_, time_of = case_schedule(name)
    x = mains[0].clone()
    mi, ci = 1, 0
    for op, u in ops_:
        if op == "jump":
            ja, jb = jump_coefficients(gd.np_betas, time_of(u), time_of(u + j))
            x = ja * x + jb * mains[mi]
            mi += 1
            continue
        kdraw = full_rows(gdraws[ci])
        ci += 1
        if S is None:
            t_ = torch.full((1,), u, dtype=torch.int64)
            x = torch.where(mb, gd.q_sample(kb, t_, noise=kdraw), x)
            x = gd.p_sample(dp._denoise, data=x, t=t_, condition=cond, condition_cross=cross, noise_fn=Replay([mains[mi]]),
                            clip_denoised=clip, return_pred_xstart=False)
            mi += 1
        else:
            last = u == 0
            x = reference_ddim_pair(dp, cond, cross, eta, time_of(u), -1 if last else time_of(u - 1), x, kb, mb, kdraw,
                                    None if last else mains[mi])
            mi += 0 if last else 1
    assert mi == len(mains) and ci == len(gdraws), (mi, ci)
    return torch.where(mb, kb, x)


def run_reference(name, stats_file):
    """(float32 final states of the B reference runs at B = 1, denoiser state dict, net kwargs, cond (B, ...), cross or None, np_betas)."""
    from oracle.make_golden_wrapper import build_reference_wrapper
    case, mt, T, S, eta, clip, jr, K, kind, seed = CASES[name]
    known, mask, main, gn = chain_inputs(name)
    mod, m, cfg = build_reference_wrapper(case, stats_file, time_num=T)
    if mt != cfg["diffusion_kwargs"]["model_mean_type"]:
        with contextlib.redirect_stdout(io.StringIO()):
            m.diffusion = type(m.diffusion)(m.diffusion.model, cfg, **dict(cfg["diffusion_kwargs"], model_mean_type=mt))
    dp = m.diffusion
    quiet = contextlib.redirect_stdout(io.StringIO())
    room = torch.zeros(1, 1, 64, 64)
    rows, conds, crosses = [], [], []
    for b in range(B):
        if case == "text":
            # the reference's own sample() assembles both conditions and hands them to gen_samples: that call is caught on the instance
            got = {}
            dp.gen_samples = lambda shp, device, condition=None, condition_cross=None, clip_denoised=True: \
                got.update(cond=condition, cross=condition_cross) or torch.zeros(shp)
            with torch.no_grad(), quiet:
                m.sample(room, N, C, batch_size=1, text=[case_texts()[b]], clip_denoised=clip)
            del dp.gen_samples
            cond, cross = got["cond"], got["cross"]
            null = torch.zeros_like(cross)
            w = torch.tensor(SCALES[b], dtype=torch.float32)

            def bridged(data, t, condition, condition_cross):                # the reference's _denoise, bridged on the instance
                c = dp.model(data, t, condition, condition_cross)
                un = dp.model(data, t, condition, null)
                return un + w * (c - un)
            dp._denoise = bridged
        else:
            cond, cross = m.positional_embedding[None].detach(), None
        mains = [main[k, b:b + 1] for k in range(main.shape[0])]
        gdraws = [gn[k, b:b + 1] for k in range(gn.shape[0])]
        try:
            with torch.no_grad():
                rows.append(reference_scene(name, dp, cond, cross, known[b:b + 1], mask[b:b + 1], mains, gdraws))
        finally:
            if case == "text":
                del dp._denoise
        conds.append(cond.detach())
        crosses.append(None if cross is None else cross.detach())
    sd = {k[len("diffusion.model."):]: v.detach() for k, v in m.state_dict().items() if k.startswith("diffusion.model.")}
    return (torch.cat(rows), sd, cfg["net_kwargs"], torch.cat(conds), None if crosses[0] is None else torch.cat(crosses),
            np.array(dp.diffusion.np_betas, dtype=np.float64))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    only = sys.argv[1:]
    stats_file = os.path.join(tempfile.mkdtemp(), "dataset_stats.txt")
    with open(stats_file, "w") as f:
        json.dump(W.DATASET_STATS, f)
    path = os.path.join(GOLDEN, "resample.npz")
    out = dict(np.load(path)) if only and os.path.exists(path) else {}
    for name in CASES:
        if only and name not in only:
            continue
        y, sd, kw, cond, cross, np_betas = run_reference(name, stats_file)
        y64 = run_float64(name, sd, kw, cond, cross, np_betas)
        r, ew = distance(y, y64)
        known, mask = chain_inputs(name)[:2]
        ops_, _ = case_schedule(name)
        assert torch.isfinite(y).all(), name
        assert torch.equal(y[mask], known[mask]), name                        # the given elements come back bit-equal
        print("%-15s %4d calls %3d jumps  mean|x| %.5f  reference f32 vs f64: norm-relative %.3g, element-wise %.3g"
              % (name, sum(1 for op, _ in ops_ if op == "call"), sum(1 for op, _ in ops_ if op == "jump"), float(y.abs().mean()), r, ew),
              flush=True)
        out[name] = y.numpy().astype(np.float32)
        out[name + ".sens"] = np.array([r, ew], dtype=np.float64)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
