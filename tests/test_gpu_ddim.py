"""GPU: DDIM sampling (reference ddim_sample_loop, diffusion_ddpm.py:402-444).

* the fused step kernel (dsc_ddim_step_f32) against a float32 torch evaluation of the reference's expressions, bit for bit;
* every chain of tests/golden/ddim.npz (the REAL reference's loop, tools/make_golden_ddim.py) eager and as the captured graph,
  under both GEMM arithmetics, with the criteria of tests/test_gpu_wide.py; eager and graph bit-identical;
* the seeded default call: graph and eager loop draw the same numbers and return the same scenes;
* DDIM with S = T and eta = 1 against the DDPM loop (the same process in exact arithmetic);
* DDPM and DDIM calls interleaved on one model never replay a stale graph;
* the public entry points with ``sampling_timesteps``."""
import contextlib
import io
import json
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import weights as W  # noqa: E402
from oracle.make_golden import noise_list  # noqa: E402
from tools.make_golden_ddim import CASES, T, ddim_inputs, scale_heads  # noqa: E402

from test_gpu_wide import check, dev  # noqa: E402


def _diffusion(T_, mean_type="v"):
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    return GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, T_),
                             "mse", mean_type, "fixedsmall", False, False, None)


def _expected(gd, x, m, noise, k, pairs, coef):
    """The reference's float32 expressions on the CPU (model_predictions(clip_x_start=True) + the DDIM update), op by op."""
    t, tn = pairs[k]
    if gd.model_mean_type == "v":
        x0 = gd.sqrt_alphas_cumprod[t] * x - gd.sqrt_one_minus_alphas_cumprod[t] * m
    elif gd.model_mean_type == "eps":
        x0 = gd.sqrt_recip_alphas_cumprod[t] * x - gd.sqrt_recipm1_alphas_cumprod[t] * m
    else:
        x0 = m
    x0 = torch.clamp(x0, min=-1., max=1.)
    if tn < 0:
        return x0, x0
    pn = m if gd.model_mean_type == "eps" else (gd.sqrt_recip_alphas_cumprod[t] * x - x0) / gd.sqrt_recipm1_alphas_cumprod[t]
    return x0 * coef[0, k] + coef[1, k] * pn + coef[2, k] * noise, x0


@pytest.mark.parametrize("shape", [(1, 12, 65), (256, 80, 65), (3, 7, 37)])
@pytest.mark.parametrize("mean_type", ["v", "eps", "x0"])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_step_kernel_is_the_reference_expression_bit_for_bit(shape, mean_type, eta):
    from diffuscene_amd import _lib, ops
    _lib.fn("dsc_device_error_count")(1)
    gd = _diffusion(1000, mean_type)
    dtab = gd.ddim_tables(50, eta, dev())
    pairs, times, _, coef = dtab
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, mean_type, eta)).encode()))
    x = torch.randn(shape, generator=g) * 1.5
    m = torch.randn(shape, generator=g) * 1.5
    noise = torch.randn(shape, generator=g)
    xd, md, nd = x.to(dev()), m.to(dev()), noise.to(dev())
    for k in (0, 17, 48, 49):                                 # 49: the final pair (t, -1), which takes x_start and reads no noise
        step = torch.tensor([k], dtype=torch.int64, device=dev())
        want, want_x0 = _expected(gd, x, m, noise, k, pairs, coef[:, :].cpu())
        x0 = torch.empty_like(xd)
        got = gd.ddim_step(xd, md, nd, step, dtab, x0_out=x0)
        assert torch.equal(got.cpu(), want), (k, float((got.cpu() - want).abs().max()))
        assert torch.equal(x0.cpu(), want_x0)
        xi = xd.clone()                                       # in place: out aliases x_t
        gd.ddim_step(xi, md, nd, step, dtab, out=xi)
        assert torch.equal(xi.cpu(), want)
        if k == 49:                                           # the final step never reads the noise operand
            assert torch.equal(gd.ddim_step(xd, md, torch.full_like(nd, float("nan")), step, dtab).cpu(), want)
    # the advance kernel: step += 1, t = times[step]
    step = torch.tensor([17], dtype=torch.int64, device=dev())
    t = torch.zeros(shape[0], dtype=torch.int64, device=dev())
    ops.ddim_advance(step, times, t)
    assert int(step.item()) == 18 and t.eq(pairs[18][0]).all()
    assert _lib.fn("dsc_device_error_count")(1) == 0


# ------------------------------------------------------------------------------------------------ reference chains
_NETS = {}


def _point(name, time_num=T):
    from diffuscene_amd.networks.denoise_net import Unet1D
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint
    kw, mt = CASES[name][0], CASES[name][1]
    key = (repr(sorted(kw.items())), CASES[name][-1])
    if key not in _NETS:
        net = Unet1D(**kw)
        net.load_state_dict(W.synth_state_dict(kw))
        scale_heads(net, CASES[name][-1])
        _NETS[key] = net.to(dev())
    cfg = dict(objectness_dim=0, class_dim=kw["class_dim"], angle_dim=2, objfeat_dim=32)
    return DiffusionPoint(_NETS[key], cfg, time_num=time_num, model_mean_type=mt)


def _replay(seq):
    from diffuscene_amd.sampler import NoiseReplay
    return NoiseReplay(torch.stack(seq).to(dev()))


@pytest.mark.parametrize("gemm_arith", ["split", "f32"], indirect=True)
def test_reference_chains_eager_and_graph(golden_dir, gemm_arith):
    g = np.load(os.path.join(golden_dir, "ddim.npz"))
    assert sorted(g.files) == sorted(CASES)
    for name in CASES:
        kw, mt, shape, cond, cross, S, eta, all_steps, noise = ddim_inputs(name)
        diff = _point(name)
        cond = cond.to(dev())
        cross = cross.to(dev()) if cross is not None else None
        res = []
        for graph in ((False,) if all_steps else (False, True)):
            with torch.no_grad():
                r = diff.gen_samples_ddim(shape, dev(), condition=cond, condition_cross=cross, noise_fn=_replay(noise),
                                          sampling_timesteps=S, ddim_sampling_eta=eta, return_all_timesteps=all_steps, graph=graph)
            if all_steps:
                assert len(r) == S + 1
                r = torch.stack(r)
            check(r, g[name], "ddim %s (%s, graph=%s)" % (name, gemm_arith, graph))
            res.append(r)
        if len(res) == 2:
            assert torch.equal(res[0], res[1]), name


# ------------------------------------------------------------------------------------------------ seeded default call
def test_seeded_default_call_is_the_graph_and_draws_like_the_eager_loop(monkeypatch):
    from diffuscene_amd import sampler
    calls = []
    orig = sampler.graph_ddim_sample_loop
    monkeypatch.setattr(sampler, "graph_ddim_sample_loop", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    monkeypatch.delenv("DSC_GRAPH", raising=False)
    diff = _point("one.S50")
    cond = W.synth_condition(3, 12, 128, seed=2).to(dev())
    out = {}
    with torch.no_grad():
        for graph in (None, False):
            torch.manual_seed(11)
            y = diff.gen_samples_ddim((3, 12, 62), dev(), condition=cond, sampling_timesteps=10, ddim_sampling_eta=0.5, graph=graph)
            out[graph] = (y, torch.randn(5, device=dev()))
            assert len(calls) == 1
    assert torch.equal(out[None][0], out[False][0])
    assert torch.equal(out[None][1], out[False][1])
    assert torch.isfinite(out[None][0]).all()


# ------------------------------------------------------------------------------------------------ DDIM(S=T, eta=1) == DDPM
def test_ddim_with_every_step_and_eta_one_is_the_ddpm_loop():
    """With S = T and eta = 1, sigma_t^2 is the posterior variance and the DDIM update is the DDPM posterior step (exact arithmetic);
    the two loops differ only in how fp32 rounds the same quantity and in the DDPM loop's extra (unused) draw at t = 0.
    Measured on MI355X (T = 50, v, B = 2, N = 12): max |ddim - ddpm| / max |ddpm| = 1.66e-4 (the DDIM noise term divides by
    sqrt(1/alpha_t - 1), 0.01 at t = 0, and 50 large-beta steps through the network amplify the rounding); bound at 3x that."""
    diff = _point("traj.S10", time_num=50)
    cond = W.synth_condition(2, 12, 128, seed=3).contiguous().to(dev())
    seq = noise_list([(2, 12, 62)] * 51, 70, "ddim_vs_ddpm_")
    with torch.no_grad():
        a = diff.gen_samples_ddim((2, 12, 62), dev(), condition=cond, noise_fn=_replay(seq[:50]), sampling_timesteps=50,
                                  ddim_sampling_eta=1.0)
        b = diff.gen_samples((2, 12, 62), dev(), condition=cond, noise_fn=_replay(seq), clip_denoised=True)
    d = float((a - b).abs().max() / b.abs().max())
    print("DDIM(S=T, eta=1) vs DDPM: norm-relative %.3g" % d)
    assert d < 5e-4


# ------------------------------------------------------------------------------------------------ interleaving
def test_interleaved_ddpm_and_ddim_calls_never_replay_a_stale_graph():
    """DDPM -> DDIM S=50 (eta 0) -> DDIM S=50 (eta 0.5: same graph, tables refreshed in place) -> DDIM S=20 -> DDPM on one model; each
    result equals the same call on a fresh DiffusionPoint over the same weights."""
    from diffuscene_amd.sampler import _DDIMGraph
    shape = (2, 12, 62)
    cond = W.synth_condition(2, 12, 128, seed=4).contiguous().to(dev())
    T_ = 100
    calls = [("ddpm", None, None, 71), ("ddim", 50, 0.0, 72), ("ddim", 50, 0.5, 73), ("ddim", 20, 0.3, 74), ("ddpm", None, None, 75)]

    def run(diff, kind, S, eta, seed):
        if kind == "ddpm":
            return diff.gen_samples(shape, dev(), condition=cond, noise_fn=_replay(noise_list([shape] * (T_ + 1), seed, "il_")),
                                    clip_denoised=True)
        return diff.gen_samples_ddim(shape, dev(), condition=cond, noise_fn=_replay(noise_list([shape] * S, seed, "il_")),
                                     sampling_timesteps=S, ddim_sampling_eta=eta)

    one = _point("traj.S10", time_num=T_)
    seen = []
    with torch.no_grad():
        for kind, S, eta, seed in calls:
            got = run(one, kind, S, eta, seed)
            want = run(_point("traj.S10", time_num=T_), kind, S, eta, seed)
            assert torch.equal(got, want), (kind, S, eta)
            (g,) = one.diffusion._graphs.values()
            assert isinstance(g, _DDIMGraph) == (kind == "ddim") and (kind == "ddpm" or g.S == S)
            seen.append((g, g.coef.data_ptr() if kind == "ddim" else None))
    assert seen[1][0] is seen[2][0] and seen[1][1] == seen[2][1]          # eta changed: the live graph and its tables stayed
    assert seen[2][0] is not seen[3][0]


# ------------------------------------------------------------------------------------------------ public entry points
class _FakeBertCache:
    def batch(self, texts, device):
        from oracle.make_golden_wrapper import fake_bert_features
        return fake_bert_features(list(texts)).to(device)


@pytest.mark.parametrize("case", ["uncond", "text"])
def test_public_entry_points_with_sampling_timesteps(case, golden_dir, tmp_path, monkeypatch):
    from diffuscene_amd import sampler
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    from oracle.make_golden_wrapper import N, network_config, sample_text_arg, wrapper_state_dict
    calls = []
    orig = sampler.graph_ddim_sample_loop
    monkeypatch.setattr(sampler, "graph_ddim_sample_loop", lambda *a, **k: (calls.append(a[6]), orig(*a, **k))[1])
    monkeypatch.delenv("DSC_GRAPH", raising=False)
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = network_config(case, str(stats), 1000)
    if case == "text":
        cfg["text_bert_cached"] = True
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
    m.load_state_dict(wrapper_state_dict(m))
    m.to(dev())
    m.eval()
    if case == "text":
        m.attach_bert_cache(_FakeBertCache())
    text = sample_text_arg(case)
    C = cfg["point_dim"]
    room = torch.zeros(4, 1, 64, 64, device=dev())
    g = np.load(os.path.join(golden_dir, "wrapper.npz"))
    keys = sorted(k[len(case) + 8:] for k in g.files if k.startswith(case + ".layout."))
    torch.manual_seed(3)
    with quiet:
        d = m.generate_layout(room[:1], N, C, batch_size=1, text=None if text is None else text[:1], clip_denoised=True,
                              sampling_timesteps=50)
        scenes = m.generate_layout_batched(room, N, C, 4, text=text, clip_denoised=True, sampling_timesteps=50,
                                           ddim_sampling_eta=0.2)
    assert calls == [50, 50]
    assert sorted(d) == keys
    for k, v in d.items():
        assert v.device.type == "cpu" and v.shape[0] == 1 and tuple(v.shape[2:]) == tuple(g[case + ".layout." + k].shape[2:])
        assert torch.isfinite(v).all()
    assert len(scenes) == 4 and all(sorted(s) == keys and s["translations"].shape[0] == 1 for s in scenes)
