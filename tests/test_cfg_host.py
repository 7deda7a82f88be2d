"""Classifier-free guidance on the host: the four new C symbols, ``ops.guidance_scales`` on every accepted form and every refusal, the
refusals of ``guidance_scale`` on the wrapper, the draws of ``text_drop_prob`` up to the first device op, and a CPU restatement of both
guided loops and of the gated training loss -- written here from oracle.ref_torch's p_sample_step / p_losses and the reference's DDIM
expressions -- against tests/golden/cfg.npz (tools/make_golden_cfg.py: the REAL reference around the bridged guided denoiser), which
pins the fixture without a GPU."""
import contextlib
import io
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from oracle import weights as W
from oracle.make_golden_wrapper import fake_bert_features, network_config, wrapper_batch, wrapper_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsc_cfg_combine_f32", "dsc_p_sample_cfg_f32", "dsc_ddim_cfg_step_f32", "dsc_scene_gate_f32")
RTOL = 2e-5            # tests/test_oracle.py: oracle vs real reference


def _tool():
    import tools.make_golden_cfg as tool
    return tool


def test_header_declares_and_library_exports_the_new_symbols():
    from diffuscene_amd import _lib, autograd_ops, ops, sampler
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint, GaussianDiffusion
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dsc_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, "%s not declared in include/diffuscene_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), "%s not exported / bound" % name
    for name in ("cfg_combine", "p_sample_cfg", "ddim_cfg_step", "scene_gate", "guidance_scales"):
        assert callable(getattr(ops, name))
    assert callable(autograd_ops.SceneGateFn.apply)
    assert callable(sampler.graph_guided_loop) and callable(sampler.graph_ddim_guided_loop)
    assert callable(GaussianDiffusion.p_sample_loop_guided) and callable(GaussianDiffusion.ddim_guided_loop)
    assert callable(DiffusionPoint.gen_samples_guided) and callable(DiffusionPoint.gen_samples_guided_ddim)


# ------------------------------------------------------------------------------------------------------------------- ops.guidance_scales
def test_guidance_scales_normalises_every_accepted_form():
    from diffuscene_amd import ops
    for scale, want in ((2.5, [2.5] * 3), (0, [0.0] * 3), (-0.5, [-0.5] * 3), ([0, 1.5, 3], [0.0, 1.5, 3.0]), ((0.0, 1.5, 3.0), [0.0, 1.5, 3.0]),
                        (torch.tensor([0.0, 1.5, 3.0]), [0.0, 1.5, 3.0]), (torch.tensor([0, 1, 3]), [0.0, 1.0, 3.0]),
                        (torch.tensor(2.0), [2.0] * 3), (np.array([0.0, 1.5, 3.0]), [0.0, 1.5, 3.0]), (np.float32(2.0), [2.0] * 3),
                        (torch.tensor([0.0, 1.5, 3.0], dtype=torch.float64), [0.0, 1.5, 3.0])):
        out = ops.guidance_scales(scale, 3, "cpu")
        assert out.dtype == torch.float32 and tuple(out.shape) == (3,) and out.is_contiguous()
        assert out.tolist() == want, (scale, out)
    assert ops.guidance_scales([7.0], 1, "cpu").tolist() == [7.0]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), [0.0, float("nan"), 1.0], torch.tensor([0.0, float("inf"), 1.0]),
                                 [1.0, 2.0], [1.0, 2.0, 3.0, 4.0], torch.zeros(2), torch.zeros(3, 1), torch.zeros(1, 3), [], None, "2.0", True,
                                 ["a", "b", "c"], torch.tensor([True, False, True]), [[1.0], [2.0], [3.0]]])
def test_guidance_scales_refuses_non_finite_values_and_wrong_lengths(bad):
    from diffuscene_amd import ops
    with pytest.raises(ValueError, match="guidance_scale"):
        ops.guidance_scales(bad, 3, "cpu")


# ------------------------------------------------------------------------------------------------------------------- the wrapper
class _Recorder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def _rec(self, name, shape, kw):
        self.calls.append((name, tuple(shape), kw))
        return torch.zeros(shape)

    def gen_samples(self, shape, device, **kw):
        return self._rec("gen_samples", shape, kw)

    def gen_samples_ddim(self, shape, device, **kw):
        return self._rec("gen_samples_ddim", shape, kw)

    def gen_samples_guided(self, shape, device, **kw):
        return self._rec("gen_samples_guided", shape, kw)

    def gen_samples_guided_ddim(self, shape, device, **kw):
        return self._rec("gen_samples_guided_ddim", shape, kw)


N, C, L, D = 12, 62, 7, 512


def _wrapper(case, tmp_path, **extra):
    """The wrapper of a reference config on the CPU with a recording diffusion and a text encoder that returns CPU features."""
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = network_config(case, str(stats))
    if case == "text":
        cfg["text_bert_cached"] = True
    cfg.update(extra)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
    m.diffusion = _Recorder()
    m.delete_empty_per_scene = lambda samples, keep_empty=False: list(samples)     # its compaction is a device kernel
    m.delete_empty_from_network_samples = lambda samples, device="cpu", keep_empty=False: samples
    if case == "text":
        feats = {}

        def text_condition(text, desc_emb, device, desc_bert=None):               # fc_text_f is a device GEMM: stand-in features
            n = len(text) if text is not None else desc_bert.shape[0]
            return feats.setdefault(n, torch.randn((n, L, D), generator=torch.Generator().manual_seed(n)))
        m._text_condition = text_condition
    return m.eval()


def test_guidance_scale_reaches_the_guided_loops_and_none_is_the_old_path(tmp_path):
    m = _wrapper("text", tmp_path)
    room = torch.zeros(3, 1, 64, 64)
    text = ["a", "b", "c"]
    with contextlib.redirect_stdout(io.StringIO()):
        m.generate_layout_batched(room, N, C, 3, text=text)
        m.generate_layout_batched(room, N, C, 3, text=text, sampling_timesteps=50)
        m.generate_layout_batched(room, N, C, 3, text=text, guidance_scale=[0, 1.5, 3], clip_denoised=True)
        m.generate_layout_batched(room, N, C, 3, text=text, guidance_scale=2.0, sampling_timesteps=50, ddim_sampling_eta=0.5)
        m.generate_layout(room[:1], N, C, batch_size=1, text=text[:1], guidance_scale=2.0)
        m.sample(room, N, C, batch_size=3, text=text, guidance_scale=torch.tensor([1.0, 2.0, 3.0]))
        prog = m.generate_layout_progressive(room[:1], N, C, batch_size=1, text=text[:1], guidance_scale=1.5)
    calls = m.diffusion.calls
    assert [c[0] for c in calls] == ["gen_samples", "gen_samples_ddim", "gen_samples_guided", "gen_samples_guided_ddim", "gen_samples_guided",
                                     "gen_samples_guided", "gen_samples_guided"]
    assert "guidance_scale" not in calls[0][2] and "guidance_scale" not in calls[1][2]            # None: the call as it was
    assert set(calls[0][2]) == {"condition", "condition_cross", "clip_denoised"}
    assert calls[2][2]["guidance_scale"].tolist() == [0.0, 1.5, 3.0] and calls[2][2]["clip_denoised"] is True
    assert calls[3][2]["guidance_scale"].tolist() == [2.0] * 3 and calls[3][2]["sampling_timesteps"] == 50 and calls[3][2]["ddim_sampling_eta"] == 0.5
    assert calls[4][1] == (1, N, C) and calls[4][2]["guidance_scale"].tolist() == [2.0]
    assert calls[5][2]["guidance_scale"].tolist() == [1.0, 2.0, 3.0]
    assert tuple(calls[2][2]["condition_cross"].shape) == (3, L, D)
    assert list(prog) == [0]


def test_guidance_scale_refusals(tmp_path):
    room = torch.zeros(2, 1, 64, 64)
    text = ["a", "b"]
    un = _wrapper("uncond", tmp_path)
    for fn, kw in ((un.sample, {}), (un.generate_layout, {}), (un.generate_layout_batched, {}), (un.generate_layout_progressive, {})):
        with pytest.raises(ValueError, match="text_condition"):                     # a model without text_condition
            fn(room, N, C, 2, text=text, guidance_scale=2.0, **kw)
    m = _wrapper("text", tmp_path)
    for fn in (m.sample, m.generate_layout, m.generate_layout_batched, m.generate_layout_progressive):
        with pytest.raises(ValueError, match="text"):                               # text=None
            fn(room, N, C, 2, guidance_scale=2.0)
    flat = torch.zeros(2, D)
    m._text_condition = lambda text, desc_emb, device, desc_bert=None: flat         # e.g. the CLIP encoder: (B, D), not 3-D
    with contextlib.redirect_stdout(io.StringIO()):
        for fn in (m.sample, m.generate_layout, m.generate_layout_batched):
            with pytest.raises(ValueError, match="3|L, text_embed_dim"):
                fn(room, N, C, 2, text=text, guidance_scale=2.0)
    m = _wrapper("text", tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        for bad in (float("nan"), [1.0], [1.0, 2.0, 3.0], "x"):
            with pytest.raises(ValueError, match="guidance_scale"):
                m.generate_layout_batched(room, N, C, 2, text=text, guidance_scale=bad)
        with pytest.raises(ValueError, match="generation only"):
            m.sample(room, N, C, 2, text=text, partial_boxes=torch.zeros(2, 3, C), guidance_scale=2.0)
        with pytest.raises(ValueError, match="generation only"):
            m.sample(room, N, C, 2, text=text, input_boxes=torch.zeros(2, N, C), guidance_scale=2.0)
    assert m.diffusion.calls == [] and un.diffusion.calls == []
    # completion, re-arrangement and in-painting do not take the keyword
    for fn in (m.complete_scene, m.arrange_scene, m.complete_scene_batched, m.arrange_scene_batched, m.inpaint_scene_batched):
        with pytest.raises(TypeError):
            fn(room, N, C, torch.zeros(2, N, C), guidance_scale=2.0)


def test_guided_loops_check_their_arguments_on_the_cpu():
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    gd = GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, 50),
                           "mse", "v", "fixedsmall", False, False, None)
    shape = (2, N, C)
    cross = torch.zeros(2, L, D)
    for bad_cross in (None, torch.zeros(2, D), torch.zeros(3, L, D)):
        with pytest.raises(ValueError, match="condition_cross"):
            gd.p_sample_loop_guided(None, shape, "cpu", None, bad_cross, 2.0)
        with pytest.raises(ValueError, match="condition_cross"):
            gd.ddim_guided_loop(None, shape, "cpu", None, bad_cross, 2.0, sampling_timesteps=10)
    for bad in (float("inf"), [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="guidance_scale"):
            gd.p_sample_loop_guided(None, shape, "cpu", None, cross, bad)
    for S, eta in ((0, 0.0), (51, 0.0), (10, 1.5)):
        with pytest.raises(ValueError):
            gd.ddim_guided_loop(None, shape, "cpu", None, cross, 2.0, sampling_timesteps=S, ddim_sampling_eta=eta)
    # a stride-0 (per-slot) condition stays per-slot at 2 B; the null half of condition_cross is zeros
    cond = torch.randn(1, N, 128).expand(2, -1, -1)
    c2, x2, w = gd._guided_inputs(shape, "cpu", cond, cross + 1.0, [0.5, 2.0], "test")
    assert tuple(c2.shape) == (4, N, 128) and c2.stride(0) == 0 and w.tolist() == [0.5, 2.0]
    assert tuple(x2.shape) == (4, L, D) and bool((x2[:2] == 1).all()) and not x2[2:].any()
    dense = torch.randn(2, N, 128)
    c2, _, _ = gd._guided_inputs(shape, "cpu", dense, cross, 1.0, "test")
    assert torch.equal(c2[:2], dense) and torch.equal(c2[2:], dense)


# ------------------------------------------------------------------------------------------------------------------- text_drop_prob
def _text_batch():
    s, _ = wrapper_batch("text")
    return s


def _state_after(m, s, train, expect_gate):
    """CPU generator state after _loss_inputs' host logic: the call runs up to the first device op (the gate kernel refuses CPU tensors)."""
    m.train(train)
    torch.manual_seed(11)
    if expect_gate:
        with pytest.raises(RuntimeError, match="HIP device"):
            m._loss_inputs(s)
    else:
        m._loss_inputs(s)
    m.eval()
    return torch.get_rng_state()


def test_text_drop_prob_makes_one_draw_in_training_mode_and_none_otherwise(tmp_path):
    s = _text_batch()
    Bt = s["class_labels"].shape[0]
    torch.manual_seed(11)
    untouched = torch.get_rng_state()
    plain = _wrapper("text", tmp_path)
    assert plain.text_drop_prob == 0.0
    for train in (False, True):
        assert torch.equal(_state_after(plain, s, train, False), untouched)          # no key: no draw
    zero = _wrapper("text", tmp_path, text_drop_prob=0.0)
    assert torch.equal(_state_after(zero, s, True, False), untouched)                # p == 0: no draw
    m = _wrapper("text", tmp_path, text_drop_prob=0.3)
    assert torch.equal(_state_after(m, s, False, False), untouched)                  # eval mode: no draw
    got = _state_after(m, s, True, True)
    torch.manual_seed(11)
    u = torch.rand((Bt,))
    assert torch.equal(got, torch.get_rng_state())                                   # exactly one (B,) draw
    m.train()
    torch.manual_seed(11)
    keep = m._text_keep(s, Bt, "cpu")
    m.eval()
    assert keep.dtype == torch.bool and torch.equal(keep, u >= 0.3)
    # _cond_keep overrides the draw, in any mode
    forced = dict(s, _cond_keep=torch.tensor([True, False, True, False]))
    for model, train in ((m, True), (m, False), (plain, False)):
        assert torch.equal(_state_after(model, forced, train, True), untouched)
    assert torch.equal(m._text_keep(forced, Bt, "cpu"), forced["_cond_keep"])
    for bad in (torch.tensor([True, False]), torch.tensor([1, 0, 1, 0]), torch.ones(4)):
        with pytest.raises(ValueError, match="_cond_keep"):
            m._loss_inputs(dict(s, _cond_keep=bad))
    with pytest.raises(ValueError, match="text_drop_prob"):
        _wrapper("text", tmp_path, text_drop_prob=1.5)


# ------------------------------------------------------------------------------------------------------------------- the fixture
def _cpu_model(tmp_path, T):
    """(denoiser state dict, net kwargs, wrapper state dict, config) of the text wrapper, on the CPU."""
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = network_config("text", str(stats), T)
    cfg["text_bert_cached"] = True
    with contextlib.redirect_stdout(io.StringIO()):
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
    wsd = wrapper_state_dict(m)
    sd = {k[len("diffusion.model."):]: v for k, v in wsd.items() if k.startswith("diffusion.model.")}
    return sd, cfg["net_kwargs"], wsd, cfg


def _guided(denoise, x, t, cross, w):
    c = denoise(x, t, cross)
    u = denoise(x, t, torch.zeros_like(cross))
    return u + w * (c - u)


def _restated_tstep(tb, denoise, T, clip, mt, cross, w, noise):
    x = noise[0]
    for i, step in enumerate(reversed(range(T))):
        t = torch.full((x.shape[0],), step, dtype=torch.int64)
        x = R.p_sample_step(tb, x, t, _guided(denoise, x, t, cross, w), noise[i + 1], clip, mt)
    return x


def _restated_ddim(tb, denoise, T, S, eta, mt, cross, w, noise):
    """ddim_sample_loop (reference :402-444) with model_predictions(clip_x_start=True) (:242-264) on the guided output."""
    times = list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))
    ac = tb["alphas_cumprod"]
    x = noise[0]
    k = 1
    for time, time_next in zip(times[:-1], times[1:]):
        t = torch.full((x.shape[0],), time, dtype=torch.int64)
        out = _guided(denoise, x, t, cross, w)
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


@pytest.mark.parametrize("name", ["v.T1000", "eps.T50", "ddim.S20.eta0", "ddim.S7.eta0.5"])
def test_cpu_restatement_of_the_guided_loops_reproduces_the_fixture(name, golden_dir, tmp_path):
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "cfg.npz"))
    mt, T, S, eta, clip, seed = tool.CASES[name]
    sd, kw, wsd, _ = _cpu_model(tmp_path, T)
    Bc = tool.B
    cond = wsd["positional_embedding"][None].expand(Bc, -1, -1).contiguous()
    cross = torch.nn.functional.linear(fake_bert_features(tool.case_texts()), wsd["fc_text_f.weight"], wsd["fc_text_f.bias"])
    w = torch.tensor(tool.SCALES, dtype=torch.float32)[:, None, None]
    tb = R.schedule_tables(1e-4, 0.02, T, mt)
    noise = tool.chain_noise(name)
    torch.set_num_threads(min(8, os.cpu_count() or 1))

    def denoise(x, t, cr):
        return R.unet1d_forward(sd, kw, x, t, cond, cr)

    with torch.no_grad():
        if S is None:
            y = _restated_tstep(tb, denoise, T, clip, mt, cross, w, noise)
        else:
            y = _restated_ddim(tb, denoise, T, S, eta, mt, cross, w, noise)
    want = torch.from_numpy(g[name])
    rel = float((y - want).abs().max() / want.abs().max())
    print("%s: restatement vs fixture, max-abs / max-abs %.3g" % (name, rel))
    assert rel < RTOL, (name, rel)


def test_cpu_restatement_of_the_gated_training_loss_reproduces_the_fixture(golden_dir, tmp_path):
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "cfg.npz"))
    sd, kw, wsd, cfg = _cpu_model(tmp_path, 1000)
    s, x0 = wrapper_batch("text")
    Bt = x0.shape[0]
    assert tuple(g["train.keep"].tolist()) == tuple(tool.TRAIN_KEEP) and Bt == tool.TRAIN_B
    keep = torch.tensor(tool.TRAIN_KEEP)[:, None, None]
    wt, bt = wsd["fc_text_f.weight"].clone().requires_grad_(True), wsd["fc_text_f.bias"].clone().requires_grad_(True)
    cond = wsd["positional_embedding"][None].expand(Bt, -1, -1).contiguous()
    feats = torch.nn.functional.linear(fake_bert_features(s["description"]), wt, bt)
    cross = torch.where(keep, feats, torch.zeros_like(feats))
    dk = cfg["diffusion_kwargs"]
    tb = R.schedule_tables(dk.get("beta_start", 1e-4), dk.get("beta_end", 0.02), 1000, dk["model_mean_type"])
    torch.manual_seed(tool.SEED_TRAIN)
    t = torch.randint(0, 1000, size=(Bt,))
    noise = torch.randn(x0.shape)
    lw, scal, _ = R.p_losses(tb, lambda xt, tt: R.unet1d_forward(sd, kw, xt, tt, cond, cross), x0, t, noise, R.dims_from_kwargs(kw),
                             loss_separate=dk.get("loss_separate", False), loss_iou=dk.get("loss_iou", False), stats=W.DATASET_STATS,
                             mean_type=dk["model_mean_type"])
    loss = lw.mean()
    loss.backward()
    want = float(g["train.loss"])
    assert abs(float(loss.detach()) - want) <= RTOL * abs(want), (float(loss.detach()), want)
    parts = [k[len("train.part."):] for k in g.files if k.startswith("train.part.")]
    assert parts
    for k in parts:
        assert k in scal, (k, sorted(scal))
        ref = float(g["train.part." + k])
        assert abs(float(scal[k].detach()) - ref) <= RTOL * max(1.0, abs(ref)), k
    gw, gb = torch.from_numpy(g["train.grad.fc_text_f.weight"]), torch.from_numpy(g["train.grad.fc_text_f.bias"])
    rw = float((wt.grad[list(tool.GRAD_ROWS)] - gw).abs().max() / gw.abs().max())
    rb = float((bt.grad - gb).abs().max() / gb.abs().max())
    print("gated training loss: gradient of fc_text_f, weight rows %.3g, bias %.3g" % (rw, rb))
    assert rw < RTOL and rb < RTOL
    # the select: a dropped scene contributes nothing -- with every scene dropped the gradient is exactly zero
    wt.grad = bt.grad = None
    feats = torch.nn.functional.linear(fake_bert_features(s["description"]), wt, bt)
    cross = torch.where(torch.zeros_like(keep), feats, torch.zeros_like(feats))
    lw, _, _ = R.p_losses(tb, lambda xt, tt: R.unet1d_forward(sd, kw, xt, tt, cond, cross), x0, t, noise, R.dims_from_kwargs(kw),
                          loss_separate=dk.get("loss_separate", False), loss_iou=dk.get("loss_iou", False), stats=W.DATASET_STATS,
                          mean_type=dk["model_mean_type"])
    lw.mean().backward()
    assert not wt.grad.any() and not bt.grad.any()


def test_every_chain_is_pinable_and_the_fixture_lists_the_documented_cases(golden_dir):
    """The stored reference sensitivity (reference float32 against the float64 run) of every chain is at most a quarter of the bound the
    GPU test uses -- max(chain criterion, 4 x sensitivity) per figure -- and small against the criterion's scale, so the bound still
    separates the scenes' scales."""
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "cfg.npz"))
    assert tool.B == 3 and tool.SCALES == (0.0, 1.5, 3.0) and (tool.N, tool.C) == (12, 62)
    assert sorted(tool.CASES) == sorted(["v.T1000", "eps.T50", "ddim.S20.eta0", "ddim.S7.eta0.5"])
    assert tool.CASES["v.T1000"][:5] == ("v", 1000, None, 0.0, True) and tool.CASES["eps.T50"][:5] == ("eps", 50, None, 0.0, False)
    assert tool.CASES["ddim.S20.eta0"][:4] == ("v", 1000, 20, 0.0) and tool.CASES["ddim.S7.eta0.5"][:4] == ("v", 1000, 7, 0.5)
    for name in tool.CASES:
        y = g[name]
        assert tuple(y.shape) == (3, 12, 62) and y.dtype == np.float32 and np.isfinite(y).all()
        sr, sew = (float(v) for v in g[name + ".sens"])
        print("%s: reference sensitivity norm-relative %.3g, element-wise %.3g" % (name, sr, sew))
        assert 0 <= sr <= max(5e-6, 4 * sr) / 4 and 0 <= sew <= max(1e-4, 4 * sew) / 4
        # the scenes differ by their scale far beyond the bound: the bound can tell a wrong scale
        spread = float(np.abs(y[1] - y[0]).max() / np.abs(y).max())
        assert spread > 100 * max(5e-6, 4 * sr), (name, spread)
    assert tuple(g["train.grad.fc_text_f.weight"].shape) == (8, 768) and tuple(g["train.grad.fc_text_f.bias"].shape) == (512,)
    assert os.path.getsize(os.path.join(golden_dir, "cfg.npz")) <= os.path.getsize(os.path.join(golden_dir, "masked.npz"))
