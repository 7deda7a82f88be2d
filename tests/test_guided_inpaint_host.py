"""Text-guided in-painting on the host: the two new C symbols, the refusals of ``guidance_scale`` on ``inpaint_scene_batched`` (all of
them before anything is drawn), ``guidance_scale=None`` as the call it was, the argument checks of the two loops, and a float32 CPU
restatement of both guided masked loops -- written here from oracle.ref_torch's q_sample / p_sample_step and the reference's DDIM
expressions -- against tests/golden/guided_inpaint.npz (tools/make_golden_guided_inpaint.py: the REAL reference one scene at a time around
the select and the guided bridge), which pins the fixture without a GPU."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from oracle.make_golden_wrapper import fake_bert_features

from test_cfg_host import C, D, L, N, RTOL, _cpu_model, _guided, _wrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsc_p_sample_masked_cfg_f32", "dsc_ddim_masked_cfg_step_f32")


def _tool():
    import tools.make_golden_guided_inpaint as tool
    return tool


def test_header_declares_and_library_exports_the_new_symbols():
    from diffuscene_amd import _lib, ops, sampler
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint, GaussianDiffusion
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dsc_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, "%s not declared in include/diffuscene_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), "%s not exported / bound" % name
    assert callable(ops.p_sample_masked_cfg) and callable(ops.ddim_masked_cfg_step)
    assert callable(sampler.graph_masked_guided_loop) and callable(sampler.graph_ddim_masked_guided_loop)
    for cls, schedule in ((sampler._MaskedGuidedGraph, sampler._PosteriorLoop), (sampler._DDIMMaskedGuidedGraph, sampler._DDIMLoop)):
        assert issubclass(cls, schedule) and cls.given is sampler._Masked and cls.guided is True      # the row: all three parts
    assert callable(GaussianDiffusion.p_sample_loop_masked_guided) and callable(GaussianDiffusion.ddim_masked_guided_loop)
    assert callable(DiffusionPoint.inpaint_samples_guided) and callable(DiffusionPoint.inpaint_samples_guided_ddim)


# ------------------------------------------------------------------------------------------------------------------- the wrapper
def _recording(m):
    """``m.diffusion`` (test_cfg_host._Recorder) with the four in-painting entry points recorded too."""
    rec = m.diffusion
    for name in ("inpaint_samples", "inpaint_samples_ddim", "inpaint_samples_guided", "inpaint_samples_guided_ddim"):
        setattr(rec, name, lambda shape, device, _n=name, **kw: rec._rec(_n, shape, kw))
    return m


def test_guidance_scale_reaches_the_guided_loops_and_none_passes_no_new_keyword_down(tmp_path):
    m = _recording(_wrapper("text", tmp_path))
    room = torch.zeros(3, 1, 64, 64)
    text = ["a", "b", "c"]
    boxes = torch.zeros(3, N, C)
    mask = torch.zeros(3, N, dtype=torch.bool)
    with contextlib.redirect_stdout(io.StringIO()):
        m.inpaint_scene_batched(room, N, C, boxes, mask, text=text)
        m.inpaint_scene_batched(room, N, C, boxes, mask, text=text, sampling_timesteps=50, guidance_scale=None)
        m.inpaint_scene_batched(room, N, C, boxes, mask, text=text, guidance_scale=[0, 1.5, 3], clip_denoised=True)
        m.inpaint_scene_batched(room, N, C, boxes, mask, text=text, guidance_scale=2.0, sampling_timesteps=50, ddim_sampling_eta=0.5)
    calls = m.diffusion.calls
    assert [c[0] for c in calls] == ["inpaint_samples", "inpaint_samples_ddim", "inpaint_samples_guided", "inpaint_samples_guided_ddim"]
    assert set(calls[0][2]) == {"condition", "condition_cross", "clip_denoised", "known", "mask"}          # None: the call as it was
    assert set(calls[1][2]) == {"condition", "condition_cross", "known", "mask", "sampling_timesteps", "ddim_sampling_eta"}
    assert calls[2][2]["guidance_scale"].tolist() == [0.0, 1.5, 3.0] and calls[2][2]["clip_denoised"] is True
    assert calls[3][2]["guidance_scale"].tolist() == [2.0] * 3 and calls[3][2]["sampling_timesteps"] == 50 and calls[3][2]["ddim_sampling_eta"] == 0.5
    assert "clip_denoised" not in calls[3][2] and all(c[1] == (3, N, C) for c in calls)
    assert tuple(calls[2][2]["condition_cross"].shape) == (3, L, D) and tuple(calls[2][2]["mask"].shape) == (3, N, C)


def test_guidance_scale_refusals_come_before_anything_is_drawn(tmp_path):
    room = torch.zeros(2, 1, 64, 64)
    text = ["a", "b"]
    boxes = torch.zeros(2, N, C)
    mask = torch.zeros(2, N, dtype=torch.bool)
    torch.manual_seed(5)
    untouched = torch.get_rng_state()
    un = _recording(_wrapper("uncond", tmp_path))
    torch.manual_seed(5)
    with pytest.raises(ValueError, match="text_condition"):                         # a model without text_condition
        un.inpaint_scene_batched(room, N, C, boxes, mask, text=text, guidance_scale=2.0)
    m = _recording(_wrapper("text", tmp_path))
    torch.manual_seed(5)
    with pytest.raises(ValueError, match="text"):                                   # text=None
        m.inpaint_scene_batched(room, N, C, boxes, mask, guidance_scale=2.0)
    for bad in (float("nan"), [1.0], [1.0, 2.0, 3.0], "x"):
        with pytest.raises(ValueError, match="guidance_scale"):
            m.inpaint_scene_batched(room, N, C, boxes, mask, text=text, guidance_scale=bad)
    flat = torch.zeros(2, D)
    m._text_condition = lambda text, desc_emb, device, desc_bert=None: flat         # e.g. the CLIP encoder: (B, D), not 3-D
    with contextlib.redirect_stdout(io.StringIO()):
        for kw in ({}, dict(sampling_timesteps=10)):
            with pytest.raises(ValueError, match="3|L, text_embed_dim"):
                m.inpaint_scene_batched(room, N, C, boxes, mask, text=text, guidance_scale=2.0, **kw)
    assert torch.equal(torch.get_rng_state(), untouched)                            # not even the CPU draw the method keeps
    assert m.diffusion.calls == [] and un.diffusion.calls == []
    # the models that condition on a prefix / a sub-shape stay refused, guidance or not
    part = _recording(_wrapper("partial", tmp_path))
    with pytest.raises(ValueError, match="room_partial_condition"):
        part.inpaint_scene_batched(room, N, C, boxes, mask, guidance_scale=2.0)


def test_guided_masked_loops_check_their_arguments_on_the_cpu():
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    gd = GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, 50),
                           "mse", "v", "fixedsmall", False, False, None)
    shape = (2, N, C)
    cross = torch.zeros(2, L, D)
    known, mask = torch.zeros(shape), torch.zeros(shape, dtype=torch.bool)
    for loop, kw in ((gd.p_sample_loop_masked_guided, {}), (gd.ddim_masked_guided_loop, dict(sampling_timesteps=10))):
        for bad_cross in (None, torch.zeros(2, D), torch.zeros(3, L, D)):
            with pytest.raises(ValueError, match="condition_cross"):
                loop(None, shape, "cpu", None, bad_cross, 2.0, known=known, mask=mask, **kw)
        for bad in (float("inf"), [1.0, 2.0, 3.0]):
            with pytest.raises(ValueError, match="guidance_scale"):
                loop(None, shape, "cpu", None, cross, bad, known=known, mask=mask, **kw)
        with pytest.raises(ValueError, match="known"):
            loop(None, shape, "cpu", None, cross, 2.0, known=None, mask=mask, **kw)
        with pytest.raises(ValueError, match="mask"):
            loop(None, shape, "cpu", None, cross, 2.0, known=known, mask=mask.float(), **kw)
    for S, eta in ((0, 0.0), (51, 0.0), (10, 1.5)):
        with pytest.raises(ValueError):
            gd.ddim_masked_guided_loop(None, shape, "cpu", None, cross, 2.0, sampling_timesteps=S, ddim_sampling_eta=eta, known=known, mask=mask)


# ------------------------------------------------------------------------------------------------------------------- the fixture
def _restated_tstep(tb, denoise, T, clip, mt, cross, w, known, mask, main, kn):
    x = main[0]
    for i, step in enumerate(reversed(range(T))):
        t = torch.full((x.shape[0],), step, dtype=torch.int64)
        x = torch.where(mask, R.q_sample(tb, known, t, kn[i]), x)
        x = R.p_sample_step(tb, x, t, _guided(denoise, x, t, cross, w), main[i + 1], clip, mt)
    return torch.where(mask, known, x)


def _restated_ddim(tb, denoise, T, S, eta, mt, cross, w, known, mask, main, kn):
    """ddim_sample_loop (reference :402-444) with model_predictions(clip_x_start=True) (:242-264) on the guided output; the select in
    front of every model call and after the last pair."""
    times = list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))
    ac = tb["alphas_cumprod"]
    x = main[0]
    for j, (time, time_next) in enumerate(zip(times[:-1], times[1:])):
        t = torch.full((x.shape[0],), time, dtype=torch.int64)
        x = torch.where(mask, R.q_sample(tb, known, t, kn[j]), x)
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
        x = x0 * alpha_next.sqrt() + c * pred_noise + sigma * main[j + 1]
    return torch.where(mask, known, x)


@pytest.mark.parametrize("name", ["v.T1000", "eps.T50", "ddim.S20.eta0", "ddim.S7.eta0.5"])
def test_cpu_restatement_of_the_guided_masked_loops_reproduces_the_fixture(name, golden_dir, tmp_path):
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "guided_inpaint.npz"))
    mt, T, S, eta, clip, seed = tool.CASES[name]
    sd, kw, wsd, _ = _cpu_model(tmp_path, T)
    Bc = tool.B
    cond = wsd["positional_embedding"][None].expand(Bc, -1, -1).contiguous()
    cross = torch.nn.functional.linear(fake_bert_features(tool.case_texts()), wsd["fc_text_f.weight"], wsd["fc_text_f.bias"])
    w = torch.tensor(tool.SCALES, dtype=torch.float32)[:, None, None]
    tb = R.schedule_tables(1e-4, 0.02, T, mt)
    known, mask, main, kn = tool.chain_inputs(name)
    torch.set_num_threads(min(8, os.cpu_count() or 1))

    def denoise(x, t, cr):
        return R.unet1d_forward(sd, kw, x, t, cond, cr)

    with torch.no_grad():
        if S is None:
            y = _restated_tstep(tb, denoise, T, clip, mt, cross, w, known, mask, main, kn)
        else:
            y = _restated_ddim(tb, denoise, T, S, eta, mt, cross, w, known, mask, main, kn)
    want = torch.from_numpy(g[name])
    rel = float((y - want).abs().max() / want.abs().max())
    print("%s: restatement vs fixture, max-abs / max-abs %.3g" % (name, rel))
    assert rel < RTOL, (name, rel)
    assert torch.equal(y[mask], known[mask]) and torch.equal(want[mask], known[mask])


def test_every_chain_meets_the_chain_criterion_and_the_fixture_lists_the_documented_cases(golden_dir):
    """The stored reference sensitivity (reference float32 against the float64 run) of every chain is at most the project's chain
    criterion, 5e-6 norm-relative and 1e-4 element-wise; masks, scales and chains are the documented ones; the file holds outputs only."""
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "guided_inpaint.npz"))
    assert tool.B == 3 and tool.SCALES == (0.0, 1.5, 3.0) and (tool.N, tool.C) == (12, 62) and tool.CRITERION == (5e-6, 1e-4)
    assert sorted(tool.CASES) == sorted(["v.T1000", "eps.T50", "ddim.S20.eta0", "ddim.S7.eta0.5"])
    assert tool.CASES["v.T1000"][:5] == ("v", 1000, None, 0.0, True) and tool.CASES["eps.T50"][:5] == ("eps", 50, None, 0.0, False)
    assert tool.CASES["ddim.S20.eta0"][:4] == ("v", 1000, 20, 0.0) and tool.CASES["ddim.S7.eta0.5"][:4] == ("v", 1000, 7, 0.5)
    assert sorted(g.files) == sorted(list(tool.CASES) + [n + ".sens" for n in tool.CASES])
    m = tool.scene_masks()
    rows = m.all(dim=2)
    assert rows[0].tolist() == [True] * 4 + [False] * 8 and not m[0, 4:].any()          # scene 0: whole rows [0, 4)
    chan = torch.zeros(tool.C, dtype=torch.bool)
    chan[3:6] = chan[8:30] = True
    assert bool((m[1] == chan[None, :]).all())                                           # scene 1: sizes and class_labels of all rows
    per_row = m[2].sum(dim=1)
    assert 0 < int(m[2].sum()) == len(tool.SCATTER) and int(per_row.max()) <= 3 and int((per_row == 0).sum()) >= 3      # scene 2: scattered
    for name in tool.CASES:
        y = g[name]
        assert tuple(y.shape) == (3, 12, 62) and y.dtype == np.float32 and np.isfinite(y).all()
        known, mask = tool.chain_inputs(name)[:2]
        assert float(known.abs().max()) <= 1.0
        assert np.array_equal(y[mask.numpy()], known.numpy()[mask.numpy()])
        sr, sew = (float(v) for v in g[name + ".sens"])
        print("%s: reference sensitivity norm-relative %.3g, element-wise %.3g" % (name, sr, sew))
        assert 0 <= sr <= 5e-6 and 0 <= sew <= 1e-4, (name, sr, sew)
        assert tool.MEASURED_SENSITIVITIES[name] == (float("%.2g" % sr), float("%.2g" % sew))      # the docstring's record is the file's
        # the scenes' free parts differ far beyond the bound the GPU test uses
        free = ~(mask[0] | mask[1]).numpy()
        spread = float(np.abs(y[1] - y[0])[free].max() / np.abs(y).max())
        assert spread > 100 * max(5e-6, 4 * sr), (name, spread)
    assert os.path.getsize(os.path.join(golden_dir, "guided_inpaint.npz")) <= 1.25 * os.path.getsize(os.path.join(golden_dir, "cfg.npz"))
