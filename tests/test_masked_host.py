"""Element-wise scene in-painting on the host: the three new C symbols, ``ops.known_mask`` and ``attribute_mask`` on every accepted form
and every refusal, the refusals of ``inpaint_scene_batched``, and a CPU restatement of both masked loops -- written here from
oracle.ref_torch's q_sample / p_sample_step and the reference's DDIM expressions -- against tests/golden/masked.npz
(tools/make_golden_masked.py: the REAL reference, one scene at a time), which pins the fixture without a GPU."""
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
from oracle.make_golden_wrapper import fake_bert_features, network_config, wrapper_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsc_masked_overwrite_f32", "dsc_p_sample_masked_f32", "dsc_ddim_masked_step_f32")
RTOL = 2e-5            # tests/test_oracle.py: oracle vs real reference


def _tool():
    from tools.make_golden_masked import CASES, case_texts, masked_inputs, scene_masks
    return CASES, case_texts, masked_inputs, scene_masks


def test_header_declares_and_library_exports_the_new_symbols():
    from diffuscene_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dsc_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, "%s not declared in include/diffuscene_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), "%s not exported / bound" % name
    for name in ("masked_overwrite", "p_sample_masked", "ddim_masked_step", "known_mask"):
        assert callable(getattr(ops, name))
    from diffuscene_amd import sampler
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint, GaussianDiffusion
    assert callable(sampler.graph_masked_loop) and callable(sampler.graph_ddim_masked_loop)
    assert callable(GaussianDiffusion.p_sample_loop_masked) and callable(GaussianDiffusion.ddim_masked_loop)
    assert callable(DiffusionPoint.inpaint_samples) and callable(DiffusionPoint.inpaint_samples_ddim)


# ------------------------------------------------------------------------------------------------------------------- ops.known_mask
def test_known_mask_normalises_every_accepted_form():
    from diffuscene_amd import ops
    B, N, C = 3, 4, 5
    g = torch.Generator().manual_seed(5)
    full = torch.rand((B, N, C), generator=g) < 0.4
    rows = torch.rand((B, N), generator=g) < 0.5
    for m, want in ((full, full), (full.to(torch.uint8) * 255, full), (full.to(torch.uint8) * 2, full),
                    (rows, rows[:, :, None].expand(B, N, C)), (rows.to(torch.uint8), rows[:, :, None].expand(B, N, C)),
                    (full.transpose(0, 1).contiguous().transpose(0, 1), full)):
        out = ops.known_mask(m, (B, N, C), "cpu")
        assert out.dtype == torch.uint8 and tuple(out.shape) == (B, N, C) and out.is_contiguous()
        assert torch.equal(out != 0, want)
    keep = torch.tensor([[[0, 2, 255, 1, 0]]], dtype=torch.uint8)
    assert torch.equal(ops.known_mask(keep, (1, 1, 5), "cpu"), keep)          # any byte is valid and kept as it is


@pytest.mark.parametrize("bad", [torch.zeros(3, 4, 5), torch.zeros(3, 4, 5, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int32),
                                 torch.zeros(3, 5, dtype=torch.bool), torch.zeros(4, 3, 5, dtype=torch.bool),
                                 torch.zeros(3, 4, 5, 1, dtype=torch.uint8), torch.zeros(60, dtype=torch.bool), [[True] * 4] * 3, None])
def test_known_mask_refuses_other_dtypes_and_shapes(bad):
    from diffuscene_amd import ops
    with pytest.raises(ValueError, match="mask"):
        ops.known_mask(bad, (3, 4, 5), "cpu")


# ------------------------------------------------------------------------------------------------------------------- the wrapper
def _config(golden_dir, tmp_path, yaml="uncond/diffusion_bedrooms_instancond_lat32_v.yaml", **extra):
    import copy
    cfgs = json.load(open(os.path.join(golden_dir, "reference_configs.json")))
    config = copy.deepcopy(cfgs[yaml])
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    config["network"]["diffusion_kwargs"]["train_stats_file"] = str(stats)
    config["network"].update(extra)
    return config


class _Recorder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def inpaint_samples(self, shape, device, **kw):
        self.calls.append(("inpaint_samples", tuple(shape), kw))
        return torch.zeros(shape)

    def inpaint_samples_ddim(self, shape, device, **kw):
        self.calls.append(("inpaint_samples_ddim", tuple(shape), kw))
        return torch.zeros(shape)


def _layout_net(golden_dir, tmp_path, **extra):
    import diffuscene_amd.networks as ours
    config = _config(golden_dir, tmp_path, **extra)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net, _, _ = ours.build_network(None, 22, config, None, device="cpu")
    net.diffusion = _Recorder()
    net.delete_empty_per_scene = lambda samples, keep_empty=False: list(samples)     # its compaction is a device kernel
    net.eval()
    return net, config["network"]["sample_num_points"], config["network"]["point_dim"]


@pytest.fixture
def layout_net(golden_dir, tmp_path):
    return _layout_net(golden_dir, tmp_path)


def test_attribute_mask_marks_the_channel_slices_of_split_boxes(layout_net):
    net, N, C = layout_net
    B = 3
    probe = torch.arange(C, dtype=torch.float32).expand(1, N, C).contiguous()          # every element holds its channel index
    split = net._split_boxes(probe)
    for name in net.ATTRIBUTES:
        m = net.attribute_mask(N, (name,), B, N)
        assert m.dtype == torch.bool and tuple(m.shape) == (B, N, C)
        assert bool((m == m[0, 0]).all())
        chans = set(torch.nonzero(m[0, 0]).flatten().tolist())
        got = set(int(v) for v in split[name][0, 0].tolist())
        if name == "class_labels":
            got.add(net.bbox_dim + net.class_dim - 1)                                   # the 'empty' column goes with the class
        assert chans == got, name
    every = net.attribute_mask(N, net.ATTRIBUTES, B, N)
    assert bool(every.all())                                                            # the five attributes tile the row
    assert torch.equal(net.attribute_mask(N, "sizes", B, N), net.attribute_mask(N, ("sizes",), B, N))


def test_attribute_mask_accepts_counts_index_lists_and_bool_rows(layout_net):
    net, N, C = layout_net
    B = 3
    tr = net.translation_dim
    by_count = net.attribute_mask([0, 2, N], ("translations",), B, N)
    assert torch.equal(by_count, net.attribute_mask(torch.tensor([0, 2, N]), ("translations",), B, N))
    rows = by_count.any(-1)
    assert rows.sum(1).tolist() == [0, 2, N] and bool(rows[1, :2].all()) and bool(by_count[:, :, tr:].logical_not().all())
    by_index = net.attribute_mask([[], [1, 5, N - 1], torch.tensor([0])], ("translations",), B, N)
    assert [torch.nonzero(r).flatten().tolist() for r in by_index.any(-1)] == [[], [1, 5, N - 1], [0]]
    sel = torch.zeros(B, N, dtype=torch.bool)
    sel[1, [1, 5, N - 1]] = True
    sel[2, 0] = True
    assert torch.equal(net.attribute_mask(sel, ("translations",), B, N), by_index)
    assert torch.equal(net.attribute_mask(2, ("angles",), B, N), net.attribute_mask([2, 2, 2], ("angles",), B, N))
    both = net.attribute_mask(4, ("translations",), B, N) | net.attribute_mask([[6, 7]] * B, ("class_labels",), B, N)
    assert int(both[0].sum()) == 4 * tr + 2 * net.class_dim
    assert not net.attribute_mask(N, (), B, N).any()


def test_attribute_mask_refusals_name_the_scene_or_argument(layout_net):
    net, N, C = layout_net
    with pytest.raises(ValueError, match="attributes"):
        net.attribute_mask(N, ("colours",), 2, N)
    with pytest.raises(ValueError, match="scene 1"):
        net.attribute_mask([0, N + 1], ("sizes",), 2, N)
    with pytest.raises(ValueError, match="scene 1"):
        net.attribute_mask([[0], [N]], ("sizes",), 2, N)
    with pytest.raises(ValueError, match="scene 0"):
        net.attribute_mask([-1, 0], ("sizes",), 2, N)
    with pytest.raises(ValueError, match="scene 0"):
        net.attribute_mask([1.5, 0], ("sizes",), 2, N)
    with pytest.raises(ValueError, match="rows"):
        net.attribute_mask([1, 2, 3], ("sizes",), 2, N)
    with pytest.raises(ValueError, match="rows"):
        net.attribute_mask(torch.zeros(2, N + 1, dtype=torch.bool), ("sizes",), 2, N)
    with pytest.raises(ValueError, match="rows"):
        net.attribute_mask(torch.zeros(2, N), ("sizes",), 2, N)
    net.objfeat_dim = 0                                          # a model without object features
    with pytest.raises(ValueError, match="objfeats"):
        net.attribute_mask(N, ("objfeats",), 2, N)


def test_inpaint_scene_batched_reaches_the_loops_with_normalised_inputs(layout_net):
    net, N, C = layout_net
    B = 3
    room = torch.zeros(B, 1, 64, 64)
    g = torch.Generator().manual_seed(9)
    boxes = torch.randn((B, N, C), generator=g)
    mask = net.attribute_mask([1, N, 0], ("sizes", "class_labels"), B, N)
    res = net.inpaint_scene_batched(room, N, C, boxes, mask, clip_denoised=True)
    (kind, shape, kw), = net.diffusion.calls
    assert kind == "inpaint_samples" and shape == (B, N, C) and len(res) == B
    assert set(kw) == {"condition", "condition_cross", "clip_denoised", "known", "mask"} and kw["clip_denoised"] is True
    assert torch.equal(kw["known"], boxes) and kw["mask"].dtype == torch.uint8 and torch.equal(kw["mask"] != 0, mask)
    assert tuple(kw["condition"].shape[:2]) == (B, N) and kw["condition_cross"] is None
    # a list of shorter scenes: padded with zeros, padded rows never known; (B, N) row masks; the strided switch
    net.diffusion.calls.clear()
    scenes = [boxes[0, :2], boxes[1], boxes[2, :0]]
    rows = torch.ones(B, N, dtype=torch.uint8)
    net.inpaint_scene_batched(room, N, C, scenes, rows, sampling_timesteps=20, ddim_sampling_eta=0.3)
    (kind, shape, kw), = net.diffusion.calls
    assert kind == "inpaint_samples_ddim" and kw["sampling_timesteps"] == 20 and kw["ddim_sampling_eta"] == 0.3
    assert set(kw) == {"condition", "condition_cross", "known", "mask", "sampling_timesteps", "ddim_sampling_eta"}
    assert torch.equal(kw["known"][0, :2], boxes[0, :2]) and bool(kw["known"][0, 2:].eq(0).all()) and bool(kw["known"][2].eq(0).all())
    assert (kw["mask"] != 0).any(-1).sum(1).tolist() == [2, N, 0] and bool(kw["mask"][1].all())
    # the CPU draw of sample() is kept: the CPU generator advances by one (B, N, C) draw
    torch.manual_seed(3)
    net.inpaint_scene_batched(room, N, C, boxes, mask)
    after = torch.randn(4)
    torch.manual_seed(3)
    torch.randn((B, N, C))
    assert torch.equal(after, torch.randn(4))


def test_inpaint_scene_batched_refusals(layout_net, golden_dir, tmp_path):
    net, N, C = layout_net
    B = 2
    room = torch.zeros(B, 1, 64, 64)
    boxes, mask = torch.zeros(B, N, C), torch.zeros(B, N, C, dtype=torch.bool)
    for bad_boxes, pat in ((torch.zeros(B, N + 1, C), "boxes"), (torch.zeros(B, N, C - 1), "boxes"), (torch.zeros(B + 1, N, C), "boxes"),
                           ([boxes[0]], "boxes"), ([boxes[0], torch.zeros(N + 1, C)], "scene 1"), ([boxes[0], torch.zeros(3, C - 1)], "scene 1"),
                           ([boxes[0], torch.zeros(C)], "scene 1")):
        with pytest.raises(ValueError, match=pat):
            net.inpaint_scene_batched(room, N, C, bad_boxes, mask, batch_size=B)
    for bad_mask in (torch.zeros(B, N, C), torch.zeros(B, N + 1, dtype=torch.bool), torch.zeros(B, N, C - 1, dtype=torch.bool), None):
        with pytest.raises(ValueError, match="known_mask"):
            net.inpaint_scene_batched(room, N, C, boxes, bad_mask)
    for S, eta in ((0, 0.0), (1001, 0.0), (50, 1.5), (True, 0.0)):
        with pytest.raises(ValueError):
            net.inpaint_scene_batched(room, N, C, boxes, mask, sampling_timesteps=S, ddim_sampling_eta=eta)
    assert net.diffusion.calls == []


@pytest.mark.parametrize("flag", ["room_partial_condition", "room_arrange_condition"])
def test_prefix_and_arrange_models_are_refused(flag, golden_dir, tmp_path):
    """Models constructed with room_partial_condition / room_arrange_condition: their condition tensors already encode a prefix / a
    sub-shape, the call names the flag."""
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = network_config({"room_partial_condition": "partial", "room_arrange_condition": "arrange"}[flag], str(stats))
    with contextlib.redirect_stdout(io.StringIO()):
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
    assert getattr(m, flag)
    m.diffusion = _Recorder()
    N, C = 12, 62
    with pytest.raises(ValueError, match=flag):
        m.inpaint_scene_batched(torch.zeros(1, 1, 64, 64), N, C, torch.zeros(1, N, C), torch.zeros(1, N, dtype=torch.bool))
    assert m.diffusion.calls == []


def test_masked_loops_check_their_arguments_on_the_cpu():
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    gd = GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, 50),
                           "mse", "v", "fixedsmall", False, False, None)
    shape = (2, 12, 62)
    ok_k, ok_m = torch.zeros(shape), torch.zeros(shape, dtype=torch.bool)
    for known, mask in ((None, ok_m), (ok_k, None), (torch.zeros(2, 11, 62), ok_m), (ok_k, torch.zeros(2, 11, dtype=torch.bool)),
                        (ok_k, torch.zeros(shape)), (ok_k, torch.zeros(2, 12, 61, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            gd.p_sample_loop_masked(None, shape, "cpu", None, None, known=known, mask=mask)
        with pytest.raises(ValueError):
            gd.ddim_masked_loop(None, shape, "cpu", None, None, sampling_timesteps=10, known=known, mask=mask)
    for S, eta in ((0, 0.0), (51, 0.0), (10, 1.5)):
        with pytest.raises(ValueError):
            gd.ddim_masked_loop(None, shape, "cpu", None, None, sampling_timesteps=S, ddim_sampling_eta=eta, known=ok_k, mask=ok_m)


# ------------------------------------------------------------------------------------------------------------------- the fixture
def _cpu_model(name, tmp_path):
    """(state dict of the denoiser, net kwargs, condition (B, N, .), condition_cross or None) of a golden case, on the CPU: the seeded
    wrapper parameters of oracle.make_golden_wrapper put through the restatement's pieces."""
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    CASES, case_texts, masked_inputs, _ = _tool()
    case = CASES[name][0]
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = network_config(case, str(stats), CASES[name][2])
    if case == "text":
        cfg["text_bert_cached"] = True
    with contextlib.redirect_stdout(io.StringIO()):
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
    wsd = wrapper_state_dict(m)
    sd = {k[len("diffusion.model."):]: v for k, v in wsd.items() if k.startswith("diffusion.model.")}
    B = len(CASES[name][6])
    cond = wsd["positional_embedding"][None].expand(B, -1, -1).contiguous()
    cross = None
    texts = case_texts(name)
    if texts is not None:
        cross = torch.nn.functional.linear(fake_bert_features(texts), wsd["fc_text_f.weight"], wsd["fc_text_f.bias"])
    return sd, cfg["net_kwargs"], cond, cross


def _restated_tstep(tb, denoise, T, clip, mt, known, mask, main, kn):
    x = main[0]
    for i, step in enumerate(reversed(range(T))):
        t = torch.full((known.shape[0],), step, dtype=torch.int64)
        x = torch.where(mask, R.q_sample(tb, known, t, kn[i]), x)
        x = R.p_sample_step(tb, x, t, denoise(x, t), main[i + 1], clip, mt)
    return torch.where(mask, known, x)


def _restated_ddim(tb, denoise, T, S, eta, mt, known, mask, main, kn):
    """ddim_sample_loop (reference :402-444) with model_predictions(clip_x_start=True) (:242-264), the select in front of the model call."""
    times = list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))
    ac = tb["alphas_cumprod"]
    x = main[0]
    k = 1
    for i, (time, time_next) in enumerate(zip(times[:-1], times[1:])):
        t = torch.full((known.shape[0],), time, dtype=torch.int64)
        x = torch.where(mask, R.q_sample(tb, known, t, kn[i]), x)
        out = denoise(x, t)
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
        x = x0 * alpha_next.sqrt() + c * pred_noise + sigma * main[k]
        k += 1
    return torch.where(mask, known, x)


@pytest.mark.parametrize("name", ["v.T1000", "eps.T50", "ddim.S20.eta0", "ddim.S7.eta0.3", "text.T50"])
def test_cpu_restatement_of_the_masked_loops_reproduces_the_fixture(name, golden_dir, tmp_path):
    CASES, case_texts, masked_inputs, scene_masks = _tool()
    g = np.load(os.path.join(golden_dir, "masked.npz"))
    case, mt, T, S, eta, clip, known, mask, main, kn = masked_inputs(name)
    sd, kw, cond, cross = _cpu_model(name, tmp_path)
    tb = R.schedule_tables(1e-4, 0.02, T, mt)
    torch.set_num_threads(min(8, os.cpu_count() or 1))

    def denoise(x, t):
        return R.unet1d_forward(sd, kw, x, t, cond, cross)

    with torch.no_grad():
        if S is None:
            y = _restated_tstep(tb, denoise, T, clip, mt, known, mask, main, kn)
        else:
            y = _restated_ddim(tb, denoise, T, S, eta, mt, known, mask, main, kn)
    want = torch.from_numpy(g[name])
    rel = float((y - want).abs().max() / want.abs().max())
    print("%s: restatement vs fixture, max-abs / max-abs %.3g" % (name, rel))
    assert torch.equal(y[mask], known[mask]) and torch.equal(want[mask], known[mask])         # given elements come back bit-equal
    assert rel < RTOL, (name, rel)


def test_fixture_lists_the_documented_scenes_and_cases(golden_dir):
    CASES, _, masked_inputs, scene_masks = _tool()
    g = np.load(os.path.join(golden_dir, "masked.npz"))
    m = scene_masks()
    assert tuple(m.shape) == (7, 12, 62)
    assert not m[0].any() and bool(m[5].all())
    assert m[1].all(-1).nonzero().flatten().tolist() == [0, 1, 2] and m[2].all(-1).nonzero().flatten().tolist() == [1, 5, 11]
    assert bool(m[3][:, 8:30].all()) and int(m[3].sum()) == 12 * 22
    assert int(m[4].sum()) == 12 * (3 + 22 + 32) and not m[4][:, 0:3].any() and not m[4][:, 6:8].any()
    assert int(m[6].sum()) == 4 * 3 + 6 * 22
    for name, (case, mt, T, S, eta, clip, scenes, seed) in CASES.items():
        assert tuple(g[name].shape) == (len(scenes), 12, 62) and np.isfinite(g[name]).all()
    assert os.path.getsize(os.path.join(golden_dir, "masked.npz")) < 256 * 1024
