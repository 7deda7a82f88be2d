"""Strided (DDIM) scene completion and re-arrangement on the host: the new C symbol, the plumbing of ``sampling_timesteps`` /
``ddim_sampling_eta`` through ``complete_scene_batched`` / ``arrange_scene_batched`` / ``complete_scene`` / ``arrange_scene``, the unchanged
call patterns without the keyword, the refusals, the argument checks of ``ddim_complete_ragged_loop`` and the replay protocol of its 2 S
draws.  No GPU needed: a recording stub stands in for DiffusionPoint, as in tests/test_complete_ragged_host.py."""
import copy
import json
import os
import re

import pytest
import torch

from oracle import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsc_ddim_inpaint_step_f32",)


def test_header_declares_and_library_exports_the_new_symbol():
    from diffuscene_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dsc_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, "%s not declared in include/diffuscene_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), "%s not exported / bound" % name
    assert callable(ops.ddim_inpaint_step)


class _Recorder(torch.nn.Module):
    """Stands in for DiffusionPoint under the wrapper: records which loop a call reaches and with what."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def _rec(self, kind, shape, kw):
        self.calls.append((kind, tuple(shape), kw))
        return torch.zeros(shape)

    def gen_samples(self, shape, device, **kw):
        return self._rec("gen_samples", shape, kw)

    def complete_samples(self, shape, device, **kw):
        return self._rec("complete_samples", shape, kw)

    def complete_samples_ragged(self, shape, device, **kw):
        return self._rec("complete_samples_ragged", shape, kw)

    def complete_samples_ragged_ddim(self, shape, device, **kw):
        return self._rec("complete_samples_ragged_ddim", shape, kw)

    def arrange_samples(self, shape, device, **kw):
        return self._rec("arrange_samples", shape, kw)

    def arrange_samples_ddim(self, shape, device, **kw):
        return self._rec("arrange_samples_ddim", shape, kw)


@pytest.fixture
def layout_net(golden_dir, tmp_path):
    """The shipped unconditional bedroom config (instance-conditioned, v) with a recorder under it."""
    import diffuscene_amd.networks as ours
    cfgs = json.load(open(os.path.join(golden_dir, "reference_configs.json")))
    config = copy.deepcopy(cfgs["uncond/diffusion_bedrooms_instancond_lat32_v.yaml"])
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    config["network"]["diffusion_kwargs"]["train_stats_file"] = str(stats)
    torch.manual_seed(0)
    net, _, _ = ours.build_network(None, 22, config, None, device="cpu")
    net.diffusion = _Recorder()
    net.delete_empty_per_scene = lambda samples, keep_empty=False: list(samples)     # its compaction is a device kernel
    net.eval()
    return net, config["network"]["sample_num_points"], config["network"]["point_dim"]


def _scenes(counts, C, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((p, C), generator=g) for p in counts]


STRIDED_KEYS = {"condition", "condition_cross", "partial_boxes", "num_partial", "sampling_timesteps", "ddim_sampling_eta"}


def test_complete_scene_batched_reaches_the_strided_loop_once(layout_net):
    net, N, C = layout_net
    mask = torch.zeros(4, 1, 64, 64)
    counts = [3, 0, N, 5]
    scenes = _scenes(counts, C)
    res = net.complete_scene_batched(mask, N, C, scenes, sampling_timesteps=20, ddim_sampling_eta=0.3)
    (kind, shape, kw), = net.diffusion.calls
    assert kind == "complete_samples_ragged_ddim" and shape == (4, N, C) and len(res) == 4
    assert set(kw) == STRIDED_KEYS
    assert kw["sampling_timesteps"] == 20 and kw["ddim_sampling_eta"] == 0.3 and list(kw["num_partial"]) == counts
    pb = kw["partial_boxes"]
    assert tuple(pb.shape) == (4, N, C) and pb.dtype == torch.float32              # normalised: padded to num_points with zeros
    for b, s in enumerate(scenes):
        assert torch.equal(pb[b, :counts[b]], s) and pb[b, counts[b]:].eq(0).all()
    assert kw["condition"] is not None and tuple(kw["condition"].shape[:2]) == (4, N)
    # the padded form, junk in its padding rows, normalises to the same call
    padded = torch.full((4, N, C), 123.0)
    for b, s in enumerate(scenes):
        padded[b, :counts[b]] = s
    net.complete_scene_batched(mask, N, C, padded, num_partial=torch.tensor(counts), batch_size=4, sampling_timesteps=20,
                               ddim_sampling_eta=0.3)
    assert [c[0] for c in net.diffusion.calls] == ["complete_samples_ragged_ddim"] * 2
    kw1 = net.diffusion.calls[1][2]
    assert torch.equal(kw1["partial_boxes"], pb) and list(kw1["num_partial"]) == counts and set(kw1) == STRIDED_KEYS
    assert kw1["sampling_timesteps"] == 20 and kw1["ddim_sampling_eta"] == 0.3


def test_the_other_entry_points_reach_their_strided_loops(layout_net):
    net, N, C = layout_net
    boxes = torch.randn(5, N, C)
    res = net.arrange_scene_batched(torch.zeros(5, 1, 64, 64), N, C, boxes, sampling_timesteps=10)
    (kind, shape, kw), = net.diffusion.calls
    assert kind == "arrange_samples_ddim" and shape == (5, N, C) and kw["input_boxes"] is boxes and len(res) == 5
    assert kw["sampling_timesteps"] == 10 and kw["ddim_sampling_eta"] == 0.0
    assert set(kw) == {"condition", "condition_cross", "input_boxes", "sampling_timesteps", "ddim_sampling_eta"}
    net.diffusion.calls.clear()
    mask = torch.zeros(1, 1, 64, 64)
    given = torch.randn(1, 3, C)
    out = net.complete_scene(mask, N, C, given, batch_size=1, sampling_timesteps=50, ddim_sampling_eta=1.0)
    (kind, shape, kw), = net.diffusion.calls
    assert kind == "complete_samples_ragged_ddim" and shape == (1, N, C) and list(kw["num_partial"]) == [3]          # uniform counts
    assert torch.equal(kw["partial_boxes"][:, :3], given) and kw["partial_boxes"][:, 3:].eq(0).all()
    assert kw["sampling_timesteps"] == 50 and kw["ddim_sampling_eta"] == 1.0
    assert set(out) >= {"class_labels", "translations", "sizes", "angles"}                                           # the batch-row-0 post-filter
    net.diffusion.calls.clear()
    out = net.arrange_scene(mask, N, C, boxes[:1], batch_size=1, sampling_timesteps=7, ddim_sampling_eta=0.5)
    (kind, shape, kw), = net.diffusion.calls
    assert kind == "arrange_samples_ddim" and shape == (1, N, C) and kw["sampling_timesteps"] == 7 and kw["ddim_sampling_eta"] == 0.5
    assert set(out) >= {"class_labels", "translations", "sizes", "angles"}


def test_without_the_keyword_all_four_record_todays_calls(layout_net):
    net, N, C = layout_net
    mask = torch.zeros(1, 1, 64, 64)
    given, full = torch.zeros(1, 3, C), torch.zeros(1, N, C)
    net.complete_scene_batched(mask, N, C, given, clip_denoised=True, sampling_timesteps=None)
    net.arrange_scene_batched(mask, N, C, full, sampling_timesteps=None, ddim_sampling_eta=0.7)       # eta alone switches nothing
    net.complete_scene(mask, N, C, given, batch_size=1, clip_denoised=True, sampling_timesteps=None)
    net.arrange_scene(mask, N, C, full, batch_size=1, sampling_timesteps=None)
    kinds = [c[0] for c in net.diffusion.calls]
    assert kinds == ["complete_samples_ragged", "arrange_samples", "complete_samples", "arrange_samples"]
    assert set(net.diffusion.calls[0][2]) == {"condition", "condition_cross", "clip_denoised", "partial_boxes", "num_partial"}
    assert set(net.diffusion.calls[1][2]) == {"condition", "condition_cross", "clip_denoised", "input_boxes"}
    assert set(net.diffusion.calls[2][2]) == {"condition", "condition_cross", "clip_denoised", "partial_boxes"}
    assert net.diffusion.calls[2][2]["partial_boxes"] is given
    assert set(net.diffusion.calls[3][2]) == {"condition", "condition_cross", "clip_denoised", "input_boxes"}


@pytest.mark.parametrize("S,eta", [(0, 0.0), (-3, 0.0), (1001, 0.0), (50.0, 0.0), (True, 0.0), (50, -0.1), (50, 1.01), (50, float("nan"))])
def test_bad_strided_arguments_are_refused_before_any_loop(layout_net, S, eta):
    net, N, C = layout_net
    mask = torch.zeros(1, 1, 64, 64)
    given, full = torch.zeros(1, 3, C), torch.zeros(1, N, C)
    kw = dict(sampling_timesteps=S, ddim_sampling_eta=eta)
    for call in (lambda: net.complete_scene_batched(mask, N, C, given, **kw), lambda: net.arrange_scene_batched(mask, N, C, full, **kw),
                 lambda: net.complete_scene(mask, N, C, given, batch_size=1, **kw),
                 lambda: net.arrange_scene(mask, N, C, full, batch_size=1, **kw)):
        with pytest.raises(ValueError):
            call()
    assert net.diffusion.calls == []


def test_sample_still_refuses_both_combinations_and_says_where_the_feature_lives(layout_net):
    net, N, C = layout_net
    mask = torch.zeros(1, 1, 64, 64)
    with pytest.raises(NotImplementedError, match="completion"):
        net.sample(mask, N, C, 1, partial_boxes=torch.zeros(1, 3, C), sampling_timesteps=50)
    with pytest.raises(NotImplementedError, match="re-arrangement"):
        net.sample(mask, N, C, 1, input_boxes=torch.zeros(1, N, C), sampling_timesteps=50)
    assert net.diffusion.calls == []
    assert "complete_scene_batched" in type(net).sample.__doc__


def test_strided_ragged_loop_checks_its_arguments_on_the_cpu():
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint, GaussianDiffusion, get_betas
    gd = GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, 50),
                           "mse", "v", "fixedsmall", False, False, None)
    shape = (2, 12, 62)
    for partial, counts in ((None, [1, 1]), (torch.zeros(2, 3, 62), None), (torch.zeros(2, 13, 62), [1, 1]), (torch.zeros(2, 0, 62), [0, 0]),
                            (torch.zeros(3, 3, 62), [1, 1]), (torch.zeros(2, 3, 61), [1, 1]), (torch.zeros(2, 3, 62), [1, 4]),
                            (torch.zeros(2, 3, 62), [-1, 2]), (torch.zeros(2, 3, 62), [1, 2, 3])):
        with pytest.raises(ValueError):
            gd.ddim_complete_ragged_loop(None, shape, "cpu", None, None, sampling_timesteps=10, partial_boxes=partial, num_partial=counts)
    for S, eta in ((0, 0.0), (51, 0.0), (10, 1.5)):
        with pytest.raises(ValueError):
            gd.ddim_complete_ragged_loop(None, shape, "cpu", None, None, sampling_timesteps=S, ddim_sampling_eta=eta,
                                         partial_boxes=torch.zeros(2, 3, 62), num_partial=[1, 1])
        with pytest.raises(ValueError):
            gd.ddim_arrange_loop(None, shape, "cpu", None, None, sampling_timesteps=S, ddim_sampling_eta=eta, input_boxes=torch.zeros(shape))
    assert callable(DiffusionPoint.complete_samples_ragged_ddim) and callable(DiffusionPoint.arrange_samples_ddim)


def test_ragged_replay_yields_the_two_s_draws_in_the_loop_order_at_pmax_equal_n():
    """x_T, then per pair a partial draw and a main draw; the last pair makes the partial draw only: 2 S draws, served by
    RaggedNoiseReplay from (S, B, N, C) and (S, B, Pmax, C) buffers, also when Pmax == N.  The loop itself exists.
    This pins the replay protocol only: the loop cannot run on the CPU (its tables and kernels live on a HIP device, no CPU fallback),
    so the order in which the loop itself draws is pinned on the device by
    tests/test_gpu_ddim_complete.py::test_the_eager_loop_makes_its_two_s_draws_in_the_documented_order."""
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion
    from diffuscene_amd.sampler import RaggedNoiseReplay, graph_ddim_complete_ragged_loop  # noqa: F401
    assert hasattr(GaussianDiffusion, "ddim_complete_ragged_loop")
    S, shape = 4, (2, 4, 5)
    main = torch.arange(S * 40, dtype=torch.float32).view(S, *shape)
    part = -torch.arange(S * 40, dtype=torch.float32).view(S, *shape) - 1
    r = RaggedNoiseReplay(main, part)
    got = [r(size=shape) for _ in range(2 * S)]
    assert torch.equal(got[0], main[0])
    for k in range(S):
        assert torch.equal(got[1 + 2 * k], part[k])
        if k < S - 1:
            assert torch.equal(got[2 + 2 * k], main[k + 1])
    assert r.i == S and r.ip == S
