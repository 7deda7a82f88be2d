"""Batched completion / re-arrangement with per-scene counts, on the host: the two new C symbols, the input normalisation of
``complete_scene_batched`` (list form, padded form, zero padding to ``num_points``, the refusals), the plumbing of ``arrange_scene_batched``,
the count checks of the kernel wrappers, the replay protocol at Pmax == N, and the unchanged call patterns of the existing entry points.
No GPU needed: a recording stub stands in for DiffusionPoint, as in tests/test_ddim_host.py."""
import copy
import json
import os
import re

import pytest
import torch

from oracle import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsc_complete_overwrite_ragged_f32", "dsc_p_sample_inpaint_f32")


def test_header_declares_and_library_exports_the_new_symbols():
    from diffuscene_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dsc_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, "%s not declared in include/diffuscene_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), "%s not exported / bound" % name


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

    def arrange_samples(self, shape, device, **kw):
        return self._rec("arrange_samples", shape, kw)


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


def test_list_form_and_padded_form_normalise_identically(layout_net):
    net, N, C = layout_net
    mask = torch.zeros(4, 1, 64, 64)
    counts = [3, 0, N, 5]
    scenes = _scenes(counts, C)
    res = net.complete_scene_batched(mask, N, C, scenes, clip_denoised=True)
    pmax = 7                                                      # a padded tensor narrower than num_points, junk in its padding rows
    padded = torch.full((4, N, C), 123.0)
    for b, s in enumerate(scenes):
        padded[b, :counts[b]] = s
    net.complete_scene_batched(mask, N, C, padded, num_partial=torch.tensor(counts), batch_size=4, clip_denoised=True)
    narrow = [min(p, pmax) for p in counts]
    net.complete_scene_batched(mask, N, C, padded[:, :pmax].contiguous(), num_partial=narrow)
    (k0, s0, kw0), (k1, s1, kw1), (k2, s2, kw2) = net.diffusion.calls
    assert k0 == k1 == k2 == "complete_samples_ragged" and s0 == s1 == s2 == (4, N, C)
    assert len(res) == 4
    assert torch.equal(kw0["partial_boxes"], kw1["partial_boxes"]) and list(kw0["num_partial"]) == list(kw1["num_partial"]) == counts
    assert list(kw2["num_partial"]) == narrow
    for kw, cnt in ((kw0, counts), (kw2, narrow)):
        pb = kw["partial_boxes"]
        assert tuple(pb.shape) == (4, N, C) and pb.dtype == torch.float32      # padded to num_points ...
        for b, s in enumerate(scenes):
            assert torch.equal(pb[b, :cnt[b]], s[:cnt[b]])
            assert pb[b, cnt[b]:].eq(0).all()                                      # ... with zeros, whatever the caller's padding held
    assert kw0["clip_denoised"] is True and kw2["clip_denoised"] is False
    assert kw0["condition"] is not None and tuple(kw0["condition"].shape[:2]) == (4, N)


def test_padded_form_without_counts_means_uniform(layout_net):
    net, N, C = layout_net
    given = torch.stack(_scenes([4, 4, 4], C))
    net.complete_scene_batched(torch.zeros(3, 1, 64, 64), N, C, given)
    (kind, shape, kw), = net.diffusion.calls
    assert kind == "complete_samples_ragged" and shape == (3, N, C) and list(kw["num_partial"]) == [4, 4, 4]
    assert torch.equal(kw["partial_boxes"][:, :4], given) and kw["partial_boxes"][:, 4:].eq(0).all()


@pytest.mark.parametrize("bad,match", [
    (dict(partial=lambda N, C: _scenes([2, N + 1], C)), "scene 1"),                                     # more objects than num_points
    (dict(partial=lambda N, C: [torch.zeros(2, C), torch.zeros(2, C - 1)]), "scene 1"),                 # wrong channel count
    (dict(partial=lambda N, C: _scenes([2, 2, 2], C)), "3 scenes for a batch of 2"),                    # list length != batch
    (dict(partial=lambda N, C: torch.zeros(2, 5, C), num_partial=[5, 6]), "scene 1"),                   # count > Pmax
    (dict(partial=lambda N, C: torch.zeros(2, 5, C), num_partial=[-1, 2]), "scene 0"),                  # count < 0
    (dict(partial=lambda N, C: torch.zeros(2, 5, C), num_partial=[1, 2, 3]), "3 entries for a batch of 2"),
    (dict(partial=lambda N, C: torch.zeros(2, N + 2, C)), "scene 0"),                                   # uniform, beyond num_points
    (dict(partial=lambda N, C: torch.zeros(2, 5, C + 1), num_partial=[0, 2]), "scene 0"),               # wrong channel count, padded form
])
def test_bad_input_raises_value_error_naming_the_scene(layout_net, bad, match):
    net, N, C = layout_net
    with pytest.raises(ValueError, match=match):
        net.complete_scene_batched(torch.zeros(2, 1, 64, 64), N, C, bad["partial"](N, C), num_partial=bad.get("num_partial"),
                                   batch_size=2)
    assert net.diffusion.calls == []


def test_arrange_scene_batched_calls_arrange_samples_once_with_the_batch(layout_net):
    net, N, C = layout_net
    boxes = torch.randn(5, N, C)
    res = net.arrange_scene_batched(torch.zeros(5, 1, 64, 64), N, C, boxes, clip_denoised=True)
    (kind, shape, kw), = net.diffusion.calls
    assert kind == "arrange_samples" and shape == (5, N, C) and kw["input_boxes"] is boxes and kw["clip_denoised"] is True
    assert len(res) == 5
    net.diffusion.calls.clear()
    with pytest.raises(ValueError, match="5 scenes for a batch of 4"):
        net.arrange_scene_batched(torch.zeros(4, 1, 64, 64), N, C, boxes, batch_size=4)
    with pytest.raises(ValueError, match="every scene must be"):
        net.arrange_scene_batched(torch.zeros(5, 1, 64, 64), N, C, boxes[:, :N - 1])
    assert net.diffusion.calls == []


def test_existing_entry_points_record_the_same_calls_as_before(layout_net):
    net, N, C = layout_net
    mask = torch.zeros(1, 1, 64, 64)
    given, full = torch.zeros(1, 3, C), torch.zeros(1, N, C)
    net.sample(mask, N, C, 1, partial_boxes=given)
    net.complete_scene(mask, N, C, given, batch_size=1, clip_denoised=True)
    net.arrange_scene(mask, N, C, full, batch_size=1)
    net.generate_layout(mask, N, C)
    kinds = [c[0] for c in net.diffusion.calls]
    assert kinds == ["complete_samples", "complete_samples", "arrange_samples", "gen_samples"]
    for kind, shape, kw in net.diffusion.calls[:2]:
        assert shape == (1, N, C) and set(kw) == {"condition", "condition_cross", "clip_denoised", "partial_boxes"}
        assert kw["partial_boxes"] is given and "num_partial" not in kw
    assert set(net.diffusion.calls[2][2]) == {"condition", "condition_cross", "clip_denoised", "input_boxes"}
    with pytest.raises(NotImplementedError, match="completion"):
        net.sample(mask, N, C, 1, partial_boxes=given, sampling_timesteps=50)


@pytest.mark.parametrize("counts", [[0, 13], [-1, 2], [1.5, 2], [True, 2], [1, 2, 3], torch.tensor([0.0, 1.0]), torch.tensor([[1, 2]])])
def test_host_counts_are_checked_before_upload(counts):
    """The kernel wrappers reject host-side counts outside [0, Pmax] before anything touches a device."""
    from diffuscene_amd import ops
    with pytest.raises(ValueError):
        ops.ragged_counts(counts, 2, 12, "cpu")
    ok = ops.ragged_counts([0, 12], 2, 12, "cpu")
    assert ok.dtype == torch.int64 and ok.tolist() == [0, 12]
    assert ops.ragged_counts(torch.tensor([3, 4], dtype=torch.int32), 2, 12, "cpu").tolist() == [3, 4]


def test_ragged_loop_refuses_missing_or_misshapen_partial():
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    gd = GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, 50),
                           "mse", "v", "fixedsmall", False, False, None)
    shape = (2, 12, 62)
    for partial, counts in ((None, [1, 1]), (torch.zeros(2, 3, 62), None), (torch.zeros(2, 13, 62), [1, 1]), (torch.zeros(2, 0, 62), [0, 0]),
                            (torch.zeros(3, 3, 62), [1, 1]), (torch.zeros(2, 3, 61), [1, 1]), (torch.zeros(2, 3, 62), [1, 4])):
        with pytest.raises(ValueError):
            gd.p_sample_loop_complete_ragged(None, shape, "cpu", None, None, partial_boxes=partial, num_partial=counts)


def test_ragged_replay_follows_the_protocol_when_pmax_equals_n():
    """NoiseReplay tells the two draws apart by shape, which cannot work at Pmax == N; RaggedNoiseReplay goes by call order.  NoiseReplay
    itself is unchanged for its callers."""
    from diffuscene_amd.sampler import NoiseReplay, RaggedNoiseReplay
    T, shape = 3, (2, 4, 5)
    main = torch.arange((T + 1) * 40, dtype=torch.float32).view(T + 1, *shape)
    part = -torch.arange(T * 40, dtype=torch.float32).view(T, *shape) - 1
    r = RaggedNoiseReplay(main, part)
    assert isinstance(r, NoiseReplay)
    got = [r(size=shape) for _ in range(2 * T + 1)]
    assert torch.equal(got[0], main[0])
    for i in range(T):
        assert torch.equal(got[1 + 2 * i], part[i]) and torch.equal(got[2 + 2 * i], main[i + 1])
    old = NoiseReplay(main, part[:, :, :2].contiguous())
    assert torch.equal(old(size=shape), main[0]) and torch.equal(old(size=(2, 2, 5)), part[0, :, :2]) and torch.equal(old(size=shape), main[1])
    same = NoiseReplay(main, part)                       # equal shapes: every draw comes from the main buffer, as before
    assert torch.equal(same(size=shape), main[0]) and torch.equal(same(size=shape), main[1])
