"""Collision steering on the host -- no kernel is executed here.

* the in-test float64 oracle (tests/steer_oracle.py: torch autograd over diffuscene_amd.networks.loss.axis_aligned_bbox_overlaps_3d) has
  the pair matrix of the REFERENCE's axis_aligned_bbox_overlaps_3d (oracle.ref_loader), and its gradient is a finite difference of its
  energy;
* the generator of the device tests satisfies the margin condition for every size and seed they use, and every batch of two or more boxes
  holds an overlapping valid pair;
* ``collision_scale`` / ``collision_steps`` on every accepted form and every refusal, on ops, on the loops of GaussianDiffusion and on the
  wrapper; re-arrangement refuses the keyword; ``None`` is the call as it was;
* the step family is what it was: ops.STEP_ENTRY and the ten graph_*_loop front ends; the new symbol is declared in the header, exported
  and bound."""
import contextlib
import io
import json
import os
import re

import pytest
import torch

import steer_oracle as O
from oracle import weights as W
from oracle.make_golden_wrapper import network_config
from oracle.ref_loader import load_reference, reference_available
from test_cfg_host import _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, SEEDS = (1, 2, 5, 64, 65, 160), (0, 1, 2)
TAIL_SIZES = (5, 65)               # the sizes the device tests also run with a 32-d objfeat tail


# ------------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.skipif(not reference_available(), reason="the reference tree is only present in the build container")
def test_oracle_pair_matrix_is_the_reference_overlap():
    ref_loss = load_reference()[0]
    for n, seed in ((5, 0), (65, 1)):
        x = O.make_scenes(n, seed).double().clamp(-1, 1)
        box = O.boxes(x)
        _, _, iou, _ = O.energy_grad(x)
        assert torch.equal(iou, ref_loss.axis_aligned_bbox_overlaps_3d(box, box))
        assert torch.equal(iou, iou.transpose(-1, -2)) and float(iou.max()) <= 1.0


def test_oracle_gradient_is_the_slope_of_its_energy():
    x = O.make_scenes(5, 0).double()
    E, g, _, pairs = O.energy_grad(x)
    assert int(pairs.sum()) > 0 and float(g.abs().max()) > 0
    h = 1e-6
    for b, i, k in ((0, 0, 0), (0, 3, 2), (2, 1, 1), (2, 4, 0)):
        xp, xm = x.clone(), x.clone()
        xp[b, i, k] += h
        xm[b, i, k] -= h
        slope = (O.energy_grad(xp)[0][b] - O.energy_grad(xm)[0][b]) / (2 * h)
        assert abs(float(slope - g[b, i, k])) <= 1e-6 * max(1.0, abs(float(g[b, i, k]))), (b, i, k, float(slope), float(g[b, i, k]))
    # sizes, angle and logits carry no gradient; an invalid box neither feels nor exerts a force
    x = O.make_scenes(64, 0).double()
    invalid = x[..., O.EMPTY] >= 0
    assert bool(invalid.any()) and float(O.energy_grad(x)[1][invalid].abs().max()) == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_generator_meets_the_margin_condition(n):
    for seed in SEEDS:
        for c in (O.C12,) + ((O.C12 + 32,) if n in TAIL_SIZES else ()):
            x = O.make_scenes(n, seed, c=c)
            assert x.shape == (3, n, c) and float(x[..., O.EMPTY].abs().min()) >= 0.05
            O.assert_margins(x, (n, seed, c))           # and, for n >= 2, an overlapping valid pair in the batch
    if n > 16:
        assert float(O.make_scenes(n, 0)[..., 0:3].abs().max()) > 1.0                   # some translations beyond the clamp


# ------------------------------------------------------------------------------------------------------------------- the scales
def test_collision_scales_and_steps_normalise_and_refuse():
    from diffuscene_amd import ops
    for scale, want in ((0.02, [0.02] * 3), (0, [0.0] * 3), ([0, 0.5, 3], [0.0, 0.5, 3.0]), (torch.tensor([0.0, 0.5, 3.0]), [0.0, 0.5, 3.0])):
        out = ops.collision_scales(scale, 3, "cpu")
        assert out.dtype == torch.float32 and out.is_contiguous() and out.tolist() == torch.tensor(want, dtype=torch.float32).tolist()
    for bad in (float("nan"), float("inf"), -0.5, [0.1, -1e-9, 0.2], [0.1, 0.2], None, "1", True, [0.1, float("nan"), 0.2]):
        with pytest.raises(ValueError, match="collision_scale"):
            ops.collision_scales(bad, 3, "cpu")
    assert ops.collision_steps(None, 1000) == 1000 and ops.collision_steps(0, 1000) == 0 and ops.collision_steps(1000, 1000) == 1000
    for bad in (-1, 1001, 2.5, True, "3"):
        with pytest.raises(ValueError, match="collision_steps"):
            ops.collision_steps(bad, 1000)
    with pytest.raises(ValueError, match="bounds"):
        ops.steer_bounds([0.0] * 11)
    with pytest.raises(ValueError, match="bounds"):
        ops.steer_bounds([0.0] * 11 + [float("inf")])
    assert list(ops.steer_bounds(O.BOUNDS)) == torch.tensor(O.BOUNDS, dtype=torch.float32).tolist()


def _gd(stats=None, **cfg):
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    base = dict(objectness_dim=0, class_dim=4, angle_dim=2, objfeat_dim=0)
    base.update(cfg)
    return GaussianDiffusion(base, get_betas("linear", 1e-4, 0.02, 50), "mse", "eps", "fixedsmall", False, False, stats)


def test_the_loops_refuse_before_anything_is_drawn(tmp_path):
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))

    def never(*a, **k):
        raise AssertionError("a refused call drew noise")
    shape = (2, 5, 12)
    gd = _gd(str(stats))
    weight, k, bounds, bbox_dim, class_dim = gd._steer_inputs(shape, "cpu", [0.0, 0.5], 7, "loop")
    assert weight.tolist() == [0.0, 0.5] and (k, bbox_dim, class_dim) == (7, 8, 4)
    assert list(bounds) == torch.tensor(W.DATASET_STATS["bounds_translations"] + W.DATASET_STATS["bounds_sizes"]).tolist()
    assert gd._steer_inputs(shape, "cpu", 1.0, None, "loop")[1] == 50
    for loop, kw in ((gd.p_sample_loop, {}), (gd.ddim_sample_loop, {}), (gd.p_sample_loop_masked, dict(known=torch.zeros(shape), mask=torch.zeros(shape) > 0))):
        with pytest.raises(ValueError, match="collision_scale"):
            loop(None, shape, "cpu", None, None, noise_fn=never, collision_scale=-1.0, **kw)
        with pytest.raises(ValueError, match="collision_steps"):
            loop(None, shape, "cpu", None, None, noise_fn=never, collision_scale=1.0, collision_steps=51, **kw)
        with pytest.raises(ValueError, match="collision_scale"):                     # steps without a scale
            loop(None, shape, "cpu", None, None, noise_fn=never, collision_steps=3, **kw)
        with pytest.raises(ValueError, match="at most 160"):
            loop(None, (2, 161, 12), "cpu", None, None, noise_fn=never, collision_scale=1.0,
                 **{k_: torch.zeros((2, 161, 12)) > 0 if k_ == "mask" else torch.zeros((2, 161, 12)) for k_ in kw})
    with pytest.raises(ValueError, match="train_stats_file"):                        # no statistics file: the key is named
        _gd(None).p_sample_loop(None, shape, "cpu", None, None, noise_fn=never, collision_scale=1.0)
    with pytest.raises(ValueError, match="angle_dim = 2"):
        _gd(str(stats), angle_dim=1).p_sample_loop(None, (2, 5, 11), "cpu", None, None, noise_fn=never, collision_scale=1.0)
    with pytest.raises(ValueError, match="full object layout"):                      # a re-arrangement sub-shape
        gd.p_sample_loop(None, (2, 5, 5), "cpu", None, None, noise_fn=never, collision_scale=1.0)
    for name in ("p_sample_loop_arrange", "ddim_arrange_loop"):                      # the arrange loops do not take the keyword at all
        with pytest.raises(TypeError):
            getattr(gd, name)(None, shape, "cpu", None, None, collision_scale=1.0)


# ------------------------------------------------------------------------------------------------------------------- the wrapper
class _AllLoops(_Recorder):
    def __getattr__(self, name):
        if name.startswith(("gen_samples", "complete_samples", "inpaint_samples", "arrange_samples")):
            return lambda shape, device, **kw: self._rec(name, shape, kw)
        return super().__getattr__(name)


def _wrapper(case, tmp_path):
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = network_config(case, str(stats))
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
    rec = _AllLoops()
    rec.diffusion = m.diffusion.diffusion              # the checks of the keyword live on the GaussianDiffusion
    m.diffusion = rec
    m.delete_empty_per_scene = lambda samples, keep_empty=False: list(samples)
    m.delete_empty_from_network_samples = lambda samples, device="cpu", keep_empty=False: samples
    return m.eval()


def test_the_wrapper_hands_the_keywords_on_and_none_is_the_old_call(tmp_path):
    N, C = 12, 62
    m = _wrapper("uncond", tmp_path)
    room = torch.zeros(3, 1, 64, 64)
    steer = dict(collision_scale=[0.0, 0.02, 0.1], collision_steps=20)
    known = torch.zeros(3, N, C)
    with contextlib.redirect_stdout(io.StringIO()):
        m.generate_layout_batched(room, N, C, 3)
        m.generate_layout_batched(room, N, C, 3, **steer)
        m.generate_layout_batched(room, N, C, 3, sampling_timesteps=50, scene_seeds=[1, 2, 3], **steer)
        m.generate_layout(room, N, C, 3, collision_scale=0.02)
        m.complete_scene_batched(room, N, C, [known[0, :2], known[1, :0], known[2, :5]], **steer)
        m.complete_scene_batched(room, N, C, known[:, :4], sampling_timesteps=10, **steer)
        m.complete_scene(room, N, C, known[:, :4], 3, **steer)
        m.inpaint_scene_batched(room, N, C, known, torch.zeros(3, N, dtype=torch.bool), **steer)
        m.inpaint_scene_batched(room, N, C, known, torch.zeros(3, N, dtype=torch.bool))
    calls = m.diffusion.calls
    names = [c[0] for c in calls]
    assert names == ["gen_samples", "gen_samples", "gen_samples_ddim", "gen_samples", "complete_samples_ragged", "complete_samples_ragged_ddim",
                     "complete_samples", "inpaint_samples", "inpaint_samples"]
    for i in (0, 8):                                                                 # None: not a keyword more than before
        assert "collision_scale" not in calls[i][2] and "collision_steps" not in calls[i][2]
    for i in (1, 2, 4, 5, 6, 7):
        assert calls[i][2]["collision_scale"] == steer["collision_scale"] and calls[i][2]["collision_steps"] == 20
    assert calls[3][2]["collision_scale"] == 0.02 and calls[3][2]["collision_steps"] is None
    assert "noise_fn" in calls[2][2] and calls[2][2]["sampling_timesteps"] == 50     # combines with seeds and the strided loop
    before = len(calls)
    cpu_rng = torch.get_rng_state()
    for bad in (dict(collision_scale=-1.0), dict(collision_scale=[0.1, 0.2]), dict(collision_scale=0.1, collision_steps=-1),
                dict(collision_steps=5), dict(collision_scale=float("nan"))):
        for fn, args in ((m.generate_layout_batched, (room, N, C, 3)), (m.sample, (room, N, C, 3)),
                         (m.complete_scene_batched, (room, N, C, known[:, :4])),
                         (m.inpaint_scene_batched, (room, N, C, known, torch.zeros(3, N, dtype=torch.bool)))):
            with pytest.raises(ValueError, match="collision_s"):
                fn(*args, **bad)
    with pytest.raises(ValueError, match="ret_traj"):
        m.sample(room, N, C, 3, ret_traj=True, collision_scale=0.1)
    with pytest.raises(ValueError, match="at most 160"):
        m.generate_layout_batched(room, 161, C, 3, collision_scale=0.1)
    assert len(calls) == before and torch.equal(torch.get_rng_state(), cpu_rng)      # refused before anything is drawn


def test_rearrangement_refuses_the_keyword(tmp_path):
    m = _wrapper("arrange", tmp_path)
    N, C = 12, 62
    room, boxes = torch.zeros(2, 1, 64, 64), torch.zeros(2, N, C)
    for fn, args in ((m.arrange_scene, (room, N, C, boxes, 2)), (m.arrange_scene_batched, (room, N, C, boxes))):
        for kw in (dict(collision_scale=0.1), dict(collision_steps=3), dict(collision_scale=0.1, sampling_timesteps=5)):
            with pytest.raises(ValueError, match="re-arrangement"):
                fn(*args, **kw)
    with pytest.raises(ValueError, match="re-arrangement"):
        m.sample(room, N, C, 2, input_boxes=boxes, collision_scale=0.1)
    assert m.diffusion.calls == []
    assert m._check_steer(None, None, (2, N, C), boxes) == {}                        # without the keyword: the call as it was


# ------------------------------------------------------------------------------------------------------------------- the tables
def test_the_step_family_and_the_front_ends_are_what_they_were():
    from diffuscene_amd import ops, sampler
    from test_step_args_host import ENTRY_POINTS
    from test_step_table_host import FRONT_ENDS
    names = [name for name, _ in ops.STEP_ENTRY.values()]
    assert len(names) == 10 and set(names) == {n for n in ENTRY_POINTS if "overwrite" not in n}
    assert "dsc_steer_boxes_f32" not in names
    fronts = {n for n in vars(sampler) if n.startswith("graph_") and n.endswith("_loop")}
    assert fronts == set(FRONT_ENDS.values()) and len(fronts) == 10
    x = torch.zeros(2, 3, 12)
    for front in sorted(fronts):                                                     # each takes steer=; None reaches the loop as before
        with pytest.raises(RuntimeError, match="graph sampling needs"):
            getattr(sampler, front)(None, None, (2, 3, 12), "cpu", None, None, *([x[:, 0, 0]] if "guided" in front else []),
                                    *((5, 0.0) if "ddim" in front else (True, 5)), steer=None)


def test_the_new_symbol_is_declared_exported_and_bound():
    import ctypes
    from diffuscene_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    m = re.search(r"^int dsc_steer_boxes_f32\((.*?)\);", hdr, flags=re.M | re.S)
    assert m, "dsc_steer_boxes_f32 is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["dsc_steer_boxes_f32"]
    assert hasattr(_lib.load(), "dsc_steer_boxes_f32") and restype is ctypes.c_int and len(argtypes) == len(params)
    for p, ty in zip(params, argtypes):
        assert (ty is ctypes.c_int32) == p.startswith("int32_t"), p
    for name in ("weight", "t_below", "bounds", "energy_out", "grad_out", "cfg_scale", "bbox_dim", "class_dim"):
        assert any(p.endswith(name) for p in params), name


def test_steer_rec_checks_its_operands_on_the_host():
    from diffuscene_amd import ops
    x = torch.zeros(2, 3, 12)
    steer = (x, x, O.BOUNDS, 8, 4)
    with pytest.raises(ValueError, match="one time source"):
        ops.steer_rec(x, x, 0, (x, x), steer)
    with pytest.raises(ValueError, match="one given part"):
        ops.steer_rec(x, x, 0, (x, x), steer, t=x, rows=(x, x, x), mask=(x, x, x))
    with pytest.raises(RuntimeError, match="HIP device"):                            # no CPU path
        ops.steer_rec(x, x, 0, (x, x), steer, t=x)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.box_repulsion(x, O.BOUNDS, class_dim=4)
