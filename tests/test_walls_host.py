"""Floor-plan steering on the host -- no kernel is executed here.

* the in-test float64 oracle (tests/wall_oracle.py) is sane: a full mask gives energy 0 and a zero gradient, a point exactly on a
  pixel-centre line takes the cell to its right (above) and that cell's slope, and the gradient is a finite difference of the energy;
* the generator of the device tests satisfies the margin condition for every size, seed and room they use, every batch holds a valid
  box with a point outside its room, and the 2 m room has points outside the image;
* ``wall_scale`` / ``wall_steps`` / ``room_side`` and the room mask on every refusal, on ops, on the loops of GaussianDiffusion and on
  the wrapper, before anything is drawn; re-arrangement refuses the keywords; ``None`` is the call as it was;
* the launch sits after the collision launch and before the multistep one, in the eager model call and in the captured step, and
  without the keyword no such launch is issued;
* the two new symbols are declared in the header, exported and bound."""
import contextlib
import io
import json
import os
import re
from types import SimpleNamespace

import pytest
import torch

import wall_oracle as O
from oracle import weights as W
from test_steer_host import _gd, _wrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, SEEDS = (1, 5, 64, 65, 160), (0, 1)


# ------------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_field_is_the_distance_to_the_nearest_inside_pixel():
    side = 3.1
    m = O.room("pixel", 8, 12, side)
    (i0, j0), = m.nonzero().tolist()
    s = float(torch.tensor(side, dtype=torch.float32))
    dx, dz = 2 * s / 12, 2 * s / 8
    f = O.field(m, side)
    assert f.dtype == torch.float32 and float(f[i0, j0]) == 0.0
    for i, j in ((0, 0), (7, 11), (i0, 0), (3, j0)):
        assert float(f[i, j]) == float(torch.tensor(0.5 * (((i - i0) * dz) ** 2 + ((j - j0) * dx) ** 2), dtype=torch.float32))
    assert float(O.field(O.room("none", 8, 12, side), side).abs().max()) == 0.0         # no inside pixel: F == 0
    assert float(O.field(O.room("full", 8, 12, side), side).abs().max()) == 0.0


def test_oracle_full_mask_gives_zero_energy_and_gradient():
    x = O.make_scenes(5, 0, spread=0.25)                                            # centres within +-0.75 m: every point inside the image
    assert O.outside_image(x, 16, 16, 3.1) == 0
    for kind in ("full", "none"):                                                   # no inside pixel: F == 0 as well
        E, g, out = O.energy_grad(x, O.room(kind, 16, 16, 3.1)[None, None], 3.1)
        assert float(E.abs().max()) == 0.0 and float(g.abs().max()) == 0.0 and int(out.sum()) == 0
    x = O.make_scenes(5, 0)                                                         # the continuation: outside the 2 m image even a full mask pulls
    assert O.outside_image(x, 16, 16, 2.0) > 0
    E, g, out = O.energy_grad(x, O.room("full", 16, 16, 2.0)[None, None], 2.0)
    assert float(E.min()) > 0 and int(out.sum()) > 0


def test_oracle_takes_the_cell_to_the_right_of_an_exact_pixel_line():
    """One box of zero size (nine coincident points) exactly on the centre line of column 5, row 2.5: the energy is the field's value
    there and the x gradient the slope of the cell [5, 6], not a mean with the cell [4, 5]."""
    h = w = 8
    side = 4.0                                                                      # dx = dz = 1: pixel centres at -3.5 + j
    bounds = (-4.0, 0.0, -4.0, 4.0, 1.0, 4.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0)         # centre = 4 x0, half size = (x0 + 1) / 2
    m = torch.zeros(h, w)
    m[:, :4] = 1.0                                                                  # inside: columns 0 .. 3; F[i, j] = (j - 3)^2 / 2 right of them
    f = O.field(m, side)
    assert f[2].tolist() == [0.0, 0.0, 0.0, 0.0, 0.5, 2.0, 4.5, 8.0]
    x = torch.zeros(1, 1, O.C12, dtype=torch.float64)
    x[..., 3:6], x[..., 6], x[..., O.EMPTY] = -1.0, 1.0, -1.0
    x[0, 0, 0], x[0, 0, 2] = 1.5 / 4, -1.0 / 4                                      # x = 1.5 -> u = 5 exactly; z = -1 -> v = 2.5
    E, g, out = O.energy_grad(x, m[None, None], side, bounds)
    assert float(E) == 2.0 and int(out) == 1
    assert float(g[0, 0, 0]) == (4.5 - 2.0) * 4.0 and float(g[0, 0, 2]) == 0.0      # the slope of the cell to the right, times span / 2
    x[0, 0, 0] = 1.0                                                                # x = 4, half a pixel beyond the last centre: the continuation
    E, g, _ = O.energy_grad(x, m[None, None], side, bounds)
    assert float(E) == 8.0 + 0.5 * 0.5 ** 2 and float(g[0, 0, 0]) == 0.5 * 4.0


def test_oracle_gradient_is_the_slope_of_its_energy():
    x, m = O.make_scenes(5, 0).double(), O.rooms(16, 16, 3.1)
    E, g, out = O.energy_grad(x, m, 3.1)
    assert int(out.sum()) > 0 and float(g.abs().max()) > 0 and float(g[..., 1].abs().max()) == 0.0
    O.assert_margins(x, m, 3.1, "finite differences")
    h = 1e-7                                                                        # far below the 1e-6 px margin: no cell changes
    for b, i, k in ((0, 0, 0), (0, 3, 2), (1, 1, 0), (2, 4, 2), (2, 2, 1)):
        xp, xm = x.clone(), x.clone()
        xp[b, i, k] += h
        xm[b, i, k] -= h
        slope = (O.energy_grad(xp, m, 3.1)[0][b] - O.energy_grad(xm, m, 3.1)[0][b]) / (2 * h)
        assert abs(float(slope - g[b, i, k])) <= 1e-6 * max(1.0, abs(float(g[b, i, k]))), (b, i, k, float(slope), float(g[b, i, k]))
    x = O.make_scenes(64, 0).double()                                               # an empty box feels no force
    invalid = x[..., O.EMPTY] >= 0
    assert bool(invalid.any()) and float(O.energy_grad(x, O.rooms(16, 16, 3.1), 3.1)[1][invalid].abs().max()) == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_generator_meets_the_margin_condition(n):
    for seed in SEEDS:
        for h, w, side in O.ROOMS:
            x, m, E, g, out = O.case(n, seed, h, w, side)                           # asserts the margins and a box outside its room
            assert x.shape == (3, n, O.C12) and m.shape == (3, 1, h, w) and int(out.sum()) >= 1
            if side == 2.0:
                assert O.outside_image(x, h, w, side) > 0
    x = O.make_scenes(n, 0)
    E0 = O.energy_grad(x, O.rooms(16, 16, 3.1), 3.1)[0]                              # the oracle's own step lowers the energy (the effect test)
    E1 = O.energy_grad(O.step(x, O.rooms(16, 16, 3.1), 3.1, [0.05] * 3), O.rooms(16, 16, 3.1), 3.1)[0]
    assert bool((E1 <= E0).all()) and bool((E1 < E0).any())


# ------------------------------------------------------------------------------------------------------------------- the keywords
def test_wall_scales_steps_side_and_mask_normalise_and_refuse():
    from diffuscene_amd import ops
    assert ops.wall_scales([0, 0.5, 3], 3, "cpu").tolist() == [0.0, 0.5, 3.0] and ops.wall_scales(0.05, 2, "cpu").dtype == torch.float32
    for bad in (float("nan"), float("inf"), -0.5, [0.1, -1e-9, 0.2], [0.1, 0.2], None, "1", True):
        with pytest.raises(ValueError, match="wall_scale") as e:
            ops.wall_scales(bad, 3, "cpu")
        assert "collision" not in str(e.value)
    assert ops.wall_steps(None, 1000) == 1000 and ops.wall_steps(0, 1000) == 0
    for bad in (-1, 1001, 2.5, True, "3"):
        with pytest.raises(ValueError, match="wall_steps"):
            ops.wall_steps(bad, 1000)
    assert ops.room_side_value(3.1) == 3.1 and ops.room_side_value(2) == 2.0
    for bad in (0, -1.0, float("inf"), float("nan"), None, "3", True):
        with pytest.raises(ValueError, match="room_side"):
            ops.room_side_value(bad)
    assert ops.room_mask_dims(torch.zeros(3, 1, 8, 12), 3) == (3, 8, 12) and ops.room_mask_dims(torch.zeros(1, 1, 2, 256, dtype=torch.uint8), 3) == (1, 2, 256)
    for bad in (None, torch.zeros(3, 8, 12), torch.zeros(3, 2, 8, 12), torch.zeros(2, 1, 8, 12), torch.zeros(3, 1, 1, 12), torch.zeros(3, 1, 8, 257),
                torch.zeros(3, 1, 8, 12, dtype=torch.int64)):
        with pytest.raises(ValueError, match="room_mask"):
            ops.room_mask_dims(bad, 3)
    x = torch.zeros(2, 3, 12)
    with pytest.raises(RuntimeError, match="HIP device"):                            # no CPU path
        ops.floor_field(torch.zeros(2, 1, 8, 12), 3.1)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.floor_violation(x, torch.zeros(2, 1, 8, 12), 3.1, O.BOUNDS, class_dim=4)
    with pytest.raises(ValueError, match="one time source"):
        ops.walls_rec(x, x, 0, (x, x), (x, x, O.BOUNDS, 8, 4, x, x))


def test_the_loops_refuse_before_anything_is_drawn(tmp_path):
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))

    def never(*a, **k):
        raise AssertionError("a refused call drew noise")
    shape = (2, 5, 12)
    room = torch.zeros(2, 1, 8, 12)
    gd = _gd(str(stats))
    weight, k, bounds, bbox_dim, class_dim, field, side = gd._wall_inputs(shape, "cpu", [0.0, 0.5], 7, 3.1, room, "loop", field=False)
    assert weight.tolist() == [0.0, 0.5] and (k, bbox_dim, class_dim, field, side) == (7, 8, 4, None, 3.1)
    assert list(bounds) == torch.tensor(W.DATASET_STATS["bounds_translations"] + W.DATASET_STATS["bounds_sizes"]).tolist()
    ok = dict(wall_scale=1.0, room_side=3.1, room_mask=room)
    for loop, kw in ((gd.p_sample_loop, {}), (gd.ddim_sample_loop, {}), (gd.p_sample_loop_masked, dict(known=torch.zeros(shape), mask=torch.zeros(shape) > 0))):
        for bad, match in ((dict(ok, wall_scale=-1.0), "wall_scale"), (dict(ok, wall_scale=[0.1] * 3), "wall_scale"),
                           (dict(ok, wall_steps=51), "wall_steps"), (dict(wall_steps=3), "wall_scale"),
                           (dict(room_side=3.1, room_mask=room), "wall_scale"), (dict(wall_scale=1.0, room_mask=room), "room_side"),
                           (dict(ok, room_side=0.0), "room_side"), (dict(ok, room_side=float("inf")), "room_side"),
                           (dict(ok, room_mask=None), "room_mask"), (dict(ok, room_mask=room[:, 0]), "room_mask"),
                           (dict(ok, room_mask=torch.zeros(3, 1, 8, 12)), "room_mask"), (dict(ok, room_mask=torch.zeros(2, 1, 1, 12)), "room_mask"),
                           (dict(ok, room_mask=torch.zeros(2, 1, 300, 12)), "room_mask")):
            with pytest.raises(ValueError, match=match):
                loop(None, shape, "cpu", None, None, noise_fn=never, **bad, **kw)
        with pytest.raises(ValueError, match="at most 160"):
            loop(None, (2, 161, 12), "cpu", None, None, noise_fn=never, **ok,
                 **{k_: torch.zeros((2, 161, 12)) > 0 if k_ == "mask" else torch.zeros((2, 161, 12)) for k_ in kw})
    with pytest.raises(ValueError, match="train_stats_file") as e:                   # no statistics file: the key is named
        _gd(None).p_sample_loop(None, shape, "cpu", None, None, noise_fn=never, **ok)
    assert "wall_scale" in str(e.value)
    with pytest.raises(ValueError, match="angle_dim = 2"):
        _gd(str(stats), angle_dim=1).p_sample_loop(None, (2, 5, 11), "cpu", None, None, noise_fn=never, **ok)
    with pytest.raises(ValueError, match="full object layout"):                      # a re-arrangement sub-shape
        gd.p_sample_loop(None, (2, 5, 5), "cpu", None, None, noise_fn=never, **ok)
    for name in ("p_sample_loop_arrange", "ddim_arrange_loop"):                      # the arrange loops do not take the keyword at all
        with pytest.raises(TypeError):
            getattr(gd, name)(None, shape, "cpu", None, None, wall_scale=1.0)


def test_the_wrapper_hands_the_keywords_on_and_none_is_the_old_call(tmp_path):
    N, C = 12, 62
    m = _wrapper("uncond", tmp_path)
    room = torch.zeros(3, 1, 64, 64)
    room[:, :, 16:48, 16:48] = 1
    walls = dict(wall_scale=[0.0, 0.02, 0.1], wall_steps=20, room_side=3.1)
    known = torch.zeros(3, N, C)
    with contextlib.redirect_stdout(io.StringIO()):
        m.generate_layout_batched(room, N, C, 3)
        m.generate_layout_batched(room, N, C, 3, **walls)
        m.generate_layout_batched(room[:1], N, C, 3, sampling_timesteps=50, scene_seeds=[1, 2, 3], collision_scale=0.1, **walls)
        m.generate_layout(room, N, C, 3, wall_scale=0.05, room_side=3.1)
        m.complete_scene_batched(room, N, C, [known[0, :2], known[1, :0], known[2, :5]], **walls)
        m.complete_scene_batched(room, N, C, known[:, :4], sampling_timesteps=10, **walls)
        m.complete_scene(room, N, C, known[:, :4], 3, **walls)
        m.complete_scene(room, N, C, known[:, :4], 3, sampling_timesteps=10, **walls)
        m.inpaint_scene_batched(room, N, C, known, torch.zeros(3, N, dtype=torch.bool), **walls)
        m.inpaint_scene_batched(room, N, C, known, torch.zeros(3, N, dtype=torch.bool))
    calls = m.diffusion.calls
    assert [c[0] for c in calls] == ["gen_samples", "gen_samples", "gen_samples_ddim", "gen_samples", "complete_samples_ragged",
                                     "complete_samples_ragged_ddim", "complete_samples", "complete_samples_ragged_ddim", "inpaint_samples",
                                     "inpaint_samples"]
    for i in (0, 9):                                                                 # None: not a keyword more than before
        assert not {"wall_scale", "wall_steps", "room_side", "room_mask"} & set(calls[i][2])
    for i in (1, 2, 4, 5, 6, 7, 8):
        kw = calls[i][2]
        assert kw["wall_scale"] == walls["wall_scale"] and kw["wall_steps"] == 20 and kw["room_side"] == 3.1
        assert kw["room_mask"] is (room if i != 2 else kw["room_mask"]) and kw["room_mask"].shape[1:] == (1, 64, 64)
    assert calls[2][2]["room_mask"].shape[0] == 1 and calls[2][2]["collision_scale"] == 0.1 and "noise_fn" in calls[2][2]
    assert calls[3][2]["wall_scale"] == 0.05 and calls[3][2]["wall_steps"] is None and "collision_scale" not in calls[3][2]
    before = len(calls)
    cpu_rng = torch.get_rng_state()
    ok = dict(wall_scale=0.1, room_side=3.1)
    bads = ((dict(ok, wall_scale=-1.0), room), (dict(ok, wall_scale=[0.1, 0.2]), room), (dict(ok, wall_steps=-1), room), (dict(wall_steps=5), room),
            (dict(room_side=3.1), room), (dict(wall_scale=0.1), room), (dict(ok, room_side=-2.0), room), (dict(ok, room_side=float("nan")), room),
            (dict(ok, wall_scale=float("nan")), room), (ok, room[:, 0]), (ok, room[:2]), (ok, torch.zeros(3, 1, 64, 300)),
            (ok, torch.zeros(3, 3, 64, 64)))
    for bad, mask in bads:
        for fn, args in ((m.generate_layout_batched, (mask, N, C, 3)), (m.sample, (mask, N, C, 3)),
                         (m.complete_scene_batched, (mask, N, C, known[:, :4])), (m.complete_scene, (mask, N, C, known[:, :4], 3)),
                         (m.inpaint_scene_batched, (mask, N, C, known, torch.zeros(3, N, dtype=torch.bool)))):
            with pytest.raises(ValueError, match="wall_s|room_side|room_mask"):
                fn(*args, **bad)
    with pytest.raises(ValueError, match="ret_traj"):
        m.sample(room, N, C, 3, ret_traj=True, **ok)
    with pytest.raises(ValueError, match="at most 160"):
        m.generate_layout_batched(room, 161, C, 3, **ok)
    assert len(calls) == before and torch.equal(torch.get_rng_state(), cpu_rng)      # refused before anything is drawn


def test_a_missing_statistics_file_is_refused_by_the_wrapper(tmp_path):
    m = _wrapper("uncond", tmp_path)
    m.diffusion.diffusion.train_stats_file = None
    m.diffusion.diffusion.loss_iou = False
    m.diffusion.diffusion._box_bounds = None
    cpu_rng = torch.get_rng_state()
    with pytest.raises(ValueError, match="train_stats_file"):
        m.generate_layout_batched(torch.ones(1, 1, 8, 8), 12, 62, 3, wall_scale=0.05, room_side=3.1)
    assert m.diffusion.calls == [] and torch.equal(torch.get_rng_state(), cpu_rng)


def test_rearrangement_refuses_the_keywords(tmp_path):
    m = _wrapper("arrange", tmp_path)
    N, C = 12, 62
    room, boxes = torch.zeros(2, 1, 64, 64), torch.zeros(2, N, C)
    for fn, args in ((m.arrange_scene, (room, N, C, boxes, 2)), (m.arrange_scene_batched, (room, N, C, boxes))):
        for kw in (dict(wall_scale=0.1, room_side=3.1), dict(wall_steps=3), dict(room_side=3.1), dict(wall_scale=0.1, room_side=3.1, sampling_timesteps=5)):
            with pytest.raises(ValueError, match="re-arrangement"):
                fn(*args, **kw)
    with pytest.raises(ValueError, match="re-arrangement"):
        m.sample(room, N, C, 2, input_boxes=boxes, wall_scale=0.1, room_side=3.1)
    assert m.diffusion.calls == []
    assert m._check_walls(None, None, None, room, (2, N, C), boxes) == {}            # without the keywords: the call as it was


# ------------------------------------------------------------------------------------------------------------------- the order of the launches
RECS = (("steer_rec", "dsc_steer_boxes_f32"), ("walls_rec", "dsc_steer_walls_f32"), ("multistep_rec", "dsc_multistep_x0_f32"), ("step_rec", "the step"))


def _record(monkeypatch):
    """ops.*_rec return their entry point's name, ops.issue records it: the launches of a step, in order, without a device."""
    from diffuscene_amd import ops
    names = []
    for rec, name in RECS:
        monkeypatch.setattr(ops, rec, lambda *a, _n=name, **k: (_n, (), ()))
    monkeypatch.setattr(ops, "issue", lambda rec, stream=None: names.append(rec[0]))
    monkeypatch.setattr(ops, "cfg_combine", lambda mo, scale: names.append("dsc_cfg_combine_f32") or mo)
    return names


def test_the_eager_model_call_issues_walls_after_collision_and_before_multistep(monkeypatch, tmp_path):
    from diffuscene_amd.networks import diffusion_ddpm as D
    names = _record(monkeypatch)
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    gd = _gd(str(stats))
    gd.tables, gd._coeffs = (lambda device: None), (lambda tb: (None, None))
    shape = (2, 5, 12)
    x, t = torch.zeros(shape), torch.zeros(2, dtype=torch.int64)
    steer = gd._steer_inputs(shape, "cpu", 0.1, None, "loop")
    walls = gd._wall_inputs(shape, "cpu", 0.05, None, 3.1, torch.ones(1, 1, 8, 8), "loop", field=False)
    post = lambda x, mo: names.append("dsc_multistep_x0_f32")  # noqa: E731
    plain = D._model(lambda x, t_, c, cc: x.clone(), None, None)
    D._corrected(plain, gd, "cpu", D._FREE, steer=steer, walls=walls)(x, t, post)
    assert names == ["dsc_steer_boxes_f32", "dsc_steer_walls_f32", "dsc_multistep_x0_f32"]
    del names[:]
    D._corrected(plain, gd, "cpu", D._FREE, walls=walls)(x, t)                            # walls alone, no solver
    assert names == ["dsc_steer_walls_f32"]
    del names[:]
    scale = torch.ones(2)
    guided = D._guided_model(lambda x, t_, c, cc: x.clone(), None, None, scale)     # under guidance: on the 2 B output, before the mix
    D._corrected(guided, gd, "cpu", D._FREE, scale, walls=walls)(x, t, post)
    assert names == ["dsc_steer_walls_f32", "dsc_multistep_x0_f32", "dsc_cfg_combine_f32"]
    del names[:]
    D._corrected(plain, gd, "cpu", D._FREE, steer=steer)(x, t, post)                      # without the keyword: no such launch
    plain(x, t)
    assert names == ["dsc_steer_boxes_f32", "dsc_multistep_x0_f32"]
    assert D._wall_kw(None, None, None, torch.ones(1, 1, 8, 8)) == {}               # a room mask alone asks for nothing


def test_the_captured_step_issues_walls_after_collision_and_before_multistep(monkeypatch):
    from diffuscene_amd import sampler
    names = _record(monkeypatch)

    def part(cls, **attrs):
        o = object.__new__(cls)
        o.__dict__.update(attrs)
        return o
    g = SimpleNamespace(x=None, mean_type=0, sched={}, guide=None, _model_call=lambda: None, _main_draw=lambda final: None, _move=lambda: None,
                        part=SimpleNamespace(before=lambda g: None, operands=lambda g, final: {}, steer_operands=lambda g: {}),
                        steer=part(sampler._Steer, spec=()), walls=part(sampler._Walls, spec=()),
                        multistep=part(sampler._Multistep, hist=None, weights=None))
    sampler._Loop._step(g, False)
    assert names == [name for _, name in RECS]
    del names[:]
    sampler._Loop._step(g, True)                                                     # the last pair has no multistep launch
    assert names == ["dsc_steer_boxes_f32", "dsc_steer_walls_f32", "the step"]
    del names[:]
    g.walls = None                                                                   # wall_scale=None: the step as it was
    sampler._Loop._step(g, False)
    assert names == ["dsc_steer_boxes_f32", "dsc_multistep_x0_f32", "the step"]
    g.steer = g.multistep = None
    del names[:]
    sampler._Loop._step(g, False)
    assert names == ["the step"]


def test_every_front_end_takes_the_keyword_and_none_reaches_the_loop_as_before():
    from diffuscene_amd import sampler
    from test_step_table_host import FRONT_ENDS
    x = torch.zeros(2, 3, 12)
    for front in sorted(FRONT_ENDS.values()):
        with pytest.raises(RuntimeError, match="graph sampling needs"):
            getattr(sampler, front)(None, None, (2, 3, 12), "cpu", None, None, *([x[:, 0, 0]] if "guided" in front else []),
                                    *((5, 0.0) if "ddim" in front else (True, 5)), walls=None)


# ------------------------------------------------------------------------------------------------------------------- the symbols
@pytest.mark.parametrize("symbol,names", [("dsc_floor_field_f32", ("mask", "field", "room_side")),
                                          ("dsc_steer_walls_f32", ("weight", "t_below", "bounds", "field", "room_side", "energy_out", "grad_out",
                                                                   "outside_out", "cfg_scale", "field_b", "h", "w"))])
def test_the_new_symbols_are_declared_exported_and_bound(symbol, names):
    import ctypes
    from diffuscene_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % symbol, hdr, flags=re.M | re.S)
    assert m, "%s is not declared" % symbol
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES[symbol]
    assert hasattr(_lib.load(), symbol) and restype is ctypes.c_int and len(argtypes) == len(params)
    for p, ty in zip(params, argtypes):
        assert (ty is ctypes.c_int32) == p.startswith("int32_t "), p                # a value, not the int32_t* of outside_out
        assert (ty is ctypes.c_float) == p.startswith("float "), p
    for name in names:
        assert any(p.endswith(name) for p in params), name
