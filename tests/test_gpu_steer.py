"""GPU: collision steering (dsc_steer_boxes_f32, ops.box_repulsion / steer_boxes, the ``collision_scale`` keyword of the loops).

The reference of every comparison is the float64 oracle of tests/steer_oracle.py -- torch autograd over networks/loss.py, the definition
of INTEGRATION.md 9 -- on inputs whose three kinds of decision (sign of an overlap, which face is the inner one, validity) it takes with
a float64 margin of 1e-4 or more; that condition is asserted before the device is touched.  The yardstick is the same oracle evaluated
in float32 on the CPU, per scene, as max |delta| / max |g|; the kernel is held to 4 x that yardstick, measured here for the same inputs
(it may order the sum over j and form r - l differently; each is worth about a factor of two).  DSC_PARITY_LOG=<file> records the
measured values (profiles/steer_parity.txt).

 1. ops.box_repulsion: gradient and energy against the oracle; N = 1, all-empty and touching-only scenes give exactly zero; N = 161 is
    refused.
 2. the steered output: steer, then the UNCHANGED ops.p_sample(clip=True, x0_out=...): its x0 is clamp(x0 - w g64), for eps, x0 and v
    at t in {0, 1, T - 1}; only valid free translation elements of model_out change.
 3. given parts: given boxes repel free ones and are never written; a whole-row prefix mask is the rows form bit for bit.
 4. guidance: both halves receive the same delta; the fused guided step on the steered 2 B output equals cfg_combine + steer at B + the
    plain step to the bound of 2.
 5. inactivity: collision_scale = 0, collision_steps = 0 and a zero weight for one scene of a mixed batch are the unsteered loop, bitwise.
 6. batch independence: scene b alone is scene b of the batch, bitwise.
 7. loops: eager == captured (torch.equal) at T = 8 and S = 4 on seeded weights, B = 2, N = 5; one graph serves two (weight, K).
 8. effect: on the last step E(x0') <= E(x0) for every scene."""
import contextlib
import functools
import io
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import steer_oracle as O  # noqa: E402
from oracle import weights as W  # noqa: E402

SIZES, SEEDS, TAIL_SIZES = (1, 2, 5, 64, 65, 160), (0, 1, 2), (5, 65)
T = 1000
MEAN = {"eps": 0, "x0": 1, "v": 2}
QUIET = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def no_device_errors():
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    yield
    assert _lib.device_error_count(reset=True) == 0


def log(line):
    print(line)
    if os.environ.get("DSC_PARITY_LOG"):
        with open(os.environ["DSC_PARITY_LOG"], "a") as f:
            f.write(line + "\n")


def held(what, err, yard):
    """err <= 4 x yard, scene by scene; both are printed first."""
    log("%s: kernel %s, float32 oracle %s" % (what, ["%.3g" % v for v in err.tolist()], ["%.3g" % v for v in yard.tolist()]))
    assert bool((err <= 4 * yard).all()), (what, err.tolist(), yard.tolist())


@functools.lru_cache(maxsize=None)
def scene(n, seed, c=O.C12):
    """(scenes, E64, g64, E32, g32), computed once and shared; the margin condition is asserted here, before any launch."""
    x = O.make_scenes(n, seed, c=c)
    O.assert_margins(x, (n, seed, c))
    E, g, _, _ = O.energy_grad(x)
    E32, g32, _, _ = O.energy_grad(x, torch.float32)
    return x, E, g, E32, g32


def repulsion(x):
    from diffuscene_amd import ops
    E, g = ops.box_repulsion(x.to(dev()), O.BOUNDS, class_dim=O.CLASSES)
    return E.cpu(), g.cpu()


# ------------------------------------------------------------------------------------------------------------------- 1. standalone
@pytest.mark.parametrize("n", SIZES)
def test_gradient_and_energy_against_the_float64_oracle(n):
    for seed in SEEDS:
        for c in (O.C12,) + ((O.C12 + 32,) if n in TAIL_SIZES and seed == 0 else ()):
            x, E, g, E32, g32 = scene(n, seed, c)
            x_dev = x.to(dev())
            before = x_dev.clone()
            gotE, gotg = repulsion(x)
            assert torch.equal(x_dev, before)                                   # weight 0: nothing is written
            if n == 1:
                assert float(gotE.abs().max()) == 0.0 and float(gotg.abs().max()) == 0.0
                continue
            held("box_repulsion gradient n=%d seed=%d c=%d" % (n, seed, c), O.rel_err(gotg, g, g), O.rel_err(g32, g, g))
            held("box_repulsion energy   n=%d seed=%d c=%d" % (n, seed, c), O.rel_err(gotE, E, E), O.rel_err(E32, E, E))
            invalid = x[..., O.EMPTY] >= 0
            assert float(gotg[invalid].abs().max() if bool(invalid.any()) else 0.0) == 0.0


def test_empty_and_touching_scenes_give_exactly_zero_and_161_is_refused():
    from diffuscene_amd import _lib, ops
    x = O.make_scenes(64, 0)
    x[..., O.EMPTY] = x[..., O.EMPTY].abs()                                     # every box empty
    E, g = repulsion(x)
    assert float(E.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
    # boxes that touch along x and coincide in y and z, in exact arithmetic: centre = 2 x, half size = x_s + 1, angle 0
    bounds = (-2.0, -2.0, -2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0, 2.0, 2.0, 2.0)
    t = torch.zeros(2, 4, O.C12)
    t[..., 3:6], t[..., 6], t[..., O.EMPTY] = -0.5, 1.0, -1.0
    t[:, :, 0] = torch.tensor([-0.5, 0.0, 0.5, 1.0])                            # [-1.5, -0.5] [-0.5, 0.5] [0.5, 1.5] [1.5, 2.5]
    E, g = ops.box_repulsion(t.to(dev()), bounds, class_dim=O.CLASSES)
    assert float(E.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
    mo = t.to(dev())
    ops.steer_boxes(None, mo, torch.ones(2, device=dev()), torch.ones(1, device=dev(), dtype=torch.int64), bounds, MEAN["x0"],
                    class_dim=O.CLASSES, t=torch.zeros(2, device=dev(), dtype=torch.int64))
    assert torch.equal(mo.cpu(), t)
    t[:, 1, 0] = -0.25                                                          # now boxes 0 and 1 overlap by 0.5: the control
    E, g = ops.box_repulsion(t.to(dev()), bounds, class_dim=O.CLASSES)
    assert float(E.min()) > 0 and float(g[:, 0, 0].min()) > 0 > float(g[:, 1, 0].max())     # moving them together raises the energy
    # the limit
    big = torch.zeros(1, 161, O.C12, device=dev())
    with pytest.raises(ValueError, match="at most 160"):
        ops.box_repulsion(big, O.BOUNDS, class_dim=O.CLASSES)
    z = torch.zeros(1, device=dev())
    zi = torch.zeros(1, device=dev(), dtype=torch.int64)
    rc = _lib.fn("dsc_steer_boxes_f32")(None, big.data_ptr(), zi.data_ptr(), None, None, None, None, None, None, None, None, None, z.data_ptr(),
                                        zi.data_ptr(), ops.steer_bounds(O.BOUNDS), None, None, MEAN["x0"], 1, 161, 0, O.C12, 8, 4, 0, 1,
                                        ops.stream_ptr())
    assert rc == -3                                                             # DSC_ERANGE
    rc = _lib.fn("dsc_steer_boxes_f32")(None, big.data_ptr(), zi.data_ptr(), None, None, None, None, None, None, None, None, None, z.data_ptr(),
                                        zi.data_ptr(), ops.steer_bounds(O.BOUNDS), None, None, MEAN["x0"], 1, 160, 0, 5, 5, 0, 0, 1,
                                        ops.stream_ptr())
    assert rc == -1                                                             # a re-arrangement sub-shape: DSC_EINVAL


# ------------------------------------------------------------------------------------------------------------------- 2. the steered output
@functools.lru_cache(maxsize=None)
def diffusion(mean_type):
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    return GaussianDiffusion(dict(objectness_dim=0, class_dim=O.CLASSES, angle_dim=2, objfeat_dim=0), get_betas("linear", 1e-4, 0.02, T),
                             "mse", mean_type, "fixedsmall", False, False, None)


def chain_inputs(gd, x0, t, seed):
    """(x_t, m) on the CPU such that the model output m predicts the scenes x0 at the timesteps t: x_t = q_sample(x0, t, eps)."""
    eps = torch.randn(x0.shape, generator=torch.Generator().manual_seed(100 + seed))
    sa, sb = gd.sqrt_alphas_cumprod[t][:, None, None], gd.sqrt_one_minus_alphas_cumprod[t][:, None, None]
    x_t = sa * x0 + sb * eps
    m = {"eps": eps, "x0": x0.clone(), "v": sa * eps - sb * x0}[gd.model_mean_type]
    return x_t.contiguous(), m.contiguous()


def coeffs(gd, t, dtype):
    if gd.model_mean_type == "x0":
        return None, None
    a, b = (gd.sqrt_recip_alphas_cumprod, gd.sqrt_recipm1_alphas_cumprod) if gd.model_mean_type == "eps" else \
        (gd.sqrt_alphas_cumprod, gd.sqrt_one_minus_alphas_cumprod)
    return a[t][:, None, None].to(dtype), b[t][:, None, None].to(dtype)


def steered_x0(gd, x_t, m, t, w, dtype, given=None):
    """The definition, in ``dtype`` on the CPU: (x0' = the step's clamped x0 after steering, w g, the elements that move, raw x0).
    ``given`` = (known, mask): those elements take their known value and are never moved."""
    A, Bc = coeffs(gd, t, dtype)
    x, mo = x_t.to(dtype), m.to(dtype)
    raw = mo if A is None else A * x - Bc * mo
    x0 = raw.clamp(-1, 1)
    free = torch.ones_like(x0, dtype=torch.bool)
    if given is not None:
        x0 = torch.where(given[1], given[0].to(dtype), x0)
        free = ~given[1]
    _, g, _, _ = O.energy_grad(x0, dtype)
    wg = torch.zeros_like(x0)
    wg[..., 0:3] = w.to(dtype)[:, None, None] * g
    moves = free & (wg != 0) & (x0[..., O.EMPTY] < 0)[..., None]
    d = wg + (raw - raw.clamp(-1, 1))
    new_m = torch.where(moves, mo - d if A is None else mo + d / Bc, mo)
    new_raw = new_m if A is None else A * x - Bc * new_m
    out = new_raw.clamp(-1, 1)
    if dtype == torch.float64:                                                  # the reference: exactly clamp(x0 - w g) where it moves
        out = torch.where(moves, (x0 - wg).clamp(-1, 1), raw.clamp(-1, 1))
    return out, wg, moves, raw


def run_steer_then_step(gd, x_t, m, t, w, k_below=T, **operands):
    """steer in place, then the unchanged posterior step -> (model_out after steering, the step's x0_out), on the CPU."""
    from diffuscene_amd import ops
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    mo = m.to(dev()).clone()
    xd, td = x_t.to(dev()), t.to(dev())
    ops.steer_boxes(xd, mo, w.to(dev()), torch.full((1,), k_below, device=dev(), dtype=torch.int64), O.BOUNDS, MEAN[gd.model_mean_type],
                    ca, cb, class_dim=O.CLASSES, t=td, **operands)
    x0_out = torch.empty_like(xd)
    ops.p_sample(xd, mo, torch.zeros_like(xd), td, ca, cb, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], gd._sigma(tb),
                 MEAN[gd.model_mean_type], True, x0_out=x0_out)
    return mo.cpu(), x0_out.cpu()


W3 = torch.tensor([0.02, 0.01, 0.03])
T_SETS = ([0, 0, 0], [1, 1, 1], [T - 1] * 3, [0, 1, T - 1])


@pytest.mark.parametrize("mean_type", ["eps", "x0", "v"])
@pytest.mark.parametrize("n", [5, 65])
def test_the_unchanged_step_sees_the_steered_x0(mean_type, n):
    gd = diffusion(mean_type)
    x0 = scene(n, 0)[0]
    for tv in T_SETS:
        t = torch.tensor(tv, dtype=torch.int64)
        x_t, m = chain_inputs(gd, x0, t, n)
        want, wg, moves, raw = steered_x0(gd, x_t, m, t, W3, torch.float64)
        O.assert_margins(raw, (mean_type, n, tv))                               # on the float64 x0 of these very inputs
        yard = O.rel_err(steered_x0(gd, x_t, m, t, W3, torch.float32)[0][..., 0:3], want[..., 0:3], wg)
        mo, x0_out = run_steer_then_step(gd, x_t, m, t, W3)
        held("steered x0 %s n=%d t=%s" % (mean_type, n, tv), O.rel_err(x0_out[..., 0:3], want[..., 0:3], wg), yard)
        changed = mo != m
        assert bool(changed.any()) and not bool((changed & ~moves).any()), (mean_type, n, tv)      # only valid free translation elements
        assert torch.equal(x0_out[..., 3:], raw.float().clamp(-1, 1)[..., 3:]) or mean_type != "x0"


# ------------------------------------------------------------------------------------------------------------------- 3. given parts
def given_inputs(n):
    x0 = scene(n, 0)[0]
    known = scene(n, 1)[0].clamp(-1, 1)
    mask = torch.rand(x0.shape, generator=torch.Generator().manual_seed(5)) < 0.3
    mask[:, 0] = True                                                           # a box given whole ...
    mask[:, 1, 0:3] = True                                                      # ... one with its translation given ...
    mask[:, 2] = False                                                          # ... and a free one
    return x0, known, mask


@pytest.mark.parametrize("n", [5, 65])
def test_given_boxes_repel_free_ones_and_are_never_written(n):
    from diffuscene_amd import ops
    gd = diffusion("x0")
    x0, known, mask = given_inputs(n)
    t = torch.zeros(3, dtype=torch.int64)
    want, wg, moves, raw = steered_x0(gd, x0, x0, t, W3, torch.float64, (known, mask))
    O.assert_margins(torch.where(mask, known, x0.clamp(-1, 1)), ("given", n))
    yard = O.rel_err(steered_x0(gd, x0, x0, t, W3, torch.float32, (known, mask))[0][..., 0:3], want[..., 0:3], wg)
    m8 = mask.to(torch.uint8).to(dev())
    mo, x0_out = run_steer_then_step(gd, x0, x0, t, W3, mask=(known.to(dev()), None, m8))
    assert not bool(((mo != x0) & (mask | ~moves)).any())                       # a given element is never written, nor any other that must not move
    free_moves = moves & ~mask
    assert bool(free_moves.any()) and bool((mo != x0)[free_moves].any())
    got = torch.where(mask, want.float(), x0_out)                               # the step knows no given part: judge the free elements
    held("steered x0 under a mask n=%d" % n, O.rel_err(got[..., 0:3], want[..., 0:3], wg), yard)
    # the force a free box feels from a given one: move a given box away and the free boxes' gradient changes
    E = torch.empty(3, device=dev())
    g = torch.empty(3, n, 3, device=dev())
    ops.steer_boxes(None, x0.to(dev()), torch.zeros(3, device=dev()), torch.zeros(1, device=dev(), dtype=torch.int64), O.BOUNDS, MEAN["x0"],
                    class_dim=O.CLASSES, t=t.to(dev()), mask=(known.to(dev()), None, m8), energy_out=E, grad_out=g)
    _, g64, _, _ = O.energy_grad(torch.where(mask, known, x0.clamp(-1, 1)))
    held("gradient under a mask n=%d" % n, O.rel_err(g.cpu(), g64, g64),
         O.rel_err(O.energy_grad(torch.where(mask, known, x0.clamp(-1, 1)), torch.float32)[1], g64, g64))


@pytest.mark.parametrize("mean_type", ["x0", "eps"])
def test_a_whole_row_prefix_mask_is_the_rows_form_bit_for_bit(mean_type):
    from diffuscene_amd import ops
    gd = diffusion(mean_type)
    n, pmax, counts = 65, 40, [0, 7, 40]
    x0, known = scene(n, 0)[0], scene(n, 1)[0].clamp(-1, 1)
    t = torch.tensor([1, 0, 1], dtype=torch.int64)
    x_t, m = chain_inputs(gd, x0, t, 3)
    cnt = torch.tensor(counts, dtype=torch.int64)
    mask = (torch.arange(n)[None, :, None] < cnt[:, None, None]).expand(3, n, O.C12).contiguous()
    partial = known[:, :pmax].contiguous().to(dev())
    outs = []
    for operands in (dict(rows=(partial, None, cnt.to(dev()))), dict(mask=(known.to(dev()), None, mask.to(torch.uint8).to(dev())))):
        tb = gd.tables(dev())
        ca, cb = gd._coeffs(tb)
        mo = m.to(dev()).clone()
        E, g = torch.empty(3, device=dev()), torch.empty(3, n, 3, device=dev())
        ops.steer_boxes(x_t.to(dev()), mo, W3.to(dev()), torch.full((1,), T, device=dev(), dtype=torch.int64), O.BOUNDS, MEAN[mean_type], ca, cb,
                        class_dim=O.CLASSES, t=t.to(dev()), energy_out=E, grad_out=g, **operands)
        outs.append((mo.cpu(), E.cpu(), g.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    mo = outs[0][0]
    assert bool((mo != m).any()) and torch.equal(mo[mask], m[mask])             # steered, and never inside the given rows
    assert float(outs[0][2][1, :7].abs().max()) > 0                             # the given boxes feel the force they exert; they are not moved


# ------------------------------------------------------------------------------------------------------------------- 4. guidance
@pytest.mark.parametrize("mean_type,tv", [("x0", [0, 1, T - 1]), ("eps", [0, 1, 1])])
def test_guided_both_halves_move_by_the_same_delta(mean_type, tv):
    from diffuscene_amd import ops
    gd = diffusion(mean_type)
    n = 65
    x0 = scene(n, 0)[0]
    t = torch.tensor(tv, dtype=torch.int64)
    x_t, m = chain_inputs(gd, x0, t, 4)
    gen = torch.Generator().manual_seed(9)
    spread = 0.02 * torch.randn(m.shape, generator=gen)
    spread[..., O.EMPTY] = 0                                                    # the validity of a box does not hang on the mix
    c, u = m + spread, m - 0.5 * spread
    s = torch.tensor([0.0, 1.0, 2.5])
    mix = u + s[:, None, None] * (c - u)                                        # cfg_mix in float32, its three roundings
    mix64 = u.double() + s.double()[:, None, None] * (c.double() - u.double())
    want, wg, moves, raw = steered_x0(gd, x_t, mix64, t, W3, torch.float64)
    O.assert_margins(raw, ("guided", mean_type))
    yard = O.rel_err(steered_x0(gd, x_t, mix, t, W3, torch.float32)[0][..., 0:3], want[..., 0:3], wg)
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    post = (ca, cb, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], gd._sigma(tb), MEAN[mean_type], True)
    xd, td, sd, wd = x_t.to(dev()), t.to(dev()), s.to(dev()), W3.to(dev())
    kb = torch.full((1,), T, device=dev(), dtype=torch.int64)
    zero = torch.zeros_like(xd)
    # fused: steer the 2 B output with the scales, then the fused guided step
    mo2 = torch.cat([c, u]).to(dev())
    ops.steer_boxes(xd, mo2, wd, kb, O.BOUNDS, MEAN[mean_type], ca, cb, class_dim=O.CLASSES, t=td, scale=sd)
    fused = torch.empty_like(xd)
    ops.p_sample_cfg(xd, mo2, sd, zero, td, *post, x0_out=fused)
    # unfused: cfg_combine, steer at B, the plain step
    mB = ops.cfg_combine(torch.cat([c, u]).to(dev()), sd)
    assert torch.equal(mB.cpu(), mix)
    ops.steer_boxes(xd, mB, wd, kb, O.BOUNDS, MEAN[mean_type], ca, cb, class_dim=O.CLASSES, t=td)
    plain = torch.empty_like(xd)
    ops.p_sample(xd, mB, zero, td, *post, x0_out=plain)
    held("guided fused   %s" % mean_type, O.rel_err(fused.cpu()[..., 0:3], want[..., 0:3], wg), yard)
    held("guided unfused %s" % mean_type, O.rel_err(plain.cpu()[..., 0:3], want[..., 0:3], wg), yard)
    dc, du = mo2[:3].cpu() - c, mo2[3:].cpu() - u
    assert bool((dc != 0).any()) and torch.equal(dc != 0, du != 0) and not bool(((dc != 0) & ~moves).any())
    delta = (mB.cpu().double() - mix.double())                                  # what the unfused arm added to m
    ulp = 2.0 ** -22 * torch.maximum(torch.maximum(c.abs(), u.abs()), mix.abs()).double().clamp(min=float(delta.abs().max()))
    assert bool(((dc.double() - delta).abs() <= ulp).all()) and bool(((du.double() - delta).abs() <= ulp).all())


# ------------------------------------------------------------------------------------------------------------------- 6. batch independence
@pytest.mark.parametrize("n", [5, 160])
def test_scene_b_alone_is_scene_b_of_the_batch(n):
    from diffuscene_amd import ops
    gd = diffusion("v")
    x0 = scene(n, 1)[0]
    t = torch.tensor([1, 0, 5], dtype=torch.int64)
    x_t, m = chain_inputs(gd, x0, t, 6)
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    kb = torch.full((1,), T, device=dev(), dtype=torch.int64)

    def run(sl):
        mo = m[sl].to(dev()).clone()
        b = mo.shape[0]
        E, g = torch.empty(b, device=dev()), torch.empty(b, n, 3, device=dev())
        ops.steer_boxes(x_t[sl].to(dev()), mo, W3[sl].to(dev()), kb, O.BOUNDS, MEAN["v"], ca, cb, class_dim=O.CLASSES, t=t[sl].to(dev()),
                        energy_out=E, grad_out=g)
        return mo.cpu(), E.cpu(), g.cpu()
    batch = run(slice(0, 3))
    assert bool((batch[0] != m).any())
    for b in range(3):
        for whole, alone in zip(batch, run(slice(b, b + 1))):
            assert torch.equal(whole[b:b + 1], alone), (n, b)


# ------------------------------------------------------------------------------------------------------------------- 8. effect
@pytest.mark.parametrize("n", [5, 64, 65, 160])
def test_the_last_step_does_not_raise_the_energy(n):
    """t = 0 (the x0 the posterior step forms) and the last strided pair (its output is x0'), w = 0.02: E(x0') <= E(x0) for every scene."""
    from diffuscene_amd import ops
    gd = diffusion("x0")
    tb = gd.tables(dev())
    w = torch.full((3,), 0.02)
    kb = torch.full((1,), T, device=dev(), dtype=torch.int64)
    for seed in SEEDS:
        x0 = scene(n, seed)[0]
        E0 = O.energy_grad(x0)[0]
        t = torch.zeros(3, dtype=torch.int64)
        mo, x0_out = run_steer_then_step(gd, x0, x0, t, w)
        # the last strided pair: times_next < 0, the output is x0'
        step, times, tn = torch.zeros(1, dtype=torch.int64, device=dev()), torch.zeros(1, dtype=torch.int64, device=dev()), \
            torch.full((1,), -1, dtype=torch.int64, device=dev())
        mo2 = x0.to(dev()).clone()
        ops.steer_boxes(None, mo2, w.to(dev()), kb, O.BOUNDS, MEAN["x0"], tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"],
                        class_dim=O.CLASSES, strided=(step, times, tn, torch.zeros(3, 1, device=dev())))
        assert torch.equal(mo2.cpu(), mo)                                       # the strided time source reads the same t
        last = ops.ddim_step(x0.to(dev()), mo2, x0.to(dev()), step, times, tn, torch.zeros(3, 1, device=dev()), None, None,
                             tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"], MEAN["x0"]).cpu()
        assert torch.equal(last, x0_out)
        E1 = O.energy_grad(x0_out)[0]
        log("effect n=%d seed=%d: E(x0') / E(x0) = %s" % (n, seed, ["%.4f" % (float(a) / float(b)) if float(b) > 0 else "-" for a, b in zip(E1, E0)]))
        assert bool((E1 <= E0).all()), (n, seed, E1.tolist(), E0.tolist())
        assert bool((E1 < E0).any())


# ------------------------------------------------------------------------------------------------------------------- 5. and 7. the loops
LB, LN = 2, 5
_MODELS = {}


def model(mean_type, tmp_path_factory):
    """(DiffusionPoint over the seeded bedroom denoiser at T = 8 with a statistics file, the (B, N, 128) condition)."""
    from diffuscene_amd.networks.denoise_net import Unet1D
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint
    if "net" not in _MODELS:
        kw = dict(W.UNCOND_BEDROOM)
        net = Unet1D(**kw)
        net.load_state_dict(W.synth_state_dict(kw))
        stats = tmp_path_factory.mktemp("steer") / "dataset_stats.txt"
        stats.write_text(json.dumps(W.DATASET_STATS))
        _MODELS["net"], _MODELS["stats"] = net.to(dev()), str(stats)
        _MODELS["cond"] = W.synth_condition(LB, LN, 128, 0).contiguous().to(dev())
    if mean_type not in _MODELS:
        _MODELS[mean_type] = DiffusionPoint(_MODELS["net"], dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), time_num=8,
                                            model_mean_type=mean_type, train_stats_file=_MODELS["stats"])
    return _MODELS[mean_type], _MODELS["cond"]


def sample(dp, cond, strided, graph, seed=3, **steer):
    torch.manual_seed(seed)
    with torch.no_grad(), QUIET():
        if strided:
            return dp.gen_samples_ddim((LB, LN, 62), dev(), condition=cond, sampling_timesteps=4, ddim_sampling_eta=0.5, graph=graph, **steer)
        return dp.gen_samples((LB, LN, 62), dev(), condition=cond, clip_denoised=True, graph=graph, **steer)


@pytest.mark.parametrize("strided,mean_type", [(False, "v"), (True, "eps")])
def test_loops_eager_is_captured_and_inactive_is_unsteered(strided, mean_type, tmp_path_factory):
    dp, cond = model(mean_type, tmp_path_factory)
    plain = sample(dp, cond, strided, True)
    assert torch.equal(plain, sample(dp, cond, strided, False))
    # 7. eager == captured, steered; the steering moves the scenes
    steer = dict(collision_scale=[0.05, 0.02], collision_steps=None)
    eager = sample(dp, cond, strided, False, **steer)
    captured = sample(dp, cond, strided, True, **steer)
    assert torch.equal(eager, captured)
    assert not torch.equal(captured, plain)
    g = next(iter(dp.diffusion._graphs.values()))
    assert g.steer is not None
    # one graph, replayed with another (weight, K), no re-capture
    # (on these seeded weights only the first steps, t >= 5, see overlapping non-empty boxes: K is chosen to keep some of them)
    steer2 = dict(collision_scale=[0.0, 0.1], collision_steps=6 if strided else 7)
    captured2 = sample(dp, cond, strided, True, **steer2)
    assert next(iter(dp.diffusion._graphs.values())) is g and len(dp.diffusion._graphs) == 1
    assert torch.equal(captured2, sample(dp, cond, strided, False, **steer2))
    assert not torch.equal(captured2, captured) and not torch.equal(captured2, plain)
    # 5. a zero weight for one scene of a mixed batch: that scene is the unsteered one
    assert torch.equal(captured2[0], plain[0])
    # 5. collision_scale = 0 and collision_steps = 0: the unsteered loop, eager and captured
    for off in (dict(collision_scale=0.0), dict(collision_scale=[0.05, 0.02], collision_steps=0)):
        assert torch.equal(sample(dp, cond, strided, True, **off), plain)
        assert torch.equal(sample(dp, cond, strided, False, **off), plain)
    assert next(iter(dp.diffusion._graphs.values())) is g
    # without the keyword the unsteered graph is built again, as before
    assert torch.equal(sample(dp, cond, strided, True), plain)
    assert next(iter(dp.diffusion._graphs.values())).steer is None


def _given_scene(seed):
    """(LB, LN, 62) scenes of the bedroom layout [3 | 3 | 2 | 22 | 32] whose boxes are non-empty and crowd the middle of the room."""
    x = O.make_scenes(LN, seed, b=LB, c=62).clamp(-1, 1)
    x[..., 0:3] *= 0.4
    x[..., 8 + 22 - 1] = -x[..., 8 + 22 - 1].abs()
    return x.to(dev())


def _text_model(tmp_path_factory):
    from diffuscene_amd.networks.denoise_net import Unet1D
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint
    model("v", tmp_path_factory)
    if "text" not in _MODELS:
        kw = dict(W.TEXT_BEDROOM)
        net = Unet1D(**kw)
        net.load_state_dict(W.synth_state_dict(kw))
        _MODELS["text"] = DiffusionPoint(net.to(dev()), dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), time_num=8,
                                         model_mean_type="eps", train_stats_file=_MODELS["stats"])
        _MODELS["cross"] = W.synth_text_condition(LB, 7, 512, 0).contiguous().to(dev())
    return _MODELS["text"], _MODELS["cond"], _MODELS["cross"]


@pytest.mark.parametrize("kind", ["dense", "ragged", "ragged-ddim", "masked", "masked-ddim", "guided", "guided-ddim", "masked-guided"])
def test_loops_with_a_given_part_or_guidance_eager_is_captured(kind, tmp_path_factory):
    """The other rows of the loop table under steering: eager == captured (torch.equal), and with weight 0 the unsteered loop."""
    shape = (LB, LN, 62)
    strided = dict(sampling_timesteps=4, ddim_sampling_eta=0.5) if kind.endswith("ddim") else {}
    known = _given_scene(11)
    mask = torch.zeros(shape, dtype=torch.bool, device=dev())
    mask[:, :2] = True
    mask[:, 2, 3:] = True                                                       # a box whose translation is free, everything else given
    if "guided" in kind:
        dp, cond, cross = _text_model(tmp_path_factory)
        kw = dict(condition=cond, condition_cross=cross, guidance_scale=[1.5, 0.5])
        if kind == "masked-guided":
            call, kw = dp.inpaint_samples_guided, dict(kw, known=known, mask=mask)
        else:
            call = dp.gen_samples_guided_ddim if strided else dp.gen_samples_guided
    else:
        dp, cond = model("eps" if strided else "v", tmp_path_factory)
        kw = dict(condition=cond)
        if kind == "dense":
            call, kw = dp.complete_samples, dict(kw, partial_boxes=known[:, :2].contiguous())
        elif kind.startswith("ragged"):
            call = dp.complete_samples_ragged_ddim if strided else dp.complete_samples_ragged
            kw.update(partial_boxes=known[:, :3].contiguous(), num_partial=[3, 1])
        else:
            call = dp.inpaint_samples_ddim if strided else dp.inpaint_samples
            kw.update(known=known, mask=mask)

    def run(graph, **steer):
        torch.manual_seed(5)
        with torch.no_grad(), QUIET():
            return call(shape, dev(), graph=graph, **kw, **strided, **steer)
    plain = run(True)
    steer = dict(collision_scale=[0.2, 0.1])
    eager, captured = run(False, **steer), run(True, **steer)
    assert torch.equal(eager, captured), kind
    moved = [float((captured[b] - plain[b]).abs().max()) for b in range(LB)]
    log("loop %s: steering moved the scenes by %s" % (kind, moved))
    assert torch.equal(run(True, collision_scale=0.0), plain) and torch.equal(run(False, collision_scale=[0.2, 0.1], collision_steps=0), plain)
    if "guided" not in kind:                                                    # the given elements come back as they were given
        given = mask if "masked" in kind else None
        if given is not None:
            assert torch.equal(captured[given], known[given])
        assert max(moved) > 0, kind                                             # given boxes in the middle of the room: the free ones are pushed
