"""GPU: floor-plan steering (dsc_floor_field_f32, dsc_steer_walls_f32, ops.floor_field / floor_violation / steer_walls, the ``wall_scale``
keyword of the loops, scene_stats.out_of_room).

The reference of every comparison is the float64 oracle of tests/wall_oracle.py -- the definition of INTEGRATION.md 9 in torch -- on
inputs whose decisions (the cell of a sample point, the clamp at the image border, validity) it takes with a margin: every sample point
of a valid box lies 1e-6 px or more from every integer pixel coordinate, every empty logit is 1e-4 or more from 0.  That condition is
asserted before the device is touched, and so is that every batch holds a valid box with a point outside its room.
DSC_PARITY_LOG=<file> records the measured values (profiles/walls_parity.txt).

 1. the field: bit-identical to the oracle's brute force -- both take the minimum of the same float64 expressions and round once.
 2. ops.floor_violation: per scene max |got - want| <= 2^-23 max |want| for the gradient and for the energy (float64 arithmetic, one
    final rounding of half an ulp, reordering noise of order 1e-13); ``outside`` exactly.
 3. a full mask, an all-empty scene, a scene of weight 0 and a mask without an inside pixel: energy 0, gradient 0, the model output
    bit for bit what it was (NaN-poisoned where it must not even be read); N = 161 is refused.
 4. the unchanged step (p_sample, ddim_step) after the launch forms clamp(x0) - w g in channels 0 and 2, to the rounding of the step;
    every other element of its x0 is bit-identical to the unsteered step's.
 5. given parts: given elements are never written; a whole-row prefix mask is the rows form bit for bit.
 6. guidance: both halves move by the same delta.
 7. batch independence: scene b alone is scene b of the batch; a shared (1, 1, H, W) mask is the mask expanded to B.
 8. effect: at t = 0 and at the last strided pair, w = 0.05, E(x0') <= E(x0) for every scene, < for one.
 9. loops at T = 8 on seeded weights, B = 2, N = 5: eager == captured (torch.equal) on every row; one graph serves another mask, other
    weights and another K; inactive is unsteered; without the keyword the unsteered graph is built as before.
10. scene_stats.out_of_room equals the oracle on the scenes of 2."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import wall_oracle as O  # noqa: E402
from test_gpu_steer import LB, LN, MEAN, QUIET, T, _given_scene, _text_model, chain_inputs, dev, diffusion, model  # noqa: E402

SIZES, SEEDS = (1, 5, 64, 65, 160), (0, 1)
EPS = 2.0 ** -23
W3 = torch.tensor([0.05, 0.02, 0.1])
SIDE = 3.1


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


def bits(x):
    return x.contiguous().view(torch.int32)


def violation(x, mask, side):
    from diffuscene_amd import ops
    E, g, out = ops.floor_violation(x.to(dev()), mask.to(dev()), side, O.BOUNDS, class_dim=O.CLASSES)
    return E.cpu(), g.cpu(), out.cpu()


def one_pair(t):
    """The strided time source of a one-pair schedule at timestep t[0]: (step counter, times, times_next = -1, coefficient rows)."""
    return (torch.zeros(1, dtype=torch.int64, device=dev()), t[:1].contiguous(), torch.full((1,), -1, dtype=torch.int64, device=dev()),
            torch.zeros(3, 1, device=dev()))


def walls(w, mask, side, k_below=T):
    """(weight, t_below, bounds, field, room_side) of ops.steer_walls on the device."""
    from diffuscene_amd import ops
    return (w.to(dev()), torch.full((1,), k_below, device=dev(), dtype=torch.int64), O.BOUNDS, ops.floor_field(mask.to(dev()), side),
            torch.full((1,), side, device=dev()))


# ------------------------------------------------------------------------------------------------------------------- 1. the field
@pytest.mark.parametrize("h,w", [(2, 2), (8, 12), (64, 64)])
def test_the_field_is_the_oracle_bit_for_bit(h, w):
    from diffuscene_amd import ops
    for side in (3.1, 2.0):
        for kinds in (("none", "full", "pixel"), ("L", "random", "rect")):
            mask = torch.stack([O.room(k, h, w, side, seed=h + i) for i, k in enumerate(kinds)])[:, None]
            want = O.field(mask[:, 0], side)
            got = ops.floor_field(mask.to(dev()), side).cpu()
            assert got.shape == (3, h, w) and got.dtype == torch.float32
            assert torch.equal(got, want), (h, w, side, kinds, float((got - want).abs().max()))
            assert float(got[mask[:, 0] > 0.5].abs().max() if bool((mask > 0.5).any()) else 0.0) == 0.0
            assert torch.equal(ops.floor_field(mask.to(torch.uint8).to(dev()), side).cpu(), want)      # a uint8 mask is the same mask
    assert float(O.field(O.room("none", h, w, 3.1), 3.1).abs().max()) == 0.0         # no inside pixel: F == 0


# ------------------------------------------------------------------------------------------------------------------- 2. energy and gradient
@pytest.mark.parametrize("n", SIZES)
def test_energy_gradient_and_outside_against_the_float64_oracle(n):
    from diffuscene_amd import ops
    for seed in SEEDS:
        for h, w, side in O.ROOMS:
            x, mask, E, g, out = O.case(n, seed, h, w, side)
            x_dev = x.to(dev())
            before = x_dev.clone()
            gotE, gotg, got_out = (v.cpu() for v in ops.floor_violation(x_dev, mask.to(dev()), side, O.BOUNDS, class_dim=O.CLASSES))
            assert torch.equal(x_dev, before)                                       # weight 0: nothing is written
            eg, ee = O.rel_err(gotg, g, g), O.rel_err(gotE, E, E)
            log("floor_violation n=%d seed=%d %dx%d s=%.1f: gradient %s, energy %s of 2^-23 max|want|"
                % (n, seed, h, w, side, ["%.3f" % (v / EPS) for v in eg.tolist()], ["%.3f" % (v / EPS) for v in ee.tolist()]))
            assert bool((eg <= EPS).all()) and bool((ee <= EPS).all()), (n, seed, h, w, side, eg.tolist(), ee.tolist())
            assert torch.equal(got_out.long(), out), (n, seed, h, w, side)
            assert float(gotg[..., 1].abs().max()) == 0.0                           # the y column stays 0
            invalid = x[..., O.EMPTY] >= 0
            assert float(gotg[invalid].abs().max() if bool(invalid.any()) else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------------------------- 3. exactly zero, refusals
def test_exactly_zero_cases_store_nothing_and_161_is_refused():
    from diffuscene_amd import _lib, ops
    n, side = 65, 6.0                                                               # a 12 m window: every sample point is inside the image
    x = O.make_scenes(n, 0)
    assert O.outside_image(x, 16, 16, side) == 0 and float(x[..., 0:3].abs().max()) > 1.0       # a store would clamp these translations
    t = torch.zeros(3, dtype=torch.int64, device=dev())
    L = O.rooms(16, 16, side)
    empty = x.clone()
    empty[..., O.EMPTY] = empty[..., O.EMPTY].abs()
    for what, scenes, mask in (("a full mask", x, O.room("full", 16, 16, side)[None, None]), ("an all-empty scene", empty, L),
                               ("no inside pixel", x, O.room("none", 16, 16, side)[None, None])):
        E, g, out = violation(scenes, mask, side)
        assert float(E.abs().max()) == 0.0 and float(g.abs().max()) == 0.0 and int(out.abs().max()) == 0, what
        mo = scenes.to(dev()).clone()
        wt, kb, bd, fld, rs = walls(torch.ones(3), mask, side)
        ops.steer_walls(None, mo, wt, kb, bd, fld, rs, MEAN["x0"], class_dim=O.CLASSES, t=t)
        assert torch.equal(bits(mo.cpu()), bits(scenes)), what
    # the control: the L-shaped rooms do move these scenes; a scene of weight 0 and a launch at t >= K are not even read
    assert float(violation(x, L, side)[0].min()) > 0
    poisoned = x.clone()
    poisoned[1] = float("nan")
    mo = poisoned.to(dev()).clone()
    wt, kb, bd, fld, rs = walls(torch.tensor([0.05, 0.0, 0.05]), L, side)
    ops.steer_walls(None, mo, wt, kb, bd, fld, rs, MEAN["x0"], class_dim=O.CLASSES, t=t)
    got = mo.cpu()
    assert torch.equal(bits(got[1]), bits(poisoned[1])) and not torch.equal(got[0], x[0]) and not torch.equal(got[2], x[2])
    mo = torch.full_like(mo, float("nan"))
    before = bits(mo.cpu())
    ops.steer_walls(None, mo, wt, torch.zeros(1, device=dev(), dtype=torch.int64), bd, fld, rs, MEAN["x0"], class_dim=O.CLASSES, t=t)
    assert torch.equal(bits(mo.cpu()), before)
    # the limit
    big = torch.zeros(1, 161, O.C12, device=dev())
    with pytest.raises(ValueError, match="at most 160"):
        ops.floor_violation(big, L[:1], side, O.BOUNDS, class_dim=O.CLASSES)
    z, zi = torch.zeros(1, device=dev()), torch.zeros(1, device=dev(), dtype=torch.int64)

    def raw(n_, c, bbox, classes, fb=1, h=16, w=16):
        return _lib.fn("dsc_steer_walls_f32")(None, big.data_ptr(), zi.data_ptr(), None, None, None, None, None, None, None, None, None,
                                              z.data_ptr(), zi.data_ptr(), ops.steer_bounds(O.BOUNDS), fld.data_ptr(), rs.data_ptr(), None,
                                              None, None, MEAN["x0"], 1, n_, 0, c, bbox, classes, 0, 1, fb, h, w, ops.stream_ptr())
    assert raw(161, O.C12, 8, 4) == -3                                              # DSC_ERANGE
    assert raw(160, O.C12, 8, 4, h=1) == -3 and raw(160, O.C12, 8, 4, w=257) == -3
    assert raw(160, 5, 5, 0) == -1                                                  # a re-arrangement sub-shape: DSC_EINVAL
    assert raw(160, O.C12, 8, 4, fb=3) == -1                                        # a field for another batch


# ------------------------------------------------------------------------------------------------------------------- 4. the steered x0
def step_x0(gd, x_t, mo, t, strided):
    """The x0 the UNCHANGED step forms from (x_t, mo): p_sample(clip=True) at the per-scene t, or ddim_step on a one-pair schedule."""
    from diffuscene_amd import ops
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    x0 = torch.empty_like(x_t)
    if strided:
        ops.ddim_step(x_t, mo, x_t, *one_pair(t), ca, cb, tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"],
                      MEAN[gd.model_mean_type], x0_out=x0)
    else:
        ops.p_sample(x_t, mo, torch.zeros_like(x_t), t, ca, cb, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], gd._sigma(tb),
                     MEAN[gd.model_mean_type], True, x0_out=x0)
    return x0


def step_bound(gd, x_t, m, mo, t, want):
    """The rounding of the step, element by element.  The launch forms d from the float32 raw = fl(fl(A x) - fl(B m)) and stores
    m' = fl(m + d / B); the step then forms fl(fl(A x) - fl(B m')).  Against the exact raw - d that is: the rounding of raw, of B m inside
    it, of m' (times B), of B m' and of the last difference -- half an ulp each, 2^-24 (|raw| + |B m| + 2 |B m'| + |x0'|); mean type x0
    has A = B = 0 and only the rounding of m' = x0'."""
    if gd.model_mean_type == "x0":
        return 2.0 ** -24 * want.abs() + 1e-12
    tb = gd.tables(dev())
    ca, cb = (v.cpu().double()[t][:, None, None] for v in gd._coeffs(tb))
    raw = ca * x_t.double() - cb * m.double()
    return 2.0 ** -24 * (raw.abs() + (cb * m.double()).abs() + 2 * (cb * mo.double()).abs() + want.abs()) + 1e-12


@pytest.mark.parametrize("mean_type", ["eps", "x0", "v"])
@pytest.mark.parametrize("n", [5, 65])
def test_the_unchanged_step_sees_the_steered_x0(mean_type, n):
    from diffuscene_amd import ops
    gd = diffusion(mean_type)
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    x0 = O.make_scenes(n, 0)
    mask = O.rooms(16, 16, SIDE)
    for tv in ([0, 0, 0], [1, 1, 1], [T - 1] * 3, [0, 1, T - 1]):
        t = torch.tensor(tv, dtype=torch.int64)
        x_t, m = chain_inputs(gd, x0, t, n)
        xd, td = x_t.to(dev()), t.to(dev())
        for strided in ((False, True) if len(set(tv)) == 1 else (False,)):
            plain = step_x0(gd, xd, m.to(dev()), td, strided).cpu()                 # the clamped float32 x0 the launch steers
            O.assert_margins(plain, mask, SIDE, (mean_type, n, tv))
            _, g, _ = O.energy_grad(plain, mask, SIDE)
            wg = torch.zeros_like(plain, dtype=torch.float64)
            wg[..., 0:3] = W3.double()[:, None, None] * g
            moves = wg != 0
            want = torch.where(moves, (plain.double() - wg).clamp(-1, 1), plain.double())
            mo = m.to(dev()).clone()
            wt, kb, bd, fld, rs = walls(W3, mask, SIDE)
            operands = dict(strided=one_pair(td)) if strided else dict(t=td)
            ops.steer_walls(xd, mo, wt, kb, bd, fld, rs, MEAN[mean_type], ca, cb, class_dim=O.CLASSES, **operands)
            got = step_x0(gd, xd, mo, td, strided).cpu()
            mo = mo.cpu()
            changed = mo != m
            assert bool(changed.any()) and not bool((changed & ~moves).any()), (mean_type, n, tv)      # only valid boxes, channels 0 and 2
            assert not bool(changed[..., 1].any()) and not bool(changed[..., 3:].any())
            assert torch.equal(bits(got)[~changed], bits(plain)[~changed])          # every other element of the step's x0 is what it was
            err, bound = (got.double() - want).abs(), step_bound(gd, x_t, m, mo, t, want)
            log("steered x0 %s n=%d t=%s %s: worst error / bound %.3f" % (mean_type, n, tv, "ddim" if strided else "p_sample",
                                                                           float((err / bound)[changed].max())))
            assert bool((err <= bound)[changed].all()), (mean_type, n, tv, strided, float((err / bound)[changed].max()))


# ------------------------------------------------------------------------------------------------------------------- 5. given parts
@pytest.mark.parametrize("n", [5, 65])
def test_given_elements_are_never_written(n):
    from diffuscene_amd import ops
    x0 = O.make_scenes(n, 0)
    known = O.make_scenes(n, 1).clamp(-1, 1)
    given = torch.rand(x0.shape, generator=torch.Generator().manual_seed(5)) < 0.3
    given[:, 0] = True                                                              # a box given whole ...
    given[:, 1 % n, 0:3] = True                                                     # ... one with its translation given ...
    if n > 2:
        given[:, 2] = False                                                         # ... and a free one
    mask = O.rooms(16, 16, SIDE)
    seen = torch.where(given, known, x0.clamp(-1, 1))                               # the scene the launch sees
    O.assert_margins(seen, mask, SIDE, ("given", n))
    E, g, out = O.energy_grad(seen, mask, SIDE)
    t = torch.zeros(3, dtype=torch.int64, device=dev())
    mo = x0.to(dev()).clone()
    gE, gg, gout = torch.empty(3, device=dev()), torch.empty(3, n, 3, device=dev()), torch.empty(3, device=dev(), dtype=torch.int32)
    wt, kb, bd, fld, rs = walls(W3, mask, SIDE)
    ops.steer_walls(None, mo, wt, kb, bd, fld, rs, MEAN["x0"], class_dim=O.CLASSES, t=t,
                    mask=(known.to(dev()), None, given.to(torch.uint8).to(dev())), energy_out=gE, grad_out=gg, outside_out=gout)
    mo = mo.cpu()
    assert torch.equal(bits(mo)[given], bits(x0)[given])                            # a given element is never written
    assert bool((O.rel_err(gg.cpu(), g, g) <= EPS).all()) and bool((O.rel_err(gE.cpu(), E, E) <= EPS).all())      # it enters with its given value
    assert torch.equal(gout.cpu().long(), out)
    wg = torch.zeros_like(seen, dtype=torch.float64)
    wg[..., 0:3] = W3.double()[:, None, None] * g
    free_moves = (wg != 0) & ~given
    assert bool(free_moves.any()) and bool((mo != x0)[free_moves].any()) and not bool(((mo != x0) & ~free_moves).any())
    want = (seen.double() - wg).clamp(-1, 1)
    assert bool(((mo.double().clamp(-1, 1) - want).abs() <= 2.0 ** -24 * want.abs() + 1e-12)[free_moves].all())


@pytest.mark.parametrize("mean_type", ["x0", "eps"])
def test_a_whole_row_prefix_mask_is_the_rows_form_bit_for_bit(mean_type):
    from diffuscene_amd import ops
    gd = diffusion(mean_type)
    n, pmax, counts = 65, 40, [0, 7, 40]
    x0, known = O.make_scenes(n, 0), O.make_scenes(n, 1).clamp(-1, 1)
    t = torch.tensor([1, 0, 1], dtype=torch.int64)
    x_t, m = chain_inputs(gd, x0, t, 3)
    cnt = torch.tensor(counts, dtype=torch.int64)
    given = (torch.arange(n)[None, :, None] < cnt[:, None, None]).expand(3, n, O.C12).contiguous()
    partial = known[:, :pmax].contiguous().to(dev())
    ca, cb = gd._coeffs(gd.tables(dev()))
    wt, kb, bd, fld, rs = walls(W3, O.rooms(16, 16, SIDE), SIDE)
    outs = []
    for operands in (dict(rows=(partial, None, cnt.to(dev()))), dict(mask=(known.to(dev()), None, given.to(torch.uint8).to(dev())))):
        mo = m.to(dev()).clone()
        E, g, out = torch.empty(3, device=dev()), torch.empty(3, n, 3, device=dev()), torch.empty(3, device=dev(), dtype=torch.int32)
        ops.steer_walls(x_t.to(dev()), mo, wt, kb, bd, fld, rs, MEAN[mean_type], ca, cb, class_dim=O.CLASSES, t=t.to(dev()),
                        energy_out=E, grad_out=g, outside_out=out, **operands)
        outs.append((mo.cpu(), E.cpu(), g.cpu(), out.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    mo = outs[0][0]
    assert bool((mo != m).any()) and torch.equal(bits(mo)[given], bits(m)[given])    # steered, and never inside the given rows
    assert float(outs[0][2][1, :7].abs().max()) > 0                                 # the given boxes enter the energy; they are not moved


# ------------------------------------------------------------------------------------------------------------------- 6. guidance
@pytest.mark.parametrize("mean_type,tv", [("x0", [0, 1, T - 1]), ("eps", [0, 1, 1])])
def test_guided_both_halves_move_by_the_same_delta(mean_type, tv):
    from diffuscene_amd import ops
    gd = diffusion(mean_type)
    n = 65
    t = torch.tensor(tv, dtype=torch.int64)
    x_t, m = chain_inputs(gd, O.make_scenes(n, 0), t, 4)
    spread = 0.02 * torch.randn(m.shape, generator=torch.Generator().manual_seed(9))
    spread[..., O.EMPTY] = 0                                                        # the validity of a box does not hang on the mix
    c, u = m + spread, m - 0.5 * spread
    s = torch.tensor([0.0, 1.0, 2.5])
    ca, cb = gd._coeffs(gd.tables(dev()))
    xd, td, sd = x_t.to(dev()), t.to(dev()), s.to(dev())
    mask = O.rooms(16, 16, SIDE)
    wt, kb, bd, fld, rs = walls(W3, mask, SIDE)
    mix = ops.cfg_combine(torch.cat([c, u]).to(dev()), sd)                          # m = u + s (c - u) as the step forms it
    O.assert_margins(step_x0(gd, xd, mix, td, False).cpu(), mask, SIDE, ("guided", mean_type))
    mo2 = torch.cat([c, u]).to(dev())
    ops.steer_walls(xd, mo2, wt, kb, bd, fld, rs, MEAN[mean_type], ca, cb, class_dim=O.CLASSES, t=td, scale=sd)
    mB = mix.clone()
    ops.steer_walls(xd, mB, wt, kb, bd, fld, rs, MEAN[mean_type], ca, cb, class_dim=O.CLASSES, t=td)
    dc, du = mo2[:3].cpu() - c, mo2[3:].cpu() - u
    delta = mB.cpu().double() - mix.cpu().double()                                  # what the unguided launch added to the mix
    assert bool((dc != 0).any()) and torch.equal(dc != 0, du != 0)
    assert not bool((dc != 0)[..., 1].any()) and not bool((dc != 0)[..., 3:].any())
    # the same delta up to the rounding of the three stores (half an ulp of c', u' and m' each, and of the float32 differences above)
    ulp = 2.0 ** -22 * torch.maximum(torch.maximum(c.abs(), u.abs()), mix.cpu().abs()).double().clamp(min=float(delta.abs().max()))
    assert bool(((dc.double() - delta).abs() <= ulp).all()) and bool(((du.double() - delta).abs() <= ulp).all())


# ------------------------------------------------------------------------------------------------------------------- 7. batch independence
@pytest.mark.parametrize("n", [5, 160])
def test_scene_b_alone_is_scene_b_of_the_batch_and_a_shared_mask_is_the_expanded_one(n):
    from diffuscene_amd import ops
    gd = diffusion("v")
    x0 = O.make_scenes(n, 1)
    t = torch.tensor([1, 0, 5], dtype=torch.int64)
    x_t, m = chain_inputs(gd, x0, t, 6)
    ca, cb = gd._coeffs(gd.tables(dev()))
    rooms3 = O.rooms(16, 16, SIDE)

    def run(sl, mask):
        mo = m[sl].to(dev()).clone()
        b = mo.shape[0]
        E, g, out = torch.empty(b, device=dev()), torch.empty(b, n, 3, device=dev()), torch.empty(b, device=dev(), dtype=torch.int32)
        wt, kb, bd, fld, rs = walls(W3[sl], mask, SIDE)
        ops.steer_walls(x_t[sl].to(dev()), mo, wt, kb, bd, fld, rs, MEAN["v"], ca, cb, class_dim=O.CLASSES, t=t[sl].to(dev()),
                        energy_out=E, grad_out=g, outside_out=out)
        return mo.cpu(), E.cpu(), g.cpu(), out.cpu()
    batch = run(slice(0, 3), rooms3)
    assert bool((batch[0] != m).any())
    for b in range(3):
        for whole, alone in zip(batch, run(slice(b, b + 1), rooms3[b:b + 1])):
            assert torch.equal(whole[b:b + 1], alone), (n, b)
    shared = run(slice(0, 3), rooms3[:1])                                           # (1, 1, H, W): one field for every scene
    for a, b in zip(shared, run(slice(0, 3), rooms3[:1].expand(3, 1, 16, 16).contiguous())):
        assert torch.equal(a, b)
    assert not torch.equal(shared[0], batch[0])


# ------------------------------------------------------------------------------------------------------------------- 8. effect
@pytest.mark.parametrize("n", [5, 65, 160])
def test_the_last_step_does_not_raise_the_energy(n):
    """t = 0 (the x0 the posterior step forms) and the last strided pair (its output is x0'), w = 0.05: E(x0') <= E(x0) for every scene,
    < for at least one -- on inputs for which the float64 oracle's own step x0 - w g does the same, asserted first."""
    from diffuscene_amd import ops
    gd = diffusion("x0")
    w = torch.full((3,), 0.05)
    t = torch.zeros(3, dtype=torch.int64, device=dev())
    for seed in SEEDS:
        for h, wd, side in ((64, 64, 3.1), (16, 16, 2.0)):
            x0, mask, E0, _, _ = O.case(n, seed, h, wd, side)
            E64 = O.energy_grad(O.step(x0, mask, side, w), mask, side)[0]
            assert bool((E64 <= E0).all()) and bool((E64 < E0).any()), (n, seed, "the oracle's own step")
            xd = x0.to(dev())
            wt, kb, bd, fld, rs = walls(w, mask, side)
            mo = xd.clone()
            ops.steer_walls(None, mo, wt, kb, bd, fld, rs, MEAN["x0"], class_dim=O.CLASSES, t=t)
            x0_out = step_x0(gd, xd, mo, t, False).cpu()
            mo2 = xd.clone()                                                        # the last strided pair reads the same t
            ops.steer_walls(None, mo2, wt, kb, bd, fld, rs, MEAN["x0"], class_dim=O.CLASSES, strided=one_pair(t))
            assert torch.equal(mo2, mo)
            tb = gd.tables(dev())
            last = ops.ddim_step(xd, mo2, xd, *one_pair(t), None, None, tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"],
                                 MEAN["x0"]).cpu()
            assert torch.equal(last, x0_out)
            E1 = O.energy_grad(x0_out, mask, side)[0]
            log("effect n=%d seed=%d %dx%d s=%.1f: E(x0') / E(x0) = %s" % (n, seed, h, wd, side, ["%.4f" % (float(a) / float(b)) for a, b in zip(E1, E0)]))
            assert bool((E1 <= E0).all()) and bool((E1 < E0).any()), (n, seed, E1.tolist(), E0.tolist())


# ------------------------------------------------------------------------------------------------------------------- 9. the loops
def loop_rooms(flip=False):
    """(LB, 1, 16, 16) on the device: small rooms, so that the boxes of the seeded model reach outside them."""
    m = torch.stack([O.room("pixel", 16, 16, SIDE), O.room("rect", 16, 16, SIDE)])[:, None]
    return (m.flip(0) if flip else m).contiguous().to(dev())


def graph_of(dp):
    assert len(dp.diffusion._graphs) == 1
    return next(iter(dp.diffusion._graphs.values()))


def sample(dp, cond, strided, graph, seed=3, **kw):
    torch.manual_seed(seed)
    with torch.no_grad(), QUIET():
        if strided:
            return dp.gen_samples_ddim((LB, LN, 62), dev(), condition=cond, sampling_timesteps=4, ddim_sampling_eta=0.5, graph=graph, **kw)
        return dp.gen_samples((LB, LN, 62), dev(), condition=cond, clip_denoised=True, graph=graph, **kw)


@pytest.mark.parametrize("strided,mean_type", [(False, "v"), (True, "eps")])
def test_loops_eager_is_captured_and_inactive_is_unsteered(strided, mean_type, tmp_path_factory):
    dp, cond = model(mean_type, tmp_path_factory)
    plain = sample(dp, cond, strided, True)
    assert torch.equal(plain, sample(dp, cond, strided, False))
    on = dict(wall_scale=[0.05, 0.02], room_side=SIDE, room_mask=loop_rooms())
    eager = sample(dp, cond, strided, False, **on)
    captured = sample(dp, cond, strided, True, **on)
    assert torch.equal(eager, captured)
    log("loop %s: floor-plan steering moved the scenes by %.3g (max abs)" % ("ddim" if strided else "ddpm", float((captured - plain).abs().max())))
    assert not torch.equal(captured, plain)
    g = graph_of(dp)
    assert g.walls is not None and g.steer is None
    # one graph, replayed with another mask, other weights, another K and another room side: no re-capture
    other = dict(wall_scale=[0.0, 0.1], wall_steps=6 if strided else 7, room_side=2.0, room_mask=loop_rooms(flip=True))
    captured2 = sample(dp, cond, strided, True, **other)
    assert graph_of(dp) is g
    assert torch.equal(captured2, sample(dp, cond, strided, False, **other))
    assert not torch.equal(captured2, captured) and not torch.equal(captured2, plain)
    assert torch.equal(captured2[0], plain[0])                                      # weight 0 in a mixed batch: the unsteered scene
    shared = dict(on, room_mask=loop_rooms()[1:])                                   # a shared (1, 1, H, W) mask on the same graph
    assert torch.equal(sample(dp, cond, strided, True, **shared), sample(dp, cond, strided, False, **shared)) and graph_of(dp) is g
    for off in (dict(on, wall_scale=0.0), dict(on, wall_steps=0)):
        assert torch.equal(sample(dp, cond, strided, True, **off), plain)
        assert torch.equal(sample(dp, cond, strided, False, **off), plain)
    assert graph_of(dp) is g
    assert torch.equal(sample(dp, cond, strided, True), plain)                      # without the keyword the unsteered graph is built, as before
    assert graph_of(dp).walls is None


@pytest.mark.parametrize("kind", ["ragged", "ragged-ddim", "masked", "masked-ddim", "guided", "guided-ddim", "collision", "solver-seeded"])
def test_the_other_rows_eager_is_captured(kind, tmp_path_factory):
    """Ragged, masked and guided rows, collision_scale + wall_scale, and wall_scale + dpmpp_2m + per-scene seeds: eager == captured
    (torch.equal), the launch moves the scenes, and with weight 0 the loop is the one without the keyword."""
    from diffuscene_amd import ops
    from diffuscene_amd.scene_noise import SceneNoise
    shape = (LB, LN, 62)
    strided = dict(sampling_timesteps=4, ddim_sampling_eta=0.0 if kind == "solver-seeded" else 0.5) if kind.endswith(("ddim", "seeded")) else {}
    known = _given_scene(11)
    given = torch.zeros(shape, dtype=torch.bool, device=dev())
    given[:, :2] = True
    given[:, 2, 3:] = True                                                          # a box whose translation is free, everything else given
    extra = {}
    if "guided" in kind:
        dp, cond, cross = _text_model(tmp_path_factory)
        kw = dict(condition=cond, condition_cross=cross, guidance_scale=[1.5, 0.5])
        call = dp.gen_samples_guided_ddim if strided else dp.gen_samples_guided
    else:
        dp, cond = model("eps" if strided else "v", tmp_path_factory)
        kw = dict(condition=cond)
        if kind.startswith("ragged"):
            call = dp.complete_samples_ragged_ddim if strided else dp.complete_samples_ragged
            kw.update(partial_boxes=known[:, :3].contiguous(), num_partial=[3, 1])
        elif kind.startswith("masked"):
            call = dp.inpaint_samples_ddim if strided else dp.inpaint_samples
            kw.update(known=known, mask=given)
        elif kind == "collision":
            call, extra = dp.gen_samples, dict(collision_scale=[0.2, 0.1])
        else:
            call, extra = dp.gen_samples_ddim, dict(sampling_solver="dpmpp_2m")

    def run(graph, **more):
        torch.manual_seed(5)
        seeded = dict(noise_fn=SceneNoise(ops.scene_seeds([5, 6], LB, dev()), dev())) if kind == "solver-seeded" else {}
        with torch.no_grad(), QUIET():
            return call(shape, dev(), graph=graph, **kw, **strided, **extra, **seeded, **more)
    plain = run(True)
    on = dict(wall_scale=[0.05, 0.1], room_side=SIDE, room_mask=loop_rooms())
    eager, captured = run(False, **on), run(True, **on)
    assert torch.equal(eager, captured), kind
    g = graph_of(dp)
    assert g.walls is not None and (g.steer is not None) == (kind == "collision") and (g.multistep is not None) == (kind == "solver-seeded")
    moved = [float((captured[b] - plain[b]).abs().max()) for b in range(LB)]
    log("loop %s: floor-plan steering moved the scenes by %s" % (kind, moved))
    assert max(moved) > 0, kind
    assert torch.equal(run(True, **dict(on, wall_scale=0.0)), plain) and torch.equal(run(False, **dict(on, wall_steps=0)), plain)
    if kind.startswith("masked"):
        assert torch.equal(captured[given], known[given])                          # the given elements come back as they were given
    if kind.startswith("ragged"):
        assert torch.equal(captured[0, :3], known[0, :3]) and torch.equal(captured[1, :1], known[1, :1])


# ------------------------------------------------------------------------------------------------------------------- 10. statistics
def test_out_of_room_is_the_oracle():
    from diffuscene_amd import scene_stats
    for n, (h, w, side) in ((5, O.ROOMS[0]), (65, O.ROOMS[2]), (160, O.ROOMS[3])):
        x, mask, E, _, out = O.case(n, 0, h, w, side)
        energy, share = scene_stats.out_of_room(x, mask, side, O.BOUNDS, class_dim=O.CLASSES)
        kept = (x[..., O.EMPTY] < 0).sum(dim=1)
        assert bool((O.rel_err(energy.cpu(), E, E) <= EPS).all())
        assert torch.equal(share.cpu(), out.float() / kept.clamp(min=1).float()) and float(share.max()) <= 1.0
        log("out_of_room n=%d %dx%d s=%.1f: energy %s, share %s" % (n, h, w, side, ["%.4f" % v for v in energy.tolist()], ["%.3f" % v for v in share.tolist()]))
    energy, share = scene_stats.out_of_room(x.numpy(), mask[:1].numpy(), side, O.BOUNDS, class_dim=O.CLASSES)      # numpy in, a shared mask
    assert energy.shape == (3,) and share.shape == (3,)
