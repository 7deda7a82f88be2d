"""GPU: resampling jumps (RePaint) on the completion and in-painting loops.

* kernels: dsc_resample_jump_f32 in every instantiation (posterior / strided x rows / mask / none, with and without x_dup) against the
  composition it replaces -- dsc_q_sample_f32 on the tables (ja, jb) at t = s, then the matching overwrite at the target time --
  torch.equal, with NaN in every operand a lane must not read and canaries around the output; dsc_ddim_seek_i64;
* no-op schedules (r == 1, j >= U) are the call without the keyword, bit for bit, generator state included;
* the captured loops are the eager loops bit for bit in the three noise modes, fused and unfused, and leave the same generator state;
  one graph set serves every (r, K) and every mask;
* given elements come back bit-equal;
* reference chains: tests/golden/resample.npz against ONE batched captured call on the same draws, under both GEMM arithmetics;
* the effect: the analytic toy of tests/test_resample_host.py through the real eager kernels."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import weights as W  # noqa: E402

from test_gpu_cfg import QUIET, _conditions, build_model  # noqa: E402
from test_gpu_complete_ragged import build_net, build_wrapper, dev, padded_partial, rnd  # noqa: E402
from tools.make_golden_guided_inpaint import case_texts  # noqa: E402

NAN = float("nan")
T_MODEL, S_LOOP = 50, 8
RES_T, RES_S = (5, 3), (2, 3)


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


def _gd(T=1000, mean="v"):
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    return GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, T),
                             "mse", mean, "fixedsmall", False, False, None)


# ------------------------------------------------------------------------------------------------------------------- kernels
SHAPES = ((3, 12, 62), (2, 21, 65), (1, 1, 5), (2, 80, 65))          # inner 744 / 1365 (off the 16-byte grid) / 5 / 5200 (several blocks)
PAD = 64


def _framed(x):
    """A copy of ``x`` inside a larger allocation with canary values on both sides -> (the view, the whole buffer)."""
    buf = torch.full((x.numel() + 2 * PAD,), 12345.0, device=x.device)
    view = buf[PAD:PAD + x.numel()].view(x.shape)
    view.copy_(x)
    return view, buf


def _canaries_intact(buf):
    return bool((buf[:PAD] == 12345.0).all()) and bool((buf[-PAD:] == 12345.0).all())


def _given_parts(shape):
    """name -> (kind, given bool (B, N, C), the operands of ops.jump_rec without the draw)."""
    B, N, C = shape
    g = torch.Generator().manual_seed(3)
    out = {"none": (None, torch.zeros(shape, dtype=torch.bool), None)}
    masks = {"free": torch.zeros(shape, dtype=torch.uint8), "given": torch.full(shape, 255, dtype=torch.uint8),
             "30%": torch.where(torch.rand(shape, generator=g) < 0.3, torch.randint(1, 256, shape, generator=g), torch.zeros((), dtype=torch.int64)).to(torch.uint8)}
    for name, m in masks.items():
        out["mask " + name] = ("mask", m != 0, m.to(dev()))
    for pmax in sorted({N, max(1, N // 2)}):
        counts = [(0, pmax, pmax // 2)[b % 3] for b in range(B)]
        given = (torch.arange(N)[None, :] < torch.tensor(counts)[:, None])[:, :, None].expand(shape)
        out["rows pmax %d" % pmax] = ("rows", given, (pmax, torch.tensor(counts, dtype=torch.int64, device=dev())))
    return out


def _poison(t, where):
    return torch.where(where, torch.full_like(t, NAN), t)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("strided", [False, True])
def test_jump_kernel_is_q_sample_then_the_overwrite(strided, shape):
    from diffuscene_amd import ops
    B, N, C = shape
    gd = _gd()
    tb = gd.tables(dev())
    q = (tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"])
    T, S, j = 1000, 20, (10 if not strided else 4)
    ja, jb = gd.jump_table(j, dev(), S if strided else None)
    dtab = gd.ddim_tables(S, 0.0, dev())
    times = dtab[1]
    x0, noise = rnd(*shape, seed=900).to(dev()), rnd(*shape, seed=901).to(dev())
    positions = (j, S // 2, S - 1) if strided else (0, 417, T - 1 - j)        # the first and last jumpable counter / s = 0 ... the largest
    for pos in positions:
        if strided:
            step = torch.tensor([pos], dtype=torch.int64, device=dev())
            src = dict(strided=(step, times))
            t_pos = torch.full((B,), pos, dtype=torch.int64, device=dev())     # q_sample indexes the S-row tables by the counter
            t_target = torch.full((B,), int(times[pos - j]), dtype=torch.int64, device=dev())
        else:
            t_pos = torch.tensor([(pos, max(pos - 1, 0), 0)[b % 3] if pos else 0 for b in range(B)], dtype=torch.int64, device=dev())
            src = dict(t=t_pos)
            t_target = t_pos + j
        jumped = ops.q_sample(x0, noise, t_pos, ja, jb)
        for name, (kind, given, extra) in _given_parts(shape).items():
            gdev = given.to(dev())
            for dup in (False, True):
                x, frame = _framed(x0)
                xd, dframe = _framed(torch.zeros_like(x0)) if dup else (None, None)
                kw = dict(src, x_dup=xd) if dup else dict(src)
                if kind is None:
                    want = jumped
                    ops.resample_jump(x, _poison(noise, gdev), ja, jb, j, **kw)
                elif kind == "mask":
                    known, nk = rnd(*shape, seed=902).to(dev()), rnd(*shape, seed=903).to(dev())
                    want = ops.masked_overwrite(jumped.clone(), known, nk, extra, t_target, *q)
                    # NaN wherever a lane must not read: x and the jump draw under the mask, known and its draw outside it
                    x.copy_(_poison(x0, gdev))
                    ops.resample_jump(x, _poison(noise, gdev), ja, jb, j, mask=(_poison(known, ~gdev), _poison(nk, ~gdev), extra), q=q, **kw)
                else:
                    pmax, counts = extra
                    part, pn = rnd(B, pmax, C, seed=904).to(dev()), rnd(B, pmax, C, seed=905).to(dev())
                    want = ops.complete_overwrite_ragged(jumped.clone(), part, pn, counts, t_target, *q)
                    gp = gdev[:, :pmax]
                    x.copy_(_poison(x0, gdev))
                    ops.resample_jump(x, _poison(noise, gdev), ja, jb, j, rows=(_poison(part, ~gp), _poison(pn, ~gp), counts), q=q, **kw)
                assert torch.isfinite(x).all() and torch.equal(x, want), (strided, shape, pos, name, dup)
                assert _canaries_intact(frame), (strided, shape, pos, name)
                if dup:
                    assert torch.equal(xd, want) and _canaries_intact(dframe), (strided, shape, pos, name)
                if kind is not None and not given.any():
                    assert torch.equal(x, jumped)                              # nothing given: the plain jump


def test_jump_refuses_bad_operand_groups_and_counts_bad_indices():
    from diffuscene_amd import _lib, ops
    gd = _gd()
    tb = gd.tables(dev())
    q = (tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"])
    shape = (3, 21, 65)
    x, noise, known = rnd(*shape, seed=910).to(dev()), rnd(*shape, seed=911).to(dev()), rnd(*shape, seed=912).to(dev())
    mask = torch.ones(shape, dtype=torch.uint8, device=dev())
    ja, jb = gd.jump_table(10, dev())
    t = torch.tensor([0, 5, 989], dtype=torch.int64, device=dev())
    step = torch.zeros(1, dtype=torch.int64, device=dev())
    for bad in (dict(), dict(t=t, strided=(step, t)), dict(t=t, mask=(known, noise, mask)), dict(t=t, q=q),
                dict(t=t, mask=(known, noise, mask), rows=(known, noise, t), q=q)):
        with pytest.raises(ValueError):
            ops.jump_rec(x, noise, ja, jb, 10, **bad)
    with pytest.raises(ValueError):
        ops.jump_rec(x, noise, ja, jb, 0, t=t)
    # t = 995: the position is in range, the target 1005 is not -- counted once for that scene, and only where a given part looks it up
    t_bad = torch.tensor([0, 995, 1003], dtype=torch.int64, device=dev())
    y = x.clone()
    ops.resample_jump(y, noise, ja, jb, 10, t=t_bad)
    assert _lib.device_error_count(reset=True) == 1
    ops.resample_jump(y, noise, ja, jb, 10, t=t_bad, mask=(known, noise, mask), q=q)
    assert _lib.device_error_count(reset=True) == 3
    assert torch.equal(y[1], ops.q_sample(known, noise, torch.full((3,), 999, dtype=torch.int64, device=dev()), *q)[1])      # clamped


@pytest.mark.parametrize("count", [1, 6, 600])
def test_ddim_seek_moves_the_counter_and_fills_t(count):
    from diffuscene_amd import _lib, ops
    times = torch.tensor([999, 856, 713, 570, 427, 284, 141], dtype=torch.int64, device=dev())
    step = torch.tensor([5], dtype=torch.int64, device=dev())
    t = torch.full((count,), -7, dtype=torch.int64, device=dev())
    assert ops.ddim_seek(step, times, t, -2) is t
    assert int(step) == 3 and bool((t == 570).all())
    ops.ddim_seek(step, times, t, 3)
    assert int(step) == 6 and bool((t == 141).all())
    ops.ddim_seek(step, times, t, -9)                                              # out of range: clamped and counted once
    assert int(step) == 0 and bool((t == 999).all()) and _lib.device_error_count(reset=True) == 1


# ------------------------------------------------------------------------------------------------------------------- the loops
_SHARED = {}


def _bedroom(N):
    """(DiffusionPoint at T = 50, shape, condition, scenes, a (B, N, C) bool mask) of the bedroom network at B = 3."""
    if N not in _SHARED:
        B, C = 3, 62
        cond = W.synth_condition(B, N, 128, 5, shared=True).contiguous().to(dev())
        x = W.synth_scene_batch(B, N, 22, 32, 5)
        mask = torch.zeros((B, N, C), dtype=torch.bool)
        mask[0, :4] = True                     # whole rows [0, 4)
        mask[1, :, 3:6] = True                 # sizes + classes of all rows
        mask[1, :, 8:30] = True
        mask[2] = torch.rand((N, C), generator=torch.Generator().manual_seed(4)) < 0.1          # scattered single elements
        _SHARED[N] = ((B, N, C), cond, x, mask)
    return (build_net(W.UNCOND_BEDROOM, "v")[1],) + _SHARED[N]


COUNTS = (0, 3, 5)


def _loop_calls(N):
    """name -> (call(graph=, noise_fn=, **resample keywords), the given bool mask, the clean values, U of the loop)."""
    diff, shape, cond, x, mask = _bedroom(N)
    B = shape[0]
    part = padded_partial(x, COUNTS)[:, :6].contiguous()
    rows = (torch.arange(N)[None, :] < torch.tensor(COUNTS)[:, None])[:, :, None].expand(shape)
    dense = torch.zeros(shape, dtype=torch.bool)
    dense[:, :3] = True
    xd = x.to(dev())
    ddim = dict(sampling_timesteps=S_LOOP)
    return {
        "dense": (lambda **kw: diff.complete_samples(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=xd[:, :3].contiguous(), **kw),
                  dense, T_MODEL),
        "ragged": (lambda **kw: diff.complete_samples_ragged(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=part,
                                                             num_partial=list(COUNTS), **kw), rows, T_MODEL),
        "ragged ddim": (lambda eta=0.0, **kw: diff.complete_samples_ragged_ddim(shape, dev(), condition=cond, partial_boxes=part,
                                                                                num_partial=list(COUNTS), ddim_sampling_eta=eta, **ddim, **kw), rows, S_LOOP),
        "masked": (lambda **kw: diff.inpaint_samples(shape, dev(), condition=cond, clip_denoised=True, known=xd, mask=mask, **kw), mask, T_MODEL),
        "masked ddim": (lambda eta=0.0, **kw: diff.inpaint_samples_ddim(shape, dev(), condition=cond, known=xd, mask=mask, ddim_sampling_eta=eta,
                                                                        **ddim, **kw), mask, S_LOOP),
    }, diff, x


def _guided_calls(tmp_path):
    m = build_model("v", T_MODEL, tmp_path)
    if "text" not in _SHARED:
        shape = (3, 12, 62)
        cond, cross = _conditions(m, 3, case_texts())
        x = W.synth_scene_batch(3, 12, 22, 32, 7)
        _SHARED["text"] = (shape, cond, cross, x)
    shape, cond, cross, x = _SHARED["text"]
    mask = _bedroom(12)[4]
    diff, xd = m.diffusion, x.to(dev())
    common = dict(condition=cond, condition_cross=cross, guidance_scale=(0.0, 1.5, 3.0), known=xd, mask=mask)
    return {
        "guided": (lambda **kw: diff.inpaint_samples_guided(shape, dev(), clip_denoised=True, **common, **kw), mask, T_MODEL),
        "guided ddim": (lambda eta=0.0, **kw: diff.inpaint_samples_guided_ddim(shape, dev(), sampling_timesteps=S_LOOP, ddim_sampling_eta=eta,
                                                                               **common, **kw), mask, S_LOOP),
    }, diff, x


def _run(call, seed=2468, **kw):
    torch.manual_seed(seed)
    with torch.no_grad(), QUIET():
        out = call(**kw)
    return out, torch.cuda.get_rng_state(dev())


@pytest.mark.parametrize("graph", [False, True])
def test_schedules_without_a_jump_are_the_call_without_the_keyword(graph, tmp_path):
    calls = dict(_loop_calls(12)[0])
    calls.update(_guided_calls(tmp_path)[0])
    for name, (call, _, U) in calls.items():
        plain, state = _run(call, graph=graph)
        for res in (dict(resample=(3, 1)), dict(resample=(U, 4)), dict(resample=(U + 9, 2)), dict(resample=(2, 3), resample_steps=0)):
            out, after = _run(call, graph=graph, **res)
            assert torch.equal(out, plain) and torch.equal(after, state), (name, res)


def _replay_buffers(shape, pshape, sched, strided):
    n_main = sched.calls + sched.jumps + (0 if strided else 1)
    main = torch.stack([rnd(*shape, seed=3000 + i) for i in range(n_main)]).to(dev())
    given = torch.stack([rnd(*pshape, seed=6000 + i) for i in range(sched.calls)]).to(dev())
    return main, given


def _check_loop(name, call, given, x, diff, shape, pshape, U, eta=None):
    """captured == eager, bit for bit, in the three noise modes; the same generator state; the given elements bit-equal."""
    from diffuscene_amd import sampler
    from diffuscene_amd.scene_noise import SceneNoise
    strided = eta is not None
    res = dict(resample=RES_S if strided else RES_T)
    kw = dict(res, eta=eta) if strided else res
    gd = diff.diffusion
    sched = gd.resample_schedule(*res["resample"], **(dict(sampling_timesteps=U) if strided else {}))
    assert sched.jumps > 0
    eager, se = _run(call, graph=False, **kw)
    captured, sc = _run(call, graph=True, **kw)
    assert torch.equal(eager, captured) and torch.equal(se, sc), name
    assert torch.isfinite(captured).all() and torch.equal(captured.cpu()[given], x[given]), name
    (g,) = gd._graphs.values()
    assert g.resample is not None and g.jump is not None and (g.prejump is not None) == g.part.fused, name
    plain, _ = _run(call, graph=True, **({"eta": eta} if strided else {}))
    assert not torch.equal(plain, captured), name                                  # the jumps do something
    main, gn = _replay_buffers(shape, pshape, sched, strided)
    er, _ = _run(call, graph=False, noise_fn=sampler.RaggedNoiseReplay(main, gn), **kw)
    gr, _ = _run(call, graph=True, noise_fn=sampler.RaggedNoiseReplay(main, gn), **kw)
    assert torch.equal(er, gr) and not torch.equal(gr, captured), name
    with pytest.raises(ValueError, match="resampling jumps|resampled"):
        _run(call, graph=True, noise_fn=sampler.RaggedNoiseReplay(main[:-1], gn), **kw)
    seeds = [11, 2 ** 40 + 5, 11]
    es, s1 = _run(call, graph=False, noise_fn=SceneNoise(seeds, dev()), **kw)
    gs, s2 = _run(call, graph=True, noise_fn=SceneNoise(seeds, dev()), **kw)
    assert torch.equal(es, gs) and torch.equal(s1, s2), name
    if not given[0].any() and not given[2].any():
        assert torch.equal(gs[0], gs[2])                                           # equal seeds, equal scenes
    return captured


@pytest.mark.parametrize("N", [12, 21])
@pytest.mark.parametrize("name", ["dense", "ragged", "masked"])
def test_captured_tstep_loops_are_the_eager_loops(name, N):
    calls, diff, x = _loop_calls(N)
    call, given, U = calls[name]
    shape = (3, N, 62)
    _check_loop(name, call, given, x, diff, shape, {"dense": (3, 3, 62), "ragged": (3, 6, 62), "masked": shape}[name], U)


@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("N", [12, 21])
@pytest.mark.parametrize("name", ["ragged ddim", "masked ddim"])
def test_captured_strided_loops_are_the_eager_loops(name, N, eta):
    calls, diff, x = _loop_calls(N)
    call, given, U = calls[name]
    shape = (3, N, 62)
    _check_loop(name, call, given, x, diff, shape, (3, 6, 62) if name.startswith("ragged") else shape, U, eta)


@pytest.mark.parametrize("name,eta", [("guided", None), ("guided ddim", 0.0), ("guided ddim", 0.7)])
def test_captured_guided_loops_are_the_eager_loops(name, eta, tmp_path):
    calls, diff, x = _guided_calls(tmp_path)
    call, given, U = calls[name]
    _check_loop(name, call, given, x, diff, (3, 12, 62), (3, 12, 62), U, eta)


def test_unfused_captured_steps_are_the_fused_ones(tmp_path):
    from diffuscene_amd import ops, sampler
    # the ragged overwrite unfused
    calls, diff, x = _loop_calls(12)
    gd = diff.diffusion
    shape, cond = (3, 12, 62), _bedroom(12)[2]
    part = padded_partial(x, COUNTS)[:, :6].contiguous()
    counts = ops.ragged_counts(list(COUNTS), 3, 6, dev())
    for strided in (False, True):
        front = sampler.graph_ddim_complete_ragged_loop if strided else sampler.graph_complete_ragged_loop
        sched_args = (S_LOOP, 0.7) if strided else (True, T_MODEL)
        outs = []
        with torch.no_grad():
            jumps = gd._resample_inputs(dev(), *(RES_S if strided else RES_T), None, *((S_LOOP, 0.7) if strided else (T_MODEL,)))
            main, gn = _replay_buffers(shape, (3, 6, 62), jumps[0], strided)
            for fused in (True, False):
                torch.manual_seed(99)
                outs.append(front(gd, diff._denoise, shape, dev(), cond, None, *sched_args, partial_boxes=part, counts=counts, fused=fused,
                                  jumps=jumps))
                outs.append(torch.cuda.get_rng_state(dev()))
                (g,) = gd._graphs.values()
                assert g.part.fused is fused and (g.prejump is not None) == fused
                outs.append(front(gd, diff._denoise, shape, dev(), cond, None, *sched_args, noise_fn=sampler.RaggedNoiseReplay(main, gn),
                                  partial_boxes=part, counts=counts, fused=fused, jumps=jumps))
        assert torch.equal(outs[0], outs[3]) and torch.equal(outs[1], outs[4]) and torch.equal(outs[2], outs[5]), strided
    # the guidance unfused
    gcalls, gdiff, gx = _guided_calls(tmp_path)
    gd = gdiff.diffusion
    shape, cond, cross, _ = _SHARED["text"]
    mask = _bedroom(12)[4]
    with torch.no_grad():
        cond2, cross2, scale = gd._guided_inputs(shape, dev(), cond, cross, (0.0, 1.5, 3.0), "test")
        kd, mk = gd._masked_inputs(shape, dev(), gx, mask, "test")
        for strided in (False, True):
            front = sampler.graph_ddim_masked_guided_loop if strided else sampler.graph_masked_guided_loop
            sched_args = (S_LOOP, 0.7) if strided else (True, T_MODEL)
            jumps = gd._resample_inputs(dev(), *(RES_S if strided else RES_T), None, *((S_LOOP, 0.7) if strided else (T_MODEL,)))
            outs = []
            for fused in (True, False):
                torch.manual_seed(98)
                outs.append(front(gd, gdiff._denoise, shape, dev(), cond2, cross2, scale, *sched_args, known=kd, mask=mk, fused=fused, jumps=jumps))
                (g,) = gd._graphs.values()
                assert g.fused is fused and (g.m is None) == fused and g.prejump is not None
            assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all(), strided
            eager, _ = _run(gcalls["guided ddim" if strided else "guided"][0], seed=98, graph=False, resample=RES_S if strided else RES_T,
                            **(dict(eta=0.7) if strided else {}))
            assert torch.equal(eager, outs[1])


def test_one_graph_set_serves_every_r_k_and_mask():
    calls, diff, x = _loop_calls(12)
    gd = diff.diffusion
    shape, cond, mask = (3, 12, 62), _bedroom(12)[2], _bedroom(12)[4]
    xd = x.to(dev())
    for strided in (False, True):
        if strided:
            call = lambda **kw: diff.inpaint_samples_ddim(shape, dev(), condition=cond, known=xd, sampling_timesteps=S_LOOP,  # noqa: E731
                                                          ddim_sampling_eta=0.3, **kw)
            settings = (dict(resample=(2, 3)), dict(resample=(2, 2), resample_steps=20))
        else:
            call = lambda **kw: diff.inpaint_samples(shape, dev(), condition=cond, clip_denoised=True, known=xd, **kw)  # noqa: E731
            settings = (dict(resample=(5, 3)), dict(resample=(5, 2), resample_steps=20))
        seen, outs = [], []
        for res, m in zip(settings, (mask, mask.roll(1, 0))):
            out, _ = _run(call, graph=True, mask=m, **res)
            (g,) = gd._graphs.values()
            seen.append((g, g.jump, g.prejump, g.graph, g.final, g.mask.data_ptr(), g.resample.ja.data_ptr()))
            assert len(gd._graphs) == 1
            eager, _ = _run(call, graph=False, mask=m, **res)
            assert torch.equal(out, eager), (strided, res)
            outs.append(out)
        assert all(a is b for a, b in zip(seen[0][:5], seen[1][:5])) and seen[0][5:] == seen[1][5:], strided      # no re-capture
        assert not torch.equal(outs[0], outs[1])
        # another jump length is another graph: j is baked into the launch and the move
        _run(call, graph=True, mask=mask, resample=(3, 2))
        (g2,) = gd._graphs.values()
        assert g2 is not seen[0][0] and g2.resample.j == 3


def test_all_given_returns_the_scene_and_an_empty_mask_runs():
    calls, diff, x = _loop_calls(12)
    shape, cond = (3, 12, 62), _bedroom(12)[2]
    xd = x.to(dev())
    mask = torch.zeros(shape, dtype=torch.bool)
    mask[1] = True                                                                 # scene 0 and 2: nothing given; scene 1: everything
    for graph in (False, True):
        out, _ = _run(lambda **kw: diff.inpaint_samples(shape, dev(), condition=cond, clip_denoised=True, known=xd, mask=mask, **kw),
                      graph=graph, resample=RES_T)
        assert torch.equal(out[1], xd[1]) and torch.isfinite(out).all() and not torch.equal(out[0], xd[0])
        out, _ = _run(lambda **kw: diff.inpaint_samples_ddim(shape, dev(), condition=cond, known=xd, mask=mask, sampling_timesteps=S_LOOP, **kw),
                      graph=graph, resample=RES_S)
        assert torch.equal(out[1], xd[1]) and torch.isfinite(out).all()
        part = xd.contiguous()
        out, _ = _run(lambda **kw: diff.complete_samples_ragged(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=part,
                                                                num_partial=[0, 12, 5], **kw), graph=graph, resample=RES_T)
        assert torch.equal(out[1], xd[1]) and torch.equal(out[2, :5], xd[2, :5]) and torch.isfinite(out).all()


def test_steering_runs_at_every_model_call_of_a_resampled_loop(tmp_path):
    m = build_model("v", T_MODEL, tmp_path)
    gcalls, gdiff, gx = _guided_calls(tmp_path)
    shape, cond, cross, _ = _SHARED["text"]
    mask = _bedroom(12)[4]
    xd = gx.to(dev())
    room = torch.zeros(3, 1, 16, 16, device=dev())
    room[:, :, 5:11, 5:11] = 1.0
    steer = dict(collision_scale=[0.05, 0.0, 0.1], wall_scale=0.05, room_side=3.1, room_mask=room)
    call = lambda **kw: gdiff.inpaint_samples(shape, dev(), condition=cond, condition_cross=cross, clip_denoised=True, known=xd, mask=mask, **kw)  # noqa: E731
    eager, se = _run(call, graph=False, resample=RES_T, **steer)
    captured, sc = _run(call, graph=True, resample=RES_T, **steer)
    assert torch.equal(eager, captured) and torch.equal(se, sc)
    (g,) = gdiff.diffusion._graphs.values()
    assert g.steer is not None and g.walls is not None and g.resample is not None
    unsteered, _ = _run(call, graph=True, resample=RES_T)
    assert not torch.equal(unsteered, captured) and torch.equal(captured.cpu()[mask], gx[mask])


def test_scene_level_calls_take_the_keyword(tmp_path):
    m = build_model("v", T_MODEL, tmp_path)
    B, N, C = 3, 12, 62
    x = W.synth_scene_batch(B, N, 22, 32, 9).to(dev())
    mask = _bedroom(12)[4]
    room = torch.zeros(B, 1, 64, 64, device=dev())
    for kw in (dict(clip_denoised=True), dict(sampling_timesteps=S_LOOP, ddim_sampling_eta=0.5)):
        res = RES_S if "sampling_timesteps" in kw else RES_T
        outs = []
        for extra in ({}, dict(resample=res), dict(resample=(res[0], 1))):
            torch.manual_seed(5)
            with torch.no_grad(), QUIET():
                outs.append(m.inpaint_scene_batched(room, N, C, x, mask, text=case_texts(), guidance_scale=2.0, keep_empty=True, **kw, **extra))
        same = lambda a, b: all(torch.equal(a[i][k], b[i][k]) for i in range(B) for k in a[i])  # noqa: E731
        assert same(outs[0], outs[2]) and not same(outs[0], outs[1])
    plain_model, _ = build_wrapper("uncond", tmp_path)
    for kw in (dict(clip_denoised=True), dict(sampling_timesteps=S_LOOP, ddim_sampling_eta=0.5)):
        torch.manual_seed(5)
        with torch.no_grad(), QUIET():
            done = plain_model.complete_scene_batched(room, N, C, [x[0, :2], x[1, :0], x[2, :5]], keep_empty=True,
                                                      resample=RES_S if "sampling_timesteps" in kw else RES_T, **kw)
        assert len(done) == B and all(torch.isfinite(v).all() for d in done for v in d.values())


# ------------------------------------------------------------------------------------------------------------------- the effect
def test_toy_through_the_eager_kernels():
    """The 2-D toy of tests/test_resample_host.py through the real eager loop: mean type x0, T = 200, unclipped, the analytic denoiser as
    a Python denoise_fn (which keeps the loop eager), channel 0 given at 0.8 by a mask.  B * N = 4096 rows: standard error 0.0035."""
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    B, N, C, T = 64, 64, 2, 200
    gd = GaussianDiffusion(dict(objectness_dim=0, class_dim=1, angle_dim=1, objfeat_dim=0), get_betas("linear", 1e-4, 0.02, T),
                           "mse", "x0", "fixedsmall", False, False, None)
    ac = np.cumprod(1.0 - gd.np_betas)
    sig = 0.25 * np.array([[1.0, 0.9], [0.9, 1.0]])
    den = np.stack([np.sqrt(ac[t]) * sig @ np.linalg.inv(ac[t] * sig + (1 - ac[t]) * np.eye(2)) for t in range(T)])
    den = torch.from_numpy(den).float().to(dev())                                  # (T, 2, 2)

    def denoise(x, t, condition, condition_cross):
        return torch.einsum("bij,bnj->bni", den[t], x).contiguous()

    known = torch.zeros((B, N, C), device=dev())
    known[:, :, 0] = 0.8
    mask = torch.zeros((B, N, C), dtype=torch.bool)
    mask[:, :, 0] = True
    means = []
    for res in ({}, dict(resample=(5, 5))):
        torch.manual_seed(0)
        with torch.no_grad():
            out = gd.p_sample_loop_masked(denoise, (B, N, C), dev(), None, None, clip_denoised=False, known=known, mask=mask, **res)
        assert bool((out[:, :, 0] == 0.8).all())
        means.append(float(out[:, :, 1].double().mean()))
    log("resample toy (eager kernels, 4096 rows): channel 1 mean %.4f plain, %.4f with resample=(5, 5); conditional mean 0.72" % tuple(means))
    assert abs(means[0] - 0.72) >= 0.15
    assert abs(means[1] - 0.72) <= 0.08


# ------------------------------------------------------------------------------------------------------------------- golden chains
from tools import make_golden_resample as G  # noqa: E402
from tools.make_golden_cfg import distance  # noqa: E402

BOTH = pytest.mark.parametrize("gemm_arith", ["split", "f32"], indirect=True)
_GOLDEN_MODELS = {}


def _golden_model(name, tmp_path):
    """(DiffusionPoint, condition, condition_cross or None) of a golden case: the seeded wrapper at the case's T and mean type."""
    case, mt, T = G.CASES[name][:3]
    if case == "text":
        m = build_model(mt, T, tmp_path)
        cond, cross = _conditions(m, G.B, G.case_texts())
        return m.diffusion, cond, cross
    if (mt, T) not in _GOLDEN_MODELS:
        import contextlib
        import io
        import json
        from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
        from oracle.make_golden_wrapper import network_config, wrapper_state_dict
        stats = tmp_path / "dataset_stats.txt"
        stats.write_text(json.dumps(W.DATASET_STATS))
        cfg = network_config("uncond", str(stats), T)
        cfg["diffusion_kwargs"]["model_mean_type"] = mt
        with contextlib.redirect_stdout(io.StringIO()):
            m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
        m.load_state_dict(wrapper_state_dict(m))
        _GOLDEN_MODELS[(mt, T)] = m.to(dev()).eval()
    m = _GOLDEN_MODELS[(mt, T)]
    with torch.no_grad():
        cond = m._base_condition(None, G.B, G.N, dev()).contiguous()
    return m.diffusion, cond, None


@BOTH
@pytest.mark.parametrize("name", list(G.CASES))
def test_resampled_chain_matches_the_reference_within_four_times_its_sensitivity(name, golden_dir, tmp_path, gemm_arith):
    """One batched captured call on the fixture's draws against the REAL reference's chains run scene by scene (tests/golden/resample.npz).
    Bound per chain: the project's chain criterion (5e-6 norm-relative, 1e-4 element-wise: tests/test_gpu_masked.py) or 4 x the chain's
    recorded float32 / float64 sensitivity, whichever is larger -- the rule of tests/test_gpu_cfg.py."""
    from diffuscene_amd.sampler import RaggedNoiseReplay
    g = np.load(os.path.join(golden_dir, "resample.npz"))
    case, mt, T, S, eta, clip, jr, K, kind, seed = G.CASES[name]
    known, mask, main, gn = G.chain_inputs(name)
    diff, cond, cross = _golden_model(name, tmp_path)
    shape = (G.B, G.N, G.C)
    common = dict(condition=cond, condition_cross=cross, noise_fn=RaggedNoiseReplay(main.to(dev()), gn.to(dev())), graph=True, resample=jr,
                  resample_steps=K)
    strided = {} if S is None else dict(sampling_timesteps=S, ddim_sampling_eta=eta)
    with torch.no_grad(), QUIET():
        if kind == "rows":
            y = diff.complete_samples_ragged(shape, dev(), clip_denoised=clip, partial_boxes=known[:, :G.PMAX].contiguous().to(dev()),
                                             num_partial=list(G.COUNTS), **common)
        elif case == "text":
            y = diff.inpaint_samples_guided(shape, dev(), clip_denoised=clip, guidance_scale=G.SCALES, known=known.to(dev()), mask=mask, **common)
        elif S is None:
            y = diff.inpaint_samples(shape, dev(), clip_denoised=clip, known=known.to(dev()), mask=mask, **common)
        else:
            y = diff.inpaint_samples_ddim(shape, dev(), known=known.to(dev()), mask=mask, **strided, **common)
    assert torch.equal(y.cpu()[mask], known[mask])                   # the given elements come back bit-equal
    r, ew = distance(y.cpu(), g[name])
    sr, sew = (float(v) for v in g[name + ".sens"])
    br, bew = max(5e-6, 4 * sr), max(1e-4, 4 * sew)
    line = "resampled %s %s: norm-relative %.3g (bound %.3g), element-wise %.3g (bound %.3g)" % (name, gemm_arith, r, br, ew, bew)
    log(line)
    assert r < br and ew < bew, line
