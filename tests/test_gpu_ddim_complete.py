"""GPU: strided (DDIM) scene completion with per-scene counts (ddim_complete_ragged_loop), strided re-arrangement (ddim_arrange_loop) and
the scene-level entry points over them.

* kernel: dsc_ddim_inpaint_step_f32 against the composition of the kernels it fuses (ddim_step, then the ragged overwrite at t_next or the
  restore), bit for bit; out-of-range device values clamped and counted;
* degenerate counts: all 0 is gen_samples_ddim on the main draws, all N returns the given scenes;
* reference chains: tests/golden/ddim_complete.npz (tools/make_golden_ddim_complete.py: the REAL reference's ddim_sample_loop once per scene
  at B = 1, with the in-place overwrite bridged in front of its model call) against ONE batched call on the same noise, under both GEMM
  arithmetics, eager and graph, with the project's ``check`` at 1e-4 (tests/test_gpu_wide.py, as tests/test_gpu_ddim.py and
  tests/test_gpu_complete_ragged.py apply it to the same kind of chain);
* the captured loop: bit-identical to the eager one under torch.manual_seed across two calls, one graph for every eta and mix of counts,
  re-capture on a change of S, interleaving with the other loops, S = 1;
* complete_scene_batched / arrange_scene_batched with ``sampling_timesteps`` against the reference's per-scene dicts."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import weights as W  # noqa: E402
from tools.make_golden_ddim_complete import CASES, T, ddim_complete_inputs  # noqa: E402

from test_gpu_wide import check, dev  # noqa: E402
from test_gpu_complete_ragged import _inject, build_wrapper, padded_partial, rnd  # noqa: E402

BOTH = pytest.mark.parametrize("gemm_arith", ["split", "f32"], indirect=True)
QUIET = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731


@pytest.fixture(autouse=True)
def no_device_errors():
    """dsc_device_error_count is 0 after every test of this file (the one that provokes clamps counts and resets them itself)."""
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    yield
    assert _lib.device_error_count(reset=True) == 0


def _diffusion(mean_type="v", T_=1000):
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    return GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, T_),
                             "mse", mean_type, "fixedsmall", False, False, None)


# ------------------------------------------------------------------------------------------------------------------- kernel
def _step_args(gd, dtab):
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    _, times, times_next, coef = dtab
    return (times, times_next, coef, ca, cb, tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"], tb["sqrt_alphas_cumprod"],
            tb["sqrt_one_minus_alphas_cumprod"], {"eps": 0, "x0": 1, "v": 2}[gd.model_mean_type])


@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("mean_type", ["v", "eps", "x0"])
def test_fused_step_is_the_composition_of_the_unfused_kernels(mean_type, eta):
    """dsc_ddim_inpaint_step_f32 == ddim_step, then the ragged overwrite at times_next[k] (or the restore on the last pair): torch.equal."""
    from diffuscene_amd import ops
    gd = _diffusion(mean_type)
    S = 50
    dtab = gd.ddim_tables(S, eta, dev())
    pairs = dtab[0]
    args = _step_args(gd, dtab)
    sa, sb = args[7], args[8]
    B, N, C = 6, 21, 65
    xt, mo, noise = (rnd(B, N, C, seed=163) * 1.5).to(dev()), (rnd(B, N, C, seed=164) * 1.5).to(dev()), rnd(B, N, C, seed=165).to(dev())
    for pmax, counts in ((N, [0, 1, 4, N, 20, 7]), (9, [9, 0, 3, 9, 1, 8])):
        part, pn = rnd(B, pmax, C, seed=166).to(dev()), rnd(B, pmax, C, seed=167).to(dev())
        cnt = torch.tensor(counts, dtype=torch.int64, device=dev())
        given = torch.arange(pmax, device=dev())[None, :, None] < cnt[:, None, None]
        for k in (0, S // 2, S - 2, S - 1):
            step = torch.tensor([k], dtype=torch.int64, device=dev())
            last = pairs[k][1] < 0
            assert last == (k == S - 1)
            want = gd.ddim_step(xt, mo, noise, step, dtab)
            free = want.clone()
            if last:
                want[:, :pmax] = torch.where(given, part, want[:, :pmax])                                  # the final restore
            else:
                t_next = torch.full((B,), pairs[k][1], dtype=torch.int64, device=dev())
                ops.complete_overwrite_ragged(want, part, pn, cnt, t_next, sa, sb)                          # what the next pair's overwrite writes
            got = ops.ddim_inpaint_step(xt, mo, noise, part, pn, counts, step, *args)
            assert torch.equal(got, want), (mean_type, eta, k, pmax, float((got - want).abs().max()))
            rest = torch.ones((B, N, 1), dtype=torch.bool, device=dev())
            rest[:, :pmax] = ~given
            assert torch.equal(torch.where(rest, got, free), free)                                         # the free rows are ddim_step's
            inplace = xt.clone()
            ops.ddim_inpaint_step(inplace, mo, noise, part, pn, cnt, step, *args, out=inplace)
            assert torch.equal(inplace, want)
            if last:                                                                                       # the last pair reads neither draw
                nan = float("nan")
                got = ops.ddim_inpaint_step(xt, mo, torch.full_like(noise, nan), part, torch.full_like(pn, nan), cnt, step, *args)
                assert torch.equal(got, want)


def test_out_of_range_device_values_are_clamped_and_counted():
    from diffuscene_amd import _lib, ops
    gd = _diffusion("v")
    S = 50
    dtab = gd.ddim_tables(S, 0.3, dev())
    args = _step_args(gd, dtab)
    B, N, C, pmax = 3, 12, 62, 5
    xt, mo, noise = rnd(B, N, C, seed=168).to(dev()), rnd(B, N, C, seed=171).to(dev()), rnd(B, N, C, seed=172).to(dev())
    part, pn = rnd(B, pmax, C, seed=169).to(dev()), rnd(B, pmax, C, seed=170).to(dev())
    step = torch.tensor([7], dtype=torch.int64, device=dev())
    bad = torch.tensor([-2, 3, pmax + 4], dtype=torch.int64, device=dev())            # on the device: the host cannot check them
    got = ops.ddim_inpaint_step(xt, mo, noise, part, pn, bad, step, *args)
    assert _lib.device_error_count(reset=True) == 2                                     # one per out-of-range scene
    assert torch.equal(got, ops.ddim_inpaint_step(xt, mo, noise, part, pn, [0, 3, pmax], step, *args))
    for bad_step, clamped in ((S + 7, S - 1), (-1, 0)):
        got = ops.ddim_inpaint_step(xt, mo, noise, part, pn, [0, 3, pmax], torch.tensor([bad_step], dtype=torch.int64, device=dev()), *args)
        assert _lib.device_error_count(reset=True) == 1                                 # one per launch
        want = ops.ddim_inpaint_step(xt, mo, noise, part, pn, [0, 3, pmax], torch.tensor([clamped], dtype=torch.int64, device=dev()), *args)
        assert torch.equal(got, want)
    # a table entry outside the schedule: times[k] and times_next[k] are clamped into [0, T)
    times, times_next = args[0].clone(), args[1].clone()
    times[7], times_next[7] = T + 5, T + 1
    got = ops.ddim_inpaint_step(xt, mo, noise, part, pn, [0, 3, pmax], step, times, times_next, *args[2:])
    assert _lib.device_error_count(reset=True) == 2
    times[7], times_next[7] = T - 1, T - 1
    assert torch.equal(got, ops.ddim_inpaint_step(xt, mo, noise, part, pn, [0, 3, pmax], step, times, times_next, *args[2:]))
    with pytest.raises(ValueError, match="scene 2"):
        ops.ddim_inpaint_step(xt, mo, noise, part, pn, [0, 1, pmax + 1], step, *args)


# ------------------------------------------------------------------------------------------------------------------- models
_NETS = {}


def build_net(kw, mean_type, time_num=T):
    from diffuscene_amd.networks.denoise_net import Unet1D
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint
    key = json.dumps(kw, sort_keys=True)
    if key not in _NETS:
        net = Unet1D(**kw)
        net.load_state_dict(W.synth_state_dict(kw))
        _NETS[key] = net.to(dev())
    cfg = dict(objectness_dim=0, class_dim=kw["class_dim"], angle_dim=2, objfeat_dim=32)
    return DiffusionPoint(_NETS[key], cfg, time_num=time_num, model_mean_type=mean_type)


def _ragged(main, part):
    from diffuscene_amd.sampler import RaggedNoiseReplay
    return RaggedNoiseReplay(main.to(dev()), part.to(dev()))


def _bedroom(time_num=T):
    kind, kw, mt, shape, counts, S, eta, x, main, part, cond = ddim_complete_inputs("eps")
    return build_net(W.UNCOND_BEDROOM, "v", time_num), shape, cond.to(dev()), x, main, part


# ------------------------------------------------------------------------------------------------------------------- degenerate counts
def test_counts_of_zero_are_generation_and_counts_of_n_return_the_scenes():
    from diffuscene_amd.sampler import NoiseReplay
    diff, shape, cond, x, main, part = _bedroom()
    B, N, C = shape
    S = 10
    given = x.to(dev())
    with torch.no_grad(), QUIET():
        gen = diff.gen_samples_ddim(shape, dev(), condition=cond, noise_fn=NoiseReplay(main[:S].to(dev())), sampling_timesteps=S,
                                    ddim_sampling_eta=0.5, graph=False)
        for graph in (False, True):
            kw = dict(condition=cond, sampling_timesteps=S, ddim_sampling_eta=0.5, partial_boxes=given, graph=graph)
            zero = diff.complete_samples_ragged_ddim(shape, dev(), noise_fn=_ragged(main, part), num_partial=[0] * B, **kw)
            assert torch.equal(zero, gen), (graph, float((zero - gen).abs().max()))
            full = diff.complete_samples_ragged_ddim(shape, dev(), noise_fn=_ragged(main, part), num_partial=[N] * B, **kw)
            assert torch.equal(full, given), graph


def test_the_eager_loop_makes_its_two_s_draws_in_the_documented_order():
    """x_T (B, N, C); then per pair a partial draw (B, Pmax, C) BEFORE the model call and a main draw (B, N, C) AFTER it; the last
    pair makes the partial draw only: 2 S draws.  Pmax < N here, so the two kinds of draw differ in shape.  (The loop's tables and
    kernels live on the device only, which is why this is not a host test.)"""
    diff, shape, cond, x, _, _ = _bedroom()
    B, N, C = shape
    S, pmax, counts = 5, 7, [0, 2, 6, 7]
    events = []

    def noise_fn(size, dtype, device):
        events.append(tuple(size))
        return torch.randn(size, dtype=dtype, device=device)

    def denoise(data, t, condition, condition_cross):
        events.append("model")
        return diff._denoise(data, t, condition, condition_cross)

    with torch.no_grad(), QUIET():
        out = diff.diffusion.ddim_complete_ragged_loop(denoise, shape, dev(), cond, None, noise_fn=noise_fn, sampling_timesteps=S,
                                                       ddim_sampling_eta=0.4, partial_boxes=x[:, :pmax].contiguous().to(dev()),
                                                       num_partial=counts, graph=False)
    want = [(B, N, C)]
    for k in range(S):
        want += [(B, pmax, C), "model"] + ([(B, N, C)] if k < S - 1 else [])
    assert events == want
    assert sum(e != "model" for e in events) == 2 * S
    for b, p in enumerate(counts):
        assert torch.equal(out[b, :p].cpu(), x[b, :p])


# ------------------------------------------------------------------------------------------------------------------- reference chains
@BOTH
@pytest.mark.parametrize("name", list(CASES))
def test_batched_chain_matches_the_reference_run_scene_by_scene(name, golden_dir, tmp_path, gemm_arith):
    """One batched call against B calls of the reference's ddim_sample_loop at B = 1 (the definition of the strided loops), eager and graph."""
    g = np.load(os.path.join(golden_dir, "ddim_complete.npz"))
    kind, kw, mt, shape, counts, S, eta, x, main, part, cond = ddim_complete_inputs(name)
    B, N, C = shape
    if kind == "net":
        diff, cond = build_net(kw, mt), cond.to(dev())
    else:
        m, cfg = build_wrapper(kw, tmp_path, time_num=T)
        diff = m.diffusion
        with torch.no_grad():
            cond = m._base_condition(None, B, N, dev())
            if counts is not None:
                cond = torch.cat([cond, m.fc_partial_condition(padded_partial(x, counts))], dim=-1).contiguous()
            else:
                cond = torch.cat([cond, m.fc_arrange_condition(m._arrange_input(x.to(dev())))], dim=-1).contiguous()
    res = []
    for graph in (False, True):
        with torch.no_grad(), QUIET():
            if counts is not None:
                res.append(diff.complete_samples_ragged_ddim(shape, dev(), condition=cond, noise_fn=_ragged(main, part), sampling_timesteps=S,
                                                             ddim_sampling_eta=eta, partial_boxes=padded_partial(x, counts),
                                                             num_partial=list(counts), graph=graph))
            else:
                from diffuscene_amd.sampler import NoiseReplay
                res.append(diff.arrange_samples_ddim(shape, dev(), condition=cond, noise_fn=NoiseReplay(main.to(dev())), sampling_timesteps=S,
                                                     ddim_sampling_eta=eta, input_boxes=x.to(dev()), graph=graph))
        check(res[-1], g[name], "ddim completion %s S=%d eta=%g %s (graph=%s)" % (name, S, eta, gemm_arith, graph))
        for b, p in enumerate(counts or ()):
            assert torch.equal(res[-1][b, :p].cpu(), x[b, :p])            # the given objects come back untouched
        if counts is None:
            assert torch.equal(res[-1][:, :, 3:6].cpu(), x[:, :, 3:6]) and torch.equal(res[-1][:, :, 8:].cpu(), x[:, :, 8:])
    assert torch.equal(res[0], res[1])


# ------------------------------------------------------------------------------------------------------------------- the captured loop
def test_graph_and_eager_agree_under_manual_seed_twice_and_share_one_graph():
    diff, shape, cond, x, _, _ = _bedroom()
    mixes = (([0, 2, 6, 12], 0.0), ([12, 0, 1, 5], 0.7))
    S = 12
    runs = {}
    for graph in (False, True):
        torch.manual_seed(1234)
        out = []
        with torch.no_grad(), QUIET():
            for counts, eta in mixes:                              # seeded once: the second call starts where the first left the generator
                out.append(diff.complete_samples_ragged_ddim(shape, dev(), condition=cond, sampling_timesteps=S, ddim_sampling_eta=eta,
                                                             partial_boxes=padded_partial(x, counts), num_partial=counts, graph=graph))
                if graph:
                    out.append(list(diff.diffusion._graphs.values()))
        out.append(torch.cuda.get_rng_state(dev()))
        runs[graph] = out
    (e1, e2, es), (g1, graphs1, g2, graphs2, gs) = runs[False], runs[True]
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    assert torch.equal(e1, g1) and torch.equal(e2, g2)
    assert torch.equal(es, gs)                                     # the device generator ends in the same state
    assert len(graphs1) == len(graphs2) == 1 and graphs1[0] is graphs2[0]     # one graph for both mixes of counts and both eta
    assert type(graphs1[0]).__name__ == "_DDIMCompleteGraph" and graphs1[0].S == S
    for out, (counts, _) in ((g1, mixes[0]), (g2, mixes[1])):
        for b, p in enumerate(counts):
            assert torch.equal(out[b, :p].cpu(), x[b, :p])
    # a change of S re-captures
    with torch.no_grad(), QUIET():
        diff.complete_samples_ragged_ddim(shape, dev(), condition=cond, sampling_timesteps=S + 1, partial_boxes=padded_partial(x, mixes[0][0]),
                                          num_partial=mixes[0][0], graph=True)
    (g,) = diff.diffusion._graphs.values()
    assert g is not graphs1[0] and g.S == S + 1


def test_interleaving_with_the_other_loops_on_one_model():
    diff, shape, cond, x, _, _ = _bedroom(time_num=50)
    counts = [3, 0, 12, 7]
    given = padded_partial(x, counts)

    def sequence(graph):
        torch.manual_seed(99)
        strided = dict(condition=cond, sampling_timesteps=10, ddim_sampling_eta=0.5, partial_boxes=given, num_partial=counts, graph=graph)
        with torch.no_grad(), QUIET():
            return [diff.gen_samples(shape, dev(), condition=cond, clip_denoised=True, graph=graph),
                    diff.complete_samples_ragged_ddim(shape, dev(), **strided),
                    diff.gen_samples_ddim(shape, dev(), condition=cond, sampling_timesteps=10, ddim_sampling_eta=0.5, graph=graph),
                    diff.complete_samples_ragged_ddim(shape, dev(), **strided),
                    diff.complete_samples_ragged(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=given, num_partial=counts, graph=graph),
                    diff.complete_samples_ragged_ddim(shape, dev(), **strided),
                    diff.complete_samples(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=given[:, :3].contiguous(), graph=graph),
                    diff.complete_samples_ragged_ddim(shape, dev(), **strided)]
    eager, graphed = sequence(False), sequence(True)
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert torch.isfinite(b).all() and torch.equal(a, b), (i, float((a - b).abs().max()))
    assert len(diff.diffusion._graphs) == 1                        # the one-live-graph rule


def test_a_single_step_runs_the_final_graph_only():
    diff, shape, cond, x, main, part = _bedroom()
    counts = [0, 2, 6, 12]
    res = []
    for graph in (False, True):
        with torch.no_grad(), QUIET():
            res.append(diff.complete_samples_ragged_ddim(shape, dev(), condition=cond, noise_fn=_ragged(main, part), sampling_timesteps=1,
                                                         partial_boxes=padded_partial(x, counts), num_partial=counts, graph=graph))
    (g,) = diff.diffusion._graphs.values()
    assert g.S == 1 and g.graph is None and g.final is not None
    assert torch.equal(res[0], res[1]) and torch.isfinite(res[1]).all()
    for b, p in enumerate(counts):
        assert torch.equal(res[1][b, :p].cpu(), x[b, :p])
        assert p == shape[1] or float(res[1][b, p:].abs().max()) <= 1.0          # the free rows are the clamped x_start


# ------------------------------------------------------------------------------------------------------------------- entry points
def _check_dicts(got, g, name, b, what):
    want = {k.rsplit(".", 1)[1]: g[k] for k in g.files if k.startswith("%s.dict.%d." % (name, b))}
    assert sorted(got) == sorted(want)
    for k, v in got.items():
        assert v.device.type == "cpu" and tuple(v.shape) == tuple(want[k].shape), (name, b, k, tuple(v.shape), want[k].shape)
        if v.numel():
            check(v, want[k], "%s scene %d %s (%s)" % (name, b, k, what))


@pytest.mark.parametrize("graph_env", ["1", "0"])
def test_complete_scene_batched_strided_gives_the_reference_dicts(graph_env, golden_dir, tmp_path, monkeypatch):
    monkeypatch.setenv("DSC_GRAPH", graph_env)
    g = np.load(os.path.join(golden_dir, "ddim_complete.npz"))
    name = "partial"
    kind, kw, mt, shape, counts, S, eta, x, main, part, _ = ddim_complete_inputs(name)
    B, N, C = shape
    m, cfg = build_wrapper(kw, tmp_path, time_num=T)
    _inject(monkeypatch, "ddim_complete_ragged_loop", lambda: _ragged(main, part))
    room = torch.zeros(B, 1, 64, 64, device=dev())
    scenes = [x[b, :p].contiguous().to(dev()) for b, p in enumerate(counts)]
    with QUIET():
        as_list = m.complete_scene_batched(room, N, C, scenes, sampling_timesteps=S, ddim_sampling_eta=eta)
        junk = torch.full((B, N, C), 7.0)
        for b, p in enumerate(counts):
            junk[b, :p] = x[b, :p]
        as_padded = m.complete_scene_batched(room, N, C, junk.to(dev()), num_partial=list(counts), sampling_timesteps=S, ddim_sampling_eta=eta)
    assert len(as_list) == len(as_padded) == B
    for b in range(B):
        _check_dicts(as_list[b], g, name, b, "complete_scene_batched S=%d DSC_GRAPH=%s" % (S, graph_env))
        for k, v in as_list[b].items():
            assert torch.equal(v, as_padded[b][k])
    # complete_scene: uniform counts, the batch-row-0 post-filter -- scene 2 (3 given objects) alone is the reference's B = 1 run
    _inject(monkeypatch, "ddim_complete_ragged_loop", lambda: _ragged(main[:, 2:3].contiguous(), part[:, 2:3].contiguous()))
    with QUIET():
        one = m.complete_scene(room[:1], N, C, scenes[2][None], batch_size=1, sampling_timesteps=S, ddim_sampling_eta=eta)
    _check_dicts(one, g, name, 2, "complete_scene S=%d DSC_GRAPH=%s" % (S, graph_env))


@pytest.mark.parametrize("graph_env", ["1", "0"])
def test_arrange_scene_batched_strided_gives_the_reference_dicts(graph_env, golden_dir, tmp_path, monkeypatch):
    from diffuscene_amd.sampler import NoiseReplay
    monkeypatch.setenv("DSC_GRAPH", graph_env)
    g = np.load(os.path.join(golden_dir, "ddim_complete.npz"))
    name = "arrange"
    kind, kw, mt, shape, counts, S, eta, x, main, _, _ = ddim_complete_inputs(name)
    B, N, C = shape
    m, cfg = build_wrapper(kw, tmp_path, time_num=T)
    current = {"buf": main.to(dev())}
    _inject(monkeypatch, "ddim_arrange_loop", lambda: NoiseReplay(current["buf"]))
    room = torch.zeros(B, 1, 64, 64, device=dev())
    with QUIET():
        batched = m.arrange_scene_batched(room, N, C, x.to(dev()), sampling_timesteps=S, ddim_sampling_eta=eta)
    assert len(batched) == B
    for b in range(B):
        _check_dicts(batched[b], g, name, b, "arrange_scene_batched S=%d DSC_GRAPH=%s" % (S, graph_env))
    current["buf"] = main[:, 1:2].contiguous().to(dev())
    with QUIET():
        one = m.arrange_scene(room[:1], N, C, x[1:2].to(dev()), batch_size=1, sampling_timesteps=S, ddim_sampling_eta=eta)
    _check_dicts(one, g, name, 1, "arrange_scene S=%d DSC_GRAPH=%s" % (S, graph_env))
