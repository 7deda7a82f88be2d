"""GPU: batched scene completion with per-scene counts (p_sample_loop_complete_ragged) and the batched entry points over it.

* kernels: dsc_complete_overwrite_ragged_f32 against the fp32 CPU expression and dsc_p_sample_inpaint_f32 against the composition of the
  kernels it fuses, bit for bit;
* uniform counts: the ragged loop is the existing (reference-pinned) uniform loop, value for value, eager and graph;
* reference chains: tests/golden/complete_ragged.npz (tools/make_golden_complete_ragged.py: the REAL reference's complete_samples run once
  per scene at B = 1) against ONE batched call on the same noise, under both GEMM arithmetics, with the criterion of the project's other
  T = 50 completion chain (tests/test_gpu_wide.py::test_completion_n80_p20_eager_and_graph: ``check`` at 1e-4, copied below);
* the captured loop: bit-identical to the eager one under torch.manual_seed (second call included), one graph for every mix of counts,
  interleaving with the DDPM / DDIM generation graphs;
* complete_scene_batched / arrange_scene_batched against the reference's per-scene dicts."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import ref_torch as R  # noqa: E402
from oracle import weights as W  # noqa: E402
from oracle.make_golden import noise_list  # noqa: E402
from oracle.make_golden_wide import WIDE, wide_inputs  # noqa: E402
from oracle.make_golden_wrapper import network_config, wrapper_batch, wrapper_state_dict  # noqa: E402
from oracle.make_golden_wrapper import B as WB, N as WN, SAMPLE_T  # noqa: E402
from make_golden_complete_ragged import CASES, T, ragged_inputs  # noqa: E402

TOL = 1e-4
BOTH = pytest.mark.parametrize("gemm_arith", ["split", "f32"], indirect=True)


def dev():
    return torch.device("cuda:0")


def check(a, b, what, tol=TOL):
    """The criterion of tests/test_gpu_wide.py: norm-relative AND element-wise (relative to max(|b|, 5 % of the range)) distance below `tol`."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bmax = float(b.abs().max())
    r = float((a - b).abs().max() / bmax)
    ew = float(((a - b).abs() / torch.clamp(b.abs(), min=5e-2 * bmax)).max())
    strict = float((((a - b).abs() <= 1e-4 * torch.clamp(b.abs(), min=1e-3)).double()).mean())
    line = "%s: norm-relative %.3g, element-wise %.3g (%.2f%% of elements within 1e-4*max(|b|,1e-3))" % (what, r, ew, 100 * strict)
    print(line)
    if os.environ.get("DSC_PARITY_LOG"):
        with open(os.environ["DSC_PARITY_LOG"], "a") as f:
            f.write(line + "\n")
    assert r < tol and ew < tol, (what, r, ew)


def no_device_errors():
    from diffuscene_amd import _lib
    assert _lib.device_error_count(reset=True) == 0


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------- kernels
T_K = 1000
T_SETS = ([0] * 6, [1] * 6, [T_K - 1] * 6, [0, 1, 500, 998, 999, 0], [2, 0, 999, 1, 0, 17])


def _tables():
    tb = R.schedule_tables(1e-4, 0.02, T_K, "v")
    d = {k: tb[k].to(dev()) for k in tb}
    d["sigma"] = torch.exp(0.5 * tb["posterior_log_variance_clipped"]).to(dev())
    return tb, d


@pytest.mark.parametrize("pmax,counts", [(21, [0, 1, 4, 21, 20, 7]), (9, [9, 0, 3, 9, 1, 8]), (1, [1, 0, 1, 0, 0, 1])])
def test_ragged_overwrite_is_the_cpu_expression_bit_for_bit(pmax, counts):
    from diffuscene_amd import _lib, ops
    _lib.device_error_count(reset=True)
    tb, d = _tables()
    B, N, C = 6, 21, 65
    part, pn = rnd(B, pmax, C, seed=60), rnd(B, pmax, C, seed=61)
    for tv in T_SETS:
        t = torch.tensor(tv, dtype=torch.int64)
        x0 = rnd(B, N, C, seed=62)
        x = x0.to(dev())
        ops.complete_overwrite_ragged(x, part.to(dev()), pn.to(dev()), counts, t.to(dev()), d["sqrt_alphas_cumprod"],
                                      d["sqrt_one_minus_alphas_cumprod"])
        want = x0.clone()
        q = R.q_sample(tb, part, t, pn)
        for b, p in enumerate(counts):
            want[b, :p] = q[b, :p]
        assert torch.equal(x.cpu(), want), (tv, float((x.cpu() - want).abs().max()))
    # counts already on the device are taken as they are; uniform counts are dsc_complete_overwrite_f32
    x, y = x0.to(dev()), x0.to(dev())
    full = torch.full((B,), pmax, dtype=torch.int64, device=dev())
    ops.complete_overwrite_ragged(x, part.to(dev()), pn.to(dev()), full, t.to(dev()), d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"])
    ops.complete_overwrite(y, part.to(dev()), pn.to(dev()), t.to(dev()), d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"])
    assert torch.equal(x, y)
    with pytest.raises(ValueError, match="scene 2"):
        ops.complete_overwrite_ragged(x, part.to(dev()), pn.to(dev()), [0, 1, pmax + 1, 0, 0, 0], t.to(dev()), d["sqrt_alphas_cumprod"],
                                      d["sqrt_one_minus_alphas_cumprod"])
    no_device_errors()


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("mt,ca,cb", [(2, "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"),
                                      (0, "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"), (1, None, None)])
def test_fused_step_is_the_composition_of_the_unfused_kernels(mt, ca, cb, clip):
    """dsc_p_sample_inpaint_f32 == p_sample, then the ragged overwrite at t - 1 (t > 0) or the restore (t == 0): torch.equal."""
    from diffuscene_amd import _lib, ops
    _lib.device_error_count(reset=True)
    tb, d = _tables()
    B, N, C = 6, 21, 65
    sa, sb = d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"]
    k1, k2 = d["posterior_mean_coef1"], d["posterior_mean_coef2"]
    A, Bc = (d[ca] if ca else None), (d[cb] if cb else None)
    xt, mo, noise = rnd(B, N, C, seed=63).to(dev()), (rnd(B, N, C, seed=64) * 2).to(dev()), rnd(B, N, C, seed=65).to(dev())
    for pmax, counts in ((N, [0, 1, 4, N, 20, 7]), (9, [9, 0, 3, 9, 1, 8])):
        part, pn = rnd(B, pmax, C, seed=66).to(dev()), rnd(B, pmax, C, seed=67).to(dev())
        cnt = torch.tensor(counts, dtype=torch.int64, device=dev())
        given = torch.arange(pmax, device=dev())[None, :, None] < cnt[:, None, None]
        for tv in T_SETS:
            t = torch.tensor(tv, dtype=torch.int64, device=dev())
            want = ops.p_sample(xt, mo, noise, t, A, Bc, k1, k2, d["sigma"], mt, clip)
            free = want.clone()
            ops.complete_overwrite_ragged(want, part, pn, cnt, torch.clamp(t - 1, min=0), sa, sb)      # what the next step's overwrite writes
            last = (t == 0)[:, None, None] & given
            want[:, :pmax] = torch.where(last, part, want[:, :pmax])                                    # t == 0: the final restore
            got = ops.p_sample_inpaint(xt, mo, noise, part, pn, counts, t, A, Bc, k1, k2, d["sigma"], sa, sb, mt, clip)
            assert torch.equal(got, want), (mt, clip, tv, pmax, float((got - want).abs().max()))
            rest = torch.ones((B, N, 1), dtype=torch.bool, device=dev())
            rest[:, :pmax] = ~given
            assert torch.equal(torch.where(rest, got, free), free)                                      # the free rows are p_sample's
            inplace = xt.clone()
            ops.p_sample_inpaint(inplace, mo, noise, part, pn, cnt, t, A, Bc, k1, k2, d["sigma"], sa, sb, mt, clip, out=inplace)
            assert torch.equal(inplace, want)
    no_device_errors()


def test_out_of_range_device_counts_are_clamped_and_counted():
    from diffuscene_amd import _lib, ops
    _lib.device_error_count(reset=True)
    tb, d = _tables()
    B, N, C, pmax = 3, 12, 62, 5
    sa, sb = d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"]
    x0, part, pn = rnd(B, N, C, seed=68).to(dev()), rnd(B, pmax, C, seed=69).to(dev()), rnd(B, pmax, C, seed=70).to(dev())
    t = torch.tensor([3, 0, 999], dtype=torch.int64, device=dev())
    bad = torch.tensor([-2, 3, pmax + 4], dtype=torch.int64, device=dev())          # on the device: the host cannot check them
    x, y = x0.clone(), x0.clone()
    ops.complete_overwrite_ragged(x, part, pn, bad, t, sa, sb)
    assert _lib.device_error_count(reset=True) == 2                                   # one per out-of-range scene
    ops.complete_overwrite_ragged(y, part, pn, [0, 3, pmax], t, sa, sb)
    assert torch.equal(x, y)
    mo, noise = rnd(B, N, C, seed=71).to(dev()), rnd(B, N, C, seed=72).to(dev())
    args = (t, sa, sb, d["posterior_mean_coef1"], d["posterior_mean_coef2"], d["sigma"], sa, sb, 2, True)
    got = ops.p_sample_inpaint(x0, mo, noise, part, pn, bad, *args)
    assert _lib.device_error_count(reset=True) == 2
    assert torch.equal(got, ops.p_sample_inpaint(x0, mo, noise, part, pn, [0, 3, pmax], *args))
    no_device_errors()


# ------------------------------------------------------------------------------------------------------------------- models
_NETS = {}


def build_net(kw, mean_type):
    """(net, DiffusionPoint) of a diffusion-level case: seeded weights, T = 50."""
    from diffuscene_amd.networks.denoise_net import Unet1D
    from diffuscene_amd.networks.diffusion_ddpm import DiffusionPoint
    key = json.dumps(kw, sort_keys=True)
    if key not in _NETS:
        net = Unet1D(**kw)
        net.load_state_dict(W.synth_state_dict(kw))
        _NETS[key] = net.to(dev())
    cfg = dict(objectness_dim=0, class_dim=kw["class_dim"], angle_dim=2, objfeat_dim=32)
    return _NETS[key], DiffusionPoint(_NETS[key], cfg, time_num=T, model_mean_type=mean_type)


def build_wrapper(case, tmp_path, time_num=T):
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = network_config(case, str(stats), time_num)
    with contextlib.redirect_stdout(io.StringIO()):
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
    m.load_state_dict(wrapper_state_dict(m))
    return m.to(dev()).eval(), cfg


def padded_partial(x, counts):
    """(B, N, C): the given rows of every scene, zeros beyond its count -- what complete_scene_batched builds."""
    p = torch.zeros_like(x)
    for b, c in enumerate(counts):
        p[b, :c] = x[b, :c]
    return p.to(dev())


def case_model(name, tmp_path):
    """(DiffusionPoint, condition on the device, wrapper or None) of a golden case."""
    kind, kw, mt, shape, counts, clip, x, main, part, cond = ragged_inputs(name)
    if kind == "net":
        return build_net(kw, mt)[1], cond.to(dev()), None
    m, cfg = build_wrapper(kw, tmp_path)
    B, N, C = shape
    with torch.no_grad():
        condition = m._base_condition(None, B, N, dev())
        if m.room_partial_condition:
            condition = torch.cat([condition, m.fc_partial_condition(padded_partial(x, counts))], dim=-1)
    return m.diffusion, condition.contiguous(), m


# ------------------------------------------------------------------------------------------------------------------- uniform counts
def test_uniform_counts_are_the_existing_loop_value_for_value(golden_dir):
    """complete_samples_ragged with every count = P is complete_samples on the same replayed noise, eager and graph: the new loop hangs
    on one that tests/test_gpu_wide.py already pins to the reference."""
    from diffuscene_amd import _lib
    from diffuscene_amd.sampler import NoiseReplay
    _lib.device_error_count(reset=True)
    kw, x, t, cond, _ = wide_inputs("living80")
    B, N, C = x.shape
    P = 20
    net, diff = build_net(WIDE["living80"][0], "v")
    shapes = [(B, N, C)]
    for _ in range(T):
        shapes += [(B, P, C), (B, N, C)]
    seq = noise_list(shapes, 41, "complete80_")
    main, part = torch.stack([seq[0]] + seq[2::2]).to(dev()), torch.stack(seq[1::2]).to(dev())
    partial = x[:, :P, :].contiguous().to(dev())
    kwargs = dict(condition=cond.to(dev()), clip_denoised=True, partial_boxes=partial)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        old = diff.complete_samples((B, N, C), dev(), noise_fn=NoiseReplay(main, part), graph=False, **kwargs)
        for graph in (False, True):
            for counts in ([P] * B, torch.full((B,), P, dtype=torch.int64, device=dev())):
                new = diff.complete_samples_ragged((B, N, C), dev(), noise_fn=NoiseReplay(main, part), num_partial=counts, graph=graph, **kwargs)
                assert torch.equal(new, old), (graph, float((new - old).abs().max()))
    check(old, np.load(os.path.join(golden_dir, "wide.npz"))["complete80.T50"], "uniform completion N=80 P=20 T=50")
    no_device_errors()


# ------------------------------------------------------------------------------------------------------------------- reference chains
@BOTH
@pytest.mark.parametrize("name", list(CASES))
def test_batched_chain_matches_the_reference_run_scene_by_scene(name, golden_dir, tmp_path, gemm_arith):
    """One batched call against B calls of the reference at B = 1 (the definition of the ragged loop), eager and graph.  The batched side
    runs the batch-B GEMM dispatch, the reference side one scene: a miss here would be a finding about dispatch, not noise to absorb."""
    from diffuscene_amd import _lib
    from diffuscene_amd.sampler import RaggedNoiseReplay
    _lib.device_error_count(reset=True)
    g = np.load(os.path.join(golden_dir, "complete_ragged.npz"))
    kind, kw, mt, shape, counts, clip, x, main, part, _ = ragged_inputs(name)
    diff, cond, _ = case_model(name, tmp_path)
    given = padded_partial(x, counts)
    res = []
    for graph in (False, True):
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            res.append(diff.complete_samples_ragged(shape, dev(), condition=cond, noise_fn=RaggedNoiseReplay(main.to(dev()), part.to(dev())),
                                                    clip_denoised=clip, partial_boxes=given, num_partial=list(counts), graph=graph))
        check(res[-1], g[name], "ragged completion %s T=%d %s (graph=%s)" % (name, T, gemm_arith, graph))
        for b, p in enumerate(counts):
            assert torch.equal(res[-1][b, :p].cpu(), x[b, :p])            # the given objects come back untouched
    assert torch.equal(res[0], res[1])
    no_device_errors()


# ------------------------------------------------------------------------------------------------------------------- the captured loop
def _bedroom(tmp_path=None):
    kind, kw, mt, shape, counts, clip, x, main, part, cond = ragged_inputs("eps")
    net, diff = build_net(W.UNCOND_BEDROOM, "v")
    return diff, shape, cond.to(dev()), x


def test_graph_and_eager_agree_under_manual_seed_twice_and_share_one_graph():
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    diff, shape, cond, x = _bedroom()
    B, N, C = shape
    mixes = ([0, 2, 6, 12], [12, 0, 1, 5])
    runs = {}
    for graph in (False, True):
        torch.manual_seed(1234)
        out = []
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            for counts in mixes:                                   # seeded once: the second call starts where the first left the generator
                out.append(diff.complete_samples_ragged(shape, dev(), condition=cond, clip_denoised=True,
                                                        partial_boxes=padded_partial(x, counts), num_partial=counts, graph=graph))
                if graph:
                    out.append(list(diff.diffusion._graphs.values()))
        out.append(torch.cuda.get_rng_state(dev()))
        runs[graph] = out
    (e1, e2, es), (g1, graphs1, g2, graphs2, gs) = runs[False], runs[True]
    assert torch.equal(e1, g1) and torch.equal(e2, g2)
    assert torch.equal(es, gs)                                     # the device generator ends in the same state
    assert not torch.equal(e1[1], e2[1])
    assert len(graphs1) == len(graphs2) == 1 and graphs1[0] is graphs2[0]     # one graph for both mixes of counts
    assert type(graphs1[0]).__name__ == "_RaggedCompleteGraph"
    for out, counts in ((g1, mixes[0]), (g2, mixes[1])):
        for b, p in enumerate(counts):
            assert torch.equal(out[b, :p].cpu(), x[b, :p])
    no_device_errors()


def test_interleaving_with_ddpm_and_ddim_generation_on_one_model():
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    diff, shape, cond, x = _bedroom()
    counts = [3, 0, 12, 7]
    given = padded_partial(x, counts)

    def sequence(graph):
        torch.manual_seed(99)
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            return [diff.gen_samples(shape, dev(), condition=cond, clip_denoised=True, graph=graph),
                    diff.complete_samples_ragged(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=given, num_partial=counts, graph=graph),
                    diff.gen_samples_ddim(shape, dev(), condition=cond, sampling_timesteps=10, ddim_sampling_eta=0.5, graph=graph),
                    diff.complete_samples_ragged(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=given, num_partial=counts, graph=graph),
                    diff.complete_samples(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=given[:, :3].contiguous(), graph=graph),
                    diff.gen_samples(shape, dev(), condition=cond, clip_denoised=True, graph=graph)]
    eager, graphed = sequence(False), sequence(True)
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert torch.isfinite(b).all() and torch.equal(a, b), (i, float((a - b).abs().max()))
    assert len(diff.diffusion._graphs) == 1                        # the one-live-graph rule
    no_device_errors()


# ------------------------------------------------------------------------------------------------------------------- entry points
def _inject(monkeypatch, loop, make_noise_fn):
    from diffuscene_amd.networks import diffusion_ddpm as dd
    orig = getattr(dd.GaussianDiffusion, loop)

    def wrapped(self, *a, **kw):
        if kw.get("noise_fn", torch.randn) is torch.randn:
            kw["noise_fn"] = make_noise_fn()
        return orig(self, *a, **kw)
    monkeypatch.setattr(dd.GaussianDiffusion, loop, wrapped)


@pytest.mark.parametrize("graph_env", ["1", "0"])
@pytest.mark.parametrize("name", ["bedroom", "partial"])
def test_complete_scene_batched_gives_the_reference_dicts(name, graph_env, golden_dir, tmp_path, monkeypatch):
    """The list of dicts of ONE complete_scene_batched call against the dict the reference's delete_empty_from_network_samples makes of
    each of its B = 1 runs ('partial': a room_partial_condition model, whose condition the reference builds from cat([partial, zeros]))."""
    from diffuscene_amd import _lib
    from diffuscene_amd.sampler import RaggedNoiseReplay
    _lib.device_error_count(reset=True)
    monkeypatch.setenv("DSC_GRAPH", graph_env)
    g = np.load(os.path.join(golden_dir, "complete_ragged.npz"))
    kind, kw, mt, shape, counts, clip, x, main, part, _ = ragged_inputs(name)
    B, N, C = shape
    m, cfg = build_wrapper(kw, tmp_path)
    _inject(monkeypatch, "p_sample_loop_complete_ragged", lambda: RaggedNoiseReplay(main.to(dev()), part.to(dev())))
    room = torch.zeros(B, 1, 64, 64, device=dev())
    scenes = [x[b, :p].contiguous().to(dev()) for b, p in enumerate(counts)]
    with contextlib.redirect_stdout(io.StringIO()):
        as_list = m.complete_scene_batched(room, N, C, scenes, clip_denoised=clip)
        junk = torch.full((B, N, C), 7.0)
        for b, p in enumerate(counts):
            junk[b, :p] = x[b, :p]
        as_padded = m.complete_scene_batched(room, N, C, junk.to(dev()), num_partial=list(counts), clip_denoised=clip)
    assert len(as_list) == len(as_padded) == B
    for b in range(B):
        want = {k.rsplit(".", 1)[1]: g[k] for k in g.files if k.startswith("%s.dict.%d." % (name, b))}
        assert sorted(as_list[b]) == sorted(want) == sorted(as_padded[b])
        for k, v in as_list[b].items():
            assert v.device.type == "cpu" and tuple(v.shape) == tuple(want[k].shape), (name, b, k, tuple(v.shape), want[k].shape)
            assert torch.equal(v, as_padded[b][k])
            if v.numel():
                check(v, want[k], "%s complete_scene_batched scene %d %s (DSC_GRAPH=%s)" % (name, b, k, graph_env))
    no_device_errors()


def test_arrange_scene_batched_scene_b_is_arrange_scene_at_batch_one(tmp_path, monkeypatch):
    from diffuscene_amd import _lib
    from diffuscene_amd.sampler import NoiseReplay
    _lib.device_error_count(reset=True)
    m, cfg = build_wrapper("arrange", tmp_path, time_num=SAMPLE_T)
    C = cfg["point_dim"]
    _, x = wrapper_batch("arrange")
    x = x.to(dev())
    room = torch.zeros(WB, 1, 64, 64, device=dev())
    buf = torch.stack(noise_list([(WB, WN, 5)] * (SAMPLE_T + 1), 74, "arrange_batched_")).to(dev())
    current = {}
    _inject(monkeypatch, "p_sample_loop_arrange", lambda: NoiseReplay(current["buf"]))
    with contextlib.redirect_stdout(io.StringIO()):
        current["buf"] = buf
        batched = m.arrange_scene_batched(room, WN, C, x, clip_denoised=True)
        assert len(batched) == WB
        for b in range(WB):
            current["buf"] = buf[:, b:b + 1].contiguous()
            one = m.arrange_scene(room[:1], WN, C, x[b:b + 1], batch_size=1, clip_denoised=True)
            assert sorted(one) == sorted(batched[b])
            for k, v in one.items():
                assert tuple(v.shape) == tuple(batched[b][k].shape), (b, k)
                if v.numel():
                    check(batched[b][k], v, "arrange_scene_batched scene %d %s" % (b, k))
    no_device_errors()
