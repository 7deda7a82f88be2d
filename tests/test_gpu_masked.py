"""GPU: element-wise scene in-painting (p_sample_loop_masked / ddim_masked_loop) and ``inpaint_scene_batched`` over them.

* kernels: dsc_masked_overwrite_f32, dsc_p_sample_masked_f32 and dsc_ddim_masked_step_f32 against the composition of the existing ops they
  replace (ops.p_sample / ddim_step, ops.q_sample at t - 1 resp. t_next, torch.where), bit for bit, in place and out of place; operands a
  lane must not read are poisoned with NaN; out-of-range device timesteps clamped and counted;
* reduction: a mask of whole rows [0, counts[b]) is the prefix loop (complete_samples_ragged / _ddim) bit for bit under the same seed,
  captured and eager; an all-zero mask is gen_samples / gen_samples_ddim on the main draws; an all-ones mask returns ``known``;
* reference chains: tests/golden/masked.npz (tools/make_golden_masked.py: the REAL reference's q_sample / p_sample / ddim_sample_loop one
  scene at a time, the select bridged) against ONE batched call on the same noise, under both GEMM arithmetics, eager and graph, with the
  project's ``check`` at 1e-4 (tests/test_gpu_wide.py, as tests/test_gpu_complete_ragged.py applies it);
* the captured loops: one graph per shape for every mask, bit-identical to the eager loops under torch.manual_seed across two calls,
  interleaving with the other loops of one model;
* inpaint_scene_batched against the reference's per-scene dicts, and attribute-level editing through ``attribute_mask``."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import weights as W  # noqa: E402
from oracle.make_golden_wrapper import fake_bert_features, network_config, wrapper_state_dict  # noqa: E402
from tools.make_golden_masked import CASES, TEXT_FREE, case_texts, masked_inputs  # noqa: E402

from test_gpu_complete_ragged import T_SETS, _inject, _tables, build_net, check, dev, padded_partial, rnd  # noqa: E402

BOTH = pytest.mark.parametrize("gemm_arith", ["split", "f32"], indirect=True)
QUIET = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731
NAN = float("nan")


@pytest.fixture(autouse=True)
def no_device_errors():
    """dsc_device_error_count is 0 after every test of this file (the one that provokes clamps counts and resets them itself)."""
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    yield
    assert _lib.device_error_count(reset=True) == 0


# ------------------------------------------------------------------------------------------------------------------- kernels
KB, KC = 6, 62
K_N = (1, 12, 21)                  # inner sizes 62 / 744 / 1302: none a multiple of the 256-thread block, the last two span several blocks


def kernel_masks(N):
    """name -> (KB, N, KC) uint8 on the device: all-zero, all-ones, prefix rows, scattered rows, one channel column, the last element only,
    random bytes (0, 1, 2 and 255 among them)."""
    z = lambda: torch.zeros((KB, N, KC), dtype=torch.uint8)  # noqa: E731
    out = {"zero": z(), "ones": z() + 1}
    m = z()
    for b, p in enumerate([0, 1, 4, N, N - 1, 7]):
        m[b, :min(p, N)] = 1
    out["prefix"] = m
    m = z()
    m[:, ::3] = 255
    m[2] = 0
    out["scattered"] = m
    m = z()
    m[:, :, 29] = 2
    out["column"] = m
    m = z()
    m[:, -1, -1] = 1
    out["last"] = m
    g = torch.Generator().manual_seed(7)
    out["random"] = torch.tensor([0, 0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 5, (KB, N, KC), generator=g)]
    return {k: v.to(dev()) for k, v in out.items()}


def poisoned(t, given):
    """``t`` with NaN wherever ``given`` (a bool tensor broadcastable to t) holds."""
    return torch.where(given, torch.full_like(t, NAN), t)


def test_masked_overwrite_is_q_sample_under_the_mask():
    from diffuscene_amd import ops
    tb, d = _tables()
    sa, sb = d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"]
    for N in K_N:
        x0, known, noise = rnd(KB, N, KC, seed=200).to(dev()), rnd(KB, N, KC, seed=201).to(dev()), rnd(KB, N, KC, seed=202).to(dev())
        for name, mask in kernel_masks(N).items():
            given = mask != 0
            for tv in T_SETS:
                t = torch.tensor(tv, dtype=torch.int64, device=dev())
                want = torch.where(given, ops.q_sample(known, noise, t, sa, sb), x0)
                x = x0.clone()
                assert ops.masked_overwrite(x, known, noise, mask, t, sa, sb) is x
                assert torch.equal(x, want), (N, name, tv)
                x = x0.clone()                                    # a free element reads neither known nor the noise
                ops.masked_overwrite(x, poisoned(known, ~given), poisoned(noise, ~given), mask, t, sa, sb)
                assert torch.equal(x, want), (N, name, tv)


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("mt,ca,cb", [(2, "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"),
                                      (0, "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"), (1, None, None)])
def test_fused_step_is_the_composition_of_the_ops_it_replaces(mt, ca, cb, clip):
    """dsc_p_sample_masked_f32 == where(mask, t > 0 ? q_sample(known, t - 1, noise_k) : known, p_sample(...)): torch.equal."""
    from diffuscene_amd import ops
    tb, d = _tables()
    sa, sb = d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"]
    k1, k2 = d["posterior_mean_coef1"], d["posterior_mean_coef2"]
    A, Bc = (d[ca] if ca else None), (d[cb] if cb else None)
    for N in K_N:
        xt, mo, noise = rnd(KB, N, KC, seed=203).to(dev()), (rnd(KB, N, KC, seed=204) * 2).to(dev()), rnd(KB, N, KC, seed=205).to(dev())
        known, nk = rnd(KB, N, KC, seed=206).to(dev()), rnd(KB, N, KC, seed=207).to(dev())
        for name, mask in kernel_masks(N).items():
            given = mask != 0
            for tv in T_SETS:
                t = torch.tensor(tv, dtype=torch.int64, device=dev())
                last = (t == 0)[:, None, None]
                free = ops.p_sample(xt, mo, noise, t, A, Bc, k1, k2, d["sigma"], mt, clip)
                renoised = ops.q_sample(known, nk, torch.clamp(t - 1, min=0), sa, sb)
                want = torch.where(given, torch.where(last, known, renoised), free)
                args = (t, A, Bc, k1, k2, d["sigma"], sa, sb, mt, clip)
                got = ops.p_sample_masked(xt, mo, noise, known, nk, mask, *args)
                assert torch.equal(got, want), (mt, clip, N, name, tv, float((got - want).abs().max()))
                inplace = xt.clone()
                assert ops.p_sample_masked(inplace, mo, noise, known, nk, mask, *args, out=inplace) is inplace
                assert torch.equal(inplace, want), (mt, clip, N, name, tv)
                # what a lane must not read is NaN: noise_k at t == 0; x_t / model_out / noise under the mask; known / noise_k outside it
                got = ops.p_sample_masked(poisoned(xt, given), poisoned(mo, given), poisoned(noise, given), poisoned(known, ~given),
                                          poisoned(nk, ~given | last), mask, *args)
                assert torch.isfinite(got).all() and torch.equal(got, want), (mt, clip, N, name, tv)


def _diffusion(mean_type="v", T_=1000):
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    return GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, T_),
                             "mse", mean_type, "fixedsmall", False, False, None)


def _step_args(gd, dtab):
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    _, times, times_next, coef = dtab
    return (times, times_next, coef, ca, cb, tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"], tb["sqrt_alphas_cumprod"],
            tb["sqrt_one_minus_alphas_cumprod"], {"eps": 0, "x0": 1, "v": 2}[gd.model_mean_type])


@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("mean_type", ["v", "eps", "x0"])
def test_fused_ddim_step_is_the_composition_of_the_ops_it_replaces(mean_type, eta):
    """dsc_ddim_masked_step_f32 == where(mask, last ? known : q_sample(known, t_next, noise_k), ddim_step(...)): torch.equal."""
    from diffuscene_amd import ops
    gd = _diffusion(mean_type)
    S = 50
    dtab = gd.ddim_tables(S, eta, dev())
    pairs = dtab[0]
    args = _step_args(gd, dtab)
    sa, sb = args[7], args[8]
    for N in K_N:
        xt, mo, noise = (rnd(KB, N, KC, seed=208) * 1.5).to(dev()), (rnd(KB, N, KC, seed=209) * 1.5).to(dev()), rnd(KB, N, KC, seed=210).to(dev())
        known, nk = rnd(KB, N, KC, seed=211).to(dev()), rnd(KB, N, KC, seed=212).to(dev())
        for name, mask in kernel_masks(N).items():
            given = mask != 0
            for k in (0, S // 2, S - 2, S - 1):
                step = torch.tensor([k], dtype=torch.int64, device=dev())
                last = pairs[k][1] < 0
                assert last == (k == S - 1)
                free = gd.ddim_step(xt, mo, noise, step, dtab)
                if last:
                    want = torch.where(given, known, free)
                else:
                    t_next = torch.full((KB,), pairs[k][1], dtype=torch.int64, device=dev())
                    want = torch.where(given, ops.q_sample(known, nk, t_next, sa, sb), free)
                got = ops.ddim_masked_step(xt, mo, noise, known, nk, mask, step, *args)
                assert torch.equal(got, want), (mean_type, eta, N, name, k, float((got - want).abs().max()))
                inplace = xt.clone()
                assert ops.ddim_masked_step(inplace, mo, noise, known, nk, mask, step, *args, out=inplace) is inplace
                assert torch.equal(inplace, want), (mean_type, eta, N, name, k)
                # NaN where a lane must not read: both noises on the last pair; x_t / model_out / noise under the mask; known / noise_k outside
                everywhere = torch.ones_like(given)
                got = ops.ddim_masked_step(poisoned(xt, given), poisoned(mo, given), poisoned(noise, everywhere if last else given),
                                           poisoned(known, ~given), poisoned(nk, everywhere if last else ~given), mask, step, *args)
                assert torch.isfinite(got).all() and torch.equal(got, want), (mean_type, eta, N, name, k)


def test_out_of_range_device_timesteps_are_clamped_and_counted_once_per_scene():
    from diffuscene_amd import _lib, ops
    tb, d = _tables()
    T = 1000
    sa, sb = d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"]
    N = 21                                                                    # several blocks per scene: still one count per scene
    x0, mo, noise = rnd(KB, N, KC, seed=213).to(dev()), rnd(KB, N, KC, seed=214).to(dev()), rnd(KB, N, KC, seed=215).to(dev())
    known, nk = rnd(KB, N, KC, seed=216).to(dev()), rnd(KB, N, KC, seed=217).to(dev())
    mask = kernel_masks(N)["random"]
    bad = torch.tensor([-2, 3, T + 4, 0, T, 999], dtype=torch.int64, device=dev())
    good = torch.tensor([0, 3, T - 1, 0, T - 1, 999], dtype=torch.int64, device=dev())
    x, y = x0.clone(), x0.clone()
    ops.masked_overwrite(x, known, noise, mask, bad, sa, sb)
    assert _lib.device_error_count(reset=True) == 3
    ops.masked_overwrite(y, known, noise, mask, good, sa, sb)
    assert torch.equal(x, y)
    args = (sa, sb, d["posterior_mean_coef1"], d["posterior_mean_coef2"], d["sigma"], sa, sb, 2, True)
    got = ops.p_sample_masked(x0, mo, noise, known, nk, mask, bad, *args)
    assert _lib.device_error_count(reset=True) == 3
    assert torch.equal(got, ops.p_sample_masked(x0, mo, noise, known, nk, mask, good, *args))
    # the strided step: the step index and the table entries, one count per launch (as dsc_ddim_inpaint_step_f32)
    gd = _diffusion("v")
    S = 50
    dtab = gd.ddim_tables(S, 0.3, dev())
    dargs = _step_args(gd, dtab)
    for bad_step, clamped in ((S + 7, S - 1), (-1, 0)):
        got = ops.ddim_masked_step(x0, mo, noise, known, nk, mask, torch.tensor([bad_step], dtype=torch.int64, device=dev()), *dargs)
        assert _lib.device_error_count(reset=True) == 1
        want = ops.ddim_masked_step(x0, mo, noise, known, nk, mask, torch.tensor([clamped], dtype=torch.int64, device=dev()), *dargs)
        assert torch.equal(got, want)
    step = torch.tensor([7], dtype=torch.int64, device=dev())
    times, times_next = dargs[0].clone(), dargs[1].clone()
    times[7], times_next[7] = T + 5, T + 1
    got = ops.ddim_masked_step(x0, mo, noise, known, nk, mask, step, times, times_next, *dargs[2:])
    assert _lib.device_error_count(reset=True) == 2
    times[7], times_next[7] = T - 1, T - 1
    assert torch.equal(got, ops.ddim_masked_step(x0, mo, noise, known, nk, mask, step, times, times_next, *dargs[2:]))
    with pytest.raises(RuntimeError):
        ops.p_sample_masked(x0, mo, noise, known, nk, mask.bool(), good, *args)          # the kernels take bytes: ops.known_mask makes them


# ------------------------------------------------------------------------------------------------------------------- reduction to the prefix loops
PREFIX_COUNTS = (0, 1, 4, 12, 11, 7)


def _bedroom():
    """(DiffusionPoint, shape, condition, scenes) of the bedroom network at T = 50, B = 6."""
    B, N, C = len(PREFIX_COUNTS), 12, 62
    net, diff = build_net(W.UNCOND_BEDROOM, "v")
    return diff, (B, N, C), W.synth_condition(B, N, 128, 5, shared=True).contiguous().to(dev()), W.synth_scene_batch(B, N, 22, 32, 5)


def _prefix_mask(counts, N):
    return torch.arange(N)[None, :] < torch.tensor(counts)[:, None]                        # (B, N) bool: whole rows


@pytest.mark.parametrize("graph_env", ["1", "0"])
def test_a_prefix_mask_is_the_prefix_loop_bit_for_bit_under_the_same_seed(graph_env, monkeypatch):
    monkeypatch.setenv("DSC_GRAPH", graph_env)
    diff, shape, cond, x = _bedroom()
    B, N, C = shape
    given = padded_partial(x, PREFIX_COUNTS)
    mask = _prefix_mask(PREFIX_COUNTS, N)
    junk = torch.where(mask[:, :, None], x, torch.full_like(x, 7.0)).to(dev())             # what the mask does not mark is never read
    with torch.no_grad(), QUIET():
        torch.manual_seed(77)
        old = diff.complete_samples_ragged(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=given, num_partial=list(PREFIX_COUNTS))
        s_old = torch.cuda.get_rng_state(dev())
        torch.manual_seed(77)
        new = diff.inpaint_samples(shape, dev(), condition=cond, clip_denoised=True, known=junk, mask=mask)
        assert torch.equal(s_old, torch.cuda.get_rng_state(dev()))
        assert torch.equal(new, old), float((new - old).abs().max())
        assert [type(g).__name__ for g in diff.diffusion._graphs.values()] == (["_MaskedGraph"] if graph_env == "1" else [])
        for S, eta in ((10, 0.5), (1, 0.0)):
            torch.manual_seed(78)
            old = diff.complete_samples_ragged_ddim(shape, dev(), condition=cond, partial_boxes=given, num_partial=list(PREFIX_COUNTS),
                                                    sampling_timesteps=S, ddim_sampling_eta=eta)
            s_old = torch.cuda.get_rng_state(dev())
            torch.manual_seed(78)
            new = diff.inpaint_samples_ddim(shape, dev(), condition=cond, known=junk, mask=mask.to(torch.uint8) * 255,
                                            sampling_timesteps=S, ddim_sampling_eta=eta)
            assert torch.equal(s_old, torch.cuda.get_rng_state(dev()))
            assert torch.equal(new, old), (S, float((new - old).abs().max()))
    for b, p in enumerate(PREFIX_COUNTS):
        assert torch.equal(new[b, :p].cpu(), x[b, :p])


@pytest.mark.parametrize("graph", [False, True])
def test_an_empty_mask_is_plain_generation_and_a_full_mask_returns_known(graph):
    from diffuscene_amd.sampler import NoiseReplay, RaggedNoiseReplay
    from oracle.make_golden import noise_list
    diff, shape, cond, x = _bedroom()
    B, N, C = shape
    T = diff.diffusion.num_timesteps
    main = torch.stack(noise_list([shape] * (T + 1), 31, "masked_edge_main_")).to(dev())
    kn = torch.stack(noise_list([shape] * T, 31, "masked_edge_known_")).to(dev())
    known = x.to(dev())
    zero, ones = torch.zeros(shape, dtype=torch.bool), torch.ones((B, N), dtype=torch.bool)
    S = 10
    with torch.no_grad(), QUIET():
        gen = diff.gen_samples(shape, dev(), condition=cond, noise_fn=NoiseReplay(main), clip_denoised=True, graph=graph)
        got = diff.inpaint_samples(shape, dev(), condition=cond, noise_fn=RaggedNoiseReplay(main, kn), clip_denoised=True, known=known,
                                   mask=zero, graph=graph)
        assert torch.equal(got, gen)
        gen = diff.gen_samples_ddim(shape, dev(), condition=cond, noise_fn=NoiseReplay(main[:S]), sampling_timesteps=S, ddim_sampling_eta=0.4,
                                    graph=graph)
        got = diff.inpaint_samples_ddim(shape, dev(), condition=cond, noise_fn=RaggedNoiseReplay(main[:S], kn[:S]), known=known, mask=zero,
                                        sampling_timesteps=S, ddim_sampling_eta=0.4, graph=graph)
        assert torch.equal(got, gen)
        assert torch.equal(diff.inpaint_samples(shape, dev(), condition=cond, known=known, mask=ones, graph=graph), known)
        assert torch.equal(diff.inpaint_samples_ddim(shape, dev(), condition=cond, known=known, mask=ones, sampling_timesteps=S, graph=graph), known)


# ------------------------------------------------------------------------------------------------------------------- golden
_MODELS = {}


class _FakeBertCache:
    """text_cache.BertFeatureCache protocol over the golden generator's stand-in encoder (as tests/test_gpu_wrapper.py)."""

    def batch(self, texts, device):
        return fake_bert_features(list(texts)).to(device)


def build_model(name, tmp_path):
    """The wrapper model of a golden case on the device (cached per configuration): seeded parameters, the case's T and mean type."""
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    case, mt, T = CASES[name][:3]
    if (case, mt, T) not in _MODELS:
        stats = tmp_path / "dataset_stats.txt"
        stats.write_text(json.dumps(W.DATASET_STATS))
        cfg = network_config(case, str(stats), T)
        cfg["diffusion_kwargs"]["model_mean_type"] = mt
        if case == "text":
            cfg["text_bert_cached"] = True
        with QUIET():
            m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
        m.load_state_dict(wrapper_state_dict(m))
        if case == "text":
            m.attach_bert_cache(_FakeBertCache())
        _MODELS[(case, mt, T)] = m.to(dev()).eval()
    return _MODELS[(case, mt, T)]


def run_case(m, name, graph):
    from diffuscene_amd.sampler import RaggedNoiseReplay
    case, mt, T, S, eta, clip, known, mask, main, kn = masked_inputs(name)
    B, N, C = known.shape
    room = torch.zeros(B, 1, 64, 64, device=dev())
    with torch.no_grad(), QUIET():
        cond, cross = m._sampling_conditions(room, N, dev(), text=case_texts(name))
        replay = RaggedNoiseReplay(main.to(dev()), kn.to(dev()))
        if S is None:
            return m.diffusion.inpaint_samples((B, N, C), dev(), condition=cond, condition_cross=cross, noise_fn=replay, clip_denoised=clip,
                                               known=known.to(dev()), mask=mask, graph=graph)
        return m.diffusion.inpaint_samples_ddim((B, N, C), dev(), condition=cond, condition_cross=cross, noise_fn=replay,
                                                known=known.to(dev()), mask=mask, sampling_timesteps=S, ddim_sampling_eta=eta, graph=graph)


@BOTH
@pytest.mark.parametrize("name", list(CASES))
def test_batched_masked_chain_matches_the_reference_run_scene_by_scene(name, golden_dir, tmp_path, gemm_arith):
    """One batched call against B runs of the reference's own pieces at B = 1 (the definition of the masked loops), eager and graph."""
    g = np.load(os.path.join(golden_dir, "masked.npz"))
    known, mask = masked_inputs(name)[6:8]
    m = build_model(name, tmp_path)
    res = []
    for graph in (False, True):
        res.append(run_case(m, name, graph))
        check(res[-1], g[name], "masked in-painting %s %s (graph=%s)" % (name, gemm_arith, graph))
        assert torch.equal(res[-1].cpu()[mask], known[mask])                 # the given elements come back bit-equal
    assert torch.equal(res[0], res[1])


# ------------------------------------------------------------------------------------------------------------------- the captured loops
def _two_masks(shape):
    B, N, C = shape
    a = _prefix_mask(PREFIX_COUNTS, N)[:, :, None].expand(B, N, C).clone()
    b = torch.zeros(shape, dtype=torch.bool)
    b[:, :, 8:30] = True                                                     # the class channels of every row
    b[0] = False
    b[1, 3, 0:3] = True
    return a, b


def test_one_graph_per_shape_serves_every_mask_and_agrees_with_the_eager_loop_under_a_seed():
    diff, shape, cond, x = _bedroom()
    known = x.to(dev())
    masks = _two_masks(shape)
    for loop, kw, cls in (("inpaint_samples", dict(clip_denoised=True), "_MaskedGraph"),
                          ("inpaint_samples_ddim", dict(sampling_timesteps=10, ddim_sampling_eta=0.5), "_DDIMMaskedGraph")):
        runs = {}
        for graph in (False, True):
            torch.manual_seed(1234)
            out = []
            with torch.no_grad(), QUIET():
                for mask in masks:                                   # seeded once: the second call starts where the first left the generator
                    out.append(getattr(diff, loop)(shape, dev(), condition=cond, known=known, mask=mask, graph=graph, **kw))
                    if graph:
                        out.append(list(diff.diffusion._graphs.values()))
            out.append(torch.cuda.get_rng_state(dev()))
            runs[graph] = out
        (e1, e2, es), (g1, graphs1, g2, graphs2, gs) = runs[False], runs[True]
        assert torch.equal(e1, g1) and torch.equal(e2, g2), loop
        assert torch.equal(es, gs)                                   # the device generator ends in the same state
        assert len(graphs1) == len(graphs2) == 1 and graphs1[0] is graphs2[0]     # one graph for both masks
        assert type(graphs1[0]).__name__ == cls
        for out, mask in ((g1, masks[0]), (g2, masks[1])):
            assert torch.equal(out.cpu()[mask], x[mask]) and torch.isfinite(out).all()
        if loop == "inpaint_samples_ddim":                           # eta is not part of the key either
            with torch.no_grad(), QUIET():
                diff.inpaint_samples_ddim(shape, dev(), condition=cond, known=known, mask=masks[0], graph=True, sampling_timesteps=10,
                                          ddim_sampling_eta=0.0)
            assert list(diff.diffusion._graphs.values())[0] is graphs1[0]


def test_interleaving_with_the_other_loops_on_one_model(tmp_path):
    diff, shape, cond, x = _bedroom()
    known = x.to(dev())
    given = padded_partial(x, PREFIX_COUNTS)
    ma, mb = _two_masks(shape)

    def sequence(graph):
        torch.manual_seed(99)
        with torch.no_grad(), QUIET():
            return [diff.gen_samples(shape, dev(), condition=cond, clip_denoised=True, graph=graph),
                    diff.inpaint_samples(shape, dev(), condition=cond, clip_denoised=True, known=known, mask=mb, graph=graph),
                    diff.complete_samples_ragged(shape, dev(), condition=cond, clip_denoised=True, partial_boxes=given,
                                                 num_partial=list(PREFIX_COUNTS), graph=graph),
                    diff.inpaint_samples_ddim(shape, dev(), condition=cond, known=known, mask=ma, sampling_timesteps=10, graph=graph),
                    diff.gen_samples_ddim(shape, dev(), condition=cond, sampling_timesteps=10, ddim_sampling_eta=0.5, graph=graph),
                    diff.inpaint_samples(shape, dev(), condition=cond, clip_denoised=True, known=known, mask=ma, graph=graph),
                    diff.inpaint_samples_ddim(shape, dev(), condition=cond, known=known, mask=mb, sampling_timesteps=10, graph=graph)]
    eager, graphed = sequence(False), sequence(True)
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert torch.isfinite(b).all() and torch.equal(a, b), (i, float((a - b).abs().max()))
    assert len(diff.diffusion._graphs) == 1                          # the one-live-graph rule

    # the scene-level entry points of one wrapper model, captured loops throughout
    m = build_model("eps.T50", tmp_path)
    B, N, C = shape
    room = torch.zeros(B, 1, 64, 64, device=dev())
    rows = m.attribute_mask(list(PREFIX_COUNTS), m.ATTRIBUTES, B, N)
    with QUIET():
        torch.manual_seed(5)
        first = m.inpaint_scene_batched(room, N, C, known, rows, clip_denoised=True, keep_empty=True)
        m.generate_layout(room[:1], N, C, batch_size=1, clip_denoised=True)
        m.complete_scene_batched(room, N, C, [x[b, :p].to(dev()) for b, p in enumerate(PREFIX_COUNTS)], clip_denoised=True)
        m.generate_layout_batched(room, N, C, B, sampling_timesteps=5)
        torch.manual_seed(5)
        again = m.inpaint_scene_batched(room, N, C, known, rows, clip_denoised=True, keep_empty=True)
    for a, b in zip(first, again):
        assert all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------------------------- the wrapper
@pytest.mark.parametrize("name", list(TEXT_FREE))
def test_inpaint_scene_batched_gives_the_reference_filtered_dicts(name, golden_dir, tmp_path, monkeypatch):
    from diffuscene_amd.sampler import RaggedNoiseReplay
    g = np.load(os.path.join(golden_dir, "masked.npz"))
    case, mt, T, S, eta, clip, known, mask, main, kn = masked_inputs(name)
    B, N, C = known.shape
    m = build_model(name, tmp_path)
    _inject(monkeypatch, "p_sample_loop_masked" if S is None else "ddim_masked_loop", lambda: RaggedNoiseReplay(main.to(dev()), kn.to(dev())))
    room = torch.zeros(B, 1, 64, 64, device=dev())
    kw = dict(clip_denoised=clip) if S is None else dict(sampling_timesteps=S, ddim_sampling_eta=eta)
    with QUIET():
        got = m.inpaint_scene_batched(room, N, C, known.to(dev()), mask, **kw)
    assert len(got) == B
    for b in range(B):
        want = {k.rsplit(".", 1)[1]: g[k] for k in g.files if k.startswith("%s.dict.%d." % (name, b))}
        assert sorted(got[b]) == sorted(want)
        for k, v in got[b].items():
            assert v.device.type == "cpu" and tuple(v.shape) == tuple(want[k].shape), (name, b, k, tuple(v.shape), want[k].shape)   # kept-box counts
            if v.numel():
                check(v, want[k], "%s inpaint_scene_batched scene %d %s" % (name, b, k))


@pytest.mark.parametrize("strided", [False, True])
def test_given_sizes_and_classes_come_back_bit_for_bit(strided, tmp_path):
    """'These are the furniture classes and sizes, place them': sizes | class_labels | objfeats known on all rows."""
    m = build_model("eps.T50", tmp_path)
    B, N, C = 5, 12, 62
    x = W.synth_scene_batch(B, N, 22, 32, 9)
    mask = m.attribute_mask(N, ("sizes",), B, N) | m.attribute_mask(N, ("class_labels",), B, N) | m.attribute_mask(N, ("objfeats",), B, N)
    room = torch.zeros(B, 1, 64, 64, device=dev())
    torch.manual_seed(11)
    with QUIET():
        scenes = m.inpaint_scene_batched(room, N, C, [x[b] for b in range(B)], mask, **(dict(sampling_timesteps=8) if strided else {}))
    assert len(scenes) == B
    for b, d in enumerate(scenes):
        keep = ~(x[b, :, 29] >= 0)                                   # given rows are filtered like any others: by their own 'empty' logit
        assert d["sizes"].shape[1] == int(keep.sum())
        assert torch.equal(d["sizes"][0], x[b, keep, 3:6]) and torch.equal(d["class_labels"][0], x[b, keep, 8:29])
        assert torch.equal(d["objfeats"][0], x[b, keep, 30:62])
        assert torch.isfinite(d["translations"]).all() and torch.isfinite(d["angles"]).all()
