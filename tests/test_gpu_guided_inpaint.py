"""GPU: text-guided element-wise in-painting (p_sample_loop_masked_guided / ddim_masked_guided_loop) and ``guidance_scale`` on
``inpaint_scene_batched``.

* kernels: dsc_p_sample_masked_cfg_f32 / dsc_ddim_masked_cfg_step_f32 against dsc_cfg_combine_f32 followed by the existing masked step
  (torch.equal), out of place and in place with x_dup, every operand a lane must not read poisoned with NaN, an all-free mask against the
  guided step, scale 0 against the masked step on the null half, out-of-range indices clamped and counted;
* the captured loops against the eager ones bit for bit under a seed, through a replay buffer and with per-scene seeds; the unfused
  captured step against the fused one; one graph for every mask and every mix of scales; an all-zero mask is guided generation;
* reference chains: tests/golden/guided_inpaint.npz (tools/make_golden_guided_inpaint.py: the REAL reference one scene at a time around
  the select and the guided bridge) under both GEMM arithmetics, bounded by the larger of the project's chain criterion and 4 x the
  chain's stored reference sensitivity -- the rule of tests/test_gpu_cfg.py;
* inpaint_scene_batched with ``guidance_scale``, T-step and strided; ``guidance_scale=None`` is the call as it was."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import weights as W  # noqa: E402
from tools.make_golden_cfg import distance  # noqa: E402
from tools.make_golden_guided_inpaint import B as GB, C as GC, CASES, N as GN, SCALES, case_texts, chain_inputs, scene_masks  # noqa: E402

from test_gpu_cfg import BOTH, KB, QUIET, SCALE_SET, SHAPES, T_K, T_SETS, _conditions, _diffusion, _scales, build_model  # noqa: E402
from test_gpu_complete_ragged import _tables, dev, rnd  # noqa: E402
from test_gpu_masked import _step_args, poisoned  # noqa: E402

NAN = float("nan")


@pytest.fixture(autouse=True)
def no_device_errors():
    """dsc_device_error_count is 0 after every test of this file (the one that provokes clamps counts and resets them itself)."""
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    yield
    assert _lib.device_error_count(reset=True) == 0


# ------------------------------------------------------------------------------------------------------------------- kernels
def _operands(N, C, seed):
    """x, model_out (2 KB), noise, known, noise_k."""
    x, noise = rnd(KB, N, C, seed=seed).to(dev()), rnd(KB, N, C, seed=seed + 2).to(dev())
    mo = (rnd(2 * KB, N, C, seed=seed + 1) * 2).to(dev())
    return x, mo, noise, rnd(KB, N, C, seed=seed + 3).to(dev()), rnd(KB, N, C, seed=seed + 4).to(dev())


def _masks(N, C):
    """all-free, all-given and random (about 30 % given; non-zero bytes of several values) (KB, N, C) uint8 masks."""
    g = torch.Generator().manual_seed(17)
    rand = torch.where(torch.rand((KB, N, C), generator=g) < 0.3, torch.randint(1, 256, (KB, N, C), generator=g), torch.zeros((), dtype=torch.int64))
    return {"free": torch.zeros((KB, N, C), dtype=torch.uint8, device=dev()), "given": torch.ones((KB, N, C), dtype=torch.uint8, device=dev()),
            "random": rand.to(torch.uint8).to(dev())}


def test_scale_set_and_shapes_are_the_ones_the_kernels_are_specified_on():
    assert KB == 3 and SHAPES == ((5, 7), (80, 62)) and SCALE_SET == (0.0, 1.0, 2.5, -0.5)
    assert [list(t) for t in T_SETS] == [[0, 0, 0], [1, 1, 1], [999, 999, 999], [0, 999, 17]]
    frac = float((_masks(80, 62)["random"] != 0).float().mean())
    assert 0.25 < frac < 0.35


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("mt,ca,cb", [(2, "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"),
                                      (0, "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"), (1, None, None)])
def test_p_sample_masked_cfg_is_cfg_combine_then_p_sample_masked(mt, ca, cb, clip):
    from diffuscene_amd import ops
    tb, d = _tables()
    sa, sb = d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"]
    k1, k2 = d["posterior_mean_coef1"], d["posterior_mean_coef2"]
    A, Bc = (d[ca] if ca else None), (d[cb] if cb else None)
    for N, C in SHAPES:
        x, mo, noise, known, nk = _operands(N, C, 500)
        for name, mask in _masks(N, C).items():
            given = mask != 0
            given2 = torch.cat([given, given])
            for shift in (0, 1):
                w = _scales(shift)
                for tv in T_SETS:
                    t = torch.tensor(tv, dtype=torch.int64, device=dev())
                    last = (t == 0)[:, None, None]
                    post = (t, A, Bc, k1, k2, d["sigma"])
                    args = post + (sa, sb, mt, clip)
                    what = (mt, clip, N, name, shift, tv)
                    want = ops.p_sample_masked(x, ops.cfg_combine(mo, w), noise, known, nk, mask, *args)
                    got = ops.p_sample_masked_cfg(x, mo, w, noise, known, nk, mask, *args)
                    assert torch.equal(got, want), what + (float((got - want).abs().max()),)
                    inplace, dup = x.clone(), torch.full_like(x, NAN)
                    assert ops.p_sample_masked_cfg(inplace, mo, w, noise, known, nk, mask, *args, out=inplace, x_dup=dup) is inplace
                    assert torch.equal(inplace, want) and torch.equal(dup, want), what
                    # NaN where a lane must not read: x_t / both halves of model_out / noise under the mask; known / noise_k outside it;
                    # noise_k everywhere at t == 0
                    got = ops.p_sample_masked_cfg(poisoned(x, given), poisoned(mo, given2), w, poisoned(noise, given), poisoned(known, ~given),
                                                  poisoned(nk, ~given | last), mask, *args)
                    assert torch.isfinite(got).all() and torch.equal(got, want), what
                    if name == "free":                               # nothing given: the guided step
                        assert torch.equal(got, ops.p_sample_cfg(x, mo, w, noise, *post, mt, clip)), what
                    # scale 0: the masked step on the null half
                    plain = ops.p_sample_masked(x, mo[KB:].contiguous(), noise, known, nk, mask, *args)
                    assert torch.equal(ops.p_sample_masked_cfg(x, mo, torch.zeros_like(w), noise, known, nk, mask, *args), plain), what


@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("mean_type", ["v", "eps", "x0"])
def test_ddim_masked_cfg_step_is_cfg_combine_then_ddim_masked_step(mean_type, eta):
    from diffuscene_amd import ops
    gd = _diffusion(mean_type)
    S = 50
    dtab = gd.ddim_tables(S, eta, dev())
    args = _step_args(gd, dtab)
    guided_args = args[:7] + args[9:]                                # ddim_cfg_step: the same run without (sqrt_ac, sqrt_1mac)
    for N, C in SHAPES:
        x, mo, noise, known, nk = _operands(N, C, 520)
        for name, mask in _masks(N, C).items():
            given = mask != 0
            given2 = torch.cat([given, given])
            everywhere = torch.ones_like(given)
            for shift in (0, 1):
                w = _scales(shift)
                for k in (0, S - 2, S - 1):
                    step = torch.tensor([k], dtype=torch.int64, device=dev())
                    last = dtab[0][k][1] < 0
                    assert last == (k == S - 1)
                    what = (mean_type, eta, N, name, shift, k)
                    want = ops.ddim_masked_step(x, ops.cfg_combine(mo, w), noise, known, nk, mask, step, *args)
                    got = ops.ddim_masked_cfg_step(x, mo, w, noise, known, nk, mask, step, *args)
                    assert torch.equal(got, want), what + (float((got - want).abs().max()),)
                    inplace, dup = x.clone(), torch.full_like(x, NAN)
                    assert ops.ddim_masked_cfg_step(inplace, mo, w, noise, known, nk, mask, step, *args, out=inplace, x_dup=dup) is inplace
                    assert torch.equal(inplace, want) and torch.equal(dup, want), what
                    # NaN where a lane must not read; on the last pair both noises everywhere
                    got = ops.ddim_masked_cfg_step(poisoned(x, given), poisoned(mo, given2), w, poisoned(noise, everywhere if last else given),
                                                   poisoned(known, ~given), poisoned(nk, everywhere if last else ~given), mask, step, *args)
                    assert torch.isfinite(got).all() and torch.equal(got, want), what
                    if name == "free":
                        assert torch.equal(got, ops.ddim_cfg_step(x, mo, w, noise, step, *guided_args)), what
                    plain = ops.ddim_masked_step(x, mo[KB:].contiguous(), noise, known, nk, mask, step, *args)
                    assert torch.equal(ops.ddim_masked_cfg_step(x, mo, torch.zeros_like(w), noise, known, nk, mask, step, *args), plain), what


def test_out_of_range_indices_are_clamped_and_counted_once():
    from diffuscene_amd import _lib, ops
    tb, d = _tables()
    sa, sb = d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"]
    N, C = SHAPES[1]                                                 # several blocks per scene: still one count per scene
    x, mo, noise, known, nk = _operands(N, C, 540)
    mask = _masks(N, C)["random"]
    w = _scales(0)
    args = (sa, sb, d["posterior_mean_coef1"], d["posterior_mean_coef2"], d["sigma"], sa, sb, 2, True)
    bad = torch.tensor([-2, 3, T_K + 4], dtype=torch.int64, device=dev())
    good = torch.tensor([0, 3, T_K - 1], dtype=torch.int64, device=dev())
    _lib.device_error_count(reset=True)
    got = ops.p_sample_masked_cfg(x, mo, w, noise, known, nk, mask, bad, *args)
    assert _lib.device_error_count(reset=True) == 2
    assert torch.equal(got, ops.p_sample_masked_cfg(x, mo, w, noise, known, nk, mask, good, *args))
    gd = _diffusion("v")
    S = 50
    dargs = _step_args(gd, gd.ddim_tables(S, 0.3, dev()))
    for bad_step, clamped in ((S + 7, S - 1), (-1, 0)):
        got = ops.ddim_masked_cfg_step(x, mo, w, noise, known, nk, mask, torch.tensor([bad_step], dtype=torch.int64, device=dev()), *dargs)
        assert _lib.device_error_count(reset=True) == 1              # one count per launch
        want = ops.ddim_masked_cfg_step(x, mo, w, noise, known, nk, mask, torch.tensor([clamped], dtype=torch.int64, device=dev()), *dargs)
        assert torch.equal(got, want)
    step = torch.tensor([7], dtype=torch.int64, device=dev())
    times, times_next = dargs[0].clone(), dargs[1].clone()
    times[7], times_next[7] = T_K + 5, T_K + 1
    got = ops.ddim_masked_cfg_step(x, mo, w, noise, known, nk, mask, step, times, times_next, *dargs[2:])
    assert _lib.device_error_count(reset=True) == 2
    times[7], times_next[7] = T_K - 1, T_K - 1
    assert torch.equal(got, ops.ddim_masked_cfg_step(x, mo, w, noise, known, nk, mask, step, times, times_next, *dargs[2:]))
    with pytest.raises(RuntimeError):
        ops.p_sample_masked_cfg(x, mo[:KB].contiguous(), w, noise, known, nk, mask, good, *args)        # model_out must hold 2 B scenes
    with pytest.raises(RuntimeError):
        ops.p_sample_masked_cfg(x, mo, w[:2].contiguous(), noise, known, nk, mask, good, *args)
    with pytest.raises(RuntimeError):
        ops.p_sample_masked_cfg(x, mo, w, noise, known[:2].contiguous(), nk, mask, good, *args)         # known / noise_k / mask at B
    with pytest.raises(RuntimeError):
        ops.p_sample_masked_cfg(x, mo, w, noise, known, nk, mask.bool(), good, *args)
    with pytest.raises(RuntimeError):
        ops.p_sample_masked_cfg(x, mo, w, noise, known, nk, mask, good, *args, out=x, x_dup=x)          # x_dup must not overlap x_t / out


# ------------------------------------------------------------------------------------------------------------------- the loops
T_LOOP, S_LOOP = 50, 10
LOOPS = (("inpaint_samples_guided", dict(clip_denoised=True), "_MaskedGuidedGraph"),
         ("inpaint_samples_guided_ddim", dict(sampling_timesteps=S_LOOP, ddim_sampling_eta=0.5), "_DDIMMaskedGuidedGraph"))
SHAPE = (GB, GN, GC)
_SHARED = {}


def _setup(tmp_path):
    """(model at T = 50, condition, condition_cross, known on the device, two masks, main buffer (T + 1 draws), known-draw buffer)."""
    m = build_model("v", T_LOOP, tmp_path)
    if "loop" not in _SHARED:
        cond, cross = _conditions(m, GB, case_texts())
        known = W.synth_scene_batch(GB, GN, 22, 32, 7)
        masks = (scene_masks(), scene_masks().roll(1, 0))
        main = torch.stack([rnd(*SHAPE, seed=600 + i) for i in range(T_LOOP + 1)]).to(dev())
        kn = torch.stack([rnd(*SHAPE, seed=700 + i) for i in range(T_LOOP)]).to(dev())
        _SHARED["loop"] = (cond, cross, known, masks, main, kn)
    return (m,) + _SHARED["loop"]


def _buffers(loop, main, kn):
    return (main, kn) if loop == "inpaint_samples_guided" else (main[:S_LOOP], kn[:S_LOOP])


def test_captured_loops_are_the_eager_loops_bit_for_bit_and_one_graph_serves_every_mask_and_scale(tmp_path):
    from diffuscene_amd import sampler
    from diffuscene_amd.scene_noise import SceneNoise
    m, cond, cross, known, masks, main, kn = _setup(tmp_path)
    diff = m.diffusion
    kd = known.to(dev())
    scale_sets = ((0.0, 1.5, 3.0), (2.0, -0.5, 1.0))
    for loop, kw, cls in LOOPS:
        bm, bk = _buffers(loop, main, kn)
        runs = {}
        for graph in (False, True):
            call = lambda **k: getattr(diff, loop)(SHAPE, dev(), condition=cond, condition_cross=cross, known=kd, graph=graph, **kw, **k)  # noqa: E731
            torch.manual_seed(2468)
            out = []
            with torch.no_grad():
                for mask, scale in zip(masks, scale_sets):           # seeded once: the second call continues the generator
                    out.append(call(mask=mask, guidance_scale=scale))
                    if graph:
                        (g,) = diff.diffusion._graphs.values()
                        out.append((g, g.scale.data_ptr(), g.mask.data_ptr(), g.known.data_ptr()))
                out.append(torch.cuda.get_rng_state(dev()))
                out.append(call(mask=masks[0], guidance_scale=scale_sets[0], noise_fn=sampler.RaggedNoiseReplay(bm, bk)))
                out.append(call(mask=masks[1], guidance_scale=scale_sets[0], noise_fn=SceneNoise([11, 2 ** 40 + 5, 11], dev())))
            runs[graph] = out
        (e1, e2, es, er, en), (g1, ga, g2, gb, gs, gr, gn) = runs[False], runs[True]
        assert torch.equal(e1, g1) and torch.equal(e2, g2), loop
        assert torch.equal(es, gs)                                   # the device generator ends in the same state
        assert torch.equal(er, gr) and torch.isfinite(gr).all(), loop        # through the replay buffers
        assert torch.equal(en, gn) and torch.isfinite(gn).all(), loop        # with per-scene seeds
        assert ga[0] is gb[0] and ga[1:] == gb[1:] and type(ga[0]).__name__ == cls      # one graph, one set of buffers
        for out, mask in ((g1, masks[0]), (g2, masks[1]), (gr, masks[0]), (gn, masks[1])):
            assert torch.equal(out.cpu()[mask], known[mask])         # the given elements come back bit-equal
        assert not torch.equal(g1, gr)
        if loop.endswith("ddim"):                                    # eta is not part of the key either
            seen = []
            with torch.no_grad():
                for eta in (0.5, 0.0):
                    diff.inpaint_samples_guided_ddim(SHAPE, dev(), condition=cond, condition_cross=cross, known=kd, mask=masks[0],
                                                     guidance_scale=1.0, graph=True, sampling_timesteps=S_LOOP, ddim_sampling_eta=eta)
                    seen.append(list(diff.diffusion._graphs.values()))
            assert len(seen[0]) == len(seen[1]) == 1 and seen[0][0] is seen[1][0]


def test_the_unfused_captured_step_is_the_fused_one(tmp_path):
    from diffuscene_amd import sampler
    m, cond, cross, known, masks, main, kn = _setup(tmp_path)
    diff, gd = m.diffusion, m.diffusion.diffusion
    with torch.no_grad():
        cond2, cross2, scale = gd._guided_inputs(SHAPE, dev(), cond, cross, SCALES, "test")
        kd, mk = gd._masked_inputs(SHAPE, dev(), known, masks[0], "test")
        for name, front, extra in (("T-step", sampler.graph_masked_guided_loop, (True, T_LOOP)),
                                   ("strided", sampler.graph_ddim_masked_guided_loop, (S_LOOP, 0.5))):
            bm, bk = (main, kn) if name == "T-step" else (main[:S_LOOP], kn[:S_LOOP])
            outs = []
            for fused in (True, False):
                outs.append(front(gd, diff._denoise, SHAPE, dev(), cond2, cross2, scale, *extra, noise_fn=sampler.RaggedNoiseReplay(bm, bk),
                                  known=kd, mask=mk, fused=fused))
                (g,) = gd._graphs.values()
                assert g.fused is fused and (g.m is None) == fused
            assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all(), name


def test_an_all_zero_mask_is_guided_generation_on_the_main_draws(tmp_path):
    from diffuscene_amd.sampler import NoiseReplay, RaggedNoiseReplay
    m, cond, cross, known, masks, main, kn = _setup(tmp_path)
    diff = m.diffusion
    zero = torch.zeros(SHAPE, dtype=torch.bool)
    common = dict(condition=cond, condition_cross=cross, guidance_scale=SCALES)
    with torch.no_grad():
        gen = diff.gen_samples_guided(SHAPE, dev(), noise_fn=NoiseReplay(main), clip_denoised=True, **common)
        got = diff.inpaint_samples_guided(SHAPE, dev(), noise_fn=RaggedNoiseReplay(main, kn), clip_denoised=True, known=known.to(dev()),
                                          mask=zero, **common)
        assert torch.equal(got, gen)
        strided = dict(sampling_timesteps=S_LOOP, ddim_sampling_eta=0.4)
        gen = diff.gen_samples_guided_ddim(SHAPE, dev(), noise_fn=NoiseReplay(main[:S_LOOP]), **strided, **common)
        got = diff.inpaint_samples_guided_ddim(SHAPE, dev(), noise_fn=RaggedNoiseReplay(main[:S_LOOP], kn[:S_LOOP]), known=known.to(dev()),
                                               mask=zero, **strided, **common)
        assert torch.equal(got, gen)


# ------------------------------------------------------------------------------------------------------------------- golden chains
@BOTH
@pytest.mark.parametrize("name", list(CASES))
def test_guided_masked_chain_matches_the_reference_within_four_times_its_sensitivity(name, golden_dir, tmp_path, gemm_arith):
    from diffuscene_amd.sampler import RaggedNoiseReplay
    g = np.load(os.path.join(golden_dir, "guided_inpaint.npz"))
    mt, T, S, eta, clip, seed = CASES[name]
    known, mask, main, kn = chain_inputs(name)
    m = build_model(mt, T, tmp_path)
    cond, cross = _conditions(m, GB, case_texts())
    replay = RaggedNoiseReplay(main.to(dev()), kn.to(dev()))
    common = dict(condition=cond, condition_cross=cross, guidance_scale=SCALES, noise_fn=replay, known=known.to(dev()), mask=mask, graph=True)
    with torch.no_grad():
        if S is None:
            y = m.diffusion.inpaint_samples_guided(SHAPE, dev(), clip_denoised=clip, **common)
        else:
            y = m.diffusion.inpaint_samples_guided_ddim(SHAPE, dev(), sampling_timesteps=S, ddim_sampling_eta=eta, **common)
    assert torch.equal(y.cpu()[mask], known[mask])                   # the given elements come back bit-equal
    r, ew = distance(y.cpu(), g[name])
    sr, sew = (float(v) for v in g[name + ".sens"])
    br, bew = max(5e-6, 4 * sr), max(1e-4, 4 * sew)
    line = "guided in-painting %s %s: norm-relative %.3g (bound %.3g), element-wise %.3g (bound %.3g)" % (name, gemm_arith, r, br, ew, bew)
    print(line)
    if os.environ.get("DSC_PARITY_LOG"):
        with open(os.environ["DSC_PARITY_LOG"], "a") as f:
            f.write(line + "\n")
    assert r < br and ew < bew, line


# ------------------------------------------------------------------------------------------------------------------- the public interface
@pytest.mark.parametrize("strided", [False, True])
def test_inpaint_scene_batched_with_guidance_scale(strided, tmp_path, monkeypatch):
    from diffuscene_amd import sampler
    monkeypatch.delenv("DSC_GRAPH", raising=False)
    calls = []
    for fn in ("graph_masked_guided_loop", "graph_ddim_masked_guided_loop", "graph_masked_loop", "graph_ddim_masked_loop"):
        monkeypatch.setattr(sampler, fn, lambda *a, _f=getattr(sampler, fn), _n=fn, **k: (calls.append(_n), _f(*a, **k))[1])
    m = build_model("v", T_LOOP, tmp_path)
    x = W.synth_scene_batch(GB, GN, 22, 32, 9)
    mask = scene_masks()
    room = torch.zeros(GB, 1, 64, 64, device=dev())
    kw = dict(sampling_timesteps=7, ddim_sampling_eta=0.5) if strided else dict(clip_denoised=True)
    with QUIET():
        torch.manual_seed(21)
        scenes = m.inpaint_scene_batched(room, GN, GC, x.to(dev()), mask, text=case_texts(), guidance_scale=[0, 1.5, 3], keep_empty=True, **kw)
        seeded = [m.inpaint_scene_batched(room, GN, GC, x.to(dev()), mask, text=case_texts(), guidance_scale=2.0, keep_empty=True,
                                          scene_seeds=[5, 6, 7], **kw) for _ in range(2)]
    assert calls == ["graph_ddim_masked_guided_loop" if strided else "graph_masked_guided_loop"] * 3
    assert len(scenes) == GB and len(seeded[0]) == GB
    spans = {"translations": (0, 3), "sizes": (3, 6), "angles": (6, 8), "class_labels": (8, 29), "objfeats": (30, 62)}
    for b, d in enumerate(scenes):
        assert sorted(d) == sorted(spans)
        for k, (lo, hi) in spans.items():
            v = d[k]
            assert v.device.type == "cpu" and tuple(v.shape) == (1, GN, hi - lo) and torch.isfinite(v).all()
            sel = mask[b, :, lo:hi]
            assert torch.equal(v[0][sel], x[b, :, lo:hi][sel]), (b, k)    # known elements come back bit-equal to ``boxes``
            assert torch.equal(seeded[0][b][k], seeded[1][b][k])          # seeded: the same scenes again
    assert any(not torch.equal(scenes[0][k], scenes[1][k]) for k in spans)


@pytest.mark.parametrize("strided", [False, True])
def test_guidance_scale_none_is_the_call_as_it_was(strided, tmp_path, monkeypatch):
    monkeypatch.delenv("DSC_GRAPH", raising=False)
    m = build_model("v", T_LOOP, tmp_path)
    x = W.synth_scene_batch(GB, GN, 22, 32, 9).to(dev())
    mask = scene_masks()
    room = torch.zeros(GB, 1, 64, 64, device=dev())
    kw = dict(sampling_timesteps=7, ddim_sampling_eta=0.5) if strided else dict(clip_denoised=True)
    outs, states = [], []
    with QUIET():
        for extra in ({}, dict(guidance_scale=None)):
            torch.manual_seed(31)
            outs.append(m.inpaint_scene_batched(room, GN, GC, x, mask, text=case_texts(), keep_empty=True, **kw, **extra))
            states.append((torch.cuda.get_rng_state(dev()), torch.get_rng_state()))
            (g,) = m.diffusion.diffusion._graphs.values()
            assert type(g).__name__ == ("_DDIMMaskedGraph" if strided else "_MaskedGraph")
        # and it is what the loop underneath returns for the same seed: the keyword added nothing in front of it
        torch.manual_seed(31)
        torch.randn((GB, GN, GC))
        cond, cross = m._sampling_conditions(room, GN, dev(), text=case_texts())
        loop = m.diffusion.inpaint_samples_ddim if strided else m.diffusion.inpaint_samples
        raw = loop((GB, GN, GC), dev(), condition=cond, condition_cross=cross, known=x, mask=mask, **kw)
        want = m.delete_empty_per_scene(raw, keep_empty=True)
    for a, b, c in zip(outs[0], outs[1], want):
        assert sorted(a) == sorted(b) == sorted(c)
        assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in a)
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])
