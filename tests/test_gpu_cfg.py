"""GPU: classifier-free guidance on the text path (p_sample_loop_guided / ddim_guided_loop), ``guidance_scale`` on the public entry points
and the text-condition dropout of training (``text_drop_prob``).

* kernels: dsc_p_sample_cfg_f32 / dsc_ddim_cfg_step_f32 against dsc_cfg_combine_f32 followed by the existing step (torch.equal), in place
  and out of place, with and without x_dup / x0_out, noise poisoned where it must not be read, scale 0 against the plain step on the null
  half, out-of-range indices clamped and counted; dsc_scene_gate_f32 forward and backward against torch.where;
* the captured loops against the eager ones bit for bit under a seed and through NoiseReplay, one graph for every mix of scales;
* reference chains: tests/golden/cfg.npz (tools/make_golden_cfg.py: the REAL reference's loops around the bridged guided denoiser) under
  both GEMM arithmetics.  Bound per chain: the larger of the project's chain criterion (5e-6 norm-relative / 1e-4 element-wise with the
  5 % range floor, tests/test_gpu_wide.py) and 4 x the chain's stored reference sensitivity (reference float32 against a float64 run of
  the same chain): the HIP path is another f32 realisation of the chain with another summation order in every GEMM, two such
  realisations can differ by twice their distance from f64, doubled again for the second arithmetic;
* the gated training loss against the reference's get_loss_iter on gated features, and exact zeros for dropped scenes;
* generate_layout / generate_layout_batched with ``guidance_scale``."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import weights as W  # noqa: E402
from oracle.make_golden_wrapper import fake_bert_features, network_config, wrapper_batch, wrapper_state_dict  # noqa: E402
from tools.make_golden_cfg import B as GB, C as GC, CASES, N as GN, SCALES, SEED_TRAIN, TRAIN_KEEP, GRAD_ROWS, case_texts, chain_noise, distance  # noqa: E402

from test_gpu_complete_ragged import _tables, dev, rnd  # noqa: E402
from test_gpu_wrapper import cpu_rng  # noqa: E402,F401  (fixture)

BOTH = pytest.mark.parametrize("gemm_arith", ["split", "f32"], indirect=True)
QUIET = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731
NAN = float("nan")
KB = 3
SHAPES = ((5, 7), (80, 62))          # inner 35: the tail is shorter than one wave; inner 4960: several blocks per scene
SCALE_SET = (0.0, 1.0, 2.5, -0.5)
T_K = 1000
T_SETS = ([0] * KB, [1] * KB, [T_K - 1] * KB, [0, 999, 17])


@pytest.fixture(autouse=True)
def no_device_errors():
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    yield
    assert _lib.device_error_count(reset=True) == 0


def _scales(shift):
    return torch.tensor([SCALE_SET[(b + shift) % 4] for b in range(KB)], dtype=torch.float32, device=dev())


def _operands(N, C, seed):
    x = rnd(KB, N, C, seed=seed).to(dev())
    mo = (rnd(2 * KB, N, C, seed=seed + 1) * 2).to(dev())
    noise = rnd(KB, N, C, seed=seed + 2).to(dev())
    return x, mo, noise


# ------------------------------------------------------------------------------------------------------------------- kernels
def test_cfg_combine_is_the_three_rounded_ops():
    from diffuscene_amd import ops
    for N, C in SHAPES:
        _, mo, _ = _operands(N, C, 300)
        for shift in (0, 1):
            w = _scales(shift)
            c, u = mo[:KB], mo[KB:]
            want = u + w[:, None, None] * (c - u)
            got = ops.cfg_combine(mo, w)
            assert torch.equal(got, want), (N, C, shift)
            assert torch.equal(ops.cfg_combine(mo, torch.zeros_like(w)), u)
            assert float((ops.cfg_combine(mo, torch.ones_like(w)) - c).abs().max()) <= 1e-6 * float(c.abs().max())


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("mt,ca,cb", [(2, "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"),
                                      (0, "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"), (1, None, None)])
def test_p_sample_cfg_is_cfg_combine_then_p_sample(mt, ca, cb, clip):
    from diffuscene_amd import ops
    tb, d = _tables()
    k1, k2 = d["posterior_mean_coef1"], d["posterior_mean_coef2"]
    A, Bc = (d[ca] if ca else None), (d[cb] if cb else None)
    for N, C in SHAPES:
        x, mo, noise = _operands(N, C, 310)
        for shift in (0, 1):
            w = _scales(shift)
            for tv in T_SETS:
                t = torch.tensor(tv, dtype=torch.int64, device=dev())
                args = (t, A, Bc, k1, k2, d["sigma"], mt, clip)
                x0_want = torch.empty_like(x)
                want = ops.p_sample(x, ops.cfg_combine(mo, w), noise, *args, x0_out=x0_want)
                got = ops.p_sample_cfg(x, mo, w, noise, *args)
                assert torch.equal(got, want), (mt, clip, N, shift, tv, float((got - want).abs().max()))
                inplace, dup, x0 = x.clone(), torch.full_like(x, NAN), torch.full_like(x, NAN)
                assert ops.p_sample_cfg(inplace, mo, w, noise, *args, out=inplace, x_dup=dup, x0_out=x0) is inplace
                assert torch.equal(inplace, want) and torch.equal(dup, want) and torch.equal(x0, x0_want), (mt, clip, N, shift, tv)
                # at t == 0 sigma is forced to 0 and the noise is not read
                zero = (t == 0)[:, None, None]
                got = ops.p_sample_cfg(x, mo, w, torch.where(zero, torch.full_like(noise, NAN), noise), *args)
                assert torch.isfinite(got).all() and torch.equal(got, want), (mt, clip, N, shift, tv)
                # scale 0: the plain step on the null half
                plain = ops.p_sample(x, mo[KB:].contiguous(), noise, *args)
                assert torch.equal(ops.p_sample_cfg(x, mo, torch.zeros_like(w), noise, *args), plain), (mt, clip, N, tv)


def _diffusion(mean_type="v", T_=T_K):
    from diffuscene_amd.networks.diffusion_ddpm import GaussianDiffusion, get_betas
    return GaussianDiffusion(dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32), get_betas("linear", 1e-4, 0.02, T_),
                             "mse", mean_type, "fixedsmall", False, False, None)


def _ddim_args(gd, dtab):
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    _, times, times_next, coef = dtab
    return (times, times_next, coef, ca, cb, tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"],
            {"eps": 0, "x0": 1, "v": 2}[gd.model_mean_type])


@pytest.mark.parametrize("eta", [0.0, 0.7])
@pytest.mark.parametrize("mean_type", ["v", "eps", "x0"])
def test_ddim_cfg_step_is_cfg_combine_then_ddim_step(mean_type, eta):
    from diffuscene_amd import ops
    gd = _diffusion(mean_type)
    S = 50
    dtab = gd.ddim_tables(S, eta, dev())
    args = _ddim_args(gd, dtab)
    for N, C in SHAPES:
        x, mo, noise = _operands(N, C, 320)
        for shift in (0, 1):
            w = _scales(shift)
            for k in (0, S - 2, S - 1):
                step = torch.tensor([k], dtype=torch.int64, device=dev())
                last = dtab[0][k][1] < 0
                assert last == (k == S - 1)
                x0_want = torch.empty_like(x)
                want = ops.ddim_step(x, ops.cfg_combine(mo, w), noise, step, *args, x0_out=x0_want)
                got = ops.ddim_cfg_step(x, mo, w, noise, step, *args)
                assert torch.equal(got, want), (mean_type, eta, N, shift, k, float((got - want).abs().max()))
                inplace, dup, x0 = x.clone(), torch.full_like(x, NAN), torch.full_like(x, NAN)
                assert ops.ddim_cfg_step(inplace, mo, w, noise, step, *args, out=inplace, x_dup=dup, x0_out=x0) is inplace
                assert torch.equal(inplace, want) and torch.equal(dup, want) and torch.equal(x0, x0_want), (mean_type, eta, N, shift, k)
                if last:                                             # the last pair takes x_start: the noise is not read
                    got = ops.ddim_cfg_step(x, mo, w, torch.full_like(noise, NAN), step, *args)
                    assert torch.isfinite(got).all() and torch.equal(got, want), (mean_type, eta, N, shift)
                plain = ops.ddim_step(x, mo[KB:].contiguous(), noise, step, *args)
                assert torch.equal(ops.ddim_cfg_step(x, mo, torch.zeros_like(w), noise, step, *args), plain), (mean_type, eta, N, k)


def test_out_of_range_indices_are_clamped_and_counted_not_faulted():
    from diffuscene_amd import _lib, ops
    tb, d = _tables()
    N, C = SHAPES[1]                                                     # several blocks per scene: still one count per scene
    x, mo, noise = _operands(N, C, 330)
    w = _scales(0)
    args = (d["sqrt_alphas_cumprod"], d["sqrt_one_minus_alphas_cumprod"], d["posterior_mean_coef1"], d["posterior_mean_coef2"], d["sigma"], 2, True)
    bad = torch.tensor([-2, 3, T_K + 4], dtype=torch.int64, device=dev())
    good = torch.tensor([0, 3, T_K - 1], dtype=torch.int64, device=dev())
    assert _lib.device_error_count() == 0
    got = ops.p_sample_cfg(x, mo, w, noise, bad, *args)
    assert _lib.device_error_count(reset=True) == 2
    assert torch.equal(got, ops.p_sample_cfg(x, mo, w, noise, good, *args))
    gd = _diffusion("v")
    S = 50
    dargs = _ddim_args(gd, gd.ddim_tables(S, 0.3, dev()))
    for bad_step, clamped in ((S + 7, S - 1), (-1, 0)):
        got = ops.ddim_cfg_step(x, mo, w, noise, torch.tensor([bad_step], dtype=torch.int64, device=dev()), *dargs)
        assert _lib.device_error_count(reset=True) == 1                  # one count per launch
        assert torch.equal(got, ops.ddim_cfg_step(x, mo, w, noise, torch.tensor([clamped], dtype=torch.int64, device=dev()), *dargs))
    step = torch.tensor([7], dtype=torch.int64, device=dev())
    times = dargs[0].clone()
    times[7] = T_K + 5
    got = ops.ddim_cfg_step(x, mo, w, noise, step, times, *dargs[1:])
    assert _lib.device_error_count(reset=True) == 1
    times[7] = T_K - 1
    assert torch.equal(got, ops.ddim_cfg_step(x, mo, w, noise, step, times, *dargs[1:]))
    with pytest.raises(RuntimeError):
        ops.p_sample_cfg(x, mo[:KB].contiguous(), w, noise, good, *args)            # model_out must hold 2 B scenes
    with pytest.raises(RuntimeError):
        ops.p_sample_cfg(x, mo, w[:2].contiguous(), noise, good, *args)
    with pytest.raises(RuntimeError):
        ops.p_sample_cfg(x, mo, w, noise, good, *args, out=x, x_dup=x)              # x_dup must not overlap x_t / out


def test_scene_gate_forward_and_backward_against_where():
    from diffuscene_amd import ops
    from diffuscene_amd.autograd_ops import SceneGateFn
    Bq, L, D = 4, 3, 5
    keep = torch.tensor([True, False, True, False], device=dev())
    sel = keep[:, None, None]
    x = rnd(Bq, L, D, seed=340).to(dev())
    dy = rnd(Bq, L, D, seed=341).to(dev())
    xp = torch.where(sel, x, torch.full_like(x, NAN)).requires_grad_(True)          # NaN in the dropped scenes' rows ...
    dyp = torch.where(sel, dy, torch.full_like(dy, NAN))                            # ... and in their incoming gradient
    y = SceneGateFn.apply(xp, keep)
    assert torch.equal(y, torch.where(sel, x, torch.zeros_like(x)))
    y.backward(dyp)
    assert torch.equal(xp.grad, torch.where(sel, dy, torch.zeros_like(dy)))
    assert torch.equal(ops.scene_gate(x, keep.to(torch.uint8) * 255), torch.where(sel, x, torch.zeros_like(x)))
    assert torch.equal(ops.scene_gate(x, torch.ones(Bq, dtype=torch.bool, device=dev())), x)
    assert not ops.scene_gate(xp.detach(), torch.zeros(Bq, dtype=torch.bool, device=dev())).any()
    with pytest.raises(RuntimeError):
        ops.scene_gate(x, keep[:3])
    with pytest.raises(RuntimeError):
        ops.scene_gate(x, keep.float())


# ------------------------------------------------------------------------------------------------------------------- the model
_MODELS = {}


class _FakeBertCache:
    def batch(self, texts, device):
        return fake_bert_features(list(texts)).to(device)


def build_model(mt, T, tmp_path, zero_text=False, tag=None, **extra):
    """The text wrapper on the device with seeded parameters (cached per argument set; ``tag`` only separates cache entries);
    ``zero_text``: fc_text_f zeroed, i.e. condition_cross == 0."""
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    key = (mt, T, zero_text, tag, tuple(sorted(extra.items())))
    if key not in _MODELS:
        stats = tmp_path / "dataset_stats.txt"
        stats.write_text(json.dumps(W.DATASET_STATS))
        cfg = network_config("text", str(stats), T)
        cfg["diffusion_kwargs"]["model_mean_type"] = mt
        cfg["text_bert_cached"] = True
        cfg.update(extra)
        with QUIET():
            m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
        sd = wrapper_state_dict(m)
        if zero_text:
            sd["fc_text_f.weight"], sd["fc_text_f.bias"] = torch.zeros_like(sd["fc_text_f.weight"]), torch.zeros_like(sd["fc_text_f.bias"])
        m.load_state_dict(sd)
        m.attach_bert_cache(_FakeBertCache())
        _MODELS[key] = m.to(dev()).eval()
    return _MODELS[key]


def _conditions(m, batch, texts):
    room = torch.zeros(batch, 1, 64, 64, device=dev())
    with torch.no_grad(), QUIET():
        return m._sampling_conditions(room, GN, dev(), text=texts)


# ------------------------------------------------------------------------------------------------------------------- graph against eager
def test_captured_guided_loops_are_the_eager_loops_bit_for_bit(tmp_path):
    from diffuscene_amd.sampler import NoiseReplay, _DDIMGuidedGraph, _GuidedStepGraph, _StepGraph
    m = build_model("v", 50, tmp_path)
    diff = m.diffusion
    shape = (GB, GN, GC)
    cond, cross = _conditions(m, GB, case_texts())
    T, S = 50, 10
    buf = torch.stack([rnd(*shape, seed=400 + i) for i in range(T + 1)]).to(dev())
    for loop, kw, cls, n in (("gen_samples_guided", dict(clip_denoised=True), _GuidedStepGraph, T + 1),
                             ("gen_samples_guided_ddim", dict(sampling_timesteps=S, ddim_sampling_eta=0.5), _DDIMGuidedGraph, S)):
        runs = {}
        for graph in (False, True):
            torch.manual_seed(4321)
            out = []
            with torch.no_grad():
                for scale in ((0.0, 1.5, 3.0), (2.0, -0.5, 1.0)):       # seeded once: the second call continues the generator
                    out.append(getattr(diff, loop)(shape, dev(), condition=cond, condition_cross=cross, guidance_scale=scale,
                                                   graph=graph, **kw))
                    if graph:
                        (g,) = diff.diffusion._graphs.values()
                        out.append((g, g.scale.data_ptr()))
                out.append(torch.cuda.get_rng_state(dev()))
                out.append(getattr(diff, loop)(shape, dev(), condition=cond, condition_cross=cross, guidance_scale=(0.0, 1.5, 3.0),
                                               noise_fn=NoiseReplay(buf[:n]), graph=graph, **kw))
            runs[graph] = out
        (e1, e2, es, er), (g1, ga, g2, gb, gs, gr) = runs[False], runs[True]
        assert torch.equal(e1, g1) and torch.equal(e2, g2), loop
        assert torch.equal(es, gs)                                       # the device generator ends in the same state
        assert torch.equal(er, gr) and torch.isfinite(gr).all(), loop    # through NoiseReplay too
        assert ga[0] is gb[0] and ga[1] == gb[1] and isinstance(ga[0], cls)     # one graph, one scale buffer for both scale vectors
    # guidance_scale=None afterwards: the ordinary graph
    with torch.no_grad():
        diff.gen_samples(shape, dev(), condition=cond, condition_cross=cross, clip_denoised=True, graph=True)
    (g,) = diff.diffusion._graphs.values()
    assert type(g) is _StepGraph and g.plan.B == GB


def test_scale_one_is_the_conditional_model_up_to_rounding(tmp_path):
    """The unclipped T-step loop (nothing hides behind a clamp): u + 1 * (c - u) is c up to one rounding per element and step."""
    from diffuscene_amd.sampler import NoiseReplay
    m = build_model("v", 50, tmp_path)
    shape = (GB, GN, GC)
    cond, cross = _conditions(m, GB, case_texts())
    buf = torch.stack([rnd(*shape, seed=450 + i) for i in range(51)]).to(dev())
    with torch.no_grad():
        plain = m.diffusion.gen_samples(shape, dev(), condition=cond, condition_cross=cross, noise_fn=NoiseReplay(buf), clip_denoised=False)
        one = m.diffusion.gen_samples_guided(shape, dev(), condition=cond, condition_cross=cross, guidance_scale=1.0,
                                             noise_fn=NoiseReplay(buf), clip_denoised=False)
        two = m.diffusion.gen_samples_guided(shape, dev(), condition=cond, condition_cross=cross, guidance_scale=2.0,
                                             noise_fn=NoiseReplay(buf), clip_denoised=False)
    r, ew = distance(one, plain)
    r2, _ = distance(two, plain)
    print("scale 1 vs the conditional model, T = 50 unclipped: norm-relative %.3g, element-wise %.3g (scale 2: %.3g)" % (r, ew, r2))
    assert r < 1e-4 and ew < 1e-4                                       # the project's chain criterion (tests/test_gpu_wide.py)
    assert r2 > 10 * 1e-4                                               # and another scale moves the result well beyond that criterion


# ------------------------------------------------------------------------------------------------------------------- golden chains
@BOTH
@pytest.mark.parametrize("name", list(CASES))
def test_guided_chain_matches_the_reference_within_four_times_its_sensitivity(name, golden_dir, tmp_path, gemm_arith):
    from diffuscene_amd.sampler import NoiseReplay
    g = np.load(os.path.join(golden_dir, "cfg.npz"))
    mt, T, S, eta, clip, seed = CASES[name]
    m = build_model(mt, T, tmp_path)
    shape = (GB, GN, GC)
    cond, cross = _conditions(m, GB, case_texts())
    replay = NoiseReplay(chain_noise(name).to(dev()))
    with torch.no_grad():
        if S is None:
            y = m.diffusion.gen_samples_guided(shape, dev(), condition=cond, condition_cross=cross, guidance_scale=SCALES, noise_fn=replay,
                                               clip_denoised=clip, graph=True)
        else:
            y = m.diffusion.gen_samples_guided_ddim(shape, dev(), condition=cond, condition_cross=cross, guidance_scale=SCALES,
                                                    noise_fn=replay, sampling_timesteps=S, ddim_sampling_eta=eta, graph=True)
    r, ew = distance(y.cpu(), g[name])
    sr, sew = (float(v) for v in g[name + ".sens"])
    br, bew = max(5e-6, 4 * sr), max(1e-4, 4 * sew)
    line = "guided %s %s: norm-relative %.3g (bound %.3g), element-wise %.3g (bound %.3g)" % (name, gemm_arith, r, br, ew, bew)
    print(line)
    if os.environ.get("DSC_PARITY_LOG"):
        with open(os.environ["DSC_PARITY_LOG"], "a") as f:
            f.write(line + "\n")
    assert r < br and ew < bew, line


# ------------------------------------------------------------------------------------------------------------------- training
def _train_batch():
    s, _ = wrapper_batch("text")
    s["desc_bert"] = fake_bert_features(s["description"])
    return {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in s.items()}


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("path", ["autograd", "plan"])
def test_gated_training_loss_and_text_gradients_match_the_reference(path, golden_dir, tmp_path, cpu_rng):  # noqa: F811
    """Loss and parts within the training tolerance of tests/test_gpu_train.py (1e-4), the fc_text_f gradients within its gradient
    tolerance against the reference (1e-4 norm-relative on the committed slices); a batch with every scene dropped leaves
    fc_text_f.weight.grad exactly zero."""
    from diffuscene_amd.train_step import loss_step, plan_supported
    g = np.load(os.path.join(golden_dir, "cfg.npz"))
    m = build_model("v", 1000, tmp_path, tag=path, text_drop_prob=0.25)      # the plan re-homes the parameters: one model per path
    m.train()
    try:
        def run(keep):
            s = dict(_train_batch(), _cond_keep=torch.tensor(keep))
            torch.manual_seed(SEED_TRAIN)
            if path == "plan":
                assert plan_supported(m)
                loss, parts, _ = loss_step(m, s, backward=True)
            else:
                m.zero_grad(set_to_none=True)
                loss, parts = m.get_loss(s)
                loss.backward()
            return loss, parts

        loss, parts = run(TRAIN_KEEP)
        want = float(g["train.loss"])
        print("%s: loss %.7f, reference %.7f" % (path, float(loss.detach()), want))
        assert abs(float(loss.detach()) - want) <= 1e-4 * abs(want)
        keys = [k[len("train.part."):] for k in g.files if k.startswith("train.part.")]
        assert keys and sorted(parts) == sorted(keys)
        for k in keys:
            w = float(g["train.part." + k])
            assert abs(float(parts[k]) - w) <= 1e-4 * max(1.0, abs(w)), (k, float(parts[k]), w)
        gw, gb = m.fc_text_f.weight.grad, m.fc_text_f.bias.grad
        rw, rb = _rel(gw[list(GRAD_ROWS)], g["train.grad.fc_text_f.weight"]), _rel(gb, g["train.grad.fc_text_f.bias"])
        print("%s: fc_text_f gradient rel err: weight rows %.3g, bias %.3g" % (path, rw, rb))
        assert rw < 1e-4 and rb < 1e-4
        run((False,) * len(TRAIN_KEEP))
        assert m.fc_text_f.weight.grad is not None and not m.fc_text_f.weight.grad.any()
        assert not m.fc_text_f.bias.grad.any()
    finally:
        m.eval()


def test_text_drop_prob_draws_once_in_training_mode_only(tmp_path):
    m = build_model("v", 1000, tmp_path, text_drop_prob=0.5)
    plain = build_model("v", 1000, tmp_path)
    s = _train_batch()
    Bt = len(TRAIN_KEEP)

    def after(model, train):
        model.train(train)
        try:
            torch.manual_seed(7)
            with torch.no_grad():
                cross = model._loss_inputs(s)[2]
            return cross, torch.cuda.get_rng_state(dev())
        finally:
            model.eval()

    base, s0 = after(plain, True)
    ev, s1 = after(m, False)
    assert torch.equal(s0, s1) and torch.equal(base, ev)                     # eval mode: no draw, nothing changes
    tr, s2 = after(m, True)
    torch.manual_seed(7)
    u = torch.rand((Bt,), device=dev())
    assert torch.equal(s2, torch.cuda.get_rng_state(dev()))                  # exactly one (B,) draw
    keep = u >= 0.5
    assert torch.equal(tr, torch.where(keep[:, None, None], base, torch.zeros_like(base)))


# ------------------------------------------------------------------------------------------------------------------- public entry points
def test_public_entry_points_with_guidance_scale(golden_dir, tmp_path, monkeypatch):
    from diffuscene_amd import sampler
    monkeypatch.delenv("DSC_GRAPH", raising=False)
    calls = []
    for fn in ("graph_guided_loop", "graph_ddim_guided_loop", "graph_sample_loop", "graph_ddim_sample_loop"):
        monkeypatch.setattr(sampler, fn, lambda *a, _f=getattr(sampler, fn), _n=fn, **k: (calls.append(_n), _f(*a, **k))[1])
    m = build_model("v", 1000, tmp_path)
    zero = build_model("v", 1000, tmp_path, zero_text=True)
    from oracle.make_golden_wrapper import texts
    text = texts()
    C = GC
    room = torch.zeros(4, 1, 64, 64, device=dev())
    g = np.load(os.path.join(golden_dir, "wrapper.npz"))
    keys = sorted(k[len("text.layout."):] for k in g.files if k.startswith("text.layout."))
    with QUIET():
        torch.manual_seed(3)
        plain_one = m.generate_layout(room[:1], GN, C, batch_size=1, text=text[:1], clip_denoised=True, sampling_timesteps=20)
        d = m.generate_layout(room[:1], GN, C, batch_size=1, text=text[:1], clip_denoised=True, sampling_timesteps=20, guidance_scale=2.0)
        torch.manual_seed(5)
        scenes = m.generate_layout_batched(room, GN, C, 4, text=text, guidance_scale=[0, 1, 2, 3], sampling_timesteps=50, keep_empty=True)
        torch.manual_seed(5)
        null = zero.generate_layout_batched(room, GN, C, 4, text=text, sampling_timesteps=50, keep_empty=True)
    assert calls == ["graph_ddim_sample_loop", "graph_ddim_guided_loop", "graph_ddim_guided_loop", "graph_ddim_sample_loop"]
    assert sorted(d) == sorted(plain_one) == keys
    for k, v in d.items():
        assert v.device.type == "cpu" and v.shape[0] == 1 and tuple(v.shape[2:]) == tuple(plain_one[k].shape[2:])
        assert torch.isfinite(v).all()
    assert len(scenes) == 4
    for sc, ref in zip(scenes, null):
        assert sorted(sc) == keys
        for k in keys:
            assert tuple(sc[k].shape) == tuple(ref[k].shape) and torch.isfinite(sc[k]).all()
    # scene 0 runs at scale 0: the model whose text features are zeroed, up to the per-step parity tolerance (another batch size)
    for k in keys:
        r, ew = distance(scenes[0][k], null[0][k])
        print("scale 0 vs zeroed text features, %s: norm-relative %.3g, element-wise %.3g" % (k, r, ew))
        assert r < 1e-4 and ew < 1e-4, (k, r, ew)
    # the T-step guided call through generate_layout (T = 1000 replays of one captured step)
    with QUIET():
        d = m.generate_layout(room[:1], GN, C, batch_size=1, text=text[:1], clip_denoised=True, guidance_scale=2.0)
    assert calls[-1] == "graph_guided_loop" and sorted(d) == keys and all(torch.isfinite(v).all() for v in d.values())
