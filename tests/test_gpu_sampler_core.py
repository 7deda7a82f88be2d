"""GPU: what the eight captured loops share (sampler._LoopGraph and its two layers) and what the ten step entry points share (the
step_kernel template of csrc/diffusion.hip and its device helpers), at the shapes where the shared code can go wrong and no per-feature
test looks.

* the capture path at its edge step counts: every loop at 1 and 2 steps -- with one step the step graph is never replayed (the strided
  loops have none), only the standalone overwrite and ``final`` run -- eager, then graph (capturing), then graph (cached) under one
  seed: equal outputs, equal generator state afterwards (capture costs no random numbers), one live graph, reused;
* the grid-stride loop of the step kernels: the grid is capped at 64 blocks of 256 threads, so a scene of more than 16384 elements is the
  smallest at which a thread takes a second element (260 x 65 = 16900), next to one of 3 x 37 = 111 (less than one block, odd);
  every fused kernel against the composition of the unfused ops, p_sample and ddim_step against the fp32 CPU expression, torch.equal;
* which kernel reads the noise at t == 0 / on the last pair, with infinite noise.

A one-step T-step loop cannot come from time_num = 1 (GaussianDiffusion cannot tabulate a one-row schedule: its fixedlarge row is
empty); it is a two-row schedule with num_timesteps = 1 -- the difference keep_running is about -- and keep_running=True walks both rows."""
import contextlib
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_cfg import GC, GN, _conditions, _ddim_args, build_model, case_texts  # noqa: E402
from test_gpu_complete_ragged import dev, rnd  # noqa: E402
from test_gpu_masked import _diffusion, _step_args  # noqa: E402

QUIET = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731
INF = float("inf")
MT = {"eps": 0, "x0": 1, "v": 2}


@pytest.fixture(autouse=True)
def no_device_errors():
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    yield
    assert _lib.device_error_count(reset=True) == 0


# ------------------------------------------------------------------------------------------------------------------- the capture path
B, T_STRIDED = 2, 50
#         entry point                      class                 strided
LOOPS = {"gen_samples": ("_StepGraph", False),
         "gen_samples_ddim": ("_DDIMGraph", True),
         "complete_samples_ragged": ("_RaggedCompleteGraph", False),
         "complete_samples_ragged_ddim": ("_DDIMCompleteGraph", True),
         "inpaint_samples": ("_MaskedGraph", False),
         "inpaint_samples_ddim": ("_DDIMMaskedGraph", True),
         "gen_samples_guided": ("_GuidedStepGraph", False),
         "gen_samples_guided_ddim": ("_DDIMGuidedGraph", True),
         "inpaint_samples_guided": ("_MaskedGuidedGraph", False),
         "inpaint_samples_guided_ddim": ("_DDIMMaskedGuidedGraph", True),
         "complete_samples": ("_StepGraph", False),                             # the dense prefix: the unfused overwrite in the step
         "complete_samples_ragged/Pmax5": ("_RaggedCompleteGraph", False),      # Pmax < N: the given stream's shape is not the state's
         "complete_samples_ragged_ddim/Pmax5": ("_DDIMCompleteGraph", True)}
PMAX = 5


def _loop_kwargs(loop, strided, steps, shape):
    _, N, C = shape
    kw = dict(sampling_timesteps=steps, ddim_sampling_eta=0.5) if strided else dict(clip_denoised=True, keep_running=steps == 2)
    given = rnd(*shape, seed=501).clamp(-1, 1).to(dev())
    if loop == "complete_samples":
        kw.update(partial_boxes=given[:, :PMAX].contiguous())
    elif loop.endswith("/Pmax5"):
        kw.update(partial_boxes=given[:, :PMAX].contiguous(), num_partial=[0, PMAX])
    elif loop.startswith("complete"):
        kw.update(partial_boxes=given, num_partial=[0, 5])                      # Pmax == N; a scene without and one with given objects
    elif loop.startswith("inpaint"):
        kw.update(known=given, mask=(rnd(*shape, seed=502) > 0.3).to(dev()))
    if "guided" in loop:
        kw.update(guidance_scale=(0.0, 3.0))
    return kw


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("loop", list(LOOPS))
def test_every_loop_at_one_and_two_steps_is_the_eager_loop_and_capture_draws_nothing(loop, steps, tmp_path):
    from diffuscene_amd import _lib
    cls, strided = LOOPS[loop]
    if strided:
        m = build_model("v", T_STRIDED, tmp_path)
    else:
        m = build_model("v", 2, tmp_path, tag="sampler_core_%d" % steps)    # its own model: no graph of the other step count to reuse
        # two rows; keep_running=True walks both.  Only the loops' step count follows num_timesteps: tables() is built from the
        # betas-sized attributes, and the kernels take their bound from the tables' rows -- so row 1 stays addressable
        m.diffusion.diffusion.num_timesteps = 1
    diff, gd = m.diffusion, m.diffusion.diffusion
    cond, cross = _conditions(m, B, case_texts()[:B])
    shape = (B, GN, GC)
    kw = _loop_kwargs(loop, strided, steps, shape)
    before = list(gd._graphs.values())
    outs, states, graphs = [], [], []
    for graph in (False, True, True):                                           # eager, graph (this call captures), graph (cached)
        torch.manual_seed(2468)
        with torch.no_grad(), QUIET():
            outs.append(getattr(diff, loop.split("/")[0])(shape, dev(), condition=cond, condition_cross=cross, graph=graph, **kw))
        states.append(torch.cuda.get_rng_state(dev()))
        if graph:
            assert len(gd._graphs) == 1                                         # the one-live-graph rule
            graphs.append(next(iter(gd._graphs.values())))
    assert all(graphs[0] is not g for g in before)                              # the first graph call had to capture ...
    assert torch.equal(states[1], states[0]) and torch.equal(states[2], states[0])      # ... and that cost no random numbers
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), (loop, steps, float((outs[1] - outs[0]).abs().max()))
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    assert graphs[1] is graphs[0] and type(graphs[0]).__name__ == cls
    if strided:
        assert graphs[0].S == steps and (graphs[0].graph is None) == (steps == 1) and graphs[0].final is not None
    assert _lib.device_error_count(reset=True) == 0                             # the warm-up of the capture included


# the rows that take ``fused=``: entry point -> (front end, class, strided).  fused=False unfuses the overwrite of the ragged rows and the
# guidance of the guided rows; outside this test only tools/bench_*.py run those captured paths (the two guided in-painting rows also
# in tests/test_gpu_guided_inpaint.py, through the replay buffers)
UNFUSED = {"complete_samples_ragged": ("graph_complete_ragged_loop", "_RaggedCompleteGraph", False),
           "complete_samples_ragged_ddim": ("graph_ddim_complete_ragged_loop", "_DDIMCompleteGraph", True),
           "complete_samples_ragged/Pmax5": ("graph_complete_ragged_loop", "_RaggedCompleteGraph", False),
           "complete_samples_ragged_ddim/Pmax5": ("graph_ddim_complete_ragged_loop", "_DDIMCompleteGraph", True),
           "gen_samples_guided": ("graph_guided_loop", "_GuidedStepGraph", False),
           "gen_samples_guided_ddim": ("graph_ddim_guided_loop", "_DDIMGuidedGraph", True),
           "inpaint_samples_guided": ("graph_masked_guided_loop", "_MaskedGuidedGraph", False),
           "inpaint_samples_guided_ddim": ("graph_ddim_masked_guided_loop", "_DDIMMaskedGuidedGraph", True)}


def _front_end(gd, diff, loop, strided, shape, cond, cross, kw, fused):
    """The captured loop behind entry point ``loop`` called as GaussianDiffusion calls it, with ``fused`` passed on."""
    from diffuscene_amd import sampler
    sched = (kw["sampling_timesteps"], kw["ddim_sampling_eta"]) if strided else (kw["clip_denoised"], 2)
    head, given = (cond, cross), {}
    if "guided" in loop:
        head = gd._guided_inputs(shape, dev(), cond, cross, kw["guidance_scale"], loop)
    if loop.startswith("complete"):
        given = dict(zip(("partial_boxes", "counts"), gd._ragged_inputs(shape, dev(), kw["partial_boxes"], kw["num_partial"], loop)))
    elif loop.startswith("inpaint"):
        given = dict(zip(("known", "mask"), gd._masked_inputs(shape, dev(), kw["known"], kw["mask"], loop)))
    return getattr(sampler, UNFUSED[loop][0])(gd, diff._denoise, shape, dev(), *head, *sched, noise_fn=torch.randn, fused=fused, **given)


@pytest.mark.parametrize("loop", list(UNFUSED))
def test_the_unfused_captured_loop_is_the_fused_one_and_the_eager_loop(loop, tmp_path):
    _, cls, strided = UNFUSED[loop]
    m = build_model("v", T_STRIDED, tmp_path) if strided else build_model("v", 2, tmp_path, tag="sampler_core_unfused")
    diff, gd = m.diffusion, m.diffusion.diffusion
    cond, cross = _conditions(m, B, case_texts()[:B])
    shape = (B, GN, GC)
    kw = _loop_kwargs(loop, strided, 2, shape)                                  # two steps / S = 2
    outs, states, graphs = [], [], []
    for fused in (None, True, False):                                           # eager, captured fused, captured unfused
        torch.manual_seed(1357)
        with torch.no_grad(), QUIET():
            if fused is None:
                outs.append(getattr(diff, loop.split("/")[0])(shape, dev(), condition=cond, condition_cross=cross, graph=False, **kw))
            else:
                outs.append(_front_end(gd, diff, loop, strided, shape, cond, cross, kw, fused))
                (g,) = gd._graphs.values()
                assert g.fused is fused and type(g).__name__ == cls
                if "guided" in loop:
                    assert (g.m is None) == fused
                graphs.append(g)
        states.append(torch.cuda.get_rng_state(dev()))
    assert graphs[0] is not graphs[1]                                           # ``fused`` is part of the key
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), (loop, float((outs[2] - outs[0]).abs().max()))
    assert torch.equal(states[1], states[0]) and torch.equal(states[2], states[0])
    assert bool(torch.isfinite(outs[0]).all())


# ------------------------------------------------------------------------------------------------------------------- the step kernels
KSHAPES = ((260, 65), (3, 37))         # inner 16900 > 64 blocks x 256 threads: a second trip of the grid-stride loop; inner 111: < 1 block, odd
S_K, ETA_K = 50, 0.7
_GD = {}


def _gdiff(mean_type):
    if mean_type not in _GD:
        _GD[mean_type] = _diffusion(mean_type)
    return _GD[mean_type]


def _operands(N, C):
    d = dev()
    x, mo, noise = rnd(B, N, C, seed=510).to(d), (rnd(2 * B, N, C, seed=511) * 2).to(d), rnd(B, N, C, seed=512).to(d)
    given, gnoise = rnd(B, N, C, seed=513).to(d), rnd(B, N, C, seed=514).to(d)
    mask = (rnd(B, N, C, seed=515) > 0).to(torch.uint8)
    assert 0 < int(mask.sum()) < mask.numel()
    counts = torch.tensor([0, N], dtype=torch.int64, device=d)                  # pmax == N: a scene all free, a scene all given
    scale = torch.tensor([0.0, 3.0], dtype=torch.float32, device=d)
    return x, mo, noise, given, gnoise, mask.to(d), counts, scale


def _posterior_args(gd):
    tb = gd.tables(dev())
    ca, cb = gd._coeffs(tb)
    return (ca, cb, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], gd._sigma(tb)), \
        (tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]), MT[gd.model_mean_type]


def _host_x0(gd, x, m, t, clip):
    """The x_start of the step on the host: each product and the difference one fp32 torch op."""
    if gd.model_mean_type == "x0":
        x0 = m
    else:
        ca, cb = (gd.sqrt_alphas_cumprod, gd.sqrt_one_minus_alphas_cumprod) if gd.model_mean_type == "v" else \
            (gd.sqrt_recip_alphas_cumprod, gd.sqrt_recipm1_alphas_cumprod)
        x0 = ca[t][:, None, None] * x - cb[t][:, None, None] * m
    return x0.clamp(-1.0, 1.0) if clip else x0


def _host_posterior_mean(gd, x, m, t, clip):
    x0 = _host_x0(gd, x, m, t, clip)
    return gd.posterior_mean_coef1[t][:, None, None] * x0 + gd.posterior_mean_coef2[t][:, None, None] * x


def _host_p_sample(gd, x, m, noise, t, clip):
    sg = torch.where(t != 0, gd._sigma_small[t], torch.zeros(()))[:, None, None]
    return _host_posterior_mean(gd, x, m, t, clip) + sg * noise


def _host_ddim_step(gd, x, m, noise, k):
    pairs, coef = gd.ddim_schedule(S_K, ETA_K)
    t = torch.full((x.shape[0],), pairs[k][0], dtype=torch.int64)
    x0 = _host_x0(gd, x, m, t, True)
    if pairs[k][1] < 0:
        return x0
    if gd.model_mean_type == "eps":
        pn = m
    else:
        pn = (gd.sqrt_recip_alphas_cumprod[t][:, None, None] * x - x0) / gd.sqrt_recipm1_alphas_cumprod[t][:, None, None]
    return x0 * coef[0, k] + coef[1, k] * pn + coef[2, k] * noise


@pytest.mark.parametrize("N,C", KSHAPES)
@pytest.mark.parametrize("mean_type", ["v", "eps", "x0"])
def test_posterior_kernels_past_one_trip_of_the_grid_stride_loop(mean_type, N, C):
    from diffuscene_amd import ops
    gd = _gdiff(mean_type)
    post, (sa, sb), mt = _posterior_args(gd)
    x, mo2, noise, given, gnoise, mask, counts, scale = _operands(N, C)
    mo = mo2[:B].contiguous()
    t = torch.tensor([0, 7], dtype=torch.int64, device=dev())
    t_prev, last = torch.clamp(t - 1, min=0), (t == 0)[:, None, None]
    for clip in (True, False):
        tail = (mt, clip)
        plain = ops.p_sample(x, mo, noise, t, *post, *tail)
        assert torch.equal(plain.cpu(), _host_p_sample(gd, x.cpu(), mo.cpu(), noise.cpu(), t.cpu(), clip)), (mean_type, clip)
        # completion: p_sample, then the ragged overwrite at t - 1 or the restore at t == 0 (tests/test_gpu_complete_ragged.py)
        want = plain.clone()
        ops.complete_overwrite_ragged(want, given, gnoise, counts, t_prev, sa, sb)
        is_given = torch.arange(N, device=dev())[None, :, None] < counts[:, None, None]
        want = torch.where(last & is_given, given, want)
        got = ops.p_sample_inpaint(x, mo, noise, given, gnoise, counts, t, *post, sa, sb, *tail)
        assert torch.equal(got, want), (mean_type, clip, float((got - want).abs().max()))
        # in-painting: where(mask, t > 0 ? q_sample(known, t - 1, noise_k) : known, p_sample) (tests/test_gpu_masked.py)
        want = torch.where(mask != 0, torch.where(last, given, ops.q_sample(given, gnoise, t_prev, sa, sb)), plain)
        got = ops.p_sample_masked(x, mo, noise, given, gnoise, mask, t, *post, sa, sb, *tail)
        assert torch.equal(got, want), (mean_type, clip, float((got - want).abs().max()))
        # guidance: cfg_combine, then p_sample (tests/test_gpu_cfg.py)
        x0_want, x0_got, dup = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        want = ops.p_sample(x, ops.cfg_combine(mo2, scale), noise, t, *post, *tail, x0_out=x0_want)
        got = ops.p_sample_cfg(x, mo2, scale, noise, t, *post, *tail, x_dup=dup, x0_out=x0_got)
        assert torch.equal(got, want) and torch.equal(dup, want) and torch.equal(x0_got, x0_want), (mean_type, clip)
        # guided in-painting: cfg_combine, then p_sample_masked (tests/test_gpu_guided_inpaint.py)
        dup = torch.empty_like(x)
        want = ops.p_sample_masked(x, ops.cfg_combine(mo2, scale), noise, given, gnoise, mask, t, *post, sa, sb, *tail)
        got = ops.p_sample_masked_cfg(x, mo2, scale, noise, given, gnoise, mask, t, *post, sa, sb, *tail, x_dup=dup)
        assert torch.equal(got, want) and torch.equal(dup, want), (mean_type, clip, float((got - want).abs().max()))


@pytest.mark.parametrize("N,C", KSHAPES)
@pytest.mark.parametrize("mean_type", ["v", "eps", "x0"])
def test_ddim_kernels_past_one_trip_of_the_grid_stride_loop(mean_type, N, C):
    from diffuscene_amd import ops
    gd = _gdiff(mean_type)
    dtab = gd.ddim_tables(S_K, ETA_K, dev())
    pairs = dtab[0]
    wide, narrow = _step_args(gd, dtab), _ddim_args(gd, dtab)                   # with / without the (sa, sb) of the re-noising
    sa, sb = wide[7], wide[8]
    x, mo2, noise, given, gnoise, mask, counts, scale = _operands(N, C)
    x, mo2 = x * 1.5, mo2 * 0.75
    mo = mo2[:B].contiguous()
    is_given = torch.arange(N, device=dev())[None, :, None] < counts[:, None, None]
    for k in (S_K // 2, S_K - 1):                                               # a middle pair and the last pair
        step = torch.tensor([k], dtype=torch.int64, device=dev())
        last = pairs[k][1] < 0
        assert last == (k == S_K - 1)
        plain = gd.ddim_step(x, mo, noise, step, dtab)
        assert torch.equal(plain.cpu(), _host_ddim_step(gd, x.cpu(), mo.cpu(), noise.cpu(), k)), (mean_type, k)
        t_next = torch.full((B,), max(pairs[k][1], 0), dtype=torch.int64, device=dev())
        # completion: ddim_step, then the ragged overwrite at t_next or the restore on the last pair (tests/test_gpu_ddim_complete.py)
        want = plain.clone()
        if last:
            want = torch.where(is_given, given, want)
        else:
            ops.complete_overwrite_ragged(want, given, gnoise, counts, t_next, sa, sb)
        got = ops.ddim_inpaint_step(x, mo, noise, given, gnoise, counts, step, *wide)
        assert torch.equal(got, want), (mean_type, k, float((got - want).abs().max()))
        # in-painting (tests/test_gpu_masked.py)
        want = torch.where(mask != 0, given if last else ops.q_sample(given, gnoise, t_next, sa, sb), plain)
        got = ops.ddim_masked_step(x, mo, noise, given, gnoise, mask, step, *wide)
        assert torch.equal(got, want), (mean_type, k, float((got - want).abs().max()))
        # guidance (tests/test_gpu_cfg.py)
        x0_want, x0_got, dup = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        want = ops.ddim_step(x, ops.cfg_combine(mo2, scale), noise, step, *narrow, x0_out=x0_want)
        got = ops.ddim_cfg_step(x, mo2, scale, noise, step, *narrow, x_dup=dup, x0_out=x0_got)
        assert torch.equal(got, want) and torch.equal(dup, want) and torch.equal(x0_got, x0_want), (mean_type, k)
        # guided in-painting (tests/test_gpu_guided_inpaint.py)
        dup = torch.empty_like(x)
        want = ops.ddim_masked_step(x, ops.cfg_combine(mo2, scale), noise, given, gnoise, mask, step, *wide)
        got = ops.ddim_masked_cfg_step(x, mo2, scale, noise, given, gnoise, mask, step, *wide, x_dup=dup)
        assert torch.equal(got, want) and torch.equal(dup, want), (mean_type, k, float((got - want).abs().max()))


def test_who_reads_the_noise_at_t_zero_and_on_the_last_pair():
    """p_sample, p_sample_inpaint, p_sample_masked and p_sample_masked_cfg force sigma to 0 at t == 0 and still add 0 * noise: infinite
    noise gives NaN on every free element; p_sample_cfg does not read it.  A given element reads neither.  On the last DDIM pair no
    kernel reads a noise."""
    from diffuscene_amd import ops
    N, C = KSHAPES[1]
    gd = _gdiff("v")
    post, (sa, sb), mt = _posterior_args(gd)
    x, mo2, _, given, _, mask, _, scale = _operands(N, C)
    mo = mo2[:B].contiguous()
    inf = torch.full_like(x, INF)
    t = torch.zeros((B,), dtype=torch.int64, device=dev())
    counts = torch.tensor([1, 2], dtype=torch.int64, device=dev())
    is_given = (torch.arange(N, device=dev())[None, :, None] < counts[:, None, None]).expand(B, N, C)
    assert torch.isnan(ops.p_sample(x, mo, inf, t, *post, mt, True)).all()
    got = ops.p_sample_inpaint(x, mo, inf, given, inf, counts, t, *post, sa, sb, mt, True)
    assert torch.isnan(got[~is_given]).all() and torch.equal(got[is_given], given[is_given])
    got = ops.p_sample_masked(x, mo, inf, given, inf, mask, t, *post, sa, sb, mt, True)
    assert torch.isnan(got[mask == 0]).all() and torch.equal(got[mask != 0], given[mask != 0])
    got = ops.p_sample_cfg(x, mo2, scale, inf, t, *post, mt, True)
    m = ops.cfg_combine(mo2, scale)
    assert torch.isfinite(got).all() and torch.equal(got.cpu(), _host_posterior_mean(gd, x.cpu(), m.cpu(), t.cpu(), True))
    got = ops.p_sample_masked_cfg(x, mo2, scale, inf, given, inf, mask, t, *post, sa, sb, mt, True)
    assert torch.isnan(got[mask == 0]).all() and torch.equal(got[mask != 0], given[mask != 0])
    # the last pair: x_start, whatever the noises hold
    dtab = gd.ddim_tables(S_K, ETA_K, dev())
    wide, narrow = _step_args(gd, dtab), _ddim_args(gd, dtab)
    step = torch.tensor([S_K - 1], dtype=torch.int64, device=dev())
    t_last = torch.full((B,), dtab[0][-1][0], dtype=torch.int64)
    x_start = _host_x0(gd, x.cpu(), mo.cpu(), t_last, True).to(dev())
    got = ops.ddim_step(x, mo, inf, step, *narrow)
    assert torch.isfinite(got).all() and torch.equal(got, x_start)
    got = ops.ddim_inpaint_step(x, mo, inf, given, inf, counts, step, *wide)
    assert torch.isfinite(got).all() and torch.equal(got, torch.where(is_given, given, x_start))
    got = ops.ddim_masked_step(x, mo, inf, given, inf, mask, step, *wide)
    assert torch.isfinite(got).all() and torch.equal(got, torch.where(mask != 0, given, x_start))
    x_start_g = _host_x0(gd, x.cpu(), m.cpu(), t_last, True).to(dev())
    got = ops.ddim_cfg_step(x, mo2, scale, inf, step, *narrow)
    assert torch.isfinite(got).all() and torch.equal(got, x_start_g)
    got = ops.ddim_masked_cfg_step(x, mo2, scale, inf, given, inf, mask, step, *wide)
    assert torch.isfinite(got).all() and torch.equal(got, torch.where(mask != 0, given, x_start_g))
