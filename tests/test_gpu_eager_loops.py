"""GPU: what the twelve eager sampling loops of diffusion_ddpm.py share -- the T-step body, the strided body, the given parts, the model
call -- and what the step wrappers of ops.py share, where no per-feature test looks:

* the draw protocol of every loop (order, count, size, dtype, device of each noise_fn call) against a literal list written from the
  docstrings, at 1, 2 and 3 steps, Pmax in {1, N}, counts that include 0 and Pmax;
* a custom noise_fn that is torch.randn underneath takes the eager path and returns what the captured loop returns under the same seed,
  bit for bit, and leaves the device generator in the same state;
* a loop that overwrites its state in place leaves a caller's replay buffers untouched;
* the reference's ``print('last:', ...)``: one line from the dense, ragged and arrange T-step loops, eager and captured, none elsewhere;
* the trajectory and ``return_all_timesteps`` lists;
* the refusals that the step wrappers share, before any launch.

Step counts: the strided loops run S in {1, 2, 3} on a 50-row schedule.  A T-step loop of k steps is a 3-row schedule with
num_timesteps = k (tests/test_gpu_sampler_core.py: only the loops' step count follows num_timesteps) -- eager runs only; the runs that
capture use the untouched 3-row schedule."""
import contextlib
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.make_golden import case_inputs  # noqa: E402
from test_gpu_cfg import GC, GN, _conditions, _ddim_args, build_model, case_texts  # noqa: E402
from test_gpu_complete_ragged import dev, rnd  # noqa: E402
from test_gpu_masked import _diffusion, _step_args  # noqa: E402
from test_gpu_net import build as build_net  # noqa: E402

B, T_ROWS, T_STRIDED, ETA = 2, 3, 50, 0.5
SHAPE = (B, GN, GC)
AN, AC, ASUB = 21, 65, 5                  # the re-arrangement network: N = 21, full rows of 65, diffused [translation | angle] = 3 + 2

#        loop             entry point                      strided  captured form
LOOPS = {"plain": ("gen_samples", False, True),
         "trajectory": ("gen_sample_traj", False, False),
         "ddim": ("gen_samples_ddim", True, True),
         "guided": ("gen_samples_guided", False, True),
         "guided_ddim": ("gen_samples_guided_ddim", True, True),
         "dense": ("complete_samples", False, True),
         "ragged": ("complete_samples_ragged", False, True),
         "ragged_ddim": ("complete_samples_ragged_ddim", True, True),
         "masked": ("inpaint_samples", False, True),
         "masked_ddim": ("inpaint_samples_ddim", True, True),
         "arrange": ("arrange_samples", False, True),
         "arrange_ddim": ("arrange_samples_ddim", True, True)}
PRINTS = ("dense", "ragged", "arrange")
HAS_PMAX = ("dense", "ragged", "ragged_ddim")


@pytest.fixture(autouse=True)
def no_device_errors():
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    yield
    assert _lib.device_error_count(reset=True) == 0


class Recorder:
    """torch.randn behind the noise_fn protocol; keeps the keywords and the tensor of every draw."""

    def __init__(self):
        self.sizes, self.dtypes, self.devices, self.draws = [], [], [], []

    def __call__(self, size=None, dtype=None, device=None):
        self.sizes.append(tuple(size))
        self.dtypes.append(dtype)
        self.devices.append(torch.device(device))
        self.draws.append(torch.randn(size, dtype=dtype, device=device))
        return self.draws[-1]


def _setup(loop, tmp_path):
    """(DiffusionPoint, shape, condition, condition_cross) of a loop: the tiny text model, or the re-arrangement network."""
    strided = LOOPS[loop][1]
    T = T_STRIDED if strided else T_ROWS
    if loop.startswith("arrange"):
        _, _, _, cond, _ = case_inputs("rearrange_living")
        _, diff = build_net("rearrange_living", time_num=T, model_mean_type="v", config_extra={"room_arrange_condition": True})
        return diff, (B, AN, AC), cond.to(dev()), None
    m = build_model("v", T, tmp_path, tag=None if strided else "eager_loops")
    cond, cross = _conditions(m, B, case_texts()[:B])
    return m.diffusion, SHAPE, cond, cross


def _kwargs(loop, steps, shape, pmax):
    _, N, C = shape
    strided = LOOPS[loop][1]
    kw = dict(sampling_timesteps=steps, ddim_sampling_eta=ETA) if strided else dict(clip_denoised=True)
    given = rnd(*shape, seed=601).clamp(-1, 1).to(dev())
    if loop == "trajectory":
        kw.update(freq=2)
    elif loop == "dense":
        kw.update(partial_boxes=given[:, :pmax].contiguous())
    elif loop.startswith("ragged"):
        kw.update(partial_boxes=given[:, :pmax].contiguous(), num_partial=[0, pmax])        # a scene without, a scene full of given rows
    elif loop.startswith("masked"):
        kw.update(known=given, mask=(rnd(*shape, seed=602) > 0.3).to(dev()))
    elif loop.startswith("guided"):
        kw.update(guidance_scale=(0.0, 3.0))
    elif loop.startswith("arrange"):
        kw.update(input_boxes=given)
    return kw


def _call(loop, setup, steps, pmax=1, **over):
    """One call of the loop's entry point -> (result, what it printed)."""
    diff, shape, cond, cross = setup
    kw = _kwargs(loop, steps, shape, pmax)
    kw.update(over)
    out = io.StringIO()
    with torch.no_grad(), contextlib.redirect_stdout(out):
        res = getattr(diff, LOOPS[loop][0])(shape, dev(), condition=cond, condition_cross=cross, **kw)
    return res, out.getvalue()


@contextlib.contextmanager
def _t_steps(diff, loop, steps):
    """A T-step loop of ``steps`` steps on the 3-row schedule (eager runs only: a captured graph sizes its buffers by num_timesteps)."""
    gd = diff.diffusion
    keep = gd.num_timesteps
    if not LOOPS[loop][1]:
        gd.num_timesteps = steps
    try:
        yield
    finally:
        gd.num_timesteps = keep


def _last_lines(text):
    return [line for line in text.splitlines() if line.startswith("last:")]


# ------------------------------------------------------------------------------------------------------------------- 1. the draw protocol
def _documented_sizes(loop, n, shape, pmax):
    """The ``size`` of every draw, in order, as the docstrings of diffusion_ddpm.py state them (n: T or S)."""
    Bs, N, C = shape
    pshape, sub = (Bs, pmax, C), (Bs, N, ASUB)
    return {"plain": [shape] * (n + 1),
            "trajectory": [shape] * (n + 1),
            "guided": [shape] * (n + 1),
            "dense": [shape] + [pshape, shape] * n,
            "ragged": [shape] + [pshape, shape] * n,
            "masked": [shape] * (2 * n + 1),
            "ddim": [shape] * n,
            "guided_ddim": [shape] * n,
            "ragged_ddim": [shape] + [pshape, shape] * (n - 1) + [pshape],
            "masked_ddim": [shape] + [shape, shape] * (n - 1) + [shape],
            "arrange": [sub] * (n + 1),
            "arrange_ddim": [sub] * n}[loop]


DRAW_CASES = [(loop, steps, pmax) for loop in LOOPS for steps in (1, 2, 3) for pmax in ((1, None) if loop in HAS_PMAX else (1,))]


@pytest.mark.parametrize("loop,steps,pmax", DRAW_CASES)
def test_every_loop_makes_the_documented_draws(loop, steps, pmax, tmp_path):
    setup = _setup(loop, tmp_path)
    shape = setup[1]
    pmax = shape[1] if pmax is None else pmax
    rec = Recorder()
    with _t_steps(setup[0], loop, steps):
        res, _ = _call(loop, setup, steps, pmax, noise_fn=rec)               # not a NoiseReplay: the loop runs eagerly
    assert rec.sizes == _documented_sizes(loop, steps, shape, pmax), (loop, steps, pmax)
    assert all(d == torch.float for d in rec.dtypes) and all(d == dev() for d in rec.devices)
    out = res[-1] if loop == "trajectory" else res
    assert tuple(out.shape) == tuple(shape) and bool(torch.isfinite(out).all())
    if loop in HAS_PMAX:                                                        # counts [0, pmax] (dense: pmax rows of every scene)
        given = _kwargs(loop, steps, shape, pmax)["partial_boxes"]
        assert torch.equal(out[1, :pmax], given[1])
        if loop == "dense":
            assert torch.equal(out[0, :pmax], given[0])


# ------------------------------------------------------------------------------------------------- 2. + 4. eager is the default path; prints
_RUNS = {}


def _eager_and_captured(loop, tmp_path):
    """Under one seed: the loop behind a recording noise_fn (eager) and with torch.randn and graph=True (captured); 3 steps.  Run once."""
    if loop not in _RUNS:
        setup = _setup(loop, tmp_path)
        pmax = setup[1][1]
        run = {}
        for kind, over in (("eager", dict(noise_fn=Recorder())), ("captured", dict(noise_fn=torch.randn, graph=True))):
            if kind == "captured" and not LOOPS[loop][2]:
                continue
            torch.manual_seed(97531)
            res, printed = _call(loop, setup, 3, pmax, **over)
            run[kind] = (res, printed, torch.cuda.get_rng_state(dev()))
        _RUNS[loop] = run, setup[0].diffusion
    return _RUNS[loop]


@pytest.mark.parametrize("loop", [name for name in LOOPS if LOOPS[name][2]])
def test_a_custom_noise_fn_runs_the_eager_loop_and_it_is_the_captured_loop(loop, tmp_path):
    run, gd = _eager_and_captured(loop, tmp_path)
    (eager, _, state_e), (captured, _, state_c) = run["eager"], run["captured"]
    assert len(gd._graphs) == 1                                                 # the second run did go through a captured graph
    assert torch.equal(eager, captured), (loop, float((eager - captured).abs().max()))
    assert torch.equal(state_e, state_c)


@pytest.mark.parametrize("loop", list(LOOPS))
def test_the_reference_prints_last_once_from_three_loops_and_never_elsewhere(loop, tmp_path):
    run, gd = _eager_and_captured(loop, tmp_path)
    want = ["last: 0 %d %d" % (gd.num_timesteps, len(gd.betas))] if loop in PRINTS else []
    for kind, (_, printed, _) in run.items():
        assert _last_lines(printed) == want, (loop, kind, printed)


# ------------------------------------------------------------------------------------------------------------------- 3. replay buffers
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("loop", ["dense", "ragged", "ragged_ddim", "masked", "masked_ddim"])
def test_replay_buffers_are_read_only(loop, steps, tmp_path):
    """These loops overwrite the state in place before the first model call, and the state starts as row 0 of the caller's buffer."""
    from diffuscene_amd.sampler import NoiseReplay, RaggedNoiseReplay
    setup = _setup(loop, tmp_path)
    strided = LOOPS[loop][1]
    pmax = 1 if loop == "dense" else GN                                         # dense: NoiseReplay tells the draws apart by shape
    pshape = SHAPE if loop.startswith("masked") else (B, pmax, GC)
    main = torch.stack([rnd(*SHAPE, seed=610 + i) for i in range(steps + (0 if strided else 1))]).to(dev())
    part = torch.stack([rnd(*pshape, seed=620 + i) for i in range(steps)]).to(dev())
    main0, part0 = main.clone(), part.clone()
    replay = NoiseReplay(main, part) if loop == "dense" else RaggedNoiseReplay(main, part)
    with _t_steps(setup[0], loop, steps):
        out, _ = _call(loop, setup, steps, pmax, noise_fn=replay, graph=False)
    assert torch.equal(main, main0) and torch.equal(part, part0)
    assert out.data_ptr() != main.data_ptr() and bool(torch.isfinite(out).all())
    assert replay.i == main.shape[0] and replay.ip == steps                     # every row was drawn, in the eager loop


# ------------------------------------------------------------------------------------------------------------------- 5. lists of states
def test_trajectory_states_and_their_order(tmp_path):
    """freq = 2, T = 3: x_T, the state after t = 2 (== total - 1) and the state after t = 0 (0 % 2 == 0) -- not the one after t = 1."""
    setup = _setup("trajectory", tmp_path)
    diff, shape, cond, cross = setup
    rec = Recorder()
    torch.manual_seed(1357)
    traj, _ = _call("trajectory", setup, 3, noise_fn=rec)
    assert len(traj) == 3 and len(rec.draws) == 4 and traj[0] is rec.draws[0]
    # the same chain one public p_sample at a time, on the recorded draws
    x, states = rec.draws[0], {}
    with torch.no_grad():
        for k, t in enumerate((2, 1, 0)):
            t_ = torch.full((B,), t, dtype=torch.int64, device=dev())
            x = diff.diffusion.p_sample(diff._denoise, x, t_, cond, cross, noise_fn=lambda size, dtype, device, k=k: rec.draws[k + 1],
                                        clip_denoised=True)
            states[t] = x
    assert torch.equal(traj[1], states[2]) and torch.equal(traj[2], states[0])
    assert not torch.equal(traj[1], states[1]) and not torch.equal(traj[2], states[1])
    torch.manual_seed(1357)
    plain, _ = _call("plain", setup, 3, graph=False)
    assert torch.equal(traj[-1], plain)


@pytest.mark.parametrize("S", [1, 3])
def test_return_all_timesteps_lists_the_s_plus_one_states(S, tmp_path):
    setup = _setup("ddim", tmp_path)
    rec = Recorder()
    torch.manual_seed(2468)
    states, _ = _call("ddim", setup, S, noise_fn=rec, return_all_timesteps=True)
    assert isinstance(states, list) and len(states) == S + 1 and states[0] is rec.draws[0]
    assert all(tuple(s.shape) == SHAPE for s in states)
    assert all(not torch.equal(states[k], states[k + 1]) for k in range(S))
    torch.manual_seed(2468)
    last, _ = _call("ddim", setup, S, graph=False, return_all_timesteps=False)
    assert torch.equal(states[-1], last)


# ------------------------------------------------------------------------------------------------------------------- 6. refusals
def _wrapper_calls():
    """name -> (call(**replaced operands), strided): every step wrapper of ops.py on valid operands of one small shape."""
    from diffuscene_amd import ops
    gd = _diffusion("v")
    d = dev()
    N, C, S = 5, 7, 4
    dtab = gd.ddim_tables(S, ETA, d)
    wide, narrow = _step_args(gd, dtab), _ddim_args(gd, dtab)           # times, times_next, coef, ...: with / without the re-noising tables
    tb = gd.tables(d)
    ca, cb = gd._coeffs(tb)
    post = (ca, cb, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], gd._sigma(tb))
    q = (tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"])
    x, mo, noise, given, gnoise = (rnd(B, N, C, seed=630 + i).to(d) for i in range(5))
    mo2 = rnd(2 * B, N, C, seed=636).to(d)
    mask = (rnd(B, N, C, seed=637) > 0).to(torch.uint8).to(d)
    counts = torch.tensor([0, N], dtype=torch.int64, device=d)
    scale = torch.tensor([0.0, 3.0], dtype=torch.float32, device=d)
    t = torch.tensor([0, 7], dtype=torch.int64, device=d)
    step = torch.ones((1,), dtype=torch.int64, device=d)

    def tables(args, times_next=None, coef=None):
        return (args[0], args[1] if times_next is None else times_next, args[2] if coef is None else coef) + tuple(args[3:])

    return {
        "ddim_step": (lambda model_out=mo, noise=noise, out=None, **tabs: ops.ddim_step(x, model_out, noise, step, *tables(narrow, **tabs), out=out), True),
        "p_sample_inpaint": (lambda model_out=mo, noise=noise, out=None: ops.p_sample_inpaint(x, model_out, noise, given, gnoise, counts, t, *post, *q,
                                                                                              2, True, out=out), False),
        "ddim_inpaint_step": (lambda model_out=mo, noise=noise, out=None, **tabs: ops.ddim_inpaint_step(x, model_out, noise, given, gnoise, counts, step,
                                                                                                        *tables(wide, **tabs), out=out), True),
        "p_sample_masked": (lambda model_out=mo, noise=noise, out=None: ops.p_sample_masked(x, model_out, noise, given, gnoise, mask, t, *post, *q, 2,
                                                                                            True, out=out), False),
        "ddim_masked_step": (lambda model_out=mo, noise=noise, out=None, **tabs: ops.ddim_masked_step(x, model_out, noise, given, gnoise, mask, step,
                                                                                                      *tables(wide, **tabs), out=out), True),
        "p_sample_cfg": (lambda model_out=mo2, noise=noise, out=None: ops.p_sample_cfg(x, model_out, scale, noise, t, *post, 2, True, out=out), False),
        "ddim_cfg_step": (lambda model_out=mo2, noise=noise, out=None, **tabs: ops.ddim_cfg_step(x, model_out, scale, noise, step,
                                                                                                 *tables(narrow, **tabs), out=out), True),
    }, (x, S)


def test_the_step_wrappers_refuse_bad_tables_shapes_and_outputs_before_any_launch():
    """One bad call per shared argument check, for every wrapper that makes that check.  Nothing may launch: every bad call that can
    take one is handed an ``out`` full of NaN, which must still be full of NaN afterwards (every kernel writes all of ``out``), and the
    autouse fixture counts the indices a kernel had to clamp."""
    calls, (x, S) = _wrapper_calls()
    d = dev()
    good = {name: call() for name, (call, _) in calls.items()}                  # the operands are valid: every wrapper runs
    for name, (call, strided) in calls.items():
        sentinel = torch.full_like(x, float("nan"))
        if strided:
            with pytest.raises(RuntimeError):
                call(times_next=torch.zeros((S + 1,), dtype=torch.int64, device=d), out=sentinel)
            with pytest.raises(RuntimeError):
                call(coef=torch.zeros((2, S), dtype=torch.float32, device=d), out=sentinel)
        with pytest.raises(RuntimeError):                                       # the guided wrappers: refused with their 2 B check
            call(model_out=torch.zeros((B, 5, 8), dtype=torch.float32, device=d), out=sentinel)
        with pytest.raises(RuntimeError):                                       # the shared shape check, in all seven
            call(noise=torch.zeros((B, 5, 8), dtype=torch.float32, device=d), out=sentinel)
        if name != "ddim_step":                                                 # ddim_step takes ``out`` as it is given, like p_sample
            with pytest.raises(RuntimeError):
                call(out=torch.zeros((B, 7, 5), dtype=torch.float32, device=d).transpose(1, 2))
        assert bool(torch.isnan(sentinel).all()), name
    for name, (call, _) in calls.items():
        assert torch.equal(call(), good[name]), name
