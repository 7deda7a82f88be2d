"""DDPM process of DiffuScene on MI355X -- drop-in for scene_synthesis/networks/diffusion_ddpm.py.

Same names, signatures, assertion behaviour and RNG draw order as the reference (``get_betas`` :45-91,
``GaussianDiffusion`` :125-717, ``DiffusionPoint`` :721-804).  Differences are internal:

* the 13 schedule tables are built exactly as the reference builds them (float64 numpy -> fp32 torch) but are
  uploaded ONCE per device instead of on every ``_extract`` call (:220,:232,:284,...);
* ``q_sample`` / v-target and the whole ``p_mean_variance`` + ``p_sample`` chain (:242-352) are single HIP
  kernels (csrc/diffusion.hip), bit-identical to the reference's fp32 expressions;
* the reverse loops run as a replayed hipGraph (default since round 6; ``graph=False`` or env DSC_GRAPH=0 for the eager loop): one captured step
  with a device-resident timestep, replayed T times -- no Python, no launches on the critical path.

The eager loops -- what the captured loops of sampler.py are tested against, built from the unfused kernels on purpose -- are two cores,
each a generator of states (x_T, then the state after every step), and two independent variations handed to a core as small objects:
  GaussianDiffusion._t_states        T steps: fill t_, model call, one draw (also at t == 0), ops.p_sample
  GaussianDiffusion._strided_states  S strided (DDIM) pairs: device step counter, model call, a draw except on the last pair, ddim_step,
                                     ddim_advance
  the given part   _FREE (nothing), _GivenRows / _GivenRagged (a dense / ragged row prefix), _GivenMask (a byte mask): drawn for and
                   written over the state in place BEFORE every model call, restored in the last state; x_T is cloned only if it is
                   written
  the model call   _model (plain) or _guided_model (the denoiser at 2 B, then cfg_combine); under ``collision_scale`` / ``wall_scale``
                   _corrected hands either one a ``post`` hook that issues, on the output in place and before the guidance mix, collision
                   steering (dsc_steer_boxes_f32), floor-plan steering (dsc_steer_walls_f32), then the solver's launch
  the solver       ``sampling_solver="dpmpp_2m"`` (strided loops): _strided_states hands the model call a ``post`` hook that issues
                   dsc_multistep_x0_f32 on the (steered) output, before the guidance mix, on every pair but the last; the step is unchanged
A ``noise_fn`` that is a scene_noise.SceneNoise (per-scene seeds) is armed by the core it runs under -- told whether the loop has a given
part -- and then numbers its own draws: main stream x_T = 0, 1, 2, ..., given stream 0, 1, 2, ... (scene_noise.py).
The public loops state their spec -- strided (S, eta) or not, the given part, the guidance scale -- and GaussianDiffusion._loop does the
rest once: validates, hands over to the captured loop under _use_graph, builds the two objects and runs a core: nothing given --
p_sample_loop, _trajectory, _arrange / ddim_sample_loop, ddim_arrange_loop (both arrange loops on the sub-shape); guided --
p_sample_loop_guided / ddim_guided_loop; rows -- p_sample_loop_complete, _complete_ragged / ddim_complete_ragged_loop; mask --
p_sample_loop_masked / ddim_masked_loop; mask and guided -- p_sample_loop_masked_guided / ddim_masked_guided_loop.
"""
import json
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..scene_noise import SceneNoise
from .loss import axis_aligned_bbox_overlaps_3d  # noqa: F401  (re-exported: the reference module exposes it, :16)

ModelPrediction = namedtuple('ModelPrediction', ['pred_noise', 'pred_x_start'])

_MEAN = {"eps": ops.MEAN_EPS, "x0": ops.MEAN_X0, "v": ops.MEAN_V}


def getGradNorm(net):
    """(parameter norm, gradient norm), reference :28-31 -- two fused multi-tensor reductions instead of 2x|params| kernels."""
    ps = [p for p in net.parameters()]
    pNorm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(ps)))
    gradNorm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm([p.grad for p in ps])))
    return pNorm, gradNorm


def normal_kl(mean1, logvar1, mean2, logvar2):
    """KL( N(mean1, e^logvar1) || N(mean2, e^logvar2) ) per element -- what the variational-bound diagnostics (_vb_terms_bpd,
    _prior_bpd) need of the reference's helper block (:94-99); its other helpers (identity, norm, weights_init, the discretized
    log-likelihood) have no caller on this path and are not carried."""
    dlog = logvar2 - logvar1
    return 0.5 * (dlog - 1.0 + torch.exp(-dlog) + (mean1 - mean2).pow(2) * torch.exp(-logvar2))


def get_betas(schedule_type, b_start, b_end, time_num):
    if schedule_type == 'linear':
        betas = np.linspace(b_start, b_end, time_num)
    elif schedule_type in ('warm0.1', 'warm0.2', 'warm0.5'):
        frac = float(schedule_type[4:])
        betas = b_end * np.ones(time_num, dtype=np.float64)
        warm = int(time_num * frac)
        betas[:warm] = np.linspace(b_start, b_end, warm, dtype=np.float64)
    else:
        # the reference's 'cosine' branch never assigns betas (diffusion_ddpm.py:84-87, UnboundLocalError)
        raise NotImplementedError(schedule_type)
    return betas


# ---------------------------------------------------------------------- the variations of an eager loop (module docstring)
class _Free:
    """The given part of a loop that is given nothing.  ``before(x, t_)``: draw noise and write q_sample(given, t, noise) over the state
    in place, in front of the model call; ``finish(x)``: the clean values into the last state; ``inplace``: does ``before`` write."""
    inplace = False

    def before(self, x, t_):
        pass

    def finish(self, x):
        return x

    def steer_operands(self):
        """What the part adds to ops.steer_rec: a given element enters the boxes with its given value and is never moved."""
        return {}


_FREE = _Free()


class _Given:
    """A given part that writes: the q_sample tables and one draw of ``size`` per step."""
    inplace = True

    def __init__(self, diff, device, noise_fn, size):
        tb = diff.tables(device)
        self.q = (tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"])
        self.draw = lambda: noise_fn(size=size, dtype=torch.float, device=device).contiguous()


class _GivenRows(_Given):
    """The first P rows of every scene are given by ``boxes`` (B, P, C): p_sample_loop_complete, reference :461-473."""

    def __init__(self, diff, device, noise_fn, boxes):
        super().__init__(diff, device, noise_fn, boxes.shape)
        self.boxes = boxes

    def before(self, x, t_):
        ops.complete_overwrite(x, self.boxes, self.draw(), t_, *self.q)

    def finish(self, x):
        x[:, :self.boxes.shape[1], :] = self.boxes
        return x

    def steer_operands(self):
        b, p = self.boxes.shape[:2]
        return dict(rows=(self.boxes, None, torch.full((b,), p, device=self.boxes.device, dtype=torch.int64)))


class _GivenRagged(_GivenRows):
    """Rows [0, counts[b]) of scene b are given by ``boxes`` (B, Pmax, C); ``counts``: (B,) int64 on the device (ops.ragged_counts)."""

    def __init__(self, diff, device, noise_fn, boxes, counts):
        super().__init__(diff, device, noise_fn, boxes)
        self.counts = counts

    def before(self, x, t_):
        ops.complete_overwrite_ragged(x, self.boxes, self.draw(), self.counts, t_, *self.q)

    def finish(self, x):
        return restore_given_rows(x, self.boxes, self.counts)

    def steer_operands(self):
        return dict(rows=(self.boxes, None, self.counts))


class _GivenMask(_Given):
    """The elements marked by ``mask`` (B, N, C) uint8 (ops.known_mask) are given by ``known``.  One draw of the full shape per step."""

    def __init__(self, diff, device, noise_fn, shape, known, mask):
        super().__init__(diff, device, noise_fn, shape)
        self.known, self.mask = known, mask

    def before(self, x, t_):
        ops.masked_overwrite(x, self.known, self.draw(), self.mask, t_, *self.q)

    def finish(self, x):
        return torch.where(self.mask != 0, self.known, x)

    def steer_operands(self):
        return dict(mask=(self.known, None, self.mask))


def restore_given_rows(x, boxes, counts):
    """x[b, :counts[b]] = boxes[b, :counts[b]], in place: the restore of the ragged completion loops, eager and captured unfused."""
    pmax = boxes.shape[1]
    given = torch.arange(pmax, device=x.device)[None, :, None] < counts[:, None, None]
    x[:, :pmax, :] = torch.where(given, boxes, x[:, :pmax, :])
    return x


def _model(denoise_fn, condition, condition_cross):
    """The model call of a loop: (x, t_) -> model output.  ``post`` (x, model output), where a loop passes one, corrects the output in
    place before it is returned (the multistep solver of _strided_states)."""
    def call(x, t_, post=None):
        mo = denoise_fn(x, t_, condition, condition_cross)
        if post is not None:
            mo = mo.contiguous()
            post(x, mo)
        return mo
    return call


def _guided_model(denoise_fn, cond2, cross2, scale):
    """The guided model call: the denoiser at 2 B on the same x and t in both halves (conditions of _guided_inputs), then
    m = u + scale[b] * (c - u) (dsc_cfg_combine_f32).  ``post`` sees the 2 B output, before the mix."""
    def call(x, t_, post=None):
        mo = denoise_fn(torch.cat([x, x], dim=0), torch.cat([t_, t_]), cond2, cross2).contiguous()
        if post is not None:
            post(x, mo)
        return ops.cfg_combine(mo, scale)
    return call


def _corrected(model, diff, device, part, scale=None, steer=None, walls=None):
    """The model call of a loop under steering: ``model`` -- _model or, with its (B,) ``scale``, _guided_model -- with the corrections of
    its output issued in place through the ``post`` hook, in the order of the captured loop: collision steering (dsc_steer_boxes_f32,
    ``steer`` of _steer_inputs), floor-plan steering (dsc_steer_walls_f32, ``walls`` of _wall_inputs), then the caller's ``post`` (the
    multistep launch); under guidance on the 2 B output, before the mix."""
    ca, cb = diff._coeffs(diff.tables(device))
    one = lambda v, dtype: torch.full((1,), v, device=device, dtype=dtype)  # noqa: E731
    recs = []
    if steer is not None:
        weight, k, bounds, bbox_dim, class_dim = steer
        recs.append(("steer_rec", (weight, one(k, torch.int64), ops.steer_bounds(bounds), bbox_dim, class_dim)))
    if walls is not None:
        weight, k, bounds, bbox_dim, class_dim, field, room_side = walls
        recs.append(("walls_rec", (weight, one(k, torch.int64), ops.steer_bounds(bounds), bbox_dim, class_dim, field,
                                   one(room_side, torch.float32))))

    def call(x, t_, post=None):
        def corrections(x, mo):
            for rec, spec in recs:
                ops.issue(getattr(ops, rec)(x.contiguous(), mo, _MEAN[diff.model_mean_type], (ca, cb), spec, t=t_, scale=scale,
                                            **part.steer_operands()))
            if post is not None:
                post(x, mo)
        return model(x, t_, corrections)
    return call


def _steer_kw(collision_scale, collision_steps):
    """The steering keyword a public loop hands to _loop: none at all without it, so that call stays what it was."""
    return {} if collision_scale is None and collision_steps is None else dict(steer=(collision_scale, collision_steps))


def _wall_kw(wall_scale, wall_steps, room_side, room_mask):
    """The floor-plan keyword a public loop hands to _loop: none at all without it, so that call stays what it was."""
    if wall_scale is None and wall_steps is None and room_side is None:
        return {}
    return dict(walls=(wall_scale, wall_steps, room_side, room_mask))


def _solver_kw(sampling_solver):
    """The solver keyword a public strided loop hands to _loop: none at all without it, so that call stays what it was."""
    return {} if sampling_solver is None else dict(multistep=sampling_solver)


def _check_solver(solver, strided, what):
    """The refusals of ``sampling_solver``, before anything is drawn or computed: an unknown name, a loop that is not strided, eta != 0
    (the solver is the deterministic ODE form)."""
    if not isinstance(solver, str) or solver not in ops.SOLVERS:
        raise ValueError("%s: sampling_solver must be None or one of %s, got %r" % (what, ops.SOLVERS, solver))
    if strided is None or strided[0] is None:
        raise ValueError("%s: sampling_solver=%r goes with sampling_timesteps: the solver rides on the strided loops" % (what, solver))
    if float(strided[1]) != 0.0:
        raise ValueError("%s: sampling_solver=%r needs ddim_sampling_eta = 0 (the deterministic ODE form), got %r"
                         % (what, solver, strided[1]))
    return solver


def _resample_kw(resample, resample_steps):
    """The resampling keyword a public loop hands to _loop: none at all without it, so that call stays what it was."""
    return {} if resample is None and resample_steps is None else dict(resample=(resample, resample_steps))


def _jump_draw(noise_fn, shape, device):
    """The draw of a resampling jump: one more draw of the MAIN stream right after the step's.  A noise_fn that tells its streams apart by
    counting calls (RaggedNoiseReplay, SceneNoise) has ``main_draw`` for it; any other is simply called."""
    draw = getattr(noise_fn, "main_draw", noise_fn)
    return draw(size=shape, dtype=torch.float, device=device).contiguous()


def _arm(noise_fn, given):
    """A SceneNoise starts a new loop here: its draw numbers go back to 0 and it learns whether the loop draws for a given part."""
    if isinstance(noise_fn, SceneNoise):
        noise_fn.arm(given.inplace)


def _last(states, shape):
    for x in states:
        pass
    assert x.shape == tuple(shape)
    return x


class GaussianDiffusion:
    def __init__(self, config, betas, loss_type, model_mean_type, model_var_type, loss_separate, loss_iou,
                 train_stats_file):
        self.objectness_dim = config.get("objectness_dim", 1)
        self.class_dim = config.get("class_dim", 21)
        self.translation_dim = config.get("translation_dim", 3)
        self.size_dim = config.get("size_dim", 3)
        self.angle_dim = config.get("angle_dim", 1)
        self.bbox_dim = self.translation_dim + self.size_dim + self.angle_dim
        self.objfeat_dim = config.get("objfeat_dim", 0)
        self.loss_separate = loss_separate
        self.loss_iou = loss_iou
        self.train_stats_file = train_stats_file
        if self.loss_iou:
            with open(train_stats_file, "r") as f:
                train_stats = json.load(f)
            c = train_stats["bounds_translations"]
            self._centroids = (np.array(c[:3]), np.array(c[3:]))
            self._centroids_min = torch.from_numpy(self._centroids[0]).float()
            self._centroids_max = torch.from_numpy(self._centroids[1]).float()
            print('load centriods min {} and max {} in Gausssion Diffusion'.format(*self._centroids))
            s = train_stats["bounds_sizes"]
            self._sizes = (np.array(s[:3]), np.array(s[3:]))
            self._sizes_min = torch.from_numpy(self._sizes[0]).float()
            self._sizes_max = torch.from_numpy(self._sizes[1]).float()
            print('load sizes min {} and max {} in Gausssion Diffusion'.format(*self._sizes))
            a = train_stats["bounds_angles"]
            self._angles = (np.array(a[0]), np.array(a[1]))
        self.room_partial_condition = config.get("room_partial_condition", False)
        self.room_arrange_condition = config.get("room_arrange_condition", False)
        self.loss_type = loss_type
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        assert isinstance(betas, np.ndarray)
        self.np_betas = betas = betas.astype(np.float64)
        assert (betas > 0).all() and (betas <= 1).all()
        timesteps, = betas.shape
        self.num_timesteps = int(timesteps)

        # float64 numpy -> fp32 torch, op for op as the reference (:168-203) so the tables are bit-identical
        alphas = 1. - betas
        alphas_cumprod = torch.from_numpy(np.cumprod(alphas, axis=0)).float()
        alphas_cumprod_prev = torch.from_numpy(np.append(1., alphas_cumprod[:-1])).float()
        self.betas = torch.from_numpy(betas).float()
        self.alphas_cumprod = alphas_cumprod.float()
        self.alphas_cumprod_prev = alphas_cumprod_prev.float()
        self.sqrt_alphas_cumprod = torch.sqrt(alphas_cumprod).float()
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1. - alphas_cumprod).float()
        self.log_one_minus_alphas_cumprod = torch.log(1. - alphas_cumprod).float()
        self.sqrt_recip_alphas_cumprod = torch.sqrt(1. / alphas_cumprod).float()
        self.sqrt_recipm1_alphas_cumprod = torch.sqrt(1. / alphas_cumprod - 1).float()
        betas_t = torch.from_numpy(betas).float()
        alphas_t = torch.from_numpy(alphas).float()
        posterior_variance = betas_t * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod)
        self.posterior_variance = posterior_variance
        self.posterior_log_variance_clipped = torch.log(
            torch.max(posterior_variance, 1e-20 * torch.ones_like(posterior_variance)))
        self.posterior_mean_coef1 = betas_t * torch.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod)
        self.posterior_mean_coef2 = (1. - alphas_cumprod_prev) * torch.sqrt(alphas_t) / (1. - alphas_cumprod)
        snr = alphas_cumprod / (1 - alphas_cumprod)
        if model_mean_type == 'eps':
            loss_weight = torch.ones_like(snr)
        elif model_mean_type == 'x0':
            loss_weight = snr
        elif model_mean_type == 'v':
            loss_weight = snr / (snr + 1)
        self.loss_weight = loss_weight
        # sigma_t = exp(0.5 * log-variance) of p_sample (:350), tabulated with the same fp32 torch ops
        self._sigma_small = torch.exp(0.5 * self.posterior_log_variance_clipped)
        self._logvar_large = torch.log(torch.cat([self.posterior_variance[1:2], self.betas[1:]]))
        self._sigma_large = torch.exp(0.5 * self._logvar_large)
        self._dev = {}
        self._graphs = {}
        self._ddim_host = {}
        self._ddim_dev = {}

    # ------------------------------------------------------------------ device-resident tables
    _TABLE_NAMES = ("betas", "alphas_cumprod", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                    "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
                    "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2", "loss_weight",
                    "_sigma_small", "_sigma_large", "_logvar_large", "log_one_minus_alphas_cumprod")

    def tables(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("diffuscene_amd.GaussianDiffusion runs on a HIP device only (got %s); there is no CPU "
                               "fallback" % device)
        tb = self._dev.get(device)
        if tb is None:
            flat = torch.stack([getattr(self, n) for n in self._TABLE_NAMES]).to(device)
            tb = {n: flat[i] for i, n in enumerate(self._TABLE_NAMES)}
            self._dev[device] = tb
        return tb

    @staticmethod
    def _extract(a, t, x_shape):
        bs, = t.shape
        assert x_shape[0] == bs
        out = torch.gather(a, 0, t)
        assert out.shape == torch.Size([bs])
        return torch.reshape(out, [bs] + ((len(x_shape) - 1) * [1]))

    # -- parameterisation conversions (not on the fused fast path; device torch ops on resident tables) --
    def _predict_xstart_from_eps(self, x_t, t, eps):
        assert x_t.shape == eps.shape
        tb = self.tables(x_t.device)
        return (self._extract(tb["sqrt_recip_alphas_cumprod"], t, x_t.shape) * x_t -
                self._extract(tb["sqrt_recipm1_alphas_cumprod"], t, x_t.shape) * eps)

    def _predict_eps_from_start(self, x_t, t, x0):
        tb = self.tables(x_t.device)
        return ((self._extract(tb["sqrt_recip_alphas_cumprod"], t, x_t.shape) * x_t - x0) /
                self._extract(tb["sqrt_recipm1_alphas_cumprod"], t, x_t.shape))

    def _predict_v(self, x0, t, eps):
        tb = self.tables(x0.device)
        return (self._extract(tb["sqrt_alphas_cumprod"], t, x0.shape) * eps -
                self._extract(tb["sqrt_one_minus_alphas_cumprod"], t, x0.shape) * x0)

    def _predict_start_from_v(self, x_t, t, v):
        tb = self.tables(x_t.device)
        return (self._extract(tb["sqrt_alphas_cumprod"], t, x_t.shape) * x_t -
                self._extract(tb["sqrt_one_minus_alphas_cumprod"], t, x_t.shape) * v)

    def _coeffs(self, tb):
        """(ca, cb) of dsc_p_sample_f32 for the configured mean type."""
        if self.model_mean_type == 'v':
            return tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
        if self.model_mean_type == 'eps':
            return tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
        return None, None

    def _sigma(self, tb):
        if self.model_var_type == 'fixedsmall':
            return tb["_sigma_small"]
        if self.model_var_type == 'fixedlarge':
            return tb["_sigma_large"]
        raise NotImplementedError(self.model_var_type)

    def model_predictions(self, denoise_fn, x_t, t, condition, condition_cross, x_self_cond=None,
                          clip_x_start=False, rederive_pred_noise=False):
        model_output = denoise_fn(x_t, t, condition, condition_cross)
        clip = (lambda z: torch.clamp(z, min=-1., max=1.)) if clip_x_start else (lambda z: z)
        if self.model_mean_type == 'eps':
            pred_noise = model_output
            x_start = clip(self._predict_xstart_from_eps(x_t, t, pred_noise))
            if clip_x_start and rederive_pred_noise:
                pred_noise = self._predict_eps_from_start(x_t, t, x_start)
        elif self.model_mean_type == 'x0':
            x_start = clip(model_output)
            pred_noise = self._predict_eps_from_start(x_t, t, x_start)
        elif self.model_mean_type == 'v':
            x_start = clip(self._predict_start_from_v(x_t, t, model_output))
            pred_noise = self._predict_eps_from_start(x_t, t, x_start)
        return ModelPrediction(pred_noise, x_start)

    def q_mean_variance(self, x_start, t):
        tb = self.tables(x_start.device)
        mean = self._extract(tb["sqrt_alphas_cumprod"], t, x_start.shape) * x_start
        variance = self._extract(1. - tb["alphas_cumprod"], t, x_start.shape)
        log_variance = self._extract(tb["log_one_minus_alphas_cumprod"], t, x_start.shape)
        return mean, variance, log_variance

    def q_sample(self, x_start, t, noise=None):
        """q(x_t | x_0), reference :276-286 -- one HIP kernel."""
        if noise is None:
            noise = torch.randn(x_start.shape, device=x_start.device)
        assert noise.shape == x_start.shape
        tb = self.tables(x_start.device)
        return ops.q_sample(x_start.contiguous(), noise.contiguous(), t, tb["sqrt_alphas_cumprod"],
                            tb["sqrt_one_minus_alphas_cumprod"])

    def q_posterior_mean_variance(self, x_start, x_t, t):
        assert x_start.shape == x_t.shape
        tb = self.tables(x_start.device)
        posterior_mean = (self._extract(tb["posterior_mean_coef1"], t, x_t.shape) * x_start +
                          self._extract(tb["posterior_mean_coef2"], t, x_t.shape) * x_t)
        posterior_variance = self._extract(tb["posterior_variance"], t, x_t.shape)
        posterior_log_variance_clipped = self._extract(tb["posterior_log_variance_clipped"], t, x_t.shape)
        assert (posterior_mean.shape[0] == posterior_variance.shape[0] == posterior_log_variance_clipped.shape[0] ==
                x_start.shape[0])
        return posterior_mean, posterior_variance, posterior_log_variance_clipped

    def p_mean_variance(self, denoise_fn, data, t, condition, condition_cross, clip_denoised: bool,
                        return_pred_xstart: bool):
        """reference :305-335.  Mean and x_recon come from the fused kernel (zero noise)."""
        if self.model_var_type not in ('fixedsmall', 'fixedlarge'):
            raise NotImplementedError(self.model_var_type)
        model_output = denoise_fn(data, t, condition, condition_cross)
        tb = self.tables(data.device)
        ca, cb = self._coeffs(tb)
        if torch.is_grad_enabled() and model_output.requires_grad:
            # loss_type 'kl' training (:657-660): the KL back-propagates through model_mean to the denoiser, so this
            # branch stays on differentiable device ops over the same tables (the fused kernel has no autograd)
            if self.model_mean_type == 'eps':
                x_recon = self._predict_xstart_from_eps(data, t, eps=model_output)
            elif self.model_mean_type == 'x0':
                x_recon = model_output
            else:
                x_recon = self._predict_start_from_v(data, t, v=model_output)
            if clip_denoised:
                x_recon = torch.clamp(x_recon, -1.0, 1.0)
            model_mean, _, _ = self.q_posterior_mean_variance(x_start=x_recon, x_t=data, t=t)
        else:
            x_recon = torch.empty_like(data)
            model_mean = ops.p_sample(data.contiguous(), model_output.contiguous(), torch.zeros_like(data), t, ca, cb,
                                      tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], self._sigma(tb),
                                      _MEAN[self.model_mean_type], clip_denoised, x0_out=x_recon)
        var_tab = tb["posterior_variance"] if self.model_var_type == 'fixedsmall' else tb["betas"]
        logvar_tab = (tb["posterior_log_variance_clipped"] if self.model_var_type == 'fixedsmall'
                      else tb["_logvar_large"])
        model_variance = self._extract(var_tab, t, data.shape) * torch.ones_like(data)
        model_log_variance = self._extract(logvar_tab, t, data.shape) * torch.ones_like(data)
        assert model_mean.shape == x_recon.shape == data.shape
        assert model_variance.shape == model_log_variance.shape == data.shape
        if return_pred_xstart:
            return model_mean, model_variance, model_log_variance, x_recon
        return model_mean, model_variance, model_log_variance

    # ------------------------------------------------------------------ sampling
    def _posterior_step(self, data, model_output, t, noise_fn, clip_denoised, x0_out=None, draw=None):
        """The update of one reverse step, reference :344-352: ONE noise draw (also at t == 0), then the fused x0-from-output / clamp /
        posterior-mean / masked noise-add kernel.  ``draw``: the keywords of the draw where they are not the reference's."""
        noise = noise_fn(**(draw or dict(size=data.shape, dtype=data.dtype, device=data.device)))
        assert noise.shape == data.shape
        tb = self.tables(data.device)
        ca, cb = self._coeffs(tb)
        sample = ops.p_sample(data.contiguous(), model_output.contiguous(), noise.contiguous(), t, ca, cb,
                              tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], self._sigma(tb),
                              _MEAN[self.model_mean_type], clip_denoised, x0_out=x0_out)
        assert sample.shape == data.shape
        return sample

    def p_sample(self, denoise_fn, data, t, condition, condition_cross, noise_fn, clip_denoised=False,
                 return_pred_xstart=False):
        """One reverse step, reference :339-352: model call, then _posterior_step."""
        model_output = denoise_fn(data, t, condition, condition_cross)
        pred_xstart = torch.empty_like(data) if return_pred_xstart else None
        sample = self._posterior_step(data, model_output, t, noise_fn, clip_denoised, pred_xstart)
        return (sample, pred_xstart) if return_pred_xstart else sample

    def _total_steps(self, keep_running):
        return self.num_timesteps if not keep_running else len(self.betas)

    def _say_last(self):
        print('last:', 0, self.num_timesteps, len(self.betas))          # the reference's print at t == 0 (:469, :497)

    # the two eager loops (module docstring); a state that a given part overwrites in place stays the same tensor until the update
    def _t_states(self, model, shape, device, noise_fn, clip_denoised, total_steps, given=_FREE, draw=None, jumps=None):
        """The T-step loop, reference :355-371: fill t_, [overwrite the given part], model call, one draw, ops.p_sample -- at t == 0 too.
        ``jumps`` = (schedule, (ja, jb), j) of _resample_inputs: the loop walks the schedule's op list instead -- a call is the step
        below, a jump one more main draw and dsc_resample_jump_f32 on the whole state at t = s."""
        _arm(noise_fn, given)
        x = noise_fn(size=shape, dtype=torch.float, device=device)
        if given.inplace:
            x = x.clone()                       # a caller's tensor (a row of a NoiseReplay buffer) is not written
        yield x
        if jumps is not None:
            sched, (ja, jb), j = jumps
            for op, u in sched.ops:
                t_ = torch.empty(shape[0], dtype=torch.int64, device=device).fill_(u)
                if op == "jump":
                    ops.resample_jump(x, _jump_draw(noise_fn, shape, device), ja, jb, j, t=t_)
                    continue
                given.before(x, t_)
                x = self._posterior_step(x, model(x, t_), t_, noise_fn, clip_denoised, draw=draw)
                yield given.finish(x) if u == 0 else x
            return
        for t in reversed(range(0, total_steps)):
            t_ = torch.empty(shape[0], dtype=torch.int64, device=device).fill_(t)
            given.before(x, t_)
            x = self._posterior_step(x, model(x, t_), t_, noise_fn, clip_denoised, draw=draw)
            yield given.finish(x) if t == 0 else x      # not a copy: ``given.before`` of the next step writes into it (keep a clone)

    def _strided_states(self, model, shape, device, noise_fn, S, eta, given=_FREE, multistep=None, jumps=None):
        """The strided (DDIM) loop, reference :402-444: a device step counter, [overwrite the given part], model call, a draw except on
        the last pair ((t, -1) takes x_start), ddim_step, ddim_advance.  ``multistep`` = (the (B,) guidance scales or None,): the
        DPM-Solver++(2M) launch (dsc_multistep_x0_f32) on the (steered) model output of every pair but the last, before ddim_step; the
        x0 history and the weight table live here."""
        dtab = self.ddim_tables(S, eta, device)
        pairs = dtab[0]
        step = torch.zeros((1,), dtype=torch.int64, device=device)
        solve = None
        if multistep is not None:
            hist = torch.empty(tuple(shape), dtype=torch.float32, device=device)
            weights = self.multistep_table(S, device)
            coeffs = self._coeffs(self.tables(device))

            def solve(x, mo):
                ops.issue(ops.multistep_rec(x.contiguous(), mo, hist, weights, _MEAN[self.model_mean_type], coeffs,
                                            strided=(step,) + tuple(dtab[1:]), scale=multistep[0], **given.steer_operands()))
        t_ = torch.empty(shape[0], dtype=torch.int64, device=device).fill_(pairs[0][0])
        _arm(noise_fn, given)
        x = noise_fn(size=shape, dtype=torch.float, device=device)
        if given.inplace:
            x = x.clone()
        yield x
        if jumps is not None:                   # walk the op list: the pair of call u is k = S - 1 - u, where the counter stands
            sched, (ja, jb), j = jumps
            for op, u in sched.ops:
                if op == "jump":                # the counter stands on the pair at s: jump, then seek back j pairs
                    ops.resample_jump(x, _jump_draw(noise_fn, shape, device), ja, jb, j, strided=(step, dtab[1]))
                    ops.ddim_seek(step, dtab[1], t_, -j)
                    continue
                given.before(x, t_)
                last = u == 0
                model_output = model(x, t_)
                noise = x if last else noise_fn(size=shape, dtype=torch.float, device=device)
                x = self.ddim_step(x.contiguous(), model_output.contiguous(), noise.contiguous(), step, dtab)
                if not last:
                    ops.ddim_advance(step, dtab[1], t_)
                yield given.finish(x) if last else x
            return
        for time, time_next in pairs:
            given.before(x, t_)
            last = time_next < 0
            model_output = model(x, t_) if solve is None or last else model(x, t_, solve)
            noise = x if last else noise_fn(size=shape, dtype=torch.float, device=device)      # not read on the last pair
            x = self.ddim_step(x.contiguous(), model_output.contiguous(), noise.contiguous(), step, dtab)
            if not last:
                ops.ddim_advance(step, dtab[1], t_)
            yield given.finish(x) if last else x        # not a copy, as in _t_states

    def p_sample_loop(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn,
                      clip_denoised=True, keep_running=False, graph=None,
                      collision_scale=None, collision_steps=None, wall_scale=None, wall_steps=None, room_side=None, room_mask=None):
        """Generate samples, reference :355-371 (draw order: x_T, then one draw per step)."""
        return self._loop("p_sample_loop", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          clip_denoised=clip_denoised, keep_running=keep_running,
                          **_steer_kw(collision_scale, collision_steps), **_wall_kw(wall_scale, wall_steps, room_side, room_mask))

    def _loop(self, what, denoise_fn, shape, device, condition, condition_cross, noise_fn, graph, strided=None, given=None, scale=None,
              clip_denoised=True, keep_running=False, say_last=False, all_states=False, steer=None, multistep=None, walls=None,
              resample=None):
        """What every public loop does behind its signature.  The spec: ``strided`` = (sampling_timesteps, ddim_sampling_eta) or None for
        T steps; ``given`` = None, ("dense", partial_boxes), ("ragged", partial_boxes, num_partial) or ("mask", known, mask); ``scale`` =
        the guidance scale or None.  Validates (ValueError names ``what``), keeps (eta, S) on the instance as the reference does (:404-405),
        hands over to the captured loop under _use_graph -- the front end front_end_name(spec) of sampler.py, looked up when called -- and
        otherwise runs the eager core on the given part and the model call of the spec.  ``say_last``: the reference's print, after the
        eager loop / before the captured one; ``all_states``: the list of states (eager).  ``steer`` = (collision_scale, collision_steps)
        or None: collision steering after every model call (_steer_inputs), on either path.  ``multistep`` = the name of a multistep
        solver (ops.SOLVERS) or None: the strided loop takes its steps on the solver's extrapolated x0 (_check_solver).
        ``walls`` = (wall_scale, wall_steps, room_side, room_mask) or None: floor-plan steering after the collision steering
        (_wall_inputs), on either path.  ``resample`` = ((jump_length, n_resample), resample_steps) or None: RePaint's resampling jumps
        (_check_resample, _resample_inputs) on a loop with a given part, on either path."""
        assert isinstance(shape, (tuple, list))
        if strided is not None:
            S, eta = _check_ddim(self.num_timesteps, *strided)
        if multistep is not None:
            _check_solver(multistep, strided, what)
        if resample is not None:
            resample = self._check_resample(what, *resample, given=given, multistep=multistep, all_states=all_states)
        kind, values = (None, ()) if given is None else (given[0], given[1:])
        if kind == "dense":
            values = (values[0].contiguous(),)
        elif kind == "ragged":
            values = self._ragged_inputs(shape, device, *values, what)
        elif kind == "mask":
            values = self._masked_inputs(shape, device, *values, what)
        if steer is not None:
            steer = self._steer_inputs(shape, device, *steer, what)
        if walls is not None:
            walls = self._wall_inputs(shape, device, *walls, what)
        if scale is not None:
            condition, condition_cross, scale = self._guided_inputs(shape, device, condition, condition_cross, scale, what)
        if strided is not None:
            self.ddim_sampling_eta, self.sampling_timesteps = eta, S
            sched = (S, eta)
        else:
            sched = (clip_denoised, self._total_steps(keep_running))
        # (schedule, (ja, jb) on the device, j), or None where the schedule holds no jump: then the loop is the one without the keyword
        jumps = None if resample is None else self._resample_inputs(device, *resample, *((S, eta) if strided is not None else (sched[1],)))
        jump_kw = {} if jumps is None else dict(jumps=jumps)
        if not all_states and _use_graph(graph, noise_fn, denoise_fn):
            from .. import sampler
            if say_last:
                self._say_last()
            front = getattr(sampler, front_end_name(strided is not None, kind, scale is not None))
            return front(self, denoise_fn, tuple(shape), device, condition, condition_cross, *(() if scale is None else (scale,)), *sched,
                         noise_fn, *values, **({} if steer is None else dict(steer=steer)),
                         **({} if multistep is None else dict(multistep=self.multistep_table(S, device))),
                         **({} if walls is None else dict(walls=walls)), **jump_kw)
        part = _FREE if kind is None else {"dense": _GivenRows, "ragged": _GivenRagged, "mask": _GivenMask}[kind](
            self, device, noise_fn, *((shape,) if kind == "mask" else ()), *values)
        model = _model(denoise_fn, condition, condition_cross) if scale is None else _guided_model(denoise_fn, condition, condition_cross, scale)
        if steer is not None or walls is not None:
            model = _corrected(model, self, device, part, scale, steer, walls)
        if strided is not None:
            states = self._strided_states(model, shape, device, noise_fn, S, eta, part,
                                          *(() if multistep is None else ((scale,),)), **jump_kw)
        elif scale is not None and kind is None:        # p_sample_loop_guided: the device check before the first draw, its own draw keywords
            self.tables(device)
            states = self._t_states(model, shape, device, noise_fn, *sched, part, draw=dict(size=shape, dtype=torch.float, device=device))
        else:
            states = self._t_states(model, shape, device, noise_fn, *sched, part, **jump_kw)
        if all_states:
            imgs = list(states)
            assert imgs[-1].shape == tuple(shape)
            return imgs
        img = _last(states, shape)
        if say_last:
            self._say_last()
        return img

    # ------------------------------------------------------------------ resampling jumps (RePaint)
    def _check_resample(self, what, resample, resample_steps, given=None, multistep=None, all_states=False):
        """The refusals of ``resample`` / ``resample_steps``, before anything is drawn or computed -> (j, r, K)."""
        if resample is None:
            raise ValueError("%s: resample_steps goes with resample=(jump_length, n_resample)" % what)
        j, r = ops.resample_pair(resample, what)
        k = ops.resample_steps_value(resample_steps, self.num_timesteps, what)
        if given is None:
            raise ValueError("%s: resample needs a given part (completion, in-painting): nothing is given here" % what)
        if multistep is not None:
            raise ValueError("%s: resample does not combine with sampling_solver=%r: the x0 history is void after a jump" % (what, multistep))
        if all_states:
            raise ValueError("%s: resample returns the final scenes only (no trajectory)" % what)
        if self.room_partial_condition or self.room_arrange_condition:
            raise ValueError("%s: resample on a room_partial_condition / room_arrange_condition model: its condition tensors already "
                             "encode a prefix / a sub-shape of the scene" % what)
        return j, r, k

    def resample_schedule(self, jump_length, n_resample, resample_steps=None, total_steps=None, sampling_timesteps=None):
        """The op list and the counts of a resampled loop (ops.resample_schedule): of the T-step loop of ``total_steps`` (default T)
        steps, or of the strided loop of ``sampling_timesteps`` pairs on ddim_schedule's times."""
        if sampling_timesteps is None:
            return ops.resample_schedule(self.num_timesteps if total_steps is None else total_steps, jump_length, n_resample,
                                         resample_steps=resample_steps)
        pairs, _ = self.ddim_schedule(sampling_timesteps, 0.0)
        return ops.resample_schedule(len(pairs), jump_length, n_resample, [p[0] for p in pairs], resample_steps)

    def jump_table(self, jump_length, device, sampling_timesteps=None):
        """(ja, jb) of ops.jump_tables from the float64 alphas_cumprod, on ``device``: T rows indexed by s, or -- strided -- S rows indexed
        by the step counter on ddim_schedule's times; once per (j, S, device)."""
        device = torch.device(device)
        key = ("jump", int(jump_length), sampling_timesteps, device)
        hit = self._ddim_dev.get(key)
        if hit is None:
            times = None if sampling_timesteps is None else [p[0] for p in self.ddim_schedule(sampling_timesteps, 0.0)[0]]
            hit = tuple(tb.to(device) for tb in ops.jump_tables(np.cumprod(1. - self.np_betas, axis=0), jump_length, times))
            self._ddim_dev[key] = hit
        return hit

    def _resample_inputs(self, device, j, r, k, U, eta=None):
        """(schedule, (ja, jb) on the device, j) of a resampled loop of ``U`` calls (strided when ``eta`` is given), or None where the
        schedule holds no jump -- r == 1, j >= U, K below every jump point's time: the loop is then the one without the keyword."""
        sched = self.resample_schedule(j, r, k, *((U,) if eta is None else (None, U)))
        if sched.jumps == 0:
            return None
        return sched, self.jump_table(j, device, None if eta is None else U), j

    def p_sample_loop_trajectory(self, denoise_fn, shape, device, freq, condition, condition_cross,
                                 noise_fn=torch.randn, clip_denoised=True, keep_running=False):
        """reference :373-398"""
        assert isinstance(shape, (tuple, list))
        total_steps = self._total_steps(keep_running)
        states = self._t_states(_model(denoise_fn, condition, condition_cross), shape, device, noise_fn, clip_denoised, total_steps)
        imgs = [next(states)]
        for t, img_t in zip(reversed(range(0, total_steps)), states):
            if t % freq == 0 or t == total_steps - 1:
                imgs.append(img_t)
        assert imgs[-1].shape == shape
        return imgs

    # ------------------------------------------------------------------ DDIM (reference :401-444)
    def ddim_schedule(self, sampling_timesteps, ddim_sampling_eta):
        """Host side of ddim_sample_loop: the (t, t_next) pairs exactly as the reference derives them (:409-411: float32 linspace,
        truncating .int(), the last pair ends at -1) and the (3, S) float32 rows [sqrt(alpha_next), c, sigma] from the reference's own
        scalar expressions (:428-432; zeros on the final pair, which takes x_start).  Cached per (S, eta)."""
        S, eta = _check_ddim(self.num_timesteps, sampling_timesteps, ddim_sampling_eta)
        key = (S, eta)
        hit = self._ddim_host.get(key)
        if hit is not None:
            return hit
        times = torch.linspace(-1, self.num_timesteps - 1, steps=S + 1)
        times = list(reversed(times.int().tolist()))
        pairs = list(zip(times[:-1], times[1:]))
        coef = torch.zeros((3, S), dtype=torch.float32)
        for k, (time, time_next) in enumerate(pairs):
            if time_next < 0:
                continue
            alpha = self.alphas_cumprod[time]
            alpha_next = self.alphas_cumprod[time_next]
            sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            coef[0, k] = alpha_next.sqrt()
            coef[1, k] = c
            coef[2, k] = sigma
        self._ddim_host[key] = (pairs, coef)
        return pairs, coef

    def ddim_tables(self, sampling_timesteps, ddim_sampling_eta, device):
        """Device copy of ddim_schedule: (pairs, times (S,) int64, times_next (S,) int64, coef (3, S) fp32), once per (S, eta, device)."""
        pairs, coef = self.ddim_schedule(sampling_timesteps, ddim_sampling_eta)
        device = torch.device(device)
        key = (len(pairs), float(ddim_sampling_eta), device)
        hit = self._ddim_dev.get(key)
        if hit is None:
            self.tables(device)                 # the device check
            times = torch.tensor([p[0] for p in pairs], dtype=torch.int64).to(device)
            times_next = torch.tensor([p[1] for p in pairs], dtype=torch.int64).to(device)
            hit = (pairs, times, times_next, coef.to(device))
            self._ddim_dev[key] = hit
        return hit

    def multistep_table(self, sampling_timesteps, device):
        """The (S,) float32 history weights of DPM-Solver++(2M) on the pairs of ddim_schedule(S, 0) (ops.multistep_weights, from the
        float64 alphas_cumprod), on ``device``; once per (S, device)."""
        device = torch.device(device)
        key = ("multistep", int(sampling_timesteps), device)
        hit = self._ddim_dev.get(key)
        if hit is None:
            pairs, _ = self.ddim_schedule(sampling_timesteps, 0.0)
            hit = ops.multistep_weights(pairs, np.cumprod(1. - self.np_betas, axis=0)).to(device)
            self._ddim_dev[key] = hit
        return hit

    def ddim_step(self, x_t, model_output, noise, step, dtab, out=None, x0_out=None):
        """One DDIM update at the step held by the device counter ``step`` (dtab = ddim_tables(...)): the fused HIP kernel."""
        _, times, times_next, coef = dtab
        tb = self.tables(x_t.device)
        ca, cb = self._coeffs(tb)
        return ops.ddim_step(x_t, model_output, noise, step, times, times_next, coef, ca, cb, tb["sqrt_recip_alphas_cumprod"],
                             tb["sqrt_recipm1_alphas_cumprod"], _MEAN[self.model_mean_type], out=out, x0_out=x0_out)

    @torch.no_grad()
    def ddim_sample_loop(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn, clip_denoised=True,
                         sampling_timesteps=50, ddim_sampling_eta=0., return_all_timesteps=False, graph=None,
                         collision_scale=None, collision_steps=None,
                         wall_scale=None, wall_steps=None, room_side=None, room_mask=None, sampling_solver=None):
        """DDIM sampling, reference :402-444 (its two call-site slips bridged: model_predictions gets ``denoise_fn``, and there is no
        self-conditioning).  Draw order: x_T, then one draw per pair except the last ((t, -1) takes x_start): S draws in all.
        x_start is always clamped to [-1, 1], as in the reference, whatever ``clip_denoised`` says.  The network runs on the static
        plan, each update is one HIP kernel (dsc_ddim_step_f32); by default (``graph=None``, the rules of p_sample_loop) the loop is a
        replayed hipGraph step.  ``return_all_timesteps=True`` returns the S + 1 states (eager loop).
        ``sampling_solver`` (None: this loop as it was; "dpmpp_2m", on every strided loop): the multistep DPM-Solver++(2M) -- one more
        launch per pair (dsc_multistep_x0_f32) moves the model output so that the unchanged step runs on the extrapolated x0 estimate
        D = x0 + e_k (x0 - x0_prev); same draws, needs ddim_sampling_eta == 0, S <= 2 is DDIM bit for bit."""
        return self._loop("ddim_sample_loop", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          strided=(sampling_timesteps, ddim_sampling_eta), all_states=return_all_timesteps,
                          **_steer_kw(collision_scale, collision_steps),
                          **_wall_kw(wall_scale, wall_steps, room_side, room_mask), **_solver_kw(sampling_solver))

    # ------------------------------------------------------------------ classifier-free guidance
    def _guided_inputs(self, shape, device, condition, condition_cross, guidance_scale, what):
        """(condition at 2 B, condition_cross at 2 B = cat([cross, zeros]), scale (B,) f32 on the device) of a guided loop."""
        B = shape[0]
        if condition_cross is None or not isinstance(condition_cross, torch.Tensor) or condition_cross.dim() != 3 \
                or condition_cross.shape[0] != B:
            raise ValueError("%s needs condition_cross (B, L, text_embed_dim): guidance contrasts the text features with the null "
                             "condition (all zeros)" % what)
        scale = ops.guidance_scales(guidance_scale, B, device)
        cross2 = torch.cat([condition_cross, torch.zeros_like(condition_cross)], dim=0).contiguous()
        cond2 = condition
        if condition is not None:
            # a stride-0 (per-slot) condition stays per-slot at 2 B; any other is repeated for the null half
            cond2 = condition[:1].expand(2 * B, -1, -1) if condition.stride(0) == 0 else torch.cat([condition, condition], dim=0).contiguous()
        return cond2, cross2, scale

    # ------------------------------------------------------------------ collision steering
    def box_bounds(self, keyword="collision_scale"):
        """The de-normalisation bounds of the boxes, 12 floats (translation lo[3], hi[3], size lo[3], hi[3]), from the train-stats file
        (``bounds_translations`` / ``bounds_sizes``); loaded on first use whether or not ``loss_iou`` is set.  ``keyword``: the one a
        refusal names."""
        hit = getattr(self, "_box_bounds", None)
        if hit is None:
            if self.loss_iou:
                c, s = np.concatenate(self._centroids), np.concatenate(self._sizes)
            else:
                if not self.train_stats_file:
                    raise ValueError("%s needs the de-normalisation bounds of the boxes: set train_stats_file "
                                     "(diffusion_kwargs) to the dataset's statistics file" % keyword)
                with open(self.train_stats_file, "r") as f:
                    train_stats = json.load(f)
                c, s = train_stats["bounds_translations"], train_stats["bounds_sizes"]
            hit = self._box_bounds = tuple(float(v) for v in np.float32(list(c) + list(s)))
            if len(hit) != 12:
                raise ValueError("train_stats_file: bounds_translations and bounds_sizes must hold 6 numbers each")
        return hit

    def _check_steer_layout(self, shape, noun, what):
        """The refusals every steering term shares: it reads boxes in the full object layout, one thread per box."""
        B, N, C = shape
        if (self.translation_dim, self.size_dim, self.angle_dim) != (3, 3, 2):
            raise ValueError("%s: %s needs translation_dim = 3, size_dim = 3 and angle_dim = 2 (cos, sin), got %d / %d / %d"
                             % (what, noun, self.translation_dim, self.size_dim, self.angle_dim))
        if self.class_dim < 1 or C < self.bbox_dim + self.class_dim:
            raise ValueError("%s: %s needs the full object layout, at least %d channels, got %d"
                             % (what, noun, self.bbox_dim + max(self.class_dim, 1), C))
        if N > ops.STEER_MAX_OBJECTS:
            raise ValueError("%s: %s handles at most %d objects per scene, got %d" % (what, noun, ops.STEER_MAX_OBJECTS, N))

    def _steer_inputs(self, shape, device, collision_scale, collision_steps, what):
        """(weight (B,) f32 on the device, K, bounds, bbox_dim, class_dim) of a steered loop (ops.steer_rec), or ValueError -- before
        anything is drawn.  At every step whose t < K the clamped x0 estimate of scene b moves by -weight[b] * d E / d x0[:, 0:3], E the
        pairwise IoU of its non-empty boxes; ``collision_steps`` None steers every step."""
        B, N, C = shape
        if collision_scale is None:
            raise ValueError("%s: collision_steps goes with collision_scale" % what)
        self._check_steer_layout(shape, "collision steering", what)
        weight = ops.collision_scales(collision_scale, B, "cpu")
        k = ops.collision_steps(collision_steps, self.num_timesteps)
        return weight.to(device), k, self.box_bounds(), self.bbox_dim, self.class_dim

    def _wall_inputs(self, shape, device, wall_scale, wall_steps, room_side, room_mask, what, field=True):
        """(weight (B,) f32 on the device, K, bounds, bbox_dim, class_dim, field (B or 1, H, W) f32 on the device, room_side) of a loop
        under floor-plan steering (ops.walls_rec), or ValueError -- before anything is drawn.  At every step whose t < K the clamped x0
        estimate of scene b moves by -weight[b] * d E / d x0[:, {0, 2}], E the out-of-room energy of the footprints of its non-empty
        boxes over the distance field of ``room_mask``; ``wall_steps`` None steers every step.  ``field=False``: the
        checks alone (the field is None)."""
        B, N, C = shape
        if wall_scale is None:
            raise ValueError("%s: wall_steps and room_side go with wall_scale" % what)
        if room_side is None:
            raise ValueError("%s: wall_scale needs room_side, half the side in metres of the window the room mask was rendered in" % what)
        side = ops.room_side_value(room_side)
        if room_mask is None:
            raise ValueError("%s: wall_scale needs the room_mask" % what)
        ops.room_mask_dims(room_mask, B)
        self._check_steer_layout(shape, "floor-plan steering", what)
        weight = ops.wall_scales(wall_scale, B, "cpu")
        k = ops.wall_steps(wall_steps, self.num_timesteps)
        return (weight.to(device), k, self.box_bounds("wall_scale"), self.bbox_dim, self.class_dim,
                ops.floor_field(room_mask.to(device), side) if field else None, side)

    @torch.no_grad()
    def p_sample_loop_guided(self, denoise_fn, shape, device, condition, condition_cross, guidance_scale, noise_fn=torch.randn,
                             clip_denoised=True, keep_running=False, graph=None,
                             collision_scale=None, collision_steps=None, wall_scale=None, wall_steps=None, room_side=None, room_mask=None):
        """Classifier-free guidance in T steps.  Scene b is the reference's p_sample_loop (:355-371) with
        m = u + w[b] * (c - u) in place of the model output inside p_mean_variance: c the denoiser on (x, t, condition, condition_cross),
        u the denoiser on (x, t, condition, 0) -- the null condition is condition_cross == 0, the features AFTER fc_text_f --, the
        difference, the product and the sum each rounded on its own.  eps, x0 and v are linear in each other given x_t, so guiding the
        raw output is the same guidance under all three mean types.  ``guidance_scale``: a float or B per-scene values
        (ops.guidance_scales); 1 is the conditional model up to rounding, 0 the null-conditioned one.  Draws: exactly those of
        p_sample_loop at batch B, in its order; both halves of the 2 B model call see the same x_t.  This eager loop is built from the
        unfused pieces -- the denoiser at 2 B, cfg_combine, p_sample; the graph path (the default, by the rules of p_sample_loop)
        replays one captured step whose update is the fused dsc_p_sample_cfg_f32, bit-identical."""
        return self._loop("p_sample_loop_guided", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          scale=guidance_scale, clip_denoised=clip_denoised, keep_running=keep_running,
                          **_steer_kw(collision_scale, collision_steps), **_wall_kw(wall_scale, wall_steps, room_side, room_mask))

    @torch.no_grad()
    def ddim_guided_loop(self, denoise_fn, shape, device, condition, condition_cross, guidance_scale, noise_fn=torch.randn,
                         sampling_timesteps=50, ddim_sampling_eta=0., graph=None,
                         collision_scale=None, collision_steps=None,
                         wall_scale=None, wall_steps=None, room_side=None, room_mask=None, sampling_solver=None):
        """Classifier-free guidance in S strided (DDIM) steps: scene b is the reference's ddim_sample_loop (:402-444) with the guided
        output m of p_sample_loop_guided in place of the model output inside model_predictions.  x_start is always clamped to [-1, 1].
        Draws: exactly those of ddim_sample_loop at batch B (x_T, then one per pair except the last).  The eager loop is built from the
        unfused pieces (the denoiser at 2 B, cfg_combine, ddim_step); the graph path replays one captured step whose update is the fused
        dsc_ddim_cfg_step_f32, bit-identical."""
        return self._loop("ddim_guided_loop", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          strided=(sampling_timesteps, ddim_sampling_eta), scale=guidance_scale,
                          **_steer_kw(collision_scale, collision_steps),
                          **_wall_kw(wall_scale, wall_steps, room_side, room_mask), **_solver_kw(sampling_solver))

    # ------------------------------------------------------------------ completion, in-painting, re-arrangement
    def p_sample_loop_complete(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn,
                               clip_denoised=True, keep_running=False, partial_boxes=None, graph=None,
                               collision_scale=None, collision_steps=None,
                               wall_scale=None, wall_steps=None, room_side=None, room_mask=None,
                               resample=None, resample_steps=None):
        """Scene completion, reference :447-476: every step re-noises the given objects (noise drawn BEFORE the
        model call) and overwrites the first P rows of x_t in place; at t == 0 the clean objects are restored."""
        return self._loop("p_sample_loop_complete", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          given=("dense", partial_boxes), clip_denoised=clip_denoised, keep_running=keep_running, say_last=True,
                          **_steer_kw(collision_scale, collision_steps), **_wall_kw(wall_scale, wall_steps, room_side, room_mask),
                          **_resample_kw(resample, resample_steps))

    @torch.no_grad()
    def p_sample_loop_complete_ragged(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn,
                                      clip_denoised=True, keep_running=False, partial_boxes=None, num_partial=None, graph=None,
                                      collision_scale=None, collision_steps=None,
                                      wall_scale=None, wall_steps=None, room_side=None, room_mask=None,
                                      resample=None, resample_steps=None):
        """Scene completion of a batch whose scenes are given DIFFERENT numbers of objects.  ``partial_boxes`` is (B, Pmax, C) with
        1 <= Pmax <= N, ``num_partial`` the (B,) integer counts, 0 <= num_partial[b] <= Pmax; rows >= num_partial[b] of scene b are
        padding and never read.  Scene b is the reference's p_sample_loop_complete (:447-476) run on that scene alone with
        partial_boxes[b, :num_partial[b]]: a count of 0 is plain generation, a count of N returns the given scene.  Draw order: x_T,
        then per step noise_fn(size=(B, Pmax, C)) (rows at or beyond the count are ignored) followed by noise_fn(size=(B, N, C)).
        This eager loop is built from the unfused pieces -- ragged overwrite, p_sample, restore; the graph path (the default, by the
        rules of p_sample_loop) replays one captured step whose update is the fused dsc_p_sample_inpaint_f32, bit-identical."""
        return self._loop("p_sample_loop_complete_ragged", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          given=("ragged", partial_boxes, num_partial), clip_denoised=clip_denoised, keep_running=keep_running, say_last=True,
                          **_steer_kw(collision_scale, collision_steps), **_wall_kw(wall_scale, wall_steps, room_side, room_mask),
                          **_resample_kw(resample, resample_steps))

    @torch.no_grad()
    def ddim_complete_ragged_loop(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn,
                                  sampling_timesteps=50, ddim_sampling_eta=0., partial_boxes=None, num_partial=None, graph=None,
                                  collision_scale=None, collision_steps=None,
                                  wall_scale=None, wall_steps=None, room_side=None, room_mask=None, sampling_solver=None,
                                  resample=None, resample_steps=None):
        """Strided (DDIM) scene completion of a batch with per-scene numbers of given objects.  Scene b is ddim_sample_loop (reference
        :402-444) run on that scene alone with ONE addition taken from p_sample_loop_complete (:447-476): before every model call at pair
        (t, t_next) the first num_partial[b] rows of the state are overwritten in place with q_sample(partial_boxes[b], t, fresh noise);
        after the last pair the given rows are restored to the clean objects.  The DDIM update reads x_t only through x_start and
        pred_noise, so the overwrite in front of the model call is the whole change.  ``partial_boxes`` / ``num_partial`` as in
        p_sample_loop_complete_ragged: a count of 0 is plain gen_samples_ddim on the main draws, a count of N returns the given scene.
        Draw order: x_T (B, N, C); then per pair a partial draw (B, Pmax, C), the model call and a main draw (B, N, C); the last pair
        (t, -1) makes the partial draw but no main draw -- 2 S draws in all.  x_start is always clamped to [-1, 1], as in
        ddim_sample_loop.  The given rows are re-noised with fresh noise at every pair whatever eta is: at eta = 0 the free rows are
        deterministic given x_T AND the partial draws, not given x_T alone.
        This eager loop is built from the unfused pieces -- ragged overwrite at the pair's t, model call, ddim_step, ddim_advance,
        restore; the graph path (the default, by the rules of p_sample_loop) replays one captured step whose update is the fused
        dsc_ddim_inpaint_step_f32, bit-identical."""
        return self._loop("ddim_complete_ragged_loop", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          strided=(sampling_timesteps, ddim_sampling_eta), given=("ragged", partial_boxes, num_partial),
                          **_steer_kw(collision_scale, collision_steps),
                          **_wall_kw(wall_scale, wall_steps, room_side, room_mask), **_solver_kw(sampling_solver),
                          **_resample_kw(resample, resample_steps))

    def _ragged_inputs(self, shape, device, partial_boxes, num_partial, what):
        """(partial_boxes (B, Pmax, C) contiguous, counts (B,) int64 on the device: ops.ragged_counts) of a ragged completion loop."""
        B, N, C = shape
        if partial_boxes is None or num_partial is None:
            raise ValueError("%s needs partial_boxes (B, Pmax, C) and num_partial (B,)" % what)
        if partial_boxes.dim() != 3 or partial_boxes.shape[0] != B or partial_boxes.shape[2] != C or not 1 <= partial_boxes.shape[1] <= N:
            raise ValueError("partial_boxes must be (%d, 1 <= Pmax <= %d, %d), got %s" % (B, N, C, tuple(partial_boxes.shape)))
        partial_boxes = partial_boxes.contiguous()
        return partial_boxes, ops.ragged_counts(num_partial, B, partial_boxes.shape[1], device)

    def _masked_inputs(self, shape, device, known, mask, what):
        B, N, C = shape
        if known is None or mask is None:
            raise ValueError("%s needs known (B, N, C) and mask (B, N, C) or (B, N)" % what)
        if not isinstance(known, torch.Tensor) or tuple(known.shape) != (B, N, C):
            raise ValueError("known must be a (%d, %d, %d) tensor, got %s" % (B, N, C, tuple(getattr(known, "shape", ()))))
        return known.to(device=device, dtype=torch.float32).contiguous(), ops.known_mask(mask, (B, N, C), device)

    @torch.no_grad()
    def p_sample_loop_masked(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn, clip_denoised=True,
                             keep_running=False, known=None, mask=None, graph=None,
                             collision_scale=None, collision_steps=None, wall_scale=None, wall_steps=None, room_side=None, room_mask=None,
                             resample=None, resample_steps=None):
        """Element-wise in-painting in T steps.  ``known`` is (B, N, C) f32 in the network's encoding, ``mask`` (B, N, C) or (B, N) bool /
        uint8 (ops.known_mask), non-zero = this element is given.  Scene b is the reference's p_sample_loop_complete (:447-476) on that
        scene alone with its two torch.cat's replaced by a select: before the model call at step t,
        x = where(mask, q_sample(known, t, fresh noise), x); after the p_sample at t == 0, x = where(mask, known, x).  Draw order: x_T
        (B, N, C), then per step a known-draw noise_fn(size=(B, N, C)) -- full shape whatever the mask is -- followed by the p_sample draw
        (B, N, C): the draws of p_sample_loop_complete_ragged at Pmax == N, so a mask of whole rows [0, counts[b]) returns what that loop
        returns, bit for bit under the same seed.  An all-zero mask is plain generation on the main draws, an all-ones mask returns
        ``known``.  This eager loop is built from the unfused pieces -- masked overwrite, p_sample, select; the graph path (the default,
        by the rules of p_sample_loop) replays one captured step whose update is the fused dsc_p_sample_masked_f32, bit-identical."""
        return self._loop("p_sample_loop_masked", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          given=("mask", known, mask), clip_denoised=clip_denoised, keep_running=keep_running,
                          **_steer_kw(collision_scale, collision_steps), **_wall_kw(wall_scale, wall_steps, room_side, room_mask),
                          **_resample_kw(resample, resample_steps))

    @torch.no_grad()
    def ddim_masked_loop(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn, sampling_timesteps=50,
                         ddim_sampling_eta=0., known=None, mask=None, graph=None,
                         collision_scale=None, collision_steps=None,
                         wall_scale=None, wall_steps=None, room_side=None, room_mask=None, sampling_solver=None,
                         resample=None, resample_steps=None):
        """Element-wise in-painting in S strided (DDIM) steps; ``known`` / ``mask`` as in p_sample_loop_masked.  Scene b is ddim_sample_loop
        (reference :402-444) on that scene alone: before every model call at pair (t, t_next),
        x = where(mask, q_sample(known, t, fresh noise), x); after the last pair, x = where(mask, known, x).  x_start is always clamped
        to [-1, 1] (there is no ``clip_denoised``).  Draw order: that of ddim_complete_ragged_loop at Pmax == N -- x_T, then per pair a
        known-draw (B, N, C), the model call and a main draw (B, N, C), the last pair without the main draw: 2 S draws -- so a mask of
        whole rows [0, counts[b]) returns what that loop returns, bit for bit.  The eager loop is built from the unfused pieces; the
        graph path replays one captured step whose update is the fused dsc_ddim_masked_step_f32, bit-identical."""
        return self._loop("ddim_masked_loop", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          strided=(sampling_timesteps, ddim_sampling_eta), given=("mask", known, mask),
                          **_steer_kw(collision_scale, collision_steps),
                          **_wall_kw(wall_scale, wall_steps, room_side, room_mask), **_solver_kw(sampling_solver),
                          **_resample_kw(resample, resample_steps))

    @torch.no_grad()
    def p_sample_loop_masked_guided(self, denoise_fn, shape, device, condition, condition_cross, guidance_scale, noise_fn=torch.randn,
                                    clip_denoised=True, keep_running=False, known=None, mask=None, graph=None,
                                    collision_scale=None, collision_steps=None,
                                    wall_scale=None, wall_steps=None, room_side=None, room_mask=None,
                                    resample=None, resample_steps=None):
        """Text-guided element-wise in-painting in T steps: scene b is p_sample_loop_masked with m = u + w[b] * (c - u) in place of the
        model output (c, u and ``guidance_scale`` as in p_sample_loop_guided; ``known`` / ``mask`` as in p_sample_loop_masked).  Both
        halves of the 2 B model call see the same overwritten x_t.  Draws: exactly those of p_sample_loop_masked at batch B, in its
        order.  The eager loop is built from the unfused pieces -- masked overwrite, the denoiser at 2 B, cfg_combine, p_sample, select;
        the graph path (the default, by the rules of p_sample_loop) replays one captured step whose update is the fused
        dsc_p_sample_masked_cfg_f32, bit-identical."""
        return self._loop("p_sample_loop_masked_guided", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          given=("mask", known, mask), scale=guidance_scale, clip_denoised=clip_denoised, keep_running=keep_running,
                          **_steer_kw(collision_scale, collision_steps), **_wall_kw(wall_scale, wall_steps, room_side, room_mask),
                          **_resample_kw(resample, resample_steps))

    @torch.no_grad()
    def ddim_masked_guided_loop(self, denoise_fn, shape, device, condition, condition_cross, guidance_scale, noise_fn=torch.randn,
                                sampling_timesteps=50, ddim_sampling_eta=0., known=None, mask=None, graph=None,
                                collision_scale=None, collision_steps=None,
                                wall_scale=None, wall_steps=None, room_side=None, room_mask=None, sampling_solver=None,
                                resample=None, resample_steps=None):
        """Text-guided element-wise in-painting in S strided (DDIM) steps: scene b is ddim_masked_loop with the guided output m of
        p_sample_loop_masked_guided in place of the model output.  x_start is always clamped to [-1, 1].  Draws: exactly those of
        ddim_masked_loop at batch B (2 S in all).  The eager loop is built from the unfused pieces; the graph path replays one captured
        step whose update is the fused dsc_ddim_masked_cfg_step_f32, bit-identical."""
        return self._loop("ddim_masked_guided_loop", denoise_fn, shape, device, condition, condition_cross, noise_fn, graph,
                          strided=(sampling_timesteps, ddim_sampling_eta), given=("mask", known, mask), scale=guidance_scale,
                          **_steer_kw(collision_scale, collision_steps),
                          **_wall_kw(wall_scale, wall_steps, room_side, room_mask), **_solver_kw(sampling_solver),
                          **_resample_kw(resample, resample_steps))

    @torch.no_grad()
    def ddim_arrange_loop(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn, sampling_timesteps=50,
                          ddim_sampling_eta=0., input_boxes=None, graph=None, sampling_solver=None):
        """Strided (DDIM) re-arrangement: ddim_sample_loop on the sub-shape (B, N, translation_dim + angle_dim) under the arrange
        condition, then the re-assembly of p_sample_loop_arrange (reference :496-503).  Draws: those of ddim_sample_loop on the
        sub-shape (S in all).  ``sampling_solver``: as in ddim_sample_loop."""
        assert isinstance(shape, (tuple, list))
        _check_ddim(self.num_timesteps, sampling_timesteps, ddim_sampling_eta)
        if sampling_solver is not None:
            _check_solver(sampling_solver, (sampling_timesteps, ddim_sampling_eta), "ddim_arrange_loop")
        if input_boxes is None or tuple(input_boxes.shape) != tuple(shape):
            raise ValueError("ddim_arrange_loop needs input_boxes of shape %s" % (tuple(shape),))
        sub = (shape[0], shape[1], self.translation_dim + self.angle_dim)
        img = self.ddim_sample_loop(denoise_fn, sub, device, condition, condition_cross, noise_fn=noise_fn,
                                    sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta, graph=graph,
                                    **({} if sampling_solver is None else dict(sampling_solver=sampling_solver)))
        img = self._arranged(img, input_boxes)
        assert img.shape == tuple(shape)
        return img

    def _arranged(self, img, input_boxes):
        """The re-assembly of a re-arrangement, reference :496-503: the diffused [translation | angle] into the given rows."""
        tr, sz, bb = self.translation_dim, self.size_dim, self.bbox_dim
        return torch.cat([img[:, :, 0:tr], input_boxes[:, :, tr:tr + sz], img[:, :, tr:], input_boxes[:, :, bb:]], dim=-1).contiguous()

    def p_sample_loop_arrange(self, denoise_fn, shape, device, condition, condition_cross, noise_fn=torch.randn,
                              clip_denoised=True, keep_running=False, input_boxes=None, graph=None):
        """Re-arrangement, reference :478-506: diffuse [translation | angle] only, re-assemble at t == 0."""
        assert isinstance(shape, (tuple, list))
        sub = (shape[0], shape[1], self.translation_dim + self.angle_dim)
        img_t = self._loop("p_sample_loop_arrange", denoise_fn, sub, device, condition, condition_cross, noise_fn, graph,
                           clip_denoised=clip_denoised, keep_running=keep_running)
        self._say_last()
        img_t = self._arranged(img_t, input_boxes)
        assert img_t.shape == shape
        return img_t

    # ------------------------------------------------------------------ losses
    def p_losses(self, denoise_fn, data_start, t, noise=None, condition=None, condition_cross=None):
        """Training loss, reference :520-665 (loss_type 'mse')."""
        if len(data_start.shape) == 3:
            B, D, N = data_start.shape
        elif len(data_start.shape) == 4:
            B, D, M, N = data_start.shape
        assert t.shape == torch.Size([B])
        if noise is None:
            noise = torch.randn(data_start.shape, dtype=data_start.dtype, device=data_start.device)
        assert noise.shape == data_start.shape and noise.dtype == data_start.dtype
        if self.loss_type not in ('mse', 'kl'):
            raise NotImplementedError(self.loss_type)
        tb = self.tables(data_start.device)
        if self.loss_type == 'kl':
            # reference :657-660 -- a (B,) tensor only, no loss dict
            data_t = ops.q_sample(data_start.contiguous(), noise.contiguous(), t, tb["sqrt_alphas_cumprod"],
                                  tb["sqrt_one_minus_alphas_cumprod"])
            losses = self._vb_terms_bpd(denoise_fn=denoise_fn, data_start=data_start, data_t=data_t, t=t,
                                        condition=condition, condition_cross=condition_cross, clip_denoised=False,
                                        return_pred_xstart=False)
            assert losses.shape == torch.Size([B])
            return losses
        with torch.no_grad():
            data_t, v_target = ops.q_sample(data_start.contiguous(), noise.contiguous(), t, tb["sqrt_alphas_cumprod"],
                                            tb["sqrt_one_minus_alphas_cumprod"], want_v=True)
        if self.model_mean_type == 'eps':
            target = noise
        elif self.model_mean_type == 'x0':
            target = data_start
        elif self.model_mean_type == 'v':
            target = v_target
        else:
            raise NotImplementedError
        denoise_out = denoise_fn(data_t, t, condition, condition_cross)
        assert data_t.shape == data_start.shape
        assert denoise_out.shape == data_start.shape
        from ..train_loss import diffusion_losses
        return diffusion_losses(self, tb, data_start, data_t, target, denoise_out, t)

    def _vb_terms_bpd(self, denoise_fn, data_start, data_t, t, condition, condition_cross, clip_denoised: bool,
                      return_pred_xstart: bool):
        """KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t)) per scene in bits, reference :511-518."""
        true_mean, _, true_log_variance_clipped = self.q_posterior_mean_variance(x_start=data_start, x_t=data_t, t=t)
        model_mean, _, model_log_variance, pred_xstart = self.p_mean_variance(
            denoise_fn, data=data_t, t=t, condition=condition, condition_cross=condition_cross,
            clip_denoised=clip_denoised, return_pred_xstart=True)
        kl = normal_kl(true_mean, true_log_variance_clipped, model_mean, model_log_variance)
        kl = kl.mean(dim=list(range(1, len(data_start.shape)))) / np.log(2.)
        return (kl, pred_xstart) if return_pred_xstart else kl

    def descale_to_origin(self, x, minimum, maximum):
        x = (x + 1) / 2
        x = x * (maximum - minimum)[None, None, :] + minimum[None, None, :]
        return x

    # ------------------------------------------------------------------ diagnostics
    def _prior_bpd(self, x_start):
        """KL(q(x_T|x_0) || N(0,I)) per scene in bits, reference :679-688."""
        with torch.no_grad():
            B, T = x_start.shape[0], self.num_timesteps
            t_ = torch.empty(B, dtype=torch.int64, device=x_start.device).fill_(T - 1)
            qt_mean, _, qt_log_variance = self.q_mean_variance(x_start, t=t_)
            kl_prior = normal_kl(mean1=qt_mean, logvar1=qt_log_variance,
                                 mean2=torch.tensor([0.]).to(qt_mean), logvar2=torch.tensor([0.]).to(qt_log_variance))
            assert kl_prior.shape == x_start.shape
            return kl_prior.mean(dim=list(range(1, len(kl_prior.shape)))) / np.log(2.)

    def calc_bpd_loop(self, denoise_fn, x_start, condition, condition_cross, clip_denoised=True):
        """Variational bound over all T timesteps, reference :690-717.  Same draw order (one q_sample draw per
        timestep, T-1 first); the (B,T) tables are filled by column instead of the reference's mask arithmetic."""
        with torch.no_grad():
            B, T = x_start.shape[0], self.num_timesteps
            vals_bt_ = torch.zeros([B, T], device=x_start.device)
            mse_bt_ = torch.zeros([B, T], device=x_start.device)
            for t in reversed(range(T)):
                t_b = torch.empty(B, dtype=torch.int64, device=x_start.device).fill_(t)
                new_vals_b, pred_xstart = self._vb_terms_bpd(
                    denoise_fn, data_start=x_start, data_t=self.q_sample(x_start=x_start, t=t_b), t=t_b,
                    condition=condition, condition_cross=condition_cross, clip_denoised=clip_denoised,
                    return_pred_xstart=True)
                assert pred_xstart.shape == x_start.shape
                new_mse_b = ((pred_xstart - x_start) ** 2).mean(dim=list(range(1, len(x_start.shape))))
                assert new_vals_b.shape == new_mse_b.shape == torch.Size([B])
                vals_bt_[:, t] = new_vals_b
                mse_bt_[:, t] = new_mse_b
            prior_bpd_b = self._prior_bpd(x_start)
            total_bpd_b = vals_bt_.sum(dim=1) + prior_bpd_b
            assert vals_bt_.shape == mse_bt_.shape == torch.Size([B, T]) and \
                total_bpd_b.shape == prior_bpd_b.shape == torch.Size([B])
            return total_bpd_b.mean(), vals_bt_.mean(), prior_bpd_b.mean(), mse_bt_.mean()


def _check_ddim(num_timesteps, sampling_timesteps, ddim_sampling_eta):
    """(S, eta) of a DDIM call, or ValueError: 1 <= S <= T, 0 <= eta <= 1 (eta > 1 takes the root of a negative number, :431)."""
    S = sampling_timesteps
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= int(S) <= num_timesteps:
        raise ValueError("sampling_timesteps must be an integer in [1, %d], got %r" % (num_timesteps, S))
    eta = float(ddim_sampling_eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError("ddim_sampling_eta must lie in [0, 1], got %r" % (ddim_sampling_eta,))
    return int(S), eta


def front_end_name(strided, given, guided):
    """The captured loop of a spec (GaussianDiffusion._loop), by its name in sampler.py; the dense prefix rides on the plain T-step loop."""
    middle = {None: "", "dense": "", "ragged": "complete_ragged_", "mask": "masked_"}[given] + ("guided_" if guided else "")
    return "graph_%s%sloop" % ("ddim_" if strided else "", middle or "sample_")


def _use_graph(graph, noise_fn, denoise_fn=None):
    """Does this reverse loop run as the replayed hipGraph step (sampler.py)?  ``graph=True`` / ``False`` decide; None (what the
    reference's call sites pass) = yes by default since round 6 -- the captured loop is bit-identical to the eager one and not
    host-bound at small batches -- unless DSC_GRAPH=0, a custom ``noise_fn`` (its draws cannot be captured; a NoiseReplay and a
    SceneNoise can: the graph walks a buffer / counts the draws on the device) or a ``denoise_fn`` that is not DiffusionPoint._denoise
    over this package's Unet1D."""
    from ..sampler import NoiseReplay
    capturable = noise_fn is torch.randn or isinstance(noise_fn, (NoiseReplay, SceneNoise))
    if graph is None:
        if os.environ.get("DSC_GRAPH", "1") == "0" or not capturable:
            return False
        from .denoise_net import Unet1D
        return isinstance(getattr(getattr(denoise_fn, "__self__", None), "model", None), Unet1D)
    return bool(graph) and capturable


class DiffusionPoint(nn.Module):
    def __init__(self, denoise_net, config, schedule_type='linear', beta_start=0.0001, beta_end=0.02, time_num=1000,
                 loss_type='mse', model_mean_type='eps', model_var_type='fixedsmall', loss_separate=False,
                 loss_iou=False, train_stats_file=None):
        super(DiffusionPoint, self).__init__()
        betas = get_betas(schedule_type, beta_start, beta_end, time_num)
        self.diffusion = GaussianDiffusion(config, betas, loss_type, model_mean_type, model_var_type, loss_separate,
                                           loss_iou, train_stats_file)
        self.model = denoise_net

    def prior_kl(self, x0):
        return self.diffusion._prior_bpd(x0)

    def all_kl(self, x0, condition, condition_cross, clip_denoised=True):
        total_bpd_b, vals_bt, prior_bpd_b, mse_bt = self.diffusion.calc_bpd_loop(self._denoise, x0, condition,
                                                                                 condition_cross, clip_denoised)
        return {'total_bpd_b': total_bpd_b, 'terms_bpd': vals_bt, 'prior_bpd_b': prior_bpd_b, 'mse_bt': mse_bt}

    def _denoise(self, data, t, condition, condition_cross):
        B, D, N = data.shape
        assert data.dtype == torch.float
        assert t.shape == torch.Size([B]) and t.dtype == torch.int64
        out = self.model(data, t, condition, condition_cross)
        assert out.shape == torch.Size([B, D, N])
        return out

    def get_loss_iter(self, data, noises=None, condition=None, condition_cross=None):
        """reference :758-772: draws t (RNG draw #1), p_losses draws the noise (draw #2)."""
        if len(data.shape) == 3:
            B, D, N = data.shape
        elif len(data.shape) == 4:
            B, D, M, N = data.shape
        t = torch.randint(0, self.diffusion.num_timesteps, size=(B,), device=data.device)
        if noises is not None:
            noises[t != 0] = torch.randn((t != 0).sum(), *noises.shape[1:]).to(noises)
        losses, loss_dict = self.diffusion.p_losses(denoise_fn=self._denoise, data_start=data, t=t, noise=noises,
                                                    condition=condition, condition_cross=condition_cross)
        assert losses.shape == t.shape == torch.Size([B])
        return losses.mean(), loss_dict

    def gen_samples(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn,
                    clip_denoised=True, keep_running=False, graph=None, **steer):
        return self.diffusion.p_sample_loop(self._denoise, shape=shape, device=device, condition=condition,
                                            condition_cross=condition_cross, noise_fn=noise_fn,
                                            clip_denoised=clip_denoised, keep_running=keep_running, graph=graph, **steer)

    def gen_sample_traj(self, shape, device, freq, condition=None, condition_cross=None, noise_fn=torch.randn,
                        clip_denoised=True, keep_running=False):
        return self.diffusion.p_sample_loop_trajectory(self._denoise, shape=shape, device=device, condition=condition,
                                                       condition_cross=condition_cross, noise_fn=noise_fn, freq=freq,
                                                       clip_denoised=clip_denoised, keep_running=keep_running)

    def gen_samples_ddim(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn, clip_denoised=True,
                         sampling_timesteps=50, ddim_sampling_eta=0., return_all_timesteps=False, graph=None, **steer):
        return self.diffusion.ddim_sample_loop(self._denoise, shape=shape, device=device, condition=condition,
                                               condition_cross=condition_cross, noise_fn=noise_fn, clip_denoised=clip_denoised,
                                               sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta,
                                               return_all_timesteps=return_all_timesteps, graph=graph, **steer)

    def gen_samples_guided(self, shape, device, condition=None, condition_cross=None, guidance_scale=1.0, noise_fn=torch.randn,
                           clip_denoised=True, keep_running=False, graph=None, **steer):
        """gen_samples under classifier-free guidance (p_sample_loop_guided)."""
        return self.diffusion.p_sample_loop_guided(self._denoise, shape=shape, device=device, condition=condition,
                                                   condition_cross=condition_cross, guidance_scale=guidance_scale, noise_fn=noise_fn,
                                                   clip_denoised=clip_denoised, keep_running=keep_running, graph=graph, **steer)

    def gen_samples_guided_ddim(self, shape, device, condition=None, condition_cross=None, guidance_scale=1.0, noise_fn=torch.randn,
                                sampling_timesteps=50, ddim_sampling_eta=0., graph=None, **steer):
        """gen_samples_guided in S strided steps (ddim_guided_loop)."""
        return self.diffusion.ddim_guided_loop(self._denoise, shape=shape, device=device, condition=condition,
                                               condition_cross=condition_cross, guidance_scale=guidance_scale, noise_fn=noise_fn,
                                               sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta, graph=graph, **steer)

    def complete_samples(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn,
                         clip_denoised=True, keep_running=False, partial_boxes=None, graph=None, **steer):
        return self.diffusion.p_sample_loop_complete(self._denoise, shape=shape, device=device, condition=condition,
                                                     condition_cross=condition_cross, noise_fn=noise_fn,
                                                     clip_denoised=clip_denoised, keep_running=keep_running,
                                                     partial_boxes=partial_boxes, graph=graph, **steer)

    def complete_samples_ragged(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn,
                                clip_denoised=True, keep_running=False, partial_boxes=None, num_partial=None, graph=None, **steer):
        """complete_samples for a batch with per-scene numbers of given objects (p_sample_loop_complete_ragged)."""
        return self.diffusion.p_sample_loop_complete_ragged(self._denoise, shape=shape, device=device, condition=condition,
                                                            condition_cross=condition_cross, noise_fn=noise_fn,
                                                            clip_denoised=clip_denoised, keep_running=keep_running,
                                                            partial_boxes=partial_boxes, num_partial=num_partial, graph=graph, **steer)

    def complete_samples_ragged_ddim(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn,
                                     sampling_timesteps=50, ddim_sampling_eta=0., partial_boxes=None, num_partial=None, graph=None, **steer):
        """complete_samples_ragged in S strided steps (ddim_complete_ragged_loop)."""
        return self.diffusion.ddim_complete_ragged_loop(self._denoise, shape=shape, device=device, condition=condition,
                                                        condition_cross=condition_cross, noise_fn=noise_fn,
                                                        sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta,
                                                        partial_boxes=partial_boxes, num_partial=num_partial, graph=graph, **steer)

    def inpaint_samples(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn, clip_denoised=True,
                        keep_running=False, known=None, mask=None, graph=None, **steer):
        """Element-wise in-painting: the elements marked by ``mask`` are held at ``known`` (p_sample_loop_masked)."""
        return self.diffusion.p_sample_loop_masked(self._denoise, shape=shape, device=device, condition=condition,
                                                   condition_cross=condition_cross, noise_fn=noise_fn, clip_denoised=clip_denoised,
                                                   keep_running=keep_running, known=known, mask=mask, graph=graph, **steer)

    def inpaint_samples_ddim(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn, sampling_timesteps=50,
                             ddim_sampling_eta=0., known=None, mask=None, graph=None, **steer):
        """inpaint_samples in S strided steps (ddim_masked_loop)."""
        return self.diffusion.ddim_masked_loop(self._denoise, shape=shape, device=device, condition=condition,
                                               condition_cross=condition_cross, noise_fn=noise_fn,
                                               sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta,
                                               known=known, mask=mask, graph=graph, **steer)

    def inpaint_samples_guided(self, shape, device, condition=None, condition_cross=None, guidance_scale=1.0, noise_fn=torch.randn,
                               clip_denoised=True, keep_running=False, known=None, mask=None, graph=None, **steer):
        """inpaint_samples under classifier-free guidance (p_sample_loop_masked_guided)."""
        return self.diffusion.p_sample_loop_masked_guided(self._denoise, shape=shape, device=device, condition=condition,
                                                          condition_cross=condition_cross, guidance_scale=guidance_scale,
                                                          noise_fn=noise_fn, clip_denoised=clip_denoised, keep_running=keep_running,
                                                          known=known, mask=mask, graph=graph, **steer)

    def inpaint_samples_guided_ddim(self, shape, device, condition=None, condition_cross=None, guidance_scale=1.0, noise_fn=torch.randn,
                                    sampling_timesteps=50, ddim_sampling_eta=0., known=None, mask=None, graph=None, **steer):
        """inpaint_samples_guided in S strided steps (ddim_masked_guided_loop)."""
        return self.diffusion.ddim_masked_guided_loop(self._denoise, shape=shape, device=device, condition=condition,
                                                      condition_cross=condition_cross, guidance_scale=guidance_scale, noise_fn=noise_fn,
                                                      sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta,
                                                      known=known, mask=mask, graph=graph, **steer)

    def arrange_samples_ddim(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn,
                             sampling_timesteps=50, ddim_sampling_eta=0., input_boxes=None, graph=None, **solver):
        """arrange_samples in S strided steps (ddim_arrange_loop); ``solver``: sampling_solver=, where the caller passes one."""
        return self.diffusion.ddim_arrange_loop(self._denoise, shape=shape, device=device, condition=condition,
                                                condition_cross=condition_cross, noise_fn=noise_fn,
                                                sampling_timesteps=sampling_timesteps, ddim_sampling_eta=ddim_sampling_eta,
                                                input_boxes=input_boxes, graph=graph, **solver)

    def arrange_samples(self, shape, device, condition=None, condition_cross=None, noise_fn=torch.randn,
                        clip_denoised=True, keep_running=False, input_boxes=None, graph=None):
        return self.diffusion.p_sample_loop_arrange(self._denoise, shape=shape, device=device, condition=condition,
                                                    condition_cross=condition_cross, noise_fn=noise_fn,
                                                    clip_denoised=clip_denoised, keep_running=keep_running,
                                                    input_boxes=input_boxes, graph=graph)
