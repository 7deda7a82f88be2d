"""hipGraph-captured reverse diffusion loop (reference p_sample_loop, diffusion_ddpm.py:355-371).

The reference launches ~800 kernels per step from Python, 8e5 launches per sample.  Here ONE
reverse step -- the denoiser launch plan (~140 kernels), the noise draw and the fused posterior step -- is
captured once into a hipGraph whose only state is device-resident (x_t, the int64 timestep vector, the
conditioning buffers of the plan) and replayed T times; the timestep is decremented by a kernel inside the graph.
RNG draw order is the reference's: x_T first, then one draw per step (also at t == 0).
DDIM (ddim_sample_loop, :402-444) has its own captured step (_DDIMGraph): plan run, draw, fused DDIM step, advance kernel.
Batched completion with per-scene counts has another (_RaggedCompleteGraph): plan run, two draws, fused inpainting step, decrement.
Strided (DDIM) batched completion (_DDIMCompleteGraph, ddim_complete_ragged_loop) combines the two: one standalone partial draw and
ragged overwrite at times[0], then S - 1 replays of [plan run, main draw k, partial draw k + 1, fused dsc_ddim_inpaint_step_f32,
advance] and one replay of the draw-free final step.  Draw order (eager and captured): x_T, then per pair a partial draw (B, Pmax, C),
the model call and a main draw (B, N, C); the last pair makes the partial draw only -- 2 S draws.  Strided re-arrangement is
_DDIMGraph on the sub-shape.
Element-wise in-painting (_MaskedGraph, _DDIMMaskedGraph: p_sample_loop_masked / ddim_masked_loop) is the two completion graphs with
the row prefix replaced by a (B, N, C) byte mask and full-shape known-draws: the same draw shift, the fused dsc_p_sample_masked_f32 /
dsc_ddim_masked_step_f32, one graph per shape for every mask.
Classifier-free guidance (_GuidedStepGraph, _DDIMGuidedGraph: p_sample_loop_guided / ddim_guided_loop) is _StepGraph / _DDIMGraph on a plan
at 2 B (text features | zeros) with the fused dsc_p_sample_cfg_f32 / dsc_ddim_cfg_step_f32; the per-scene scales live in a device buffer.
"""
import torch

from . import ops
from .networks.denoise_net import Unet1D

_MEAN = {"eps": ops.MEAN_EPS, "x0": ops.MEAN_X0, "v": ops.MEAN_V}


class NoiseReplay:
    """noise_fn (protocol of diffusion_ddpm.py:345,355-356) that replays a pre-generated device tensor
    ``buffer[i]`` for the i-th draw.  Usable eagerly and inside the captured graph (parity tests inject the
    reference's noise this way)."""

    def __init__(self, buffer, partial_buffer=None):
        self.buffer = buffer                      # (T+1, B, N, C): x_T, then the p_sample draw of every step
        self.partial_buffer = partial_buffer      # (T, B, P, C): completion only, the draw that re-noises the given objects
        self.i = 0
        self.ip = 0

    def __call__(self, size=None, dtype=None, device=None):
        if self.partial_buffer is not None and tuple(size) == tuple(self.partial_buffer.shape[1:]) \
                and tuple(size) != tuple(self.buffer.shape[1:]):
            n = self.partial_buffer[self.ip]
            self.ip += 1
            return n
        n = self.buffer[self.i]
        self.i += 1
        assert tuple(n.shape) == tuple(size), (tuple(n.shape), tuple(size))
        return n


class RaggedNoiseReplay(NoiseReplay):
    """NoiseReplay for the ragged completion loop, which may be given Pmax == N rows -- the shape test of NoiseReplay cannot tell the
    two draws apart then.  This one goes by the loop's protocol: call 0 is x_T, then calls alternate partial draw, main draw."""

    def __init__(self, buffer, partial_buffer):
        super().__init__(buffer, partial_buffer)   # (T+1, B, N, C) and (T, B, Pmax, C); the DDIM loop: (S, B, N, C) and (S, B, Pmax, C)
        self.calls = 0

    def __call__(self, size=None, dtype=None, device=None):
        partial = self.calls % 2 == 1
        self.calls += 1
        if partial:
            n = self.partial_buffer[self.ip]
            self.ip += 1
        else:
            n = self.buffer[self.i]
            self.i += 1
        assert tuple(n.shape) == tuple(size), (tuple(n.shape), tuple(size))
        return n


def _chains_for(B):
    """Independent sub-batch chains per captured step (env DSC_CHAINS, default 1).  Scenes are independent, so the batch
    can run as several dependency chains on separate streams inside the graph.  Measured on MI355X (B=256, N=80,
    profiles/r02_chain_sweep_*.txt): with the round-1 GEMMs two 128-scene chains gained 3 % (12.07 vs 12.44 ms; starting the
    second chain 15-110 us late so that its K loops run under the first chain's epilogues lost on every offset); with the
    interleaved LDS-DMA GEMMs one chain is best (10.73 ms vs 10.97 ms for two, 12.1 ms for four) -- a single 256-scene chain
    already fills the CUs and leaves no launch gaps -- so it stays opt-in (useful when the per-GPU batch is far above 256)."""
    import os
    n = int(os.environ.get("DSC_CHAINS", "1"))
    return n if (n > 1 and B % n == 0 and B // n >= 64) else 1


class _StepGraph:
    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay=False,
                 partial_shape=None):
        B, N, C = shape
        self.shape = shape
        eng = model.engine(device)
        use_table = diff.num_timesteps <= eng.time_table.shape[0]
        nch = _chains_for(B)
        Bc = B // nch
        self.plans = [eng.prepare(Bc, N, None if condition is None else condition[i * Bc:(i + 1) * Bc],
                                  None if condition_cross is None else condition_cross[i * Bc:(i + 1) * Bc],
                                  time_table=use_table, slot=i) for i in range(nch)]
        self.plan = self.plans[0]
        self.side = [torch.cuda.Stream(device=device) for _ in range(nch - 1)]
        tb = diff.tables(device)
        ca, cb = diff._coeffs(tb)
        self.x = torch.empty(shape, device=device, dtype=torch.float32)
        self.t = torch.zeros((B,), device=device, dtype=torch.int64)
        mean_type = _MEAN[diff.model_mean_type]
        sigma = diff._sigma(tb)
        plan = self.plan
        self.replay = replay
        self.noise_buf = None                                   # (T+1, B, N, C) when replaying
        self.draw = torch.zeros((1,), device=device, dtype=torch.int64)
        # scene completion (p_sample_loop_complete, diffusion_ddpm.py:461-466): the given objects are re-noised and
        # written over the first P rows of x_t at every step, BEFORE the model call
        self.partial = torch.zeros(partial_shape, device=device) if partial_shape is not None else None
        self.pnoise_buf = None
        self.pdraw = torch.zeros((1,), device=device, dtype=torch.int64)

        xv = self.x.view(B * N, C)
        self.model_out = torch.empty(shape, device=device, dtype=torch.float32) if nch > 1 else None

        def run_chain(i):
            p = self.plans[i]
            p.x_in.copy_(xv[i * Bc * N:(i + 1) * Bc * N])
            p.t_in.copy_(self.t[i * Bc:(i + 1) * Bc])
            p.run()
            if nch > 1:
                self.model_out.view(B * N, C)[i * Bc * N:(i + 1) * Bc * N].copy_(p.out)

        def step():
            if self.partial is not None:
                if self.replay:
                    pn = self.pnoise_buf.index_select(0, self.pdraw)[0]
                    ops.add_scalar_i64(self.pdraw, 1)
                else:
                    pn = torch.randn(partial_shape, dtype=torch.float, device=device)
                ops.complete_overwrite(self.x, self.partial, pn, self.t, tb["sqrt_alphas_cumprod"],
                                       tb["sqrt_one_minus_alphas_cumprod"])
            cur = torch.cuda.current_stream(device)
            for st in self.side:
                st.wait_stream(cur)
            run_chain(0)
            for i, st in enumerate(self.side):
                with torch.cuda.stream(st):
                    run_chain(i + 1)
            for st in self.side:
                cur.wait_stream(st)
            if self.replay:
                noise = self.noise_buf.index_select(0, self.draw)[0]
                ops.add_scalar_i64(self.draw, 1)
            else:
                noise = torch.randn(shape, dtype=torch.float, device=device)
            ops.p_sample(self.x, self.model_out if nch > 1 else plan.out.view(B, N, C), noise, self.t, ca, cb,
                         tb["posterior_mean_coef1"],
                         tb["posterior_mean_coef2"], sigma, mean_type, clip_denoised, out=self.x)
            ops.add_scalar_i64(self.t, -1)

        # warm-up on a side stream (loads every code object, sizes the allocator), then capture.  Building the graph must not cost the
        # caller random numbers: the loop is the default path behind the reference's call sites (round 6), and a run seeded with
        # torch.manual_seed has to draw what the eager loop draws whether or not this call had to capture first -- the device
        # generator's state is put back afterwards (the warm-up step and normal_() below draw from it).
        rng_state = torch.cuda.get_rng_state(device)
        self.x.normal_()
        self.t.fill_(1)
        if replay:
            self.noise_buf = torch.zeros((diff.num_timesteps + 1,) + tuple(shape), device=device)
            if partial_shape is not None:
                self.pnoise_buf = torch.zeros((diff.num_timesteps,) + tuple(partial_shape), device=device)
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            step()
        torch.cuda.set_rng_state(rng_state, device)

    def check_current(self):
        """The captured launches hold raw pointers into the parameter storages of capture time.  If the parameters have moved since
        (the first training step re-homes them into flat storage, module.to() ...) the graph is stale: refuse to replay it.  (The
        plans keep the old storages alive, so a stale replay could not fault -- it would silently sample from old weights.)"""
        for p in self.plans:
            p.eng.params_moved()
            p.check_current()

    def replay_steps(self, n=1):
        """n captured reverse steps on the current stream (x, t and the conditioning buffers are the graph's own state)."""
        self.check_current()
        for _ in range(n):
            self.graph.replay()

    def run(self, x_T, total_steps, noise_buffer=None, partial=None, partial_noise=None):
        self.check_current()
        self.x.copy_(x_T)
        self.t.fill_(total_steps - 1)
        if self.partial is not None:
            self.partial.copy_(partial)
        if self.replay:
            self.noise_buf[:noise_buffer.shape[0]].copy_(noise_buffer)
            self.draw.fill_(1)                                  # draw 0 was x_T
            if self.partial is not None:
                self.pnoise_buf[:partial_noise.shape[0]].copy_(partial_noise)
                self.pdraw.fill_(0)
        for _ in range(total_steps):
            self.graph.replay()
        out = self.x.clone()
        # the in-graph timestep now holds -1: park it on a valid row, so that one replay too many (a caller driving `graph` directly)
        # still indexes the schedule tables in range (the kernels clamp and count it either way: dsc_device_error_count)
        self.t.fill_(0)
        return out


def graph_sample_loop(diff, denoise_fn, shape, device, condition, condition_cross, clip_denoised, total_steps,
                      noise_fn=torch.randn, partial_boxes=None):
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        pshape = None if partial_boxes is None else tuple(partial_boxes.shape)
        key = (id(model), tuple(shape), str(device), bool(clip_denoised), diff.model_mean_type, replay, pshape,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0),
               None if condition_cross is None else tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()              # parameters re-homed since the capture (first training step, .to()): the engine drops its plans
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = _StepGraph(diff, model, tuple(shape), device, condition, condition_cross, clip_denoised, replay, pshape)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:
            nch = len(g.plans)
            Bc = shape[0] // nch
            for i in range(nch):                                     # refresh weights + conditioning buffers
                eng.prepare(Bc, shape[1], None if condition is None else condition[i * Bc:(i + 1) * Bc],
                            None if condition_cross is None else condition_cross[i * Bc:(i + 1) * Bc],
                            time_table=g.plan.time_table, slot=i)
        if replay:
            out = g.run(noise_fn.buffer[0], total_steps, noise_fn.buffer, partial_boxes, noise_fn.partial_buffer)
        else:
            x_T = torch.randn(shape, dtype=torch.float, device=device)
            out = g.run(x_T, total_steps, partial=partial_boxes)
        if partial_boxes is not None:
            out[:, :partial_boxes.shape[1], :] = partial_boxes          # clean objects restored after the last step (:471-473)
        from ._lib import check_indices
        check_indices("graph_sample_loop")     # DSC_CHECK_INDICES=1 (debugging; synchronises)
        return out


class _DDIMGraph:
    """The captured DDIM loop (reference ddim_sample_loop, diffusion_ddpm.py:402-444).  ``graph``: plan run, noise draw, the fused
    step (dsc_ddim_step_f32) and the advance kernel (step += 1, t = times[step]), replayed S - 1 times; ``final``: plan run and the
    draw-free last step ((t, -1) -> x_start), replayed once.  The step counter and the per-step tables (t, t_next, sqrt(alpha_next), c,
    sigma) are captured by pointer: this object owns them and ``run`` refreshes them IN PLACE (eta is not part of the cache key), so
    a live graph never points at a freed table."""

    check_current = _StepGraph.check_current

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay=False):
        B, N, C = shape
        self.shape, self.S = shape, S
        eng = model.engine(device)
        use_table = diff.num_timesteps <= eng.time_table.shape[0]
        self.plans = [eng.prepare(B, N, condition, condition_cross, time_table=use_table)]
        self.plan = plan = self.plans[0]
        tb = diff.tables(device)
        ca, cb = diff._coeffs(tb)
        ra, rm = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
        mean_type = _MEAN[diff.model_mean_type]
        self.x = torch.empty(shape, device=device, dtype=torch.float32)
        self.t = torch.zeros((B,), device=device, dtype=torch.int64)
        self.step = torch.zeros((1,), device=device, dtype=torch.int64)
        self.times = torch.zeros((S,), device=device, dtype=torch.int64)
        self.times_next = torch.zeros((S,), device=device, dtype=torch.int64)
        self.coef = torch.zeros((3, S), device=device, dtype=torch.float32)
        self.replay = replay
        self.draw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.noise_buf = torch.zeros((S,) + tuple(shape), device=device) if replay else None    # x_T, then S - 1 step draws
        xv = self.x.view(B * N, C)

        def step(final):
            plan.x_in.copy_(xv)
            plan.t_in.copy_(self.t)
            plan.run()
            if final:
                noise = self.x                                   # not read on the last pair
            elif self.replay:
                noise = self.noise_buf.index_select(0, self.draw)[0]
                ops.add_scalar_i64(self.draw, 1)
            else:
                noise = torch.randn(shape, dtype=torch.float, device=device)
            ops.ddim_step(self.x, plan.out.view(B, N, C), noise, self.step, self.times, self.times_next, self.coef, ca, cb,
                          ra, rm, mean_type, out=self.x)
            if not final:
                ops.ddim_advance(self.step, self.times, self.t)

        # warm-up on a side stream, then capture; the caller's device RNG state is put back (see _StepGraph).  With all-zero tables
        # every index of the warm-up is in range (the advance moves the counter to 1 < S only when there is a non-final step).
        rng_state = torch.cuda.get_rng_state(device)
        self.x.normal_()
        kinds = ([False] if S > 1 else []) + [True]
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for final in kinds:
                step(final)
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = None
        if S > 1:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                step(False)
        self.final = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.final, pool=self.graph.pool() if self.graph is not None else None):
            step(True)
        torch.cuda.set_rng_state(rng_state, device)

    def run(self, x_T, dtab, noise_buffer=None):
        pairs, times, times_next, coef = dtab
        assert len(pairs) == self.S
        self.check_current()
        self.times.copy_(times)                 # in place: the graphs hold these pointers
        self.times_next.copy_(times_next)
        self.coef.copy_(coef)
        self.x.copy_(x_T)
        self.step.zero_()
        self.t.fill_(pairs[0][0])
        if self.replay:
            self.noise_buf.copy_(noise_buffer[:self.S])
            self.draw.fill_(1)                                  # draw 0 was x_T
        for _ in range(self.S - 1):
            self.graph.replay()
        self.final.replay()
        return self.x.clone()


def graph_ddim_sample_loop(diff, denoise_fn, shape, device, condition, condition_cross, sampling_timesteps, eta,
                           noise_fn=torch.randn):
    """ddim_sample_loop as replayed hipGraphs; bit-identical to the eager loop (same kernels, same draws in the same order)."""
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    S = int(sampling_timesteps)
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        if replay and noise_fn.buffer.shape[0] < S:
            raise ValueError("NoiseReplay holds %d draws, DDIM with S = %d makes %d" % (noise_fn.buffer.shape[0], S, S))
        dtab = diff.ddim_tables(S, eta, device)
        key = (("ddim", S), id(model), tuple(shape), str(device), diff.model_mean_type, replay,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0),
               None if condition_cross is None else tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = _DDIMGraph(diff, model, tuple(shape), device, condition, condition_cross, S, replay)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:
            eng.prepare(shape[0], shape[1], condition, condition_cross, time_table=g.plan.time_table)
        if replay:
            out = g.run(noise_fn.buffer[0], dtab, noise_fn.buffer)
        else:
            x_T = torch.randn(shape, dtype=torch.float, device=device)
            out = g.run(x_T, dtab)
        from ._lib import check_indices
        check_indices("graph_ddim_sample_loop")
        return out


class _RaggedCompleteGraph:
    """The captured ragged completion loop (p_sample_loop_complete_ragged).  ``graph``: plan run, the main draw, the partial draw of
    the NEXT step, the fused update (dsc_p_sample_inpaint_f32: posterior step on the free rows, re-noised given objects on the
    others) and the timestep decrement, replayed total_steps - 1 times; ``final``: plan run, the main draw and the fused update at
    t == 0 (given rows restored, no partial draw -- so the loop draws exactly what the eager one draws, in its order).  The first
    overwrite, at t = total_steps - 1, is one standalone launch in ``run``.  The per-scene counts and the padded given objects live in
    buffers of this object, captured by pointer and refreshed in place: one graph serves every mix of counts.
    ``fused=False`` captures the same step from the unfused kernels (partial draw, ragged overwrite, plan run, main draw, p_sample,
    decrement; restore after the loop) -- the comparison of tools/bench_complete.py."""

    check_current = _StepGraph.check_current

    def __init__(self, diff, model, shape, pmax, device, condition, condition_cross, clip_denoised, replay=False, fused=True):
        B, N, C = shape
        self.shape, self.pmax, self.fused = shape, pmax, fused
        eng = model.engine(device)
        use_table = diff.num_timesteps <= eng.time_table.shape[0]
        self.plans = [eng.prepare(B, N, condition, condition_cross, time_table=use_table)]
        self.plan = plan = self.plans[0]
        self.tb = tb = diff.tables(device)
        ca, cb = diff._coeffs(tb)
        sigma = diff._sigma(tb)
        mean_type = _MEAN[diff.model_mean_type]
        sa, sb = tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
        k1, k2 = tb["posterior_mean_coef1"], tb["posterior_mean_coef2"]
        pshape = (B, pmax, C)
        self.x = torch.empty(shape, device=device, dtype=torch.float32)
        self.t = torch.zeros((B,), device=device, dtype=torch.int64)
        self.partial = torch.zeros(pshape, device=device, dtype=torch.float32)
        self.counts = torch.zeros((B,), device=device, dtype=torch.int64)
        self.replay = replay
        self.draw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.pdraw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.noise_buf = torch.zeros((diff.num_timesteps + 1,) + tuple(shape), device=device) if replay else None
        self.pnoise_buf = torch.zeros((diff.num_timesteps,) + pshape, device=device) if replay else None
        xv = self.x.view(B * N, C)

        def draw_main():
            if not self.replay:
                return torch.randn(shape, dtype=torch.float, device=device)
            n = self.noise_buf.index_select(0, self.draw)[0]
            ops.add_scalar_i64(self.draw, 1)
            return n

        def draw_partial():
            if not self.replay:
                return torch.randn(pshape, dtype=torch.float, device=device)
            n = self.pnoise_buf.index_select(0, self.pdraw)[0]
            ops.add_scalar_i64(self.pdraw, 1)
            return n

        def model_call():
            plan.x_in.copy_(xv)
            plan.t_in.copy_(self.t)
            plan.run()
            return plan.out.view(B, N, C)

        def step(final):
            if not fused:
                ops.complete_overwrite_ragged(self.x, self.partial, draw_partial(), self.counts, self.t, sa, sb)
                mo = model_call()
                ops.p_sample(self.x, mo, draw_main(), self.t, ca, cb, k1, k2, sigma, mean_type, clip_denoised, out=self.x)
                ops.add_scalar_i64(self.t, -1)
                return
            mo = model_call()
            noise = draw_main()
            pn = self.partial if final else draw_partial()          # not read at t == 0
            ops.p_sample_inpaint(self.x, mo, noise, self.partial, pn, self.counts, self.t, ca, cb, k1, k2, sigma, sa, sb, mean_type,
                                 clip_denoised, out=self.x)
            if not final:
                ops.add_scalar_i64(self.t, -1)

        # warm-up on a side stream, then capture; the caller's device RNG state is put back (see _StepGraph).  Counts are all zero
        # and t goes 1 -> 0: every index of the warm-up is in range.
        rng_state = torch.cuda.get_rng_state(device)
        self.x.normal_()
        self.t.fill_(1)
        kinds = [False, True] if fused else [False]
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for final in kinds:
                step(final)
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            step(False)
        self.final = None
        if fused:
            self.final = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.final, pool=self.graph.pool()):
                step(True)
        torch.cuda.set_rng_state(rng_state, device)
        self.t.fill_(0)

    def run(self, x_T, total_steps, partial, counts, noise_buffer=None, partial_noise=None):
        self.check_current()
        B, N, C = self.shape
        self.x.copy_(x_T)
        self.t.fill_(total_steps - 1)
        self.partial.copy_(partial)             # in place: the graphs hold these pointers
        self.counts.copy_(counts)
        if self.replay:
            self.noise_buf[:noise_buffer.shape[0]].copy_(noise_buffer)
            self.pnoise_buf[:partial_noise.shape[0]].copy_(partial_noise)
            self.draw.fill_(1)                                  # draw 0 was x_T
            self.pdraw.fill_(1 if self.fused else 0)            # fused: partial draw 0 feeds the standalone overwrite below
        if not self.fused:
            for _ in range(total_steps):
                self.graph.replay()
            out = self.x.clone()
            given = torch.arange(self.pmax, device=out.device)[None, :, None] < self.counts[:, None, None]
            out[:, :self.pmax, :] = torch.where(given, self.partial, out[:, :self.pmax, :])
        else:
            pn = self.pnoise_buf[0] if self.replay else torch.randn((B, self.pmax, C), dtype=torch.float, device=self.x.device)
            ops.complete_overwrite_ragged(self.x, self.partial, pn, self.counts, self.t, self.tb["sqrt_alphas_cumprod"],
                                          self.tb["sqrt_one_minus_alphas_cumprod"])
            for _ in range(total_steps - 1):
                self.graph.replay()
            self.final.replay()
            out = self.x.clone()
        self.t.fill_(0)                         # a valid row for a replay too many (see _StepGraph.run)
        return out


def graph_complete_ragged_loop(diff, denoise_fn, shape, device, condition, condition_cross, clip_denoised, total_steps,
                               noise_fn=torch.randn, partial_boxes=None, counts=None, fused=True):
    """p_sample_loop_complete_ragged as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same
    order, the same generator state afterwards).  ``counts`` is the (B,) int64 device tensor of ops.ragged_counts.  The cache key
    holds Pmax but not the counts."""
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    B, N, C = shape
    pmax = partial_boxes.shape[1]
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        if replay and (noise_fn.partial_buffer is None or noise_fn.buffer.shape[0] < total_steps + 1
                       or noise_fn.partial_buffer.shape[0] < total_steps
                       or tuple(noise_fn.partial_buffer.shape[1:]) != (B, pmax, C)):
            raise ValueError("ragged completion replays %d main draws (B, N, C) and %d partial draws (B, Pmax, C)"
                             % (total_steps + 1, total_steps))
        key = (("ragged", bool(fused)), id(model), tuple(shape), pmax, str(device), bool(clip_denoised), diff.model_mean_type, replay,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0),
               None if condition_cross is None else tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = _RaggedCompleteGraph(diff, model, tuple(shape), pmax, device, condition, condition_cross, clip_denoised, replay, fused)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:
            eng.prepare(B, N, condition, condition_cross, time_table=g.plan.time_table)
        if replay:
            out = g.run(noise_fn.buffer[0], total_steps, partial_boxes, counts, noise_fn.buffer[:total_steps + 1],
                        noise_fn.partial_buffer[:total_steps])
        else:
            x_T = torch.randn(shape, dtype=torch.float, device=device)
            out = g.run(x_T, total_steps, partial_boxes, counts)
        from ._lib import check_indices
        check_indices("graph_complete_ragged_loop")
        return out


class _DDIMCompleteGraph:
    """The captured strided completion loop (ddim_complete_ragged_loop): the draw shift of _RaggedCompleteGraph applied to _DDIMGraph.
    ``graph`` (only when S > 1): plan run, main draw k, the partial draw of pair k + 1, the fused update (dsc_ddim_inpaint_step_f32:
    DDIM step on the free rows, the given objects re-noised at t_next on the others) and the advance kernel, replayed S - 1 times;
    ``final``: plan run and the draw-free fused step of the last pair (x_start on the free rows, the given rows restored), replayed
    once from ``graph``'s pool.  The first overwrite, at times[0], is one standalone draw and launch in ``run`` -- so the loop draws what
    the eager one draws, in its order.  The tables, the step counter, the padded given objects and the counts live in buffers of this
    object, captured by pointer and refreshed in place: one graph serves every eta and every mix of counts.
    ``fused=False`` captures the same step from the unfused kernels (partial draw, ragged overwrite, plan run, main draw, ddim_step,
    advance; restore after the loop) -- the comparison of tools/bench_ddim_complete.py."""

    check_current = _StepGraph.check_current

    def __init__(self, diff, model, shape, pmax, device, condition, condition_cross, S, replay=False, fused=True):
        B, N, C = shape
        self.shape, self.pmax, self.S, self.fused = shape, pmax, S, fused
        eng = model.engine(device)
        use_table = diff.num_timesteps <= eng.time_table.shape[0]
        self.plans = [eng.prepare(B, N, condition, condition_cross, time_table=use_table)]
        self.plan = plan = self.plans[0]
        self.tb = tb = diff.tables(device)
        ca, cb = diff._coeffs(tb)
        ra, rm = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
        sa, sb = tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
        mean_type = _MEAN[diff.model_mean_type]
        pshape = (B, pmax, C)
        self.x = torch.empty(shape, device=device, dtype=torch.float32)
        self.t = torch.zeros((B,), device=device, dtype=torch.int64)
        self.step = torch.zeros((1,), device=device, dtype=torch.int64)
        self.times = torch.zeros((S,), device=device, dtype=torch.int64)
        self.times_next = torch.zeros((S,), device=device, dtype=torch.int64)
        self.coef = torch.zeros((3, S), device=device, dtype=torch.float32)
        self.partial = torch.zeros(pshape, device=device, dtype=torch.float32)
        self.counts = torch.zeros((B,), device=device, dtype=torch.int64)
        self.replay = replay
        self.draw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.pdraw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.noise_buf = torch.zeros((S,) + tuple(shape), device=device) if replay else None     # x_T, then S - 1 main draws
        self.pnoise_buf = torch.zeros((S,) + pshape, device=device) if replay else None           # one partial draw per pair
        xv = self.x.view(B * N, C)

        def draw_main():
            if not self.replay:
                return torch.randn(shape, dtype=torch.float, device=device)
            n = self.noise_buf.index_select(0, self.draw)[0]
            ops.add_scalar_i64(self.draw, 1)
            return n

        def draw_partial():
            if not self.replay:
                return torch.randn(pshape, dtype=torch.float, device=device)
            n = self.pnoise_buf.index_select(0, self.pdraw)[0]
            ops.add_scalar_i64(self.pdraw, 1)
            return n

        def model_call():
            plan.x_in.copy_(xv)
            plan.t_in.copy_(self.t)
            plan.run()
            return plan.out.view(B, N, C)

        def step(final):
            if not fused:
                ops.complete_overwrite_ragged(self.x, self.partial, draw_partial(), self.counts, self.t, sa, sb)
                mo = model_call()
                noise = self.x if final else draw_main()             # not read on the last pair
                ops.ddim_step(self.x, mo, noise, self.step, self.times, self.times_next, self.coef, ca, cb, ra, rm, mean_type,
                              out=self.x)
            else:
                mo = model_call()
                noise = self.x if final else draw_main()             # neither is read on the last pair
                pn = self.partial if final else draw_partial()
                ops.ddim_inpaint_step(self.x, mo, noise, self.partial, pn, self.counts, self.step, self.times, self.times_next,
                                      self.coef, ca, cb, ra, rm, sa, sb, mean_type, out=self.x)
            if not final:
                ops.ddim_advance(self.step, self.times, self.t)

        # warm-up on a side stream, then capture; the caller's device RNG state is put back (see _StepGraph).  Tables, counts and the
        # step counter are all zero: every index of the warm-up is in range (the advance moves the counter to 1 < S only when there is
        # a non-final step; times_next[.] = 0 reads row 0 of the schedule).
        rng_state = torch.cuda.get_rng_state(device)
        self.x.normal_()
        kinds = ([False] if S > 1 else []) + [True]
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for final in kinds:
                step(final)
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = None
        if S > 1:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                step(False)
        self.final = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.final, pool=self.graph.pool() if self.graph is not None else None):
            step(True)
        torch.cuda.set_rng_state(rng_state, device)
        self.step.zero_()

    def run(self, x_T, dtab, partial, counts, noise_buffer=None, partial_noise=None):
        pairs, times, times_next, coef = dtab
        assert len(pairs) == self.S
        self.check_current()
        B, N, C = self.shape
        self.times.copy_(times)                 # in place: the graphs hold these pointers
        self.times_next.copy_(times_next)
        self.coef.copy_(coef)
        self.x.copy_(x_T)
        self.step.zero_()
        self.t.fill_(pairs[0][0])
        self.partial.copy_(partial)
        self.counts.copy_(counts)
        if self.replay:
            self.noise_buf.copy_(noise_buffer[:self.S])
            self.pnoise_buf.copy_(partial_noise[:self.S])
            self.draw.fill_(1)                                  # draw 0 was x_T
            self.pdraw.fill_(1 if self.fused else 0)            # fused: partial draw 0 feeds the standalone overwrite below
        if self.fused:
            pn = self.pnoise_buf[0] if self.replay else torch.randn((B, self.pmax, C), dtype=torch.float, device=self.x.device)
            ops.complete_overwrite_ragged(self.x, self.partial, pn, self.counts, self.t, self.tb["sqrt_alphas_cumprod"],
                                          self.tb["sqrt_one_minus_alphas_cumprod"])
        for _ in range(self.S - 1):
            self.graph.replay()
        self.final.replay()
        out = self.x.clone()
        if not self.fused:
            given = torch.arange(self.pmax, device=out.device)[None, :, None] < self.counts[:, None, None]
            out[:, :self.pmax, :] = torch.where(given, self.partial, out[:, :self.pmax, :])
        return out


def graph_ddim_complete_ragged_loop(diff, denoise_fn, shape, device, condition, condition_cross, sampling_timesteps, eta,
                                    noise_fn=torch.randn, partial_boxes=None, counts=None, fused=True):
    """ddim_complete_ragged_loop as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same order,
    the same generator state afterwards).  ``counts`` is the (B,) int64 device tensor of ops.ragged_counts.  The cache key holds S and
    Pmax; it holds neither eta nor the counts."""
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    B, N, C = shape
    S = int(sampling_timesteps)
    pmax = partial_boxes.shape[1]
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        if replay and (noise_fn.partial_buffer is None or noise_fn.buffer.shape[0] < S or noise_fn.partial_buffer.shape[0] < S
                       or tuple(noise_fn.partial_buffer.shape[1:]) != (B, pmax, C)):
            raise ValueError("strided ragged completion replays %d main draws (B, N, C) and %d partial draws (B, Pmax, C)" % (S, S))
        dtab = diff.ddim_tables(S, eta, device)
        key = (("ddim_ragged", S, bool(fused)), id(model), tuple(shape), pmax, str(device), diff.model_mean_type, replay,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0),
               None if condition_cross is None else tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = _DDIMCompleteGraph(diff, model, tuple(shape), pmax, device, condition, condition_cross, S, replay, fused)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:
            eng.prepare(B, N, condition, condition_cross, time_table=g.plan.time_table)
        if replay:
            out = g.run(noise_fn.buffer[0], dtab, partial_boxes, counts, noise_fn.buffer, noise_fn.partial_buffer)
        else:
            x_T = torch.randn(shape, dtype=torch.float, device=device)
            out = g.run(x_T, dtab, partial_boxes, counts)
        from ._lib import check_indices
        check_indices("graph_ddim_complete_ragged_loop")
        return out


class _MaskedGraph:
    """The captured masked (element-wise in-painting) loop (p_sample_loop_masked): _RaggedCompleteGraph with the fused masked step.
    ``graph``: plan run, the main draw of t, the known-draw of t - 1, the fused update (dsc_p_sample_masked_f32: posterior step on the
    free elements, the given ones re-noised for the next model call) and the timestep decrement, replayed total_steps - 1 times;
    ``final``: plan run, the main draw and the fused update at t == 0 (given elements set to ``known``, no known-draw) -- so the loop
    draws exactly what the eager one draws, in its order.  The first overwrite, at t = total_steps - 1, is one standalone draw and
    launch in ``run``.  ``known`` (B, N, C) f32 and ``mask`` (B, N, C) uint8 live in buffers of this object, captured by pointer and
    refreshed in place: one graph serves every mask."""

    check_current = _StepGraph.check_current

    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay=False):
        B, N, C = shape
        self.shape = shape
        eng = model.engine(device)
        use_table = diff.num_timesteps <= eng.time_table.shape[0]
        self.plans = [eng.prepare(B, N, condition, condition_cross, time_table=use_table)]
        self.plan = plan = self.plans[0]
        self.tb = tb = diff.tables(device)
        ca, cb = diff._coeffs(tb)
        sigma = diff._sigma(tb)
        mean_type = _MEAN[diff.model_mean_type]
        sa, sb = tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
        k1, k2 = tb["posterior_mean_coef1"], tb["posterior_mean_coef2"]
        self.x = torch.empty(shape, device=device, dtype=torch.float32)
        self.t = torch.zeros((B,), device=device, dtype=torch.int64)
        self.known = torch.zeros(shape, device=device, dtype=torch.float32)
        self.mask = torch.zeros(shape, device=device, dtype=torch.uint8)
        self.replay = replay
        self.draw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.kdraw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.noise_buf = torch.zeros((diff.num_timesteps + 1,) + tuple(shape), device=device) if replay else None
        self.knoise_buf = torch.zeros((diff.num_timesteps,) + tuple(shape), device=device) if replay else None
        xv = self.x.view(B * N, C)

        def draw(buf, counter):
            if not self.replay:
                return torch.randn(shape, dtype=torch.float, device=device)
            n = buf.index_select(0, counter)[0]
            ops.add_scalar_i64(counter, 1)
            return n

        def step(final):
            plan.x_in.copy_(xv)
            plan.t_in.copy_(self.t)
            plan.run()
            noise = draw(self.noise_buf, self.draw)
            nk = self.known if final else draw(self.knoise_buf, self.kdraw)          # not read at t == 0
            ops.p_sample_masked(self.x, plan.out.view(B, N, C), noise, self.known, nk, self.mask, self.t, ca, cb, k1, k2, sigma, sa, sb,
                                mean_type, clip_denoised, out=self.x)
            if not final:
                ops.add_scalar_i64(self.t, -1)

        # warm-up on a side stream, then capture; the caller's device RNG state is put back (see _StepGraph).  The mask is all zero
        # and t goes 1 -> 0: every index of the warm-up is in range.
        rng_state = torch.cuda.get_rng_state(device)
        self.x.normal_()
        self.t.fill_(1)
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for final in (False, True):
                step(final)
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            step(False)
        self.final = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.final, pool=self.graph.pool()):
            step(True)
        torch.cuda.set_rng_state(rng_state, device)
        self.t.fill_(0)

    def run(self, x_T, total_steps, known, mask, noise_buffer=None, known_noise=None):
        self.check_current()
        self.x.copy_(x_T)
        self.t.fill_(total_steps - 1)
        self.known.copy_(known)                 # in place: the graphs hold these pointers
        self.mask.copy_(mask)
        if self.replay:
            self.noise_buf[:noise_buffer.shape[0]].copy_(noise_buffer)
            self.knoise_buf[:known_noise.shape[0]].copy_(known_noise)
            self.draw.fill_(1)                                  # draw 0 was x_T
            self.kdraw.fill_(1)                                 # known-draw 0 feeds the standalone overwrite below
        nk = self.knoise_buf[0] if self.replay else torch.randn(self.shape, dtype=torch.float, device=self.x.device)
        ops.masked_overwrite(self.x, self.known, nk, self.mask, self.t, self.tb["sqrt_alphas_cumprod"],
                             self.tb["sqrt_one_minus_alphas_cumprod"])
        for _ in range(total_steps - 1):
            self.graph.replay()
        self.final.replay()
        out = self.x.clone()
        self.t.fill_(0)                         # a valid row for a replay too many (see _StepGraph.run)
        return out


def _masked_replay_check(noise_fn, shape, n_main, n_known, what):
    if noise_fn.partial_buffer is None or noise_fn.buffer.shape[0] < n_main or noise_fn.partial_buffer.shape[0] < n_known \
            or tuple(noise_fn.partial_buffer.shape[1:]) != tuple(shape) or tuple(noise_fn.buffer.shape[1:]) != tuple(shape):
        raise ValueError("%s replays %d main draws and %d known-draws, all of shape %s" % (what, n_main, n_known, tuple(shape)))


def graph_masked_loop(diff, denoise_fn, shape, device, condition, condition_cross, clip_denoised, total_steps, noise_fn=torch.randn,
                      known=None, mask=None):
    """p_sample_loop_masked as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same order, the
    same generator state afterwards).  ``known`` (B, N, C) f32 and ``mask`` (B, N, C) uint8 (ops.known_mask) are copied into the graph's
    own buffers: the cache key holds the shape, not the mask."""
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    B, N, C = shape
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        if replay:
            _masked_replay_check(noise_fn, shape, total_steps + 1, total_steps, "the masked loop")
        key = ("masked", id(model), tuple(shape), str(device), bool(clip_denoised), diff.model_mean_type, replay,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0),
               None if condition_cross is None else tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = _MaskedGraph(diff, model, tuple(shape), device, condition, condition_cross, clip_denoised, replay)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:
            eng.prepare(B, N, condition, condition_cross, time_table=g.plan.time_table)
        if replay:
            out = g.run(noise_fn.buffer[0], total_steps, known, mask, noise_fn.buffer[:total_steps + 1],
                        noise_fn.partial_buffer[:total_steps])
        else:
            x_T = torch.randn(shape, dtype=torch.float, device=device)
            out = g.run(x_T, total_steps, known, mask)
        from ._lib import check_indices
        check_indices("graph_masked_loop")
        return out


class _DDIMMaskedGraph:
    """The captured strided masked loop (ddim_masked_loop): _DDIMCompleteGraph with the fused masked step.  ``graph`` (only when
    S > 1): plan run, main draw k, the known-draw of pair k + 1, the fused update (dsc_ddim_masked_step_f32) and the advance kernel,
    replayed S - 1 times; ``final``: plan run and the draw-free fused step of the last pair (x_start on the free elements, ``known`` on
    the given ones), replayed once from ``graph``'s pool.  The first overwrite, at times[0], is one standalone draw and launch in
    ``run``.  The tables, the step counter, ``known`` and ``mask`` live in buffers of this object, captured by pointer and refreshed in
    place: one graph serves every eta and every mask."""

    check_current = _StepGraph.check_current

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay=False):
        B, N, C = shape
        self.shape, self.S = shape, S
        eng = model.engine(device)
        use_table = diff.num_timesteps <= eng.time_table.shape[0]
        self.plans = [eng.prepare(B, N, condition, condition_cross, time_table=use_table)]
        self.plan = plan = self.plans[0]
        self.tb = tb = diff.tables(device)
        ca, cb = diff._coeffs(tb)
        ra, rm = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
        sa, sb = tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]
        mean_type = _MEAN[diff.model_mean_type]
        self.x = torch.empty(shape, device=device, dtype=torch.float32)
        self.t = torch.zeros((B,), device=device, dtype=torch.int64)
        self.step = torch.zeros((1,), device=device, dtype=torch.int64)
        self.times = torch.zeros((S,), device=device, dtype=torch.int64)
        self.times_next = torch.zeros((S,), device=device, dtype=torch.int64)
        self.coef = torch.zeros((3, S), device=device, dtype=torch.float32)
        self.known = torch.zeros(shape, device=device, dtype=torch.float32)
        self.mask = torch.zeros(shape, device=device, dtype=torch.uint8)
        self.replay = replay
        self.draw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.kdraw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.noise_buf = torch.zeros((S,) + tuple(shape), device=device) if replay else None      # x_T, then S - 1 main draws
        self.knoise_buf = torch.zeros((S,) + tuple(shape), device=device) if replay else None     # one known-draw per pair
        xv = self.x.view(B * N, C)

        def draw(buf, counter):
            if not self.replay:
                return torch.randn(shape, dtype=torch.float, device=device)
            n = buf.index_select(0, counter)[0]
            ops.add_scalar_i64(counter, 1)
            return n

        def step(final):
            plan.x_in.copy_(xv)
            plan.t_in.copy_(self.t)
            plan.run()
            noise = self.x if final else draw(self.noise_buf, self.draw)             # neither is read on the last pair
            nk = self.known if final else draw(self.knoise_buf, self.kdraw)
            ops.ddim_masked_step(self.x, plan.out.view(B, N, C), noise, self.known, nk, self.mask, self.step, self.times,
                                 self.times_next, self.coef, ca, cb, ra, rm, sa, sb, mean_type, out=self.x)
            if not final:
                ops.ddim_advance(self.step, self.times, self.t)

        # warm-up on a side stream, then capture; the caller's device RNG state is put back (see _StepGraph).  Tables, mask and the step
        # counter are all zero: every index of the warm-up is in range (see _DDIMCompleteGraph).
        rng_state = torch.cuda.get_rng_state(device)
        self.x.normal_()
        kinds = ([False] if S > 1 else []) + [True]
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for final in kinds:
                step(final)
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = None
        if S > 1:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                step(False)
        self.final = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.final, pool=self.graph.pool() if self.graph is not None else None):
            step(True)
        torch.cuda.set_rng_state(rng_state, device)
        self.step.zero_()

    def run(self, x_T, dtab, known, mask, noise_buffer=None, known_noise=None):
        pairs, times, times_next, coef = dtab
        assert len(pairs) == self.S
        self.check_current()
        self.times.copy_(times)                 # in place: the graphs hold these pointers
        self.times_next.copy_(times_next)
        self.coef.copy_(coef)
        self.x.copy_(x_T)
        self.step.zero_()
        self.t.fill_(pairs[0][0])
        self.known.copy_(known)
        self.mask.copy_(mask)
        if self.replay:
            self.noise_buf.copy_(noise_buffer[:self.S])
            self.knoise_buf.copy_(known_noise[:self.S])
            self.draw.fill_(1)                                  # draw 0 was x_T
            self.kdraw.fill_(1)                                 # known-draw 0 feeds the standalone overwrite below
        nk = self.knoise_buf[0] if self.replay else torch.randn(self.shape, dtype=torch.float, device=self.x.device)
        ops.masked_overwrite(self.x, self.known, nk, self.mask, self.t, self.tb["sqrt_alphas_cumprod"],
                             self.tb["sqrt_one_minus_alphas_cumprod"])
        for _ in range(self.S - 1):
            self.graph.replay()
        self.final.replay()
        return self.x.clone()


def graph_ddim_masked_loop(diff, denoise_fn, shape, device, condition, condition_cross, sampling_timesteps, eta, noise_fn=torch.randn,
                           known=None, mask=None):
    """ddim_masked_loop as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same order, the same
    generator state afterwards).  The cache key holds the shape and S; it holds neither eta nor the mask."""
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    B, N, C = shape
    S = int(sampling_timesteps)
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        if replay:
            _masked_replay_check(noise_fn, shape, S, S, "the strided masked loop")
        dtab = diff.ddim_tables(S, eta, device)
        key = (("ddim_masked", S), id(model), tuple(shape), str(device), diff.model_mean_type, replay,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0),
               None if condition_cross is None else tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = _DDIMMaskedGraph(diff, model, tuple(shape), device, condition, condition_cross, S, replay)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:
            eng.prepare(B, N, condition, condition_cross, time_table=g.plan.time_table)
        if replay:
            out = g.run(noise_fn.buffer[0], dtab, known, mask, noise_fn.buffer, noise_fn.partial_buffer)
        else:
            x_T = torch.randn(shape, dtype=torch.float, device=device)
            out = g.run(x_T, dtab, known, mask)
        from ._lib import check_indices
        check_indices("graph_ddim_masked_loop")
        return out


class _GuidedStepGraph:
    """The captured guided T-step loop (p_sample_loop_guided): _StepGraph with a plan prepared at 2 B -- rows [0, B) fed the text
    features, rows [B, 2 B) zeros --, the timestep vector filled for 2 B rows and the fused update dsc_p_sample_cfg_f32, which reads
    both halves of the plan's output and writes the new x to BOTH halves of ``x`` (2 B, N, C) (its x_dup pointer), so the copy into
    the plan's input stays one node.  The (B,) scale vector is a buffer of this object, captured by pointer and refreshed in place by
    ``run``: one graph serves every per-scene mix of scales.  ``fused=False`` captures the same step from the unfused kernels
    (cfg_combine, p_sample, a copy into the null half) -- the comparison of tools/bench_cfg.py."""

    check_current = _StepGraph.check_current

    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay=False, fused=True):
        B, N, C = shape
        self.shape, self.fused = shape, fused
        eng = model.engine(device)
        use_table = diff.num_timesteps <= eng.time_table.shape[0]
        self.plans = [eng.prepare(2 * B, N, condition, condition_cross, time_table=use_table)]
        self.plan = plan = self.plans[0]
        tb = diff.tables(device)
        ca, cb = diff._coeffs(tb)
        sigma = diff._sigma(tb)
        mean_type = _MEAN[diff.model_mean_type]
        k1, k2 = tb["posterior_mean_coef1"], tb["posterior_mean_coef2"]
        self.x2 = torch.empty((2 * B, N, C), device=device, dtype=torch.float32)
        self.x, self.x_null = self.x2[:B], self.x2[B:]
        self.t = torch.zeros((2 * B,), device=device, dtype=torch.int64)
        self.scale = torch.ones((B,), device=device, dtype=torch.float32)
        self.replay = replay
        self.draw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.noise_buf = torch.zeros((diff.num_timesteps + 1,) + tuple(shape), device=device) if replay else None
        self.m = None if fused else torch.empty(shape, device=device, dtype=torch.float32)
        xv = self.x2.view(2 * B * N, C)
        tB = self.t[:B]

        def step():
            plan.x_in.copy_(xv)
            plan.t_in.copy_(self.t)
            plan.run()
            if self.replay:
                noise = self.noise_buf.index_select(0, self.draw)[0]
                ops.add_scalar_i64(self.draw, 1)
            else:
                noise = torch.randn(shape, dtype=torch.float, device=device)
            mo = plan.out.view(2 * B, N, C)
            if fused:
                ops.p_sample_cfg(self.x, mo, self.scale, noise, tB, ca, cb, k1, k2, sigma, mean_type, clip_denoised, out=self.x,
                                 x_dup=self.x_null)
            else:
                ops.cfg_combine(mo, self.scale, out=self.m)
                ops.p_sample(self.x, self.m, noise, tB, ca, cb, k1, k2, sigma, mean_type, clip_denoised, out=self.x)
                self.x_null.copy_(self.x)
            ops.add_scalar_i64(self.t, -1)

        # warm-up on a side stream, then capture; the caller's device RNG state is put back (see _StepGraph)
        rng_state = torch.cuda.get_rng_state(device)
        self.x2.normal_()
        self.t.fill_(1)
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            step()
        torch.cuda.set_rng_state(rng_state, device)
        self.t.fill_(0)

    def replay_steps(self, n=1):
        self.check_current()
        for _ in range(n):
            self.graph.replay()

    def run(self, x_T, total_steps, scale, noise_buffer=None):
        self.check_current()
        self.x.copy_(x_T)
        self.x_null.copy_(x_T)
        self.t.fill_(total_steps - 1)
        self.scale.copy_(scale)                 # in place: the graph holds this pointer
        if self.replay:
            self.noise_buf[:noise_buffer.shape[0]].copy_(noise_buffer)
            self.draw.fill_(1)                                  # draw 0 was x_T
        for _ in range(total_steps):
            self.graph.replay()
        out = self.x.clone()
        self.t.fill_(0)                         # a valid row for a replay too many (see _StepGraph.run)
        return out


def graph_guided_loop(diff, denoise_fn, shape, device, condition, condition_cross, scale, clip_denoised, total_steps,
                      noise_fn=torch.randn, fused=True):
    """p_sample_loop_guided as a replayed hipGraph; bit-identical to the eager loop (same expressions, same draws in the same order, the
    same generator state afterwards).  ``condition`` / ``condition_cross`` arrive at 2 B (GaussianDiffusion._guided_inputs), ``scale`` is
    the (B,) f32 device vector of ops.guidance_scales: the cache key holds the shape, not the scales."""
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    B, N, C = shape
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        if replay and (noise_fn.buffer.shape[0] < total_steps + 1 or tuple(noise_fn.buffer.shape[1:]) != tuple(shape)):
            raise ValueError("the guided loop replays %d draws of shape %s" % (total_steps + 1, tuple(shape)))
        key = (("guided", bool(fused)), id(model), tuple(shape), str(device), bool(clip_denoised), diff.model_mean_type, replay,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0), tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = _GuidedStepGraph(diff, model, tuple(shape), device, condition, condition_cross, clip_denoised, replay, fused)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:
            eng.prepare(2 * B, N, condition, condition_cross, time_table=g.plan.time_table)
        if replay:
            out = g.run(noise_fn.buffer[0], total_steps, scale, noise_fn.buffer[:total_steps + 1])
        else:
            x_T = torch.randn(shape, dtype=torch.float, device=device)
            out = g.run(x_T, total_steps, scale)
        from ._lib import check_indices
        check_indices("graph_guided_loop")
        return out


class _DDIMGuidedGraph:
    """The captured guided strided loop (ddim_guided_loop): _DDIMGraph with the 2 B plan, the 2 B timestep vector and the fused update
    dsc_ddim_cfg_step_f32 of _GuidedStepGraph.  Tables, step counter and the scale vector live in buffers of this object, captured by
    pointer and refreshed in place: one graph serves every eta and every mix of scales.  ``fused=False``: the unfused kernels."""

    check_current = _StepGraph.check_current

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay=False, fused=True):
        B, N, C = shape
        self.shape, self.S, self.fused = shape, S, fused
        eng = model.engine(device)
        use_table = diff.num_timesteps <= eng.time_table.shape[0]
        self.plans = [eng.prepare(2 * B, N, condition, condition_cross, time_table=use_table)]
        self.plan = plan = self.plans[0]
        tb = diff.tables(device)
        ca, cb = diff._coeffs(tb)
        ra, rm = tb["sqrt_recip_alphas_cumprod"], tb["sqrt_recipm1_alphas_cumprod"]
        mean_type = _MEAN[diff.model_mean_type]
        self.x2 = torch.empty((2 * B, N, C), device=device, dtype=torch.float32)
        self.x, self.x_null = self.x2[:B], self.x2[B:]
        self.t = torch.zeros((2 * B,), device=device, dtype=torch.int64)
        self.scale = torch.ones((B,), device=device, dtype=torch.float32)
        self.step = torch.zeros((1,), device=device, dtype=torch.int64)
        self.times = torch.zeros((S,), device=device, dtype=torch.int64)
        self.times_next = torch.zeros((S,), device=device, dtype=torch.int64)
        self.coef = torch.zeros((3, S), device=device, dtype=torch.float32)
        self.replay = replay
        self.draw = torch.zeros((1,), device=device, dtype=torch.int64)
        self.noise_buf = torch.zeros((S,) + tuple(shape), device=device) if replay else None    # x_T, then S - 1 step draws
        self.m = None if fused else torch.empty(shape, device=device, dtype=torch.float32)
        xv = self.x2.view(2 * B * N, C)

        def step(final):
            plan.x_in.copy_(xv)
            plan.t_in.copy_(self.t)
            plan.run()
            if final:
                noise = self.x                                   # not read on the last pair
            elif self.replay:
                noise = self.noise_buf.index_select(0, self.draw)[0]
                ops.add_scalar_i64(self.draw, 1)
            else:
                noise = torch.randn(shape, dtype=torch.float, device=device)
            mo = plan.out.view(2 * B, N, C)
            if fused:
                ops.ddim_cfg_step(self.x, mo, self.scale, noise, self.step, self.times, self.times_next, self.coef, ca, cb, ra, rm,
                                  mean_type, out=self.x, x_dup=self.x_null)
            else:
                ops.cfg_combine(mo, self.scale, out=self.m)
                ops.ddim_step(self.x, self.m, noise, self.step, self.times, self.times_next, self.coef, ca, cb, ra, rm, mean_type,
                              out=self.x)
                self.x_null.copy_(self.x)
            if not final:
                ops.ddim_advance(self.step, self.times, self.t)

        # warm-up on a side stream, then capture; the caller's device RNG state is put back (see _StepGraph).  With all-zero tables
        # every index of the warm-up is in range (see _DDIMGraph).
        rng_state = torch.cuda.get_rng_state(device)
        self.x2.normal_()
        kinds = ([False] if S > 1 else []) + [True]
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for final in kinds:
                step(final)
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = None
        if S > 1:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                step(False)
        self.final = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.final, pool=self.graph.pool() if self.graph is not None else None):
            step(True)
        torch.cuda.set_rng_state(rng_state, device)
        self.step.zero_()

    def run(self, x_T, dtab, scale, noise_buffer=None):
        pairs, times, times_next, coef = dtab
        assert len(pairs) == self.S
        self.check_current()
        self.times.copy_(times)                 # in place: the graphs hold these pointers
        self.times_next.copy_(times_next)
        self.coef.copy_(coef)
        self.scale.copy_(scale)
        self.x.copy_(x_T)
        self.x_null.copy_(x_T)
        self.step.zero_()
        self.t.fill_(pairs[0][0])
        if self.replay:
            self.noise_buf.copy_(noise_buffer[:self.S])
            self.draw.fill_(1)                                  # draw 0 was x_T
        for _ in range(self.S - 1):
            self.graph.replay()
        self.final.replay()
        return self.x.clone()


def graph_ddim_guided_loop(diff, denoise_fn, shape, device, condition, condition_cross, scale, sampling_timesteps, eta,
                           noise_fn=torch.randn, fused=True):
    """ddim_guided_loop as replayed hipGraphs; bit-identical to the eager loop.  The cache key holds the shape and S; it holds neither
    eta nor the scales."""
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    B, N, C = shape
    S = int(sampling_timesteps)
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        if replay and (noise_fn.buffer.shape[0] < S or tuple(noise_fn.buffer.shape[1:]) != tuple(shape)):
            raise ValueError("the guided strided loop replays %d draws of shape %s" % (S, tuple(shape)))
        dtab = diff.ddim_tables(S, eta, device)
        key = (("ddim_guided", S, bool(fused)), id(model), tuple(shape), str(device), diff.model_mean_type, replay,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0), tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = _DDIMGuidedGraph(diff, model, tuple(shape), device, condition, condition_cross, S, replay, fused)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:
            eng.prepare(2 * B, N, condition, condition_cross, time_table=g.plan.time_table)
        if replay:
            out = g.run(noise_fn.buffer[0], dtab, scale, noise_fn.buffer)
        else:
            x_T = torch.randn(shape, dtype=torch.float, device=device)
            out = g.run(x_T, dtab, scale)
        from ._lib import check_indices
        check_indices("graph_ddim_guided_loop")
        return out


def _plan_key(g):
    p = g.plan
    return (p.B, p.N, p.ctx_mode, 0 if p.ctx_in is None else p.ctx_in.shape[1], p.L,
            0 if p.cross_in is None else p.cross_in.shape[1], p.time_table)        # slot 0 carries no suffix
