"""hipGraph-captured reverse diffusion loops (reference p_sample_loop, diffusion_ddpm.py:355-371, and its variants).

The reference launches ~800 kernels per step from Python, 8e5 launches per sample.  Here ONE reverse step -- the
denoiser launch plan (~140 kernels), the noise draws and one fused update kernel -- is captured once into a hipGraph whose only state
is device-resident and replayed once per step; the timestep moves on inside the graph.  Every loop is bit-identical to its eager twin
in diffusion_ddpm.py: the same kernels, the same draws in the same order and shapes, the same generator state afterwards.

Structure:
  _Draws          one noise stream of a loop: torch.randn, the rows of a replay buffer behind a device counter, or -- seeded -- the
                  per-scene noise kernel (scene_noise.py) on the graph's seed buffer behind a device draw counter.
  _LoopGraph      the core: launch plans, the state (x, t), the main noise stream, the model call, warm-up + capture that costs the
                  caller no random numbers (``graph``: a step that is followed by another, ``final``: the last one where it differs),
                  the stale-pointer check and the replays.
  _PosteriorLoop  the T-step layer: t counts down by a kernel in the graph; T + 1 main draws (x_T, then one per step, also at t == 0).
  _DDIMLoop       the strided layer (ddim_sample_loop, :402-444): a device step counter and per-pair tables (t, t_next, coefficients)
                  owned here and refreshed in place, the advance kernel; S main draws (none on the last pair).  S == 1: no ``graph``.
  _Ragged, _Masked   the given part of a scene (a row prefix with per-scene counts / a byte mask) in graph-owned buffers, its own
                  noise stream, shifted by one: draw 0 feeds a standalone overwrite in ``run``, the fused step re-noises for the NEXT
                  model call, the last step restores -- so a given element costs no posterior step and the draw order stays the eager one.
What the ten classes add:
  _StepGraph (p_sample_loop, _complete)     optional sub-batch chains (_chains_for), optional dense overwrite before the model call
  _DDIMGraph (ddim_sample_loop, strided re-arrangement on the sub-shape)             dsc_ddim_step_f32
  _RaggedCompleteGraph / _DDIMCompleteGraph  _Ragged + dsc_p_sample_inpaint_f32 / dsc_ddim_inpaint_step_f32; fused=False: unfused kernels
  _MaskedGraph / _DDIMMaskedGraph            _Masked + dsc_p_sample_masked_f32 / dsc_ddim_masked_step_f32
  _GuidedStepGraph / _DDIMGuidedGraph        a plan at 2 B (text features | zeros), x kept in both halves of one (2 B, N, C) buffer,
                                             per-scene scales in a buffer, dsc_p_sample_cfg_f32 / dsc_ddim_cfg_step_f32; fused=False
  _MaskedGuidedGraph / _DDIMMaskedGuidedGraph   _Masked + _Guided: known, mask and the known-draws at B under a plan at 2 B,
                                             dsc_p_sample_masked_cfg_f32 / dsc_ddim_masked_cfg_step_f32; fused=False
The graph_*_loop functions are the front ends behind diffusion_ddpm.py: one cached graph per diffusion object (_cached_loop).
"""
import torch

from . import ops
from .networks.denoise_net import Unet1D
from .networks.diffusion_ddpm import restore_given_rows
from .scene_noise import GIVEN, MAIN, SceneNoise

RANDN, REPLAY, SEEDED = "randn", "replay", "seeded"            # the noise modes of a captured loop

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


def _prepare_plans(eng, rows, N, condition, condition_cross, time_table, nch=1):
    """The launch plans of one step at ``rows`` scenes -- one per sub-batch chain, each on its slice of the conditioning.  Also the
    refresh of weights + conditioning buffers before a cached graph runs again.  One chain takes the conditioning as it is given."""
    if nch == 1:
        return [eng.prepare(rows, N, condition, condition_cross, time_table=time_table)]
    Bc = rows // nch
    return [eng.prepare(Bc, N, None if condition is None else condition[i * Bc:(i + 1) * Bc],
                        None if condition_cross is None else condition_cross[i * Bc:(i + 1) * Bc],
                        time_table=time_table, slot=i) for i in range(nch)]


class _Draws:
    """One noise stream of a captured loop.  A call is one draw: torch.randn of the stream's shape; or -- when replaying -- row
    ``counter`` of ``buf``; or -- seeded -- draw number ``counter`` of stream ``stream`` under the (B,) seed buffer ``seeds`` of the
    graph (dsc_scene_randn_f32 reads the counter through its pointer).  The two counted modes end with a counter increment, device-side,
    so the captured step walks the buffer / the draw numbers as it is replayed."""

    def __init__(self, shape, device, rows=None, seeds=None, stream=MAIN):
        self.shape, self.device = tuple(shape), device
        self.buf = None if rows is None else torch.zeros((rows,) + self.shape, device=device)
        self.seeds, self.stream = seeds, stream
        self.counter = torch.zeros((1,), device=device, dtype=torch.int64)
        self.zero = torch.zeros((1,), device=device, dtype=torch.int64) if seeds is not None else None

    def __call__(self):
        if self.seeds is not None:
            n = ops.scene_randn(self.seeds, self.counter, self.stream, self.shape)
            ops.add_scalar_i64(self.counter, 1)
            return n
        if self.buf is None:
            return torch.randn(self.shape, dtype=torch.float, device=self.device)
        n = self.buf.index_select(0, self.counter)[0]
        ops.add_scalar_i64(self.counter, 1)
        return n

    def head(self):
        """Draw 0, taken outside the graph (x_T of a seeded loop, the standalone first overwrite); a counted loop then starts its
        counter at 1."""
        if self.seeds is not None:
            return ops.scene_randn(self.seeds, self.zero, self.stream, self.shape)
        return self() if self.buf is None else self.buf[0]


class _LoopGraph:
    """The core of every captured loop; a subclass adds its buffers, ``_step(final)`` and ``run``.  ``mult``: scenes of the plan per
    scene of the loop (2 for the guided loops), ``draws``: rows of the main replay buffer, ``nch``: sub-batch chains.  ``replay``: the
    noise mode -- False / RANDN, True / REPLAY, or SEEDED: the graph owns a (B,) seed buffer, refreshed in place by ``seeded_x_T``."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, replay, draws, mult=1, nch=1):
        B, N, C = shape
        self.shape, self.device = shape, device
        self.mode = {False: RANDN, True: REPLAY}.get(replay, replay)
        assert self.mode in (RANDN, REPLAY, SEEDED), replay
        self.replay = self.mode == REPLAY
        self.seeds = torch.zeros((B,), device=device, dtype=torch.int64) if self.mode == SEEDED else None
        eng = model.engine(device)
        self.plans = _prepare_plans(eng, mult * B, N, condition, condition_cross, diff.num_timesteps <= eng.time_table.shape[0], nch)
        self.plan = self.plans[0]
        self.tb = tb = diff.tables(device)
        self.ca, self.cb = diff._coeffs(tb)
        self.q = (tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"])           # q_sample of the given part
        self.mean_type = _MEAN[diff.model_mean_type]
        # the plan's input rows; guided: x is kept current in both halves, so the copy into the plan's input stays one node
        self.x2 = torch.empty((mult * B, N, C), device=device, dtype=torch.float32)
        self.x, self.x_null = (self.x2, None) if mult == 1 else (self.x2[:B], self.x2[B:])
        self.t = torch.zeros((mult * B,), device=device, dtype=torch.int64)
        self.noise = self._stream(shape, draws)
        self.graph = self.final = None

    def _stream(self, shape, rows, stream=MAIN):
        return _Draws(shape, self.device, rows if self.replay else None, self.seeds, stream)

    def seeded_x_T(self, seeds):
        """The seeds of this run into the graph's own buffer, in place (the captured launches hold its pointer) -> x_T, main draw 0."""
        self.seeds.copy_(seeds)
        return self.noise.head()

    def _model_call(self):
        plan = self.plan
        plan.x_in.copy_(self.x2.view(-1, self.shape[2]))
        plan.t_in.copy_(self.t)
        plan.run()
        return plan.out.view(self.x2.shape)

    def _capture(self, kinds):
        """Warm-up on a side stream (loads every code object, sizes the allocator), then capture: ``graph`` = _step(False) and
        ``final`` = _step(True), from ``graph``'s pool where there is one, for the kinds asked for.
        Building the graph must not cost the caller random numbers: the loops are the default path behind the reference's call sites,
        and a run seeded with torch.manual_seed has to draw what the eager loop draws whether or not this call had to capture first --
        so the device generator's state is put back afterwards (normal_() and the warm-up steps draw from it).
        Every index of the warm-up is in range (the kernels clamp and count a bad one: dsc_device_error_count): the buffers of a new
        object are all zero -- counts, mask, the strided tables and their step counter, which the advance moves to 1 < S only when
        there is a non-final step, and times_next[.] = 0 reads row 0 of the schedule; the T-step layer starts t at row 1, which the
        steps walk down to 0."""
        dev = self.device
        rng_state = torch.cuda.get_rng_state(dev)
        self.x2.normal_()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for final in kinds:
                self._step(final)
        torch.cuda.current_stream(dev).wait_stream(side)
        for final in kinds:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=None if self.graph is None else self.graph.pool()):
                self._step(final)
            if final:
                self.final = g
            else:
                self.graph = g
        torch.cuda.set_rng_state(rng_state, dev)
        self._park()

    def _park(self):
        """The in-graph timestep holds -1 after a T-step loop: put the counters on valid rows, so that one replay too many (a caller
        driving ``graph`` directly) still indexes the schedule tables in range."""
        self.t.fill_(0)

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

    def _load_x(self, x_T):
        self.x.copy_(x_T)
        if self.x_null is not None:
            self.x_null.copy_(x_T)

    def _start(self, x_T, t0):
        self._load_x(x_T)
        self.t.fill_(t0)

    def _copy_rows(self, dst, src):
        dst[:src.shape[0]].copy_(src)           # a loop of fewer steps than the schedule fills a prefix

    def _upload(self, *loads):
        """(stream, buffer, first row) each: the replay buffers go into the graph's own, in place, then the counters are set --
        main draw 0 was x_T, draw 0 of a shifted stream feeds the standalone overwrite (_Draws.head).  A seeded loop has no buffers:
        its counters start on the same numbers."""
        if self.mode == RANDN:
            return
        if self.replay:
            for d, buffer, _ in loads:
                self._copy_rows(d.buf, buffer)
        for d, _, first in loads:
            d.counter.fill_(first)

    def _replays(self, steps):
        """One loop of ``steps`` steps: the last one from ``final`` where the class has one."""
        for _ in range(steps - (self.final is not None)):
            self.graph.replay()
        if self.final is not None:
            self.final.replay()
        return self.x.clone()


class _PosteriorLoop(_LoopGraph):
    """The T-step layer: ``post`` / ``tail`` are the argument runs of ops.p_sample*, the graph decrements t."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay, mult=1, nch=1):
        super().__init__(diff, model, shape, device, condition, condition_cross, replay, diff.num_timesteps + 1, mult, nch)
        self.T = diff.num_timesteps
        tb = self.tb
        self.post = (self.ca, self.cb, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], diff._sigma(tb))
        self.tail = (self.mean_type, clip_denoised)

    def _capture(self, kinds):
        self.t.fill_(1)
        super()._capture(kinds)


class _DDIMLoop(_LoopGraph):
    """The strided layer.  The step counter and the per-pair tables (t, t_next; sqrt(alpha_next), c, sigma) are captured by pointer:
    this object owns them and ``_load_tables`` refreshes them IN PLACE (eta is not part of the cache key), so a live graph never
    points at a freed table.  ``graph`` (S > 1 only) ends with the advance kernel (step += 1, t = times[step]) and is replayed S - 1
    times; ``final`` is the draw-free last pair ((t, -1) -> x_start), from a fresh pool when S == 1."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay, mult=1):
        super().__init__(diff, model, shape, device, condition, condition_cross, replay, S, mult)
        self.S = S
        self.kinds = ([False] if S > 1 else []) + [True]
        self.step = torch.zeros((1,), device=device, dtype=torch.int64)
        self.times = torch.zeros((S,), device=device, dtype=torch.int64)
        self.times_next = torch.zeros((S,), device=device, dtype=torch.int64)
        self.coef = torch.zeros((3, S), device=device, dtype=torch.float32)
        self.tabs = (self.step, self.times, self.times_next, self.coef)                     # the argument runs of ops.ddim_*step
        self.ddim = (self.ca, self.cb, self.tb["sqrt_recip_alphas_cumprod"], self.tb["sqrt_recipm1_alphas_cumprod"])

    def _park(self):
        super()._park()
        self.step.zero_()

    def _start(self, x_T, t0):
        self._load_x(x_T)
        self.step.zero_()
        self.t.fill_(t0)

    def _copy_rows(self, dst, src):
        dst.copy_(src[:self.S])                 # the buffers hold exactly S rows

    def _advance(self, final):
        if not final:
            ops.ddim_advance(self.step, self.times, self.t)

    def _load_tables(self, dtab):
        """-> the first timestep."""
        pairs, times, times_next, coef = dtab
        assert len(pairs) == self.S
        self.check_current()
        self.times.copy_(times)                 # in place: the graphs hold these pointers
        self.times_next.copy_(times_next)
        self.coef.copy_(coef)
        return pairs[0][0]


class _Ragged:
    """Given objects as a row prefix: the padded objects (B, Pmax, C) and the (B,) int64 counts (ops.ragged_counts) live in buffers of
    the graph, captured by pointer and refreshed in place -- one graph serves every mix of counts -- with their own noise stream.
    ``fused=False`` is the comparison of tools/bench_complete.py / bench_ddim_complete.py: every step begins with the unfused overwrite."""

    def _init_given(self, pmax, rows, fused):          # _Masked._init_given takes ``rows`` alone, on purpose: a class uses one of the two
        B, N, C = self.shape
        self.pmax, self.fused = pmax, fused
        self.partial = torch.zeros((B, pmax, C), device=self.device, dtype=torch.float32)
        self.counts = torch.zeros((B,), device=self.device, dtype=torch.int64)
        self.pnoise = self._stream((B, pmax, C), rows, GIVEN)

    def _overwrite(self, pn):
        ops.complete_overwrite_ragged(self.x, self.partial, pn, self.counts, self.t, *self.q)

    def _begin_given(self, partial, counts, noise_buffer, partial_noise):
        self.partial.copy_(partial)             # in place: the graphs hold these pointers
        self.counts.copy_(counts)
        self._upload((self.noise, noise_buffer, 1), (self.pnoise, partial_noise, 1 if self.fused else 0))
        if self.fused:
            self._overwrite(self.pnoise.head())

    def _restore(self, out):
        return out if self.fused else restore_given_rows(out, self.partial, self.counts)


class _Masked:
    """Given elements as a byte mask: ``known`` (B, N, C) f32 and ``mask`` (B, N, C) uint8 (ops.known_mask) live in buffers of the
    graph, captured by pointer and refreshed in place -- one graph per shape serves every mask -- with full-shape known-draws."""

    def _init_given(self, rows):
        self.known = torch.zeros(self.shape, device=self.device, dtype=torch.float32)
        self.mask = torch.zeros(self.shape, device=self.device, dtype=torch.uint8)
        self.knoise = self._stream(self.shape, rows, GIVEN)

    def _begin_given(self, known, mask, noise_buffer, known_noise):
        self.known.copy_(known)                 # in place: the graphs hold these pointers
        self.mask.copy_(mask)
        self._upload((self.noise, noise_buffer, 1), (self.knoise, known_noise, 1))
        ops.masked_overwrite(self.x, self.known, self.knoise.head(), self.mask, self.t[:self.shape[0]], *self.q)
        if self.x_null is not None:             # guided: both halves of the state stay current
            self.x_null.copy_(self.x)


class _StepGraph(_PosteriorLoop):
    """p_sample_loop: model call, draw, dsc_p_sample_f32, decrement; no ``final`` (the draw is made at t == 0 too).  With
    ``partial_shape`` p_sample_loop_complete (:461-466): the given objects are re-noised and written over the first P rows of x_t at
    every step, BEFORE the model call."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay=False,
                 partial_shape=None):
        nch = _chains_for(shape[0])
        super().__init__(diff, model, shape, device, condition, condition_cross, clip_denoised, replay, nch=nch)
        self.side = [torch.cuda.Stream(device=device) for _ in range(nch - 1)]
        self.model_out = torch.empty(shape, device=device, dtype=torch.float32) if nch > 1 else None
        self.partial = torch.zeros(partial_shape, device=device) if partial_shape is not None else None
        self.pnoise = self._stream(partial_shape, self.T, GIVEN) if partial_shape is not None else None
        self._capture([False])

    def _model_call(self):
        nch = len(self.plans)
        if nch == 1:
            return super()._model_call()
        B, N, C = self.shape
        Bc = B // nch
        xv = self.x.view(B * N, C)

        def run_chain(i):
            p = self.plans[i]
            p.x_in.copy_(xv[i * Bc * N:(i + 1) * Bc * N])
            p.t_in.copy_(self.t[i * Bc:(i + 1) * Bc])
            p.run()
            self.model_out.view(B * N, C)[i * Bc * N:(i + 1) * Bc * N].copy_(p.out)

        cur = torch.cuda.current_stream(self.device)
        for st in self.side:
            st.wait_stream(cur)
        run_chain(0)
        for i, st in enumerate(self.side):
            with torch.cuda.stream(st):
                run_chain(i + 1)
        for st in self.side:
            cur.wait_stream(st)
        return self.model_out

    def _step(self, final):
        if self.partial is not None:
            ops.complete_overwrite(self.x, self.partial, self.pnoise(), self.t, *self.q)
        mo = self._model_call()
        ops.p_sample(self.x, mo, self.noise(), self.t, *self.post, *self.tail, out=self.x)
        ops.add_scalar_i64(self.t, -1)

    def run(self, x_T, total_steps, noise_buffer=None, partial=None, partial_noise=None):
        self.check_current()
        self._start(x_T, total_steps - 1)
        if self.partial is not None:
            self.partial.copy_(partial)
        self._upload((self.noise, noise_buffer, 1))
        if self.partial is not None:
            self._upload((self.pnoise, partial_noise, 0))
        out = self._replays(total_steps)
        self._park()
        return out


class _DDIMGraph(_DDIMLoop):
    """ddim_sample_loop: model call, draw, dsc_ddim_step_f32, advance."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay=False):
        super().__init__(diff, model, shape, device, condition, condition_cross, S, replay)
        self._capture(self.kinds)

    def _step(self, final):
        mo = self._model_call()
        noise = self.x if final else self.noise()                # not read on the last pair
        ops.ddim_step(self.x, mo, noise, *self.tabs, *self.ddim, self.mean_type, out=self.x)
        self._advance(final)

    def run(self, x_T, dtab, noise_buffer=None):
        self._start(x_T, self._load_tables(dtab))
        self._upload((self.noise, noise_buffer, 1))
        return self._replays(self.S)


class _RaggedCompleteGraph(_Ragged, _PosteriorLoop):
    """p_sample_loop_complete_ragged.  ``graph``: model call, the main draw, the partial draw of the NEXT step, the fused update
    (posterior step on the free rows, re-noised given objects on the others), decrement; replayed total_steps - 1 times.  ``final``:
    model call, the main draw and the fused update at t == 0 (given rows restored, no partial draw).  ``fused=False``: partial draw,
    ragged overwrite, model call, main draw, p_sample, decrement, every step from ``graph``; restore after the loop."""

    def __init__(self, diff, model, shape, pmax, device, condition, condition_cross, clip_denoised, replay=False, fused=True):
        super().__init__(diff, model, shape, device, condition, condition_cross, clip_denoised, replay)
        self._init_given(pmax, self.T, fused)
        self._capture([False, True] if fused else [False])

    def _step(self, final):
        if not self.fused:
            self._overwrite(self.pnoise())
            mo = self._model_call()
            ops.p_sample(self.x, mo, self.noise(), self.t, *self.post, *self.tail, out=self.x)
            ops.add_scalar_i64(self.t, -1)
            return
        mo = self._model_call()
        noise = self.noise()
        pn = self.partial if final else self.pnoise()           # not read at t == 0
        ops.p_sample_inpaint(self.x, mo, noise, self.partial, pn, self.counts, self.t, *self.post, *self.q, *self.tail, out=self.x)
        if not final:
            ops.add_scalar_i64(self.t, -1)

    def run(self, x_T, total_steps, partial, counts, noise_buffer=None, partial_noise=None):
        self.check_current()
        self._start(x_T, total_steps - 1)
        self._begin_given(partial, counts, noise_buffer, partial_noise)
        out = self._restore(self._replays(total_steps))
        self._park()
        return out


class _DDIMCompleteGraph(_Ragged, _DDIMLoop):
    """ddim_complete_ragged_loop.  ``graph``: model call, main draw k, the partial draw of pair k + 1, the fused update (DDIM step on
    the free rows, the given objects re-noised at t_next on the others), advance.  ``final``: model call and the draw-free fused step of
    the last pair (x_start on the free rows, the given rows restored).  2 S draws: x_T, then per pair a partial draw (B, Pmax, C), the
    model call and a main draw (B, N, C); the last pair makes the partial draw only.  ``fused=False``: partial draw, ragged overwrite,
    model call, main draw, ddim_step, advance; restore after the loop."""

    def __init__(self, diff, model, shape, pmax, device, condition, condition_cross, S, replay=False, fused=True):
        super().__init__(diff, model, shape, device, condition, condition_cross, S, replay)
        self._init_given(pmax, S, fused)
        self._capture(self.kinds)

    def _step(self, final):
        if not self.fused:
            self._overwrite(self.pnoise())
        mo = self._model_call()
        noise = self.x if final else self.noise()                # neither is read on the last pair
        if not self.fused:
            ops.ddim_step(self.x, mo, noise, *self.tabs, *self.ddim, self.mean_type, out=self.x)
        else:
            pn = self.partial if final else self.pnoise()
            ops.ddim_inpaint_step(self.x, mo, noise, self.partial, pn, self.counts, *self.tabs, *self.ddim, *self.q, self.mean_type,
                                  out=self.x)
        self._advance(final)

    def run(self, x_T, dtab, partial, counts, noise_buffer=None, partial_noise=None):
        self._start(x_T, self._load_tables(dtab))
        self._begin_given(partial, counts, noise_buffer, partial_noise)
        return self._restore(self._replays(self.S))


class _MaskedGraph(_Masked, _PosteriorLoop):
    """p_sample_loop_masked: _RaggedCompleteGraph's fused step on a mask -- the main draw of t, the known-draw of t - 1,
    dsc_p_sample_masked_f32; ``final`` at t == 0 sets the given elements to ``known`` and makes no known-draw."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay=False):
        super().__init__(diff, model, shape, device, condition, condition_cross, clip_denoised, replay)
        self._init_given(self.T)
        self._capture([False, True])

    def _step(self, final):
        mo = self._model_call()
        noise = self.noise()
        nk = self.known if final else self.knoise()             # not read at t == 0
        ops.p_sample_masked(self.x, mo, noise, self.known, nk, self.mask, self.t, *self.post, *self.q, *self.tail, out=self.x)
        if not final:
            ops.add_scalar_i64(self.t, -1)

    def run(self, x_T, total_steps, known, mask, noise_buffer=None, known_noise=None):
        self.check_current()
        self._start(x_T, total_steps - 1)
        self._begin_given(known, mask, noise_buffer, known_noise)
        out = self._replays(total_steps)
        self._park()
        return out


class _DDIMMaskedGraph(_Masked, _DDIMLoop):
    """ddim_masked_loop: _DDIMCompleteGraph's fused step on a mask -- main draw k, the known-draw of pair k + 1,
    dsc_ddim_masked_step_f32; ``final``: x_start on the free elements, ``known`` on the given ones, no draw."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay=False):
        super().__init__(diff, model, shape, device, condition, condition_cross, S, replay)
        self._init_given(S)
        self._capture(self.kinds)

    def _step(self, final):
        mo = self._model_call()
        noise = self.x if final else self.noise()                # neither is read on the last pair
        nk = self.known if final else self.knoise()
        ops.ddim_masked_step(self.x, mo, noise, self.known, nk, self.mask, *self.tabs, *self.ddim, *self.q, self.mean_type, out=self.x)
        self._advance(final)

    def run(self, x_T, dtab, known, mask, noise_buffer=None, known_noise=None):
        self._start(x_T, self._load_tables(dtab))
        self._begin_given(known, mask, noise_buffer, known_noise)
        return self._replays(self.S)


class _Guided:
    """Classifier-free guidance: the plan runs at 2 B -- rows [0, B) fed the text features, rows [B, 2 B) zeros -- on the same x and t
    in both halves; the fused kernels read both halves of the plan's output and write the new x to BOTH halves of ``x2`` (their x_dup
    pointer).  The (B,) scale vector (ops.guidance_scales) is a buffer of the graph, captured by pointer and refreshed in place: one
    graph serves every per-scene mix of scales.  ``fused=False`` is the comparison of tools/bench_cfg.py: cfg_combine into ``m``, the
    unguided step kernel, a copy into the null half."""

    def _init_guided(self, fused):
        self.fused = fused
        self.scale = torch.ones((self.shape[0],), device=self.device, dtype=torch.float32)
        self.m = None if fused else torch.empty(self.shape, device=self.device, dtype=torch.float32)
        self.tB = self.t[:self.shape[0]]


class _GuidedStepGraph(_Guided, _PosteriorLoop):
    """p_sample_loop_guided: _StepGraph's step with dsc_p_sample_cfg_f32."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay=False, fused=True):
        super().__init__(diff, model, shape, device, condition, condition_cross, clip_denoised, replay, mult=2)
        self._init_guided(fused)
        self._capture([False])

    def _step(self, final):
        mo = self._model_call()
        noise = self.noise()
        if self.fused:
            ops.p_sample_cfg(self.x, mo, self.scale, noise, self.tB, *self.post, *self.tail, out=self.x, x_dup=self.x_null)
        else:
            ops.cfg_combine(mo, self.scale, out=self.m)
            ops.p_sample(self.x, self.m, noise, self.tB, *self.post, *self.tail, out=self.x)
            self.x_null.copy_(self.x)
        ops.add_scalar_i64(self.t, -1)

    def run(self, x_T, total_steps, scale, noise_buffer=None):
        self.check_current()
        self._start(x_T, total_steps - 1)
        self.scale.copy_(scale)                 # in place: the graph holds this pointer
        self._upload((self.noise, noise_buffer, 1))
        out = self._replays(total_steps)
        self._park()
        return out


class _DDIMGuidedGraph(_Guided, _DDIMLoop):
    """ddim_guided_loop: _DDIMGraph's step with dsc_ddim_cfg_step_f32."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay=False, fused=True):
        super().__init__(diff, model, shape, device, condition, condition_cross, S, replay, mult=2)
        self._init_guided(fused)
        self._capture(self.kinds)

    def _step(self, final):
        mo = self._model_call()
        noise = self.x if final else self.noise()                # not read on the last pair
        if self.fused:
            ops.ddim_cfg_step(self.x, mo, self.scale, noise, *self.tabs, *self.ddim, self.mean_type, out=self.x, x_dup=self.x_null)
        else:
            ops.cfg_combine(mo, self.scale, out=self.m)
            ops.ddim_step(self.x, self.m, noise, *self.tabs, *self.ddim, self.mean_type, out=self.x)
            self.x_null.copy_(self.x)
        self._advance(final)

    def run(self, x_T, dtab, scale, noise_buffer=None):
        t0 = self._load_tables(dtab)
        self.scale.copy_(scale)
        self._start(x_T, t0)
        self._upload((self.noise, noise_buffer, 1))
        return self._replays(self.S)


class _MaskedGuidedGraph(_Masked, _Guided, _PosteriorLoop):
    """p_sample_loop_masked_guided: _MaskedGraph's step on a plan at 2 B with dsc_p_sample_masked_cfg_f32; known, mask and the
    known-draws stay at B.  ``fused=False``: cfg_combine into ``m``, dsc_p_sample_masked_f32, a copy into the null half."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay=False, fused=True):
        super().__init__(diff, model, shape, device, condition, condition_cross, clip_denoised, replay, mult=2)
        self._init_given(self.T)
        self._init_guided(fused)
        self._capture([False, True])

    def _step(self, final):
        mo = self._model_call()
        noise = self.noise()
        nk = self.known if final else self.knoise()             # not read at t == 0
        if self.fused:
            ops.p_sample_masked_cfg(self.x, mo, self.scale, noise, self.known, nk, self.mask, self.tB, *self.post, *self.q, *self.tail,
                                    out=self.x, x_dup=self.x_null)
        else:
            ops.cfg_combine(mo, self.scale, out=self.m)
            ops.p_sample_masked(self.x, self.m, noise, self.known, nk, self.mask, self.tB, *self.post, *self.q, *self.tail, out=self.x)
            self.x_null.copy_(self.x)
        if not final:
            ops.add_scalar_i64(self.t, -1)

    def run(self, x_T, total_steps, scale, known, mask, noise_buffer=None, known_noise=None):
        self.check_current()
        self._start(x_T, total_steps - 1)
        self.scale.copy_(scale)                 # in place: the graph holds this pointer
        self._begin_given(known, mask, noise_buffer, known_noise)
        out = self._replays(total_steps)
        self._park()
        return out


class _DDIMMaskedGuidedGraph(_Masked, _Guided, _DDIMLoop):
    """ddim_masked_guided_loop: _DDIMMaskedGraph's step on a plan at 2 B with dsc_ddim_masked_cfg_step_f32; ``fused=False`` as in
    _MaskedGuidedGraph, with dsc_ddim_masked_step_f32."""

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay=False, fused=True):
        super().__init__(diff, model, shape, device, condition, condition_cross, S, replay, mult=2)
        self._init_given(S)
        self._init_guided(fused)
        self._capture(self.kinds)

    def _step(self, final):
        mo = self._model_call()
        noise = self.x if final else self.noise()                # neither is read on the last pair
        nk = self.known if final else self.knoise()
        if self.fused:
            ops.ddim_masked_cfg_step(self.x, mo, self.scale, noise, self.known, nk, self.mask, *self.tabs, *self.ddim, *self.q,
                                     self.mean_type, out=self.x, x_dup=self.x_null)
        else:
            ops.cfg_combine(mo, self.scale, out=self.m)
            ops.ddim_masked_step(self.x, self.m, noise, self.known, nk, self.mask, *self.tabs, *self.ddim, *self.q, self.mean_type,
                                 out=self.x)
            self.x_null.copy_(self.x)
        self._advance(final)

    def run(self, x_T, dtab, scale, known, mask, noise_buffer=None, known_noise=None):
        t0 = self._load_tables(dtab)
        self.scale.copy_(scale)
        self._start(x_T, t0)
        self._begin_given(known, mask, noise_buffer, known_noise)
        return self._replays(self.S)


def _cached_loop(name, diff, denoise_fn, shape, device, condition, condition_cross, noise_fn, tag, make, run, mult=1, check=None,
                 ddim=None):
    """The front end of every graph_*_loop.  ``tag``: what of the loop's arguments shapes the graph (the loop, clip_denoised, S, Pmax,
    fused -- never eta, counts, mask or scales, which live in buffers); the key adds the model, the shape and the conditioning's
    shapes and the noise mode (randn / replay / seeded -- never the seeds, which live in a buffer).  ``check(noise_fn)`` validates a
    NoiseReplay, ``make(model, device, replay)`` builds the graph (``replay``: the noise mode) when there is none for the key or its plan
    is stale, ``run(g, x_T, main buffer, partial buffer, dtab)`` runs it; ``ddim`` = (S, eta) of a strided loop, whose
    device tables ``dtab`` are looked up here."""
    model = getattr(getattr(denoise_fn, "__self__", None), "model", None)
    if not isinstance(model, Unet1D):
        raise RuntimeError("graph sampling needs DiffusionPoint._denoise over a diffuscene_amd Unet1D")
    device = torch.device(device)
    shape = tuple(shape)
    with torch.no_grad():
        replay = isinstance(noise_fn, NoiseReplay)
        mode = SEEDED if isinstance(noise_fn, SceneNoise) else REPLAY if replay else RANDN
        if mode == SEEDED and noise_fn.seeds.shape[0] != shape[0]:
            raise ValueError("SceneNoise holds %d seeds, the loop samples %d scenes" % (noise_fn.seeds.shape[0], shape[0]))
        if replay and check is not None:
            check(noise_fn)
        dtab = None if ddim is None else diff.ddim_tables(ddim[0], ddim[1], device)
        key = (tag, id(model), shape, str(device), diff.model_mean_type, mode,
               None if condition is None else (tuple(condition.shape), condition.stride(0) == 0),
               None if condition_cross is None else tuple(condition_cross.shape))
        g = diff._graphs.get(key)
        eng = model.engine(device)
        eng.params_moved()              # parameters re-homed since the capture (first training step, .to()): the engine drops its plans
        if g is None or g.plan is not eng.plans.get(_plan_key(g)):
            g = make(model, device, replay if mode != SEEDED else SEEDED)
            diff._graphs = {key: g}           # one live graph per diffusion object
        else:                                 # refresh weights + conditioning buffers
            _prepare_plans(eng, mult * shape[0], shape[1], condition, condition_cross, g.plan.time_table, len(g.plans))
        if replay:
            out = run(g, noise_fn.buffer[0], noise_fn.buffer, noise_fn.partial_buffer, dtab)
        elif mode == SEEDED:                  # x_T is main draw 0; the device generator is not touched
            out = run(g, g.seeded_x_T(noise_fn.seeds.to(device)), None, None, dtab)
        else:
            out = run(g, torch.randn(shape, dtype=torch.float, device=device), None, None, dtab)
        from ._lib import check_indices
        check_indices(name)     # DSC_CHECK_INDICES=1 (debugging; synchronises)
        return out


def _head(buffer, n):
    return None if buffer is None else buffer[:n]


def _replay_check(what, n_main, shape=None, n_partial=None, pshape=None):
    """check(noise_fn) of a front end: the NoiseReplay holds ``n_main`` main draws (of ``shape``, where the loop has always checked it)
    and, for a loop with a given part, ``n_partial`` draws of ``pshape`` for it; ValueError otherwise."""
    def check(nf):
        ok = nf.buffer.shape[0] >= n_main and (shape is None or tuple(nf.buffer.shape[1:]) == tuple(shape))
        if n_partial is not None:
            ok = ok and nf.partial_buffer is not None and nf.partial_buffer.shape[0] >= n_partial \
                and tuple(nf.partial_buffer.shape[1:]) == tuple(pshape)
        if not ok:
            raise ValueError("%s replays %d main draws%s%s" % (
                what, n_main, "" if shape is None else " of shape %s" % (tuple(shape),),
                "" if n_partial is None else " and %d draws of shape %s for the given part" % (n_partial, tuple(pshape))))
    return check


def graph_sample_loop(diff, denoise_fn, shape, device, condition, condition_cross, clip_denoised, total_steps,
                      noise_fn=torch.randn, partial_boxes=None):
    pshape = None if partial_boxes is None else tuple(partial_boxes.shape)
    out = _cached_loop(
        "graph_sample_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn, ("ddpm", bool(clip_denoised), pshape),
        lambda model, dev, replay: _StepGraph(diff, model, tuple(shape), dev, condition, condition_cross, clip_denoised, replay, pshape),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, total_steps, buf, partial_boxes, pbuf))
    if partial_boxes is not None:
        out[:, :partial_boxes.shape[1], :] = partial_boxes          # clean objects restored after the last step (:471-473)
    return out


def graph_ddim_sample_loop(diff, denoise_fn, shape, device, condition, condition_cross, sampling_timesteps, eta,
                           noise_fn=torch.randn):
    """ddim_sample_loop as replayed hipGraphs; bit-identical to the eager loop (same kernels, same draws in the same order)."""
    S = int(sampling_timesteps)
    return _cached_loop(
        "graph_ddim_sample_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn, ("ddim", S),
        lambda model, dev, replay: _DDIMGraph(diff, model, tuple(shape), dev, condition, condition_cross, S, replay),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, dtab, buf), check=_replay_check("DDIM with S = %d" % S, S), ddim=(S, eta))


def graph_complete_ragged_loop(diff, denoise_fn, shape, device, condition, condition_cross, clip_denoised, total_steps,
                               noise_fn=torch.randn, partial_boxes=None, counts=None, fused=True):
    """p_sample_loop_complete_ragged as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same
    order, the same generator state afterwards).  ``counts`` is the (B,) int64 device tensor of ops.ragged_counts.  The cache key
    holds Pmax but not the counts."""
    B, N, C = shape
    pmax = partial_boxes.shape[1]
    return _cached_loop(
        "graph_complete_ragged_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn,
        ("ragged", bool(fused), pmax, bool(clip_denoised)),
        lambda model, dev, replay: _RaggedCompleteGraph(diff, model, tuple(shape), pmax, dev, condition, condition_cross, clip_denoised,
                                                        replay, fused),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, total_steps, partial_boxes, counts, _head(buf, total_steps + 1), _head(pbuf, total_steps)),
        check=_replay_check("ragged completion", total_steps + 1, None, total_steps, (B, pmax, C)))


def graph_ddim_complete_ragged_loop(diff, denoise_fn, shape, device, condition, condition_cross, sampling_timesteps, eta,
                                    noise_fn=torch.randn, partial_boxes=None, counts=None, fused=True):
    """ddim_complete_ragged_loop as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same order,
    the same generator state afterwards).  ``counts`` is the (B,) int64 device tensor of ops.ragged_counts.  The cache key holds S and
    Pmax; it holds neither eta nor the counts."""
    B, N, C = shape
    S = int(sampling_timesteps)
    pmax = partial_boxes.shape[1]
    return _cached_loop(
        "graph_ddim_complete_ragged_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn,
        ("ddim_ragged", S, bool(fused), pmax),
        lambda model, dev, replay: _DDIMCompleteGraph(diff, model, tuple(shape), pmax, dev, condition, condition_cross, S, replay, fused),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, dtab, partial_boxes, counts, buf, pbuf),
        check=_replay_check("strided ragged completion", S, None, S, (B, pmax, C)), ddim=(S, eta))


def graph_masked_loop(diff, denoise_fn, shape, device, condition, condition_cross, clip_denoised, total_steps, noise_fn=torch.randn,
                      known=None, mask=None):
    """p_sample_loop_masked as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same order, the
    same generator state afterwards).  ``known`` (B, N, C) f32 and ``mask`` (B, N, C) uint8 (ops.known_mask) are copied into the graph's
    own buffers: the cache key holds the shape, not the mask."""
    return _cached_loop(
        "graph_masked_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn, ("masked", bool(clip_denoised)),
        lambda model, dev, replay: _MaskedGraph(diff, model, tuple(shape), dev, condition, condition_cross, clip_denoised, replay),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, total_steps, known, mask, _head(buf, total_steps + 1), _head(pbuf, total_steps)),
        check=_replay_check("the masked loop", total_steps + 1, shape, total_steps, shape))


def graph_ddim_masked_loop(diff, denoise_fn, shape, device, condition, condition_cross, sampling_timesteps, eta, noise_fn=torch.randn,
                           known=None, mask=None):
    """ddim_masked_loop as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same order, the same
    generator state afterwards).  The cache key holds the shape and S; it holds neither eta nor the mask."""
    S = int(sampling_timesteps)
    return _cached_loop(
        "graph_ddim_masked_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn, ("ddim_masked", S),
        lambda model, dev, replay: _DDIMMaskedGraph(diff, model, tuple(shape), dev, condition, condition_cross, S, replay),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, dtab, known, mask, buf, pbuf),
        check=_replay_check("the strided masked loop", S, shape, S, shape), ddim=(S, eta))


def graph_guided_loop(diff, denoise_fn, shape, device, condition, condition_cross, scale, clip_denoised, total_steps,
                      noise_fn=torch.randn, fused=True):
    """p_sample_loop_guided as a replayed hipGraph; bit-identical to the eager loop (same expressions, same draws in the same order, the
    same generator state afterwards).  ``condition`` / ``condition_cross`` arrive at 2 B (GaussianDiffusion._guided_inputs), ``scale`` is
    the (B,) f32 device vector of ops.guidance_scales: the cache key holds the shape, not the scales."""
    return _cached_loop(
        "graph_guided_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn,
        ("guided", bool(fused), bool(clip_denoised)),
        lambda model, dev, replay: _GuidedStepGraph(diff, model, tuple(shape), dev, condition, condition_cross, clip_denoised, replay,
                                                    fused),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, total_steps, scale, _head(buf, total_steps + 1)), mult=2,
        check=_replay_check("the guided loop", total_steps + 1, shape))


def graph_ddim_guided_loop(diff, denoise_fn, shape, device, condition, condition_cross, scale, sampling_timesteps, eta,
                           noise_fn=torch.randn, fused=True):
    """ddim_guided_loop as replayed hipGraphs; bit-identical to the eager loop.  The cache key holds the shape and S; it holds neither
    eta nor the scales."""
    S = int(sampling_timesteps)
    return _cached_loop(
        "graph_ddim_guided_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn, ("ddim_guided", S, bool(fused)),
        lambda model, dev, replay: _DDIMGuidedGraph(diff, model, tuple(shape), dev, condition, condition_cross, S, replay, fused),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, dtab, scale, buf), mult=2, check=_replay_check("the guided strided loop", S, shape),
        ddim=(S, eta))


def graph_masked_guided_loop(diff, denoise_fn, shape, device, condition, condition_cross, scale, clip_denoised, total_steps,
                             noise_fn=torch.randn, known=None, mask=None, fused=True):
    """p_sample_loop_masked_guided as replayed hipGraphs; bit-identical to the eager loop (same expressions, same draws in the same
    order, the same generator state afterwards).  ``condition`` / ``condition_cross`` arrive at 2 B, ``scale`` (B,) f32, ``known`` /
    ``mask`` (B, N, C) are copied into the graph's own buffers: the cache key holds the shape, neither the mask nor the scales."""
    return _cached_loop(
        "graph_masked_guided_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn,
        ("masked_guided", bool(fused), bool(clip_denoised)),
        lambda model, dev, replay: _MaskedGuidedGraph(diff, model, tuple(shape), dev, condition, condition_cross, clip_denoised, replay,
                                                      fused),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, total_steps, scale, known, mask, _head(buf, total_steps + 1), _head(pbuf, total_steps)),
        mult=2, check=_replay_check("the guided masked loop", total_steps + 1, shape, total_steps, shape))


def graph_ddim_masked_guided_loop(diff, denoise_fn, shape, device, condition, condition_cross, scale, sampling_timesteps, eta,
                                  noise_fn=torch.randn, known=None, mask=None, fused=True):
    """ddim_masked_guided_loop as replayed hipGraphs; bit-identical to the eager loop.  The cache key holds the shape and S; it holds
    neither eta, the mask nor the scales."""
    S = int(sampling_timesteps)
    return _cached_loop(
        "graph_ddim_masked_guided_loop", diff, denoise_fn, shape, device, condition, condition_cross, noise_fn,
        ("ddim_masked_guided", S, bool(fused)),
        lambda model, dev, replay: _DDIMMaskedGuidedGraph(diff, model, tuple(shape), dev, condition, condition_cross, S, replay, fused),
        lambda g, x_T, buf, pbuf, dtab: g.run(x_T, dtab, scale, known, mask, buf, pbuf), mult=2,
        check=_replay_check("the guided strided masked loop", S, shape, S, shape), ddim=(S, eta))


def _plan_key(g):
    p = g.plan
    return (p.B, p.N, p.ctx_mode, 0 if p.ctx_in is None else p.ctx_in.shape[1], p.L,
            0 if p.cross_in is None else p.cross_in.shape[1], p.time_table)        # slot 0 carries no suffix
