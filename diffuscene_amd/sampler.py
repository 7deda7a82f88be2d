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
A loop is three orthogonal parts, the axes of the one step kernel (csrc/diffusion.hip: step_kernel<STRIDED, GIVEN, GUIDED>):
  the schedule    _PosteriorLoop: T steps, t counts down by a kernel in the graph, T + 1 main draws (x_T, then one per step, also at
                  t == 0), ``final`` only beside a fused given part.  _DDIMLoop (ddim_sample_loop, :402-444): a device step counter and
                  per-pair tables (t, t_next, coefficients) owned here and refreshed in place, the advance kernel, S main draws (none on
                  the last pair), always ``final``, ``graph`` when S > 1.  Each holds the time operands of the step (``sched``), the
                  in-graph move, _start / _park and what ``run`` does before and after the replays.
  the given part  _Given (nothing), _Dense (the prefix of p_sample_loop_complete, never fused), _Ragged (a row prefix with per-scene
                  counts), _Masked (a byte mask): graph-owned buffers refreshed in place, its own noise stream -- shifted by one when
                  fused: draw 0 feeds a standalone overwrite in ``run``, the fused step re-noises for the NEXT model call, the last step
                  restores, so a given element costs no posterior step and the draw order stays the eager one --, the operands it adds
                  to the step, the unfused overwrite and restore.
  guidance        _Guidance: a plan at 2 B (text features | zeros), x kept in both halves of one (2 B, N, C) buffer (x_dup), the
                  per-scene scales in a buffer, ``m`` when unfused.
  steering        _Steer (optional, ``steer=``): the per-scene weights and the step bound K in buffers of the graph, ONE launch
                  (dsc_steer_boxes_f32) after the model call that corrects its output in place; the step kernel is the unchanged one, and
                  without it the graph is what it is today.
  multistep       _Multistep (optional, ``multistep=``, strided rows only): the x0 history and the (S,) history weights of
                  DPM-Solver++(2M) in buffers of the graph, ONE launch (dsc_multistep_x0_f32) after the steering in the replayed
                  non-final graph -- the last pair has weight 0 and needs none; the step kernel is the unchanged one.
  walls           _Walls (optional, ``walls=``): floor-plan steering -- the weights, K, the distance field of the room mask and the room
                  side in buffers of the graph, ONE launch (dsc_steer_walls_f32) after _Steer and before _Multistep.
  jumps           _Jump (optional, ``jumps=``): RePaint's resampling jumps -- the jump tables in buffers of the graph, two more graphs (``jump``:
                  the jump draw, the given draw of the next call, ONE launch dsc_resample_jump_f32, the move; ``prejump``: the step a jump
                  follows, without its given draw), replayed along the host's op list (ops.resample_schedule); j is part of the key.
_Loop has the one ``_step(final)`` -- [unfused overwrite,] model call, [steering,] [walls,] [multistep unless final,] main draw, given draw unless
final, [cfg_combine,] ONE update launch laid out by ops.step_rec from the operands of the three parts, [copy into the null half,] move unless final -- and the one ``run``.
The ten classes are rows:                    schedule   given            guided   fused=False unfuses
  _StepGraph                                 T steps    - / _Dense       -        (sub-batch chains: _chains_for, this row only)
  _DDIMGraph                                 strided    -                -
  _RaggedCompleteGraph / _DDIMCompleteGraph  T / str.   _Ragged          -        the overwrite
  _MaskedGraph / _DDIMMaskedGraph            T / str.   _Masked          -
  _GuidedStepGraph / _DDIMGuidedGraph        T / str.   -                yes      the guidance
  _MaskedGuidedGraph / _DDIMMaskedGuidedGraph  T / str. _Masked (at B)   yes      the guidance
and the graph_*_loop front ends behind diffusion_ddpm.py are one _front_end over a row: one cached graph per diffusion object
(_cached_loop).  A new loop is a new row: a class line, a front-end line, a key in ops.STEP_ENTRY if it needs a kernel instantiation of
its own, and a spec in a public method of GaussianDiffusion.
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
        return self.main_draw(size)

    def main_draw(self, size=None, dtype=None, device=None):
        """The next row of the main buffer, whatever the shapes or the call count say: also the draw of a resampling jump."""
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

    resample = prejump = jump = None         # the jump part of a _Loop and its two graphs

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
        ``kinds`` may also name the two graphs of a jump part, "prejump" and "jump" (_Loop._body), kept under those names.
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
            for kind in kinds:
                self._body(kind)
        torch.cuda.current_stream(dev).wait_stream(side)
        pool = None                             # every graph from the pool of the first one captured
        for kind in kinds:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                self._body(kind)
            pool = pool or g.pool()
            if kind is True:
                self.final = g
            elif kind is False:
                self.graph = g
            else:
                setattr(self, kind, g)
        torch.cuda.set_rng_state(rng_state, dev)
        self._park()

    def _body(self, kind):
        self._step(kind)

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
    """The T-step schedule: ``sched`` is the time source of ops.step_rec, the graph decrements t; T + 1 main draws.  ``final`` exists only
    beside a fused given part (the last step restores instead of re-noising): without one the step at t == 0 is ``graph`` too."""
    strided = False

    def __init__(self, diff, model, shape, device, condition, condition_cross, clip_denoised, replay, mult=1, nch=1):
        super().__init__(diff, model, shape, device, condition, condition_cross, replay, diff.num_timesteps + 1, mult, nch)
        self.T = self.given_draws = diff.num_timesteps
        tb = self.tb
        self.sched = dict(t=self.t[:shape[0]], clip=clip_denoised,
                          tables=(self.ca, self.cb, tb["posterior_mean_coef1"], tb["posterior_mean_coef2"], diff._sigma(tb)))

    def _kinds(self, fused_given):
        return [False, True] if fused_given else [False]

    def _capture(self, kinds):
        self.t.fill_(0 if kinds[0] == "jump" else 1)    # a warm-up that opens with the jump: 0 -> j -> j - 1, all rows of the schedule
        super()._capture(kinds)

    def _main_draw(self, final):
        return self.noise()                     # at t == 0 too

    def _move(self):
        ops.add_scalar_i64(self.t, -1)

    def _jump_time(self):
        return dict(t=self.t[:self.shape[0]])

    def _jump_move(self, j):
        ops.add_scalar_i64(self.t, j)

    def _begin(self, total_steps):
        """-> (the first timestep, the steps of this run)."""
        self.check_current()
        return total_steps - 1, total_steps

    _end = _LoopGraph._park                     # t holds -1 after the loop


class _DDIMLoop(_LoopGraph):
    """The strided schedule.  The step counter and the per-pair tables (t, t_next; sqrt(alpha_next), c, sigma) are captured by pointer:
    this object owns them and ``_load_tables`` refreshes them IN PLACE (eta is not part of the cache key), so a live graph never
    points at a freed table.  ``graph`` (S > 1 only) ends with the advance kernel (step += 1, t = times[step]) and is replayed S - 1
    times; ``final`` is the draw-free last pair ((t, -1) -> x_start), from a fresh pool when S == 1.  S main draws."""
    strided = True

    def __init__(self, diff, model, shape, device, condition, condition_cross, S, replay, mult=1):
        super().__init__(diff, model, shape, device, condition, condition_cross, replay, S, mult)
        self.S = self.given_draws = S
        self.step = torch.zeros((1,), device=device, dtype=torch.int64)
        self.times = torch.zeros((S,), device=device, dtype=torch.int64)
        self.times_next = torch.zeros((S,), device=device, dtype=torch.int64)
        self.coef = torch.zeros((3, S), device=device, dtype=torch.float32)
        self.sched = dict(strided=(self.step, self.times, self.times_next, self.coef),
                          tables=(self.ca, self.cb, self.tb["sqrt_recip_alphas_cumprod"], self.tb["sqrt_recipm1_alphas_cumprod"]))

    def _kinds(self, fused_given):
        return ([False] if self.S > 1 else []) + [True]

    def _park(self):
        super()._park()
        self.step.zero_()

    def _start(self, x_T, t0):
        self._load_x(x_T)
        self.step.zero_()
        self.t.fill_(t0)

    def _copy_rows(self, dst, src):
        dst.copy_(src[:dst.shape[0]])           # the buffers hold exactly S rows (with a jump part: the rows of its schedule)

    def _capture(self, kinds):
        if self.resample:                       # the warm-up of a jump part: [j - 1 ->] j -> 0 -> 1, all pairs of the schedule
            self.step.fill_(self.resample.j - (kinds[0] == "prejump"))
        super()._capture(kinds)

    def _main_draw(self, final):
        return self.x if final else self.noise()                # not read on the last pair

    def _move(self):
        ops.ddim_advance(self.step, self.times, self.t)

    def _jump_time(self):
        return dict(strided=(self.step, self.times))

    def _jump_move(self, j):
        ops.ddim_seek(self.step, self.times, self.t, -j)

    def _begin(self, dtab, weights=None):
        """The tables of this run into the graph's own -> (the first timestep, S).  ``weights``: the (S,) history weights of a loop
        with a multistep part."""
        pairs, times, times_next, coef = dtab
        assert len(pairs) == self.S
        self.check_current()
        self.times.copy_(times)                 # in place: the graphs hold these pointers
        self.times_next.copy_(times_next)
        self.coef.copy_(coef)
        if self.multistep:
            self.multistep.load(weights)
        return pairs[0][0], self.S

    def _end(self):
        pass


class _Given:
    """The given part of a loop, here: nothing is given.  A part keeps what is given in buffers of the graph, captured by pointer and
    refreshed in place by ``load`` -- one graph serves every value -- and has its own noise stream ``noise``.  ``fused``: the step
    kernel handles the part -- the stream is shifted by one: draw 0 feeds the standalone overwrite ``first`` in ``run``, the step re-noises
    for the NEXT model call (``operands``: what the part adds to ops.step_rec), the last step restores -- so a given element costs no
    posterior step and the draw order stays the eager one.  Not fused: ``before`` draws and overwrites in front of every model call,
    ``restore`` puts the clean values into the result.  ``values``: what ``load`` takes, by the names of the front end.
    Every method is handed the loop ``g`` and no part keeps it: a reference cycle would leave a replaced graph to the cyclic collector,
    which can run inside a later capture -- and destroying a hipGraph there aborts the process."""
    values, fused, noise = (), False, None

    def __init__(self, g, shape):
        pass

    def load(self, g):
        pass

    def first(self, g):
        pass

    def before(self, g):
        pass

    def operands(self, g, final):
        return {}

    def restore(self, g, out):
        return out

    def steer_operands(self, g):
        """What the part adds to ops.steer_rec: a given element enters the boxes with its given value and is never moved."""
        return {}

    def jump_operands(self, g):
        """What a fused part adds to ops.jump_rec: its values and the given draw of the model call the jump leads to."""
        return {}


class _Dense(_Given):
    """p_sample_loop_complete (:461-466): the first P rows of every scene, re-noised and written over x_t BEFORE the model call at every
    step.  Never fused; the front end restores the clean objects."""
    values = ("partial_boxes",)

    def __init__(self, g, shape):
        self.partial = torch.zeros(shape, device=g.device)
        self.full = torch.full((shape[0],), shape[1], device=g.device, dtype=torch.int64)      # every scene is given all P rows
        self.noise = g._stream(shape, g.given_draws, GIVEN)

    def load(self, g, partial):
        self.partial.copy_(partial)

    def steer_operands(self, g):
        return dict(rows=(self.partial, None, self.full))

    def before(self, g):
        ops.complete_overwrite(g.x, self.partial, self.noise(), g.t, *g.q)


class _Ragged(_Given):
    """Given objects as a row prefix: the padded objects (B, Pmax, C) and the (B,) int64 counts (ops.ragged_counts).  ``fused=False`` is
    the comparison of tools/bench_complete.py / bench_ddim_complete.py: every step begins with the unfused overwrite."""
    values = ("partial_boxes", "counts")

    def __init__(self, g, shape, fused=True):
        self.fused = fused
        self.partial = torch.zeros(shape, device=g.device, dtype=torch.float32)
        self.counts = torch.zeros((shape[0],), device=g.device, dtype=torch.int64)
        self.noise = g._stream(shape, g.given_draws, GIVEN)

    def load(self, g, partial, counts):
        self.partial.copy_(partial)
        self.counts.copy_(counts)

    def _overwrite(self, g, pn):
        ops.complete_overwrite_ragged(g.x, self.partial, pn, self.counts, g.t, *g.q)

    def first(self, g):
        if self.fused:
            self._overwrite(g, self.noise.head())

    def before(self, g):
        if not self.fused:
            self._overwrite(g, self.noise())

    def operands(self, g, final):                  # the partial draw is not read after the last step
        return dict(rows=(self.partial, self.partial if final else self.noise(), self.counts), q=g.q) if self.fused else {}

    def jump_operands(self, g):
        return dict(rows=(self.partial, self.noise(), self.counts), q=g.q) if self.fused else {}

    def restore(self, g, out):
        return out if self.fused else restore_given_rows(out, self.partial, self.counts)

    def steer_operands(self, g):
        return dict(rows=(self.partial, None, self.counts))


class _Masked(_Given):
    """Given elements as a byte mask: ``known`` (B, N, C) f32 and ``mask`` (B, N, C) uint8 (ops.known_mask), with full-shape known-draws;
    under guidance all three stay at B.  Always fused."""
    values, fused = ("known", "mask"), True

    def __init__(self, g, shape):
        self.known = torch.zeros(g.shape, device=g.device, dtype=torch.float32)
        self.mask = torch.zeros(g.shape, device=g.device, dtype=torch.uint8)
        self.noise = g._stream(g.shape, g.given_draws, GIVEN)

    def load(self, g, known, mask):
        self.known.copy_(known)
        self.mask.copy_(mask)

    def first(self, g):
        ops.masked_overwrite(g.x, self.known, self.noise.head(), self.mask, g.t[:g.shape[0]], *g.q)

    def operands(self, g, final):                  # the known-draw is not read after the last step
        return dict(mask=(self.known, self.known if final else self.noise(), self.mask), q=g.q)

    def jump_operands(self, g):
        return dict(mask=(self.known, self.noise(), self.mask), q=g.q)

    def steer_operands(self, g):
        return dict(mask=(self.known, None, self.mask))


class _Guidance:
    """Classifier-free guidance: the plan runs at 2 B (``mult`` = 2) -- rows [0, B) fed the text features, rows [B, 2 B) zeros -- on the
    same x and t in both halves; the fused kernels read both halves of the plan's output and write the new x to BOTH halves of ``x2``
    (their x_dup pointer).  The (B,) scale vector (ops.guidance_scales) is a buffer of the graph, captured by pointer and refreshed in
    place: one graph serves every per-scene mix of scales.  ``fused=False`` is the comparison of tools/bench_cfg.py /
    bench_guided_inpaint.py: cfg_combine into ``m``, the unguided step kernel, a copy into the null half."""

    def __init__(self, g, fused):
        self.fused = fused
        self.scale = torch.ones((g.shape[0],), device=g.device, dtype=torch.float32)
        self.m = None if fused else torch.empty(g.shape, device=g.device, dtype=torch.float32)

    def apply(self, g, mo):
        """-> (the model output of the step, what guidance adds to ops.step_rec)."""
        if self.fused:
            return mo, dict(scale=self.scale, x_dup=g.x_null)
        return ops.cfg_combine(mo, self.scale, out=self.m), {}

    def after(self, g):
        if not self.fused:
            g.x_null.copy_(g.x)


class _Steer:
    """Collision steering (dsc_steer_boxes_f32): one launch between the model call and the step that corrects the model output in place,
    on what the model call returned -- under guidance the 2 B output, with the scales, so the fused and the unfused guidance see the same
    corrected halves.  ``weight`` (B,) f32 and ``t_below`` (1,) int64 are buffers of the graph, captured by pointer and refreshed in
    place: one graph serves every per-scene weight and every number of steered steps, and a weight of 0 or a timestep at or above
    t_below stores nothing.  ``layout`` = (bounds, bbox_dim, class_dim) is baked into the launch and part of the cache key.
    The base of every steering part: ``key`` and ``loaded`` split the inputs tuple of the loop (GaussianDiffusion._steer_inputs) into
    the layout and what ``load`` takes.  A part with further buffers hands them to __init__ as ``more``, in the order of its record's
    tuple, and extends ``key``, ``loaded``, ``load`` and ``_rec``."""

    def __init__(self, g, layout, more=()):
        bounds, bbox_dim, class_dim = layout
        self.weight = torch.zeros((g.shape[0],), device=g.device, dtype=torch.float32)
        self.t_below = torch.zeros((1,), device=g.device, dtype=torch.int64)
        self.spec = (self.weight, self.t_below, ops.steer_bounds(bounds), bbox_dim, class_dim) + more

    @staticmethod
    def key(inputs):
        weight, k, bounds, bbox_dim, class_dim = inputs
        return tuple(float(v) for v in bounds), int(bbox_dim), int(class_dim)

    @staticmethod
    def loaded(inputs):
        weight, k, bounds, bbox_dim, class_dim = inputs
        return weight, k

    def load(self, weight, t_below):
        self.weight.copy_(weight)               # in place: the graph holds these pointers
        self.t_below.fill_(int(t_below))

    def apply(self, g, mo):
        scale = dict(scale=g.guide.scale) if g.guide else {}
        ops.issue(self._rec(g.x, mo, g.mean_type, **g.sched, **g.part.steer_operands(g), **scale))

    def _rec(self, *args, **operands):
        return ops.steer_rec(*args, steer=self.spec, **operands)


class _Walls(_Steer):
    """Floor-plan steering (dsc_steer_walls_f32): one launch after collision steering (if any) and before the multistep launch, on
    the same output with the same operands as _Steer -- walls have the last word.  ``weight`` (B,) f32, ``t_below`` (1,) int64, ``field``
    (B, H, W) f32 and ``room_side`` (1,) f32 are buffers of the graph, captured by pointer and refreshed in place: one graph serves
    every mask, room side, per-scene weight and number of steered steps.  The field comes from ops.floor_field, once per call; a shared
    (1, H, W) field is broadcast into the buffer.  ``layout`` = (bounds, bbox_dim, class_dim, H, W) is baked into the launch and part
    of the cache key."""

    def __init__(self, g, layout):
        *steer, h, w = layout
        self.field = torch.zeros((g.shape[0], h, w), device=g.device, dtype=torch.float32)
        self.room_side = torch.ones((1,), device=g.device, dtype=torch.float32)
        super().__init__(g, steer, (self.field, self.room_side))

    @staticmethod
    def key(inputs):
        *steer, field, room_side = inputs
        return _Steer.key(steer) + tuple(field.shape[1:])

    @staticmethod
    def loaded(inputs):
        *steer, field, room_side = inputs
        return _Steer.loaded(steer) + (field, room_side)

    def load(self, weight, t_below, field, room_side):
        super().load(weight, t_below)
        self.field.copy_(field)                 # (B, H, W), or (1, H, W) broadcast
        self.room_side.fill_(float(room_side))

    def _rec(self, *args, **operands):
        return ops.walls_rec(*args, walls=self.spec, **operands)


class _Multistep:
    """DPM-Solver++(2M) (dsc_multistep_x0_f32): one launch after the model call and the steering that moves the model output -- under
    guidance the 2 B output, with the scales -- so that the unchanged strided step runs on the extrapolated x0 estimate, and keeps the
    clamped x0 of the pair in ``hist``.  ``hist`` (B, N, C) and ``weights`` (S,) f32 are buffers of the graph, captured by pointer; the
    weights are refreshed in place by _DDIMLoop._begin.  The first pair has weight 0 and does not read ``hist``, so nothing carries
    over from one run to the next; the last pair has weight 0 and writes no history: ``final`` holds no launch."""

    def __init__(self, g):
        self.hist = torch.zeros(g.shape, device=g.device, dtype=torch.float32)
        self.weights = torch.zeros((g.S,), device=g.device, dtype=torch.float32)

    def load(self, weights):
        self.weights.copy_(weights)             # in place: the graph holds this pointer

    def apply(self, g, mo):
        scale = dict(scale=g.guide.scale) if g.guide else {}
        ops.issue(ops.multistep_rec(g.x, mo, self.hist, self.weights, g.mean_type, **g.sched, **g.part.steer_operands(g), **scale))


class _Jump:
    """Resampling jumps (RePaint; INTEGRATION.md 9, dsc_resample_jump_f32).  ``j`` is baked into the launch and the move and part of the
    cache key; the tables ``ja`` / ``jb`` (T rows, or S of a strided loop) are buffers of the graph refreshed in place; r and K are host
    control -- ``run`` replays along the op list of ops.resample_schedule, so one graph set serves every (r, K).  Two more graphs:
      jump     the jump draw (main stream), the given draw of the model call at s + j where the given part is fused, ONE launch -- the
               jump of the free elements and the re-noising of the given ones at time(s + j), both halves of a guided state --, the move
               (t += j; strided: step -= j, t = times[step]);
      prejump  beside a fused given part, the step that a jump follows: the step without its given draw -- the jump makes the one the
               next model call needs, and writes every given element, so what this step leaves there is never read.
    ``rows`` = (main rows, given rows) of the replay buffers, from the schedule's counts (replay mode only: then part of the key)."""

    def __init__(self, g, j):
        self.j = int(j)
        rows = g.S if g.strided else g.T
        self.ja = torch.ones((rows,), device=g.device, dtype=torch.float32)
        self.jb = torch.zeros((rows,), device=g.device, dtype=torch.float32)

    def load(self, tables):
        self.ja.copy_(tables[0])                # in place: the graph holds these pointers
        self.jb.copy_(tables[1])

    def apply(self, g):
        noise = g.noise()
        ops.issue(ops.jump_rec(g.x, noise, self.ja, self.jb, self.j, **g._jump_time(), **g.part.jump_operands(g), x_dup=g.x_null))
        g._jump_move(self.j)


class _Loop:
    """One captured loop = a schedule (_PosteriorLoop or _DDIMLoop, by inheritance), a given part and guidance: the row a class below
    declares.  ``sched``: clip_denoised of a T-step loop, S of a strided one.  ``fused`` unfuses what the row has a kernel for: the
    overwrite of a ragged part, the guidance of a guided row.  ``partial_shape``: the shape of the given rows."""
    given, guided, chains, what, multistep = _Given, False, False, None, None

    def __init__(self, diff, model, shape, device, condition, condition_cross, sched, replay=False, fused=True, partial_shape=None,
                 steer=None, multistep=False, walls=None, resample=None):
        nch = (_chains_for(shape[0]),) if self.chains and resample is None else ()     # a loop with a jump part runs as one chain
        super().__init__(diff, model, shape, device, condition, condition_cross, sched, replay, 2 if self.guided else 1, *nch)
        self.fused = fused
        if resample is not None and self.replay:                # (j, main rows, given rows): the replay buffers follow the schedule
            self.noise = self._stream(shape, resample[1])
            self.given_draws = resample[2]
        self.side = [torch.cuda.Stream(device=device) for _ in range(len(self.plans) - 1)]
        self.model_out = torch.empty(shape, device=device, dtype=torch.float32) if self.side else None
        part = self.given if self.given is not _Dense or partial_shape is not None else _Given
        self.part = part(self, partial_shape, fused) if part is _Ragged else part(self, partial_shape)
        self.guide = _Guidance(self, fused) if self.guided else None
        self.steer = _Steer(self, steer) if steer is not None else None
        self.walls = _Walls(self, walls) if walls is not None else None
        if multistep and not self.strided:
            raise ValueError("a multistep solver rides on the strided loops")
        self.multistep = _Multistep(self) if multistep else None
        if resample is not None and multistep:
            raise ValueError("resampling jumps do not combine with a multistep solver")
        self.resample = _Jump(self, resample[0]) if resample is not None else None
        for owner in (self.part, self.guide):   # the buffers, by the names tests, tools and bench.py read
            for name in ("partial", "counts", "known", "mask", "scale", "m"):
                if hasattr(owner, name):
                    setattr(self, name, getattr(owner, name))
        kinds = self._kinds(self.part.fused)
        if self.resample:                       # the jump graphs first: the warm-up then stays on rows of the schedule (_capture)
            kinds = (["prejump"] if self.part.fused else []) + ["jump"] + kinds
        self._capture(kinds)

    def _body(self, kind):
        if kind == "jump":
            self.resample.apply(self)
        elif kind == "prejump":
            self._step(False, given_draw=False)
        else:
            self._step(kind)

    def _model_call(self):
        """One plan, or the sub-batch chains of _chains_for: chain 0 on the current stream, the others on side streams."""
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

    def _step(self, final, given_draw=True):
        """``given_draw=False``: the step a jump follows (_Jump).
        [the unfused overwrite,] model call, [collision steering,] [floor-plan steering,] [the multistep launch unless final,] main
        draw, the given draw of the NEXT step unless final,
        [cfg_combine,] one update launch, [the copy into the null half,] decrement or advance unless final."""
        self.part.before(self)
        mo = self._model_call()
        if self.steer:
            self.steer.apply(self, mo)
        if self.walls:
            self.walls.apply(self, mo)
        if self.multistep and not final:
            self.multistep.apply(self, mo)
        noise = self._main_draw(final)
        given = self.part.operands(self, final or not given_draw)
        mo, guided = self.guide.apply(self, mo) if self.guide else (mo, {})
        ops.issue(ops.step_rec(self.x, mo, noise, self.x, self.mean_type, **self.sched, **given, **guided))
        if self.guide:
            self.guide.after(self)
        if not final:
            self._move()

    def _replays_along(self, op_list):
        """One loop along the op list of ops.resample_schedule: a call is ``final`` at u == 0 where the class has one, ``prejump`` where a
        jump follows and the given part is fused, else ``graph``; a jump is ``jump``."""
        for i, (op, u) in enumerate(op_list):
            if op == "jump":
                self.jump.replay()
            elif u == 0 and self.final is not None:
                self.final.replay()
            elif self.prejump is not None and i + 1 < len(op_list) and op_list[i + 1][0] == "jump":
                self.prejump.replay()
            else:
                self.graph.replay()
        return self.x.clone()

    def run(self, x_T, sched, *values, noise_buffer=None, given_noise=None, partial=None, steer=None, multistep=None, walls=None,
            jumps=None):
        """``sched``: total_steps of a T-step loop, the device tables (GaussianDiffusion.ddim_tables) of a strided one.  ``values``: the
        (B,) scales of a guided row, then what the given part loads (``partial``: the dense prefix by keyword).  ``multistep``: the
        (S,) history weights of a loop with a multistep part.  ``jumps`` = (schedule, (ja, jb)) of a loop with a jump part."""
        t0, steps = self._begin(sched, *(() if self.multistep is None else (multistep,)))
        self._start(x_T, t0)
        if partial is not None:
            values += (partial,)
        if self.guide:
            self.guide.scale.copy_(values[0])   # in place: the graph holds this pointer
            values = values[1:]
        self.part.load(self, *values)
        if self.steer:
            self.steer.load(*steer)             # (weight (B,), K): steered while t < K
        if self.walls:
            self.walls.load(*walls)             # (weight (B,), K, field, room_side)
        if self.resample:
            self.resample.load(jumps[1])
        self._upload((self.noise, noise_buffer, 1), *([(self.part.noise, given_noise, 1 if self.part.fused else 0)] if self.part.noise else []))
        self.part.first(self)
        if self.part.fused and self.x_null is not None:         # guided: both halves of the state stay current
            self.x_null.copy_(self.x)
        out = self.part.restore(self, self._replays_along(jumps[0].ops) if self.resample else self._replays(steps))
        self._end()
        return out


# The ten loops: schedule (the base), given part, guidance; ``what`` names the loop in the refusal of a short replay buffer.
class _StepGraph(_Loop, _PosteriorLoop):        # p_sample_loop; with partial_shape p_sample_loop_complete.  No ``final``.
    given, chains = _Dense, True


class _DDIMGraph(_Loop, _DDIMLoop):             # ddim_sample_loop, strided re-arrangement on the sub-shape
    what = "DDIM with S = %d"


class _RaggedCompleteGraph(_Loop, _PosteriorLoop):              # p_sample_loop_complete_ragged
    given, what = _Ragged, "ragged completion"


class _DDIMCompleteGraph(_Loop, _DDIMLoop):     # ddim_complete_ragged_loop: 2 S draws, the last pair makes the partial draw only
    given, what = _Ragged, "strided ragged completion"


class _MaskedGraph(_Loop, _PosteriorLoop):      # p_sample_loop_masked
    given, what = _Masked, "the masked loop"


class _DDIMMaskedGraph(_Loop, _DDIMLoop):       # ddim_masked_loop
    given, what = _Masked, "the strided masked loop"


class _GuidedStepGraph(_Loop, _PosteriorLoop):  # p_sample_loop_guided
    guided, what = True, "the guided loop"


class _DDIMGuidedGraph(_Loop, _DDIMLoop):       # ddim_guided_loop
    guided, what = True, "the guided strided loop"


class _MaskedGuidedGraph(_Loop, _PosteriorLoop):                # p_sample_loop_masked_guided
    given, guided, what = _Masked, True, "the guided masked loop"


class _DDIMMaskedGuidedGraph(_Loop, _DDIMLoop):                 # ddim_masked_guided_loop
    given, guided, what = _Masked, True, "the guided strided masked loop"


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


def _front_end(name, cls):
    """graph_*_loop of one row: the loop as replayed hipGraphs, bit-identical to the eager loop (same expressions, same draws in the same
    order, the same generator state afterwards).  Called as (diff, denoise_fn, shape, device, condition, condition_cross, [scale,]
    clip_denoised, total_steps -- a strided row: sampling_timesteps, eta --, noise_fn=torch.randn, [the given values,] [fused=True]):
    ``scale`` the (B,) f32 device vector of ops.guidance_scales under conditions at 2 B (GaussianDiffusion._guided_inputs), ``counts`` the
    (B,) int64 device tensor of ops.ragged_counts, ``known`` / ``mask`` those of _masked_inputs.  The cache key holds the class,
    clip_denoised or S, ``fused`` and the shape of the given rows -- never eta, counts, mask or scales, which live in buffers.
    ``steer`` (keyword; None: the loop and its graph as they are without it) = (weight (B,) f32 on the device, K, bounds, bbox_dim,
    class_dim) of GaussianDiffusion._steer_inputs: collision steering (_Steer) after every model call; the key gains the layout -- the
    bounds and the two dims --, never the weights or K.
    ``multistep`` (keyword, strided rows; None: the loop and its graph as they are without it) = the (S,) f32 history weights of
    GaussianDiffusion.multistep_table on the device: DPM-Solver++(2M) (_Multistep) after the steering of every pair but the last; the key
    gains the flag, never the weights.
    ``walls`` (keyword; None: the loop and its graph as they are without it) = (weight (B,) f32 on the device, K, bounds, bbox_dim,
    class_dim, field (B or 1, H, W) f32 on the device, room_side) of GaussianDiffusion._wall_inputs: floor-plan steering (_Walls) after
    the collision steering; the key gains the layout and (H, W) -- never the weights, K, the mask or room_side."""
    names = (("scale",) if cls.guided else ()) + (("sampling_timesteps", "eta") if cls.strided else ("clip_denoised", "total_steps")) \
        + ("noise_fn",) + cls.given.values + (("fused",) if cls.guided or cls.given is _Ragged else ())

    def loop(diff, denoise_fn, shape, device, condition, condition_cross, *args, steer=None, multistep=None, walls=None, jumps=None,
             **kw):
        if multistep is not None and not cls.strided:
            raise ValueError("%s: a multistep solver rides on the strided loops" % name)
        if jumps is not None and multistep is not None:
            raise ValueError("%s: resampling jumps do not combine with a multistep solver" % name)
        if len(args) > len(names) or not set(kw) <= set(names[len(args):]):
            raise TypeError("%s(diff, denoise_fn, shape, device, condition, condition_cross, %s)" % (name, ", ".join(names)))
        a = dict(dict.fromkeys(names), noise_fn=torch.randn, fused=True)
        a.update(zip(names, args), **kw)
        given = [a[v] for v in cls.given.values if a[v] is not None]
        gshape = None if not given or cls.given is _Masked else (shape[0], given[0].shape[1], shape[2]) if cls.given is _Ragged \
            else tuple(given[0].shape)
        if cls.strided:
            sched = n_main = n_given = int(a["sampling_timesteps"])
        else:
            sched, n_main, n_given = bool(a["clip_denoised"]), a["total_steps"] + 1, a["total_steps"]
        total = None if cls.strided else n_given
        jump_key = jump_spec = None
        if jumps is not None:                   # (schedule, (ja, jb) on the device, j): the buffers follow the schedule's counts
            js = jumps[0]
            n_main, n_given = js.calls + js.jumps + (0 if cls.strided else 1), js.calls
            jump_spec = (int(jumps[2]), n_main, n_given)
            jump_key = ("resample",) + (jump_spec if isinstance(a["noise_fn"], NoiseReplay) else jump_spec[:1])
        # of either inputs tuple the layout is the key and the rest lives in buffers: _Steer.key / .loaded, _Walls.key / .loaded
        layout = None if steer is None else _Steer.key(steer)
        wall_layout = None if walls is None else _Walls.key(walls)
        what = cls.what or (jumps is not None and "the resampled T-step loop") or None
        check = what and _replay_check((what % sched if "%" in what else what) + (" with resampling jumps" if jumps is not None and cls.what else ""), n_main,
                                           shape if cls.guided or cls.given is _Masked else None, *((n_given, gshape or shape) if given else ()))
        out = _cached_loop(
            name, diff, denoise_fn, shape, device, condition, condition_cross, a["noise_fn"],
            (cls.__name__, sched, bool(a["fused"]), gshape) + (() if steer is None else (layout,))
            + (() if multistep is None else ("multistep",)) + (() if walls is None else (("walls",) + wall_layout,))
            + (() if jumps is None else (jump_key,)),
            lambda model, dev, replay: cls(diff, model, tuple(shape), dev, condition, condition_cross, sched, replay, a["fused"], gshape,
                                           layout, multistep is not None, *(() if walls is None else (wall_layout,)),
                                           **({} if jumps is None else dict(resample=jump_spec))),
            lambda g, x_T, buf, pbuf, dtab: g.run(x_T, dtab if cls.strided else total, *([a["scale"]] if cls.guided else []), *given,
                                                  noise_buffer=_head(buf, n_main), given_noise=_head(pbuf, n_given),
                                                  steer=None if steer is None else _Steer.loaded(steer), multistep=multistep,
                                                  **({} if walls is None else dict(walls=_Walls.loaded(walls))),
                                                  **({} if jumps is None else dict(jumps=jumps[:2]))),
            mult=2 if cls.guided else 1, check=check or None, ddim=(sched, a["eta"]) if cls.strided else None)
        if cls.given is _Dense and given:
            out[:, :gshape[1], :] = given[0]            # clean objects restored after the last step (:471-473)
        return out
    loop.__name__ = loop.__qualname__ = name
    return loop


def _head(buffer, n):
    return None if buffer is None else buffer[:n]


# module attributes on purpose: diffusion_ddpm.py looks a front end up by name at call time
graph_sample_loop = _front_end("graph_sample_loop", _StepGraph)         # (..., partial_boxes=None): with it, p_sample_loop_complete
graph_ddim_sample_loop = _front_end("graph_ddim_sample_loop", _DDIMGraph)
graph_complete_ragged_loop = _front_end("graph_complete_ragged_loop", _RaggedCompleteGraph)
graph_ddim_complete_ragged_loop = _front_end("graph_ddim_complete_ragged_loop", _DDIMCompleteGraph)
graph_masked_loop = _front_end("graph_masked_loop", _MaskedGraph)
graph_ddim_masked_loop = _front_end("graph_ddim_masked_loop", _DDIMMaskedGraph)
graph_guided_loop = _front_end("graph_guided_loop", _GuidedStepGraph)
graph_ddim_guided_loop = _front_end("graph_ddim_guided_loop", _DDIMGuidedGraph)
graph_masked_guided_loop = _front_end("graph_masked_guided_loop", _MaskedGuidedGraph)
graph_ddim_masked_guided_loop = _front_end("graph_ddim_masked_guided_loop", _DDIMMaskedGuidedGraph)


def _plan_key(g):
    p = g.plan
    return (p.B, p.N, p.ctx_mode, 0 if p.ctx_in is None else p.ctx_in.shape[1], p.L,
            0 if p.cross_in is None else p.cross_in.shape[1], p.time_table)        # slot 0 carries no suffix
