"""Fused clip + Adam for train_on_batch (reference: torch.nn.utils.clip_grad_norm_ at
diffusion_scene_layout_ddpm.py:465 and torch.optim.Adam from networks/__init__.py:29-30).

``FusedAdam`` IS a ``torch.optim.Adam`` (same constructor, ``param_groups``, ``state`` layout and ``state_dict`` format, so
``opt_XXXXX`` checkpoints are interchangeable with the reference's), but ``step()`` runs csrc/optim.hip: one sweep for the
global gradient norm, a device-side clip coefficient, one Adam sweep -- no host synchronisation, ~32 B/parameter of traffic.

Weight EMA (the average DDPM recipes sample from): ``FusedAdam(..., ema_decay=d)`` keeps it inside the Adam sweep (8 B/parameter
more, no extra launch) as ``state[p]["ema"]`` and exchanges it with the weights IN PLACE (``ema_swap`` / ``ema_weights``), so the
engine, its plans and the captured sampling graphs keep their pointers and only re-derive their weights.  ``ParamEMA`` is the same
average for any other optimizer; ``ema_model_state`` turns a model + optimizer (or ``opt_XXXXX`` dict) into the averaged
``state_dict``.  Everything is off with ``ema_decay=None``.
"""

import contextlib
import math
import warnings

import numpy as np
import torch

from . import _lib

CHUNK = 32768

_WEIGHTS_EPOCH = [0]


def weights_epoch():
    """Counter bumped by every raw-pointer parameter update of this module (part of DenoiserEngine's signature)."""
    return _WEIGHTS_EPOCH[0]


def _bump_weights_epoch():
    _WEIGHTS_EPOCH[0] += 1


def _check_ema_decay(decay):
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 <= float(decay) < 1.0):     # (nan fails the range)
        raise ValueError("ema_decay must be a float in [0, 1), got %r" % (decay,))
    return float(decay)


def ema_decay_at(decay, warmup, k):
    """Decay of EMA update ``k`` (k = updates already made, from 0): ``decay``, or with warm-up ``min(decay, (1 + k) / (10 + k))``
    -- in double, on the host."""
    return min(float(decay), (1.0 + k) / (10.0 + k)) if warmup else float(decay)


def _chunk_layout(numel):
    """Cut tensors of ``numel`` elements into chunks of <= CHUNK: (tensor index, element offset, count) of every chunk."""
    numel = np.asarray(numel, dtype=np.int64)
    nch = (numel + CHUNK - 1) // CHUNK
    tix = np.repeat(np.arange(len(numel)), nch)
    first = np.concatenate([[0], np.cumsum(nch)[:-1]])
    off = (np.arange(int(nch.sum())) - np.repeat(first, nch)) * CHUNK
    return tix, off, np.minimum(CHUNK, numel[tix] - off)


def _check_ema_tensor(p, what):
    if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
        raise RuntimeError("%s: parameters must be contiguous float32 GPU tensors (no CPU fallback)" % what)


def _ema_tables(ps, es):
    """Device work list of dsc_ema_update_f32 / dsc_ema_swap_f32 over parameters ``ps`` and their averages ``es``: the chunk table
    (param and count filled in, the entries those two kernels read) and the parallel array of average addresses."""
    tix, off, cnt = _chunk_layout([p.numel() for p in ps])
    table = np.zeros((len(tix), 5), dtype=np.int64)
    table[:, 0] = np.array([p.data_ptr() for p in ps], dtype=np.int64)[tix] + off * 4
    table[:, 4] = cnt
    eptr = np.array([e.data_ptr() for e in es], dtype=np.int64)[tix] + off * 4
    dev = ps[0].device
    return torch.from_numpy(table).to(dev), torch.from_numpy(eptr).to(dev)


def _ema_exchange(ps, tables):
    """Swap parameters ``ps`` and their averages in place (bit patterns) over the work lists ``tables`` = [(chunk table, average
    addresses)], and tell autograd and the engines that the weights changed: pointers do not move, so plans and captured graphs stay
    valid and DenoiserEngine.refresh re-derives what it caches."""
    for table, eptr in tables:
        dev = table.device
        with torch.cuda.device(dev):
            _lib.check(_lib.fn("dsc_ema_swap_f32")(table.data_ptr(), eptr.data_ptr(), table.shape[0],
                                                   torch.cuda.current_stream(dev).cuda_stream), "dsc_ema_swap_f32")
    if ps:
        torch.autograd.graph.increment_version(list(ps))
    _bump_weights_epoch()


class ParamEMA:
    """Exponential moving average of ``params`` for any optimizer: call ``update()`` after every ``optimizer.step()``.  One shadow
    tensor per parameter, made as a copy of the parameter when the object is built (so the first update averages the weights before
    and after the first step, as FusedAdam's does); ``swap()`` / ``weights()`` exchange weights and average in place (see
    ``FusedAdam.ema_swap``)."""

    def __init__(self, params, decay, warmup=False):
        self.decay = _check_ema_decay(decay)
        self.warmup = bool(warmup)
        self.params = [p for p in params]
        self.shadow = [p.detach().clone().contiguous() for p in self.params]
        self.num_updates = 0
        self.swapped = False
        self._tables = None           # (parameter pointers, chunk table, average addresses)

    def _work_list(self):
        for p in self.params:
            _check_ema_tensor(p, "ParamEMA")
        if self.num_updates == 0 and not self.swapped and any(e.device != p.device for e, p in zip(self.shadow, self.params)):
            self.shadow = [p.detach().clone() for p in self.params]       # the model moved to its device after this object was built
        ptrs = [p.data_ptr() for p in self.params]
        if self._tables is None or self._tables[0] != ptrs:
            for e, p in zip(self.shadow, self.params):
                if e.device != p.device or e.shape != p.shape:
                    raise RuntimeError("ParamEMA: a parameter changed its device or shape after the average was started")
            self._tables = (ptrs,) + _ema_tables(self.params, self.shadow)
        return self._tables[1], self._tables[2]

    @torch.no_grad()
    def update(self):
        if self.swapped:
            raise RuntimeError("ParamEMA.update() while the average is swapped in: swap back first")
        if not self.params:
            return
        table, eptr = self._work_list()
        d = ema_decay_at(self.decay, self.warmup, self.num_updates)
        dev = table.device
        with torch.cuda.device(dev):
            _lib.check(_lib.fn("dsc_ema_update_f32")(table.data_ptr(), eptr.data_ptr(), table.shape[0], d,
                                                     torch.cuda.current_stream(dev).cuda_stream), "dsc_ema_update_f32")
        self.num_updates += 1

    @torch.no_grad()
    def swap(self):
        if self.params:
            _ema_exchange(self.params, [self._work_list()])
        self.swapped = not self.swapped

    @contextlib.contextmanager
    def weights(self):
        """``with ema.weights():`` the parameters hold the average inside, the raw weights again after (also after an exception)."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def state_dict(self):
        if self.swapped:
            raise RuntimeError("ParamEMA.state_dict() while the average is swapped in: swap back first")
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates,
                "shadow": [e.clone() for e in self.shadow]}

    def load_state_dict(self, sd):
        if self.swapped:
            raise RuntimeError("ParamEMA.load_state_dict() while the average is swapped in: swap back first")
        self.num_updates = int(sd["num_updates"])
        if len(sd["shadow"]) != len(self.params):
            raise ValueError("ParamEMA: %d averages for %d parameters" % (len(sd["shadow"]), len(self.params)))
        self.shadow = [e.detach().to(device=p.device, dtype=p.dtype).clone().contiguous() for e, p in zip(sd["shadow"], self.params)]
        self._tables = None


def ema_model_state(model, optimizer):
    """``model.state_dict()`` (cloned) with every trainable parameter replaced by its average; buffers and frozen parameters as they
    are.  ``optimizer`` is a live ``FusedAdam(ema_decay=...)``, an optimizer carrying a ``ParamEMA`` as ``.ema``, a ``ParamEMA``, or the
    dict of an ``opt_XXXXX`` checkpoint.  The i-th optimizer parameter is the i-th of ``filter(requires_grad, model.parameters())``,
    the order the training script hands them to ``optimizer_factory``.  Works on CPU."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    if getattr(optimizer, "ema_swapped", False) or getattr(optimizer, "swapped", False) or \
            getattr(getattr(optimizer, "ema", None), "swapped", False):
        raise RuntimeError("ema_model_state while the average is swapped in: the model holds it already")
    if isinstance(optimizer, dict):
        ids = [i for g in optimizer["param_groups"] for i in g["params"]]
        avgs = [optimizer["state"].get(i, {}).get("ema") for i in ids]
    elif isinstance(optimizer, ParamEMA) or isinstance(getattr(optimizer, "ema", None), ParamEMA):
        ema = optimizer if isinstance(optimizer, ParamEMA) else optimizer.ema
        avgs = list(ema.shadow)
    else:
        avgs = [optimizer.state.get(p, {}).get("ema") for g in optimizer.param_groups for p in g["params"]]
    if len(avgs) != len(named):
        raise ValueError("ema_model_state: the optimizer holds %d parameters, the model has %d trainable ones" % (len(avgs), len(named)))
    out = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for (n, p), e in zip(named, avgs):
        if e is None:
            raise ValueError("ema_model_state: parameter %r has no average (no EMA update yet, or a checkpoint saved without ema_decay)" % n)
        if tuple(e.shape) != tuple(p.shape):
            raise ValueError("ema_model_state: the average of %r has shape %s, the parameter %s" % (n, tuple(e.shape), tuple(p.shape)))
        out[n] = e.detach().to(device=out[n].device, dtype=out[n].dtype).clone()
    return out


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, ema_decay=None,
                 ema_warmup=False):
        if amsgrad:
            raise NotImplementedError("amsgrad")
        # attributes, not param_groups keys: the groups (and opt_XXXXX's "param_groups") stay those of torch.optim.Adam
        self.ema_decay = None if ema_decay is None else _check_ema_decay(ema_decay)
        if ema_warmup and self.ema_decay is None:
            raise ValueError("ema_warmup needs an ema_decay")
        self.ema_warmup = bool(ema_warmup)
        self.ema_swapped = False
        self._ema_steps = {}      # id(param) -> EMA updates made (materialised into state['ema_step'] lazily)
        self._swap_tables = None  # (pointers, work lists of ema_swap)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._plans = {}          # group index -> cached chunk plan
        self._steps = {}          # id(param) -> int step count (materialised into state['step'] lazily)
        self._active_cache = {}   # id(group) -> (fingerprint, validated parameter list)

    # ---- state compatibility with torch.optim.Adam -------------------------------------------------------------
    def _sync_step_tensors(self):
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st is not None and id(p) in self._steps:
                    st["step"] = torch.tensor(float(self._steps[id(p)]), dtype=torch.float32)
                if st is not None and "ema" in st and id(p) in self._ema_steps:
                    st["ema_step"] = torch.tensor(float(self._ema_steps[id(p)]), dtype=torch.float32)

    def _refuse_swapped(self, what):
        if self.ema_swapped:
            raise RuntimeError("FusedAdam.%s while the EMA weights are swapped in (ema_swap / ema_weights): swap back first" % what)

    def state_dict(self):
        self._refuse_swapped("state_dict()")         # it would save the average as the weights' optimizer state
        self._sync_step_tensors()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self._refuse_swapped("load_state_dict()")
        super().load_state_dict(state_dict)
        self._steps = {}
        self._ema_steps = {}
        self._plans = {}
        self._active_cache = {}
        dropped = 0
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st is not None and "step" in st:
                    self._steps[id(p)] = int(float(st["step"]))
                if st is None or not ("ema" in st or "ema_step" in st):
                    continue
                if self.ema_decay is None or "ema" not in st:
                    dropped += "ema" in st
                    st.pop("ema", None)
                    st.pop("ema_step", None)
                else:
                    self._ema_steps[id(p)] = int(float(st.get("ema_step", 0.0)))
                    st["ema_step"] = torch.tensor(float(self._ema_steps[id(p)]), dtype=torch.float32)
                    if not st["ema"].is_contiguous():
                        st["ema"] = st["ema"].contiguous()
        if dropped:
            warnings.warn("FusedAdam(ema_decay=None): the checkpoint carries a weight EMA for %d parameter(s); it is dropped "
                          "(construct the optimizer with ema_decay to keep it)" % dropped)

    # ---- work lists -------------------------------------------------------------------------------------------------
    def _active(self, group):
        ps = [p for p in group["params"] if p.grad is not None]
        # validated once per (parameter set, storage): the 442-parameter loop below costs ~0.3 ms of host time per call, and
        # step() runs while the GPU waits for the Adam launch
        fast = (len(ps), ps[0].data_ptr() if ps else 0, ps[-1].data_ptr() if ps else 0, ps[0].grad.data_ptr() if ps else 0)
        cached = self._active_cache.get(id(group))
        if cached is not None and cached[0] == fast and all(a is b for a, b in zip(cached[1], ps)):
            return ps
        for p in ps:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("FusedAdam: parameters must be contiguous float32 GPU tensors (no CPU fallback)")
            if p.grad.is_sparse:
                raise RuntimeError("FusedAdam does not support sparse gradients")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                self._steps.setdefault(id(p), 0)
            elif id(p) not in self._steps:
                self._steps[id(p)] = int(float(st["step"]))
            if self.ema_decay is not None and "ema" not in st:      # the average starts as the parameter before its first update
                st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
                st["ema_step"] = torch.tensor(0.0, dtype=torch.float32)
                self._ema_steps[id(p)] = 0
        self._active_cache[id(group)] = (fast, list(ps))
        return ps

    def _plan(self, gi, ps):
        key = tuple(id(p) for p in ps)
        plan = self._plans.get(gi)
        if plan is None or plan["key"] != key or any(pp != p.data_ptr() for pp, p in zip(plan["pptr"], ps)):
            tix, off, cnt = _chunk_layout([p.numel() for p in ps])
            pptr = np.array([p.data_ptr() for p in ps], dtype=np.int64)
            mptr = np.array([self.state[p]["exp_avg"].data_ptr() for p in ps], dtype=np.int64)
            vptr = np.array([self.state[p]["exp_avg_sq"].data_ptr() for p in ps], dtype=np.int64)
            table = np.zeros((len(tix), 5), dtype=np.int64)
            table[:, 0] = pptr[tix] + off * 4
            table[:, 2] = mptr[tix] + off * 4
            table[:, 3] = vptr[tix] + off * 4
            table[:, 4] = cnt
            dev = ps[0].device
            edev = None
            if self.ema_decay is not None:      # parallel array of the averages' addresses (dsc_adam_ema_step_f32)
                eptr = np.array([self.state[p]["ema"].data_ptr() for p in ps], dtype=np.int64)
                edev = torch.from_numpy(eptr[tix] + off * 4).to(dev)
            plan = {"key": key, "pptr": pptr.tolist(), "tix": tix, "off4": off * 4, "table": table, "edev": edev,
                    "host": torch.empty((len(tix), 5), dtype=torch.int64).pin_memory(),
                    "dev": torch.empty((len(tix), 5), dtype=torch.int64, device=dev),
                    "partial": torch.empty((len(tix),), dtype=torch.float64, device=dev),
                    "norm": torch.zeros((), dtype=torch.float32, device=dev),
                    "coef": torch.ones((), dtype=torch.float32, device=dev), "gptr": None, "uploaded": None}
            self._plans[gi] = plan
        for p in ps:
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
        gptr = np.array([p.grad.data_ptr() for p in ps], dtype=np.int64)
        if plan.get("gptr") is None or not np.array_equal(gptr, plan["gptr"]):
            # the pinned staging buffer may still be the source of the previous step's asynchronous upload: wait for that
            # copy before rewriting it (callers other than train_on_batch do not synchronise between steps)
            if plan.get("uploaded") is not None:
                plan["uploaded"].synchronize()
            plan["table"][:, 1] = gptr[plan["tix"]] + plan["off4"]
            plan["host"].copy_(torch.from_numpy(plan["table"]))
            plan["dev"].copy_(plan["host"], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(plan["dev"].device))
            plan["uploaded"] = ev
            plan["gptr"] = gptr
        return plan

    # ---- clip + step ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def clip_grad_norm_(self, max_norm):
        """Global L2 norm of all gradients and the clip coefficient, both left on the device.  DEFERRED clip: unlike
        ``torch.nn.utils.clip_grad_norm_`` the gradients are NOT scaled in place -- the coefficient is applied inside the
        next ``step()`` while the Adam sweep reads them (readers of ``p.grad`` between the two calls see the unclipped
        values; the returned norm is the pre-clip norm, as in torch).  ``zero_grad()`` cancels a pending coefficient.
        With several param groups the gradients are clipped in place (torch semantics) and ``step()`` runs unclipped.
        Returns the total norm (0-d device tensor)."""
        self._refuse_swapped("clip_grad_norm_()")
        plans = []
        for gi, group in enumerate(self.param_groups):
            ps = self._active(group)
            if ps:
                plans.append(self._plan(gi, ps))
        if not plans:
            return torch.zeros(())
        if len(plans) != 1:
            from .ddp import clip_grad_norm_fused
            for pl in plans:
                pl["clip_ready"] = False
            return clip_grad_norm_fused([p for g in self.param_groups for p in g["params"]], max_norm)
        plan = plans[0]
        dev = plan["dev"].device
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            n = plan["dev"].shape[0]
            _lib.check(_lib.fn("dsc_grad_sumsq_f32")(plan["dev"].data_ptr(), n, plan["partial"].data_ptr(), s),
                       "dsc_grad_sumsq_f32")
            _lib.check(_lib.fn("dsc_clip_coef_f32")(plan["partial"].data_ptr(), n, float(max_norm), plan["norm"].data_ptr(),
                                                    plan["coef"].data_ptr(), s), "dsc_clip_coef_f32")
        plan["clip_ready"] = True
        return plan["norm"]

    def cancel_pending_clip(self):
        for plan in self._plans.values():
            plan["clip_ready"] = False          # a coefficient computed for gradients that no longer exist must not be applied

    def zero_grad(self, set_to_none=True):
        self.cancel_pending_clip()
        return super().zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None):
        self._refuse_swapped("step()")               # it would train the average
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            ps = self._active(group)
            if not ps:
                continue
            clip = bool(self._plans.get(gi, {}).get("clip_ready"))
            plan = self._plans[gi] if clip else self._plan(gi, ps)     # clip_grad_norm_ already uploaded the work list
            plan["clip_ready"] = False
            b1, b2 = group["betas"]
            ema = self.ema_decay is not None
            # (Adam step, EMA updates made) of every parameter: one launch per distinct pair
            pkey = [(self._steps[id(p)], self._ema_steps[id(p)] if ema else 0) for p in ps]
            steps = sorted(set(pkey))
            dev = plan["dev"].device
            with torch.cuda.device(dev):
                s = torch.cuda.current_stream(dev).cuda_stream
                if len(steps) == 1:
                    sel = [(steps[0], plan["dev"], plan["edev"], plan["dev"].shape[0])]
                else:      # parameters that joined later carry their own bias correction (and their own EMA warm-up)
                    sel = []
                    pix = np.array([steps.index(k) for k in pkey])
                    for j, sv in enumerate(steps):
                        rows = torch.from_numpy(np.nonzero(pix[plan["tix"]] == j)[0]).to(dev)
                        sub = plan["dev"].index_select(0, rows).contiguous()
                        esub = plan["edev"].index_select(0, rows).contiguous() if ema else None      # the same rows of the averages
                        sel.append((sv, sub, esub, sub.shape[0]))
                for (sv, ek), tab, etab, n in sel:
                    t = sv + 1
                    bc1 = 1.0 - b1 ** t
                    bc2_sqrt = (1.0 - b2 ** t) ** 0.5
                    coef = plan["coef"].data_ptr() if clip else None
                    if ema:
                        _lib.check(_lib.fn("dsc_adam_ema_step_f32")(tab.data_ptr(), etab.data_ptr(), n, group["lr"] / bc1, b1, b2,
                                                                    bc2_sqrt, group["eps"], group["weight_decay"], coef,
                                                                    ema_decay_at(self.ema_decay, self.ema_warmup, ek), s),
                                   "dsc_adam_ema_step_f32")
                    else:
                        _lib.check(_lib.fn("dsc_adam_step_f32")(tab.data_ptr(), n, group["lr"] / bc1, b1, b2, bc2_sqrt,
                                                                group["eps"], group["weight_decay"], coef, s),
                                   "dsc_adam_step_f32")
            for p in ps:
                self._steps[id(p)] += 1
                if ema:
                    self._ema_steps[id(p)] += 1
            # the kernel wrote the parameters through raw pointers: tell autograd / the engine's derived-weight cache
            # (DenoiserEngine._signature reads p._version) that they changed
            torch.autograd.graph.increment_version(ps)
            _bump_weights_epoch()
        return loss

    # ---- weight EMA: swap the average in for sampling / validation ----------------------------------------------------
    @torch.no_grad()
    def ema_swap(self):
        """Exchange every parameter with its average, in place (dsc_ema_swap_f32); call again to swap back.  Parameters that have
        had no EMA update yet are their own average and stay.  While swapped (``ema_swapped``) ``step()``, ``clip_grad_norm_()``
        and ``state_dict()`` raise."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdam.ema_swap(): this optimizer keeps no weight EMA (ema_decay=None)")
        ps = [p for g in self.param_groups for p in g["params"] if "ema" in self.state.get(p, {})]
        if ps:
            es = [self.state[p]["ema"] for p in ps]
            key = tuple(t.data_ptr() for t in ps + es)
            if self._swap_tables is None or self._swap_tables[0] != key:      # work lists per device, kept between swaps
                by_dev = {}
                for p, e in zip(ps, es):
                    _check_ema_tensor(p, "FusedAdam.ema_swap")
                    by_dev.setdefault(p.device, ([], []))
                    by_dev[p.device][0].append(p)
                    by_dev[p.device][1].append(e)
                self._swap_tables = (key, [_ema_tables(dp, de) for dp, de in by_dev.values()])
            _ema_exchange(ps, self._swap_tables[1])
        self.ema_swapped = not self.ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """``with optimizer.ema_weights(): network.generate_layout(...)`` -- the model computes with the average inside, with the
        raw weights again after (also after an exception)."""
        self.ema_swap()
        try:
            yield self
        finally:
            self.ema_swap()
