"""GPU: the weight EMA -- the three kernels of csrc/optim.hip through the C ABI on hand-made chunk tables with sentinels around every
tensor, FusedAdam(ema_decay=...) and ParamEMA against float64 recurrences, the guards while the average is swapped in, and the seam
between training and the captured sampling loops: weights exchanged in place under graphs and derived weights that must follow."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_plan import _model, _relnorm, _sample  # noqa: E402

CHUNK = 32768
COUNTS = (1, 3, 4, 255, 256, 257, 1023, 32768, 70001)          # 70001 = chunks of 32768, 32768 and 4465
GUARD = 4                                                      # sentinel elements (at least) on both sides of every tensor
SENTINEL = 12345.0
PHASES = {"aligned": (0, 0), "ema": (0, 1), "param": (1, 0), "both": (1, 1)}      # first element of (param, ema) past a 16-byte boundary
DECAY = 0.9


def dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(dev()).cuda_stream


def _layout(phase):
    """Element offset of every tensor of COUNTS in one buffer, each start ``phase`` elements past a multiple of 4 (torch allocations are
    16-byte aligned), GUARD or more sentinel elements between neighbours and at both ends: (starts, buffer length, data mask)."""
    starts, pos = [], GUARD
    for c in COUNTS:
        s = (pos + 3) // 4 * 4 + phase
        starts.append(s)
        pos = s + c + GUARD
    size = (pos + 3) // 4 * 4 + GUARD
    mask = torch.zeros(size, dtype=torch.bool)
    for s, c in zip(starts, COUNTS):
        mask[s:s + c] = True
    assert all(s >= GUARD and s + c + GUARD <= size for s, c in zip(starts, COUNTS))
    return starts, size, mask


def _buffer(layout, fill):
    """CPU float32 buffer: ``fill(count)`` inside every tensor, SENTINEL everywhere else."""
    starts, size, _ = layout
    buf = torch.full((size,), SENTINEL, dtype=torch.float32)
    for s, c in zip(starts, COUNTS):
        buf[s:s + c] = fill(c)
    return buf


def _tables(bufs, layouts, ema, ema_layout):
    """(chunk table [n, 5] int64, ema addresses [n] int64) on the device over device buffers ``bufs`` = (param, grad, exp_avg, exp_avg_sq);
    a None buffer leaves its column 0.  Every chunk lies inside its tensor: offset + count <= the tensor's count."""
    rows, eptr = [], []
    for i, c in enumerate(COUNTS):
        for off in range(0, c, CHUNK):
            n = min(CHUNK, c - off)
            assert off + n <= c
            rows.append([0 if b is None else b.data_ptr() + 4 * (lay[0][i] + off) for b, lay in zip(bufs, layouts)] + [n])
            eptr.append(ema.data_ptr() + 4 * (ema_layout[0][i] + off))
    assert [r[4] for r in rows[-3:]] == [32768, 32768, 4465]
    return torch.tensor(rows, dtype=torch.int64, device=dev()), torch.tensor(eptr, dtype=torch.int64, device=dev())


_INPUTS = {}


def _inputs(phase_name):
    """The operands of one pointer phase, drawn once on the CPU and never modified (tests clone them to the device)."""
    if phase_name not in _INPUTS:
        pp, ep = PHASES[phase_name]
        g = torch.Generator().manual_seed(11 + 2 * pp + ep)
        lp, le, l0 = _layout(pp), _layout(ep), _layout(0)
        rn = lambda scale, shift=0.0: (lambda c: torch.randn(c, generator=g).abs() * scale + shift)      # noqa: E731
        _INPUTS[phase_name] = dict(
            lp=lp, le=le, l0=l0,
            # weights and average of one sign (see test_fused_sweep...: the 2-ulp bound holds for such operands); gradients of both
            p=_buffer(lp, rn(0.3, 0.05)), e=_buffer(le, rn(0.3, 0.05)),
            g=_buffer(l0, lambda c: torch.randn(c, generator=g)), m=_buffer(l0, lambda c: torch.randn(c, generator=g) * 0.1),
            v=_buffer(l0, rn(0.01, 0.01)))
    return _INPUTS[phase_name]


ADAM = dict(step_size=2e-3 / (1 - 0.9 ** 3), beta1=0.9, beta2=0.999, bc2_sqrt=(1 - 0.999 ** 3) ** 0.5, eps=1e-8)


def _adam_args(weight_decay, scale):
    return (ADAM["step_size"], ADAM["beta1"], ADAM["beta2"], ADAM["bc2_sqrt"], ADAM["eps"], weight_decay,
            None if scale is None else scale.data_ptr())


@pytest.mark.parametrize("grad_scale,weight_decay", [(None, 0.0), (0.37, 0.01)])
@pytest.mark.parametrize("phase", list(PHASES))
def test_fused_sweep_is_adam_bit_for_bit_and_the_average_is_the_float32_expression(phase, grad_scale, weight_decay):
    """dsc_adam_ema_step_f32 against dsc_adam_step_f32 on copies (param, exp_avg, exp_avg_sq: torch.equal, sentinels included), its
    average against ``e + (p_new - e) * (1 - d)`` evaluated by torch on the CPU in float32 in that order (torch.equal) and against the
    same expression in float64 (2 ulp), and dsc_ema_update_f32 against the fused kernel's average (torch.equal).

    The 2-ulp bound: with d = 0.9 the float32 ``1 - d`` is exact, so the kernel's value carries three roundings -- of the difference
    (<= ulp(max(|e|, |p|)) / 2, scaled by 1 - d), of the product and of the sum (half an ulp each).  The test's weights and averages are
    positive, so the result is at least (1 - d) max(e, p) (d >= 1 - d) and at least the product's magnitude: the three terms are below
    1, 1/2 and 1/2 ulp of the RESULT, 2 ulp in all.  (Operands of opposite sign can cancel in the sum, and no bound in ulp of the
    result holds then.)"""
    from diffuscene_amd import _lib
    x = _inputs(phase)
    lays = (x["lp"], x["l0"], x["l0"], x["l0"])
    scale = None if grad_scale is None else torch.tensor(grad_scale, device=dev())

    def device_set():
        return [x[k].to(dev()) for k in ("p", "g", "m", "v")]

    plain = device_set()
    e_plain = x["e"].to(dev())
    tab, eptr = _tables(plain, lays, e_plain, x["le"])
    _lib.check(_lib.fn("dsc_adam_step_f32")(tab.data_ptr(), tab.shape[0], *_adam_args(weight_decay, scale), _stream()), "adam")
    fused = device_set()
    e_fused = x["e"].to(dev())
    tab_f, eptr_f = _tables(fused, lays, e_fused, x["le"])
    _lib.check(_lib.fn("dsc_adam_ema_step_f32")(tab_f.data_ptr(), eptr_f.data_ptr(), tab_f.shape[0], *_adam_args(weight_decay, scale),
                                                DECAY, _stream()), "adam_ema")
    torch.cuda.synchronize()
    for name, a, b in zip("pgmv", plain, fused):
        assert torch.equal(a, b), name
    assert torch.equal(plain[1].cpu(), x["g"]) and torch.equal(e_plain.cpu(), x["e"])                 # read-only operands
    assert not torch.equal(plain[0].cpu(), x["p"])
    for name, buf, lay in (("p", plain[0], x["lp"]), ("m", plain[2], x["l0"]), ("v", plain[3], x["l0"]), ("e", e_fused, x["le"])):
        assert bool((buf.cpu()[~lay[2]] == SENTINEL).all()), "sentinel of %s overwritten" % name
    # the float32 expression, statement by statement, on the CPU
    p_new, e_old = _gather(fused[0].cpu(), x["lp"]), _gather(x["e"], x["le"])
    omd = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(DECAY, dtype=torch.float32)
    d32 = p_new - e_old
    d32 = d32 * omd
    want = e_old + d32
    got = _gather(e_fused.cpu(), x["le"])
    assert torch.equal(got, want), int((got != want).sum())
    assert float(p_new.min()) > 0 and float(e_old.min()) > 0
    want64 = e_old.double() + (p_new.double() - e_old.double()) * (1.0 - float(np.float32(DECAY)))
    ulp = (torch.nextafter(want64.float(), torch.tensor(float("inf"))) - want64.float()).double()
    worst = float(((got.double() - want64).abs() / ulp).max())
    print("phase %s: average within %.3f ulp of float64" % (phase, worst))
    assert worst <= 2.0
    # the stand-alone kernel: it reads param and count only (every other column 0)
    e_alone = x["e"].to(dev())
    tab_a, eptr_a = _tables((fused[0], None, None, None), lays, e_alone, x["le"])
    before = fused[0].clone()
    _lib.check(_lib.fn("dsc_ema_update_f32")(tab_a.data_ptr(), eptr_a.data_ptr(), tab_a.shape[0], DECAY, _stream()), "ema_update")
    torch.cuda.synchronize()
    assert torch.equal(e_alone, e_fused) and torch.equal(fused[0], before)


def _gather(buf, layout):
    return torch.cat([buf[s:s + c] for s, c in zip(layout[0], COUNTS)])


SPECIALS = (0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001)


def _bits(layout, seed):
    """int32 buffer of random bit patterns (NaNs with payloads, signed zeros, infinities and denormals up front in every tensor that has
    room), the sentinel's pattern elsewhere."""
    starts, size, _ = layout
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((size,), SENTINEL, dtype=torch.float32).view(torch.int32).clone()
    sp = torch.tensor([s - (1 << 32) if s >= (1 << 31) else s for s in SPECIALS], dtype=torch.int64).to(torch.int32)
    for s, c in zip(starts, COUNTS):
        buf[s:s + c] = torch.randint(-2 ** 31, 2 ** 31, (c,), generator=g, dtype=torch.int64).to(torch.int32)
        k = min(c, len(sp))
        buf[s:s + k] = sp[:k] if seed % 2 else sp.flip(0)[:k]
    return buf


@pytest.mark.parametrize("phase", list(PHASES))
def test_swap_exchanges_bit_patterns_and_twice_is_the_identity(phase):
    from diffuscene_amd import _lib
    pp, ep = PHASES[phase]
    lp, le = _layout(pp), _layout(ep)
    p0, e0 = _bits(lp, 1), _bits(le, 2)
    p, e = p0.to(dev()), e0.to(dev())
    tab, eptr = _tables((p, None, None, None), (lp, lp, lp, lp), e, le)
    swap = _lib.fn("dsc_ema_swap_f32")
    _lib.check(swap(tab.data_ptr(), eptr.data_ptr(), tab.shape[0], _stream()), "swap")
    torch.cuda.synchronize()
    want_p, want_e = p0.clone(), e0.clone()
    for sp_, se_, c in zip(lp[0], le[0], COUNTS):
        want_p[sp_:sp_ + c] = e0[se_:se_ + c]
        want_e[se_:se_ + c] = p0[sp_:sp_ + c]
    assert torch.equal(p.cpu(), want_p) and torch.equal(e.cpu(), want_e)            # int32: NaN payloads and -0.0 compared as bits
    assert not torch.equal(want_p, p0)
    _lib.check(swap(tab.data_ptr(), eptr.data_ptr(), tab.shape[0], _stream()), "swap")
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0) and torch.equal(e.cpu(), e0)


def test_invalid_arguments_return_einval_without_launching():
    from diffuscene_amd import _lib
    x = _inputs("aligned")
    bufs = [x[k].to(dev()) for k in ("p", "g", "m", "v")]
    e = x["e"].to(dev())
    tab, eptr = _tables(bufs, (x["lp"], x["l0"], x["l0"], x["l0"]), e, x["le"])
    n, T, E, s = tab.shape[0], tab.data_ptr(), eptr.data_ptr(), _stream()
    adam, upd, swap = (_lib.fn(k) for k in ("dsc_adam_ema_step_f32", "dsc_ema_update_f32", "dsc_ema_swap_f32"))
    a = _adam_args(0.0, None)
    EINVAL = -1
    for decay in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert adam(T, E, n, *a, decay, s) == EINVAL and upd(T, E, n, decay, s) == EINVAL
    assert adam(T, None, n, *a, DECAY, s) == EINVAL and adam(None, E, n, *a, DECAY, s) == EINVAL and adam(T, E, 0, *a, DECAY, s) == EINVAL
    assert adam(T, E, n, a[0], a[1], a[2], 0.0, a[4], a[5], a[6], DECAY, s) == EINVAL                  # bias_correction2_sqrt, as in Adam
    assert upd(T, None, n, DECAY, s) == EINVAL and upd(None, E, n, DECAY, s) == EINVAL and upd(T, E, 0, DECAY, s) == EINVAL
    assert swap(T, None, n, s) == EINVAL and swap(None, E, n, s) == EINVAL and swap(T, E, 0, s) == EINVAL
    torch.cuda.synchronize()
    for k, b in zip(("p", "g", "m", "v"), bufs):
        assert torch.equal(b.cpu(), x[k]), k
    assert torch.equal(e.cpu(), x["e"])
    assert upd(T, E, n, 0.0, s) == 0                                                                   # decay 0 is valid: e + (p - e)
    torch.cuda.synchronize()
    e_old, p_old = _gather(x["e"], x["le"]), _gather(x["p"], x["lp"])
    assert torch.equal(_gather(e.cpu(), x["le"]), e_old + (p_old - e_old))


# ------------------------------------------------------------------------------------------------------------------ the optimizers
SHAPES = [(512, 512), (70001,), (3, 5, 7), (1,), (2048, 64), (13,)]      # test_fused_adam_matches_torch_adam_with_clipping's
LATE = len(SHAPES)                                                       # + one parameter that joins at step 3
STEPS = 4


def _grads(it):
    g = torch.Generator().manual_seed(100 + it)
    return [torch.randn(s, generator=g) * (5.0 if it % 2 == 0 else 0.01) for s in SHAPES + [(300,)]]      # clipped / unclipped steps


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * 0.3).to(dev())) for s in SHAPES + [(300,)]]


def _set_grads(ps, it):
    for i, (p, g) in enumerate(zip(ps, _grads(it))):
        p.grad = None if (i == LATE and it < 2) else g.to(dev())


@pytest.mark.parametrize("decay,warmup", [(0.5, False), (0.999, True)])
def test_fused_adam_with_ema_trains_the_same_weights_and_keeps_the_recurrence(decay, warmup):
    from diffuscene_amd.optim import FusedAdam

    def decay_at(n):                        # decay of update n (from 0), as the issue states it, in double
        return min(decay, (1 + n) / (10 + n)) if warmup else decay

    ps, qs = _params(), _params()
    opt = FusedAdam(ps, lr=2e-3, ema_decay=decay, ema_warmup=warmup)
    ref = FusedAdam(qs, lr=2e-3)
    avg = [None] * len(ps)                  # float64 recurrence from the recorded parameter values
    k = [0] * len(ps)
    for it in range(STEPS):
        _set_grads(ps, it)
        _set_grads(qs, it)
        before = [p.detach().double().cpu() for p in ps]
        opt.clip_grad_norm_(10.0)
        ref.clip_grad_norm_(10.0)
        opt.step()
        ref.step()
        for i, (p, q) in enumerate(zip(ps, qs)):
            assert torch.equal(p, q), (it, i)
            if p.grad is None:
                assert torch.equal(p.detach().double().cpu(), before[i]) and "ema" not in opt.state.get(p, {})
                continue
            if avg[i] is None:
                avg[i] = before[i]          # the average starts as the parameter before its first update
            avg[i] = avg[i] + (p.detach().double().cpu() - avg[i]) * (1.0 - decay_at(k[i]))
            k[i] += 1
            e = opt.state[p]["ema"]
            assert e.shape == p.shape and e.dtype == torch.float32 and e.device == p.device
            assert _relnorm(e.cpu(), avg[i]) < 1e-6, (it, i, _relnorm(e.cpu(), avg[i]))
    assert k == [STEPS] * LATE + [STEPS - 2]
    sd = opt.state_dict()
    for i in range(len(ps)):
        assert set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq", "ema", "ema_step"}
        es = sd["state"][i]["ema_step"]
        assert es.dim() == 0 and es.dtype == torch.float32 and float(es) == k[i] and float(sd["state"][i]["step"]) == k[i]
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in ref.state_dict()["state"].values())
    # round trip into a second optimizer over copies of the weights: the fifth step continues bit-identically
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = FusedAdam(rs, lr=2e-3, ema_decay=decay, ema_warmup=warmup)
    opt2.load_state_dict(copy.deepcopy(sd))
    _set_grads(ps, STEPS)
    _set_grads(rs, STEPS)
    for o in (opt, opt2):
        o.clip_grad_norm_(10.0)
        o.step()
    for i, (p, r) in enumerate(zip(ps, rs)):
        assert torch.equal(p, r) and torch.equal(opt.state[p]["ema"], opt2.state[r]["ema"]), i
        assert opt.state[p]["ema"].data_ptr() != opt2.state[r]["ema"].data_ptr()
    assert float(opt2.state_dict()["state"][LATE]["ema_step"]) == STEPS - 1
    # a checkpoint without the average: it starts from the loaded parameters at the next step, k = 0
    plain = copy.deepcopy(ref.state_dict())
    opt3 = FusedAdam(qs, lr=2e-3, ema_decay=decay, ema_warmup=warmup)
    opt3.load_state_dict(plain)
    _set_grads(qs, STEPS)
    start = qs[1].detach().double().cpu()
    opt3.step()
    want = start + (qs[1].detach().double().cpu() - start) * (1.0 - decay_at(0))
    assert _relnorm(opt3.state[qs[1]]["ema"].cpu(), want) < 1e-6 and float(opt3.state_dict()["state"][1]["ema_step"]) == 1.0


def test_param_ema_around_sgd_keeps_the_recurrence_and_swaps():
    from diffuscene_amd.networks import optimizer_factory
    from diffuscene_amd.optim import ParamEMA
    ps = _params()[:LATE]
    opt = optimizer_factory({"optimizer": "SGD", "lr": 0.1, "ema_decay": 0.5}, iter(ps))
    assert isinstance(opt, torch.optim.SGD) and isinstance(opt.ema, ParamEMA)
    avg = [p.detach().double().cpu() for p in ps]
    for it in range(3):
        for p, g in zip(ps, _grads(it)):
            p.grad = g.to(dev())
        opt.step()
        avg = [a + (p.detach().double().cpu() - a) * 0.5 for a, p in zip(avg, ps)]
    assert opt.ema.num_updates == 3
    for e, a, p in zip(opt.ema.shadow, avg, ps):
        assert _relnorm(e.cpu(), a) < 1e-6 and not torch.equal(e, p)
    raw = [p.detach().clone() for p in ps]
    shadow = [e.clone() for e in opt.ema.shadow]
    versions = [p._version for p in ps]
    with pytest.raises(ZeroDivisionError):
        with opt.ema.weights():
            assert opt.ema.swapped and all(torch.equal(p, e) for p, e in zip(ps, shadow))
            assert all(torch.equal(e, r) for e, r in zip(opt.ema.shadow, raw))
            assert all(p._version > v for p, v in zip(ps, versions))
            with pytest.raises(RuntimeError, match="swapped"):
                opt.ema.update()
            with pytest.raises(RuntimeError, match="swapped"):
                opt.step()
            1 / 0
    assert not opt.ema.swapped and all(torch.equal(p, r) for p, r in zip(ps, raw))
    assert all(torch.equal(e, s) for e, s in zip(opt.ema.shadow, shadow))


def test_fused_adam_refuses_to_train_clip_or_save_the_average():
    from diffuscene_amd.optim import FusedAdam, weights_epoch
    ps = _params()[:LATE]
    opt = FusedAdam(ps, lr=2e-3, ema_decay=0.5)
    for it in range(2):
        for p, g in zip(ps, _grads(it)):
            p.grad = g.to(dev())
        opt.step()
    raw = [p.detach().clone() for p in ps]
    avg = [opt.state[p]["ema"].clone() for p in ps]
    ptrs = [p.data_ptr() for p in ps]
    versions, epoch = [p._version for p in ps], weights_epoch()
    assert not any(torch.equal(r, a) for r, a in zip(raw, avg))
    with pytest.raises(KeyError):
        with opt.ema_weights() as inside:
            assert inside is opt and opt.ema_swapped
            assert all(torch.equal(p, a) for p, a in zip(ps, avg)) and all(torch.equal(opt.state[p]["ema"], r) for p, r in zip(ps, raw))
            assert [p.data_ptr() for p in ps] == ptrs and all(p._version > v for p, v in zip(ps, versions)) and weights_epoch() > epoch
            for call in (opt.step, lambda: opt.clip_grad_norm_(10.0), opt.state_dict):
                with pytest.raises(RuntimeError, match="swapped in"):
                    call()
            assert all(torch.equal(p, a) for p, a in zip(ps, avg))                      # the refused calls changed nothing
            raise KeyError("leaves through an exception")
    assert not opt.ema_swapped
    assert all(torch.equal(p, r) for p, r in zip(ps, raw)) and all(torch.equal(opt.state[p]["ema"], a) for p, a in zip(ps, avg))
    opt.state_dict()
    opt.ema_swap()
    assert opt.ema_swapped and all(torch.equal(p, a) for p, a in zip(ps, avg))
    opt.ema_swap()
    assert not opt.ema_swapped and all(torch.equal(p, r) for p, r in zip(ps, raw))
    opt.clip_grad_norm_(10.0)
    opt.step()


# ---------------------------------------------------------------------------------------------------------------------- the seam
def _flat(scene):
    return torch.cat([scene[k].reshape(scene[k].shape[0], -1).float() for k in sorted(scene)], dim=1)


def test_average_swapped_in_under_the_captured_sampling_loop_and_back_out(tmp_path):
    """Three train_on_batch steps with ema_decay=0.5; under ema_weights() the captured two-step loop computes with the average (equal to
    a second model built from ema_model_state, different from the raw weights); after leaving, sampling is bit-identical to before
    entering and a fourth training step lands where a twin that never swapped lands.  A derived weight (standardised weights, bf16
    planes, packed time MLPs) not re-derived after either exchange fails one of the four comparisons."""
    from diffuscene_amd.networks import optimizer_factory
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import train_on_batch
    from diffuscene_amd.optim import ema_model_state
    B, N = 2, 12
    tcfg = {"training": {"max_grad_norm": 10}}
    ocfg = {"optimizer": "Adam", "lr": 2e-4, "ema_decay": 0.5}
    ma, nc = _model("uncond", N, tmp_path, seed=0)
    mb, _ = _model("uncond", N, tmp_path, seed=0)
    mb.load_state_dict(ma.state_dict())
    oa = optimizer_factory(ocfg, filter(lambda p: p.requires_grad, ma.parameters()))
    ob = optimizer_factory(ocfg, filter(lambda p: p.requires_grad, mb.parameters()))
    s = _sample("uncond", B, N, nc)
    C = 8 + nc + 32
    room = torch.zeros(B, 1, 64, 64, device=dev())

    def train(model, opt, i):
        torch.manual_seed(11 + i)
        return train_on_batch(model, opt, s, tcfg)

    def sample(model):
        torch.manual_seed(5)
        with contextlib.redirect_stdout(io.StringIO()):
            return _flat(model.generate_layout(room, N, C, batch_size=B, keep_empty=True, clip_denoised=True, sampling_timesteps=2))

    for i in range(3):
        train(ma, oa, i)
        train(mb, ob, i)
    raw_before = sample(ma)
    mc, _ = _model("uncond", N, tmp_path, seed=1)
    mc.load_state_dict(ema_model_state(ma, oa))
    from_state = sample(mc)
    ptrs = [p.data_ptr() for p in ma.parameters()]
    with oa.ema_weights():
        swapped = sample(ma)
        assert oa.ema_swapped
    assert [p.data_ptr() for p in ma.parameters()] == ptrs
    assert swapped.shape == raw_before.shape and swapped.shape[0] == B and bool(torch.isfinite(swapped).all())
    print("average under the captured loop vs a model built from ema_model_state: %.3g" % _relnorm(swapped, from_state))
    assert _relnorm(swapped, from_state) < 1e-6
    assert not torch.equal(swapped, raw_before)
    assert torch.equal(sample(ma), raw_before)
    for p, q in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p, q)
    train(ma, oa, 3)
    train(mb, ob, 3)
    for (name, p), q in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(p, q), name
    for p, q in zip(oa.param_groups[0]["params"], ob.param_groups[0]["params"]):
        assert torch.equal(oa.state[p]["ema"], ob.state[q]["ema"])
