"""The multistep DPM-Solver++(2M) solver on the host -- no kernel is executed here.

* the new symbol is declared in the header, exported and bound; ops.multistep_rec checks its operands;
* ops.multistep_weights is the closed form of INTEGRATION.md 9 for S in {1, 2, 3, 20}: e_0 = e_{S-1} = 0, e_k = h_k / (2 h_{k-1}), which
  lies in (0.46, 0.80) at S = 20 on the linear schedule;
* ``sampling_solver``: the three refusals -- an unknown name, no ``sampling_timesteps``, ``ddim_sampling_eta != 0`` -- fire before anything
  is drawn, on the loops of GaussianDiffusion and on the wrapper; ``None`` hands _loop no new keyword; the wrapper hands the keyword on;
* the oracle alone (tests/multistep_oracle.py), float64, on the toy at S = 20, linear betas 1e-4 .. 0.02, T = 1000: at the state before
  the last pair (t = 49) the RMS error of the 2M chain against the exact solution is at most 0.5 x that of the eta = 0 DDIM chain.
  Computed on the host: 0.00234 against 0.00690, a ratio of 0.34, in float64 and in float32 alike -- 0.5 is a condition with that
  margin.  The clamp is never active on the toy: |D| <= 0.32."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

import multistep_oracle as O
from test_steer_host import _gd, _wrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dsc_multistep_x0_f32"


def test_the_new_symbol_is_declared_exported_and_bound():
    import ctypes
    from diffuscene_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    m = re.search(r"^int %s\((.*?)\);" % NAME, hdr, flags=re.M | re.S)
    assert m, "%s is not declared" % NAME
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert hasattr(_lib.load(), NAME) and restype is ctypes.c_int and len(argtypes) == len(params)
    for p, ty in zip(params, argtypes):
        assert (ty is ctypes.c_int32) == p.startswith("int32_t"), p
        assert (ty is ctypes.c_int64) == p.startswith("int64_t"), p
    for name in ("x_t", "model_out", "hist", "weights", "step", "times", "ca", "cb", "cfg_scale", "counts", "mask", "mean_type", "num_steps"):
        assert any(p.endswith(name) for p in params), name
    assert NAME not in [name for name, _ in ops.STEP_ENTRY.values()] and len(ops.STEP_ENTRY) == 10
    assert ops.SOLVERS == ("dpmpp_2m",)


def test_multistep_rec_checks_its_operands_on_the_host():
    from diffuscene_amd import ops
    x = torch.zeros(2, 3, 12)
    i = torch.zeros(1, dtype=torch.int64)
    strided = (i, i, i, torch.zeros(3, 1))
    with pytest.raises(ValueError, match="one given part"):
        ops.multistep_rec(x, x, x, x, 0, (x, x), strided=strided, rows=(x, x, x), mask=(x, x, x))
    with pytest.raises(ValueError, match="strided"):
        ops.multistep_rec(x, x, x, x, 0, (x, x))
    with pytest.raises(ValueError, match="strided"):
        ops.multistep_rec(x, x, x, x, 0, (x, x), strided=strided, t=i)
    with pytest.raises(RuntimeError, match="HIP device"):                            # no CPU path
        ops.multistep_rec(x, x, x, x, 0, (x, x), strided=strided)


@pytest.mark.parametrize("S", [1, 2, 3, 20])
def test_weights_are_the_closed_form(S):
    from diffuscene_amd import ops
    abar = np.cumprod(1.0 - O.betas())
    prs = O.pairs(S)
    gd = _gd()                                                                       # T = 50: the pairs are the loop's own
    assert O.pairs(min(S, 50), 50) == gd.ddim_schedule(min(S, 50), 0.0)[0]
    w = ops.multistep_weights(prs, abar)
    want = O.weights(prs, abar)
    assert w.dtype == torch.float32 and tuple(w.shape) == (S,) and w.device.type == "cpu"
    assert float(w[0]) == 0.0 and float(w[-1]) == 0.0
    assert torch.equal(w, torch.from_numpy(want).float())                            # float64 on the host, one rounding
    lam = 0.5 * np.log(abar / (1.0 - abar))
    for k in range(1, S - 1):
        h_k, h_prev = lam[prs[k][1]] - lam[prs[k][0]], lam[prs[k - 1][1]] - lam[prs[k - 1][0]]
        assert h_k > 0 and h_prev > 0 and abs(float(w[k]) - h_k / (2 * h_prev)) <= 1e-7
    if S == 20:
        assert all(0.46 < float(v) < 0.80 for v in w[1:-1]), w.tolist()
    # the table of a diffusion object: from ITS float64 alphas_cumprod and ITS pairs, cached per (S, device)
    S50 = min(S, 50)
    tab = gd.multistep_table(S50, "cpu")
    assert torch.equal(tab, ops.multistep_weights(gd.ddim_schedule(S50, 0.0)[0], np.cumprod(1.0 - gd.np_betas)))
    assert gd.multistep_table(S50, "cpu") is tab
    with pytest.raises(ValueError, match="float64"):
        ops.multistep_weights(prs, torch.zeros(3, 3))


def _never(*a, **k):
    raise AssertionError("a refused call drew noise")


def test_the_loops_refuse_before_anything_is_drawn():
    shape = (2, 5, 12)
    gd = _gd()
    known = dict(known=torch.zeros(shape), mask=torch.zeros(shape) > 0)
    x = torch.zeros(shape)
    loops = ((gd.ddim_sample_loop, (), {}), (gd.ddim_masked_loop, (), known), (gd.ddim_guided_loop, (1.0,), {}),
             (gd.ddim_masked_guided_loop, (1.0,), known), (gd.ddim_complete_ragged_loop, (), dict(partial_boxes=x[:, :2], num_partial=[1, 2])),
             (gd.ddim_arrange_loop, (), dict(input_boxes=x)))
    for loop, args, kw in loops:
        for bad in ("dpm", "DPMPP_2M", "", 2, True):
            with pytest.raises(ValueError, match="sampling_solver"):
                loop(None, shape, "cpu", None, None, *args, noise_fn=_never, sampling_timesteps=5, sampling_solver=bad, **kw)
        for eta in (0.5, 1.0, 1e-9):
            with pytest.raises(ValueError, match="ddim_sampling_eta = 0"):
                loop(None, shape, "cpu", None, None, *args, noise_fn=_never, sampling_timesteps=5, ddim_sampling_eta=eta,
                     sampling_solver="dpmpp_2m", **kw)
    with pytest.raises(ValueError, match="goes with sampling_timesteps"):            # a T-step spec
        gd._loop("p_sample_loop", None, shape, "cpu", None, None, _never, None, multistep="dpmpp_2m")
    for name in ("p_sample_loop", "p_sample_loop_masked", "p_sample_loop_guided", "p_sample_loop_arrange"):   # the T-step loops have no such keyword
        with pytest.raises(TypeError):
            getattr(gd, name)(None, shape, "cpu", None, None, sampling_solver="dpmpp_2m")


def test_none_hands_the_loop_no_new_keyword(monkeypatch):
    from diffuscene_amd.networks import diffusion_ddpm as D
    gd = _gd()
    seen = []
    monkeypatch.setattr(D.GaussianDiffusion, "_loop", lambda self, what, *a, **kw: seen.append((what, kw)) or torch.zeros(2, 5, 5))
    shape = (2, 5, 12)
    x = torch.zeros(shape)
    calls = ((gd.ddim_sample_loop, (), {}), (gd.ddim_masked_loop, (), dict(known=x, mask=x > 0)), (gd.ddim_guided_loop, (1.0,), {}),
             (gd.ddim_masked_guided_loop, (1.0,), dict(known=x, mask=x > 0)),
             (gd.ddim_complete_ragged_loop, (), dict(partial_boxes=x[:, :2], num_partial=[1, 2])), (gd.ddim_arrange_loop, (), dict(input_boxes=x)))
    for loop, args, kw in calls:
        loop(None, shape, "cpu", None, None, *args, sampling_timesteps=5, **kw)
        loop(None, shape, "cpu", None, None, *args, sampling_timesteps=5, sampling_solver=None, **kw)
        loop(None, shape, "cpu", None, None, *args, sampling_timesteps=5, sampling_solver="dpmpp_2m", **kw)
    assert len(seen) == 3 * len(calls)
    for i in range(0, len(seen), 3):
        assert "multistep" not in seen[i][1] and "multistep" not in seen[i + 1][1] and seen[i][1] == seen[i + 1][1]
        assert seen[i + 2][1]["multistep"] == "dpmpp_2m"
        assert {k: v for k, v in seen[i + 2][1].items() if k != "multistep"} == seen[i][1]
    assert D._solver_kw(None) == {} and D._solver_kw("dpmpp_2m") == dict(multistep="dpmpp_2m")


def test_the_front_ends_take_the_keyword_and_only_the_strided_ones():
    from diffuscene_amd import sampler
    fronts = sorted(n for n in vars(sampler) if n.startswith("graph_") and n.endswith("_loop"))
    assert len(fronts) == 10
    x = torch.zeros(2, 3, 12)
    for front in fronts:
        args = ([x[:, 0, 0]] if "guided" in front else []) + list((5, 0.0) if "ddim" in front else (True, 5))
        with pytest.raises(RuntimeError, match="graph sampling needs"):              # None reaches the loop as before
            getattr(sampler, front)(None, None, (2, 3, 12), "cpu", None, None, *args, multistep=None)
        if "ddim" not in front:
            with pytest.raises(ValueError, match="strided"):
                getattr(sampler, front)(None, None, (2, 3, 12), "cpu", None, None, *args, multistep=torch.zeros(5))


def test_the_wrapper_hands_the_keyword_on_and_refuses(tmp_path):
    N, C = 12, 62
    m = _wrapper("uncond", tmp_path)
    room = torch.zeros(3, 1, 64, 64)
    known = torch.zeros(3, N, C)
    none = torch.zeros(3, N, dtype=torch.bool)
    on = dict(sampling_timesteps=20, sampling_solver="dpmpp_2m")
    with contextlib.redirect_stdout(io.StringIO()):
        m.generate_layout_batched(room, N, C, 3, sampling_timesteps=20)
        m.generate_layout_batched(room, N, C, 3, **on)
        m.generate_layout_batched(room, N, C, 3, scene_seeds=[1, 2, 3], collision_scale=0.1, **on)
        m.generate_layout(room, N, C, 3, **on)
        m.sample(room, N, C, 3, **on)
        m.complete_scene_batched(room, N, C, [known[0, :2], known[1, :0], known[2, :5]], **on)
        m.complete_scene(room, N, C, known[:, :4], 3, **on)
        m.inpaint_scene_batched(room, N, C, known, none, **on)
        m.inpaint_scene_batched(room, N, C, known, none, sampling_timesteps=20)
    calls = m.diffusion.calls
    assert [c[0] for c in calls] == ["gen_samples_ddim"] * 5 + ["complete_samples_ragged_ddim"] * 2 + ["inpaint_samples_ddim"] * 2
    for i in (0, 8):                                                                 # None: not a keyword more than before
        assert "sampling_solver" not in calls[i][2]
    for i in range(1, 8):
        assert calls[i][2]["sampling_solver"] == "dpmpp_2m" and calls[i][2]["sampling_timesteps"] == 20
    assert "noise_fn" in calls[2][2] and calls[2][2]["collision_scale"] == 0.1       # combines with seeds and steering
    before = len(calls)
    cpu_rng = torch.get_rng_state()
    entries = ((m.generate_layout_batched, (room, N, C, 3)), (m.generate_layout, (room, N, C, 3)), (m.sample, (room, N, C, 3)),
               (m.complete_scene_batched, (room, N, C, known[:, :4])), (m.complete_scene, (room, N, C, known[:, :4], 3)),
               (m.inpaint_scene_batched, (room, N, C, known, none)))
    for fn, args in entries:
        with pytest.raises(ValueError, match="sampling_solver"):                     # an unknown name
            fn(*args, sampling_timesteps=20, sampling_solver="euler")
        with pytest.raises(ValueError, match="goes with sampling_timesteps"):        # the keyword without sampling_timesteps
            fn(*args, sampling_solver="dpmpp_2m")
        with pytest.raises(ValueError, match="ddim_sampling_eta = 0"):               # the SDE form
            fn(*args, sampling_timesteps=20, ddim_sampling_eta=0.5, sampling_solver="dpmpp_2m")
    assert len(calls) == before and torch.equal(torch.get_rng_state(), cpu_rng)      # refused before anything is drawn or computed


def test_the_arrange_entry_points_take_the_keyword(tmp_path):
    m = _wrapper("arrange", tmp_path)
    N, C = 12, 62
    room, boxes = torch.zeros(2, 1, 64, 64), torch.zeros(2, N, C)
    on = dict(sampling_timesteps=20, sampling_solver="dpmpp_2m")
    calls = []
    # the condition assembly of a re-arrangement model runs on the device: stand in for it, keep the call behind it
    m._sampling_conditions = lambda *a, **kw: (None, None)
    m.diffusion.arrange_samples_ddim = lambda shape, device, **kw: calls.append(kw) or torch.zeros(shape)
    with contextlib.redirect_stdout(io.StringIO()):
        m.arrange_scene(room, N, C, boxes, 2, **on)
        m.arrange_scene_batched(room, N, C, boxes, **on)
        m.arrange_scene_batched(room, N, C, boxes, sampling_timesteps=20)
    assert len(calls) == 3
    assert calls[0]["sampling_solver"] == calls[1]["sampling_solver"] == "dpmpp_2m" and "sampling_solver" not in calls[2]
    for fn, args in ((m.arrange_scene, (room, N, C, boxes, 2)), (m.arrange_scene_batched, (room, N, C, boxes))):
        with pytest.raises(ValueError, match="goes with sampling_timesteps"):
            fn(*args, sampling_solver="dpmpp_2m")
        with pytest.raises(ValueError, match="sampling_solver"):
            fn(*args, sampling_timesteps=20, sampling_solver="heun")
    assert len(calls) == 3


def test_the_oracle_chain_halves_the_error_of_ddim_on_the_toy():
    S = 20
    tab, prs = O.tables(S)
    assert prs[-1] == (49, -1) and prs[0][0] == 999 and len(prs) == S
    z = torch.randn(4096, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    exact = O.toy_exact(z, float(tab["alpha"][-1]), float(tab["sigma"][-1]))        # the state at t = 49
    for dtype in (torch.float64, torch.float32):
        ddim, _ = O.chain(tab, z, False, dtype)
        solved, dmax = O.chain(tab, z, True, dtype)
        err_2m, err_ddim = O.rms(solved[-2], exact), O.rms(ddim[-2], exact)
        print("toy chain S = 20 at t = 49 (%s): 2M %.5f, DDIM %.5f, ratio %.3f, max |D| %.3f" % (dtype, err_2m, err_ddim, err_2m / err_ddim, dmax))
        assert dmax <= 0.32                                                          # the clamp is never active
        assert err_2m <= 0.5 * err_ddim, (err_2m, err_ddim)
    # S <= 2 has no second-order pair: the solver's chain is the DDIM chain
    for s in (1, 2):
        t2, _ = O.tables(s)
        assert all(torch.equal(a, b) for a, b in zip(O.chain(t2, z, True)[0], O.chain(t2, z, False)[0]))


def test_the_statement_leaves_given_elements_and_zero_weights_alone():
    g = torch.Generator().manual_seed(1)
    x, mo, hist = (torch.randn(2, 3, 5, generator=g) for _ in range(3))
    given = torch.zeros(2, 3, 5, dtype=torch.bool)
    given[0, :2] = True
    for mt in (O.EPS, O.X0, O.V):
        m0, h0 = O.correct(x, mo, torch.full_like(hist, float("nan")), 0.0, 1.5, 0.5, mt)
        assert torch.equal(m0, mo) and bool(torch.isfinite(h0).all())                # e == 0: hist is not read, mo is not written
        m1, h1 = O.correct(x, mo, hist, 0.5, 1.5, 0.5, mt, given=given)
        assert torch.equal(m1[given], mo[given]) and torch.equal(h1[given], hist[given]) and not torch.equal(m1[~given], mo[~given])
        m2, h2 = O.correct(x, mo, hist, 0.5, 1.5, 0.5, mt, last=True)
        assert torch.equal(m2, mo) and torch.equal(h2, hist)
        # the step's x0 on the corrected output is D, up to the two roundings
        raw = mo if mt == O.X0 else 1.5 * x - 0.5 * mo
        D = raw.clamp(-1, 1).double() + 0.5 * (raw.clamp(-1, 1).double() - hist.double())
        m3, _ = O.correct(x, mo, hist, 0.5, 1.5, 0.5, mt)
        got = m3 if mt == O.X0 else 1.5 * x - 0.5 * m3
        assert float((got.double() - D).abs().max()) <= 4e-6
