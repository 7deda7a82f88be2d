"""GPU: DSC_GEMM_ROW_INVARIANT (include/diffuscene_hip.h) across every dispatch class, and the claim that rests on it: a captured reverse
loop returns the eager loop's scenes bit for bit under one seed.

The captured loops read the (scale, shift) rows of the 19 time-conditioned blocks from a table built once with m = T rows
(DenoiserEngine.ss_table: three flagged launches without planes); the eager loop computes the same rows every step with m = B rows
(Plan._build: the same three launches through Plan.gemm, which asks ops.planes_layout and attaches planes where the library wants them).
A row must come out of both with the same bits, whichever kernel an UNFLAGGED launch of that m would take.  Before this file the flag
was read by the K-parallel kernel only, and the suite's batch sizes (2, 3, 128, 256) sat where nothing else qualified: with the flag
ignored by the split dispatch, t_pack rows at m = 160, 300, 330, 390, 420, 720, 1000 differed from the table's under the split arithmetic,
and at m = 80, 330, 390, 420, 720 under BOTH arithmetics, because the exact-f32 tiles above 64 x 64 start their accumulators from the bias
while the 64 x 64 tile adds it last; ss_t differed in every scene at B = 160, 300, 420 (420 under exact-f32 too) and every loop below
returned other scenes than its eager form (largest differences 2e-7 .. 6e-7).

* kernel level: the three time-MLP products at the model's n and K, a flagged launch of rows [:m] against rows [:m] of the flagged
  m = 1000 launch (torch.equal) and every launch against float64; the library's probes on every flagged struct; and, through the
  unflagged structs of the same launches, which split-bf16 tile and which exact-f32 tile each m stands for (M_CLASSES: the test does not
  pass because its launches happen to share a kernel);
* model level: Plan(time_table=False).ss_t against DenoiserEngine.ss_table() row by row, and eager / graph (capturing) / graph (cached)
  runs of the T-step, the guided and the strided loop at batch sizes inside the split classes;
* the fragment-major copy ops.attach_planes keeps on a planes tensor follows a re-split into the same tensor;
* dsc_gemm_planes_layout answers "no planes wanted" with a value that is no error code, and ops.planes_layout raises on a real one."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_gpu_cfg import GC, GN, _conditions, build_model, case_texts  # noqa: E402

BOTH = pytest.mark.parametrize("gemm_arith", ["split", "f32"], indirect=True)
QUIET = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731
T_ROWS = 1000                                     # rows of the table launch: Unet1D's time_table_rows


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(dev())


def rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(autouse=True)
def wave_family_on():
    """The library's default kernel families, whatever an earlier test left behind."""
    from diffuscene_amd import _lib
    prev = _lib.set_split_wave(True)
    _lib.device_error_count(reset=True)
    yield
    _lib.set_split_wave(prev)
    assert _lib.device_error_count(reset=True) == 0         # no timestep had to be clamped into a table


# ------------------------------------------------------------------------------------------------------------------- kernel level
# One m inside each dispatch class of the t_pack product (n = 19 x 1024 = 19456, K = 2048), the only one of the three that leaves the
# 64 x 64 exact-f32 tile below m = 1025 and the only one that qualifies for a split tile below m = 1153.
#   m: (split-bf16 tile of the UNFLAGGED launch with planes under the split arithmetic, exact-f32 tile by the shape)
# The library's own answers (dsc_gemm_split_tile / dsc_gemm_f32_tile); test_the_m_list_stands_for_the_classes_it_names holds them.
NONE = -1
S_64x256, S_128x128, S_160x256, S_160x128_W4, S_WAVE = 9, 7, 5, 8, 11          # DSC_TILE_*
F_160x256, F_160x128, F_128x128, F_96x128, F_64x64 = 0, 1, 2, 3, 4             # DSC_F32_TILE_*
M_CLASSES = {
    1:    (NONE,         F_64x64),       # one row
    64:   (NONE,         F_64x64),       # the last m of one 64-row block
    80:   (NONE,         F_96x128),      # 65..96: another exact-f32 tile, no split tile qualifies
    128:  (NONE,         F_64x64),       # the largest batch the eager-versus-graph tests held before
    160:  (S_64x256,     F_64x64),       # 129..192
    256:  (NONE,         F_64x64),       # 193..256: the benchmark's batch, no split tile qualifies
    300:  (S_128x128,    F_64x64),       # 257..384 is 128 x 128 on the split side, three exact-f32 tiles underneath
    330:  (S_128x128,    F_128x128),
    390:  (S_160x256,    F_96x128),      # 385..400
    420:  (S_WAVE,       F_96x128),      # 401..480: wave-autonomous kernel, fragment-major planes
    720:  (S_160x128_W4, F_160x128),     # 705..800
    1000: (S_WAVE,       F_64x64),       # the table launch itself, through Plan.gemm's path
}
# Not reached at m <= 1000 by these shapes: the split 256 x 128 tile (t_pack: from m = 1041) and the exact-f32 160 x 256 tile (the cost
# rule gives its ties to 160 x 128).  The two 2048-wide products are (NONE, F_64x64) at every m of the list.
#           K     n (None: rows of the engine's t_pack_w)   activation
PRODUCTS = {"time_mlp1": (512, 2048, 1),          # Linear(512, 2048) + GELU
            "time_mlp3": (2048, 2048, 2),         # Linear(2048, 2048) + SiLU (folded into the epilogue: every consumer applies it first)
            "t_pack": (2048, None, 0)}            # the 19 Linear(2048, 1024) of the time-conditioned blocks as one product
_OPERANDS, _PLANES = {}, {}


def _t_pack_rows(tmp_path):
    m = build_model("v", 4, tmp_path, tag="row_invariant")
    return m.diffusion.model.engine(dev()).t_pack_w.shape[0]


def _operands(product, tmp_path):
    """(a, w, b, act, float64 reference of all T_ROWS rows): made once per product, shared, never written."""
    if product not in _OPERANDS:
        K, n, act = PRODUCTS[product]
        n = n or _t_pack_rows(tmp_path)
        seed = 40 + 10 * sorted(PRODUCTS).index(product)
        a, w, b = rnd(T_ROWS, K, seed=seed), rnd(n, K, seed=seed + 1, scale=0.05), rnd(n, seed=seed + 2)
        z = a.double() @ w.double().T + b.double()
        ref = F.gelu(z) if act == 1 else (F.silu(z) if act == 2 else z)
        _OPERANDS[product] = (a, w, b, act, ref)
    return _OPERANDS[product]


def _planes(product, w, layout):
    if (product, layout) not in _PLANES:
        from diffuscene_amd import ops
        (_PLANES[product, layout],) = ops.split_planes([(w, None, 2 * layout)])
    return _PLANES[product, layout]


def _as_plan_gemm(product, a, w, y, b, act, row_invariant):
    """The struct Plan.gemm builds: ask the library which planes the launch wants, make them in that layout, attach them."""
    from diffuscene_amd import ops
    g = ops.make_gemm_args(a, w, y, b, act_out=act, row_invariant=row_invariant)
    lay = ops.planes_layout(g)
    if lay >= 0:
        ops.attach_planes(g, _planes(product, w, lay), layout=lay)
    return g, lay


def _classes(product, tmp_path):
    """{m: (split tile, exact-f32 tile)} of the unflagged launches, by the library's probes."""
    from diffuscene_amd import _lib
    a, w, b, act, _ = _operands(product, tmp_path)
    out = {}
    for m in M_CLASSES:
        y = torch.empty(m, w.shape[0], device=dev())
        g, lay = _as_plan_gemm(product, a[:m], w, y, b, act, row_invariant=False)
        out[m] = (_lib.fn("dsc_gemm_split_tile")(g, 0) if lay >= 0 else NONE, _lib.fn("dsc_gemm_f32_tile")(g))
    return out


@BOTH
def test_the_m_list_stands_for_the_classes_it_names(gemm_arith, tmp_path):
    """Non-vacuity of the test below: without the flag, the launches of the m list go through the five dense split-bf16 classes 64 x 256,
    128 x 128, 160 x 256, 160 x 128 four-wave and wave-autonomous (split arithmetic) and through four exact-f32 tiles (either arithmetic)."""
    assert _t_pack_rows(tmp_path) == 19 * 1024
    got = _classes("t_pack", tmp_path)
    want = {m: (s if gemm_arith == "split" else NONE, f) for m, (s, f) in M_CLASSES.items()}
    assert got == want
    if gemm_arith == "split":
        assert {S_64x256, S_128x128, S_160x256, S_160x128_W4, S_WAVE} <= {s for s, _ in got.values()}
    assert {f for _, f in got.values()} == {F_64x64, F_96x128, F_128x128, F_160x128}
    for product in ("time_mlp1", "time_mlp3"):
        assert set(_classes(product, tmp_path).values()) == {(NONE, F_64x64)}, product


@BOTH
@pytest.mark.parametrize("product", list(PRODUCTS))
def test_a_flagged_launch_gives_a_row_the_same_bits_at_every_m(gemm_arith, product, tmp_path):
    """The table launch (m = 1000, flagged, no planes: what ss_table() makes) against flagged launches of rows [:m] made the way Plan.gemm
    makes them, and against a caller that hands the flagged launch planes all the same.  The library's probes on both structs: no split
    tile, no planes wanted, exact-f32 arithmetic, not the K-parallel kernel, and the one exact-f32 tile the table launch takes (64 x 64)
    at every m.  Bounds against float64, max-relative: a linear
    product 2e-6 * max(1, K / 1024) (tests/test_gpu_split.py::test_split_gemm_plain), an activated one 3e-6
    (tests/test_gpu_ops.py::test_gemm_epilogues_two_segments_residual) -- a swapped or dropped row passes no such comparison."""
    from diffuscene_amd import _lib, ops
    a, w, b, act, ref = _operands(product, tmp_path)
    K, n = w.shape[1], w.shape[0]
    bound = 3e-6 if act else 2e-6 * max(1.0, K / 1024)
    table = ops.gemm(a, w, b, act_out=act, row_invariant=True)
    r = rel(table, ref)
    print("%s %s table launch: rel %.3g (bound %.3g)" % (product, gemm_arith, r, bound))
    assert r < bound, (product, r)
    probes, differ = [], []
    for m in M_CLASSES:
        y = torch.full((m, n), float("nan"), device=dev())
        g, lay = _as_plan_gemm(product, a[:m], w, y, b, act, row_invariant=True)
        # a caller that attaches planes to the flagged launch (ops.gemm(..., w_planes=, row_invariant=True)): ignored, not multiplied with
        y2 = torch.full((m, n), float("nan"), device=dev())
        g2 = ops.make_gemm_args(a[:m], w, y2, b, act_out=act, row_invariant=True, w_planes=_planes(product, w, ops.PLANES_ROWMAJOR))
        for which, s in (("plan", g), ("planes given", g2)):
            answers = (_lib.fn("dsc_gemm_split_tile")(s, 0), _lib.fn("dsc_gemm_planes_layout")(s, 0), _lib.fn("dsc_gemm_arithmetic")(s, 0),
                       _lib.fn("dsc_gemm_skinny")(s, 0), _lib.fn("dsc_gemm_f32_tile")(s))
            if answers != (NONE, _lib.DSC_PLANES_NONE, 0, 0, F_64x64):
                probes.append((m, which, answers))
        if lay >= 0 or ops.planes_layout(g2) >= 0:
            probes.append((m, "ops.planes_layout", lay))
        ops.run_gemm(g)
        ops.run_gemm(g2)
        for which, out in (("plan", y), ("planes given", y2)):
            r = rel(out, ref[:m])
            print("%s %s m=%d %s: rel %.3g, equal to the table rows: %s" % (product, gemm_arith, m, which, r, torch.equal(out, table[:m])))
            if not torch.equal(out, table[:m]):
                differ.append((m, which, float((out - table[:m]).abs().max())))
            assert r < bound, (product, m, which, r)
    # (m, struct, (split tile, planes layout, arithmetic, skinny, exact-f32 tile)) of every flagged struct the library would not keep on the one
    # exact-f32 tile the table launch takes
    assert not probes, probes
    assert not differ, differ                    # (m, struct, largest difference from the table's rows)


# ------------------------------------------------------------------------------------------------------------------- model level
_COND = {}


def _model(tmp_path):
    return build_model("v", 4, tmp_path, tag="row_invariant")          # text wrapper, N = 12, a schedule of 4 timesteps


def _cond(m, B):
    if B not in _COND:
        texts = case_texts()
        _COND[B] = _conditions(m, B, [texts[i % len(texts)] for i in range(B)])
    return _COND[B]


@BOTH
@pytest.mark.parametrize("B", [160, 300, 420])        # t_pack without the flag: 64 x 256, 128 x 128, wave-autonomous (M_CLASSES)
def test_per_step_scale_shift_rows_are_the_table_rows(gemm_arith, B, tmp_path):
    """What the eager loop's denoiser call computes at B scenes (Plan(time_table=False).ss_t) against the rows the captured loops gather."""
    m = _model(tmp_path)
    eng = m.diffusion.model.engine(dev())
    cond, cross = _cond(m, B)
    T = eng.time_table.shape[0]
    t = torch.linspace(0, T - 1, B).round().to(torch.int64)
    t = t[torch.randperm(B, generator=torch.Generator().manual_seed(B))].to(dev())         # a spread over the table, out of order
    assert int(t.min()) == 0 and int(t.max()) == T - 1 == T_ROWS - 1
    plan = eng.prepare(B, GN, cond, cross, time_table=False)
    assert not plan.time_table and plan.B == B
    plan.x_in.zero_()
    plan.t_in.copy_(t)
    plan.run()
    table = eng.ss_table()
    assert tuple(plan.ss_t.shape) == (B, table.shape[1]) and tuple(table.shape) == (T, 19 * 1024)
    want = table[t]
    rows = (plan.ss_t != want).any(dim=1).nonzero().flatten().tolist()
    assert not rows, "%d of %d scenes differ from their table row (first: scene %d, t = %d), largest difference %g" % (
        len(rows), B, rows[0], int(t[rows[0]]), float((plan.ss_t - want).abs().max()))
    assert torch.isfinite(plan.ss_t).all()


#         entry point            scenes  rows of the denoiser call   extra arguments
LOOPS = [("gen_samples", 160, 160, dict(clip_denoised=True)),
         ("gen_samples", 300, 300, dict(clip_denoised=True)),
         ("gen_samples_guided", 80, 160, dict(clip_denoised=True, guidance_scale=2.0)),             # both halves in one call: 2 B rows
         ("gen_samples_ddim", 160, 160, dict(sampling_timesteps=3, ddim_sampling_eta=0.5))]


@BOTH
@pytest.mark.parametrize("loop,B,rows,kw", LOOPS, ids=["%s-%d" % (c[0], c[1]) for c in LOOPS])
def test_captured_loops_are_the_eager_loops_inside_the_split_classes(gemm_arith, loop, B, rows, kw, tmp_path):
    """Eager, graph (this call captures), graph (cached) under one seed, as tests/test_gpu_sampler_core.py, at batch sizes whose t_pack
    launch a split tile would take without the flag."""
    m = _model(tmp_path)
    diff, gd = m.diffusion, m.diffusion.diffusion
    assert M_CLASSES[rows][0] != NONE
    cond, cross = _cond(m, B)
    shape = (B, GN, GC)
    outs, states = [], []
    for graph in (False, True, True):
        torch.manual_seed(1357)
        with torch.no_grad(), QUIET():
            outs.append(getattr(diff, loop)(shape, dev(), condition=cond, condition_cross=cross, graph=graph, **kw))
        states.append(torch.cuda.get_rng_state(dev()))
    (g,) = gd._graphs.values()
    assert g.plan.time_table and g.plan.B == rows              # the captured loop read the table, at this many rows
    assert torch.equal(states[1], states[0]) and torch.equal(states[2], states[0])
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    for name, o in (("capturing", outs[1]), ("cached", outs[2])):
        scenes = (o != outs[0]).flatten(1).any(dim=1)
        assert torch.equal(o, outs[0]), "%s graph run: %d of %d scenes differ from the eager loop, largest difference %g" % (
            name, int(scenes.sum()), B, float((o - outs[0]).abs().max()))


# ------------------------------------------------------------------------------------------------------------------- two small things
@pytest.mark.parametrize("gemm_arith", ["split"], indirect=True)
def test_a_resplit_into_the_same_planes_tensor_reaches_the_wave_kernel(gemm_arith):
    """ops.attach_planes keeps a fragment-major copy on row-major planes for the wave-autonomous kernel; ops.split_planes writes the planes
    through a raw pointer.  After new weights are split into the SAME tensor the next launch must multiply with the new weights."""
    from diffuscene_amd import _lib, ops
    M, n, K = 20480, 512, 512                                           # wave-autonomous, as tests/test_gpu_wave.py
    a, w = rnd(M, K, seed=71), rnd(n, K, seed=72, scale=0.05)
    (pl,) = ops.split_planes([(w, None, False)])
    y = torch.empty(M, n, device=dev())
    g = ops.make_gemm_args(a, w, y, w_planes=pl)
    assert _lib.fn("dsc_gemm_split_tile")(g, 0) == _lib.TILE_WAVE_DENSE and g.w_planes != pl.data_ptr()       # the converted copy
    ops.run_gemm(g)
    r = rel(y, a.double() @ w.double().T)
    assert r < 2e-6, r
    w.mul_(-0.5).add_(rnd(n, K, seed=73, scale=0.05))                   # new weights in place
    assert ops.split_planes([(w, pl, False)])[0] is pl
    y2 = ops.gemm(a, w, w_planes=pl)
    r = rel(y2, a.double() @ w.double().T)
    assert not torch.equal(y2, y), "the launch still multiplies with the planes of the old weights"
    assert r < 2e-6, r


def test_no_planes_wanted_is_not_an_error_code():
    """dsc_gemm_planes_layout: "stays on the exact-f32 kernel" has a value of its own, DSC_EINVAL reaches the caller as an exception."""
    from diffuscene_amd import _lib, ops
    a, w, y = rnd(8, 512, seed=81), rnd(128, 512, seed=82), torch.empty(8, 128, device=dev())
    g = ops.make_gemm_args(a, w, y)
    assert _lib.DSC_PLANES_NONE not in (-1, -2, -3)                                                   # DSC_EINVAL, DSC_EALIGN, DSC_ERANGE
    assert _lib.fn("dsc_gemm_planes_layout")(g, 0) == _lib.DSC_PLANES_NONE                            # eight rows fill no chip
    assert ops.planes_layout(g) < 0 and not ops.gemm_would_use_split(g)
    g.m = 0
    assert _lib.fn("dsc_gemm_planes_layout")(g, 0) == -1                                              # DSC_EINVAL
    with pytest.raises(RuntimeError, match="dsc_gemm_planes_layout"):
        ops.planes_layout(g)
    with pytest.raises(RuntimeError, match="dsc_gemm_planes_layout"):
        ops.attach_planes(g, torch.empty(3, 128, 512, dtype=torch.int16, device=dev()))
