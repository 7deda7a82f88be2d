"""Every hand-written backward kernel of csrc/train.hip against the float64 statements of oracle/train_bwd_ref.py, one entry point
and one dispatch branch at a time, at the smallest shapes at which each can still go wrong (tests/test_gpu_train.py sees them only
through the autograd wrappers, dense and aligned, at product shapes).  Launches go through HipBackend's methods, as the planner's do.

Operands.  Every input with a leading dimension is a column slice of a wider tensor; every output is a slice of a wider tensor that
holds NaN where the kernel must write and 7.5 everywhere else.  After each launch: the owned elements are finite, the sentinel
elements and the inputs are bit-unchanged.  "Aligned": offset and leading dimension multiples of 4 floats; "unaligned": offset 1
or an odd width.  Every launch gets valid arguments only.

Discrete and exactly representable outcomes are compared EXACTLY: transposes, copies, one-IEEE-add accumulations, column sums of
small integers (any order is exact: tests/test_train_bwd_ref_host.py), the zero rows of idle LayerNorm blocks, LeakyReLU backward.

Everything else is held, per output tensor, to
    err = max over units ( max|got - ref64| / max|ref64| over the unit )  <=  max(4 * err_torch32, FLOOR),  FLOOR = 64 * 2^-24
where a unit is what one block computes -- a (scene, group) tile of GroupNorm, a (scene, head) slab of the attentions, a row of
LayerNorm / weight standardisation, the whole tensor for per-channel sums and activations -- and err_torch32 is the same distance
for the oracle evaluated in float32 on the CPU (the rule, factor and floor of tests/test_gpu_foldingnet_kernels.py).  A unit whose
float64 reference vanishes (max|ref64| <= 1e-12 max|dy|: identically zero up to float64 rounding, e.g. weight standardisation of
one column, dq and dk of an attention over one key) is compared absolutely: |got| <= FLOOR * max|dy|.  Every measured err goes to
$DSC_PARITY_LOG when it is set.

FLOORS lists the output tensors whose floor is not the default one, with the measurement and the arithmetic that causes it; no
floor exceeds the tolerance tests/test_gpu_train.py applies to the same operation (CAPS)."""
import os

import numpy as np
import pytest
import torch

from oracle import train_bwd_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR = 64 * 2.0 ** -24
SENT = 7.5
C = T.C
F32, F64 = torch.float32, torch.float64
CAPS = {"gn_silu_bwd": 2e-5, "linear_attention_bwd": 1e-5, "attention_bwd": 1e-5, "ws_bwd": 1e-5, "layernorm_bwd": 5e-6,
        "act_bwd gelu": 5e-6, "act_bwd silu": 2e-6}
# (entry point, tensor) -> raised floor = 2 x the worst err measured over this module's cases on the MI355X; none is needed so far
FLOORS = {}


def backend():
    from diffuscene_amd.train_plan import HipBackend
    return HipBackend(torch.device(DEV))


def lib():
    from diffuscene_amd import _lib, ops
    return _lib, ops


def launch(be, steps):
    _lib, ops = lib()
    be.finalize()
    be.run(steps if isinstance(steps, list) else [steps], ops.stream_ptr())
    torch.cuda.synchronize()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Case:
    """The operands of one launch: wide inputs (kept to prove they are unchanged) and canary outputs."""

    def __init__(self):
        self.ins, self.outs = [], []

    def inp(self, a, left=4, right=4):
        """a [rows, w] or [w] (numpy fp32) -> its slice of a wider device tensor"""
        a = np.asarray(a, np.float32)
        if a.ndim == 1:
            big = torch.full((left + a.shape[0] + right,), SENT, dtype=F32)
            big[left:left + a.shape[0]] = torch.from_numpy(a)
            big = big.to(DEV)
            self.ins.append((big, host(big).copy()))
            return big[left:left + a.shape[0]]
        big = torch.full((a.shape[0], left + a.shape[1] + right), SENT, dtype=F32)
        big[:, left:left + a.shape[1]] = torch.from_numpy(a)
        big = big.to(DEV)
        self.ins.append((big, host(big).copy()))
        return big[:, left:left + a.shape[1]]

    def out(self, rows, w, left=4, right=4, above=1, below=1, init=None):
        """-> [rows, w] slice of a [above + rows + below, left + w + right] tensor: NaN (or init) inside, 7.5 around"""
        big = torch.full((above + rows + below, left + w + right), SENT, dtype=F32)
        big[above:above + rows, left:left + w] = float("nan") if init is None else torch.from_numpy(np.asarray(init, np.float32))
        own = np.zeros(tuple(big.shape), bool)
        own[above:above + rows, left:left + w] = True
        big = big.to(DEV)
        self.outs.append((big, own))
        return big[above:above + rows, left:left + w]

    def out1(self, n, left=4, right=4):
        big = torch.full((left + n + right,), SENT, dtype=F32)
        big[left:left + n] = float("nan")
        own = np.zeros((left + n + right,), bool)
        own[left:left + n] = True
        big = big.to(DEV)
        self.outs.append((big, own))
        return big[left:left + n]

    def pool(self, sizes, gap=4, fill=None):
        """contiguous runs of sizes[i] floats, `gap` sentinel floats before, between and after (offsets stay multiples of 4 when the
        sizes are).  fill None: an output pool (NaN runs); else fill[i] are the input values.  -> list of 1-D views"""
        offs, o = [], gap
        for s in sizes:
            offs.append(o)
            o += s + (-s) % 4 + gap
        big = torch.full((o + gap,), SENT, dtype=F32)
        own = np.zeros((o + gap,), bool)
        for i, (f, s) in enumerate(zip(offs, sizes)):
            big[f:f + s] = float("nan") if fill is None else torch.from_numpy(np.asarray(fill[i], np.float32).reshape(-1))
            own[f:f + s] = True
        big = big.to(DEV)
        if fill is None:
            self.outs.append((big, own))
        else:
            self.ins.append((big, host(big).copy()))
        return [big[f:f + s] for f, s in zip(offs, sizes)]

    def check(self, what):
        for big, before in self.ins:
            assert (bits(host(big)) == bits(before)).all(), "%s: an input changed" % what
        for big, own in self.outs:
            h = host(big)
            assert np.isfinite(h[own]).all(), "%s: %d owned output elements were not written (or not finite)" % (
                what, (~np.isfinite(h[own])).sum())
            assert (bits(h[~own]) == bits(np.float32(SENT))).all(), "%s: %d elements outside the output changed" % (
                what, (bits(h[~own]) != bits(np.float32(SENT))).sum())


def _log(line):
    print(line)
    if os.environ.get("DSC_PARITY_LOG"):
        with open(os.environ["DSC_PARITY_LOG"], "a") as f:
            f.write(line + "\n")


def whole(a):
    return a.reshape(1, -1)


def rows_(a):
    return a.reshape(a.shape[0], -1)


def tiles(scenes, n):
    """[scenes*n, 512] -> [(scene, group), n*64]"""
    return lambda a: a.reshape(scenes, n, 8, 64).transpose(0, 2, 1, 3).reshape(scenes * 8, -1)


def slabs(scenes, n):
    """[scenes*n, 128] -> [(scene, head), n*32]"""
    return lambda a: a.reshape(scenes, n, 4, 32).transpose(0, 2, 1, 3).reshape(scenes * 4, -1)


def bounded(entry, tensor, case, got, ref64, t32, units=whole, dymax=1.0, prefix="train_bwd", caps=None, floors=None):
    """-> (ok, line) for one output tensor under the bound of the module docstring.  (prefix, caps, floors: the log tag and the CAPS /
    FLOORS tables of a sibling module that states the same rule; the defaults are this module's.)"""
    caps, floors = CAPS if caps is None else caps, FLOORS if floors is None else floors
    g, r, t = (units(np.asarray(host(a) if torch.is_tensor(a) else a, np.float64)) for a in (got, ref64, t32))
    assert g.shape == r.shape == t.shape, (entry, tensor, g.shape, r.shape, t.shape)
    assert np.isfinite(g).all(), (entry, tensor, case)
    floor = floors.get((entry, tensor), FLOOR)
    assert floor <= max(caps.get(entry, FLOOR), FLOOR)
    scale = np.abs(r).max(1)
    zero = scale <= 1e-12 * dymax
    ok, err, e32 = True, 0.0, 0.0
    if zero.any():
        ok = np.abs(g[zero]).max() <= floor * dymax
    if (~zero).any():
        err = (np.abs(g - r)[~zero].max(1) / scale[~zero]).max()
        e32 = (np.abs(t - r)[~zero].max(1) / scale[~zero]).max()
    bound = max(4.0 * e32, floor)
    line = "%s %s | %s | %s: err %.3g (bound %.3g, err_torch32 %.3g)%s" % (
        prefix, entry, tensor, case, err, bound, e32, " zero units: max|got| %.3g" % np.abs(g[zero]).max() if zero.any() else "")
    _log(line)
    return bool(ok and err <= bound), line


def check_all(results):
    bad = [line for ok, line in results if not ok]
    assert not bad, "\n".join(bad)


def exact(got, want):
    got, want = np.asarray(host(got) if torch.is_tensor(got) else got), np.asarray(host(want) if torch.is_tensor(want) else want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.dtype != np.float32:
        assert (want.astype(np.float32).astype(np.float64) == want).all()
        want = want.astype(np.float32)
    return bool((bits(got) == bits(want)).all())


# ================================================================================================ dsc_gn_silu_bwd_f32
def run_gn(scenes, n, mode, kind="random", unaligned=None, seed=0):
    d = T.gn_inputs(scenes, n, mode, seed=seed + 7 * n + mode, kind=kind)
    M = scenes * n
    c = Case()
    z = c.inp(d["z"], 1, 2) if unaligned == "z" else c.inp(d["z"])
    dy, gamma, beta = c.inp(d["dy"]), c.inp(d["gamma"]), c.inp(d["beta"])
    dz = c.out(M, C)
    part = c.out(scenes, 3 * C)
    ss = dss = None
    if mode:
        ss = c.inp(d["ss"], 4, 1) if unaligned == "ss_ld" else c.inp(d["ss"])
        rows = scenes if mode == T.SS_PER_SCENE else M
        dss = c.out(rows, 2 * C, 1, 3) if unaligned == "dss" else c.out(rows, 2 * C)
    assert part.stride(0) > 3 * C and dz.stride(0) > C and (dss is None or dss.stride(0) > 2 * C)
    al = lambda t: t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0
    assert all(al(t) for t in (z, dy, dz, ss, dss) if t is not None) == (unaligned is None)
    be = backend()
    launch(be, be.gn_bwd(z, dy, gamma, beta, ss, mode, dz, part, dss, scenes, n))
    case = "B%d N%d mode%d %s %s" % (scenes, n, mode, kind, "fallback(%s)" % unaligned if unaligned else "reg")
    c.check(case)
    ref = T.gn_silu_bwd(d["z"], d["dy"], d["gamma"], d["beta"], d["ss"], mode, scenes, n, dtype=F64)
    t32 = T.gn_silu_bwd(d["z"], d["dy"], d["gamma"], d["beta"], d["ss"], mode, scenes, n, dtype=F32)
    dymax = float(np.abs(d["dy"]).max())
    grp = lambda a: a.reshape(scenes * 8, 64)
    res = [bounded("gn_silu_bwd", "dz", case, dz, ref[0], t32[0], tiles(scenes, n), dymax)]
    gp = host(part)
    for k, name in enumerate(("dbias", "dgamma", "dbeta")):
        s = slice(k * C, (k + 1) * C)
        res.append(bounded("gn_silu_bwd", name, case, gp[:, s], ref[1][:, s], t32[1][:, s], grp, dymax))
    if mode:
        gs = host(dss)
        u = grp if mode == T.SS_PER_SCENE else tiles(scenes, n)
        for k, name in enumerate(("dscale", "dshift")):
            s = slice(k * C, (k + 1) * C)
            res.append(bounded("gn_silu_bwd", name, case, gs[:, s], ref[2][:, s], t32[2][:, s], u, dymax))
        if kind == "saturated":
            uu = T.gn_u(d["z"], d["gamma"], d["beta"], d["ss"], mode, scenes, n)[3].numpy()
            sat = np.abs(uu) > 90
            assert sat.any() and (uu[sat] > 0).any() and (uu[sat] < 0).any()
            du, want = gs[:, C:].astype(np.float64), ref[2][:, C:].numpy()
            assert np.abs(du - want)[sat].max() <= FLOOR * dymax, "du where |u| > 90: %g" % np.abs(du - want)[sat].max()
    check_all(res)


GN_REG = sorted({(2, n, m) for n in (1, 16, 17, 32, 33, 80, 81, 160) for m in (0, 2)} | {(2, n, m) for n in (17, 81) for m in (1, 3)})


@pytest.mark.parametrize("scenes,n,mode", GN_REG)
def test_gn_silu_bwd_register_forms(scenes, n, mode):
    """dsc_gn_silu_bwd_f32, gn_silu_bwd_reg_kernel<2|5|10>: both sides of the form switches (32|33, 80|81), of the token lane (16|17),
    N = 1 and the largest N = 160; every ss_mode; operands aligned but strided, as the planner passes them: partial_stride > 3C,
    dss strided per scene (mode 2) and per token (modes 1, 3)."""
    run_gn(scenes, n, mode)


@pytest.mark.parametrize("n,mode,unaligned", [(1, 2, "z"), (5, 2, "z"), (80, 2, "z"), (100, 2, "z"), (160, 2, "z"), (5, 1, "z"),
                                              (21, 2, "dss"), (21, 2, "ss_ld"), (21, 1, "dss")])
def test_gn_silu_bwd_lds_fallback(n, mode, unaligned):
    """dsc_gn_silu_bwd_f32, gn_silu_bwd_kernel (the LDS-cached fallback): taken for an unaligned z, for an unaligned dss alone, and for
    a scale_shift leading dimension that is no multiple of 4 alone; N = 100 and 160 need more than 48 KB of dynamic LDS (the
    hipFuncSetAttribute branch; 80 KB at 160)."""
    run_gn(2, n, mode, unaligned=unaligned)


@pytest.mark.parametrize("unaligned", [None, "z"])
@pytest.mark.parametrize("kind,mode", [("shifted", 2), ("saturated", 1)])
def test_gn_silu_bwd_numerical_edges(kind, mode, unaligned):
    """Register form and fallback at N = 21: the variance of a group at 100 +- 0.01, and u from -100 to +100 inside every tile (the
    SiLU derivative saturates: finite everywhere, du = 0 resp. dy where |u| > 90)."""
    run_gn(2, 21, mode, kind=kind, unaligned=unaligned)


def test_gn_silu_bwd_odd_scene_count():
    """three scenes at N = 12 (register form <2>), all four conditioning modes"""
    for mode in range(4):
        run_gn(3, 12, mode)


# ================================================================================================ dsc_weight_standardize_bwd_f32
def run_ws(shapes, kinds, what):
    c = Case()
    ds = [T.ws_inputs(r, cc, seed=11 * i + cc, kind=k) for i, ((r, cc), k) in enumerate(zip(shapes, kinds))]
    sizes = [r * cc for r, cc in shapes]
    w = [v.view(s) for v, s in zip(c.pool(sizes, fill=[d["w"] for d in ds]), shapes)]
    g = [v.view(s) for v, s in zip(c.pool(sizes, fill=[d["g"] for d in ds]), shapes)]
    o = [v.view(s) for v, s in zip(c.pool(sizes), shapes)]
    be = backend()
    launch(be, be.ws_bwd(w, g, o))
    c.check(what)
    res = []
    for i, d in enumerate(ds):
        res.append(bounded("ws_bwd", "dw", "%s item %d %dx%d" % (what, i, *shapes[i]), o[i], T.ws_bwd(d["w"], d["g"], dtype=F64),
                           T.ws_bwd(d["w"], d["g"], dtype=F32), rows_, float(np.abs(d["g"]).max())))
    check_all(res)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (2, 255), (2, 256), (2, 257), (5, 2047), (2, 2048)])
def test_weight_standardize_bwd_single_items(rows, cols):
    """dsc_weight_standardize_bwd_f32, ws_bwd_kernel: one column (the reference vanishes), both sides of one element per thread (256)
    and of the eight a thread can hold (2048)."""
    run_ws([(rows, cols)], ["random"], "single")


@pytest.mark.parametrize("cols", [5, 256, 2048])
def test_weight_standardize_bwd_constant_and_shifted_rows(cols):
    """row 0 constant (variance 0, rs = eps^-1/2), row 1 = 100 +- 0.01"""
    run_ws([(3, cols)], ["edges"], "edges")


def test_weight_standardize_bwd_full_batch_with_ragged_row_counts():
    """WS_MAX = 64 items in one launch, row counts 1..7 cycling under a grid of 7 rows: the blocks past an item's own rows must not
    write (the next item's NaN run and the sentinel gaps lie behind it)."""
    _lib, ops = lib()
    shapes = [(1 + i % 7, (5, 256, 1024, 2048)[i % 4]) for i in range(_lib.WS_MAX)]
    run_ws(shapes, ["random"] * len(shapes), "batch64")


# ================================================================================================ dsc_layernorm_bwd_f32
def run_ln(m, prows, with_addend, kind="random"):
    d = T.ln_inputs(m, seed=m + prows, kind=kind)
    c = Case()
    x, g, dy = c.inp(d["x"]), c.inp(d["g"]), c.inp(d["dy"])
    add = c.inp(d["addend"]) if with_addend else None
    dx = c.out(m, C)
    dgp = c.out(prows, C, left=0, right=0)
    assert x.stride(0) > C and dx.stride(0) > C and dgp.is_contiguous()
    be = backend()
    launch(be, be.layernorm_bwd(x, g, dy, dx, dgp, add))
    case = "m%d partial_rows%d %s%s" % (m, prows, kind, " addend" if with_addend else "")
    c.check(case)
    a = d["addend"] if with_addend else None
    ref, t32 = T.layernorm_bwd(d["x"], d["g"], d["dy"], a, dtype=F64), T.layernorm_bwd(d["x"], d["g"], d["dy"], a, dtype=F32)
    dymax = float(np.abs(d["dy"]).max())
    gp = host(dgp)
    idle = [b for b in range(prows) if b * 4 >= m]
    for b in idle:
        assert (bits(gp[b]) == 0).all(), "dg_partial row %d of a block that owns no token is not +0.0" % b
    check_all([bounded("layernorm_bwd", "dx", case, dx, ref[0], t32[0], rows_, dymax),
               bounded("layernorm_bwd", "dg", case, gp.astype(np.float64).sum(0), ref[1], t32[1], whole, dymax)])


@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("m,prows", [(1, 1), (3, 1), (4, 1), (5, 2), (9, 2), (9, 5), (2049, 512), (37, 3)])
def test_layernorm_bwd(m, prows, with_addend):
    """dsc_layernorm_bwd_f32: m < 4; partial_rows above ceil(m/4) ((9, 5): the spare blocks write zeros into dg_partial); below it
    ((9, 2), (2049, 512), (37, 3): the grid-stride path); the addend; x, dy, dx and addend strided."""
    run_ln(m, prows, with_addend)


def test_layernorm_bwd_shifted_rows():
    """x = 50 +- 0.01: the variance of a shifted row"""
    run_ln(9, 3, False, kind="shifted")


# ================================================================================================ attention cores
def run_attn(which, scenes, nq, nk, qk_scale=1.0, q_scale=1.0):
    d = T.attn_inputs(scenes, nq, nk, seed=nq + 3 * nk, qk_scale=qk_scale)
    d["q"] = (d["q"] * np.float32(q_scale)).astype(np.float32)
    sc = 32 ** -0.5
    c = Case()
    Mq, Mk = scenes * nq, scenes * nk
    if nq == nk:                                                    # self form: q | k | v and dq | dk | dv slices of one buffer each
        qkv = c.inp(np.concatenate([d["q"], d["k"], d["v"]], 1))
        q, k, v = qkv[:, :128], qkv[:, 128:256], qkv[:, 256:]
        o = c.out(Mq, 384)
        dq, dk, dv = o[:, :128], o[:, 128:256], o[:, 256:]
    else:                                                           # cross form: k | v slices of a [B nk, 256] buffer
        q = c.inp(d["q"])
        kv = c.inp(np.concatenate([d["k"], d["v"]], 1))
        k, v = kv[:, :128], kv[:, 128:]
        dq = c.out(Mq, 128)
        o = c.out(Mk, 256)
        dk, dv = o[:, :128], o[:, 128:]
    do = c.inp(d["dout"])
    be = backend()
    if which == "linear":
        launch(be, be.linattn_bwd(q, k, v, do, dq, dk, dv, scenes, nq, nk, sc))
        ref = T.linear_attention_bwd(d["q"], d["k"], d["v"], d["dout"], scenes, nq, nk, sc, dtype=F64)
        t32 = T.linear_attention_bwd(d["q"], d["k"], d["v"], d["dout"], scenes, nq, nk, sc, dtype=F32)
    else:
        launch(be, be.attn_bwd(q, k, v, do, dq, dk, dv, scenes, nq, sc))
        ref = T.attention_bwd(d["q"], d["k"], d["v"], d["dout"], scenes, nq, sc, dtype=F64)
        t32 = T.attention_bwd(d["q"], d["k"], d["v"], d["dout"], scenes, nq, sc, dtype=F32)
    entry = "linear_attention_bwd" if which == "linear" else "attention_bwd"
    case = "B%d nq%d nk%d%s" % (scenes, nq, nk, " x%g" % max(qk_scale, q_scale) if max(qk_scale, q_scale) > 1 else "")
    c.check(entry + " " + case)
    dymax = float(np.abs(d["dout"]).max() * max(1.0, np.abs(d["v"]).max()))
    check_all([bounded(entry, name, case, got, r, t, slabs(scenes, n), dymax)
               for name, got, r, t, n in (("dq", dq, ref[0], t32[0], nq), ("dk", dk, ref[1], t32[1], nk), ("dv", dv, ref[2], t32[2], nk))])


@pytest.mark.parametrize("scenes,nq,nk", [(1, 1, 1), (2, 3, 7), (2, 64, 8), (2, 65, 9), (3, 12, 77), (2, 129, 65), (2, 21, 64),
                                          (1, 160, 160)])
def test_linear_attention_bwd(scenes, nq, nk):
    """dsc_linear_attention_bwd_f32: nk = 1 and nk no multiple of the 8 lanes per channel, nq and nk on either side of the 64-token pass
    (64|65) and of two passes (129), nq != nk with both above 64, the largest scene; self form (nq = nk) and cross form."""
    run_attn("linear", scenes, nq, nk)


def test_linear_attention_bwd_large_logits():
    """q and k scaled by 30: both softmaxes depend on the maximum being taken over ALL lanes of a channel / token"""
    run_attn("linear", 2, 12, 12, qk_scale=30.0)


@pytest.mark.parametrize("scenes,n", [(2, n) for n in (1, 2, 16, 17, 64, 65, 80, 81, 96, 97, 128)] + [(1, 160)])
def test_attention_bwd(scenes, n):
    """dsc_attention_bwd_f32: attention_bwd_cached_kernel with 256 (n <= 64), 320 (65..80) and 384 (81..96) threads, and the 192-thread
    recomputing attention_bwd_kernel above 96; both sides of each switch."""
    run_attn("softmax", scenes, n, n)


def test_attention_bwd_large_logits():
    """dsc_attention_bwd_f32 at n = 17 with q scaled by 30: nearly one-hot rows, the row maximum and the cancellation in p (dp - <p, dp>)"""
    run_attn("softmax", 2, 17, 17, q_scale=30.0)


# ================================================================================================ dsc_activation_bwd_f32
ACTS = {"gelu": T.ACT_GELU, "silu": T.ACT_SILU, "leaky": T.ACT_LEAKY01}


@pytest.mark.parametrize("count", [1, 255, 256, 257, 4096 * 256 + 3])
@pytest.mark.parametrize("name", ["gelu", "silu", "leaky"])
def test_activation_bwd(name, count):
    """dsc_activation_bwd_f32: GELU (polynomial erf), SiLU (hardware exp and reciprocal) bounded, LeakyReLU(0.1) bit-equal including
    x = 0 -> 0.1 dy; one thread, both sides of a block, and the grid-stride above 4096 blocks; x holds 0, +-1e-4, +-30."""
    d = T.act_inputs(count, seed=count % 1000)
    c = Case()
    x, dy, dx = c.inp(d["x"]), c.inp(d["dy"]), c.out1(count)
    be = backend()
    launch(be, be.act_bwd(x, dy, dx, ACTS[name]))
    c.check("act_bwd %s %d" % (name, count))
    t32 = T.act_bwd(d["x"], d["dy"], ACTS[name], dtype=F32)
    if name == "leaky":
        assert exact(dx, t32.numpy())
        assert bits(host(dx))[0] == bits(np.float32(0.1) * d["dy"][:1])[0] and d["x"][0] == 0
        return
    check_all([bounded("act_bwd " + name, "dx", "count %d" % count, dx, T.act_bwd(d["x"], d["dy"], ACTS[name], dtype=F64), t32,
                       whole, float(np.abs(d["dy"]).max()))])


# ================================================================================================ single-launch weight gradient
@pytest.mark.parametrize("m,k1,k2,kvalid", [(5, 8, 0, None), (5, 128, 4, 130), (300, 128, 4, 130)])
def test_gemm_tn_single_launch(m, k1, k2, kvalid):
    """dsc_gemm_tn_f32 recorded by HipBackend.gemm_tn (training plans group their weight gradients, so nothing else takes this route to
    the entry point's launch record): one slab without a workspace (5 rows, strided output) and token slabs reduced through the shared
    workspace (300 rows, dense output), one K segment and two with kvalid inside the second, operands as 16-byte aligned column slices of
    wider tensors (their row strides are the leading dimensions), the bias gradient on the same pass.  Small integers: every order of
    summation is exact, so out and dbias are bit-equal to the float64 statement."""
    _lib, _ = lib()
    n, K = 12, k1 + k2
    kv = K if kvalid is None else kvalid
    slabs = _lib.fn("dsc_gemm_tn_workspace_floats")(m, n, kv) > 0
    assert slabs == (m == 300)
    a_h, dy_h = T.small_ints((m, K), seed=m + K), T.small_ints((m, n), seed=m + n)
    assert m * T.INT_MAX_ABS ** 2 < 2 ** 24
    c = Case()
    a, dy = c.inp(a_h[:, :k1]), c.inp(dy_h)
    a2 = c.inp(a_h[:, k1:]) if k2 else None
    out = c.pool([n * kv])[0].view(n, kv) if slabs else c.out(n, kv)
    dbias = c.out1(n)
    be = backend()
    launch(be, be.gemm_tn(a, dy, out, a2=a2, kvalid=kvalid, dbias=dbias))
    c.check("gemm_tn %dx%dx%d+%d" % (m, n, k1, k2))
    want, want_b = T.gemm_tn(a_h, dy_h, kv)
    assert exact(out, want.numpy()), "gemm_tn m=%d k=%d+%d kvalid=%s: integer products differ" % (m, k1, k2, kvalid)
    assert exact(dbias, want_b.numpy()), "gemm_tn m=%d: integer column sums of dy differ" % m


# ================================================================================================ column sums
COLSUM = [(1, 1), (3, 63), (29, 64), (33, 65), (256, 70), (257, 130), (257, 132), (1000, 25), (16640, 64), (1000, 24), (700, 68)]


@pytest.mark.parametrize("out_left", [4, 5])
@pytest.mark.parametrize("m,n", COLSUM)
def test_colsum(m, n, out_left):
    """dsc_colsum_f32: one block row (m <= 256), several with reduce_slabs_kernel (2 slabs at 257, 3 at 700, 4 at 1000, capped at 64 at
    16640), its 16-byte path (n % 4 == 0 and an aligned out) and scalar path (odd n, or out one float off), the nslab % 4 tails of both,
    and the tail of the 8-deep row loop (3, 29, 33 rows).  Small integers: bit-equal in any order; random values: bounded."""
    res = []
    for kind in ("ints", "random"):
        xs = T.small_ints((m, n), seed=m + n) if kind == "ints" else T.noise((m, n), seed=m + n)
        c = Case()
        x, out = c.inp(xs), c.out1(n, left=out_left, right=8 - out_left)
        assert (out.data_ptr() % 16 == 0) == (out_left == 4)
        be = backend()
        launch(be, be.colsum(x, out))
        c.check("colsum %dx%d %s" % (m, n, kind))
        if kind == "ints":
            assert exact(out, T.colsum(xs).numpy()), "colsum %dx%d out+%d: integer sums differ" % (m, n, out_left)
        else:
            res.append(bounded("colsum", "out", "%dx%d out+%d" % (m, n, out_left), out, T.colsum(xs, dtype=F64), T.colsum(xs, dtype=F32)))
    check_all(res)


def test_colsum_grouped():
    """dsc_colsum_grouped_f32: one launch over items of 1..300 rows and 1..1536 columns (max_n = 1536: most blocks of the narrow
    items return at once), strided x."""
    shapes = [(1, 1), (4, 64), (29, 65), (33, 1536), (300, 1), (300, 1536), (33, 64), (4, 65), (1, 1536), (29, 64)]
    res = []
    for kind in ("ints", "random"):
        c = Case()
        xs = [T.small_ints(s, seed=i) if kind == "ints" else T.noise(s, seed=i) for i, s in enumerate(shapes)]
        outs = c.pool([n for _, n in shapes])
        be = backend()
        launch(be, be.colsum_grouped([(c.inp(a), o) for a, o in zip(xs, outs)]))
        c.check("colsum_grouped " + kind)
        for a, o, s in zip(xs, outs, shapes):
            if kind == "ints":
                assert exact(o, T.colsum(a).numpy()), s
            else:
                res.append(bounded("colsum_grouped", "out", "%dx%d" % s, o, T.colsum(a, dtype=F64), T.colsum(a, dtype=F32)))
    check_all(res)


# ================================================================================================ transposes, copies
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 33), (31, 33), (32, 32), (33, 65), (512, 25)])
def test_transpose_strided(rows, cols):
    """dsc_transpose_f32 (transpose_kernel, 32 x 32 tiles): ragged tiles on both sides, strided input and output; bit-equal to w.t()"""
    w = T.noise((rows, cols), seed=rows + cols)
    c = Case()
    src, dst = c.inp(w, 3, 2), c.out(cols, rows, 1, 2)
    be = backend()                       # (transpose_many would batch the shapes torch calls contiguous: a single row)
    launch(be, be._call("dsc_transpose_f32", src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), rows, cols, keep=(src, dst)))
    c.check("transpose %dx%d" % (rows, cols))
    assert exact(dst, w.T)


V4_BATCH = [(4, 4), (64, 64), (68, 60), (4, 132), (512, 1024)]


@pytest.mark.parametrize("name,shapes", [("v4", V4_BATCH), ("scalar", V4_BATCH + [(5, 8)]),
                                         ("v4x64", [(4 * (1 + i % 17), 4 * (1 + i % 33)) for i in range(64)])])
def test_transpose_batched(name, shapes):
    """dsc_transpose_batched_f32: transpose_batched_v4_kernel when EVERY item has rows and columns that are multiples of 4 (64 x 64 tiles,
    ragged at 68 x 60 and 4 x 132), transpose_batched_kernel for the whole batch as soon as one item (5 x 8, the last) does not; a full
    batch of 64 items.  Bit-equal to w.t(); the sentinel gaps between the outputs stay untouched."""
    ws = [T.noise(s, seed=i) for i, s in enumerate(shapes)]
    c = Case()
    sizes = [r * cc for r, cc in shapes]
    src = [v.view(s) for v, s in zip(c.pool(sizes, fill=ws), shapes)]
    dst = [v.view(s[1], s[0]) for v, s in zip(c.pool(sizes), shapes)]
    assert all(t.data_ptr() % 16 == 0 for t in src + dst)
    be = backend()
    steps = be.transpose_many(list(zip(src, dst)))
    assert [s[2] for s in steps] == ["dsc_transpose_batched_f32"]
    launch(be, steps)
    c.check("transpose_batched " + name)
    for w, o, s in zip(ws, dst, shapes):
        assert exact(o, w.T), "item %dx%d" % s


@pytest.mark.parametrize("slicing", ["aligned", "odd_ld", "offset1"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 4), (7, 12), (7, 5), (2050, 2048)])
def test_copy2d_and_add2d(rows, cols, slicing):
    """dsc_copy2d_f32 / dsc_add2d_f32 (copy2d_kernel<false|true>): the 16-byte path (aligned slices, cols % 4 == 0) and the scalar path (an
    odd leading dimension, a one-float offset, cols 1 and 5); 2050 x 2048 exceeds 4096 blocks on either path (grid-stride).  The copy
    is bit-equal to the source, the accumulation to one IEEE fp32 add per element."""
    left, right = {"aligned": (4, 4), "odd_ld": (4, 1 + cols % 2), "offset1": (1, 3 + (-cols) % 4)}[slicing]
    a, b = T.noise((rows, cols), seed=rows), T.noise((rows, cols), seed=rows + 1)
    for op in ("copy", "add"):
        c = Case()
        src = c.inp(a, left, right)
        dst = c.out(rows, cols, left, right, init=b if op == "add" else None)
        vec = cols % 4 == 0 and all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in (src, dst))
        assert vec == (slicing == "aligned" and cols % 4 == 0)
        be = backend()
        launch(be, be.copy(dst, src) if op == "copy" else be.add(dst, src))
        c.check("%s2d %dx%d %s" % (op, rows, cols, slicing))
        want = a if op == "copy" else (torch.from_numpy(b) + torch.from_numpy(a)).numpy()
        assert exact(dst, want), "%s2d %dx%d %s" % (op, rows, cols, slicing)


# ================================================================================================ refusals
def test_documented_refusals_return_before_any_launch():
    """Every entry point returns its error code from the host checks in front of its launch, and the NaN-filled outputs stay NaN:
    tokens_per_scene = 161 and channels = 256 (dsc_gn_silu_bwd_f32), d = 256 and an unaligned x (dsc_layernorm_bwd_f32), cols = 2049
    (dsc_weight_standardize_bwd_f32), n = 161 and an unaligned operand (dsc_attention_bwd_f32, dsc_linear_attention_bwd_f32)."""
    _lib, ops = lib()
    EALIGN, ERANGE = -2, -3

    def refused(be, step, want, outs, what):
        be.finalize()
        f, args, name = step["step"] if isinstance(step, dict) else step
        rc = f(*args, ops.stream_ptr())
        torch.cuda.synchronize()
        assert rc == want, "%s: %s returned %d, expected %d" % (what, name, rc, want)
        for o in outs:
            assert np.isnan(host(o)).all(), "%s: %s wrote to an output it refused" % (what, name)

    def nan(*shape):
        return torch.full(shape, float("nan"), device=DEV, dtype=F32)

    def val(*shape):
        return torch.ones(shape, device=DEV, dtype=F32)

    for n, ch, what in ((161, 512, "tokens_per_scene 161"), (4, 256, "channels 256")):
        be = backend()
        dz, part = nan(n, ch), nan(1, 3 * ch)
        refused(be, be.gn_bwd(val(n, ch), val(n, ch), val(ch), val(ch), None, 0, dz, part, None, 1, n), ERANGE, [dz, part], what)
    be = backend()
    dx, dg = nan(4, 256), nan(1, 512)
    refused(be, be.layernorm_bwd(val(4, 256), val(512), val(4, 256), dx, dg), ERANGE, [dx, dg], "LayerNorm d 256")
    be = backend()
    dx, dg = nan(4, 512), nan(1, 512)
    refused(be, be.layernorm_bwd(val(4, 516)[:, 1:513], val(512), val(4, 512), dx, dg), EALIGN, [dx, dg], "LayerNorm unaligned x")
    be = backend()
    dw = nan(2, 2049)
    refused(be, be.ws_bwd([val(2, 2049)], [val(2, 2049)], [dw])[0], ERANGE, [dw], "weight standardisation cols 2049")
    for which in ("attn", "linattn"):
        for n, left, want, what in ((161, 0, ERANGE, "n 161"), (8, 1, EALIGN, "unaligned k")):
            be = backend()
            k = val(n, 132)[:, left:left + 128]
            dq, dk, dv = nan(n, 128), nan(n, 128), nan(n, 128)
            step = (be.attn_bwd(val(n, 128), k, val(n, 128), val(n, 128), dq, dk, dv, 1, n, 0.5) if which == "attn" else
                    be.linattn_bwd(val(n, 128), k, val(n, 128), val(n, 128), dq, dk, dv, 1, n, n, 0.5))
            refused(be, step, want, [dq, dk, dv], which + " " + what)
