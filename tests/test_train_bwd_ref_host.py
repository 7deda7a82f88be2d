"""CPU only: the float64 statements of oracle/train_bwd_ref.py are what they claim to be, and the input generators of
tests/test_gpu_train_kernels.py have the properties the GPU tests rely on.

Every closed-form backward is compared with torch.autograd of the forward definition in float64 (1e-12 of the tensor maximum) and
with the SimBackend method of tests/plan_sim.py (1e-6: the simulator stores fp32), so that the two statements cannot drift apart."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_torch as R
from oracle import train_bwd_ref as T

F64 = torch.float64


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def d64(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=F64).requires_grad_(grad)


def f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32)


def sim():
    from plan_sim import SimBackend
    return SimBackend()


# ------------------------------------------------------------------------------------------------ GroupNorm + SiLU
def _gn_autograd(d, ss_mode, scenes, n):
    M = scenes * n
    z, gm, bt = d64(d["z"], True), d64(d["gamma"])[None].repeat(scenes, 1).requires_grad_(True), \
        d64(d["beta"])[None].repeat(scenes, 1).requires_grad_(True)
    y = F.group_norm(z.reshape(scenes, n, T.C).permute(0, 2, 1), 8, None, None, eps=T.EPS).permute(0, 2, 1)      # xh [B, n, C]
    u = y * gm[:, None, :] + bt[:, None, :]
    wrt = [z, gm, bt]
    if ss_mode:
        ss = d64(d["ss"], True)
        rows = T.ss_rows(ss, ss_mode, scenes, n)
        if ss_mode != T.SS_PER_SCENE:
            rows = rows.detach().clone().requires_grad_(True)       # per-token gradients for SS_PER_TOKEN and SS_PER_SLOT
        r3 = rows.reshape(scenes, n, 2 * T.C)
        u = u * (r3[..., :T.C] + 1.0) + r3[..., T.C:]
        wrt.append(ss if ss_mode == T.SS_PER_SCENE else rows)
    g = torch.autograd.grad(F.silu(u).reshape(M, T.C), wrt, d64(d["dy"]))
    dbias = g[0].reshape(scenes, n, T.C).sum(1)
    return g[0], torch.cat([dbias, g[1], g[2]], 1), (g[3] if ss_mode else None)


@pytest.mark.parametrize("scenes,n,ss_mode", [(2, 1, 0), (2, 1, 2), (3, 5, 1), (2, 5, 2), (2, 5, 3), (1, 5, 0)])
def test_gn_silu_bwd_is_the_autograd_of_group_norm_silu_and_the_simulator(scenes, n, ss_mode):
    d = T.gn_inputs(scenes, n, ss_mode, seed=10 * n + ss_mode)
    dz, part, dss = T.gn_silu_bwd(d["z"], d["dy"], d["gamma"], d["beta"], d["ss"], ss_mode, scenes, n)
    assert dz.dtype == F64 and part.dtype == F64
    adz, apart, adss = _gn_autograd(d, ss_mode, scenes, n)
    assert rel(dz, adz) < 1e-12 and rel(part, apart) < 1e-12
    for k in range(3):                                                               # dbias, dgamma, dbeta each on its own scale
        assert rel(part[:, k * T.C:(k + 1) * T.C], apart[:, k * T.C:(k + 1) * T.C]) < 1e-12
    if ss_mode:
        assert rel(dss[:, :T.C], adss[:, :T.C]) < 1e-12 and rel(dss[:, T.C:], adss[:, T.C:]) < 1e-12
    else:
        assert dss is None
    M = scenes * n
    sdz, spart = torch.empty(M, T.C), torch.empty(scenes, 3 * T.C)
    sdss = torch.empty(tuple(dss.shape)) if ss_mode else None
    sim().run([sim().gn_bwd(f32(d["z"]), f32(d["dy"]), f32(d["gamma"]), f32(d["beta"]), f32(d["ss"]) if ss_mode else None, ss_mode,
                            sdz, spart, sdss, scenes, n)], None)
    assert rel(dz, sdz) < 1e-6 and rel(part, spart) < 1e-6
    if ss_mode:
        assert rel(dss, sdss) < 1e-6
    # the float32 evaluation is the same statement, in float32
    dz32, part32, _ = T.gn_silu_bwd(d["z"], d["dy"], d["gamma"], d["beta"], d["ss"], ss_mode, scenes, n, dtype=torch.float32)
    assert dz32.dtype == torch.float32 and part32.dtype == torch.float32 and 0 < rel(dz32, dz) < 1e-4


# ------------------------------------------------------------------------------------------------ row normalisations
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (4, 300)])
def test_ws_bwd(rows, cols):
    d = T.ws_inputs(rows, cols, seed=cols)
    got = T.ws_bwd(d["w"], d["g"])
    w = d64(d["w"], True)
    wn = (w - w.mean(1, keepdim=True)) * (w.var(1, unbiased=False, keepdim=True) + T.EPS).rsqrt()
    want, = torch.autograd.grad(wn, w, d64(d["g"]))
    if cols == 1:
        assert (got == 0).all() and (want == 0).all()           # one column: the reference is identically zero
    else:
        assert rel(got, want) < 1e-12
    out = torch.full((rows, cols), float("nan"))
    sim().run([sim().ws_bwd([f32(d["w"])], [f32(d["g"])], [out])], None)
    assert float((got - out.double()).abs().max()) <= 1e-6 * max(float(got.abs().max()), 1.0)


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("with_addend", [False, True])
def test_layernorm_bwd(m, with_addend):
    d = T.ln_inputs(m, seed=m)
    add = d["addend"] if with_addend else None
    dx, dg = T.layernorm_bwd(d["x"], d["g"], d["dy"], add)
    x, g = d64(d["x"], True), d64(d["g"], True)
    y = F.layer_norm(x, (T.C,), None, None, T.EPS) * g
    ax, ag = torch.autograd.grad(y, [x, g], d64(d["dy"]))
    if with_addend:
        ax = ax + d64(add)
    assert rel(dx, ax) < 1e-12 and rel(dg, ag) < 1e-12
    sdx, sdg = torch.empty(m, T.C), torch.full((3, T.C), float("nan"))
    sim().run([sim().layernorm_bwd(f32(d["x"]), f32(d["g"]), f32(d["dy"]), sdx, sdg, f32(add) if with_addend else None)], None)
    assert rel(dx, sdx) < 1e-6 and rel(dg, sdg.double().sum(0)) < 1e-6


# ------------------------------------------------------------------------------------------------ attention cores
def _heads_dn(t, n):
    """[B*n, 128] -> (B, 4, 32, n), the layout of the reference's cores"""
    return t.reshape(-1, n, 4, 32).permute(0, 2, 3, 1)


@pytest.mark.parametrize("scenes,nq,nk", [(1, 1, 1), (2, 3, 7), (2, 5, 1)])
def test_linear_attention_bwd(scenes, nq, nk):
    d = T.attn_inputs(scenes, nq, nk, seed=nq + nk)
    sc = 32 ** -0.5
    got = T.linear_attention_bwd(d["q"], d["k"], d["v"], d["dout"], scenes, nq, nk, sc)
    q, k, v = d64(d["q"], True), d64(d["k"], True), d64(d["v"], True)
    out = R._linear_attention_core(_heads_dn(q, nq), _heads_dn(k, nk), _heads_dn(v, nk))       # (B, 128, nq), scale 32^-1/2 inside
    want = torch.autograd.grad(out.permute(0, 2, 1).reshape(scenes * nq, 128), [q, k, v], d64(d["dout"]))
    for a, b in zip(got, want):
        if float(b.abs().max()) < 1e-15:                        # nk = 1: the key softmax is constant, dq and dk vanish (float64 rounding noise)
            assert float(a.abs().max()) < 1e-15
        else:
            assert rel(a, b) < 1e-12
    outs = [torch.empty(scenes * nq, 128), torch.empty(scenes * nk, 128), torch.empty(scenes * nk, 128)]
    sim().run([sim().linattn_bwd(f32(d["q"]), f32(d["k"]), f32(d["v"]), f32(d["dout"]), *outs, scenes, nq, nk, sc)], None)
    for a, b in zip(got, outs):
        assert float((a - b.double()).abs().max()) <= 1e-6 * max(float(a.abs().max()), 1e-3)


@pytest.mark.parametrize("scenes,n", [(1, 1), (2, 5)])
def test_attention_bwd(scenes, n):
    d = T.attn_inputs(scenes, n, n, seed=n)
    sc = 32 ** -0.5
    got = T.attention_bwd(d["q"], d["k"], d["v"], d["dout"], scenes, n, sc)
    q, k, v = d64(d["q"], True), d64(d["k"], True), d64(d["v"], True)
    att = torch.einsum("bhdi,bhdj->bhij", _heads_dn(q, n) * sc, _heads_dn(k, n)).softmax(-1)
    out = torch.einsum("bhij,bhdj->bhid", att, _heads_dn(v, n)).permute(0, 2, 1, 3).reshape(scenes * n, 128)
    want = torch.autograd.grad(out, [q, k, v], d64(d["dout"]))
    for a, b in zip(got, want):
        if float(b.abs().max()) < 1e-15:                        # n = 1: the softmax is constant, dq and dk vanish
            assert float(a.abs().max()) < 1e-15
        else:
            assert rel(a, b) < 1e-12
    outs = [torch.empty(scenes * n, 128) for _ in range(3)]
    sim().run([sim().attn_bwd(f32(d["q"]), f32(d["k"]), f32(d["v"]), f32(d["dout"]), *outs, scenes, n, sc)], None)
    for a, b in zip(got, outs):
        assert float((a - b.double()).abs().max()) <= 1e-6 * max(float(a.abs().max()), 1e-3)


# ------------------------------------------------------------------------------------------------ activations, sums
@pytest.mark.parametrize("count", [1, 300])
@pytest.mark.parametrize("kind", [T.ACT_GELU, T.ACT_SILU, T.ACT_LEAKY01])
def test_act_bwd(kind, count):
    d = T.act_inputs(count, seed=count)
    got = T.act_bwd(d["x"], d["dy"], kind)
    x = d64(d["x"], True)
    fwd = {T.ACT_GELU: F.gelu, T.ACT_SILU: F.silu, T.ACT_LEAKY01: lambda t: F.leaky_relu(t, 0.1)}[kind]
    want, = torch.autograd.grad(fwd(x), x, d64(d["dy"]))
    if kind == T.ACT_LEAKY01:
        at0 = torch.as_tensor(d["x"] == 0)
        assert at0.any() and (got[at0] == 0.1 * d64(d["dy"])[at0]).all()               # slope 0.1 at x = 0, stated by the issue
        got, want = got[~at0], want[~at0]                                              # (torch's own choice at 0 is not the reference)
        if not len(got):
            return
    assert rel(got, want) < 1e-12
    if kind != T.ACT_LEAKY01:                                                           # the simulator has no LeakyReLU
        out = torch.empty(count)
        sim().run([sim().act_bwd(f32(d["x"]), f32(d["dy"]), out, kind)], None)
        assert rel(T.act_bwd(d["x"], d["dy"], kind), out) < 1e-6


@pytest.mark.parametrize("m,n", [(1, 1), (37, 5)])
def test_colsum(m, n):
    x = T.noise((m, n), seed=m)
    got = T.colsum(x)
    b = torch.zeros(n, dtype=F64, requires_grad=True)
    want, = torch.autograd.grad(torch.zeros(m, n, dtype=F64) + b, b, d64(x))          # the gradient of a broadcast bias is a column sum
    assert rel(got, want) < 1e-12
    out = torch.empty(n)
    sim().run([sim().colsum(f32(x), out)], None)
    assert rel(got, out) < 1e-6


# ------------------------------------------------------------------------------------------------ generator properties
def test_exact_sum_inputs_sum_exactly_in_fp32_in_any_order():
    """the largest column the GPU tests sum has 16640 rows: every partial sum is an integer of magnitude <= 16640 * 8 < 2^24"""
    x = T.small_ints((16640, 64), seed=1)
    assert (x == np.round(x)).all() and np.abs(x).max() <= T.INT_MAX_ABS
    assert 16640 * T.INT_MAX_ABS < 2 ** 24
    a = x.sum(0, dtype=np.float32)
    b = x[::-1].astype(np.float64).sum(0)
    assert (a.astype(np.float64) == b).all() and np.abs(b).max() > 0


@pytest.mark.parametrize("kind", ["random", "shifted", "saturated"])
def test_no_groupnorm_or_layernorm_input_row_is_constant(kind):
    for scenes, n in [(2, 1), (2, 21), (3, 12), (2, 160)]:
        z = T.gn_inputs(scenes, n, T.SS_PER_TOKEN, seed=n, kind=kind)["z"]
        tiles = z.reshape(scenes, n, 8, 64).transpose(0, 2, 1, 3).reshape(scenes * 8, -1)
        assert (tiles.max(1) > tiles.min(1)).all()
    if kind != "saturated":
        x = T.ln_inputs(2049, seed=3, kind=kind)["x"]
        assert (x.max(1) > x.min(1)).all()


def test_saturation_inputs_reach_both_ends_in_every_group():
    scenes, n = 2, 21
    d = T.gn_inputs(scenes, n, T.SS_PER_TOKEN, seed=5, kind="saturated")
    u = T.gn_u(d["z"], d["gamma"], d["beta"], d["ss"], T.SS_PER_TOKEN, scenes, n)[3].reshape(scenes, n, 8, 64)
    assert float(u.max()) > 90 and float(u.min()) < -90
    hi, lo, mid = (u > 90).sum(dim=(1, 3)), (u < -90).sum(dim=(1, 3)), (u.abs() < 5).sum(dim=(1, 3))
    assert (hi > 0).all() and (lo > 0).all() and (mid > 0).all()                       # no (scene, group) tile vanishes
    # float64 du there: 0 below -90, dy above +90
    dss = T.gn_silu_bwd(d["z"], d["dy"], d["gamma"], d["beta"], d["ss"], T.SS_PER_TOKEN, scenes, n)[2][:, T.C:]
    u2, dy = u.reshape(scenes * n, T.C), d64(d["dy"])
    assert float(dss[u2 < -90].abs().max()) < 1e-30 and float((dss - dy)[u2 > 90].abs().max()) < 1e-30


def test_act_inputs_hold_the_special_points():
    x = T.act_inputs(257, seed=2)["x"]
    for v in (0.0, 1e-4, -1e-4, 30.0, -30.0):
        assert (x == np.float32(v)).any()
