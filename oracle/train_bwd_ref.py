"""Closed-form backward of every operation csrc/train.hip implements by hand, one plain function per entry point.

The formulas are the ones in the comments of train.hip, written out term by term (nothing here calls autograd);
tests/test_train_bwd_ref_host.py pins each of them against torch.autograd of the forward definition in float64 and against the
SimBackend of tests/plan_sim.py.  Every function takes ``dtype``: torch.float64 is the oracle, torch.float32 the plain CPU float32
evaluation of the same statement that tests/test_gpu_train_kernels.py uses as its error yardstick.  Inputs are cast to ``dtype``
first and results stay in it.

The input generators of the GPU tests live here too, so that the host test can assert the properties the GPU tests rely on.
"""
import math

import numpy as np
import torch

ACT_NONE, ACT_GELU, ACT_SILU, ACT_LEAKY01 = 0, 1, 2, 3
SS_NONE, SS_PER_TOKEN, SS_PER_SCENE, SS_PER_SLOT = 0, 1, 2, 3
EPS = 1e-5
C = 512                 # channels of GroupNorm / LayerNorm
GROUPS = 8
HEADS, DH = 4, 32


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to("cpu", dtype)


# ------------------------------------------------------------------------------------------------ GroupNorm + scale/shift + SiLU
def ss_rows(ss, ss_mode, scenes, n_tok):
    """scale/shift rows per token [M, 2C] for the conditioning modes (None for SS_NONE)."""
    if ss is None or ss_mode == SS_NONE:
        return None
    if ss_mode == SS_PER_TOKEN:
        return ss
    if ss_mode == SS_PER_SCENE:
        return ss[:, None, :].expand(scenes, n_tok, ss.shape[1]).reshape(scenes * n_tok, -1)
    if ss_mode == SS_PER_SLOT:
        return ss[None, :, :].expand(scenes, n_tok, ss.shape[1]).reshape(scenes * n_tok, -1)
    raise ValueError(ss_mode)


def gn_u(z, gamma, beta, ss, ss_mode, scenes, n_tok, eps=EPS, dtype=torch.float64):
    """-> (xh, gh, s1, u, rs): the SiLU argument u = (gamma * xh + beta) * (1 + scale) + shift and what it is made of."""
    z, gamma, beta, ss = (_t(a, dtype) for a in (z, gamma, beta, ss))
    M, ch = z.shape
    zz = z.reshape(scenes, n_tok, GROUPS, ch // GROUPS)
    cnt = n_tok * (ch // GROUPS)
    mu = zz.sum(dim=(1, 3), keepdim=True) / cnt
    d = zz - mu
    var = (d * d).sum(dim=(1, 3), keepdim=True) / cnt
    rs = 1.0 / torch.sqrt(var + eps)
    xh = (d * rs).reshape(M, ch)
    gh = gamma * xh + beta
    rows = ss_rows(ss, ss_mode, scenes, n_tok)
    if rows is None:
        s1, sh = torch.ones_like(gh), torch.zeros_like(gh)
    else:
        s1, sh = 1.0 + rows[:, :ch], rows[:, ch:]
    return xh, gh, s1, gh * s1 + sh, rs


def gn_silu_bwd(z, dy, gamma, beta, ss, ss_mode, scenes, n_tok, eps=EPS, dtype=torch.float64):
    """-> dz [M, C], part [scenes, 3C] = [dbias | dgamma | dbeta] per scene, dss ([scenes, 2C] for SS_PER_SCENE, [M, 2C] per token for
    SS_PER_TOKEN and SS_PER_SLOT, None for SS_NONE) = [dscale | dshift]."""
    dy = _t(dy, dtype)
    gamma_t = _t(gamma, dtype)
    xh, gh, s1, u, rs = gn_u(z, gamma, beta, ss, ss_mode, scenes, n_tok, eps, dtype)
    M, ch = xh.shape
    sig = torch.sigmoid(u)
    du = dy * (sig * (1.0 + u * (1.0 - sig)))
    dgh = du * s1
    dxh = dgh * gamma_t
    cnt = n_tok * (ch // GROUPS)

    def gmean(t):
        return t.reshape(scenes, n_tok, GROUPS, ch // GROUPS).sum(dim=(1, 3), keepdim=True) / cnt
    m1, m2 = gmean(dxh), gmean(dxh * xh)
    g4 = (scenes, n_tok, GROUPS, ch // GROUPS)
    dz = (rs * (dxh.reshape(g4) - m1 - xh.reshape(g4) * m2)).reshape(M, ch)

    def tok_sum(t):
        return t.reshape(scenes, n_tok, ch).sum(dim=1)
    part = torch.cat([tok_sum(dz), tok_sum(dgh * xh), tok_sum(dgh)], dim=1)
    dss = None
    if ss is not None and ss_mode != SS_NONE:
        dss = torch.cat([du * gh, du], dim=1)
        if ss_mode == SS_PER_SCENE:
            dss = dss.reshape(scenes, n_tok, 2 * ch).sum(dim=1)
    return dz, part, dss


# ------------------------------------------------------------------------------------------------ row normalisations
def ws_bwd(w, g, eps=EPS, dtype=torch.float64):
    """weight standardisation wh = (w - mean) * rs per row; g = d/d wh -> d/d w [rows, cols]."""
    w, g = _t(w, dtype), _t(g, dtype)
    n = w.shape[1]
    mean = w.sum(dim=1, keepdim=True) / n
    d = w - mean
    rs = 1.0 / torch.sqrt((d * d).sum(dim=1, keepdim=True) / n + eps)
    wh = d * rs
    m1 = g.sum(dim=1, keepdim=True) / n
    m2 = (g * wh).sum(dim=1, keepdim=True) / n
    return rs * (g - m1 - wh * m2)


def layernorm_bwd(x, g, dy, addend=None, eps=EPS, dtype=torch.float64):
    """y = xh * g per row -> dx (+ addend) [m, d], dg [d]."""
    x, g, dy, addend = (_t(a, dtype) for a in (x, g, dy, addend))
    n = x.shape[1]
    mean = x.sum(dim=1, keepdim=True) / n
    d = x - mean
    rs = 1.0 / torch.sqrt((d * d).sum(dim=1, keepdim=True) / n + eps)
    xh = d * rs
    h = dy * g
    m1 = h.sum(dim=1, keepdim=True) / n
    m2 = (h * xh).sum(dim=1, keepdim=True) / n
    dx = rs * (h - m1 - xh * m2)
    if addend is not None:
        dx = dx + addend
    return dx, (dy * xh).sum(dim=0)


# ------------------------------------------------------------------------------------------------ attention cores
def _heads(t, n):
    """[B*n, 128] -> [B, 4, n, 32]"""
    return t.reshape(-1, n, HEADS, DH).permute(0, 2, 1, 3)


def _rows(t):
    """[B, 4, n, 32] -> [B*n, 128]"""
    B, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * n, h * d)


def _softmax(t, dim):
    e = torch.exp(t - t.max(dim=dim, keepdim=True).values)
    return e / e.sum(dim=dim, keepdim=True)


def linear_attention_bwd(q, k, v, dout, scenes, nq, nk, scale, dtype=torch.float64):
    """out[i][e] = sum_d ctx[d][e] qs[i][d], ctx[d][e] = sum_j ks[j][d] v[j][e], qs = scale * softmax_d q, ks = softmax_j k
    -> dq [B*nq, 128], dk, dv [B*nk, 128]."""
    q, k, v, dout = (_t(a, dtype) for a in (q, k, v, dout))
    qh, do = _heads(q, nq), _heads(dout, nq)                    # [B, 4, nq, 32]
    kh, vh = _heads(k, nk), _heads(v, nk)                       # [B, 4, nk, 32]
    qs = _softmax(qh, -1) * scale
    ks = _softmax(kh, -2)
    ctx = torch.einsum("bhjd,bhje->bhde", ks, vh)
    dctx = torch.einsum("bhid,bhie->bhde", qs, do)
    dqs = torch.einsum("bhie,bhde->bhid", do, ctx)
    dq = qs * (dqs - (dqs * qs).sum(dim=-1, keepdim=True) / scale)
    dks = torch.einsum("bhje,bhde->bhjd", vh, dctx)
    dv = torch.einsum("bhjd,bhde->bhje", ks, dctx)
    dk = ks * (dks - (dks * ks).sum(dim=-2, keepdim=True))
    return _rows(dq), _rows(dk), _rows(dv)


def attention_bwd(q, k, v, dout, scenes, n, scale, dtype=torch.float64):
    """out[i] = sum_j p[i][j] v[j], p = softmax_j (scale q[i] . k[j]) -> dq, dk, dv [B*n, 128]."""
    q, k, v, dout = (_t(a, dtype) for a in (q, k, v, dout))
    qh, kh, vh, do = (_heads(t, n) for t in (q, k, v, dout))
    p = _softmax(torch.einsum("bhid,bhjd->bhij", qh * scale, kh), -1)
    dv = torch.einsum("bhij,bhid->bhjd", p, do)
    dp = torch.einsum("bhid,bhjd->bhij", do, vh)
    ds = p * (dp - (p * dp).sum(dim=-1, keepdim=True))
    dq = torch.einsum("bhij,bhjd->bhid", ds, kh) * scale
    dk = torch.einsum("bhij,bhid->bhjd", ds, qh) * scale
    return _rows(dq), _rows(dk), _rows(dv)


# ------------------------------------------------------------------------------------------------ activations, sums
def act_grad(x, kind):
    if kind == ACT_GELU:                                       # Phi(x) + x phi(x), exact erf
        return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))
    if kind == ACT_SILU:
        sig = torch.sigmoid(x)
        return sig * (1.0 + x * (1.0 - sig))
    if kind == ACT_LEAKY01:                                    # slope 0.1 at x = 0
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.1))
    raise ValueError(kind)


def act_bwd(x, dy, kind, dtype=torch.float64):
    x, dy = _t(x, dtype), _t(dy, dtype)
    return dy * act_grad(x, kind)


def colsum(x, dtype=torch.float64):
    return _t(x, dtype).sum(dim=0)


def gemm_tn(a, dy, kvalid=None, dtype=torch.float64):
    """weight gradient out[n][k] = sum_m dy[m][n] a[m][k] over the first ``kvalid`` columns of a, and dbias[n] = sum_m dy[m][n]"""
    a, dy = _t(a, dtype), _t(dy, dtype)
    return dy.t() @ a[:, :kvalid], dy.sum(dim=0)


# ================================================================================================ input generators (float32 numpy)
def noise(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


INT_MAX_ABS = 8


def small_ints(shape, seed):
    """integers in [-8, 8]: a sum of up to 2^24 / 8 of them is exact in fp32 in any order (every partial sum is an integer < 2^24)"""
    return np.random.RandomState(seed).randint(-INT_MAX_ABS, INT_MAX_ABS + 1, shape).astype(np.float32)


def gn_inputs(scenes, n_tok, ss_mode, seed, kind="random"):
    """-> dict(z, dy [M, C], gamma, beta [C], ss (rows by mode, 2C) or None).  kind: 'random' | 'shifted' (z = 100 + 0.01 noise) |
    'saturated' (beta + shift make u span -100 .. +100 inside EVERY group of 64 channels, so that no (scene, group) tile vanishes)."""
    M = scenes * n_tok
    z = noise((M, C), seed)
    if kind == "shifted":
        z = (100.0 + 0.01 * z).astype(np.float32)
    d = dict(z=z, dy=noise((M, C), seed + 1), gamma=(1.0 + 0.1 * noise((C,), seed + 2)).astype(np.float32),
             beta=noise((C,), seed + 3, 0.1), ss=None)
    rows = {SS_NONE: 0, SS_PER_TOKEN: M, SS_PER_SCENE: scenes, SS_PER_SLOT: n_tok}[ss_mode]
    if rows:
        d["ss"] = noise((rows, 2 * C), seed + 4, 0.5)
    if kind == "saturated":
        assert rows
        c = np.arange(C)
        ramp = ((((c % 64) * 8 + c // 64) / 511.0) * 2.0 - 1.0).astype(np.float32)      # -1 .. 1 within every group
        d["beta"] = (50.0 * ramp).astype(np.float32)
        d["ss"][:, :C] *= 0.1
        d["ss"][:, C:] = 50.0 * ramp + 0.1 * d["ss"][:, C:]
    return d


def ln_inputs(m, seed, kind="random"):
    x = noise((m, C), seed, 2.0) + np.float32(0.3)
    if kind == "shifted":
        x = (50.0 + 0.01 * noise((m, C), seed)).astype(np.float32)
    return dict(x=x.astype(np.float32), g=(1.0 + 0.1 * noise((C,), seed + 1)).astype(np.float32), dy=noise((m, C), seed + 2),
                addend=noise((m, C), seed + 3))


def ws_inputs(rows, cols, seed, kind="random"):
    """kind 'edges' (rows >= 2): row 0 constant (variance 0), row 1 = 100 + 0.01 noise"""
    w = noise((rows, cols), seed, 0.3) + np.float32(0.05)
    if kind == "edges":
        w[0, :] = 0.5
        w[1, :] = 100.0 + 0.01 * noise((cols,), seed + 9)
    return dict(w=w.astype(np.float32), g=noise((rows, cols), seed + 1))


def attn_inputs(scenes, nq, nk, seed, qk_scale=1.0):
    """-> q, dout [B*nq, 128]; k, v [B*nk, 128]"""
    return dict(q=noise((scenes * nq, 128), seed, 2.0 * qk_scale), k=noise((scenes * nk, 128), seed + 1, 2.0 * qk_scale),
                v=noise((scenes * nk, 128), seed + 2, 2.0), dout=noise((scenes * nq, 128), seed + 3))


ACT_SPECIALS = np.array([0.0, 1e-4, -1e-4, 30.0, -30.0], np.float32)


def act_inputs(count, seed):
    """x holds 0, +-1e-4, +-30 (as many as fit) in front of noise * 3"""
    x = noise((count,), seed, 3.0)
    k = min(count, len(ACT_SPECIALS))
    x[:k] = ACT_SPECIALS[:k]
    return dict(x=x, dy=noise((count,), seed + 1))
