"""Plain statements of every forward operation csrc/blocks.hip implements by hand, one function per entry point.

Every function takes float32 numpy (or tensors) and ``dtype``: torch.float64 is the oracle, torch.float32 the plain CPU float32
evaluation of the same statement that tests/test_gpu_blocks_kernels.py uses as its error yardstick (the convention of
oracle/train_bwd_ref.py, whose helpers and input generators are reused).  tests/test_blocks_ref_host.py pins each statement to
torch's own float64 operators.

The case lists and input builders of the GPU module live here too, so that the host test can assert, over exactly the inputs the
GPU tests launch, the properties those tests rely on.
"""
import math

import numpy as np
import torch

from .train_bwd_ref import (ACT_GELU, ACT_LEAKY01, ACT_NONE, ACT_SILU, ACT_SPECIALS, C, EPS, _heads, _rows, _softmax, _t,  # noqa: F401
                            act_inputs, attn_inputs, ln_inputs, noise, ws_inputs)

ACTS = {"none": ACT_NONE, "gelu": ACT_GELU, "silu": ACT_SILU, "leaky": ACT_LEAKY01}
SCALE = 32 ** -0.5          # dim_head ** -0.5 of both attentions


# ------------------------------------------------------------------------------------------------ row normalisations
def weight_standardize(w, eps=EPS, dtype=torch.float64):
    """(w - mean_row) / sqrt(var_row + eps), biased variance -> [rows, cols]"""
    w = _t(w, dtype)
    n = w.shape[1]
    mean = w.sum(dim=1, keepdim=True) / n
    d = w - mean
    var = (d * d).sum(dim=1, keepdim=True) / n
    return d / torch.sqrt(var + eps)


def layernorm(x, g, residual=None, eps=EPS, dtype=torch.float64):
    """(x - mean_row) / sqrt(var_row + eps) * g (+ residual) -> [m, d]"""
    x, g, residual = (_t(a, dtype) for a in (x, g, residual))
    n = x.shape[1]
    mean = x.sum(dim=1, keepdim=True) / n
    d = x - mean
    var = (d * d).sum(dim=1, keepdim=True) / n
    y = d / torch.sqrt(var + eps) * g
    return y if residual is None else y + residual


# ------------------------------------------------------------------------------------------------ attention cores
def linear_attention_probs(q, k, nq, nk, dtype=torch.float64):
    """-> softmax of q over the 32 head channels [B, 4, nq, 32], softmax of k over the tokens [B, 4, nk, 32]"""
    return _softmax(_heads(_t(q, dtype), nq), -1), _softmax(_heads(_t(k, dtype), nk), -2)


def linear_attention(q, k, v, scenes, nq, nk, scale, dtype=torch.float64):
    """out[i][e] = sum_d ctx[d][e] qs[i][d], ctx[d][e] = sum_j ks[j][d] v[j][e], qs = scale * softmax_d q, ks = softmax_j k
    -> [B*nq, 128]"""
    qs, ks = linear_attention_probs(q, k, nq, nk, dtype)
    ctx = torch.einsum("bhjd,bhje->bhde", ks, _heads(_t(v, dtype), nk))
    return _rows(torch.einsum("bhde,bhid->bhie", ctx, qs * scale))


def attention_probs(q, k, n, scale, dtype=torch.float64):
    """p[i][j] = softmax_j (scale q[i] . k[j]) -> [B, 4, n, n]"""
    return _softmax(torch.einsum("bhid,bhjd->bhij", _heads(_t(q, dtype), n) * scale, _heads(_t(k, dtype), n)), -1)


def attention(q, k, v, scenes, n, scale, dtype=torch.float64):
    """out[i] = sum_j p[i][j] v[j] -> [B*n, 128]"""
    return _rows(torch.einsum("bhij,bhjd->bhid", attention_probs(q, k, n, scale, dtype), _heads(_t(v, dtype), n)))


# ------------------------------------------------------------------------------------------------ small-K linear, activation, time
def activation(x, act, dtype=torch.float64):
    x = _t(x, dtype)
    if act == ACT_NONE:
        return x
    if act == ACT_GELU:                                        # exact erf
        return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    if act == ACT_SILU:
        return x / (1.0 + torch.exp(-x))
    if act == ACT_LEAKY01:
        return torch.where(x > 0, x, 0.1 * x)
    raise ValueError(act)


def linear_smallk(x, w, bias, act, dtype=torch.float64):
    """act(x @ w^T + bias) -> [m, n]"""
    x, w, bias = (_t(a, dtype) for a in (x, w, bias))
    y = x @ w.t()
    return activation(y if bias is None else y + bias, act, dtype)


def time_embedding(t, dim, freq, dtype=torch.float64):
    """[sin(a) | cos(a)], a = float32(t) * freq: the argument is ONE float32 product, as the kernel forms it; sin and cos of that
    float32 number are taken in ``dtype`` -> [b, dim]"""
    arg = (np.asarray(t).astype(np.float32)[:, None] * np.asarray(freq, np.float32)[None, :dim // 2]).astype(np.float32)
    a = _t(arg, dtype)
    return torch.cat((torch.sin(a), torch.cos(a)), dim=-1)


# ================================================================================================ cases and inputs of the GPU module
ATTN_N = [(2, n) for n in (1, 2, 63, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129)] + [(1, 160)]
ATTN_LARGE = [(2, 17), (2, 129)]                            # q scaled by LARGE
LINATTN = [(1, 1, 1), (2, 3, 7), (2, 5, 1), (2, 64, 8), (2, 65, 9), (2, 63, 64), (3, 12, 77), (2, 129, 65), (2, 128, 129),
           (1, 160, 160)]
LINATTN_LARGE = [(2, 12, 12), (2, 65, 9)]                   # qk_scale = LARGE
LARGE = 30.0


def attention_case(scenes, n, large=False):
    d = attn_inputs(scenes, n, n, seed=n + 3 * n)
    if large:
        d["q"] = (d["q"] * np.float32(LARGE)).astype(np.float32)
    return d


def linear_attention_case(scenes, nq, nk, large=False):
    return attn_inputs(scenes, nq, nk, seed=nq + 3 * nk, qk_scale=LARGE if large else 1.0)


LN_M = [1, 3, 4, 5, 9]
LN_EDGES = [(9, "shifted"), (5, "constant")]
LN_CONST_VALUE = 0.5


def ln_const_row(m):
    return m // 2


def layernorm_case(m, kind="random"):
    """train_bwd_ref.ln_inputs ('random' | 'shifted': x = 50 + 0.01 noise); 'constant': row m // 2 of the random rows is constant.
    -> dict(x, g, residual)"""
    d = ln_inputs(m, seed=m + 100, kind="random" if kind == "constant" else kind)
    if kind == "constant":
        d["x"][ln_const_row(m), :] = LN_CONST_VALUE
    return dict(x=d["x"], g=d["g"], residual=d["addend"])


WS_SINGLE = [(1, 1), (3, 5), (2, 255), (2, 256), (2, 257), (5, 2047), (2, 2048)]
WS_EDGE_COLS = [5, 256, 2048]
WS_RAGGED = [(1, 5), (70, 256), (3, 2047), (1, 2048), (70, 40), (2, 1), (7, 257)]
WS_EXTRA = 3                                                # items beyond DSC_WS_MAX in the chunked call


def ws_chunked_shapes(ws_max):
    return [(1 + i % 3, (5, 40, 9)[i % 3]) for i in range(ws_max + WS_EXTRA)]


def ws_case(shapes, kind="random"):
    """-> list of w [rows, cols]"""
    return [ws_inputs(r, c, seed=11 * i + c, kind=kind)["w"] for i, (r, c) in enumerate(shapes)]


SMALLK_N = 257
SMALLK_CROSS = [(m, k) for k in (1, 7, 8, 9, 63, 64) for m in (1, 31, 32, 33)]                        # at n = 257, bias, GELU
SMALLK_WIDTHS = [(1, "none", False), (255, "gelu", True), (256, "silu", False), (512, "leaky", True)]   # at m = 33, k_in = 9
SMALLK_GROUP_K = [1, 8, 25, 64]                              # DSC_SMALLK_MAX items, m = 33


def smallk_case(m, k_in, n, seed=0):
    s = seed + 1000 * m + 10 * k_in + n
    return dict(x=noise((m, k_in), s), w=noise((n, k_in), s + 1, 0.5), bias=noise((n,), s + 2))


ACT_COUNTS = [1, 255, 256, 257, 4096 * 256 + 3]
ACT_FWD_SPECIALS = np.concatenate([np.array([90.0, -90.0], np.float32), ACT_SPECIALS[::-1]]).astype(np.float32)


def activation_case(count):
    """train_bwd_ref.act_inputs with +-90 as well: x holds 90, -90, -30, 30, -1e-4, 1e-4, 0 (as many as fit) in front of noise * 3"""
    x = act_inputs(count, seed=count % 1000)["x"]
    k = min(count, len(ACT_FWD_SPECIALS))
    x[:k] = ACT_FWD_SPECIALS[:k]
    return x


TIME_DIMS = [2, 6, 512]
TIME_TABLE_ROWS = 8


def time_case(dim, rows=TIME_TABLE_ROWS):
    """-> t (first and last table row, then three values outside the table), freq [dim / 2], and a table of NOISE: a row taken from
    it cannot be mistaken for a computed one"""
    half = dim // 2
    freq = np.exp(np.arange(half, dtype=np.float64) * -(math.log(10000.0) / max(half - 1, 1))).astype(np.float32)
    t = np.array([0, rows - 1, rows, 1500, -3], np.int64)
    return dict(t=t, freq=freq, table=noise((rows, dim), dim))
