"""CPU only: the float64 statements of oracle/blocks_ref.py are what they claim to be, and the cases and inputs of
tests/test_gpu_blocks_kernels.py have the properties that module relies on.

Every statement is compared with torch's own float64 operator of the same operation (1e-12 of the tensor maximum)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import blocks_ref as B
from oracle import ref_torch as R
from test_gpu_train_kernels import rows_, slabs, whole

F32, F64 = torch.float32, torch.float64


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def d64(a):
    return torch.tensor(np.asarray(a), dtype=F64)


def chan_first(t, n):
    """[B*n, 128] -> (B, h, c, n), the layout of oracle.ref_torch"""
    return d64(t).reshape(-1, n, 4, 32).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ the statements
@pytest.mark.parametrize("rows,cols", [(3, 5), (2, 257), (2, 2048)])
def test_weight_standardize_is_var_unbiased_false(rows, cols):
    w = B.ws_case([(rows, cols)])[0]
    got = B.weight_standardize(w)
    assert got.dtype == F64 and B.weight_standardize(w, dtype=F32).dtype == F32
    wd = d64(w)
    ref = (wd - wd.mean(1, keepdim=True)) * (wd.var(1, unbiased=False, keepdim=True) + B.EPS).rsqrt()
    assert rel(got, ref) < 1e-12


@pytest.mark.parametrize("m,kind", [(1, "random"), (5, "random"), (9, "shifted"), (5, "constant")])
def test_layernorm_is_f_layer_norm_times_gain(m, kind):
    d = B.layernorm_case(m, kind)
    x, g, r = d64(d["x"]), d64(d["g"]), d64(d["residual"])
    ref = F.layer_norm(x, (B.C,), eps=B.EPS) * g
    assert rel(B.layernorm(d["x"], d["g"]), ref) < 1e-12
    assert rel(B.layernorm(d["x"], d["g"], d["residual"]), ref + r) < 1e-12
    assert B.layernorm(d["x"], d["g"], d["residual"], dtype=F32).dtype == F32


@pytest.mark.parametrize("scenes,nq,nk", [(2, 3, 7), (2, 5, 1), (2, 65, 9), (1, 12, 12)])
def test_linear_attention_is_einsum_softmax_and_the_reference_core(scenes, nq, nk):
    d = B.linear_attention_case(scenes, nq, nk)
    got = B.linear_attention(d["q"], d["k"], d["v"], scenes, nq, nk, B.SCALE)
    q, k, v = chan_first(d["q"], nq), chan_first(d["k"], nk), chan_first(d["v"], nk)
    core = R._linear_attention_core(q, k, v).permute(0, 2, 1).reshape(scenes * nq, 128)
    assert rel(got, core) < 1e-12
    ctx = torch.einsum("bhdn,bhen->bhde", k.softmax(-1), v)
    ref = torch.einsum("bhde,bhdn->bhne", ctx, q.softmax(-2) * B.SCALE).permute(0, 2, 1, 3).reshape(scenes * nq, 128)
    assert rel(got, ref) < 1e-12


@pytest.mark.parametrize("scenes,n", [(2, 1), (2, 17), (1, 65)])
def test_attention_is_einsum_softmax(scenes, n):
    d = B.attention_case(scenes, n)
    got = B.attention(d["q"], d["k"], d["v"], scenes, n, B.SCALE)
    q, k, v = chan_first(d["q"], n) * B.SCALE, chan_first(d["k"], n), chan_first(d["v"], n)
    attn = torch.einsum("bhdi,bhdj->bhij", q, k).softmax(-1)
    ref = torch.einsum("bhij,bhdj->bhid", attn, v).permute(0, 2, 1, 3).reshape(scenes * n, 128)
    assert rel(got, ref) < 1e-12


def test_activations_are_f_gelu_silu_leaky_relu():
    x = B.activation_case(300)
    xd = d64(x)
    assert torch.equal(B.activation(x, B.ACT_NONE), xd)
    assert rel(B.activation(x, B.ACT_GELU), F.gelu(xd)) < 1e-12
    assert rel(B.activation(x, B.ACT_SILU), F.silu(xd)) < 1e-12
    assert torch.equal(B.activation(x, B.ACT_LEAKY01), F.leaky_relu(xd, 0.1))
    assert torch.equal(B.activation(x, B.ACT_LEAKY01, dtype=F32), F.leaky_relu(torch.from_numpy(x), 0.1))
    # the special points are where a formula (not the function) breaks: 0.5 x (1 + erf) and x / (1 + exp(-x)) stay finite at +-90
    for act in (B.ACT_GELU, B.ACT_SILU):
        for dt in (F32, F64):
            assert torch.isfinite(B.activation(B.ACT_FWD_SPECIALS, act, dtype=dt)).all()


@pytest.mark.parametrize("act", sorted(B.ACTS))
def test_linear_smallk_is_matmul_bias_activation(act):
    d = B.smallk_case(33, 9, 40)
    z = d64(d["x"]) @ d64(d["w"]).T
    f = {"none": lambda a: a, "gelu": F.gelu, "silu": F.silu, "leaky": lambda a: F.leaky_relu(a, 0.1)}[act]
    assert rel(B.linear_smallk(d["x"], d["w"], None, B.ACTS[act]), f(z)) < 1e-12
    assert rel(B.linear_smallk(d["x"], d["w"], d["bias"], B.ACTS[act]), f(z + d64(d["bias"]))) < 1e-12


def test_time_embedding_is_the_sinusoidal_embedding_inside_the_table():
    """ref_torch.sinusoidal_embedding forms the same float32 product and takes sin / cos of it in float32: the float32 and the float64
    evaluation of the statement both equal it to float32 rounding of values in [-1, 1].  The frequencies are the embedding's own
    float32 vector; those of time_case are the same numbers to one ulp (float64 exp, rounded once)."""
    t = np.array([0, 1, 17, 999], np.int64)
    for dim in (6, 512):
        ref = R.sinusoidal_embedding(torch.from_numpy(t), dim)
        half = dim // 2
        fr = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1))).numpy()
        assert np.abs(fr - B.time_case(dim)["freq"]).max() <= 2.0 ** -23 * np.abs(fr).max()
        got32, got64 = B.time_embedding(t, dim, fr, dtype=F32), B.time_embedding(t, dim, fr)
        assert got32.dtype == F32 and got64.dtype == F64 and got64.shape == (4, dim)
        assert float((got32 - ref).abs().max()) <= 2.0 ** -22
        assert float((got64 - ref.double()).abs().max()) <= 2.0 ** -22
    # dim = 2: one frequency, 1.0; the argument of t = 1500 is exactly 1500
    d = B.time_case(2)
    assert d["freq"].tolist() == [1.0]
    assert rel(B.time_embedding(d["t"], 2, d["freq"])[3], torch.tensor([math.sin(1500.0), math.cos(1500.0)], dtype=F64)) < 1e-15


# ------------------------------------------------------------------------------------------------ what the GPU module relies on
def is_constant(rows):
    return (rows == rows[:, :1]).all(1)


def test_no_random_or_shifted_row_is_constant_and_the_constant_row_is():
    for m in B.LN_M:
        assert not is_constant(B.layernorm_case(m)["x"]).any()
    for m, kind in B.LN_EDGES:
        x = B.layernorm_case(m, kind)["x"]
        const = is_constant(x)
        if kind == "constant":
            assert const.tolist() == [i == B.ln_const_row(m) for i in range(m)] and m >= 3
            assert (x[B.ln_const_row(m)] == np.float32(B.LN_CONST_VALUE)).all()
        else:
            assert not const.any()
            assert np.abs(x - 50.0).max() < 0.1 and x.std(1).min() > 1e-3          # mean >> spread, and a spread
    from diffuscene_amd import _lib
    for shapes in ([[s] for s in B.WS_SINGLE] + [B.WS_RAGGED, B.ws_chunked_shapes(_lib.WS_MAX)]):
        for w in B.ws_case(shapes):
            assert w.shape[1] == 1 or not is_constant(w).any()
    for cols in B.WS_EDGE_COLS:
        w = B.ws_case([(3, cols)], "edges")[0]
        assert is_constant(w).tolist() == [True, False, False] and (w[0] == np.float32(0.5)).all()
        assert np.abs(w[1] - 100.0).max() < 0.1 and w[1].std() > 1e-3


def test_large_logit_cases_saturate_both_softmaxes_and_stay_finite_in_float32():
    for scenes, nq, nk in B.LINATTN_LARGE:
        d = B.linear_attention_case(scenes, nq, nk, large=True)
        qs, ks = B.linear_attention_probs(d["q"], d["k"], nq, nk)
        assert float(qs.max()) > 0.999 and float(ks.max()) > 0.999
        assert np.abs(d["k"]).max() > 89 and np.abs(d["q"]).max() > 89                # exp overflows float32 without the maximum
        t32 = B.linear_attention(d["q"], d["k"], d["v"], scenes, nq, nk, B.SCALE, dtype=F32)
        assert t32.dtype == F32 and torch.isfinite(t32).all()
    for scenes, n in B.ATTN_LARGE:
        d = B.attention_case(scenes, n, large=True)
        p = B.attention_probs(d["q"], d["k"], n, B.SCALE)
        assert float(p.max()) > 0.999
        logits = torch.einsum("bhid,bhjd->bhij", B._heads(d64(d["q"]), n) * B.SCALE, B._heads(d64(d["k"]), n))
        assert float(logits.max()) > 89
        t32 = B.attention(d["q"], d["k"], d["v"], scenes, n, B.SCALE, dtype=F32)
        assert t32.dtype == F32 and torch.isfinite(t32).all()


def nonzero_units(ref64, units, what, vanishing=()):
    """every unit has max|ref64| > 0, except exactly the listed ones, which are identically zero"""
    u = np.abs(units(np.asarray(ref64, np.float64))).max(1)
    zero = sorted(np.nonzero(u <= 1e-12)[0].tolist())
    assert zero == sorted(vanishing), (what, zero, vanishing)
    assert all(u[i] == 0.0 for i in zero), what


def test_every_unit_of_every_case_has_a_scale_unless_listed_as_vanishing():
    from diffuscene_amd import _lib
    for scenes, n in B.ATTN_N:
        d = B.attention_case(scenes, n)
        nonzero_units(B.attention(d["q"], d["k"], d["v"], scenes, n, B.SCALE), slabs(scenes, n), ("attention", n))
    for scenes, n in B.ATTN_LARGE:
        d = B.attention_case(scenes, n, large=True)
        nonzero_units(B.attention(d["q"], d["k"], d["v"], scenes, n, B.SCALE), slabs(scenes, n), ("attention large", n))
    for large, cases in ((False, B.LINATTN), (True, B.LINATTN_LARGE)):
        for scenes, nq, nk in cases:
            d = B.linear_attention_case(scenes, nq, nk, large)
            nonzero_units(B.linear_attention(d["q"], d["k"], d["v"], scenes, nq, nk, B.SCALE), slabs(scenes, nq), ("linattn", nq, nk))
    for m, kind in [(m, "random") for m in B.LN_M] + B.LN_EDGES:
        d = B.layernorm_case(m, kind)
        nonzero_units(B.layernorm(d["x"], d["g"]), rows_, ("layernorm", m, kind), [B.ln_const_row(m)] if kind == "constant" else [])
        nonzero_units(B.layernorm(d["x"], d["g"], d["residual"]), rows_, ("layernorm residual", m, kind))
    for shapes in ([[s] for s in B.WS_SINGLE] + [B.WS_RAGGED, B.ws_chunked_shapes(_lib.WS_MAX)]):
        for (r, c), w in zip(shapes, B.ws_case(shapes)):
            nonzero_units(B.weight_standardize(w), rows_, ("ws", r, c), list(range(r)) if c == 1 else [])        # one column: w - mean = 0
    for cols in B.WS_EDGE_COLS:
        nonzero_units(B.weight_standardize(B.ws_case([(3, cols)], "edges")[0]), rows_, ("ws edges", cols), [0])
    for m, k in B.SMALLK_CROSS:
        d = B.smallk_case(m, k, B.SMALLK_N)
        nonzero_units(B.linear_smallk(d["x"], d["w"], d["bias"], B.ACT_GELU), rows_, ("smallk", m, k))
    for n, act, with_bias in B.SMALLK_WIDTHS:
        d = B.smallk_case(33, 9, n)
        nonzero_units(B.linear_smallk(d["x"], d["w"], d["bias"] if with_bias else None, B.ACTS[act]), rows_, ("smallk n", n))
    for i, k in enumerate(B.SMALLK_GROUP_K):
        d = B.smallk_case(33, k, B.SMALLK_N, seed=i)
        nonzero_units(B.linear_smallk(d["x"], d["w"], d["bias"], B.ACT_GELU), rows_, ("smallk grouped", k))
    for count in B.ACT_COUNTS:
        x = B.activation_case(count)
        assert set(B.ACT_FWD_SPECIALS[:count].tolist()) <= set(x.tolist())
        for act in (B.ACT_GELU, B.ACT_SILU):
            nonzero_units(B.activation(x, act), whole, ("activation", act, count))
            if count > len(B.ACT_FWD_SPECIALS):
                nonzero_units(B.activation(x[len(B.ACT_FWD_SPECIALS):], act), whole, ("activation noise", act, count))
    for dim in B.TIME_DIMS:
        d = B.time_case(dim)
        assert d["t"].tolist() == [0, B.TIME_TABLE_ROWS - 1, B.TIME_TABLE_ROWS, 1500, -3]
        nonzero_units(B.time_embedding(d["t"], dim, d["freq"]), rows_, ("time", dim))
        assert not np.array_equal(d["table"][[0, -1]], B.time_embedding(d["t"][:2], dim, d["freq"], dtype=F32).numpy())
