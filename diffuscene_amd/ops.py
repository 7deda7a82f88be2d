"""Tensor-level wrappers over the C ABI (include/diffuscene_hip.h).

PyTorch is used for device memory and streams only: every function takes CUDA(HIP) fp32 tensors,
passes raw device pointers + the current torch stream to libdiffuscene_hip.so and returns the output
tensor.  There is no CPU path: a CPU tensor raises.
"""
import collections
import ctypes as C
import numbers

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_NONE, ACT_SILU, MEAN_EPS, MEAN_V, MEAN_X0, SS_NONE, SS_PER_SCENE,  # noqa: F401
                   SS_PER_SLOT, SS_PER_TOKEN, GemmArgs, SplitItem, WsItem)


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, name="tensor", dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("diffuscene_amd: %s must live on a HIP device (no CPU fallback exists)" % name)
    if t.dtype != dtype:
        raise RuntimeError("diffuscene_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
    return t


def issue(rec, stream=None):
    """Run one launch record on ``stream`` (default: the current torch stream).  A record is what every ``*_rec`` function below returns:
    (entry point name, its arguments without the trailing stream, keep) -- ``keep`` lists everything a raw pointer among the arguments
    refers to (tensors, ctypes arrays and structs).  The eager wrappers issue their record at once; launch plans (engine.Plan,
    train_plan.HipBackend) store it and own ``keep``.  A ``*_rec`` function checks its operands and never allocates."""
    name, args, _ = rec
    _lib.check(_lib.fn(name)(*args, stream if stream is not None else stream_ptr()), name)


def _mat(t, name):
    """2-D row-major view with contiguous columns; returns (ptr, ld)."""
    _dev(t, name)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError("diffuscene_amd: %s must be a 2-D tensor with contiguous rows, got shape %s strides %s"
                           % (name, tuple(t.shape), t.stride()))
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def as2d(w):
    """(out, in, 1) conv weight or (out, in) linear weight -> (out, in) view."""
    return w.view(w.shape[0], w.shape[1]) if w.dim() == 3 else w


def make_gemm_args(a, w, y, bias=None, a2=None, residual=None, act_in=ACT_NONE, act_out=ACT_NONE,
                   gamma=None, beta=None, eps=1e-5, tokens_per_scene=0, scale_shift=None, ss_mode=SS_NONE, preact=None,
                   ss_index=None, w_planes=None, actgrad_x=None, gnb=None, row_invariant=False):
    """Build a dsc_gemm_args for  y = epi(act_in([a|a2]) @ w.T + bias).  The returned struct holds raw
    pointers only; the caller keeps the tensors alive.  ``w_planes``: the weight pre-split into bf16 planes (split_planes):
    the product runs on the bf16 matrix cores with f32 accuracy where the kernel supports the shape."""
    g = GemmArgs()
    g.a1, g.lda1 = _mat(a, "a")
    g.k1 = a.shape[1]
    if a2 is not None:
        g.a2, g.lda2 = _mat(a2, "a2")
        g.k2 = a2.shape[1]
        if a2.shape[0] != a.shape[0]:
            raise RuntimeError("a and a2 row mismatch")
    w2 = as2d(w)
    g.w, g.ldw = _mat(w2, "w")
    if w2.shape[1] != g.k1 + g.k2:
        raise RuntimeError("weight K (%d) != activation K (%d)" % (w2.shape[1], g.k1 + g.k2))
    g.m, g.n = a.shape[0], w2.shape[0]
    g.y, g.ldy = _mat(y, "y")
    if tuple(y.shape) != (g.m, g.n):
        raise RuntimeError("output shape %s != (%d, %d)" % (tuple(y.shape), g.m, g.n))
    if bias is not None:
        g.bias = _dev(bias, "bias").data_ptr()
    if residual is not None:
        g.residual, g.ldr = _mat(residual, "residual")
    g.act_in, g.act_out, g.batch = act_in, act_out, 1
    if row_invariant:                      # include/diffuscene_hip.h DSC_GEMM_ROW_INVARIANT: a row's result must not depend on the number of rows
        g.flags |= _lib.GEMM_ROW_INVARIANT
    if gamma is not None:
        g.gamma, g.beta, g.eps = _dev(gamma).data_ptr(), _dev(beta).data_ptr(), eps
        g.tokens_per_scene = tokens_per_scene
    if scale_shift is not None:
        g.scale_shift, g.ld_ss = _mat(scale_shift, "scale_shift")
        g.ss_mode = ss_mode
    if preact is not None:
        g.preact, g.ld_preact = _mat(preact, "preact")
    if actgrad_x is not None:              # y = product * act_out'(actgrad_x) (split kernel only; include/diffuscene_hip.h)
        g.actgrad_x, g.ld_actgrad = _mat(actgrad_x, "actgrad_x")
        if tuple(actgrad_x.shape) != (g.m, g.n):
            raise RuntimeError("actgrad_x shape %s != (%d, %d)" % (tuple(actgrad_x.shape), g.m, g.n))
    if gnb is not None:
        # GroupNorm-backward epilogue (include/diffuscene_hip.h, gnb_*): dict(z=, dgamma=, dbeta=, dbias=, pstride=, dss=None); gamma / beta / eps /
        # tokens_per_scene / scale_shift / ss_mode above describe the Block whose output gradient this product is
        g.gnb_z, g.ld_gnb_z = _mat(gnb["z"], "gnb z")
        g.gnb_dgamma, g.gnb_dbeta, g.gnb_dbias = gnb["dgamma"], gnb["dbeta"], gnb["dbias"]
        g.gnb_pstride = gnb["pstride"]
        if gnb.get("dss") is not None:
            g.gnb_dss, g.ld_gnb_dss = _mat(gnb["dss"], "gnb dss")
    if ss_index is not None:
        if scale_shift is None:
            raise RuntimeError("ss_index (DSC_SS_BY_INDEX) needs the scale_shift table it indexes")
        g.ss_index = _dev(ss_index, "ss_index", torch.int64).data_ptr()
        g.ss_rows = scale_shift.shape[0]              # the device clamps every gathered row into the table
    if w_planes is not None:
        # (3, n, K); a grouped launch (batch set by the caller afterwards) passes the planes of the stacked weights (3, batch n, K)
        if (w_planes.dtype != torch.int16 or w_planes.dim() != 3 or w_planes.shape[0] != 3 or w_planes.shape[1] % g.n
                or w_planes.shape[2] != g.k1 + g.k2 or not w_planes.is_contiguous()):
            raise RuntimeError("w_planes must be a contiguous int16 tensor of shape (3, %d, %d)" % (g.n, g.k1 + g.k2))
        attach_planes(g, w_planes, gn=gamma is not None and gnb is None)       # (gnb: a dense product that borrows the Block's gamma / beta)
    return g


PLANES_ROWMAJOR, PLANES_FRAGMENT = 0, 1


def planes_layout(g, gn=False):
    """Which layout of the weight's bf16 planes this launch wants (dsc_gemm_planes_layout): PLANES_ROWMAJOR (the block-staged split
    kernel), PLANES_FRAGMENT (the wave-autonomous kernel reads MFMA fragments straight from memory), or -1: the launch stays on the
    exact-f32 kernel whatever it is given (always so for a row_invariant launch).  Asked BEFORE planes are made; invalid arguments raise."""
    r = _lib.fn("dsc_gemm_planes_layout")(C.byref(g), 1 if gn else 0)
    if r == _lib.DSC_PLANES_NONE:          # the library's own value for it: -1 is DSC_EINVAL there
        return -1
    if r < 0:
        _lib.check(r, "dsc_gemm_planes_layout")
    return r


def fragment_major(planes):
    """Row-major planes (3, n, K) -> the same values fragment-major, [3][n/16][K/32][lane = (k-octet & 3) * 16 + row % 16][8] (kept in a
    tensor of the same shape)."""
    _, n, k = planes.shape
    return planes.view(3, n // 16, 16, k // 32, 4, 8).permute(0, 1, 3, 4, 2, 5).contiguous().view(3, n, k)


def attach_planes(g, planes, gn=False, layout=None):
    """Hand ``planes`` to the launch.  ``layout`` says how they are laid out (what split_planes(..., fragment=) made); None = row-major
    planes from an ad-hoc caller (tests, tools): where the library wants the other layout for this launch a converted copy is made
    once and kept on the tensor -- plans ask planes_layout() first and split straight into the layout they need."""
    want = planes_layout(g, gn)
    if layout is None:
        layout = getattr(planes, "_dsc_layout", PLANES_ROWMAJOR)
        if want == PLANES_FRAGMENT and layout == PLANES_ROWMAJOR:
            cached = getattr(planes, "_dsc_fragment", None)
            if cached is None or cached[0] != planes._version:
                cached = planes._dsc_fragment = (planes._version, fragment_major(planes))
            planes, layout = cached[1], PLANES_FRAGMENT
            g._planes_keep = planes                 # the struct holds a raw pointer: keep the converted copy with it
    g.w_planes = planes.data_ptr()
    g.w_planes_layout = layout
    return g


def planes_for(g, gn, w, planes_of):
    """The planes decision of one GEMM launch, on its finished dsc_gemm_args: ask the library which layout the launch wants, fetch the
    planes of weight operand ``w`` from the caller's cache -- ``planes_of(w, layout)`` -- and attach them in that layout.  Returns the
    planes, or None when the launch stays on the exact-f32 kernel or the cache has none for it."""
    lay = planes_layout(g, gn)
    pl = planes_of(w, lay) if lay >= 0 else None
    if pl is not None:
        attach_planes(g, pl, gn, layout=lay)
    return pl


def planes_wanted(n, k):
    """Shapes the split-bf16 GEMM path covers (gemm_split.hip): callers skip the plane copy for everything else."""
    return n % 128 == 0 and k % 32 == 0 and 6 * n * k < 0x7fffffff


def split_planes(items, stream=None):
    """Exact 3-way bf16 split of f32 matrices (dsc_split_bf16x3_f32).  items: [(w2d, planes, transpose)] with ``planes`` an int16
    tensor (3, rows, cols) -- or (3, cols, rows) when ``transpose`` -- or None (allocated).  Returns the planes tensors."""
    out, batch = [], []
    for w, planes, tr in items:
        tr = int(tr)                       # bit 0: planes of w^T; bit 1 (2): fragment-major output (PLANES_FRAGMENT)
        frag, tr = tr & 2, tr & 1
        w2 = as2d(_dev(w, "w"))
        r, c = w2.shape
        shape = (3, c, r) if tr else (3, r, c)
        if planes is None:
            planes = torch.empty(shape, device=w2.device, dtype=torch.int16)
        elif tuple(planes.shape) != shape or planes.dtype != torch.int16 or not planes.is_contiguous():
            raise RuntimeError("split_planes: planes must be contiguous int16 %s" % (shape,))
        planes._dsc_layout = PLANES_FRAGMENT if frag else PLANES_ROWMAJOR
        planes._dsc_fragment = None        # attach_planes' converted copy: the kernel writes through a raw pointer, planes._version does not move
        out.append(planes)
        batch.append((w2, planes, tr | frag))
    for i in range(0, len(batch), _lib.WS_MAX):
        issue(split_rec(batch[i:i + _lib.WS_MAX]), stream)
    return out


def split_rec(ents):
    """ents: <= DSC_WS_MAX of (w2d, planes, flags): the planes of w2d -- of its transpose with bit 0 of ``flags`` --, fragment-major with bit 1."""
    arr = (SplitItem * len(ents))()
    for j, (w, planes, flags) in enumerate(ents):
        arr[j].w, arr[j].ldw = _mat(w, "w")
        arr[j].rows, arr[j].cols = w.shape
        arr[j].planes, arr[j].transpose = planes.data_ptr(), flags
    return "dsc_split_bf16x3_f32", (arr, len(ents)), (arr, ents)


def gemm_uses_split(g, gn=False):
    """True when the library would run this launch on the split-bf16 kernel (its own dispatch decision, dsc_gemm_arithmetic)."""
    return _lib.fn("dsc_gemm_arithmetic")(C.byref(g), 1 if gn else 0) == 1


def gemm_would_use_split(g, gn=False):
    """The same question BEFORE any planes exist: would this launch take the split path if the weight's planes were supplied?
    (Callers skip the plane copy -- 6 bytes per weight and a split launch per weight update -- for launches that stay on the
    exact-f32 kernel anyway: too few blocks, unsupported shape, DSC_GEMM=f32.)"""
    return planes_layout(g, gn) >= 0


def run_gemm(g, gn=False, stream=None):
    name = "dsc_gemm_gn_silu_f32" if gn else "dsc_gemm_f32"
    _lib.check(_lib.fn(name)(C.byref(g), stream if stream is not None else stream_ptr()), name)


def gemm(a, w, bias=None, a2=None, residual=None, act_in=ACT_NONE, act_out=ACT_NONE, out=None, w_planes=None, row_invariant=False):
    w2 = as2d(w)
    if out is None:
        out = torch.empty((a.shape[0], w2.shape[0]), device=a.device, dtype=torch.float32)
    run_gemm(make_gemm_args(a, w, out, bias, a2, residual, act_in, act_out, w_planes=w_planes, row_invariant=row_invariant))
    return out


def gemm_gn_silu(a, w_std, bias, gamma, beta, tokens_per_scene, a2=None, scale_shift=None, ss_mode=SS_NONE,
                 residual=None, eps=1e-5, out=None, preact=None, w_planes=None, ss_index=None):
    w2 = as2d(w_std)
    if out is None:
        out = torch.empty((a.shape[0], w2.shape[0]), device=a.device, dtype=torch.float32)
    run_gemm(make_gemm_args(a, w_std, out, bias, a2, residual, gamma=gamma, beta=beta, eps=eps,
                            tokens_per_scene=tokens_per_scene, scale_shift=scale_shift, ss_mode=ss_mode,
                            preact=preact, w_planes=w_planes, ss_index=ss_index), gn=True)
    return out


def _mats(*named):
    """The (ptr, ld, ptr, ld, ...) run of (tensor, name) pairs; an absent (None) optional operand gives (None, 0)."""
    run = ()
    for t, name in named:
        run += _mat(t, name) if t is not None else (None, 0)
    return run


def linear_smallk_rec(x, w, bias, out, act_out=ACT_NONE):
    w2 = as2d(w)
    xp, ldx, wp, ldw, yp, ldy = _mats((x, "x"), (w2, "w"), (out, "y"))
    return ("dsc_linear_smallk_f32", (xp, ldx, x.shape[1], wp, ldw, _opt(bias), yp, ldy, x.shape[0], w2.shape[0], act_out),
            (x, w, bias, out))


def linear_smallk(x, w, bias, act_out=ACT_NONE, out=None):
    """x may be a column slice of a wider row-major tensor (arbitrary alignment)."""
    if out is None:
        out = torch.empty((x.shape[0], as2d(w).shape[0]), device=x.device, dtype=torch.float32)
    issue(linear_smallk_rec(x, w, bias, out, act_out))
    return out


def weight_standardize_rec(pairs, eps=1e-5):
    """pairs: <= DSC_WS_MAX of (w, out), contiguous matrices (or (out, in, 1) conv weights)."""
    arr = (WsItem * len(pairs))()
    for i, (w, o) in enumerate(pairs):
        w2, o2 = as2d(_dev(w)), as2d(_dev(o))
        if not (w2.is_contiguous() and o2.is_contiguous()):
            raise RuntimeError("weight_standardize needs contiguous matrices")
        arr[i].w, arr[i].out, arr[i].rows, arr[i].cols = w2.data_ptr(), o2.data_ptr(), w2.shape[0], w2.shape[1]
    return "dsc_weight_standardize_f32", (arr, len(pairs), eps), (arr, pairs)


def weight_standardize(weights, outs=None, eps=1e-5):
    """Batched (w - mean_row) * rsqrt(var_row + eps); returns the standardised copies."""
    if outs is None:
        outs = [torch.empty_like(as2d(w)) for w in weights]
    for i in range(0, len(weights), _lib.WS_MAX):
        issue(weight_standardize_rec(list(zip(weights[i:i + _lib.WS_MAX], outs[i:i + _lib.WS_MAX])), eps))
    return outs


def layernorm_rec(x, g, out, residual=None, eps=1e-5):
    xp, ldx, rp, ldr, yp, ldy = _mats((x, "x"), (residual, "residual"), (out, "y"))
    return "dsc_layernorm_f32", (xp, ldx, _dev(g).data_ptr(), rp, ldr, yp, ldy, x.shape[0], x.shape[1], eps), (x, g, out, residual)


def layernorm(x, g, residual=None, eps=1e-5, out=None):
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), device=x.device, dtype=torch.float32)
    issue(layernorm_rec(x, g, out, residual, eps))
    return out


def linear_attention_rec(q, k, v, out, scenes, nq, nk, scale):
    """q, k, v may be column blocks of one wider projection buffer."""
    return ("dsc_linear_attention_f32", _mats((q, "q"), (k, "k"), (v, "v"), (out, "out")) + (scenes, nq, nk, scale), (q, k, v, out))


def linear_attention(q, k, v, scenes, nq, nk, scale, out=None):
    if out is None:
        out = torch.empty((q.shape[0], 128), device=q.device, dtype=torch.float32)
    issue(linear_attention_rec(q, k, v, out, scenes, nq, nk, scale))
    return out


def attention_rec(q, k, v, out, scenes, n, scale):
    return "dsc_attention_f32", _mats((q, "q"), (k, "k"), (v, "v"), (out, "out")) + (scenes, n, scale), (q, k, v, out)


def attention(q, k, v, scenes, n, scale, out=None):
    if out is None:
        out = torch.empty((q.shape[0], 128), device=q.device, dtype=torch.float32)
    issue(attention_rec(q, k, v, out, scenes, n, scale))
    return out


def time_embedding_rec(t, dim, table, freq, out):
    _dev(t, "t", torch.int64)
    return ("dsc_time_embedding_f32", (t.data_ptr(), t.shape[0], dim, _opt(table), table.shape[0] if table is not None else 0,
                                       _dev(freq).data_ptr(), out.data_ptr()), (t, table, freq, out))


def time_embedding(t, dim, table, freq, out=None):
    if out is None:
        out = torch.empty((t.shape[0], dim), device=t.device, dtype=torch.float32)
    issue(time_embedding_rec(t, dim, table, freq, out))
    return out


def linear_smallk_grouped_rec(xs, ws, biases, outs, act_out=ACT_NONE):
    n_items = len(xs)
    items = (_lib.SmallKItem * n_items)()
    m, n = outs[0].shape
    for i in range(n_items):
        w2 = as2d(ws[i])
        items[i].x, items[i].ldx = _mat(xs[i], "x")
        items[i].k_in = xs[i].shape[1]
        items[i].w, items[i].ldw = _mat(w2, "w")
        items[i].bias = _opt(biases[i])
        items[i].y, items[i].ldy = _mat(outs[i], "y")
        if tuple(outs[i].shape) != (m, n) or w2.shape[0] != n or xs[i].shape[0] != m:
            raise RuntimeError("linear_smallk_grouped: every head must produce the same [m, n] block")
    return "dsc_linear_smallk_grouped_f32", (items, n_items, m, n, act_out), (items, xs, ws, biases, outs)


def linear_smallk_grouped(xs, ws, biases, outs, act_out=ACT_NONE):
    """``len(xs)`` <= 4 small-K linears of one output width in ONE launch (dsc_linear_smallk_grouped_f32): xs[i] [m, k_i] may be column
    slices of a wider tensor, outs[i] [m, n] column blocks of a wider buffer."""
    issue(linear_smallk_grouped_rec(xs, ws, biases, outs, act_out))
    return outs


def gather_columns_rec(dst, src, spans):
    arr = (_lib.ColSpan * len(spans))()
    for i, (sc, dc, w) in enumerate(spans):
        arr[i].src_col, arr[i].dst_col, arr[i].width = sc, dc, w
    return "dsc_gather_columns_f32", _mats((dst, "dst"), (src, "src")) + (dst.shape[0], arr, len(spans)), (arr, dst, src)


def gather_columns(dst, src, spans):
    """dst[:, d:d+w] = src[:, s:s+w] for (s, d, w) in spans (<= 4), one launch."""
    issue(gather_columns_rec(dst, src, spans))
    return dst


def activation_rec(x, out, act):
    _dev(x)
    if not (x.is_contiguous() and out.is_contiguous()):
        raise RuntimeError("activation needs a contiguous tensor")
    return "dsc_activation_f32", (x.data_ptr(), out.data_ptr(), x.numel(), act), (x, out)


def activation(x, act, out=None):
    if out is None:
        out = torch.empty_like(x)
    issue(activation_rec(x, out, act))
    return out


# ---------------------------------------------------------------------------------- diffusion steps

def _c(t, name):
    _dev(t, name)
    if not t.is_contiguous():
        raise RuntimeError("diffuscene_amd: %s must be contiguous" % name)
    return t


def _table_rows(*tables):
    """Rows of the schedule tables a kernel indexes with the device timestep (it clamps t into them): all must agree."""
    rows = {int(tb.numel()) for tb in tables if tb is not None}
    if len(rows) != 1:
        raise RuntimeError("diffuscene_amd: schedule tables of different lengths %s" % sorted(rows))
    for tb in tables:
        if tb is not None:
            _c(tb, "schedule table")
    return rows.pop()


def _opt(t, name=None):
    """The pointer of an optional operand, None when it is absent; checked as ``name`` when given one."""
    if t is None:
        return None
    return (t if name is None else _c(t, name)).data_ptr()


def _strided_run(step, times, times_next, coef):
    """(the pointer run step, times, times_next, coef rows 0..2 of a strided step kernel, S): the (1,) int64 device counter, the (S,)
    int64 pairs and the (3, S) fp32 rows [sqrt(alpha_next), c, sigma]."""
    _dev(step, "step", torch.int64); _dev(times, "times", torch.int64); _dev(times_next, "times_next", torch.int64); _c(coef, "coef")
    S = times.numel()
    if times_next.numel() != S or tuple(coef.shape) != (3, S) or not (times.is_contiguous() and times_next.is_contiguous()):
        raise RuntimeError("diffuscene_amd: DDIM tables must be (S,) int64 pairs and (3, S) coefficients")
    return (step.data_ptr(), times.data_ptr(), times_next.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(), coef[2].data_ptr()), S


def _same_shape(what, x_t, *operands, out=None):
    if any(o is not None and o.shape != x_t.shape for o in operands + (out,)) or not (out is None or out.is_contiguous()):
        raise RuntimeError("diffuscene_amd: %s operands of different shapes" % what)


def _fresh(x_t, out):
    """``out`` of a step, allocated when absent (step_rec checks it)."""
    return torch.empty_like(x_t) if out is None else out


def q_sample_rec(x0, noise, t, sqrt_ac, sqrt_1mac, xt, v=None):
    _c(x0, "x0"); _c(noise, "noise"); _dev(t, "t", torch.int64)
    b = x0.shape[0]
    return ("dsc_q_sample_f32", (x0.data_ptr(), noise.data_ptr(), t.data_ptr(), sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(), xt.data_ptr(),
                                 _opt(v), b, x0.numel() // b, _table_rows(sqrt_ac, sqrt_1mac)), (x0, noise, t, sqrt_ac, sqrt_1mac, xt, v))


def q_sample(x0, noise, t, sqrt_ac, sqrt_1mac, want_v=False):
    xt = torch.empty_like(x0)
    v = torch.empty_like(x0) if want_v else None
    issue(q_sample_rec(x0, noise, t, sqrt_ac, sqrt_1mac, xt, v))
    return (xt, v) if want_v else xt


# The step family, one kernel template (csrc/diffusion.hip: step_kernel<STRIDED, GIVEN, GUIDED>): (strided, given, guided) -> (entry point,
# its parameters in the order of include/diffuscene_hip.h without the stream).  given: None, "rows" (a ragged row prefix) or "mask";
# guided completion -- (., "rows", True) -- has no instantiation and no key.
_POST = "ca cb coef1 coef2 sigma"
_STRIDED = "step times times_next sqrt_alpha_next c_noise sigma"
_DDIM = "ca cb sqrt_recip_ac sqrt_recipm1_ac"
_Q = "sqrt_ac sqrt_1mac"
_GIVEN = {None: "", "rows": " partial noise_p counts", "mask": " known noise_k mask"}


def _step_params(strided, given, guided):
    return " ".join(("x_t model_out" + (" scale" if guided else "") + " noise" + _GIVEN[given],
                     _STRIDED + " " + _DDIM if strided else "t " + _POST, _Q if given else "",
                     "out" + (" x_dup" if guided else "") + ("" if given else " x0_out"),
                     "mean_type" + ("" if strided else " clip"), "b n pmax c" if given == "rows" else "b inner",
                     "S T" if strided else "T")).split()


STEP_ENTRY = {key: ("dsc_%s_f32" % name, _step_params(*key)) for key, name in {
    (False, None, False): "p_sample", (True, None, False): "ddim_step",
    (False, "rows", False): "p_sample_inpaint", (True, "rows", False): "ddim_inpaint_step",
    (False, "mask", False): "p_sample_masked", (True, "mask", False): "ddim_masked_step",
    (False, None, True): "p_sample_cfg", (True, None, True): "ddim_cfg_step",
    (False, "mask", True): "p_sample_masked_cfg", (True, "mask", True): "ddim_masked_cfg_step"}.items()}


def step_rec(x_t, model_out, noise, out, mean_type, tables, t=None, clip=False, strided=None, rows=None, mask=None, q=(), scale=None,
             x_dup=None, x0_out=None):
    """The launch record of one reverse step, whichever of the ten it is.  The operand groups pick the entry point and STEP_ENTRY lays
    them out:  the state ``x_t``, ``model_out``, ``noise`` and the outputs ``out``, ``x0_out``;  the time source -- ``t`` (B,) int64 with
    ``tables`` = (ca, cb, coef1, coef2, sigma) and ``clip``, or ``strided`` = (step, times, times_next, coef) with ``tables`` = (ca, cb,
    sqrt_recip_ac, sqrt_recipm1_ac);  the given part -- ``rows`` = (partial, noise_p, counts on the device) or ``mask`` = (known, noise_k,
    mask), either with ``q`` = (sqrt_ac, sqrt_1mac);  guidance -- ``scale`` (B,) f32 under a ``model_out`` of 2 B scenes, and ``x_dup``.
    The checks are the same for every entry point; ValueError for a combination that has no kernel."""
    given = None if rows is None and mask is None else "rows" if mask is None else "mask" if rows is None else "rows and mask"
    key = (strided is not None, given, scale is not None)
    if key not in STEP_ENTRY:
        raise ValueError("diffuscene_amd: no step kernel for strided=%s, given=%s, guided=%s" % key)
    name, params = STEP_ENTRY[key]
    what = name[4:-4]
    for operand, o in (("x_dup", x_dup), ("x0_out", x0_out)):
        if o is not None and operand not in params:
            raise ValueError("diffuscene_amd: %s takes no %s" % (what, operand))
    if len(tables) != (4 if strided is not None else 5) or len(q) != (2 if given else 0):
        raise ValueError("diffuscene_amd: %s takes %s%s" % (what, _DDIM if strided is not None else _POST, " and " + _Q if given else ""))
    _c(x_t, "x_t"); _c(model_out, "model_out"); _c(noise, "noise")
    b = x_t.shape[0]
    v = dict(x_t=x_t, model_out=model_out, noise=noise, out=out, x0_out=_opt(x0_out, "x0_out"), mean_type=mean_type,
             clip=1 if clip else 0, b=b, inner=x_t.numel() // b, T=_table_rows(*tables, *q))
    _same_shape(what, x_t, None if scale is not None else model_out, noise, x0_out, out=out)
    v.update(zip((_DDIM if strided is not None else _POST).split() + _Q.split(), tuple(tables) + tuple(q)))
    if strided is not None:
        ptrs, v["S"] = _strided_run(*strided)
        v.update(zip(_STRIDED.split(), ptrs))
    else:
        _scene_t(t, b)
        v["t"] = t
    if rows is not None:
        _dev(rows[2], "counts", torch.int64)            # on the device already: a record never allocates (ops.ragged_counts uploads)
        _, v["n"], v["pmax"], v["c"], _ = _ragged_args(x_t, *rows)
        v.update(zip(("partial", "noise_p", "counts"), rows))
    if mask is not None:
        _masked_args(x_t, *mask)
        v.update(zip(("known", "noise_k", "mask"), mask))
    if scale is not None:
        _cfg_args(x_t, model_out, scale)
        v.update(scale=scale, x_dup=_cfg_dup(x_dup, x_t, out))
    args = tuple(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in (v[p] for p in params))
    return name, args, (x_t, model_out, noise, out, x0_out, tables, q, t, strided, rows, mask, scale, x_dup)


def p_sample(x_t, model_out, noise, t, ca, cb, coef1, coef2, sigma, mean_type, clip, out=None, x0_out=None):
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, coef1, coef2, sigma), t=t, clip=clip, x0_out=x0_out))
    return out


def add_scalar_i64(t, delta):
    _dev(t, "t", torch.int64)
    _lib.check(_lib.fn("dsc_add_scalar_i64")(t.data_ptr(), t.numel(), delta, stream_ptr()), "dsc_add_scalar_i64")
    return t


def ddim_step(x_t, model_out, noise, step, times, times_next, coef, ca, cb, sqrt_recip_ac, sqrt_recipm1_ac, mean_type,
              out=None, x0_out=None):
    """One DDIM step (see the C header).  ``step`` is the (1,) int64 device counter, ``times`` / ``times_next`` the (S,) int64 pairs and
    ``coef`` the (3, S) fp32 rows [sqrt(alpha_next), c, sigma]; ``noise`` is not read on the final pair (pass any tensor of x_t's shape)."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, sqrt_recip_ac, sqrt_recipm1_ac),
                   strided=(step, times, times_next, coef), x0_out=x0_out))
    return out


def ddim_advance(step, times, t):
    """step += 1; t[:] = times[step] (device-side, capturable)."""
    _dev(step, "step", torch.int64); _dev(t, "t", torch.int64); _dev(times, "times", torch.int64)
    if not times.is_contiguous():
        raise RuntimeError("diffuscene_amd: times must be contiguous")
    _lib.check(_lib.fn("dsc_ddim_advance_i64")(step.data_ptr(), times.data_ptr(), t.data_ptr(), t.numel(), times.numel(),
                                               stream_ptr()), "dsc_ddim_advance_i64")
    return t


def postfilter_compact(samples, empty_col, per_scene=False, keep_empty=False):
    """(B,N,C) generated scenes -> (packed (B,N,C) with the kept slots first, counts (B,) int32); see the C header."""
    _c(samples, "samples")
    b, n, c = samples.shape
    packed = torch.empty_like(samples)
    counts = torch.empty((b,), device=samples.device, dtype=torch.int32)
    _lib.check(_lib.fn("dsc_postfilter_compact_f32")(samples.data_ptr(), b, n, c, int(empty_col), 1 if per_scene else 0,
                                                     1 if keep_empty else 0, packed.data_ptr(), counts.data_ptr(),
                                                     stream_ptr()), "dsc_postfilter_compact_f32")
    return packed, counts


def complete_overwrite(x, partial, noise, t, sqrt_ac, sqrt_1mac):
    _c(x, "x"); _c(partial, "partial"); _c(noise, "noise"); _dev(t, "t", torch.int64)
    b, n, c = x.shape
    p = partial.shape[1]
    _lib.check(_lib.fn("dsc_complete_overwrite_f32")(x.data_ptr(), partial.data_ptr(), noise.data_ptr(), t.data_ptr(),
                                                     sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(), b, n, p, c,
                                                     _table_rows(sqrt_ac, sqrt_1mac), stream_ptr()), "dsc_complete_overwrite_f32")
    return x


def ragged_counts(counts, b, pmax, device):
    """Per-scene row counts of the ragged completion kernels as a (b,) int64 device tensor.  Counts that are still on the host (a
    sequence, a CPU tensor) are checked against [0, pmax] here -- ValueError names the scene -- and uploaded; a device tensor is taken
    as it is (the kernels clamp an out-of-range count and count it: dsc_device_error_count)."""
    if isinstance(counts, torch.Tensor) and counts.device.type != "cpu":
        _dev(counts, "counts", torch.int64)
        if tuple(counts.shape) != (b,) or not counts.is_contiguous():
            raise RuntimeError("diffuscene_amd: counts must be a contiguous (%d,) int64 tensor" % b)
        return counts
    host = counts.tolist() if isinstance(counts, torch.Tensor) else list(counts)
    if isinstance(counts, torch.Tensor) and (counts.dim() != 1 or counts.dtype.is_floating_point or counts.dtype == torch.bool):
        raise ValueError("counts must be a 1-d integer tensor, got %s %s" % (tuple(counts.shape), counts.dtype))
    if len(host) != b:
        raise ValueError("counts has %d entries for a batch of %d scenes" % (len(host), b))
    for i, v in enumerate(host):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= pmax:
            raise ValueError("scene %d: count %r outside [0, %d]" % (i, v, pmax))
    return torch.tensor([int(v) for v in host], dtype=torch.int64).to(device)


def _ragged_args(x, partial, noise_p, counts):
    _c(x, "x"); _c(partial, "partial"); _c(noise_p, "partial noise")
    b, n, c = x.shape
    pmax = partial.shape[1]
    if tuple(partial.shape) != (b, pmax, c) or tuple(noise_p.shape) != (b, pmax, c) or not 1 <= pmax <= n:
        raise RuntimeError("diffuscene_amd: partial / noise must be (%d, Pmax <= %d, %d), got %s / %s"
                           % (b, n, c, tuple(partial.shape), tuple(noise_p.shape)))
    return b, n, pmax, c, ragged_counts(counts, b, pmax, x.device)


def _scene_t(t, b):
    _dev(t, "t", torch.int64)
    if tuple(t.shape) != (b,) or not t.is_contiguous():
        raise RuntimeError("diffuscene_amd: t must be a contiguous (%d,) int64 tensor" % b)


def complete_overwrite_ragged(x, partial, noise, counts, t, sqrt_ac, sqrt_1mac):
    """complete_overwrite with per-scene counts: rows [0, counts[b]) of scene b <- q_sample(partial, t, noise); see the C header."""
    b, n, pmax, c, cnt = _ragged_args(x, partial, noise, counts)
    _scene_t(t, b)
    _lib.check(_lib.fn("dsc_complete_overwrite_ragged_f32")(x.data_ptr(), partial.data_ptr(), noise.data_ptr(), cnt.data_ptr(),
                                                            t.data_ptr(), sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(), b, n, pmax, c,
                                                            _table_rows(sqrt_ac, sqrt_1mac), stream_ptr()),
               "dsc_complete_overwrite_ragged_f32")
    return x


def p_sample_inpaint(x_t, model_out, noise, partial, noise_p, counts, t, ca, cb, coef1, coef2, sigma, sqrt_ac, sqrt_1mac, mean_type,
                     clip, out=None):
    """Fused step of the ragged completion loop: p_sample on rows >= counts[b]; the given rows get the re-noising of step t - 1
    (t > 0) or ``partial`` itself (t == 0).  See the C header."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, coef1, coef2, sigma), t=t, clip=clip,
                   rows=(partial, noise_p, _ragged_args(x_t, partial, noise_p, counts)[4]), q=(sqrt_ac, sqrt_1mac)))
    return out


def ddim_inpaint_step(x_t, model_out, noise, partial, noise_p, counts, step, times, times_next, coef, ca, cb, sqrt_recip_ac,
                      sqrt_recipm1_ac, sqrt_ac, sqrt_1mac, mean_type, out=None):
    """Fused step of the strided (DDIM) ragged completion loop: ddim_step on rows >= counts[b]; the given rows get the re-noising at
    ``times_next[step]`` or, on the last pair, ``partial`` itself (``noise`` and ``noise_p`` are not read there).  Tables as ddim_step,
    counts / partial as p_sample_inpaint.  See the C header."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, sqrt_recip_ac, sqrt_recipm1_ac), strided=(step, times, times_next, coef),
                   rows=(partial, noise_p, _ragged_args(x_t, partial, noise_p, counts)[4]), q=(sqrt_ac, sqrt_1mac)))
    return out


def known_mask(mask, shape, device):
    """The element-wise "given" mask of the masked (in-painting) kernels as a contiguous uint8 (B, N, C) tensor on ``device``.
    ``mask``: bool or uint8, (B, N, C) -- one flag per element -- or (B, N) -- whole rows; any non-zero byte means given.  A uint8
    (B, N, C) tensor already on the device is taken as it is.  ValueError on any other dtype or shape."""
    b, n, c = (int(v) for v in shape)
    if not isinstance(mask, torch.Tensor):
        raise ValueError("mask must be a bool / uint8 tensor of shape (%d, %d, %d) or (%d, %d), got %s" % (b, n, c, b, n, type(mask).__name__))
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mask must be bool or uint8, got %s" % mask.dtype)
    if tuple(mask.shape) == (b, n):
        mask = mask[:, :, None].expand(b, n, c)
    elif tuple(mask.shape) != (b, n, c):
        raise ValueError("mask must be (%d, %d, %d) or (%d, %d), got %s" % (b, n, c, b, n, tuple(mask.shape)))
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    return mask.to(device).contiguous()


def _masked_args(x, known, noise_k, mask):
    _c(x, "x"); _c(known, "known"); _c(noise_k, "known noise"); _dev(mask, "mask", torch.uint8)
    if not mask.is_contiguous():
        raise RuntimeError("diffuscene_amd: mask must be contiguous")
    if known.shape != x.shape or noise_k.shape != x.shape or mask.shape != x.shape or x.dim() < 2:
        raise RuntimeError("diffuscene_amd: known / noise / mask must have the shape of x %s, got %s / %s / %s"
                           % (tuple(x.shape), tuple(known.shape), tuple(noise_k.shape), tuple(mask.shape)))
    b = x.shape[0]
    return b, x.numel() // b


def masked_overwrite(x, known, noise, mask, t, sqrt_ac, sqrt_1mac):
    """x[i] <- q_sample(known, t, noise)[i] where mask[i] != 0 (uint8, x's shape: ops.known_mask); the rest of x is untouched.  See the C
    header."""
    b, inner = _masked_args(x, known, noise, mask)
    _scene_t(t, b)
    _lib.check(_lib.fn("dsc_masked_overwrite_f32")(x.data_ptr(), known.data_ptr(), noise.data_ptr(), mask.data_ptr(), t.data_ptr(),
                                                   sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(), b, inner, _table_rows(sqrt_ac, sqrt_1mac),
                                                   stream_ptr()), "dsc_masked_overwrite_f32")
    return x


def p_sample_masked(x_t, model_out, noise, known, noise_k, mask, t, ca, cb, coef1, coef2, sigma, sqrt_ac, sqrt_1mac, mean_type, clip,
                    out=None):
    """Fused step of the masked loop: p_sample on the free elements; the given ones get the re-noising of step t - 1 (t > 0) or
    ``known`` itself (t == 0; ``noise_k`` is not read there).  See the C header."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, coef1, coef2, sigma), t=t, clip=clip, mask=(known, noise_k, mask),
                   q=(sqrt_ac, sqrt_1mac)))
    return out


def ddim_masked_step(x_t, model_out, noise, known, noise_k, mask, step, times, times_next, coef, ca, cb, sqrt_recip_ac,
                     sqrt_recipm1_ac, sqrt_ac, sqrt_1mac, mean_type, out=None):
    """Fused step of the strided (DDIM) masked loop: ddim_step on the free elements; the given ones get the re-noising at
    ``times_next[step]`` or, on the last pair, ``known`` itself (``noise`` and ``noise_k`` are not read there).  Tables as ddim_step.
    See the C header."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, sqrt_recip_ac, sqrt_recipm1_ac), strided=(step, times, times_next, coef),
                   mask=(known, noise_k, mask), q=(sqrt_ac, sqrt_1mac)))
    return out


# ---------------------------------------------------------------------------------- classifier-free guidance

def guidance_scales(scale, b, device):
    """The per-scene guidance scales of the guided kernels as a contiguous (b,) f32 tensor on ``device``.  ``scale``: a float (every
    scene), or a length-b sequence / 1-d tensor (one scale per scene).  ValueError on NaN / inf, on a wrong length and on anything that
    is not a number."""
    return _scene_scales(scale, b, device, "guidance_scale")


def _scene_scales(scale, b, device, name, weights=False):
    """guidance_scales under the keyword ``name`` of its messages; ``weights``: steering weights, which also refuse a value below 0."""
    b = int(b)
    bad = "%s must be a number or a sequence of %d numbers, got %r" % (name, b, scale)
    if isinstance(scale, torch.Tensor):
        if scale.dim() > 1 or scale.dtype == torch.bool:
            raise ValueError("%s: a tensor must be a scalar or (%d,) of numbers, got %s %s" % (name, b, tuple(scale.shape), scale.dtype))
        scale = scale.tolist()
    if isinstance(scale, (bool, str, bytes)) or scale is None:
        raise ValueError(bad)
    if isinstance(scale, numbers.Real):
        host = [float(scale)] * b
    else:
        try:
            host = [float(v) for v in scale]
        except (TypeError, ValueError):
            raise ValueError(bad) from None
    if len(host) != b:
        raise ValueError("%s has %d entries for a batch of %d scenes" % (name, len(host), b))
    for i, v in enumerate(host):
        if v != v or v in (float("inf"), float("-inf")):
            raise ValueError("%s: scene %d: %r is not finite" % (name, i, v))
    w = torch.tensor(host, dtype=torch.float32)
    for i, v in enumerate(w.tolist() if weights else ()):
        if v < 0:
            raise ValueError("%s: scene %d: %r is negative" % (name, i, v))
    return w.to(device).contiguous()


def scene_seeds(value, batch_size, device):
    """The per-scene seeds of the seeded loops as a contiguous (batch_size,) int64 tensor on ``device``.  ``value``: a sequence (list,
    tuple, range, numpy array) or a 1-d integer tensor of exactly ``batch_size`` Python / numpy ints in [0, 2**63).  ValueError on
    bools, floats, a wrong length and values that are negative or too large.  Repeated seeds are allowed: two scenes with the same seed
    and the same inputs are the same scene."""
    b = int(batch_size)
    bad = "scene_seeds must be a sequence or 1-d integer tensor of %d ints in [0, 2**63), got %r" % (b, value)
    if isinstance(value, torch.Tensor):
        if value.dim() != 1 or value.dtype.is_floating_point or value.dtype.is_complex or value.dtype == torch.bool:
            raise ValueError("scene_seeds: a tensor must be (%d,) of integers, got %s %s" % (b, tuple(value.shape), value.dtype))
        host = value.tolist()
    elif value is None or isinstance(value, (str, bytes, numbers.Number)):
        raise ValueError(bad)
    else:
        try:
            host = [v.item() if hasattr(v, "item") and getattr(v, "ndim", 0) == 0 else v for v in value]
        except TypeError:
            raise ValueError(bad) from None
    if len(host) != b:
        raise ValueError("scene_seeds has %d entries for a batch of %d scenes" % (len(host), b))
    for i, v in enumerate(host):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("scene_seeds: scene %d: %r is not an integer" % (i, v))
        if not 0 <= int(v) < 2 ** 63:
            raise ValueError("scene_seeds: scene %d: %r outside [0, 2**63)" % (i, v))
    return torch.tensor([int(v) for v in host], dtype=torch.int64).to(device).contiguous()


def _scene_noise_args(seeds, draw, stream, shape):
    _dev(seeds, "seeds", torch.int64); _dev(draw, "draw", torch.int64)
    shape = tuple(int(s) for s in shape)
    if len(shape) < 1 or seeds.dim() != 1 or seeds.shape[0] != shape[0] or not seeds.is_contiguous():
        raise RuntimeError("diffuscene_amd: seeds must be a contiguous (%s,) int64 tensor (ops.scene_seeds), got %s"
                           % (shape[0] if shape else "B", tuple(seeds.shape)))
    if draw.numel() != 1:
        raise RuntimeError("diffuscene_amd: draw must hold ONE int64 (the device draw counter), got %s" % (tuple(draw.shape),))
    per_scene = 1
    for s in shape[1:]:
        per_scene *= s
    return shape, per_scene, int(stream)


def scene_randn(seeds, draw, stream, shape, out=None):
    """Per-scene normals: out[b] = scene_normal(seeds[b], stream, draw[0], e) over the scene's own ``shape[1:]`` block (see the C
    header, diffuscene_amd/scene_noise.py).  ``seeds``: (B,) int64 device tensor (ops.scene_seeds), ``draw``: the (1,) int64 DEVICE draw
    counter, read by the launch -- capturable --, ``stream``: 0 the main draws, 1 the draws of the given part."""
    shape, per_scene, stream = _scene_noise_args(seeds, draw, stream, shape)
    if out is None:
        out = torch.empty(shape, device=seeds.device, dtype=torch.float32)
    _c(out, "out")
    if tuple(out.shape) != shape:
        raise RuntimeError("diffuscene_amd: scene_randn: out must be %s, got %s" % (shape, tuple(out.shape)))
    if out.numel() == 0:
        return out                             # nothing to draw (an empty tensor has no address to pass)
    _lib.check(_lib.fn("dsc_scene_randn_f32")(out.data_ptr(), seeds.data_ptr(), draw.data_ptr(), stream, shape[0], per_scene,
                                              stream_ptr()), "dsc_scene_randn_f32")
    return out


def scene_philox(seeds, draw, stream, shape):
    """The raw Philox word of every element of scene_randn's draw, as int32 bit patterns (a probe for tests)."""
    shape, per_scene, stream = _scene_noise_args(seeds, draw, stream, shape)
    out = torch.empty(shape, device=seeds.device, dtype=torch.int32)
    if out.numel() == 0:
        return out
    _lib.check(_lib.fn("dsc_scene_philox_u32")(out.data_ptr(), seeds.data_ptr(), draw.data_ptr(), stream, shape[0], per_scene,
                                               stream_ptr()), "dsc_scene_philox_u32")
    return out


def _cfg_args(x_t, model_out, scale):
    """(b, inner) of a guided launch: model_out is (2 b, ...) with the conditional half first, scale a contiguous (b,) f32 device tensor."""
    _c(model_out, "model_out"); _c(scale, "scale")
    b = x_t.shape[0]
    if model_out.dim() != x_t.dim() or model_out.shape[0] != 2 * b or tuple(model_out.shape[1:]) != tuple(x_t.shape[1:]):
        raise RuntimeError("diffuscene_amd: model_out must be (2 * %d,) + %s (conditional half first), got %s"
                           % (b, tuple(x_t.shape[1:]), tuple(model_out.shape)))
    if tuple(scale.shape) != (b,):
        raise RuntimeError("diffuscene_amd: scale must be a (%d,) f32 tensor (ops.guidance_scales), got %s" % (b, tuple(scale.shape)))
    return b, x_t.numel() // b


def _cfg_dup(x_dup, x_t, out):
    if x_dup is None:
        return None
    _c(x_dup, "x_dup")
    if x_dup.shape != x_t.shape:
        raise RuntimeError("diffuscene_amd: x_dup must have the shape of x_t %s, got %s" % (tuple(x_t.shape), tuple(x_dup.shape)))
    n = x_t.numel() * 4
    for other in (x_t, out):
        if x_dup.data_ptr() < other.data_ptr() + n and other.data_ptr() < x_dup.data_ptr() + n:
            raise RuntimeError("diffuscene_amd: x_dup must not overlap x_t / out")
    return x_dup.data_ptr()


def cfg_combine(model_out, scale, out=None):
    """m = u + scale[b] * (c - u) from model_out (2 B, ...) = [c; u] -> (B, ...).  See the C header."""
    _c(model_out, "model_out")
    if model_out.shape[0] % 2 or model_out.shape[0] < 2:
        raise RuntimeError("diffuscene_amd: model_out must hold 2 B scenes, got %s" % (tuple(model_out.shape),))
    b = model_out.shape[0] // 2
    if out is None:
        out = torch.empty((b,) + tuple(model_out.shape[1:]), device=model_out.device, dtype=torch.float32)
    _c(out, "out")
    b, inner = _cfg_args(out, model_out, scale)
    _lib.check(_lib.fn("dsc_cfg_combine_f32")(model_out.data_ptr(), scale.data_ptr(), out.data_ptr(), b, inner, stream_ptr()),
               "dsc_cfg_combine_f32")
    return out


def p_sample_cfg(x_t, model_out, scale, noise, t, ca, cb, coef1, coef2, sigma, mean_type, clip, out=None, x_dup=None, x0_out=None):
    """p_sample on the guided model output, one launch: model_out (2 B, N, C) = [c; u], scale (B,) f32 (ops.guidance_scales); ``x_dup``
    receives a second copy of the result.  Bit-identical to cfg_combine followed by p_sample.  See the C header."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, coef1, coef2, sigma), t=t, clip=clip, scale=scale, x_dup=x_dup,
                   x0_out=x0_out))
    return out


def ddim_cfg_step(x_t, model_out, scale, noise, step, times, times_next, coef, ca, cb, sqrt_recip_ac, sqrt_recipm1_ac, mean_type,
                  out=None, x_dup=None, x0_out=None):
    """ddim_step on the guided model output, one launch; operands as p_sample_cfg, tables as ddim_step (``noise`` is not read on the
    final pair).  Bit-identical to cfg_combine followed by ddim_step.  See the C header."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, sqrt_recip_ac, sqrt_recipm1_ac), strided=(step, times, times_next, coef),
                   scale=scale, x_dup=x_dup, x0_out=x0_out))
    return out


def p_sample_masked_cfg(x_t, model_out, scale, noise, known, noise_k, mask, t, ca, cb, coef1, coef2, sigma, sqrt_ac, sqrt_1mac,
                        mean_type, clip, out=None, x_dup=None):
    """p_sample_masked on the guided model output, one launch: model_out (2 B, N, C) = [c; u], scale (B,) f32; known / noise_k / mask
    are (B, N, C); ``x_dup`` receives a second copy of every written element.  Bit-identical to cfg_combine followed by
    p_sample_masked.  See the C header."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, coef1, coef2, sigma), t=t, clip=clip, mask=(known, noise_k, mask),
                   q=(sqrt_ac, sqrt_1mac), scale=scale, x_dup=x_dup))
    return out


def ddim_masked_cfg_step(x_t, model_out, scale, noise, known, noise_k, mask, step, times, times_next, coef, ca, cb, sqrt_recip_ac,
                         sqrt_recipm1_ac, sqrt_ac, sqrt_1mac, mean_type, out=None, x_dup=None):
    """ddim_masked_step on the guided model output, one launch; operands as p_sample_masked_cfg, tables as ddim_masked_step (``noise``
    and ``noise_k`` are not read on the final pair).  Bit-identical to cfg_combine followed by ddim_masked_step.  See the C header."""
    out = _fresh(x_t, out)
    issue(step_rec(x_t, model_out, noise, out, mean_type, (ca, cb, sqrt_recip_ac, sqrt_recipm1_ac), strided=(step, times, times_next, coef),
                   mask=(known, noise_k, mask), q=(sqrt_ac, sqrt_1mac), scale=scale, x_dup=x_dup))
    return out


# ---------------------------------------------------------------------------------- collision steering

STEER_MAX_OBJECTS = 160            # one block per scene, one thread per box (csrc/diffusion.hip: STEER_MAXN)


def collision_scales(scale, b, device):
    """The per-scene steering weights of dsc_steer_boxes_f32 as a contiguous (b,) f32 tensor on ``device``.  ``scale``: a float (every
    scene) or b values, as guidance_scales takes them, each finite and >= 0; 0 leaves that scene unsteered.  ValueError otherwise."""
    return _scene_scales(scale, b, device, "collision_scale", weights=True)


def collision_steps(steps, num_timesteps):
    """K of dsc_steer_boxes_f32: a step at timestep t is steered iff t < K.  ``steps``: None (every step, K = num_timesteps) or an
    integer in [0, num_timesteps] -- the last K timesteps of the schedule; a strided loop steers the pairs whose t is below K."""
    return _steered_steps(steps, num_timesteps, "collision_steps")


def _steered_steps(steps, num_timesteps, name):
    if steps is None:
        return int(num_timesteps)
    if isinstance(steps, bool) or not isinstance(steps, numbers.Integral) or not 0 <= int(steps) <= num_timesteps:
        raise ValueError("%s must be None or an integer in [0, %d], got %r" % (name, num_timesteps, steps))
    return int(steps)


def steer_bounds(bounds):
    """The 12 host floats of dsc_steer_boxes_f32 / dsc_ddpm_loss_f32 -- translation lo[3], hi[3], size lo[3], hi[3] -- as a ctypes array;
    ValueError unless there are 12 finite numbers."""
    if isinstance(bounds, C.c_float * 12):
        return bounds
    try:
        host = [float(v) for v in (bounds.tolist() if isinstance(bounds, torch.Tensor) else bounds)]
    except (TypeError, ValueError):
        raise ValueError("bounds must be 12 numbers (translation lo, hi, size lo, hi), got %r" % (bounds,)) from None
    if len(host) != 12 or any(v != v or v in (float("inf"), float("-inf")) for v in host):
        raise ValueError("bounds must be 12 finite numbers (translation lo, hi, size lo, hi), got %r" % (host,))
    return (C.c_float * 12)(*host)


# The parameters of the two steering entry points in the order of include/diffuscene_hip.h without the stream: the shared operands, with
# what floor-plan steering adds where the header has it.
_STEER_IN = "x_t model_out t step times ca cb partial counts known mask scale weight t_below bounds"
_STEER_DIMS = "mean_type b n pmax c bbox_dim class_dim S T"
STEER_PARAMS = (_STEER_IN + " energy_out grad_out " + _STEER_DIMS).split()
WALLS_PARAMS = (_STEER_IN + " field room_side energy_out grad_out outside_out " + _STEER_DIMS + " field_b h w").split()


def _steer_operands(noun, x_t, model_out, mean_type, tables, steer, t=None, clip=None, strided=None, rows=None, mask=None, q=(),
                    scale=None, x_dup=None, energy_out=None, grad_out=None):
    """The operands both steering records share, checked, by the names of STEER_PARAMS (a tensor or None, a host value as it is).
    ``noun`` names the steering in the messages."""
    weight, t_below, bounds, bbox_dim, class_dim = steer
    if rows is not None and mask is not None:
        raise ValueError("diffuscene_amd: steer_boxes takes one given part, rows or mask")
    if (t is None) == (strided is None):
        raise ValueError("diffuscene_amd: steer_boxes takes one time source, t or strided")
    _c(model_out, "model_out"); _c(weight, "weight"); _dev(t_below, "t_below", torch.int64)
    if model_out.dim() != 3:
        raise RuntimeError("diffuscene_amd: model_out must be (B, N, C), got %s" % (tuple(model_out.shape),))
    mult = 1 if scale is None else 2
    b, n, c = model_out.shape[0] // mult, model_out.shape[1], model_out.shape[2]
    shape = (b, n, c)
    if x_t is not None:
        _c(x_t, "x_t")
    elif mean_type != MEAN_X0:
        raise RuntimeError("diffuscene_amd: steer_boxes needs x_t unless the model predicts x0")
    if model_out.shape[0] != mult * b or b < 1 or (x_t is not None and tuple(x_t.shape) != shape):
        raise RuntimeError("diffuscene_amd: steer_boxes: x_t %s and model_out %s do not go together"
                           % (None if x_t is None else tuple(x_t.shape), tuple(model_out.shape)))
    if tuple(weight.shape) != (b,) or t_below.numel() != 1:
        raise RuntimeError("diffuscene_amd: weight must be (%d,) f32 and t_below hold one int64" % b)
    if n > STEER_MAX_OBJECTS:
        raise ValueError("diffuscene_amd: %s handles at most %d objects per scene, got %d" % (noun, STEER_MAX_OBJECTS, n))
    if bbox_dim != 8 or class_dim < 1 or bbox_dim + class_dim > c:
        raise ValueError("diffuscene_amd: %s needs the layout [translation 3 | size 3 | cos, sin | classes ...], got "
                         "bbox_dim=%d, class_dim=%d, %d channels" % (noun, bbox_dim, class_dim, c))
    # the timestep is held to the rows of the schedule tables; a model that predicts x0 indexes none here, and without any table of the
    # step at hand only a negative timestep is out of range
    v = dict.fromkeys(STEER_PARAMS)
    v.update(x_t=x_t, model_out=model_out, ca=tables[0], cb=tables[1], scale=scale, weight=weight, t_below=t_below,
             bounds=steer_bounds(bounds), energy_out=energy_out, grad_out=grad_out, mean_type=mean_type, b=b, n=n, pmax=0, c=c,
             bbox_dim=bbox_dim, class_dim=class_dim, S=0, T=_table_rows(*tables) if any(tb is not None for tb in tables) else 2 ** 31 - 1)
    if strided is not None:
        (v["step"], v["times"], _, _, _, _), v["S"] = _strided_run(*strided)
    else:
        _scene_t(t, b)
        v["t"] = t
    if rows is not None:
        partial, counts = _c(rows[0], "partial"), _dev(rows[2], "counts", torch.int64)
        pmax = partial.shape[1]
        if tuple(partial.shape) != (b, pmax, c) or not 1 <= pmax <= n or tuple(counts.shape) != (b,) or not counts.is_contiguous():
            raise RuntimeError("diffuscene_amd: partial must be (%d, Pmax <= %d, %d) with (%d,) counts, got %s / %s"
                               % (b, n, c, b, tuple(partial.shape), tuple(counts.shape)))
        v.update(partial=partial, counts=counts, pmax=pmax)
    if mask is not None:
        known, mk = _c(mask[0], "known"), _dev(mask[2], "mask", torch.uint8)
        if tuple(known.shape) != shape or tuple(mk.shape) != shape or not mk.is_contiguous():
            raise RuntimeError("diffuscene_amd: known / mask must be %s, got %s / %s" % (shape, tuple(known.shape), tuple(mk.shape)))
        v.update(known=known, mask=mk)
    if scale is not None and (tuple(_c(scale, "scale").shape) != (b,)):
        raise RuntimeError("diffuscene_amd: scale must be a (%d,) f32 tensor (ops.guidance_scales), got %s" % (b, tuple(scale.shape)))
    for o, want, name in ((energy_out, (b,), "energy_out"), (grad_out, (b, n, 3), "grad_out")):
        if o is not None and tuple(_c(o, name).shape) != want:
            raise RuntimeError("diffuscene_amd: %s must be %s, got %s" % (name, want, tuple(o.shape)))
    return v


def _steer_record(name, params, v, keep):
    """(entry point, its arguments laid out from ``params``, what the launch keeps alive)."""
    args = tuple(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in (v[p] for p in params))
    return name, args, (tuple(v.values()), keep)


def steer_rec(x_t, model_out, mean_type, tables, steer, **operands):
    """The launch record of collision steering (dsc_steer_boxes_f32): ``model_out`` (B, N, C) -- (2 B, N, C) under ``scale`` -- is
    corrected in place between the model call and the step.  It takes the operand groups of step_rec under the same keywords, so a loop
    hands both records the same dictionaries: the time source ``t`` or ``strided`` (its step counter and times), ``tables`` (ca, cb
    first; the rest, ``clip``, ``q`` and ``x_dup`` belong to the step and are not read here), the given part ``rows`` = (partial, _,
    counts) or ``mask`` = (known, _, mask), guidance ``scale``.  ``steer`` = (weight (B,) f32, t_below (1,) int64 -- both on the device,
    read at launch --, bounds (steer_bounds), bbox_dim, class_dim).  ``x_t`` may be None for mean type x0.  ``energy_out`` (B,) /
    ``grad_out`` (B, N, 3): the optional outputs."""
    v = _steer_operands("collision steering", x_t, model_out, mean_type, tables, steer, **operands)
    return _steer_record("dsc_steer_boxes_f32", STEER_PARAMS, v, (tables, steer, operands))


def steer_boxes(x_t, model_out, weight, t_below, bounds, mean_type, ca=None, cb=None, bbox_dim=8, class_dim=1, energy_out=None,
                grad_out=None, **operands):
    """Collision steering of ``model_out`` in place, eagerly; ``operands``: the time source and the optional groups of steer_rec.
    Returns ``model_out``."""
    issue(steer_rec(x_t, model_out, mean_type, (ca, cb), (weight, t_below, bounds, bbox_dim, class_dim), energy_out=energy_out,
                    grad_out=grad_out, **operands))
    return model_out


def box_repulsion(x0, bounds, bbox_dim=8, class_dim=1):
    """The overlap energy of collision steering and its gradient, standalone: ``x0`` (B, N, C) scenes in the network's encoding (clamped
    to [-1, 1] first, as the steering does) -> (energy (B,), grad (B, N, 3) = d energy / d x0[:, :, 0:3]).  The same entry point with
    mean type x0, weight 0 and both optional outputs: nothing is written to ``x0``.  See the C header."""
    _c(x0, "x0")
    b, n = x0.shape[0], x0.shape[1]
    dev = x0.device
    energy = torch.empty((b,), device=dev, dtype=torch.float32)
    grad = torch.empty((b, n, 3), device=dev, dtype=torch.float32)
    steer_boxes(None, x0, torch.zeros((b,), device=dev), torch.zeros((1,), device=dev, dtype=torch.int64), bounds, MEAN_X0,
                bbox_dim=bbox_dim, class_dim=class_dim, energy_out=energy, grad_out=grad, t=torch.zeros((b,), device=dev, dtype=torch.int64))
    return energy, grad


# ---------------------------------------------------------------------------------- floor-plan steering

WALL_MAX_SIDE = 256                # pixels per side of the room mask (csrc/diffusion.hip: WALL_MAXHW)


def wall_scales(scale, b, device):
    """The per-scene weights of dsc_steer_walls_f32: collision_scales under the name ``wall_scale``."""
    return _scene_scales(scale, b, device, "wall_scale", weights=True)


def wall_steps(steps, num_timesteps):
    """K of dsc_steer_walls_f32: collision_steps under the name ``wall_steps``."""
    return _steered_steps(steps, num_timesteps, "wall_steps")


def room_side_value(room_side):
    """``room_side`` -- half the side of the square window the room mask was rendered in, metres -- as a float; ValueError unless it is
    one finite number > 0."""
    if isinstance(room_side, bool) or not isinstance(room_side, numbers.Real) or not 0 < float(room_side) < float("inf"):
        raise ValueError("room_side must be a finite number > 0 (half the side of the mask's window, in metres), got %r" % (room_side,))
    return float(room_side)


def room_mask_dims(room_mask, b):
    """(leading dimension 1 or b, H, W) of a room mask for b scenes, checked on the host: a (b, 1, H, W) or (1, 1, H, W) tensor, float
    or uint8 / bool, 2 <= H, W <= 256.  ValueError otherwise."""
    if not isinstance(room_mask, torch.Tensor) or room_mask.dim() != 4 or room_mask.shape[1] != 1:
        raise ValueError("room_mask must be a (B, 1, H, W) or (1, 1, H, W) tensor, got %s"
                         % (tuple(room_mask.shape) if isinstance(room_mask, torch.Tensor) else type(room_mask).__name__,))
    fb, _, h, w = (int(v) for v in room_mask.shape)
    if fb not in (1, int(b)):
        raise ValueError("room_mask holds %d masks for %d scenes (one for each, or one for all)" % (fb, b))
    if not (2 <= h <= WALL_MAX_SIDE and 2 <= w <= WALL_MAX_SIDE):
        raise ValueError("room_mask must have 2 <= H, W <= %d, got %d x %d" % (WALL_MAX_SIDE, h, w))
    if not (room_mask.is_floating_point() or room_mask.dtype in (torch.uint8, torch.bool)):
        raise ValueError("room_mask must be float or uint8, got %s" % room_mask.dtype)
    return fb, h, w


def floor_field_rec(mask, field, room_side):
    """The launch record of dsc_floor_field_f32: ``mask`` (b, H, W) f32 -> ``field`` (b, H, W) f32."""
    _c(mask, "mask"); _c(field, "field")
    if mask.dim() != 3 or tuple(field.shape) != tuple(mask.shape):
        raise RuntimeError("diffuscene_amd: mask and field must be (b, H, W), got %s / %s" % (tuple(mask.shape), tuple(field.shape)))
    b, h, w = mask.shape
    return "dsc_floor_field_f32", (mask.data_ptr(), field.data_ptr(), b, h, w, room_side_value(room_side)), (mask, field)


def floor_field(room_mask, room_side, out=None):
    """The distance field of floor-plan steering: ``room_mask`` (b, 1, H, W), float or uint8 on the device, inside
    iff > 0.5 -> (b, H, W) f32, half the squared distance in metres^2 from each pixel centre to the nearest inside one.  Once per call."""
    fb, h, w = room_mask_dims(room_mask, room_mask.shape[0] if isinstance(room_mask, torch.Tensor) and room_mask.dim() else 1)
    if not room_mask.is_cuda:
        raise RuntimeError("diffuscene_amd: room_mask must live on a HIP device (no CPU fallback exists)")
    mask = room_mask.reshape(fb, h, w).to(torch.float32).contiguous()
    field = torch.empty((fb, h, w), device=mask.device, dtype=torch.float32) if out is None else out
    issue(floor_field_rec(mask, field, room_side))
    return field


def walls_rec(x_t, model_out, mean_type, tables, walls, energy_out=None, grad_out=None, outside_out=None, **operands):
    """The launch record of floor-plan steering (dsc_steer_walls_f32), marshalled once like steer_rec and with its operand groups
    (``operands``: the time source ``t`` or ``strided``, the given part, ``scale``).  ``walls`` = (weight (B,) f32, t_below (1,) int64,
    bounds (steer_bounds), bbox_dim, class_dim, field (B or 1, H, W) f32, room_side (1,) f32) -- weight, t_below, field and room_side on
    the device, read at launch.  ``outside_out`` (B,) int32: the third optional output."""
    weight, t_below, bounds, bbox_dim, class_dim, field, room_side = walls
    v = _steer_operands("floor-plan steering", x_t, model_out, mean_type, tables,
                        (weight, t_below, bounds, bbox_dim, class_dim), energy_out=energy_out, grad_out=grad_out, **operands)
    b = v["b"]
    _c(field, "field"); _c(room_side, "room_side")
    if field.dim() != 3 or field.shape[0] not in (1, b) or not all(2 <= int(d) <= WALL_MAX_SIDE for d in field.shape[1:]):
        raise RuntimeError("diffuscene_amd: field must be (%d or 1, H, W) with 2 <= H, W <= %d, got %s" % (b, WALL_MAX_SIDE, tuple(field.shape)))
    if room_side.numel() != 1:
        raise RuntimeError("diffuscene_amd: room_side must hold one f32")
    if outside_out is not None and (tuple(_dev(outside_out, "outside_out", torch.int32).shape) != (b,) or not outside_out.is_contiguous()):
        raise RuntimeError("diffuscene_amd: outside_out must be a contiguous (%d,) int32 tensor" % b)
    v.update(field=field, room_side=room_side, outside_out=outside_out)
    v["field_b"], v["h"], v["w"] = field.shape
    return _steer_record("dsc_steer_walls_f32", WALLS_PARAMS, v, (tables, walls, operands))


def steer_walls(x_t, model_out, weight, t_below, bounds, field, room_side, mean_type, ca=None, cb=None, bbox_dim=8, class_dim=1,
                energy_out=None, grad_out=None, outside_out=None, **operands):
    """Floor-plan steering of ``model_out`` in place, eagerly; ``operands``: the time source and the optional groups of walls_rec.
    Returns ``model_out``."""
    issue(walls_rec(x_t, model_out, mean_type, (ca, cb), (weight, t_below, bounds, bbox_dim, class_dim, field, room_side),
                    energy_out=energy_out, grad_out=grad_out, outside_out=outside_out, **operands))
    return model_out


def floor_violation(x0, room_mask, room_side, bounds, bbox_dim=8, class_dim=1):
    """The out-of-room energy of floor-plan steering, standalone: ``x0`` (B, N, C) scenes in the network's encoding (clamped to [-1, 1]
    first), ``room_mask`` (B or 1, 1, H, W) -> (energy (B,), grad (B, N, 3) = d energy / d x0[:, :, 0:3], its y column 0, outside (B,)
    int32 = the number of non-empty boxes with a footprint point outside the room).  The steering entry point with mean type x0,
    weight 0 and the optional outputs: nothing is written to ``x0``."""
    _c(x0, "x0")
    b, n = x0.shape[0], x0.shape[1]
    dev = x0.device
    room_mask_dims(room_mask, b)
    field = floor_field(room_mask.to(dev), room_side)
    energy = torch.empty((b,), device=dev, dtype=torch.float32)
    grad = torch.empty((b, n, 3), device=dev, dtype=torch.float32)
    outside = torch.empty((b,), device=dev, dtype=torch.int32)
    steer_walls(None, x0, torch.zeros((b,), device=dev), torch.zeros((1,), device=dev, dtype=torch.int64), bounds, field,
                torch.full((1,), room_side_value(room_side), device=dev), MEAN_X0, bbox_dim=bbox_dim, class_dim=class_dim,
                energy_out=energy, grad_out=grad, outside_out=outside, t=torch.zeros((b,), device=dev, dtype=torch.int64))
    return energy, grad, outside


# ---------------------------------------------------------------------------------- multistep solver

SOLVERS = ("dpmpp_2m",)            # sampling_solver= of the strided loops


def multistep_weights(pairs, alphas_cumprod):
    """The (S,) float32 history weights of dsc_multistep_x0_f32 for the (t, t_next) ``pairs`` of ddim_schedule and
    the float64 ``alphas_cumprod`` (T,): with lambda(t) = 1/2 ln(abar_t / (1 - abar_t)) and h_k = lambda(t_next_k) - lambda(t_k),
    e_0 = 0, e_k = h_k / (2 h_{k-1}) for 1 <= k <= S - 2, e_{S-1} = 0 (the last pair, t_next = -1, takes x0).  Float64 on the host, one
    rounding; a CPU tensor."""
    ac = torch.as_tensor(alphas_cumprod, dtype=torch.float64).to("cpu")
    if ac.dim() != 1 or ac.dtype != torch.float64:
        raise ValueError("alphas_cumprod must be a (T,) float64 table")
    lam = 0.5 * torch.log(ac / (1.0 - ac))
    S = len(pairs)
    e = torch.zeros((S,), dtype=torch.float64)
    h = [float(lam[tn] - lam[t]) if tn >= 0 else 0.0 for t, tn in pairs]
    for k in range(1, S - 1):
        e[k] = h[k] / (2.0 * h[k - 1])
    return e.to(torch.float32)


def multistep_rec(x_t, model_out, hist, weights, mean_type, tables, strided=None, rows=None, mask=None, q=(), scale=None, x_dup=None,
                  t=None, clip=None):
    """The launch record of the multistep solver (dsc_multistep_x0_f32): ``model_out`` (B, ...) -- (2 B, ...) under ``scale`` -- is
    corrected in place between the (steered) model call and the strided step, ``hist`` (x_t's shape) keeps the clamped x0 of the pair.
    It takes the operand groups of step_rec under the same keywords, as steer_rec does: ``strided`` (its step counter and times -- the
    solver rides on the strided loops only), ``tables`` (ca, cb first; the rest, ``q`` and ``x_dup`` belong to the step), the given part
    ``rows`` = (partial, _, counts) or ``mask`` = (known, _, mask), guidance ``scale``.  ``weights``: the (S,) f32 table of
    multistep_weights on the device.  ``x_t`` may be None for mean type x0."""
    if rows is not None and mask is not None:
        raise ValueError("diffuscene_amd: multistep_x0 takes one given part, rows or mask")
    if strided is None or t is not None:
        raise ValueError("diffuscene_amd: multistep_x0 rides on a strided loop: strided=(step, times, times_next, coef)")
    _c(model_out, "model_out"); _c(hist, "hist"); _c(weights, "weights")
    mult = 1 if scale is None else 2
    b = model_out.shape[0] // mult
    shape = (b,) + tuple(model_out.shape[1:])
    if x_t is not None:
        _c(x_t, "x_t")
    elif mean_type != MEAN_X0:
        raise RuntimeError("diffuscene_amd: multistep_x0 needs x_t unless the model predicts x0")
    if model_out.dim() < 2 or model_out.shape[0] != mult * b or b < 1 or tuple(hist.shape) != shape \
            or (x_t is not None and tuple(x_t.shape) != shape):
        raise RuntimeError("diffuscene_amd: multistep_x0: x_t %s, model_out %s and hist %s do not go together"
                           % (None if x_t is None else tuple(x_t.shape), tuple(model_out.shape), tuple(hist.shape)))
    ca, cb = tables[0], tables[1]
    T = _table_rows(*tables) if any(tb is not None for tb in tables) else 2 ** 31 - 1
    (sp, tmp, _, _, _, _), S = _strided_run(*strided)
    if tuple(weights.shape) != (S,):
        raise RuntimeError("diffuscene_amd: weights must be (%d,) f32 (ops.multistep_weights), got %s" % (S, tuple(weights.shape)))
    counts = mk = None
    pmax = c = 0
    if rows is not None:
        partial, counts = rows[0], _dev(rows[2], "counts", torch.int64)
        if len(shape) != 3 or partial.dim() != 3 or partial.shape[0] != b or partial.shape[2] != shape[2] \
                or not 1 <= partial.shape[1] <= shape[1] or tuple(counts.shape) != (b,) or not counts.is_contiguous():
            raise RuntimeError("diffuscene_amd: partial must be (%d, Pmax <= N, C) of a (B, N, C) state with (%d,) counts, got %s / %s"
                               % (b, b, tuple(partial.shape), tuple(counts.shape)))
        pmax, c = partial.shape[1], shape[2]
    if mask is not None:
        mk = _dev(mask[2], "mask", torch.uint8)
        if tuple(mk.shape) != shape or not mk.is_contiguous():
            raise RuntimeError("diffuscene_amd: mask must be contiguous %s, got %s" % (shape, tuple(mk.shape)))
    if scale is not None and tuple(_c(scale, "scale").shape) != (b,):
        raise RuntimeError("diffuscene_amd: scale must be a (%d,) f32 tensor (ops.guidance_scales), got %s" % (b, tuple(scale.shape)))
    args = (_opt(x_t), model_out.data_ptr(), hist.data_ptr(), weights.data_ptr(), sp, tmp, _opt(ca), _opt(cb), _opt(scale), _opt(counts),
            _opt(mk), mean_type, b, hist.numel() // b, pmax, c, S, T)
    return "dsc_multistep_x0_f32", args, (x_t, model_out, hist, weights, tables, strided, rows, mask, scale)


# ---------------------------------------------------------------------------------- resampling jumps

ResampleSchedule = collections.namedtuple("ResampleSchedule", "ops calls jumps points")


def resample_pair(resample, what):
    """(jump_length, n_resample) of ``resample=``, two integers >= 1, or ValueError naming ``what``."""
    ok = isinstance(resample, (tuple, list)) and len(resample) == 2 and all(
        isinstance(v, numbers.Integral) and not isinstance(v, bool) and v >= 1 for v in resample)
    if not ok:
        raise ValueError("%s: resample must be (jump_length, n_resample), two integers >= 1, got %r" % (what, resample))
    return int(resample[0]), int(resample[1])


def resample_steps_value(resample_steps, num_timesteps, what):
    """K of ``resample_steps=``: None (no limit) or an integer in [0, T]; jump points whose time is below K resample."""
    if resample_steps is None:
        return None
    k = resample_steps
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 0 <= int(k) <= num_timesteps:
        raise ValueError("%s: resample_steps must be an integer in [0, %d], got %r" % (what, num_timesteps, k))
    return int(k)


def resample_schedule(U, jump_length, n_resample, times=None, resample_steps=None):
    """The op list of a resampled loop (RePaint's get_schedule_jump).  Model calls are numbered by their remaining
    index u = U - 1 ... 0; ``times`` None: time(u) = u (the T-step loops), else the (S,) times of the pairs, time(u) = times[U - 1 - u].
    Jump points are s = 0, j, 2 j, ... < U - j with time(s) < ``resample_steps`` (None: all); each is jumped from r - 1 times, to s + j.
    -> ResampleSchedule(ops, calls, jumps, points): ``ops`` the list of ("call", u) and ("jump", s) in order, a jump following the call
    at s + 1; the number of model calls, of jumps and of jump points.  calls == U + (r - 1) * j * points."""
    U, j, r = int(U), int(jump_length), int(n_resample)
    if U < 1 or j < 1 or r < 1:
        raise ValueError("resample_schedule: U, jump_length and n_resample must be >= 1, got %r" % ((U, j, r),))
    if times is not None and len(times) != U:
        raise ValueError("resample_schedule: %d times for %d calls" % (len(times), U))
    time_of = (lambda u: u) if times is None else (lambda u: int(times[U - 1 - u]))
    budget = {s: r - 1 for s in range(0, U - j, j) if resample_steps is None or time_of(s) < resample_steps}
    points = sum(1 for v in budget.values() if v > 0)
    out, calls, jumps = [], 0, 0
    u = U
    while u >= 1:
        u -= 1
        out.append(("call", u))
        calls += 1
        s = u - 1
        if budget.get(s, 0) > 0:
            budget[s] -= 1
            out.append(("jump", s))
            jumps += 1
            u = s + j + 1
    return ResampleSchedule(out, calls, jumps, points)


def jump_tables(alphas_cumprod, jump_length, times=None):
    """(ja, jb) float32 CPU tables of dsc_resample_jump_f32 from the float64 ``alphas_cumprod`` (T,): ja = sqrt(abar[time(s + j)] /
    abar[time(s)]), jb = sqrt(1 - that ratio), float64 on the host, rounded once.  ``times`` None: T rows indexed by s (time(s) = s);
    else S rows indexed by the step counter k of the pair at s (time = times[k], the target times[k - j]).  A row that no jump can start
    from (s + j > T - 1, k < j) holds (1, 0)."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    j = int(jump_length)
    if ac.ndim != 1 or j < 1:
        raise ValueError("jump_tables: alphas_cumprod must be a (T,) float64 table and jump_length >= 1")
    if times is None:
        n = ac.shape[0]
        src = np.arange(n)
        dst = src + j
        ok = dst < n
        frm, to = ac[src[ok]], ac[dst[ok]]
    else:
        tm = np.asarray([int(v) for v in times], dtype=np.int64)
        n = tm.shape[0]
        k = np.arange(n)
        ok = k >= j
        frm, to = ac[tm[k[ok]]], ac[tm[k[ok] - j]]
    ratio = np.ones((n,), dtype=np.float64)
    ratio[ok] = to / frm
    ja, jb = np.sqrt(ratio), np.sqrt(1.0 - ratio)
    return torch.from_numpy(ja.astype(np.float32)), torch.from_numpy(jb.astype(np.float32))


def jump_rec(x, noise, ja, jb, jump, t=None, strided=None, rows=None, mask=None, q=(), x_dup=None):
    """The launch record of one resampling jump (dsc_resample_jump_f32), in place on ``x``: the time source -- ``t`` (B,) int64 holding s,
    or ``strided`` = (step, times, ...) with the counter on the pair at s --, the tables of jump_tables on the device, and optionally the
    given part of the NEXT model call, ``rows`` = (partial, noise_p, counts) or ``mask`` = (known, noise_k, mask) with ``q`` = (sqrt_ac,
    sqrt_1mac): the fused form.  ``x_dup``: the null half of a guided loop's state."""
    if rows is not None and mask is not None:
        raise ValueError("diffuscene_amd: resample_jump takes one given part, rows or mask")
    if (t is None) == (strided is None):
        raise ValueError("diffuscene_amd: resample_jump takes one time source, t or strided")
    given = rows if rows is not None else mask
    if len(q) != (2 if given is not None else 0):
        raise ValueError("diffuscene_amd: resample_jump takes q = (sqrt_ac, sqrt_1mac) with a given part and only then")
    _c(x, "x"); _c(noise, "noise"); _c(ja, "ja"); _c(jb, "jb")
    jump = int(jump)
    if jump < 1:
        raise ValueError("diffuscene_amd: resample_jump needs jump >= 1, got %d" % jump)
    b = x.shape[0]
    _same_shape("resample_jump", x, noise, x_dup)
    if x_dup is not None:
        _c(x_dup, "x_dup")
    T = _table_rows(*q) if q else 2 ** 31 - 1
    tp = sp = tmp = None
    S = 0
    if strided is not None:
        step, times = strided[0], strided[1]
        _dev(step, "step", torch.int64); _dev(times, "times", torch.int64)
        if not times.is_contiguous():
            raise RuntimeError("diffuscene_amd: times must be contiguous")
        sp, tmp, S = step.data_ptr(), times.data_ptr(), times.numel()
        if _table_rows(ja, jb) != S:
            raise RuntimeError("diffuscene_amd: ja / jb of a strided jump hold one row per pair (%d)" % S)
    else:
        _scene_t(t, b)
        tp = t.data_ptr()
        rows_j = _table_rows(ja, jb)
        if q and rows_j != T:
            raise RuntimeError("diffuscene_amd: ja / jb (%d rows) and the schedule tables (%d rows) differ" % (rows_j, T))
        T = rows_j
    gp = ngp = mk = counts = None
    pmax = c = 0
    if rows is not None:
        _dev(rows[2], "counts", torch.int64)
        _, _, pmax, c, cnt = _ragged_args(x, *rows)
        gp, ngp, counts = rows[0].data_ptr(), rows[1].data_ptr(), cnt.data_ptr()
    if mask is not None:
        _masked_args(x, *mask)
        gp, ngp, mk = mask[0].data_ptr(), mask[1].data_ptr(), mask[2].data_ptr()
    args = (x.data_ptr(), noise.data_ptr(), ja.data_ptr(), jb.data_ptr(), tp, sp, tmp, gp, ngp, mk, counts,
            q[0].data_ptr() if q else None, q[1].data_ptr() if q else None, _opt(x_dup), jump, b, x.numel() // b, pmax, c, S, T)
    return "dsc_resample_jump_f32", args, (x, noise, ja, jb, t, strided, rows, mask, q, x_dup)


def resample_jump(x, noise, ja, jb, jump, **operands):
    """One resampling jump in place (jump_rec issued at once) -> x."""
    issue(jump_rec(x, noise, ja, jb, jump, **operands))
    return x


def ddim_seek(step, times, t, delta):
    """step += delta; t[:] = times[step] (device-side, capturable): the move after a jump in a strided loop."""
    _dev(step, "step", torch.int64); _dev(t, "t", torch.int64); _dev(times, "times", torch.int64)
    if not times.is_contiguous():
        raise RuntimeError("diffuscene_amd: times must be contiguous")
    _lib.check(_lib.fn("dsc_ddim_seek_i64")(step.data_ptr(), times.data_ptr(), t.data_ptr(), t.numel(), times.numel(), int(delta),
                                            stream_ptr()), "dsc_ddim_seek_i64")
    return t


def scene_gate(x, keep, out=None):
    """y[b] = keep[b] ? x[b] : 0 for a (B, ...) f32 tensor and a (B,) bool / uint8 device tensor; a dropped scene is not read.  See the C
    header."""
    _c(x, "x")
    if not isinstance(keep, torch.Tensor) or not keep.is_cuda or keep.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("diffuscene_amd: keep must be a bool / uint8 tensor on the HIP device")
    b = x.shape[0]
    if tuple(keep.shape) != (b,):
        raise RuntimeError("diffuscene_amd: keep must be (%d,), got %s" % (b, tuple(keep.shape)))
    keep = keep.contiguous()
    kb = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.fn("dsc_scene_gate_f32")(x.data_ptr(), kb.data_ptr(), _c(out, "out").data_ptr(), b, x.numel() // b, stream_ptr()),
               "dsc_scene_gate_f32")
    return out


# ---------------------------------------------------------------------------------- training (backward) kernels

_scratch = {}


def scratch(device, floats):
    """Scratch for split reductions, one buffer per (device, stream): kernels run in order on a stream, so it is reused."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    t = _scratch.get(key)
    if t is None or t.numel() < floats:
        t = torch.empty(max(int(floats), 1 << 20), device=device, dtype=torch.float32)
        _scratch[key] = t
    return t


def transpose_rec(w, out):
    if tuple(out.shape) != (w.shape[1], w.shape[0]):
        raise RuntimeError("transpose: out must be %s, got %s" % ((w.shape[1], w.shape[0]), tuple(out.shape)))
    return "dsc_transpose_f32", _mats((w, "w"), (out, "out")) + tuple(w.shape), (w, out)


def transpose(w, out=None, ldo=None):
    if out is None:
        out = torch.empty((w.shape[1], w.shape[0]), device=w.device, dtype=torch.float32)
    issue(transpose_rec(w, out))
    return out


def transpose_batched_rec(pairs):
    """pairs: <= DSC_WS_MAX of (w (rows, cols), out (cols, rows)), both contiguous."""
    arr = (WsItem * len(pairs))()
    for j, (m, o) in enumerate(pairs):
        if not (_dev(m).is_contiguous() and m.dim() == 2 and _dev(o).is_contiguous()):
            raise RuntimeError("transpose_many needs contiguous 2-D matrices")
        arr[j].w, arr[j].out = m.data_ptr(), o.data_ptr()
        arr[j].rows, arr[j].cols = m.shape
    return "dsc_transpose_batched_f32", (arr, len(pairs)), (arr, pairs)


def transpose_many(mats):
    """[w_i (rows_i, cols_i)] -> [w_i^T], one launch per DSC_WS_MAX matrices."""
    outs = [torch.empty((m.shape[1], m.shape[0]), device=m.device, dtype=torch.float32) for m in mats]
    for i in range(0, len(mats), _lib.WS_MAX):
        issue(transpose_batched_rec(list(zip(mats[i:i + _lib.WS_MAX], outs[i:i + _lib.WS_MAX]))))
    return outs


def copy2d_rec(dst, src):
    """dst = src, row-major 2-D views of one shape (arbitrary alignment)."""
    return "dsc_copy2d_f32", _mats((dst, "dst"), (src, "src")) + tuple(dst.shape), (dst, src)


def add2d_rec(dst, src):
    """dst += src."""
    return "dsc_add2d_f32", _mats((dst, "dst"), (src, "src")) + tuple(dst.shape), (dst, src)


def tn_operands(a, dy, out, a2=None, kvalid=None, what="gemm_tn"):
    """The operand run (a1, lda1, k1, a2, lda2, k2, dy, ldd, out, ldo) and (m, n, kvalid) of one weight-gradient product
    out[n][k] = sum_m dy[m][n] * [a|a2][m][k], after the shape and alignment checks dsc_gemm_tn_f32 makes on the host -- made here
    because the grouped entry points see only a device table of these."""
    ap, lda, a2p, lda2, dp, ldd, op, ldo = _mats((a, "a"), (a2, "a2"), (dy, "dy"), (out, "out"))
    k1, k2 = a.shape[1], (a2.shape[1] if a2 is not None else 0)
    m, n = dy.shape
    kv = (k1 + k2) if kvalid is None else kvalid
    if (k1 & 3) or (k2 & 3) or (n & 3) or (k2 > 0 and k1 % 128) or not (1 <= kv <= k1 + k2):
        raise RuntimeError("%s: bad shape m=%d n=%d k1=%d k2=%d kvalid=%d" % (what, m, n, k1, k2, kv))
    if (ap % 16) or (lda & 3) or (dp % 16) or (ldd & 3) or (k2 and ((a2p % 16) or (lda2 & 3))):
        raise RuntimeError("%s: operands must be 16-byte aligned with row strides multiple of 4" % what)
    if a.shape[0] != m or (a2 is not None and a2.shape[0] != m) or tuple(out.shape) != (n, kv):
        raise RuntimeError("%s: shape mismatch" % what)
    return (ap, lda, k1, a2p, lda2, k2, dp, ldd, op, ldo), (m, n, kv)


def gemm_tn_rec(a, dy, out, a2, kvalid, dbias, ws_ptr, ws_floats):
    """``ws_ptr`` / ``ws_floats``: the caller's workspace of at least dsc_gemm_tn_workspace_floats(m, n, kvalid) floats (None, 0 when that is 0)."""
    run, (m, n, kv) = tn_operands(a, dy, out, a2, kvalid)
    return "dsc_gemm_tn_f32", run + (_opt(dbias), m, n, kv, ws_ptr, ws_floats), (a, dy, out, a2, dbias)


def gemm_tn(a, dy, a2=None, kvalid=None, out=None, want_bias=False):
    """out[n][k] = sum_m dy[m][n] * [a|a2][m][k]  (+ column sums of dy when want_bias) -> out or (out, dbias)"""
    m, n = dy.shape
    kv = (a.shape[1] + (a2.shape[1] if a2 is not None else 0)) if kvalid is None else kvalid
    if out is None:
        out = torch.empty((n, kv), device=a.device, dtype=torch.float32)
    wsf = _lib.fn("dsc_gemm_tn_workspace_floats")(m, n, kv)
    ws = scratch(a.device, wsf) if wsf else None
    db = torch.empty((n,), device=a.device, dtype=torch.float32) if want_bias else None
    issue(gemm_tn_rec(a, dy, out, a2, kvalid, db, _opt(ws), ws.numel() if ws is not None else 0))
    return (out, db) if want_bias else out


def colsum_rec(x, out, ws_ptr, ws_floats):
    """out[n] = column sums of x [m, n]; the workspace holds at least 64 n floats."""
    xp, ldx = _mat(x, "x")
    m, n = x.shape
    return "dsc_colsum_f32", (xp, ldx, m, n, out.data_ptr(), ws_ptr, ws_floats), (x, out)


def colsum(x, out=None):
    if out is None:
        out = torch.empty((x.shape[1],), device=x.device, dtype=torch.float32)
    ws = scratch(x.device, 64 * x.shape[1])
    issue(colsum_rec(x, out, ws.data_ptr(), ws.numel()))
    return out


def device_table(arr, device):
    """A ctypes array of structs as a uint8 device tensor (the grouped entry points read their items from device memory)."""
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(device)


def colsum_grouped_rec(pairs, device):
    """pairs: [(x [m, n] with contiguous rows, out [n] contiguous)] -> ONE launch over a device table of them."""
    arr = (_lib.ColsumItem * len(pairs))()
    for i, (x, out) in enumerate(pairs):
        if not (out.is_contiguous() and out.numel() == x.shape[1]):
            raise RuntimeError("colsum_grouped: out must be a contiguous (%d,) tensor" % x.shape[1])
        arr[i].x, arr[i].ldx = _mat(x, "x")
        arr[i].m, arr[i].n, arr[i].out = x.shape[0], x.shape[1], out.data_ptr()
    table = device_table(arr, device)
    return "dsc_colsum_grouped_f32", (table.data_ptr(), len(pairs), max(x.shape[1] for x, _ in pairs)), (table, pairs)


def gn_silu_bwd_rec(z, dy, gamma, beta, ss, ss_mode, dz, part, order, dss, scenes, n_tok, eps=1e-5):
    """``part`` [scenes, 3 C]: the per-scene partial sums, three blocks of C columns; ``order`` = the block index of (dgamma, dbeta,
    dbias) in a row.  ``ss`` None: no scale / shift."""
    zp, ldz, dp, ldy, sp, ld_ss, dzp, lddz, dsp, ld_dss = _mats((z, "z"), (dy, "dy"), (ss, "ss"), (dz, "dz"), (dss, "dss"))
    Cc = z.shape[1]
    pg, pb, pB = (_mat(part, "part")[0] + 4 * Cc * o for o in order)
    return ("dsc_gn_silu_bwd_f32", (zp, ldz, dp, ldy, _dev(gamma).data_ptr(), _dev(beta).data_ptr(), sp, ld_ss,
                                    ss_mode if sp else SS_NONE, dzp, lddz, pg, pb, pB, part.stride(0), dsp, ld_dss, scenes, n_tok,
                                    Cc, eps), (z, dy, gamma, beta, ss, dz, part, dss))


def gn_silu_bwd(z, dy, gamma, beta, ss, ss_mode, scenes, n_tok, eps=1e-5):
    """-> dz [M,512], (dgamma, dbeta, dbias) [512] each, dss (per-scene [B,1024] | per-token [M,1024] | None)"""
    M, Cc = z.shape
    dz = torch.empty((M, Cc), device=z.device, dtype=torch.float32)
    part = torch.empty((scenes, 3 * Cc), device=z.device, dtype=torch.float32)     # [dgamma | dbeta | dbias] per scene
    dss = None
    if ss is not None and ss_mode != SS_NONE:
        dss = torch.empty((scenes if ss_mode == SS_PER_SCENE else M, 2 * Cc), device=z.device, dtype=torch.float32)
    issue(gn_silu_bwd_rec(z, dy, gamma, beta, ss if dss is not None else None, ss_mode, dz, part, (0, 1, 2), dss, scenes, n_tok, eps))
    red = colsum(part)                  # one column sum over the scenes for the three per-channel gradients
    return dz, red[:Cc], red[Cc:2 * Cc], red[2 * Cc:], dss


def weight_standardize_bwd_rec(triples, eps=1e-5):
    """triples: <= DSC_WS_MAX of (w, dw_std, dw), contiguous matrices (w, dw may be (out, in, 1) conv weights)."""
    arr = (_lib.WsBwdItem * len(triples))()
    for j, (w, g, o) in enumerate(triples):
        w2, g2, o2 = as2d(_dev(w)), _dev(g), as2d(_dev(o))
        if not (w2.is_contiguous() and g2.is_contiguous() and o2.is_contiguous()):
            raise RuntimeError("weight_standardize_bwd needs contiguous matrices")
        arr[j].w, arr[j].dw_std, arr[j].dw = w2.data_ptr(), g2.data_ptr(), o2.data_ptr()
        arr[j].rows, arr[j].cols = w2.shape
    return "dsc_weight_standardize_bwd_f32", (arr, len(triples), eps), (arr, triples)


def weight_standardize_bwd(weights, dw_stds, eps=1e-5):
    outs = [torch.empty_like(as2d(w)) for w in weights]
    for i in range(0, len(weights), _lib.WS_MAX):
        s = slice(i, i + _lib.WS_MAX)
        issue(weight_standardize_bwd_rec(list(zip(weights[s], dw_stds[s], outs[s])), eps))
    return outs


def layernorm_bwd_rec(x, g, dy, dx, dg_part, addend=None, eps=1e-5):
    """dx (+ ``addend``) and, per block of rows, one row of ``dg_part`` [blocks, D] with the gain's partial gradient."""
    run = _mats((dy, "dy"), (dx, "dx"), (addend, "addend"))
    return ("dsc_layernorm_bwd_f32", _mat(x, "x") + (_dev(g).data_ptr(),) + run + (dg_part.data_ptr(), dg_part.shape[0], x.shape[0],
                                                                                   x.shape[1], eps), (x, g, dy, dx, dg_part, addend))


def layernorm_bwd(x, g, dy, eps=1e-5):
    M, Dd = x.shape
    dx = torch.empty((M, Dd), device=x.device, dtype=torch.float32)
    part = torch.empty((min((M + 3) // 4, 512), Dd), device=x.device, dtype=torch.float32)
    issue(layernorm_bwd_rec(x, g, dy, dx, part, None, eps))
    return dx, colsum(part)


def _qkv_grads(q, k, v, dout, dq, dk, dv):
    return _mats((q, "q"), (k, "k"), (v, "v"), (dout, "dout"), (dq, "dq"), (dk, "dk"), (dv, "dv"))


def linear_attention_bwd_rec(q, k, v, dout, dq, dk, dv, scenes, nq, nk, scale):
    return "dsc_linear_attention_bwd_f32", _qkv_grads(q, k, v, dout, dq, dk, dv) + (scenes, nq, nk, scale), (q, k, v, dout, dq, dk, dv)


def linear_attention_bwd(q, k, v, dout, dq, dk, dv, scenes, nq, nk, scale):
    issue(linear_attention_bwd_rec(q, k, v, dout, dq, dk, dv, scenes, nq, nk, scale))


def attention_bwd_rec(q, k, v, dout, dq, dk, dv, scenes, n, scale):
    return "dsc_attention_bwd_f32", _qkv_grads(q, k, v, dout, dq, dk, dv) + (scenes, n, scale), (q, k, v, dout, dq, dk, dv)


def attention_bwd(q, k, v, dout, dq, dk, dv, scenes, n, scale):
    issue(attention_bwd_rec(q, k, v, dout, dq, dk, dv, scenes, n, scale))


def activation_bwd_rec(x, dy, dx, act):
    _c(x, "x"); _c(dy, "dy"); _c(dx, "dx")
    return "dsc_activation_bwd_f32", (x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), act), (x, dy, dx)


def activation_bwd(x, dy, act):
    dx = torch.empty_like(x)
    issue(activation_bwd_rec(x, dy, dx, act))
    return dx


def ddpm_loss_rec(target, out, x_t, t, loss_weight, ca, cb, alphas_cumprod, bounds, dims, separate, iou, mean_type, grad_scale,
                  losses, parts, dout):
    _c(target, "target"); _c(out, "out"); _c(x_t, "x_t"); _dev(t, "t", torch.int64)
    B, N, Cc = out.shape
    barr = (C.c_float * 12)(*[float(v) for v in bounds]) if bounds is not None else None
    return ("dsc_ddpm_loss_f32", (
        target.data_ptr(), out.data_ptr(), x_t.data_ptr(), t.data_ptr(), loss_weight.data_ptr(), _opt(ca), _opt(cb),
        _opt(alphas_cumprod), barr, losses.data_ptr(), parts.data_ptr(), dout.data_ptr(), B, N, Cc, dims["translation_dim"],
        dims["size_dim"], dims["bbox_dim"], dims["class_dim"], dims["objectness_dim"], dims["objfeat_dim"], 1 if separate else 0,
        1 if iou else 0, mean_type, float(grad_scale), _table_rows(loss_weight, ca, cb, alphas_cumprod)),
        (target, out, x_t, t, loss_weight, ca, cb, alphas_cumprod, barr, losses, parts, dout))


def ddpm_loss(target, out, x_t, t, loss_weight, ca, cb, alphas_cumprod, bounds, dims, separate, iou, mean_type,
              grad_scale=1.0):
    """-> losses_weight [B], parts [B, 9], dout [B, N, C] (grad_scale * d losses_weight[b] / d out[b])"""
    B = out.shape[0]
    losses = torch.empty((B,), device=out.device, dtype=torch.float32)
    parts = torch.empty((B, 9), device=out.device, dtype=torch.float32)
    dout = torch.empty_like(out)
    issue(ddpm_loss_rec(target, out, x_t, t, loss_weight, ca, cb, alphas_cumprod, bounds, dims, separate, iou, mean_type, grad_scale,
                        losses, parts, dout))
    return losses, parts, dout


# ---------------------------------------------------------------------------------- floor-plan encoder (csrc/floorplan.hip)

def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv_kpad(c, k):
    """Columns of a patch row: k * k * c rounded up to the K granule of the GEMMs (32)."""
    return (k * k * c + 31) // 32 * 32


def _image(x, geom, name):
    """x [b * h * w][c] contiguous on the device for geom = (b, h, w) -> c."""
    _c(x, name)
    b, h, w = geom
    if x.dim() != 2 or x.shape[0] != b * h * w:
        raise RuntimeError("diffuscene_amd: %s must be [%d * %d * %d][c], got %s" % (name, b, h, w, tuple(x.shape)))
    return x.shape[1]


def conv_patches(x, geom, k, stride, pad, out=None):
    """Patch rows of a k x k convolution over x [b * h * w][c] (dsc_conv_patches_f32) -> [b * ho * wo][conv_kpad(c, k)]."""
    c = _image(x, geom, "x")
    b, h, w = geom
    rows = b * conv_out_size(h, k, stride, pad) * conv_out_size(w, k, stride, pad)
    if out is None:
        out = torch.empty((max(rows, 0), conv_kpad(c, k)), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (rows, conv_kpad(c, k)):
        raise RuntimeError("conv_patches: out must be %s, got %s" % ((rows, conv_kpad(c, k)), tuple(out.shape)))
    _lib.check(_lib.fn("dsc_conv_patches_f32")(x.data_ptr(), _c(out, "out").data_ptr(), b, h, w, c, k, stride, pad, stream_ptr()),
               "dsc_conv_patches_f32")
    return out


def conv_patches_bwd(dpatches, geom, c, k, stride, pad, out=None):
    """Gradient of conv_patches: dpatches [b * ho * wo][kpad] -> dx [b * h * w][c] (dsc_conv_patches_bwd_f32)."""
    b, h, w = geom
    rows = b * conv_out_size(h, k, stride, pad) * conv_out_size(w, k, stride, pad)
    if tuple(_c(dpatches, "dpatches").shape) != (rows, conv_kpad(c, k)):
        raise RuntimeError("conv_patches_bwd: dpatches must be %s, got %s" % ((rows, conv_kpad(c, k)), tuple(dpatches.shape)))
    if out is None:
        out = torch.empty((b * h * w, c), device=dpatches.device, dtype=torch.float32)
    elif tuple(out.shape) != (b * h * w, c):
        raise RuntimeError("conv_patches_bwd: out must be %s, got %s" % ((b * h * w, c), tuple(out.shape)))
    _lib.check(_lib.fn("dsc_conv_patches_bwd_f32")(dpatches.data_ptr(), _c(out, "out").data_ptr(), b, h, w, c, k, stride, pad,
                                                   stream_ptr()), "dsc_conv_patches_bwd_f32")
    return out


def maxpool2d(x, geom, out=None, arg=None):
    """nn.MaxPool2d(3, 2, 1) over x [b * h * w][c] (dsc_maxpool2d_f32) -> (y [b * ho * wo][c], arg uint8 window slots)."""
    c = _image(x, geom, "x")
    b, h, w = geom
    rows = b * conv_out_size(h, 3, 2, 1) * conv_out_size(w, 3, 2, 1)
    if out is None:
        out = torch.empty((rows, c), device=x.device, dtype=torch.float32)
    if arg is None:
        arg = torch.empty((rows, c), device=x.device, dtype=torch.uint8)
    if tuple(out.shape) != (rows, c) or tuple(arg.shape) != (rows, c) or not arg.is_contiguous() or arg.dtype != torch.uint8:
        raise RuntimeError("maxpool2d: out / arg must be contiguous %s float32 / uint8" % ((rows, c),))
    _lib.check(_lib.fn("dsc_maxpool2d_f32")(x.data_ptr(), _c(out, "out").data_ptr(), arg.data_ptr(), b, h, w, c, stream_ptr()),
               "dsc_maxpool2d_f32")
    return out, arg


def maxpool2d_bwd(dy, arg, geom, out=None):
    """dy, arg [b * ho * wo][c] -> dx [b * h * w][c] (dsc_maxpool2d_bwd_f32)."""
    b, h, w = geom
    rows = b * conv_out_size(h, 3, 2, 1) * conv_out_size(w, 3, 2, 1)
    c = _c(dy, "dy").shape[1]
    if dy.shape[0] != rows or tuple(arg.shape) != (rows, c) or not arg.is_cuda or arg.dtype != torch.uint8 or not arg.is_contiguous():
        raise RuntimeError("maxpool2d_bwd: dy / arg must be contiguous %s float32 / uint8" % ((rows, c),))
    if out is None:
        out = torch.empty((b * h * w, c), device=dy.device, dtype=torch.float32)
    elif tuple(out.shape) != (b * h * w, c):
        raise RuntimeError("maxpool2d_bwd: out must be %s, got %s" % ((b * h * w, c), tuple(out.shape)))
    _lib.check(_lib.fn("dsc_maxpool2d_bwd_f32")(dy.data_ptr(), arg.data_ptr(), _c(out, "out").data_ptr(), b, h, w, c, stream_ptr()),
               "dsc_maxpool2d_bwd_f32")
    return out


def _bn_vectors(ch, *named):
    for t, name in named:
        if tuple(_c(t, name).shape) != (ch,):
            raise RuntimeError("diffuscene_amd: %s must be (%d,), got %s" % (name, ch, tuple(t.shape)))


def frozen_bn_act(x, weight, bias, running_mean, running_var, residual=None, relu=False, out=None):
    """y = act(x * s + t (+ residual)) over x [rows][ch], s = weight / sqrt(running_var), t = bias - running_mean * s
    (dsc_frozen_bn_act_f32); weight None (then all four): y = act(x (+ residual))."""
    rows, ch = _c(x, "x").shape
    if weight is not None:
        _bn_vectors(ch, (weight, "weight"), (bias, "bias"), (running_mean, "running_mean"), (running_var, "running_var"))
    if residual is not None and tuple(_c(residual, "residual").shape) != (rows, ch):
        raise RuntimeError("frozen_bn_act: residual must be %s" % ((rows, ch),))
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != (rows, ch):
        raise RuntimeError("frozen_bn_act: out must be %s" % ((rows, ch),))
    _lib.check(_lib.fn("dsc_frozen_bn_act_f32")(x.data_ptr(), _opt(weight), _opt(bias), _opt(running_mean), _opt(running_var),
                                                _opt(residual), _c(out, "out").data_ptr(), rows, ch, 1 if relu else 0, stream_ptr()),
               "dsc_frozen_bn_act_f32")
    return out


def frozen_bn_act_bwd(dy, y, x, weight, running_mean, running_var, relu=False, want_residual=False, outs=None):
    """-> (dx, dresidual or None, dweight or None, dbias or None) of frozen_bn_act (dsc_frozen_bn_act_bwd_f32); ``y`` is the forward's
    output (read only with ``relu``), ``x`` its input (read only with a ``weight``).  ``outs``: that tuple preallocated."""
    rows, ch = _c(dy, "dy").shape
    for t, name in ((y, "y"), (x, "x")):
        if t is not None and tuple(_c(t, name).shape) != (rows, ch):
            raise RuntimeError("frozen_bn_act_bwd: %s must be %s" % (name, (rows, ch)))
    dx, dres, dw, db = outs if outs is not None else (None, None, None, None)
    dx = torch.empty_like(dy) if dx is None else dx
    dres = torch.empty_like(dy) if want_residual and dres is None else dres
    ws = None
    if weight is not None:
        _bn_vectors(ch, (weight, "weight"), (running_mean, "running_mean"), (running_var, "running_var"))
        dw = torch.empty((ch,), device=dy.device, dtype=torch.float32) if dw is None else dw
        db = torch.empty((ch,), device=dy.device, dtype=torch.float32) if db is None else db
        _bn_vectors(ch, (dw, "dweight"), (db, "dbias"))
    for t, name in ((dx, "dx"), (dres, "dresidual")):
        if t is not None and tuple(_c(t, name).shape) != (rows, ch):
            raise RuntimeError("frozen_bn_act_bwd: %s must be %s" % (name, (rows, ch)))
    if weight is not None:
        wsf = _lib.fn("dsc_frozen_bn_workspace_floats")(rows, ch)
        if wsf < 0:
            _lib.check(int(wsf), "dsc_frozen_bn_workspace_floats")
        ws = scratch(dy.device, wsf)
    _lib.check(_lib.fn("dsc_frozen_bn_act_bwd_f32")(dy.data_ptr(), _opt(y), _opt(x if weight is not None else None), _opt(weight),
                                                    _opt(running_mean), _opt(running_var), dx.data_ptr(), _opt(dres), _opt(dw), _opt(db),
                                                    rows, ch, 1 if relu else 0, _opt(ws), ws.numel() if ws is not None else 0,
                                                    stream_ptr()), "dsc_frozen_bn_act_bwd_f32")
    return dx, dres, dw, db


def avgpool_rows(x, b, out=None):
    """x [b * hw][ch] -> the mean over hw, [b][ch] (dsc_avgpool_rows_f32)."""
    rows, ch = _c(x, "x").shape
    if b < 1 or rows % b:
        raise RuntimeError("avgpool_rows: %d rows are not %d images" % (rows, b))
    if out is None:
        out = torch.empty((b, ch), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (b, ch):
        raise RuntimeError("avgpool_rows: out must be %s" % ((b, ch),))
    _lib.check(_lib.fn("dsc_avgpool_rows_f32")(x.data_ptr(), _c(out, "out").data_ptr(), b, rows // b, ch, stream_ptr()),
               "dsc_avgpool_rows_f32")
    return out


def avgpool_rows_bwd(dy, hw, out=None):
    """dy [b][ch] -> dx [b * hw][ch] = dy / hw (dsc_avgpool_rows_bwd_f32)."""
    b, ch = _c(dy, "dy").shape
    if out is None:
        out = torch.empty((b * hw, ch), device=dy.device, dtype=torch.float32)
    elif tuple(out.shape) != (b * hw, ch):
        raise RuntimeError("avgpool_rows_bwd: out must be %s" % ((b * hw, ch),))
    _lib.check(_lib.fn("dsc_avgpool_rows_bwd_f32")(dy.data_ptr(), _c(out, "out").data_ptr(), b, hw, ch, stream_ptr()),
               "dsc_avgpool_rows_bwd_f32")
    return out
