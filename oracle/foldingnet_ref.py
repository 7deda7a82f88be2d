"""Numpy float64 statements of the FoldingNet kernels (TEST INFRASTRUCTURE, see oracle/__init__.py): one function per C entry
point of csrc/foldingnet.hip, written from the operation each kernel's comment states, plus the input builders whose
discrete outcomes (neighbour lists, arg-max winners, scatter sums) have exactly one right answer in fp32.  No torch in the
maths; tests/test_foldingnet_ref_host.py pins every function against torch in float64 and asserts the builders'
properties.

Layout everywhere: token-major rows [cloud * n + point][channel]."""
import numpy as np

K = 16


def _f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------ neighbour search
def knn_scores(x, clouds, n):
    """score[b, i, j] = 2 <x_i, x_j> - |x_j|^2 inside cloud b (the ranking of reference knn() without the per-query constant)."""
    x = _f64(x).reshape(clouds, n, -1)
    return 2.0 * np.einsum("bid,bjd->bij", x, x) - (x * x).sum(-1)[:, None, :]


def knn16(x, clouds, n):
    """x [clouds*n, d] -> (idx int32 [clouds*n, 16], gap [clouds*n], min_adjacent_gap [clouds*n]).

    idx: the 16 best scores per query inside its cloud, best first, ties to the lowest index.  gap: score_16th - score_17th
    (inf when n == 16).  min_adjacent_gap: the smallest difference between neighbouring entries of the first 17 sorted scores:
    0 means the ORDER rests on the tie rule somewhere, gap == 0 means the neighbour SET does."""
    s = knn_scores(x, clouds, n)
    order = np.argsort(-s, axis=-1, kind="stable")
    top = np.take_along_axis(s, order[..., :min(n, K + 1)], -1)
    gap = top[..., K - 1] - top[..., K] if n > K else np.full(s.shape[:2], np.inf)
    adj = (top[..., :-1] - top[..., 1:]).min(-1)
    return order[..., :K].reshape(clouds * n, K).astype(np.int32), gap.reshape(-1), adj.reshape(-1)


def rowsq(x):
    x = _f64(x)
    return (x * x).sum(-1)


def knn_cov(xyz, idx, clouds, n):
    """[rows, 12]: xyz | row-major 3x3 sum over the 16 neighbours of (x_k - mean)(x_k - mean)^T."""
    xyz = _f64(xyz).reshape(clouds, n, 3)
    nb = np.take_along_axis(xyz[:, None, :, :], np.asarray(idx, np.int64).reshape(clouds, n, K, 1), 2)      # [b, n, 16, 3]
    c = nb - nb.mean(2, keepdims=True)
    cov = np.einsum("bnka,bnkc->bnac", c, c).reshape(clouds, n, 9)
    return np.concatenate([xyz, cov], -1).reshape(clouds * n, 12)


# ------------------------------------------------------------------------------------------------ pooling
def _gathered(x, idx, clouds, n):
    x = _f64(x)
    ch = x.shape[1]
    idx = np.asarray(idx, np.int64).reshape(clouds, n, K)
    return np.take_along_axis(x.reshape(clouds, 1, n, ch), idx[..., None], 2)                                # [b, n, 16, ch]


def gather_max(x, idx, clouds, n):
    """(value [rows, ch], k [rows, ch]): maximum over the 16 listed neighbours; the first maximum in list order wins."""
    g = _gathered(x, idx, clouds, n)
    k = g.argmax(2)                                                                                          # first occurrence
    return np.take_along_axis(g, k[:, :, None, :], 2)[:, :, 0, :].reshape(clouds * n, -1), k.reshape(clouds * n, -1)


def gather_max_ties(x, idx, clouds, n):
    """Number of (query, channel) pairs whose maximum is attained by more than one list entry."""
    g = _gathered(x, idx, clouds, n)
    return int(((g == g.max(2, keepdims=True)).sum(2) > 1).sum())


def gather_max_bwd(dy, idx, k, clouds, n):
    """dx[cloud row of idx[q, k[q, c]], c] += dy[q, c]."""
    dy = _f64(dy)
    rows, ch = dy.shape
    idx = np.asarray(idx, np.int64)
    src = np.take_along_axis(idx, np.asarray(k, np.int64), 1) + (np.arange(rows) // n * n)[:, None]         # [rows, ch]
    dx = np.zeros((rows, ch))
    np.add.at(dx, (src, np.broadcast_to(np.arange(ch), (rows, ch))), dy)
    return dx


def rowmax(x, clouds, n):
    """(value [clouds, ch], point [clouds, ch]): maximum over the points of a cloud; the lowest point index wins."""
    x = _f64(x).reshape(clouds, n, -1)
    p = x.argmax(1)
    return np.take_along_axis(x, p[:, None, :], 1)[:, 0, :], p.astype(np.int32)


def rowmax_bwd(dy, arg, clouds, n):
    dy = _f64(dy)
    hit = np.arange(n)[None, :, None] == np.asarray(arg)[:, None, :]
    return np.where(hit, dy[:, None, :], 0.0).reshape(clouds * n, -1)


# ------------------------------------------------------------------------------------------------ BatchNorm1d
def batchnorm_fwd(x, gamma, beta, eps, relu, running_mean=None, running_var=None, momentum=0.1):
    """Training mode over the rows of x.  Returns a dict: y, xhat, mean, var (biased), rstd, pre (the value before the ReLU)
    and, when running statistics are given, their update running_mean / running_var (momentum, unbiased variance)."""
    x, gamma, beta = _f64(x), _f64(gamma), _f64(beta)
    rows = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    pre = xhat * gamma + beta
    out = dict(y=np.maximum(pre, 0.0) if relu else pre, pre=pre, xhat=xhat, mean=mean, var=var, rstd=rstd)
    if running_mean is not None:
        unb = var * rows / (rows - 1) if rows > 1 else var
        out["running_mean"] = (1.0 - momentum) * _f64(running_mean) + momentum * mean
        out["running_var"] = (1.0 - momentum) * _f64(running_var) + momentum * unb
    return out


def batchnorm_bwd(dy, x, gamma, beta, eps, relu):
    """(dx, dgamma, dbeta) of y = relu?(BatchNorm(x)) for the upstream gradient dy; with ReLU the mask is y > 0."""
    f = batchnorm_fwd(x, gamma, beta, eps, relu)
    g = _f64(dy)
    if relu:
        g = np.where(f["y"] > 0.0, g, 0.0)
    xhat = f["xhat"]
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    rows = xhat.shape[0]
    dx = _f64(gamma) * f["rstd"] * (g - dbeta / rows - xhat * (dgamma / rows))
    return dx, dgamma, dbeta


def batchnorm_eval(x, gamma, beta, running_mean, running_var, eps, relu):
    pre = (_f64(x) - _f64(running_mean)) / np.sqrt(_f64(running_var) + eps) * _f64(gamma) + _f64(beta)
    return np.maximum(pre, 0.0) if relu else pre


# ------------------------------------------------------------------------------------------------ fold convolution
def _point_rows(x, clouds, n, per_cloud):
    x = _f64(x)
    return x.reshape(clouds, n, -1) if per_cloud else np.broadcast_to(x[None], (clouds,) + x.shape)


def point_affine(x, wp, t, clouds, n, per_cloud):
    """y[b*n + p] = wp . x[row] + t[b]; row = b*n + p (per_cloud) or p (one grid shared by all clouds)."""
    y = np.einsum("bpd,cd->bpc", _point_rows(x, clouds, n, per_cloud), _f64(wp)) + _f64(t)[:, None, :]
    return y.reshape(clouds * n, -1)


def point_affine_bwd(dy, x, wp, clouds, n, per_cloud):
    """(dx [clouds*n, d] -- the per-row gradient, also for a shared grid, where the caller does not ask for it --, dwp, dt)."""
    dy = _f64(dy).reshape(clouds, n, -1)
    dx = np.einsum("bpc,cd->bpd", dy, _f64(wp)).reshape(clouds * n, -1)
    dwp = np.einsum("bpc,bpd->cd", dy, _point_rows(x, clouds, n, per_cloud))
    return dx, dwp, dy.sum(1)


# ------------------------------------------------------------------------------------------------ inputs
def lattice_cloud(clouds, n, seed):
    """float32 [clouds*n, 3], coordinates k/16 with |k| <= 32, three planted duplicate points per cloud.  Products lie on
    a 1/256 grid and every score is below 36, so 2<x_i,x_j> - |x_j|^2 is exact in fp32 in any evaluation order, fused or not:
    the complete ordered neighbour list has one right answer, and equal scores (duplicates, equidistant lattice points)
    exercise the tie rule."""
    rng = np.random.RandomState(seed)
    p = rng.randint(-32, 33, (clouds, n, 3)).astype(np.float32) / 16.0
    for b in range(clouds):
        for _ in range(3):
            src, dst = rng.choice(n, 2, replace=False)
            p[b, dst] = p[b, src]
    return p.reshape(clouds * n, 3)


def lattice_features(rows, d, seed):
    """float32 [rows, d], values k/8 with |k| <= 16: representable in bf16, Gram entries on a 1/64 grid and at most 4 d, so
    a Gram matrix and the squared norms are exact in fp32 under any summation order and in bf16-split arithmetic."""
    return np.random.RandomState(seed).randint(-16, 17, (rows, d)).astype(np.float32) / 8.0


def lattice_grad(shape, seed):
    """float32, values k/64 with |k| <= 64: sums of up to 2048 of them are exact in fp32 in any order."""
    return np.random.RandomState(seed).randint(-64, 65, shape).astype(np.float32) / 64.0


def relu_edge_margin(x, gamma, beta, eps):
    """min |pre-activation| of BatchNorm(x): how far every element is from the ReLU's kink."""
    return float(np.abs(batchnorm_fwd(x, gamma, beta, eps, False)["pre"]).min())


def off_relu_edge(x, gamma, beta, eps, margin):
    """float32 copy of x in which no BatchNorm pre-activation lies within `margin` of 0: elements that do are pushed away
    from the kink by 2 * margin (the statistics barely move: only a few elements do).  The ReLU mask of the backward is then
    the same in fp32 and fp64, so the gradient has one right answer up to rounding."""
    x = np.array(x, np.float32)
    g = _f64(gamma)
    for _ in range(8):
        f = batchnorm_fwd(x, gamma, beta, eps, False)
        near = np.abs(f["pre"]) < margin
        if not near.any():
            return x
        step = np.where(f["pre"] >= 0.0, 1.0, -1.0) * 2.0 * margin / (f["rstd"] * g)
        x = np.where(near, x + step, x).astype(np.float32)
    raise ValueError("off_relu_edge did not converge")
