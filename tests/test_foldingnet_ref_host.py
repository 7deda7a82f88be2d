"""The float64 oracle of the FoldingNet kernels (oracle/foldingnet_ref.py) against torch in float64, and the properties of its
input builders that tests/test_gpu_foldingnet_kernels.py relies on.  No GPU.

Agreement with torch is held to 1e-12 relative (both sides are float64; they differ in summation order only).  The
builder properties are exact statements: lattice scores, Gram matrices and gradient sums have no rounding in fp32, so the
GPU tests may compare neighbour lists, arg-max winners and scatter sums bit for bit."""
import numpy as np
import pytest
import torch

from oracle import foldingnet_ref as F
from oracle import weights as W

TOL = 1e-12
SYNTH = [(4, 256, 5), (3, 100, 7), (2, 333, 8), (1, 2048, 6)]          # the shape-like clouds of the GPU test: (clouds, n, seed)
LATTICE_N = [(1, 16), (3, 17), (2, 63), (2, 65), (1, 200)]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


# ------------------------------------------------------------------------------------------------ oracle vs torch float64
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows,ch", [(2, 1), (37, 5), (513, 12)])
def test_batchnorm_matches_torch_float64(rows, ch, relu):
    rng = np.random.RandomState(rows + ch)
    # two rows: xhat = +-1 / sqrt(1 + eps / var) and dx ~ eps / var; a spread of the size of sqrt(eps) keeps dx well conditioned
    x = rng.randn(rows, ch) * (0.002 if rows == 2 else 1.7) + 0.3
    gamma, beta = rng.uniform(0.5, 1.5, ch) * rng.choice([-1.0, 1.0], ch), rng.uniform(-0.5, 0.5, ch)
    rm, rv, dy = rng.randn(ch), rng.uniform(0.5, 2.0, ch), rng.randn(rows, ch)
    bn = torch.nn.BatchNorm1d(ch, eps=1e-5, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(t64(gamma)); bn.bias.copy_(t64(beta)); bn.running_mean.copy_(t64(rm)); bn.running_var.copy_(t64(rv))
    xt = t64(x, True)
    y = bn(xt)
    if relu:
        y = torch.relu(y)
    y.backward(t64(dy))
    f = F.batchnorm_fwd(x, gamma, beta, 1e-5, relu, rm, rv, 0.1)
    assert rel(f["y"], y.detach()) < TOL
    assert rel(f["running_mean"], bn.running_mean) < TOL and rel(f["running_var"], bn.running_var) < TOL
    assert rel(f["mean"], x.mean(0)) < TOL and rel(f["var"], x.var(0)) < TOL
    dx, dg, db = F.batchnorm_bwd(dy, x, gamma, beta, 1e-5, relu)
    assert rel(dx, xt.grad) < TOL
    assert rel(dg, bn.weight.grad) < TOL and rel(db, bn.bias.grad) < TOL
    bn.eval()
    with torch.no_grad():
        ye = bn(t64(x))
        ye = torch.relu(ye) if relu else ye
    assert rel(F.batchnorm_eval(x, gamma, beta, f["running_mean"], f["running_var"], 1e-5, relu), ye) < TOL


def test_knn16_matches_topk_on_a_tie_free_cloud():
    clouds, n = 3, 100
    x = W.synth_point_clouds(clouds, n, seed=7).reshape(clouds * n, 3).numpy()
    idx, gap, adj = F.knn16(x, clouds, n)
    assert adj.min() > 0.0 and (gap >= adj).all()
    xt = t64(x).view(clouds, n, 3)
    pd = 2.0 * xt @ xt.transpose(1, 2) - (xt ** 2).sum(-1)[:, None, :]
    assert (pd.topk(16, dim=-1)[1].view(clouds * n, 16).numpy() == idx).all()
    assert rel(F.rowsq(x), (t64(x) ** 2).sum(-1)) < TOL
    # the covariance features as the reference states them: neighbours minus their mean, then X^T X
    nb = xt.reshape(clouds * n, 3)[(torch.as_tensor(idx, dtype=torch.int64) + (torch.arange(clouds * n) // n * n)[:, None])]
    c = nb - nb.mean(1, keepdim=True)
    want = torch.cat([t64(x), (c.transpose(1, 2) @ c).reshape(clouds * n, 9)], 1)
    assert rel(F.knn_cov(x, idx, clouds, n), want) < TOL


def test_knn16_ties_go_to_the_lowest_index():
    x = np.zeros((17, 3))
    x[:, 0] = [0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7, -7, 8, -8]
    idx, gap, adj = F.knn16(x, 1, 17)
    assert idx[0].tolist() == list(range(16)) and gap[0] == 0.0 and adj[0] == 0.0       # +-k are equidistant from 0: lower index first
    assert idx[15].tolist()[:3] == [15, 13, 11] and gap[15] > 0.0


@pytest.mark.parametrize("ch", [1, 65])
def test_pooling_matches_torch_autograd(ch):
    clouds, n = 3, 17
    rng = np.random.RandomState(ch)
    x = rng.randn(clouds * n, ch)                                                        # no equal values: torch's tie rule is not relied on
    idx = rng.randint(0, n, (clouds * n, 16)).astype(np.int32)
    idx[:, 5] = idx[:, 2]                                                                # a repeated neighbour: the first listing must win
    dy = rng.randn(clouds * n, ch)
    xt = t64(x, True)
    rows = torch.as_tensor(idx, dtype=torch.int64) + (torch.arange(clouds * n) // n * n)[:, None]
    xt[rows].amax(1).backward(t64(dy))
    val, k = F.gather_max(x, idx, clouds, n)
    assert rel(val, x[rows.numpy()].max(1)) == 0.0
    assert (k != 5).all()
    assert rel(F.gather_max_bwd(dy, idx, k, clouds, n), xt.grad) < TOL
    # global pooling
    xt = t64(x, True)
    dyc = rng.randn(clouds, ch)
    v, p = xt.view(clouds, n, ch).max(1)
    v.backward(t64(dyc))
    val, arg = F.rowmax(x, clouds, n)
    assert rel(val, v.detach()) == 0.0 and (arg == p.numpy()).all()
    assert rel(F.rowmax_bwd(dyc, arg, clouds, n), xt.grad) == 0.0


def test_pooling_tie_rules():
    x = np.array([[1.0], [3.0], [3.0], [2.0]] + [[0.0]] * 13)
    idx = np.array([[3, 2, 1, 1] + [0] * 12] * 17, np.int32)
    val, k = F.gather_max(x, idx, 1, 17)
    assert (val == 3.0).all() and (k == 1).all()                                         # list position 1 (row 2) precedes position 2 (row 1)
    dx = F.gather_max_bwd(np.ones((17, 1)), idx, k, 1, 17)
    assert dx[2, 0] == 17.0 and dx.sum() == 17.0
    val, arg = F.rowmax(x, 1, 17)
    assert val[0, 0] == 3.0 and arg[0, 0] == 1                                           # lowest point index
    assert F.gather_max_ties(x, idx, 1, 17) == 17


@pytest.mark.parametrize("per_cloud", [False, True])
@pytest.mark.parametrize("d,ch", [(1, 1), (2, 65), (3, 12), (4, 7)])
def test_point_affine_matches_the_concatenated_convolution(d, ch, per_cloud):
    """The reference's first fold convolution: cat([points | codeword]) @ W.T + bias, codeword repeated over the points."""
    clouds, n, cw = 3, 7, 6
    rng = np.random.RandomState(10 * d + ch)
    x = rng.randn(clouds * n if per_cloud else n, d)
    w, bias, code, dy = rng.randn(ch, d + cw), rng.randn(ch), rng.randn(clouds, cw), rng.randn(clouds * n, ch)
    xt, wt, ct = t64(x, True), t64(w, True), t64(code, True)
    pts = xt.view(clouds, n, d) if per_cloud else xt[None].expand(clouds, n, d)
    y = torch.cat([pts, ct[:, None, :].expand(clouds, n, cw)], -1).reshape(clouds * n, d + cw) @ wt.t() + t64(bias)
    y.backward(t64(dy))
    t = code @ w[:, d:].T + bias
    assert rel(F.point_affine(x, w[:, :d], t, clouds, n, per_cloud), y.detach()) < TOL
    dx, dwp, dt = F.point_affine_bwd(dy, x, w[:, :d], clouds, n, per_cloud)
    assert rel(dwp, wt.grad[:, :d]) < TOL
    assert rel(dt @ w[:, d:], ct.grad) < TOL and rel(dt.T @ code, wt.grad[:, d:]) < TOL  # dt is the gradient of t = Wc . code + bias
    assert rel(dx if per_cloud else dx.reshape(clouds, n, d).sum(0), xt.grad) < TOL


# ------------------------------------------------------------------------------------------------ input properties
def _score_fp32(x, clouds, n):
    """The xyz kernel's expression in float32: 2 * (qx*jx + qy*jy + qz*jz) - (jx*jx + jy*jy + jz*jz)."""
    x = np.asarray(x, np.float32).reshape(clouds, n, 3)
    q, j = x[:, :, None, :], x[:, None, :, :]
    dot = (q[..., 0] * j[..., 0] + q[..., 1] * j[..., 1]) + q[..., 2] * j[..., 2]
    sq = (j[..., 0] * j[..., 0] + j[..., 1] * j[..., 1]) + j[..., 2] * j[..., 2]
    s = np.float32(2.0) * dot - sq
    assert s.dtype == np.float32
    return s


@pytest.mark.parametrize("clouds,n", LATTICE_N)
def test_lattice_cloud_scores_are_exact_in_float32_and_tie_at_the_boundary(clouds, n):
    x = F.lattice_cloud(clouds, n, seed=n)
    assert x.dtype == np.float32 and np.abs(x).max() <= 2.0 and (x * 16 == np.round(x * 16)).all()
    s64 = F.knn_scores(x, clouds, n)
    assert (_score_fp32(x, clouds, n).astype(np.float64) == s64).all()
    assert np.abs(s64).max() < 36.0 and (s64 * 256 == np.round(s64 * 256)).all()         # 36 * 256 < 2^24: any order, fused or not
    idx, gap, adj = F.knn16(x, clouds, n)
    dup = sum(len(np.unique(x[b * n:(b + 1) * n], axis=0)) < n for b in range(clouds))
    assert dup == clouds                                                                  # every cloud holds duplicate points
    assert (adj == 0.0).any()                                                             # the order rests on the tie rule somewhere
    if n > 16:
        assert (gap == 0.0).any(), "no tie at the 16th/17th boundary"                     # and so does the neighbour set
    print("lattice cloud %dx%d: boundary ties %.1f%%, order ties %.1f%%" % (clouds, n, 100 * (gap == 0).mean(), 100 * (adj == 0).mean()))


@pytest.mark.parametrize("clouds,n,d", [(3, 80, 32), (2, 16, 64), (1, 200, 64)])
def test_lattice_features_are_exact_in_float32_and_bfloat16(clouds, n, d):
    x = F.lattice_features(clouds * n, d, seed=d + n)
    assert (torch.from_numpy(x).bfloat16().float().numpy() == x).all()
    x3 = x.reshape(clouds, n, d)
    gram64 = np.einsum("bid,bjd->bij", x3.astype(np.float64), x3.astype(np.float64))
    assert np.abs(gram64).max() <= 4.0 * d and (gram64 * 64 == np.round(gram64 * 64)).all()      # 4 d * 64 <= 2^14: every partial sum is exact
    for order in (np.arange(d), np.arange(d)[::-1], np.random.RandomState(0).permutation(d)):
        acc = np.zeros((clouds, n, n), np.float32)
        for k in order:
            acc = acc + x3[:, :, None, k] * x3[:, None, :, k]
        assert acc.dtype == np.float32 and (acc.astype(np.float64) == gram64).all()
    sq = (x * x).sum(-1, dtype=np.float32)
    assert (sq.astype(np.float64) == F.rowsq(x)).all()
    s64 = F.knn_scores(x, clouds, n)
    assert ((np.float32(2.0) * gram64.astype(np.float32) - sq.reshape(clouds, 1, n)).astype(np.float64) == s64).all()
    idx, gap, adj = F.knn16(x, clouds, n)
    assert (idx[:, 0] == np.tile(np.arange(n), clouds)).all()                             # no duplicate rows: a row is its own best match


def test_lattice_grad_sums_are_exact_in_float32():
    g = F.lattice_grad((2048, 3), seed=1)
    assert np.abs(g).max() <= 1.0 and (g * 64 == np.round(g * 64)).all()
    want = g.astype(np.float64).sum(0)
    for order in (np.arange(2048), np.arange(2048)[::-1], np.random.RandomState(0).permutation(2048)):
        acc = np.zeros(3, np.float32)
        for r in order:
            acc = acc + g[r]
        assert (acc.astype(np.float64) == want).all()
    assert (np.abs(g).cumsum(0)[-1] * 64 < 2 ** 24).all()                                 # every partial sum fits the fp32 mantissa


@pytest.mark.parametrize("clouds,n,seed", SYNTH)
def test_shape_like_clouds_are_ambiguous_for_at_most_one_percent_of_the_queries(clouds, n, seed):
    """A query is ambiguous when its 16th and 17th score are closer than 1e-6 of the cloud's largest |score|: the GPU test
    compares the neighbour sets of all the others.  The fp32 score expression is about 1.3e-7 of that scale away from
    float64 (printed below), and no unambiguous query changes its neighbour set under it."""
    x = W.synth_point_clouds(clouds, n, seed=seed).reshape(clouds * n, 3).numpy()
    idx, gap, adj = F.knn16(x, clouds, n)
    s64 = F.knn_scores(x, clouds, n)
    scale = np.abs(s64).max(axis=(1, 2))
    amb = gap < 1e-6 * np.repeat(scale, n)
    s32 = _score_fp32(x, clouds, n)
    err = (np.abs(s32 - s64).max(axis=(1, 2)) / scale).max()
    idx32 = np.argsort(-s32, axis=-1, kind="stable")[..., :16].reshape(clouds * n, 16)
    same = (np.sort(idx32, -1) == np.sort(idx, -1)).all(-1)
    print("synth cloud %dx%d seed %d: ambiguous %.2f%%, fp32 score error %.3g of the scale" % (clouds, n, seed, 100 * amb.mean(), err))
    assert amb.mean() <= 0.01
    assert err < 1e-6
    assert same[~amb].all()


def test_off_relu_edge_moves_few_elements_and_clears_the_margin():
    rng = np.random.RandomState(3)
    x = (rng.randn(4099, 12) * 2.0 + 0.5).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, 12) * rng.choice([-1.0, 1.0], 12), rng.uniform(-0.5, 0.5, 12)
    assert F.relu_edge_margin(x, gamma, beta, 1e-5) < 1e-3
    y = F.off_relu_edge(x, gamma, beta, 1e-5, 1e-3)
    assert y.dtype == np.float32 and F.relu_edge_margin(y, gamma, beta, 1e-5) >= 1e-3
    assert (y != x).mean() < 0.01
