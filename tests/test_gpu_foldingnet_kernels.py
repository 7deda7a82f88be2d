"""Every kernel of csrc/foldingnet.hip against the float64 statements of oracle/foldingnet_ref.py, one entry point at a time, at
the smallest shapes at which each can still go wrong (tests/test_gpu_foldingnet.py sees them only through the whole auto-encoder).

Discrete outcomes are compared EXACTLY.  The inputs make that possible: lattice clouds and features whose fp32 scores carry no
rounding (neighbour lists, ordered, ties included), coarse-valued features whose equal maxima are real ties (arg-max winners), and
lattice gradients whose sums are exact in any order (the atomic scatter).  tests/test_foldingnet_ref_host.py asserts those
properties and pins the oracle against torch in float64.

Everything else (knn_cov, BatchNorm, point_affine) is held, per output tensor, to
    err = max|got - ref64| / max|ref64|  <=  max(4 * err_torch32, 64 * 2^-24)
where err_torch32 is the same distance for a plain torch float32 evaluation ON THE CPU of the same operation on the same inputs.
The factor 4: kernel and torch sum in different orders and both errors are a few ulp times the square root of a run length.  The
floor: the column reductions sum runs of 128 rows per lane in fp32 before they combine in double, which lands at 4e-7 .. 1e-6
where torch's pairwise sums give 1.5e-7; 64 * 2^-24 (3.8e-6) leaves that 4x headroom and is 150x below what a first-row pivot of
the BatchNorm variance loses on the outlier input below (6e-4).  Every measured err goes to $DSC_PARITY_LOG when it is set.

Inputs with a row stride are column slices of a wider tensor, as in the product; every launch gets valid arguments only."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from oracle import foldingnet_ref as F
from oracle import weights as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR = 64 * 2.0 ** -24
EPS = 1e-5
SYNTH = [(4, 256, 5), (3, 100, 7), (2, 333, 8), (1, 2048, 6)]


def net():
    from diffuscene_amd.networks import foldingnet_autoencoder as A
    return A


def lib():
    from diffuscene_amd import _lib, ops
    return _lib, ops


def sliced(a, left=2, right=2, fill=7.5, grad=False):
    """a [rows, w] (numpy) -> (wide device tensor [rows, left + w + right], its column slice holding a)."""
    a = np.array(a, np.float32)
    big = torch.full((a.shape[0], left + a.shape[1] + right), fill, dtype=torch.float32)
    big[:, left:left + a.shape[1]] = torch.from_numpy(a)
    big = big.to(DEV).requires_grad_(grad)
    return big, big[:, left:left + a.shape[1]]


def dev(a, dtype=torch.float32, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype).to(DEV).requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy()


def exact(got, want):
    """bit-equal to the float64 oracle rounded to fp32 (the oracle's value is an fp32 number wherever this is used)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.dtype == np.float32:
        assert (want.astype(np.float32).astype(np.float64) == want).all()
    return bool((got == want).all())


def _log(line):
    print(line)
    if os.environ.get("DSC_PARITY_LOG"):
        with open(os.environ["DSC_PARITY_LOG"], "a") as f:
            f.write(line + "\n")


def bounded(what, got, ref64, t32):
    """-> (ok, line) for one output tensor under the bound of the module docstring."""
    got, ref64, t32 = (np.asarray(host(a) if torch.is_tensor(a) else a, np.float64) for a in (got, ref64, t32))
    assert got.shape == ref64.shape == t32.shape, (what, got.shape, ref64.shape, t32.shape)
    scale = np.abs(ref64).max()
    assert scale > 0.0 and np.isfinite(got).all(), what
    err, e32 = np.abs(got - ref64).max() / scale, np.abs(t32 - ref64).max() / scale
    bound = max(4.0 * e32, FLOOR)
    line = "foldingnet %s: err %.3g (bound %.3g, err_torch32 %.3g)" % (what, err, bound, e32)
    _log(line)
    return err <= bound, line


def check_all(results):
    bad = [line for ok, line in results if not ok]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def lattice_knn(clouds, n):
    x = F.lattice_cloud(clouds, n, seed=n)
    idx, gap, adj = F.knn16(x, clouds, n)
    for a in (x, idx):
        a.setflags(write=False)
    return x, idx


@functools.lru_cache(maxsize=None)
def synth_knn(clouds, n, seed):
    x = W.synth_point_clouds(clouds, n, seed=seed).reshape(clouds * n, 3).numpy()
    idx, gap, adj = F.knn16(x, clouds, n)
    scale = np.abs(F.knn_scores(x, clouds, n)).max(axis=(1, 2))
    amb = gap < 1e-6 * np.repeat(scale, n)
    for a in (x, idx, amb):
        a.setflags(write=False)
    return x, idx, amb


# ------------------------------------------------------------------------------------------------ knn16, xyz path
@pytest.mark.parametrize("clouds,n", [(1, 16), (3, 17), (2, 63), (2, 65), (1, 200), (1, 2048)])
def test_knn16_xyz_ordered_lists_equal_the_oracle_on_lattice_clouds(clouds, n):
    """All points chosen (16), a row count that is no multiple of 4 (3 x 17), both sides of one candidate per lane (63, 65), all
    32 candidate slots (2048).  Equal scores are frequent here, so the full ordered list pins the tie rule of both arg-max levels."""
    x, want = lattice_knn(clouds, n)
    big, xs = sliced(x, left=2, right=2)
    assert xs.stride(0) == 7
    got = host(net().knn16(xs, clouds, n))
    assert got.dtype == np.int32 and got.min() >= 0 and got.max() < n
    wrong = (got != want).any(-1)
    assert not wrong.any(), "%d of %d ordered lists differ, first: query %d got %s want %s" % (
        wrong.sum(), len(wrong), wrong.argmax(), got[wrong.argmax()], want[wrong.argmax()])


@pytest.mark.parametrize("clouds,n,seed", SYNTH)
def test_knn16_xyz_neighbour_sets_on_shape_like_clouds(clouds, n, seed):
    """Continuous coordinates: fp32 scores round, so only the neighbour SETS are compared, for every query whose 16th and 17th
    float64 score are at least 1e-6 of the cloud's score scale apart (at most 1 % are not: tests/test_foldingnet_ref_host.py)."""
    x, want, amb = synth_knn(clouds, n, seed)
    big, xs = sliced(x, left=2, right=2)
    got = host(net().knn16(xs, clouds, n))
    assert (got[:, 0] == np.tile(np.arange(n), clouds)).all()                           # a point is its own nearest neighbour
    assert amb.mean() <= 0.01
    same = (np.sort(got, -1) == np.sort(want, -1)).all(-1)
    assert same[~amb].all(), "%d unambiguous queries differ" % (~same[~amb]).sum()


def test_knn16_rejects_unsupported_sizes_on_the_host():
    A = net()
    for n in (15, 2049):
        with pytest.raises(RuntimeError, match="dsc_knn16_f32"):
            A.knn16(torch.zeros((n, 3), device=DEV), 1, n)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        A.knn16(torch.zeros((64, 48), device=DEV), 1, 64)


# ------------------------------------------------------------------------------------------------ knn16, Gram path
@pytest.mark.parametrize("gemm_arith", ["split", "f32"], indirect=True)
@pytest.mark.parametrize("clouds,n,d", [(3, 80, 32), (2, 16, 64), (1, 200, 64)])
def test_knn16_gram_path_and_rowsq_equal_the_oracle_on_lattice_features(clouds, n, d, gemm_arith):
    _lib, ops = lib()
    x = F.lattice_features(clouds * n, d, seed=d + n)
    want, gap, adj = F.knn16(x, clouds, n)
    big, xs = sliced(x, left=3, right=2)
    sq = torch.empty((clouds * n,), device=DEV, dtype=torch.float32)
    _lib.check(_lib.fn("dsc_rowsq_f32")(xs.data_ptr(), xs.stride(0), d, clouds * n, sq.data_ptr(), ops.stream_ptr()), "dsc_rowsq_f32")
    assert exact(host(sq), F.rowsq(x))
    got = host(net().knn16(dev(x), clouds, n))
    wrong = (got != want).any(-1)
    assert not wrong.any(), "%s: %d of %d ordered lists differ, first: query %d got %s want %s" % (
        gemm_arith, wrong.sum(), len(wrong), wrong.argmax(), got[wrong.argmax()], want[wrong.argmax()])


# ------------------------------------------------------------------------------------------------ knn_cov
def _knn_cov_torch32(x, idx, clouds, n):
    xt = torch.tensor(np.asarray(x, np.float32))
    rows = torch.from_numpy(np.asarray(idx, np.int64)) + (torch.arange(clouds * n) // n * n)[:, None]
    nb = xt[rows]
    c = nb - nb.mean(1, keepdim=True)
    return torch.cat([xt, (c.transpose(1, 2) @ c).reshape(clouds * n, 9)], 1).numpy()


@pytest.mark.parametrize("kind,clouds,n", [("lattice", 3, 17), ("lattice", 2, 100), ("synth", 3, 17), ("synth", 3, 100)])
def test_knn_cov(kind, clouds, n):
    _lib, ops = lib()
    if kind == "lattice":
        x, idx = lattice_knn(clouds, n)
    else:
        x, idx, _ = synth_knn(clouds, n, 7)
    ref, t32 = F.knn_cov(x, idx, clouds, n), _knn_cov_torch32(x, idx, clouds, n)
    big, xs = sliced(x)
    di = dev(idx, torch.int32)
    res = []
    got = host(net().knn_cov(xs, di, clouds, n))
    assert exact(got[:, :3], x)                                                          # the xyz columns are a copy
    res.append(bounded("knn_cov %s %dx%d" % (kind, clouds, n), got, ref, t32))
    # output rows wider than the 12 features: the columns behind them stay untouched
    sentinel = np.float32(-1234.5)
    out = torch.full((clouds * n, 16), float(sentinel), device=DEV, dtype=torch.float32)
    _lib.check(_lib.fn("dsc_knn_cov_f32")(xs.data_ptr(), xs.stride(0), di.data_ptr(), clouds, n, out.data_ptr(), 16,
                                          ops.stream_ptr()), "dsc_knn_cov_f32")
    out = host(out)
    assert (out[:, 12:].view(np.uint32) == sentinel.view(np.uint32)).all()
    res.append(bounded("knn_cov %s %dx%d ldo=16" % (kind, clouds, n), out[:, :12], ref, t32))
    check_all(res)


# ------------------------------------------------------------------------------------------------ gather_max
def _pool_features(rows, ch, n, seed):
    """values k/4 with |k| <= 8: equal maxima among 16 neighbours are the rule; plus duplicated rows inside every cloud"""
    rng = np.random.RandomState(seed)
    x = rng.randint(-8, 9, (rows, ch)).astype(np.float32) / 4.0
    for b in range(rows // n):
        for _ in range(3):
            src, dst = rng.choice(n, 2, replace=False)
            x[b * n + dst] = x[b * n + src]
    return x


def _neighbour_lists(kind, clouds, n):
    if kind == "knn":
        return lattice_knn(clouds, n)[1]
    rng = np.random.RandomState(n)
    idx = rng.randint(0, n, (clouds * n, 16)).astype(np.int32)                           # any valid list, in any order
    idx[:, 9] = idx[:, 4]                                                                # a neighbour listed twice
    idx[::3, 1] = idx[::3, 0]
    return idx


@pytest.mark.parametrize("kind", ["knn", "arbitrary"])
@pytest.mark.parametrize("clouds,n", [(3, 17), (1, 257)])
@pytest.mark.parametrize("ch", [1, 12, 64, 65, 200])
def test_gather_max_forward_and_backward_equal_the_oracle(ch, clouds, n, kind):
    """The forward is a selection, the backward a scatter of lattice gradients whose sums are exact in any order: both bit-equal.
    The scatter lands on the right rows only if the stored arg is the FIRST maximum of the list and no atomic addition is lost."""
    A = net()
    rows = clouds * n
    idx = _neighbour_lists(kind, clouds, n)
    x = _pool_features(rows, ch, n, seed=ch + n)
    assert F.gather_max_ties(x, idx, clouds, n) > 0
    val, k = F.gather_max(x, idx, clouds, n)
    dy = F.lattice_grad((rows, ch), seed=ch)
    big, xs = sliced(x, left=3, right=2, grad=True)
    out = A.GatherMaxFn.apply(xs, dev(idx, torch.int32), clouds, n)
    assert exact(host(out), val)
    out.backward(dev(dy))
    g = host(big.grad)
    assert exact(g[:, 3:3 + ch], F.gather_max_bwd(dy, idx, k, clouds, n))
    assert (g[:, :3] == 0).all() and (g[:, 3 + ch:] == 0).all()


def test_gather_max_keeps_its_row_strides():
    """ldo, ldy and lddx wider than the channel count (the Python op always passes the channel count)."""
    _lib, ops = lib()
    clouds, n, ch = 3, 17, 65
    rows = clouds * n
    idx = lattice_knn(clouds, n)[1]
    x = _pool_features(rows, ch, n, seed=5)
    val, k = F.gather_max(x, idx, clouds, n)
    dy = F.lattice_grad((rows, ch), seed=6)
    sentinel = np.float32(-1234.5)
    big, xs = sliced(x)
    di = dev(idx, torch.int32)
    out = torch.full((rows, ch + 3), float(sentinel), device=DEV, dtype=torch.float32)
    arg = torch.zeros((rows, ch), device=DEV, dtype=torch.uint8)
    _lib.check(_lib.fn("dsc_gather_max_f32")(xs.data_ptr(), xs.stride(0), di.data_ptr(), clouds, n, ch, out.data_ptr(), ch + 3,
                                             arg.data_ptr(), ops.stream_ptr()), "dsc_gather_max_f32")
    o = host(out)
    assert exact(o[:, :ch], val) and (o[:, ch:] == sentinel).all()
    assert (host(arg) == k).all()
    bigdy, dys = sliced(dy, left=1, right=1)
    dx = torch.zeros((rows, ch + 4), device=DEV, dtype=torch.float32)
    _lib.check(_lib.fn("dsc_gather_max_bwd_f32")(dys.data_ptr(), dys.stride(0), di.data_ptr(), arg.data_ptr(), clouds, n, ch,
                                                 dx.data_ptr(), ch + 4, ops.stream_ptr()), "dsc_gather_max_bwd_f32")
    d = host(dx)
    assert exact(d[:, :ch], F.gather_max_bwd(dy, idx, k, clouds, n)) and (d[:, ch:] == 0).all()


# ------------------------------------------------------------------------------------------------ rowmax
@pytest.mark.parametrize("ch", [1, 64, 65])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_rowmax_forward_and_backward_equal_the_oracle(n, ch):
    """Equal maxima sit at point indices of different row lanes (p mod 4), the later lane holding the LOWER index in half of the
    columns: value, arg (through the routed gradient) and gradient are bit-equal."""
    A = net()
    clouds = 3
    rng = np.random.RandomState(10 * n + ch)
    x = rng.randint(-8, 9, (clouds * n, ch)).astype(np.float32) / 4.0
    planted = 0
    if n >= 3:
        for b in range(clouds):
            for c in range(ch):
                p, q = rng.choice(n, 2, replace=False)
                if p % 4 != q % 4:
                    x[b * n + p, c] = x[b * n + q, c] = 2.5
                    planted += 1
        assert planted > 0
    val, arg = F.rowmax(x, clouds, n)
    dy = F.lattice_grad((clouds, ch), seed=n)
    big, xs = sliced(x, left=1, right=3, grad=True)
    out = A.RowMaxFn.apply(xs, clouds, n)
    assert exact(host(out), val)
    out.backward(dev(dy))
    g = host(big.grad)
    assert exact(g[:, 1:1 + ch], F.rowmax_bwd(dy, arg, clouds, n))
    assert (g[:, :1] == 0).all() and (g[:, 1 + ch:] == 0).all()


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_params(ch, seed):
    rng = np.random.RandomState(seed)
    gamma = (rng.uniform(0.5, 1.5, ch) * rng.choice([-1.0, 1.0], ch)).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, ch).astype(np.float32)
    rm, rv = rng.randn(ch).astype(np.float32), rng.uniform(0.5, 2.0, ch).astype(np.float32)
    return gamma, beta, rm, rv


def _bn_torch32(x, gamma, beta, rm, rv, dy, relu):
    xt, g, b = (torch.tensor(a, dtype=torch.float32, requires_grad=True) for a in (x, gamma, beta))
    rmt, rvt = torch.tensor(rm), torch.tensor(rv)
    y = torch.nn.functional.batch_norm(xt, rmt, rvt, g, b, True, 0.1, EPS)
    y = torch.relu(y) if relu else y
    y.backward(torch.tensor(dy))
    with torch.no_grad():
        ye = torch.nn.functional.batch_norm(xt, torch.tensor(rm), torch.tensor(rv), g, b, False, 0.1, EPS)
        ye = torch.relu(ye) if relu else ye
    return dict(y=y.detach().numpy(), running_mean=rmt.numpy(), running_var=rvt.numpy(), dx=xt.grad.numpy(), dgamma=g.grad.numpy(),
                dbeta=b.grad.numpy(), eval=ye.numpy())


def _bn_case(tag, x, relu, seed):
    A = net()
    rows, ch = x.shape
    gamma, beta, rm, rv = _bn_params(ch, seed)
    if relu:
        x = F.off_relu_edge(x, gamma, beta, EPS, 1e-3)
    x = np.asarray(x, np.float32)
    dy = np.random.RandomState(seed + 1).randn(rows, ch).astype(np.float32)
    f = F.batchnorm_fwd(x, gamma, beta, EPS, relu, rm, rv, 0.1)
    dx, dg, db = F.batchnorm_bwd(dy, x, gamma, beta, EPS, relu)
    ref = dict(y=f["y"], running_mean=f["running_mean"], running_var=f["running_var"], dx=dx, dgamma=dg, dbeta=db,
               eval=F.batchnorm_eval(x, gamma, beta, rm, rv, EPS, relu))
    t32 = _bn_torch32(x, gamma, beta, rm, rv, dy, relu)
    big, xs = sliced(x, left=2, right=3, grad=True)
    gt, bt = dev(gamma, grad=True), dev(beta, grad=True)
    rmt, rvt = dev(rm), dev(rv)
    y = A.BatchNormFn.apply(xs, gt, bt, rmt, rvt, EPS, 0.1, relu)
    y.backward(dev(dy))
    frozen = types.SimpleNamespace(weight=gt.detach(), bias=bt.detach(), running_mean=dev(rm), running_var=dev(rv), eps=EPS)
    got = dict(y=y, running_mean=rmt, running_var=rvt, dx=big.grad[:, 2:2 + ch], dgamma=gt.grad, dbeta=bt.grad,
               eval=A.batchnorm_eval(xs.detach(), frozen, relu))
    g = host(big.grad)
    assert (g[:, :2] == 0).all() and (g[:, 2 + ch:] == 0).all()
    res = [bounded("batchnorm %s %dx%d relu=%d %s" % (tag, rows, ch, relu, k), got[k], ref[k], t32[k]) for k in ref]
    if relu:
        # the ReLU mask of the backward has one right answer: every pre-activation is farther from 0 than y may be off
        e32 = np.abs(t32["y"] - ref["y"]).max()
        assert F.relu_edge_margin(x, gamma, beta, EPS) > max(4 * e32, FLOOR * np.abs(ref["y"]).max())
    check_all(res)


def _bn_input(rows, ch, seed):
    if rows == 2:
        # xhat = +-1 / sqrt(1 + eps / var) and dx ~ eps / var: a spread of the size of sqrt(eps), exactly centred in fp32, keeps dx
        # well conditioned (with a spread of 1 the true dx is 1e-5 of its own terms and no fp32 evaluation resolves it)
        return np.array([[0.25], [0.25 + 2.0 ** -8]], np.float32)
    return (np.random.RandomState(seed).randn(rows, ch) * 1.7 + 0.3).astype(np.float32)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows,ch", [(2, 1), (511, 12), (513, 65), (1100, 12)])
def test_batchnorm_forward_backward_eval(rows, ch, relu):
    """One split and a row tail (511), two splits and a channel tail (513 x 65), three splits (1100), the smallest batch (2)."""
    _bn_case("normal", _bn_input(rows, ch, rows), relu, seed=rows + ch)


def _bn_special(kind):
    rng = np.random.RandomState(40)
    if kind == "offset":                 # a common offset 1e4 standard deviations wide
        return 100.0 + 0.01 * rng.randn(4096, 12)
    if kind == "outlier_first_row":      # the first row is 1e5 standard deviations of the rest away from them
        x = 1000.0 + 0.01 * rng.randn(4096, 12)
        x[0] = 0.0
        return x
    if kind.startswith("first_row_"):    # the first row 3.5 / 5 standard deviations out: either side of the kernel's threshold (4) for
        x = 0.3 + 1.7 * rng.randn(4096, 12)                                             # summing a column a second time
        x[0] = x[1:].mean(0) + float(kind[10:-6]) * x[1:].std(0) * np.where(np.arange(12) % 2, 1.0, -1.0)
        return x
    x = np.where(rng.rand(4096, 12) < 0.01, np.abs(rng.randn(4096, 12)), 0.0)          # ReLU-like: 1 % active, first row active
    x[0] = np.abs(rng.randn(12)) + 0.1
    return x


@pytest.mark.parametrize("kind", ["offset", "outlier_first_row", "sparse", "first_row_3.5_sigma", "first_row_5_sigma"])
def test_batchnorm_statistics_on_hard_inputs(kind):
    """Inputs on which a variance summed about an unlucky pivot cancels.  Without ReLU: on the offset input even the fp32 mean is 1e-3 of a standard
    deviation off, so a ReLU mask would not be well defined; the statistics are what these inputs are about."""
    _bn_case(kind, _bn_special(kind).astype(np.float32), False, seed=41)


@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm_beyond_the_split_and_grid_caps(relu):
    """131100 rows: the smallest count above 256 splits x 512 rows, so the splits grow past 512 rows; with 12 channels also more than
    4096 x 256 elements, so the grid-stride loops of the element-wise kernels take a second trip."""
    rows, ch = 131100, 12
    assert rows > 256 * 512 and rows * ch > 4096 * 256
    _bn_case("large", _bn_input(rows, ch, 9), relu, seed=77)


# ------------------------------------------------------------------------------------------------ point_affine
@pytest.mark.parametrize("per_cloud", [False, True])
@pytest.mark.parametrize("clouds,n", [(3, 7), (3, 171)])
@pytest.mark.parametrize("ch", [1, 65, 512])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_point_affine_forward_and_backward(d, ch, clouds, n, per_cloud):
    """Shared grid (x needs no gradient: the dx == NULL branch) and per-cloud x with dx; 3 x 171 = 513 rows are two splits of the
    weight-gradient reduction.  wp is the first d columns of a wider weight, x a column slice."""
    A = net()
    rng = np.random.RandomState(1000 * d + ch + n)
    xr = clouds * n if per_cloud else n
    x, w = rng.randn(xr, d).astype(np.float32), rng.randn(ch, d + 5).astype(np.float32)
    t, dy = rng.randn(clouds, ch).astype(np.float32), rng.randn(clouds * n, ch).astype(np.float32)
    ref_dx, ref_dw, ref_dt = F.point_affine_bwd(dy, x, w[:, :d], clouds, n, per_cloud)
    ref = dict(y=F.point_affine(x, w[:, :d], t, clouds, n, per_cloud), dwp=ref_dw, dt=ref_dt)
    xt, wt, tt = (torch.tensor(a, requires_grad=True) for a in (x, w, t))
    pts = xt.view(clouds, n, d) if per_cloud else xt[None].expand(clouds, n, d)
    y32 = (pts @ wt[:, :d].t() + tt[:, None, :]).reshape(clouds * n, ch)
    y32.backward(torch.tensor(dy))
    t32 = dict(y=y32.detach().numpy(), dwp=wt.grad[:, :d].numpy(), dt=tt.grad.numpy())
    big, xs = sliced(x, left=2, right=1, grad=per_cloud)
    wd, td = dev(w, grad=True), dev(t, grad=True)
    wp = wd[:, :d]
    assert wp.stride(0) == d + 5 and xs.stride(0) == d + 3
    y = A.PointAffineFn.apply(xs, wp, td, clouds, n, per_cloud)
    y.backward(dev(dy))
    got = dict(y=y, dwp=wd.grad[:, :d], dt=td.grad)
    assert (host(wd.grad[:, d:]) == 0).all()
    if per_cloud:
        ref["dx"], t32["dx"], got["dx"] = ref_dx, xt.grad.numpy(), big.grad[:, 2:2 + d]
        g = host(big.grad)
        assert (g[:, :2] == 0).all() and (g[:, 2 + d:] == 0).all()
    else:
        assert big.grad is None
    check_all([bounded("point_affine d=%d ch=%d %dx%d per_cloud=%d %s" % (d, ch, clouds, n, per_cloud, k), got[k], ref[k], t32[k])
               for k in ref])
