"""GPU: the floor-plan encoder (csrc/floorplan.hip, networks/feature_extractors.py) and its wiring into the scene-layout wrapper.

 1. selection / movement kernels bit for bit: the patch gather against F.unfold (columns reordered to the kernel's (ky, kx, c) order), the
    max-pool and the routing of its backward against F.max_pool2d(return_indices=True) on the CPU;
 2. write sets: every output sits inside a sentinel-filled buffer, nothing outside it changes, the K padding of the patches is zero;
 3. summing kernels against float64 at the derived bound n * 2^-24 * sum |terms| per element, n = the roundings of the kernel's own
    expression (stated at each assert);
 4. the whole encoder, forward and every gradient, against the float64 oracle (tests/floorplan_oracle.py) evaluated under the HIP
    forward's own ReLU / max-pool decisions: the errors may be at most 2 x those of the float32 CPU oracle under the same decisions;
 5. the wrapper against the real reference class paired with the oracle encoder (tests/golden/floorplan_wrapper.npz);
 6. the training seam (autograd path, optimizer, EMA) and the sampling entry points.
DSC_PARITY_LOG=<file> records the measured figures (profiles/floorplan_parity.txt)."""
import contextlib
import copy
import io
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import weights as W  # noqa: E402

import floorplan_oracle as FO  # noqa: E402
from test_floorplan_host import room_config  # noqa: E402
from test_gpu_wide import check, dev  # noqa: E402
from test_gpu_wrapper import cpu_rng  # noqa: E402,F401

U = 2.0 ** -24
QUIET = contextlib.redirect_stdout(io.StringIO())


def _log(line):
    print(line)
    if os.environ.get("DSC_PARITY_LOG"):
        with open(os.environ["DSC_PARITY_LOG"], "a") as f:
            f.write(line + "\n")


def rows_of(x):
    """(B, C, H, W) -> the kernels' [b * h * w][c]."""
    b, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(b * h * w, c).contiguous()


def nchw(rows, b, h, w):
    return rows.reshape(b, h, w, rows.shape[1]).permute(0, 3, 1, 2).contiguous()


def unfold_rows(x, k, s, p):
    """F.unfold's columns (c, ky, kx) reordered to the kernel's (ky, kx, c), one row per output pixel, without the K padding."""
    b, c = x.shape[:2]
    u = F.unfold(x, k, padding=p, stride=s)                                  # (b, c k k, L)
    return u.reshape(b, c, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * c)


CONV_SHAPES = [(2, 9, 7, 3, 7, 2, 3), (1, 5, 6, 64, 3, 1, 1), (3, 7, 5, 64, 3, 2, 1), (2, 5, 5, 64, 1, 2, 0)]
POOL_SIDES = [(1, 1), (2, 3), (7, 8)]


# ------------------------------------------------------------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize("b,h,w,c,k,s,p", CONV_SHAPES)
def test_conv_patches_is_unfold_bit_for_bit(b, h, w, c, k, s, p):
    from diffuscene_amd import ops
    x = torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(h * w + c))
    got = ops.conv_patches(rows_of(x).to(dev()), (b, h, w), k, s, p).cpu()
    want = unfold_rows(x, k, s, p)
    kk = k * k * c
    assert got.shape == (want.shape[0], ops.conv_kpad(c, k)) and got.shape[1] % 32 == 0
    assert torch.equal(got[:, :kk], want)
    assert not got[:, kk:].any()


def _pool_inputs(b, c, h, w):
    g = torch.Generator().manual_seed(31 * h + w)
    ties = torch.relu(torch.randn(b, c, h, w, generator=g))                 # post-ReLU: exact ties at 0
    ties[0, 0] = 0.0                                                         # a plane of nothing but ties
    negative = -torch.rand(b, c, h, w, generator=g) - 0.5                    # the zero padding would win if it took part
    return {"ties": ties, "negative": negative}


def _slots_to_indices(arg, b, h, w):
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    slot = nchw(arg, b, ho, wo).to(torch.int64)
    oy, ox = torch.arange(ho).view(1, 1, -1, 1), torch.arange(wo).view(1, 1, 1, -1)
    return (oy * 2 - 1 + slot // 3) * w + (ox * 2 - 1 + slot % 3)


@pytest.mark.parametrize("c", [64, 3])
@pytest.mark.parametrize("h,w", POOL_SIDES)
def test_maxpool_and_its_routing_are_torch_bit_for_bit(h, w, c):
    from diffuscene_amd import ops
    b = 2
    for name, x in _pool_inputs(b, c, h, w).items():
        want, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
        y, arg = ops.maxpool2d(rows_of(x).to(dev()), (b, h, w))
        ho, wo = want.shape[2:]
        assert torch.equal(nchw(y.cpu(), b, ho, wo), want), name
        assert torch.equal(_slots_to_indices(arg.cpu(), b, h, w), idx), name
        if name == "negative":
            assert float(y.max()) < 0.0
        # routing: one-hot dy at a handful of outputs, then a dense integer-valued dy (sums of at most four small integers are exact)
        g = torch.Generator().manual_seed(7)
        dys = []
        for _ in range(4):
            one = torch.zeros(b, c, ho, wo)
            one.view(-1)[int(torch.randint(0, one.numel(), (1,), generator=g))] = 1.0
            dys.append(one)
        dys.append(torch.randint(-8, 9, (b, c, ho, wo), generator=g).float())
        xr = x.clone().requires_grad_()
        yr = F.max_pool2d(xr, 3, 2, 1)
        for dy in dys:
            want_dx, = torch.autograd.grad(yr, xr, dy, retain_graph=True)
            dx = ops.maxpool2d_bwd(rows_of(dy).to(dev()), arg, (b, h, w))
            assert torch.equal(nchw(dx.cpu(), b, h, w), want_dx), name


# ------------------------------------------------------------------------------------------------------------------- 2. write sets
GUARD = 64


def _guarded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), -7777.0 if dtype == torch.float32 else 0xA5, dtype=dtype, device=dev())
    return big, big[GUARD:GUARD + n].view(shape)


def _untouched(big, what):
    sent = big[0].item()
    assert bool((big[:GUARD] == sent).all()) and bool((big[-GUARD:] == sent).all()), what + ": wrote outside its output"
    assert not bool((big[GUARD:-GUARD] == sent).any()), what + ": left part of its output unwritten"


@pytest.mark.parametrize("b,h,w,c,k,s,p", CONV_SHAPES)
def test_write_sets_of_the_conv_kernels(b, h, w, c, k, s, p):
    from diffuscene_amd import ops
    x = torch.rand(b * h * w, c, device=dev()) + 1.0
    ho, wo = ops.conv_out_size(h, k, s, p), ops.conv_out_size(w, k, s, p)
    big, out = _guarded((b * ho * wo, ops.conv_kpad(c, k)))
    ops.conv_patches(x, (b, h, w), k, s, p, out=out)
    _untouched(big, "conv_patches")
    assert not out[:, k * k * c:].any()                                      # the K padding inside the output is zero, not skipped
    dp = torch.rand_like(out) + 1.0
    big, dx = _guarded((b * h * w, c))
    ops.conv_patches_bwd(dp, (b, h, w), c, k, s, p, out=dx)
    _untouched(big, "conv_patches_bwd")


@pytest.mark.parametrize("c", [64, 3])
@pytest.mark.parametrize("h,w", POOL_SIDES)
def test_write_sets_of_the_pool_kernels(h, w, c):
    from diffuscene_amd import ops
    b = 3
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = torch.rand(b * h * w, c, device=dev()) + 1.0
    big_y, y = _guarded((b * ho * wo, c))
    big_a, arg = _guarded((b * ho * wo, c), torch.uint8)
    ops.maxpool2d(x, (b, h, w), out=y, arg=arg)
    _untouched(big_y, "maxpool2d y")
    _untouched(big_a, "maxpool2d arg")
    big, dx = _guarded((b * h * w, c))
    ops.maxpool2d_bwd(y, arg, (b, h, w), out=dx)
    assert bool((big[:GUARD] == -7777.0).all()) and bool((big[-GUARD:] == -7777.0).all()) and not bool((dx == -7777.0).any())
    big, m = _guarded((b, c))
    ops.avgpool_rows(x, b, out=m)
    _untouched(big, "avgpool_rows")
    big, dxa = _guarded((b * h * w, c))
    ops.avgpool_rows_bwd(m, h * w, out=dxa)
    _untouched(big, "avgpool_rows_bwd")


@pytest.mark.parametrize("rows,ch", [(389, 64), (3, 512)])
def test_write_sets_of_the_frozen_bn_kernels(rows, ch):
    from diffuscene_amd import ops
    x = torch.rand(rows, ch, device=dev()) + 1.0
    wgt, bias, mean, var = (torch.rand(ch, device=dev()) + 0.5 for _ in range(4))
    big, y = _guarded((rows, ch))
    ops.frozen_bn_act(x, wgt, bias, mean, var, residual=x, relu=True, out=y)
    _untouched(big, "frozen_bn_act")
    bigs, outs = zip(*[_guarded(s) for s in ((rows, ch), (rows, ch), (ch,), (ch,))])
    ops.frozen_bn_act_bwd(x, y, x, wgt, mean, var, relu=True, want_residual=True, outs=outs)
    for bg, name in zip(bigs, ("dx", "dresidual", "dweight", "dbias")):
        _untouched(bg, "frozen_bn_act_bwd " + name)


# ------------------------------------------------------------------------------------------------------------------- 3. summing kernels
def _within(got, want, n, terms, what):
    """|got - want| <= n * 2^-24 * sum |terms| for every element; logs the largest ratio."""
    err = (got.double().cpu() - want).abs()
    bound = n * U * terms
    ratio = float((err / bound.clamp_min(1e-300)).max())
    _log("%s: max error / (n = %d bound) = %.3g" % (what, n, ratio))
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("b,h,w,c,k,s,p", CONV_SHAPES)
def test_conv_patches_bwd_against_float64(b, h, w, c, k, s, p):
    from diffuscene_amd import ops
    g = torch.Generator().manual_seed(k + c)
    ho, wo = ops.conv_out_size(h, k, s, p), ops.conv_out_size(w, k, s, p)
    kk, kpad = k * k * c, ops.conv_kpad(c, k)
    dp = torch.randn(b * ho * wo, kpad, generator=g)
    got = ops.conv_patches_bwd(dp.to(dev()), (b, h, w), c, k, s, p)
    x = torch.zeros(b, c, h, w, dtype=torch.float64, requires_grad=True)
    patches = unfold_rows(x, k, s, p)
    want, = torch.autograd.grad(patches, x, dp[:, :kk].double())
    terms, = torch.autograd.grad(patches, x, dp[:, :kk].double().abs())
    # n = 2: the sum is taken in float64 (its own roundings are below 2^-50 of the terms) and rounded to float32 once
    _within(nchw(got, b, h, w), want, 2, terms, "conv_patches_bwd %s" % ((b, h, w, c, k, s, p),))


@pytest.mark.parametrize("b,hw,ch", [(3, 1, 512), (2, 6, 64), (5, 56, 12), (2, 64, 3)])
def test_avgpool_both_directions_against_float64(b, hw, ch):
    from diffuscene_amd import ops
    g = torch.Generator().manual_seed(hw + ch)
    x = torch.randn(b * hw, ch, generator=g)
    x64 = x.double().view(b, hw, ch)
    # n = 2: sum and division in float64, one rounding to float32
    _within(ops.avgpool_rows(x.to(dev()), b), x64.mean(1), 2, x64.abs().sum(1) / hw, "avgpool_rows %s" % ((b, hw, ch),))
    dy = torch.randn(b, ch, generator=g)
    want = (dy.double() / hw)[:, None, :].expand(b, hw, ch).reshape(b * hw, ch)
    # n = 1: one division
    _within(ops.avgpool_rows_bwd(dy.to(dev()), hw), want, 1, want.abs(), "avgpool_rows_bwd %s" % ((b, hw, ch),))


@pytest.mark.parametrize("rows,ch,relu,res", [(389, 64, True, True), (1000, 128, True, False), (3, 512, False, True), (77, 256, False, False)])
def test_frozen_bn_act_both_directions_against_float64(rows, ch, relu, res):
    from diffuscene_amd import ops
    g = torch.Generator().manual_seed(rows + ch)
    x = torch.randn(rows, ch, generator=g)
    wgt = 1.0 + 0.3 * torch.randn(ch, generator=g)
    bias = 0.2 * torch.randn(ch, generator=g)
    mean = 0.5 * torch.randn(ch, generator=g)                                # non-trivial running statistics
    var = 0.3 + 2.0 * torch.rand(ch, generator=g)
    r = torch.randn(rows, ch, generator=g) if res else None
    d = lambda t: None if t is None else t.to(dev())                         # noqa: E731
    y = ops.frozen_bn_act(d(x), d(wgt), d(bias), d(mean), d(var), residual=d(r), relu=relu)
    s64 = wgt.double() / var.double().sqrt()
    pre = x.double() * s64 + (bias.double() - mean.double() * s64) + (r.double() if res else 0.0)
    want = pre.clamp_min(0.0) if relu else pre
    terms = (x.double() * s64).abs() + bias.double().abs() + (mean.double() * s64).abs() + (r.double().abs() if res else 0.0)
    # n = 2: the whole expression is evaluated in float64 and rounded to float32 once
    _within(y, want, 2, terms, "frozen_bn_act %s" % ((rows, ch, relu, res),))
    if relu:
        assert float(y.min()) >= 0.0
    dy = torch.randn(rows, ch, generator=g)
    dx, dres, dw, db = ops.frozen_bn_act_bwd(d(dy), y if relu else None, d(x), d(wgt), d(mean), d(var), relu=relu, want_residual=res and relu)
    mask = (y.cpu() > 0).double() if relu else torch.ones(rows, ch, dtype=torch.float64)       # the ReLU mask is the forward's own y > 0
    g64 = dy.double() * mask
    # n = 2: s and the product in float64, one rounding
    _within(dx, g64 * s64, 2, (g64 * s64).abs(), "frozen_bn_act_bwd dx %s" % ((rows, ch, relu, res),))
    if res and relu:
        assert torch.equal(dres.cpu().double(), g64)                         # a selection: exact
    xhat = (x.double() - mean.double()) / var.double().sqrt()
    # n = 2: terms and column sums in float64, one rounding of the finished sum
    _within(dw, (g64 * xhat).sum(0), 2, (g64 * xhat).abs().sum(0), "frozen_bn_act_bwd dweight %s" % ((rows, ch, relu, res),))
    # n = 2: as dweight
    _within(db, g64.sum(0), 2, g64.abs().sum(0), "frozen_bn_act_bwd dbias %s" % ((rows, ch, relu, res),))


def test_plain_relu_form_of_the_frozen_bn_kernel():
    from diffuscene_amd import ops
    x = torch.randn(5, 512, generator=torch.Generator().manual_seed(1))
    y = ops.frozen_bn_act(x.to(dev()), None, None, None, None, relu=True)
    assert torch.equal(y.cpu(), torch.relu(x))
    dy = torch.randn(5, 512, generator=torch.Generator().manual_seed(2))
    dx, dres, dw, db = ops.frozen_bn_act_bwd(dy.to(dev()), y, None, None, None, None, relu=True)
    assert torch.equal(dx.cpu(), dy * (x > 0)) and dres is None and dw is None and db is None


# ------------------------------------------------------------------------------------------------------------------- 4. whole encoder
ENCODER_CASES = [(2, 32, 32, 1, 64, 101), (3, 33, 47, 2, 64, 102), (1, 8, 8, 1, 64, 103)]       # (B, H, W, input_channels, feature_size, seed)
FLIP_MARGIN, FLIP_SHARE = 1e-5, 1e-3


def encoder_inputs(b, h, w, cin, feat, seed):
    g = torch.Generator().manual_seed(seed)
    sd = FO.init_state_dict(cin, feat, seed)
    x = (torch.rand(b, cin, h, w, generator=g) > 0.4).float() * (0.5 + torch.rand(b, cin, h, w, generator=g))
    dy = torch.randn(b, feat, generator=g)
    return sd, x, dy


def oracle_run(sd, x, dy, dtype, decisions):
    """Forward and every gradient of the oracle in ``dtype`` under ``decisions`` -> (y, {name: gradient}, trace)."""
    leaves = {k: v.to(dtype).clone().requires_grad_(not k.endswith(("running_mean", "running_var"))) for k, v in sd.items()}
    xin = x.to(dtype).clone().requires_grad_()
    trace = {}
    y = FO.forward(leaves, xin, decisions=decisions, trace=trace)
    y.backward(dy.to(dtype))
    grads = {k: v.grad for k, v in leaves.items() if v.requires_grad}
    grads["input"] = xin.grad
    return y.detach(), grads, trace


def decision_flips(decisions, free):
    """(share of decisions that differ from the free float64 oracle's, the largest |float64 pre-activation| / rms among them)."""
    flips, total, worst = 0, 0, 0.0
    for mask, fmask, pre in zip(decisions["relu"], free["relu"], free["pre"]):
        diff = mask.cpu() != fmask
        flips, total = flips + int(diff.sum()), total + diff.numel()
        if diff.any():
            worst = max(worst, float(pre[diff].abs().max() / pre.pow(2).mean().sqrt()))
    xin = free["pool_in"]
    b, c = xin.shape[:2]
    flat = xin.reshape(b, c, -1)
    diff = decisions["pool"].cpu() != free["pool"]
    flips, total = flips + int(diff.sum()), total + diff.numel()
    if diff.any():
        gap = (flat.gather(2, decisions["pool"].cpu().reshape(b, c, -1)) - flat.gather(2, free["pool"].reshape(b, c, -1))).abs()
        worst = max(worst, float(gap.max() / xin.pow(2).mean().sqrt()))
    return flips / total, worst


def distances(a, ref):
    a, ref = a.double().cpu(), ref.double()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300)), float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("b,h,w,cin,feat,seed", ENCODER_CASES)
def test_whole_encoder_forward_and_gradients_against_float64(b, h, w, cin, feat, seed):
    """Criterion: norm-relative and max element-wise error of HIP against float64 at most 2 x those of the float32 CPU oracle, all three
    under the HIP forward's decisions.  Measured on the MI355X (profiles/floorplan_parity.txt holds every tensor's figures): the largest
    ratios over the 64 tensors of the three shapes are 1.48 (norm-relative) and 1.71 (element-wise); the forward sits at 1.22 / 1.17,
    1.48 / 1.69 and 1.06 / 1.17; no decision differs from the free float64 oracle's."""
    from diffuscene_amd.networks.feature_extractors import get_feature_extractor
    sd, x, dy = encoder_inputs(b, h, w, cin, feat, seed)
    enc = get_feature_extractor("resnet18", freeze_bn=True, input_channels=cin, feature_size=feat)
    enc.load_state_dict(sd)
    enc.to(dev())
    enc._record = {"relu": [], "pool": None}
    xd = x.to(dev()).requires_grad_()
    y = enc(xd)
    decisions = {"relu": [m.cpu() for m in enc._record["relu"]], "pool": enc._record["pool"].cpu()}
    enc._record = None
    assert len(decisions["relu"]) == 18
    y.backward(dy.to(dev()))
    got = {k: p.grad for k, p in enc.named_parameters()}
    got["input"] = xd.grad
    # the HIP decisions against the free float64 oracle's: only where the oracle's own pre-activation is within rounding of zero
    _, _, free = oracle_run(sd, x, dy, torch.float64, None)
    share, worst = decision_flips(decisions, free)
    _log("encoder %s: %.4f%% of the decisions differ from float64's, largest |pre| / rms among them %.3g" % ((b, h, w, cin), 100 * share, worst))
    assert share <= FLIP_SHARE and worst < FLIP_MARGIN
    y64, g64, _ = oracle_run(sd, x, dy, torch.float64, decisions)
    y32, g32, _ = oracle_run(sd, x, dy, torch.float32, decisions)
    assert set(got) == set(g64)
    failures = []
    for name, ours, cpu32, ref in [("forward", y.detach(), y32, y64)] + [(k, got[k], g32[k], g64[k]) for k in sorted(g64)]:
        hn, hm = distances(ours, ref)
        cn, cm = distances(cpu32, ref)
        _log("encoder %s %-55s hip %.3g / %.3g  cpu-f32 %.3g / %.3g  ratio %.2f / %.2f"
             % ((b, h, w, cin), name, hn, hm, cn, cm, hn / max(cn, 1e-300), hm / max(cm, 1e-300)))
        if hn > 2 * cn or hm > 2 * cm:
            failures.append((name, hn, cn, hm, cm))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- 5. wrapper
def _golden_module():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_floorplan_golden.py")
    spec = importlib.util.spec_from_file_location("make_floorplan_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden_model(G, case, tmp_path, time_num):
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    from diffuscene_amd.networks.feature_extractors import get_feature_extractor
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = G.room_network_config(case, str(stats), time_num)
    with QUIET:
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, get_feature_extractor("resnet18", True, 1, G.FEATURE), cfg)
    m.load_state_dict(G.room_state_dict(m), strict=True)
    return m.to(dev()), cfg


@pytest.mark.parametrize("case", ["room", "roominst"])
def test_wrapper_against_the_reference_class(case, golden_dir, tmp_path, cpu_rng):  # noqa: F811
    G = _golden_module()
    g = np.load(os.path.join(golden_dir, "floorplan_wrapper.npz"))
    m, cfg = _golden_model(G, case, tmp_path, 1000)
    s = {k: v.to(dev()) for k, v in G.room_batch().items()}
    with torch.no_grad():
        _, condition, cross = m._loss_inputs(s)
    assert cross is None
    check(condition, g[case + ".condition"], case + " condition", tol=2e-5)
    torch.manual_seed(G.SEED_LOSS)
    with torch.no_grad():
        loss, parts = m.get_loss(s)
    want = float(g[case + ".loss"])
    assert abs(float(loss) - want) <= 1e-4 * abs(want), (case, float(loss), want)
    part_keys = [k[len(case) + 6:] for k in g.files if k.startswith(case + ".part.")]
    assert sorted(parts) == sorted(part_keys)
    for k in part_keys:
        wv = float(g[case + ".part." + k])
        assert abs(float(parts[k]) - wv) <= 1e-4 * max(abs(wv), 1e-3), (case, k, float(parts[k]), wv)
    m, cfg = _golden_model(G, case, tmp_path, G.SAMPLE_T)
    torch.manual_seed(G.SEED_SAMPLE)
    with torch.no_grad(), QUIET:
        y = m.sample(G.room_masks().to(dev()), G.N, cfg["point_dim"], batch_size=G.B, clip_denoised=True)
    check(y, g[case + ".sample"], "%s sample(B=%d, T=%d)" % (case, G.B, G.SAMPLE_T))


# ------------------------------------------------------------------------------------------------------------------- 6. training, sampling
B_TRAIN, N_OBJ, SIDE = 2, 12, 32


def _masks(b, seed=5):
    return _golden_module().room_masks(b, SIDE, seed).to(dev())


def _room_model(tmp_path, seed=0, time_num=1000, instance=True):
    from diffuscene_amd.networks import build_network
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = room_config(instance=instance)
    cfg["network"]["diffusion_kwargs"].update(train_stats_file=str(stats), time_num=time_num)
    torch.manual_seed(seed)
    with QUIET:
        net, _, _ = build_network(62, 23, cfg)
    sd = W.synth_state_dict(cfg["network"]["net_kwargs"], prefix="diffusion.model.")
    sd.update({"feature_extractor." + k: v for k, v in FO.init_state_dict(1, 64, 40 + seed).items()})
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"positional_embedding", "fc_room_f.weight", "fc_room_f.bias"}
    return net.to(dev())


def _train_batch():
    x = W.synth_scene_batch(B_TRAIN, N_OBJ, 22, 32, seed=3).to(dev())
    return {"translations": x[:, :, 0:3].contiguous(), "sizes": x[:, :, 3:6].contiguous(), "angles": x[:, :, 6:8].contiguous(),
            "class_labels": x[:, :, 8:30].contiguous(), "objfeats_32": x[:, :, 30:].contiguous(), "room_layout": _masks(B_TRAIN)}


def _flat(scene):
    return torch.cat([scene[k].reshape(scene[k].shape[0], -1).float() for k in sorted(scene)], dim=1)


def _flat_list(scenes):
    return [_flat(s) for s in scenes]


def test_training_seam_optimizer_and_ema(tmp_path):
    from diffuscene_amd.networks import optimizer_factory
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import train_on_batch
    from diffuscene_amd.optim import ema_model_state
    from diffuscene_amd.train_step import plan_supported
    net = _room_model(tmp_path)
    assert not plan_supported(net)                                           # these models train on the autograd path
    opt = optimizer_factory({"optimizer": "Adam", "lr": 2e-4, "ema_decay": 0.5}, filter(lambda p: p.requires_grad, net.parameters()))
    twin = copy.deepcopy(net.feature_extractor)                              # the encoder as it is BEFORE the step
    before = {k: p.detach().clone() for k, p in net.feature_extractor.named_parameters()}
    seen = {}

    def hook(module, args, output):
        output.register_hook(lambda grad: seen.__setitem__("g", grad.detach().clone()))
    handle = net.feature_extractor.register_forward_hook(hook)
    s = _train_batch()
    torch.manual_seed(9)
    loss = train_on_batch(net, opt, s, {"training": {"max_grad_norm": 10}})
    handle.remove()
    assert np.isfinite(loss) and "g" in seen and tuple(seen["g"].shape) == (B_TRAIN, 64)
    twin(s["room_layout"]).backward(seen["g"])
    for (k, p), q in zip(net.feature_extractor.named_parameters(), twin.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k          # the seam: the same kernels on the same gradient
        assert not torch.equal(p.detach(), before[k]), k + " did not move"
    mask = _masks(1, seed=8)

    def sample(model):
        torch.manual_seed(5)
        with QUIET:
            return _flat(model.generate_layout(mask, N_OBJ, 62, batch_size=1, keep_empty=True, clip_denoised=True, sampling_timesteps=2))
    raw = sample(net)
    other = _room_model(tmp_path, seed=1)
    other.load_state_dict(ema_model_state(net, opt))
    from_state = sample(other)
    with opt.ema_weights():
        swapped = sample(net)
    assert not torch.equal(swapped, raw)
    assert torch.equal(swapped, from_state)
    assert torch.equal(sample(net), raw)


def test_one_room_for_all_layouts_equals_the_repeated_mask(tmp_path):
    net = _room_model(tmp_path, time_num=20)
    one = _masks(1, seed=8)
    kw = dict(keep_empty=True, clip_denoised=True, scene_seeds=[3, 4, 5])
    with QUIET:
        a = _flat_list(net.generate_layout_batched(one, N_OBJ, 62, 3, **kw))
        b = _flat_list(net.generate_layout_batched(one.repeat(3, 1, 1, 1), N_OBJ, 62, 3, **kw))
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("strided", [None, 5])
def test_eager_and_captured_loops_agree_with_wall_steering(tmp_path, monkeypatch, strided):
    net = _room_model(tmp_path, time_num=20)
    masks = _masks(3)
    kw = dict(keep_empty=True, clip_denoised=True, scene_seeds=[1, 2, 3], wall_scale=0.5, room_side=3.1)
    if strided is not None:
        kw["sampling_timesteps"] = strided
    with QUIET:
        captured = _flat_list(net.generate_layout_batched(masks, N_OBJ, 62, 3, **kw))
        monkeypatch.setenv("DSC_GRAPH", "0")
        eager = _flat_list(net.generate_layout_batched(masks, N_OBJ, 62, 3, **kw))
    for u, v in zip(captured, eager):
        assert torch.equal(u, v) and bool(torch.isfinite(u).all())


def test_the_mask_steers_the_scene_and_a_wrong_batch_is_refused(tmp_path):
    net = _room_model(tmp_path, time_num=20)
    kw = dict(keep_empty=True, clip_denoised=True, scene_seeds=[1, 2])
    with QUIET:
        a = _flat_list(net.generate_layout_batched(_masks(2, seed=5), N_OBJ, 62, 2, **kw))
        b = _flat_list(net.generate_layout_batched(_masks(2, seed=6), N_OBJ, 62, 2, **kw))
    assert all(not torch.equal(u, v) for u, v in zip(a, b))
    state = torch.cuda.get_rng_state()
    cpu_state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match="room_mask holds 2 rooms for a batch of 3"):
        net.generate_layout_batched(_masks(2), N_OBJ, 62, 3)
    assert torch.equal(torch.cuda.get_rng_state(), state) and torch.equal(torch.random.get_rng_state(), cpu_state)
