"""GPU: the split-bf16 GEMM path (csrc/gemm_split.hip: f32 operands split exactly into 3 bf16 pieces, 6 products, f32 accumulation on
the bf16 matrix cores) behind dsc_gemm_f32 / dsc_gemm_gn_silu_f32.  Same tolerances as the exact-f32 MFMA kernels in test_gpu_ops.py
(2e-6 of the result's max against an f64 evaluation), plus: the plane split is EXACT, and the error against f64 is not larger than
the f32 path's on the same operands (the GO criterion of the round-3 experiment, profiles/r03_bf16x6_*.txt)."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def split_on():
    """The library's arithmetic switch (DSC_GEMM=f32 / set_gemm_arithmetic("f32"): every launch stays on the exact-f32 MFMA kernel)."""
    from diffuscene_amd import _lib
    return _lib.split_enabled()


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rms_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def planes_to_f32(planes):
    return (planes.to(torch.int32) << 16).view(torch.float32)


@pytest.mark.parametrize("scale", [1.0, 1e-6, 3e4])
def test_plane_split_is_exact_and_transposable(scale):
    """w1 + w2 + w3 == w bit for bit at any magnitude (bf16 keeps the f32 exponent range); the transposed form holds w^T."""
    from diffuscene_amd import ops
    w = (torch.randn(384, 160, generator=torch.Generator().manual_seed(1)) * scale).to(dev())
    w[0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 1.5e-30, 65504.0, 1.0 + 2 ** -23, -(1.0 - 2 ** -24)], device=dev())
    p, pt = ops.split_planes([(w, None, False), (w, None, True)])
    f = planes_to_f32(p)
    assert torch.equal((f[0] + f[1]) + f[2], w)
    ft = planes_to_f32(pt)
    assert tuple(pt.shape) == (3, 160, 384) and torch.equal((ft[0] + ft[1]) + ft[2], w.t())
    # a strided view (rows of a wider buffer) splits like its contiguous copy
    wide = torch.randn(64, 512, device=dev())
    (pv,) = ops.split_planes([(wide[:, 128:384], None, False)])
    (pc,) = ops.split_planes([(wide[:, 128:384].contiguous(), None, False)])
    assert torch.equal(pv, pc)


def test_plan_backend_split_steps_match_the_eager_split():
    """train_plan.HipBackend.split_steps, the training plan's route to the launch record of dsc_split_bf16x3_f32, at the smallest shape the
    plane cache takes (128 x 32): a row-strided weight in both plane layouts and a transposed copy whose planes are split straight from
    its source (the copy itself, NaN here, is never read).  The planes are exact and bit-equal to the eager wrapper's."""
    from diffuscene_amd import ops
    from diffuscene_amd.train_plan import HipBackend
    be = HipBackend(dev())
    be.split = True                                     # the plane cache whatever DSC_GEMM says: the split launch is the same
    w = rnd(128, 96, seed=3).to(dev())[:, 32:64]        # [128][32], rows of a wider buffer: ldw = 96
    src = rnd(32, 192, seed=4).to(dev())[:, 32:160]     # [32][128]; its transpose is the weight operand wt
    wt = torch.full((128, 32), float("nan"), device=dev())
    be.transposed_of[wt.data_ptr()] = src
    pr, pf = be.planes_of(w, 256, ops.PLANES_ROWMAJOR), be.planes_of(w, 256, ops.PLANES_FRAGMENT)
    pt = be.planes_of(wt, 256, ops.PLANES_ROWMAJOR)
    assert pr is not None and pf is not None and pt is not None and pr is not pf
    steps = be.split_steps()
    assert len(steps) == 1 and be.split_steps() == []
    be.finalize()
    be.run(steps, ops.stream_ptr())
    torch.cuda.synchronize()
    f, ft = planes_to_f32(pr), planes_to_f32(pt)
    assert torch.equal((f[0] + f[1]) + f[2], w) and torch.equal((ft[0] + ft[1]) + ft[2], src.t())
    er, et = ops.split_planes([(w, None, False), (src, None, True)])
    assert torch.equal(pr, er) and torch.equal(pf, ops.fragment_major(er)) and torch.equal(pt, et)


@pytest.mark.parametrize("m,n,k,taken", [(20480, 512, 512, True), (5376, 512, 512, True), (10240, 512, 1024, True), (10240, 384, 512, True),
                                         (1536, 1024, 512, False), (300, 128, 96, False), (40000, 128, 96, True), (20480, 3072, 512, True),
                                         (2560, 2048, 2048, True)])
def test_split_gemm_plain(m, n, k, taken):
    """Dense products of every tile class (160x256, 256x128, 160x128 four-wave, 128x128, 64x256) and the launches the dispatcher leaves
    to the exact-f32 kernel because they would not fill the chip (`taken` False: bit-identical to the f32 path)."""
    from diffuscene_amd import ops
    a, w, b = rnd(m, k, seed=1), rnd(n, k, seed=2, scale=0.1), rnd(n, seed=3)
    ad, wd, bd = a.to(dev()), w.to(dev()), b.to(dev())
    (pl,) = ops.split_planes([(wd, None, False)])
    y = ops.gemm(ad, wd, bd, w_planes=pl)
    y32 = ops.gemm(ad, wd, bd)
    ref = a.double() @ w.double().T + b.double()
    assert rel(y, ref) < 2e-6 * max(1.0, k / 1024), (m, n, k, rel(y, ref))     # (the exact-f32 kernel itself reaches 2.1e-6 at K = 2048)
    # same rounding-noise class as the exact-f32 kernel, whose own rms moves by 30 % with its tile's summation order (measured:
    # 0.8 .. 1.4 x the f32 kernel's at K >= 128; 2 x at K = 96 where both are ~1e-7)
    assert rms_err(y, ref) <= max(1.5 * rms_err(y32, ref), 2.5e-7), (rms_err(y, ref), rms_err(y32, ref))
    assert torch.equal(y, y32) != (taken and split_on()), "dispatch: split path %s this launch" % ("did not take" if taken else "took")
    assert ops.gemm_uses_split(ops.make_gemm_args(ad, wd, y, bd, w_planes=pl)) == (taken and split_on())      # the library's own answer
    assert not ops.gemm_uses_split(ops.make_gemm_args(ad, wd, y, bd))


@pytest.mark.parametrize("act_out", [0, 1, 2])
def test_split_gemm_two_segments_residual_activation(act_out):
    """torch.cat of a skip connection = second K segment (own row stride), fused GELU / SiLU, residual, ragged M."""
    from diffuscene_amd import ops
    m, n = 10001, 512
    wide = rnd(m, 1536, seed=4)                      # a1 = a column slice of a wider buffer: lda1 != lda2
    a1, a2 = wide[:, 512:1024], rnd(m, 512, seed=5)
    w, b, r = rnd(n, 1024, seed=6, scale=0.05), rnd(n, seed=7), rnd(m, n, seed=8)
    wd = w.to(dev())
    (pl,) = ops.split_planes([(wd, None, False)])
    y = ops.gemm(wide.to(dev())[:, 512:1024], wd, b.to(dev()), a2=a2.to(dev()), residual=r.to(dev()), act_out=act_out, w_planes=pl)
    z = torch.cat([a1, a2], 1).double() @ w.double().T + b.double()
    if act_out == 1:
        z = F.gelu(z)
    elif act_out == 2:
        z = F.silu(z)
    assert rel(y, z + r.double()) < 2e-6


def _gn_ref(a, w, b, gamma, beta, N, ss, mode, res, idx=None):
    B = a.shape[0] // N
    z = a.double() @ w.double().T + b.double()
    zg = z.view(B, N, -1, 64)
    mu = zg.mean(dim=(1, 3), keepdim=True)
    var = zg.var(dim=(1, 3), unbiased=False, keepdim=True)
    y = ((zg - mu) / (var + 1e-5).sqrt()).view(B, N, -1) * gamma.double() + beta.double()
    n = w.shape[0]
    if mode == 1:
        s = ss.double().view(B, N, 2 * n)
    elif mode == 2:
        s = ss.double()[:, None, :]
    elif mode == 3:
        s = ss.double()[None, :, :]
    elif mode == 4:
        s = ss.double()[idx][:, None, :]
    if mode:
        y = y * (s[..., :n] + 1) + s[..., n:]
    y = F.silu(y).view(B * N, n)
    return z, (y + res.double() if res is not None else y)


@pytest.mark.parametrize("B,N,mode", [(256, 80, 2), (128, 80, 4), (100, 72, 1), (250, 66, 3), (320, 64, 2), (330, 48, 3), (256, 21, 2),
                                      (170, 32, 1), (200, 17, 0), (336, 40, 4)])
def test_split_gemm_groupnorm_block(B, N, mode):
    """Block.forward in one launch on the split path: every conditioning mode, scene lengths of every RB class (17..80), the saved
    pre-activation, residual; against f64 and next to the exact-f32 kernel.  Batches are large enough for the dispatcher to take
    the split path (>= 160 blocks): 8-wave tiles at 256 scenes of 80, the 4-wave tile at 100 .. 128 scenes."""
    from diffuscene_amd import ops
    M, n, k = B * N, 512, 512
    a, w, b = rnd(M, k, seed=11), rnd(n, k, seed=12, scale=0.08), rnd(n, seed=13)
    gamma, beta, res = rnd(n, seed=14) + 1.5, rnd(n, seed=15), rnd(M, n, seed=16)
    rows = {0: 1, 1: M, 2: B, 3: N, 4: 1000}[mode]
    ss = rnd(rows, 2 * n, seed=17, scale=0.3) if mode else None
    idx = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(3)) if mode == 4 else None
    d = dev()
    wd = w.to(d)
    (pl,) = ops.split_planes([(wd, None, False)])
    kw = dict(scale_shift=ss.to(d) if mode else None, ss_mode=mode, residual=res.to(d), ss_index=idx.to(d) if mode == 4 else None)
    pre, pre32 = torch.zeros(M, n, device=d), torch.zeros(M, n, device=d)
    y = ops.gemm_gn_silu(a.to(d), wd, b.to(d), gamma.to(d), beta.to(d), N, preact=pre, w_planes=pl, **kw)
    y32 = ops.gemm_gn_silu(a.to(d), wd, b.to(d), gamma.to(d), beta.to(d), N, preact=pre32, **kw)
    z, ref = _gn_ref(a, w, b, gamma, beta, N, ss, mode, res, idx)
    assert rel(pre, z) < 2e-6 and rel(y, ref) < 5e-6, (rel(pre, z), rel(y, ref))
    assert rms_err(y, ref) <= max(1.5 * rms_err(y32, ref), 2.5e-7), (rms_err(y, ref), rms_err(y32, ref))
    assert torch.equal(pre, pre32) != split_on(), "dispatch: the split path must take this launch (and only without DSC_GEMM=f32)"


@pytest.mark.parametrize("mode", [4, 2, 0])
def test_four_wave_and_eight_wave_tiles_are_bit_identical(mode):
    """The long real-reference chains (tests/golden/chain_split.npz) run at B = 128, where the dispatcher picks the FOUR-wave tiles
    (GroupNorm <true,2,2,5>, dense 160x128); the benchmark's B = 256 runs the EIGHT-wave tiles (<true,2,4,5>, 160x256).  Same rows
    through both: every output element sees the same K order and the same product order, the GroupNorm cell is one wave either way
    -> bit-identical results, so what the B = 128 chains pin transfers to the tile the benchmark times.  (A B = 256 chain of the real
    reference is held directly as well: test_gpu_chain_split.py::test_two_hundred_step_chain_at_b256.)"""
    from diffuscene_amd import _lib, ops
    if not split_on():
        pytest.skip("exact-f32 arithmetic selected")
    B, N, n = 256, 80, 512
    d = dev()
    for k1, k2 in ((512, 0), (512, 512)):
        M = B * N
        a, a2 = rnd(M, k1, seed=31).to(d), (rnd(M, k2, seed=32).to(d) if k2 else None)
        w, b = rnd(n, k1 + k2, seed=33, scale=0.06).to(d), rnd(n, seed=34).to(d)
        gamma, beta, res = (rnd(n, seed=35) + 1.5).to(d), rnd(n, seed=36).to(d), rnd(M, n, seed=37).to(d)
        (pl,) = ops.split_planes([(w, None, False)])
        idx = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(5)).to(d)
        ss = {4: rnd(1000, 2 * n, seed=38, scale=0.3), 2: rnd(B, 2 * n, seed=38, scale=0.3), 0: None}[mode]
        ss = ss.to(d) if ss is not None else None
        h = M // 2

        def gn(rows, scenes):
            sl = slice(0, rows)
            kw = dict(scale_shift=None, ss_mode=0)
            if mode == 4:
                kw = dict(scale_shift=ss, ss_mode=4, ss_index=idx[:scenes].contiguous())
            elif mode == 2:
                kw = dict(scale_shift=ss[:scenes], ss_mode=2)
            g = ops.make_gemm_args(a[sl], w, torch.empty(rows, n, device=d), b, a2[sl] if k2 else None, res[sl], gamma=gamma, beta=beta,
                                   tokens_per_scene=N, w_planes=pl, **kw)
            tile = _lib.fn("dsc_gemm_split_tile")(g, 1)
            y = ops.gemm_gn_silu(a[sl], w, b, gamma, beta, N, a2=a2[sl] if k2 else None, residual=res[sl], w_planes=pl, **kw)
            return tile, y

        prev = _lib.set_split_wave(False)
        try:
            t8, y8 = gn(M, B)
            t4, y4 = gn(h, B // 2)
            _lib.set_split_wave(True)                     # round 6: the wave-autonomous kernel takes the B = 256 launch by default
            tw, yw = gn(M, B)
        finally:
            _lib.set_split_wave(prev)
        assert (t8, t4, tw) == (_lib.TILE_GN_80_W8, _lib.TILE_GN_80_W4, _lib.TILE_WAVE_GN), (t8, t4, tw)
        assert torch.equal(y8[:h], y4), "GroupNorm GEMM: the 4-wave and the 8-wave tile differ"
        assert torch.equal(y8, yw), "GroupNorm GEMM: the wave-autonomous kernel and the 8-wave tile differ"
        if mode == 0:
            def plain(rows):
                sl = slice(0, rows)
                out = torch.empty(rows, n, device=d)
                g = ops.make_gemm_args(a[sl], w, out, b, a2[sl] if k2 else None, res[sl], w_planes=pl)
                tile = _lib.fn("dsc_gemm_split_tile")(g, 0)
                ops.run_gemm(g)
                return tile, out
            prev = _lib.set_split_wave(False)
            try:
                p8, z8 = plain(M)
                p4, z4 = plain(h)
                _lib.set_split_wave(True)
                pw, zw = plain(M)
            finally:
                _lib.set_split_wave(prev)
            assert (p8, p4, pw) == (_lib.TILE_160x256, _lib.TILE_160x128_W4, _lib.TILE_WAVE_DENSE), (p8, p4, pw)
            assert torch.equal(z8[:h], z4), "dense GEMM: the 4-wave and the 8-wave tile differ"
            assert torch.equal(z8, zw), "dense GEMM: the wave-autonomous kernel and the 8-wave tile differ"


def test_split_path_falls_back_where_it_does_not_apply():
    """Shapes the split kernel does not cover (n not a multiple of 128, unaligned output slices, a handful of rows, scenes of <= 16
    or > 80 tokens) run the exact-f32 kernel: same results as without planes, no error."""
    from diffuscene_amd import ops
    d = dev()
    a, w, b = rnd(300, 512, seed=1).to(d), rnd(128, 512, seed=2, scale=0.1).to(d), rnd(128, seed=3).to(d)
    (pl,) = ops.split_planes([(w, None, False)])
    out = torch.zeros(300, 200, device=d)
    y1 = ops.gemm(a, w, b, out=out[:, 3:131], w_planes=pl).clone()         # unaligned column offset
    # (same output alignment on both sides: an aligned launch of this size may run the K-parallel exact-f32 kernel of round 6, whose K sum
    # is associated differently from the tile kernel an unaligned output stays on -- tests/test_gpu_skinny.py compares those two)
    assert torch.equal(y1, ops.gemm(a, w, b, out=torch.zeros(300, 200, device=d)[:, 3:131]))
    assert (y1 - ops.gemm(a, w, b)).abs().max() <= 5e-6 * y1.abs().max()
    assert torch.equal(ops.gemm(a[:100], w, b, w_planes=pl), ops.gemm(a[:100], w, b))      # < 256 rows
    for N in (12, 96):
        M = 8 * N
        x = rnd(M, 512, seed=5).to(d)
        w5, b5, g5, be5 = rnd(512, 512, seed=6, scale=0.1).to(d), rnd(512, seed=7).to(d), (rnd(512, seed=8) + 1.5).to(d), rnd(512, seed=9).to(d)
        (p5,) = ops.split_planes([(w5, None, False)])
        assert torch.equal(ops.gemm_gn_silu(x, w5, b5, g5, be5, N, w_planes=p5), ops.gemm_gn_silu(x, w5, b5, g5, be5, N))


# ---------------------------------------------------------------------------------------------------------------------
# operand range of the split arithmetic (the contract written in include/diffuscene_hip.h next to dsc_gemm_args.w_planes)
# ---------------------------------------------------------------------------------------------------------------------
def _both(a, w, b=None):
    """(split result, exact-f32 result, launch was taken by the split kernel)."""
    from diffuscene_amd import ops
    ad, wd = a.to(dev()), w.to(dev())
    bd = b.to(dev()) if b is not None else None
    (pl,) = ops.split_planes([(wd, None, False)])
    y = ops.gemm(ad, wd, bd, w_planes=pl)
    y32 = ops.gemm(ad, wd, bd)
    return y, y32, ops.gemm_uses_split(ops.make_gemm_args(ad, wd, y, bd, w_planes=pl))


@pytest.mark.parametrize("sa,sw", [(1e-15, 1e-15), (1e15, 1e15), (1e30, 1e-30), (1e-30, 1e30), (1e-18, 1e18), (1e18, 1e18), (1e-19, 1e-19)])
def test_split_product_is_scale_free(sa, sw):
    """bf16 pieces keep the f32 exponent: the six-product sum is as accurate at 1e-30 / 1e+30 operand magnitudes as at 1 (products
    from 1e-38 to 1e+36), measured against f64 and against the exact-f32 kernel on the same operands."""
    m, n, k = 20480, 512, 512
    a, w = rnd(m, k, seed=21) * sa, rnd(n, k, seed=22) * sw
    y, y32, taken = _both(a, w)
    assert taken == split_on()
    ref = a.double() @ w.double().T
    assert bool(torch.isfinite(y).all())
    assert rel(y, ref) < 2e-6, rel(y, ref)
    assert rms_err(y, ref) <= max(1.5 * rms_err(y32, ref), 2.5e-7), (rms_err(y, ref), rms_err(y32, ref))


def test_split_product_mixed_magnitudes_inside_a_k_row():
    """Columns of A and W scaled by 10^U(-6,6) with opposite exponents (every product is O(1), every OPERAND row spans 12 decades) and,
    second case, uncorrelated exponents (a few products dominate each sum): error vs f64 in the f32 kernel's class either way."""
    m, n, k = 20480, 512, 512
    g = torch.Generator().manual_seed(5)
    e = (torch.rand(k, generator=g) * 12 - 6)
    for mirrored in (True, False):
        ew = -e if mirrored else (torch.rand(k, generator=g) * 12 - 6)
        a, w = rnd(m, k, seed=23) * (10.0 ** e)[None, :], rnd(n, k, seed=24) * (10.0 ** ew)[None, :]
        y, y32, taken = _both(a, w)
        assert taken == split_on()
        ref = a.double() @ w.double().T
        assert rel(y, ref) < 2e-6, (mirrored, rel(y, ref))
        assert rms_err(y, ref) <= max(1.5 * rms_err(y32, ref), 2.5e-7), (mirrored, rms_err(y, ref), rms_err(y32, ref))


def test_split_product_large_finite_and_subnormal_operands():
    """Up to the largest bf16 (3.3895e38) an operand splits finitely: rows holding +-3.3e38 against weights of 1e-3 give the f32
    product.  Subnormal operands (|x| < 1.18e-38) and third pieces below the bf16 subnormal range may be flushed by the matrix cores:
    the absolute error they can cause is bounded by 2^-16 of the flushed terms, far below one ulp of any normal-range result."""
    m, n, k = 20480, 512, 512
    a, w = rnd(m, k, seed=25), rnd(n, k, seed=26) * 1e-3
    a[::7, ::5] = 3.3e38
    a[3::7, 1::5] = -3.3e38
    y, y32, taken = _both(a, w)
    assert taken == split_on()
    ref = a.double() @ w.double().T
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(y32).all())
    assert rel(y, ref) < 2e-6
    # subnormal and near-subnormal operands next to normal ones: result = normal part +- negligible
    a2, w2 = rnd(m, k, seed=27), rnd(n, k, seed=28)
    a2[:, ::3] *= 1e-40                               # subnormal f32
    a2[:, 1::3] *= 1e-35                              # normal, third piece below 1e-40
    y, y32, _ = _both(a2, w2)
    ref = a2.double() @ w2.double().T
    assert rel(y, ref) < 2e-6 and rel(y32, ref) < 2e-6
    # an all-tiny problem: operands 1e-25 -> products 1e-50 underflow to zero in BOTH arithmetics (f32 range, not a split property)
    y, y32, _ = _both(rnd(m, k, seed=29) * 1e-25, rnd(n, k, seed=30) * 1e-25)
    assert float(y.abs().max()) == 0.0 and float(y32.abs().max()) == 0.0


def test_split_product_non_finite_operands_stay_non_finite_where_f32_is():
    """+-inf / NaN operands and operands above the largest bf16: the outputs they reach are non-finite in BOTH arithmetics (the split
    kernel gives NaN where the exact-f32 kernel may give +-inf: inf - bf16(inf) = NaN in the residual pieces -- documented in
    include/diffuscene_hip.h), every other output is untouched; products that overflow f32 are non-finite in both."""
    m, n, k = 20480, 512, 512
    a, w = rnd(m, k, seed=31), rnd(n, k, seed=32)
    a[5, 17] = float("inf")
    a[6, 18] = float("-inf")
    a[7, 19] = float("nan")
    a[8, 20] = 3.4e38                                 # finite f32 above the largest bf16: first piece rounds to inf
    w[9, 21] = float("inf")
    w[10, 22] = float("nan")
    y, y32, taken = _both(a, w)
    assert taken == split_on()
    bad_rows = torch.zeros(m, dtype=torch.bool)
    bad_rows[[5, 6, 7]] = True
    bad_cols = torch.zeros(n, dtype=torch.bool)
    bad_cols[[9, 10]] = True
    want_bad = bad_rows[:, None] | bad_cols[None, :]
    nf, nf32 = ~torch.isfinite(y).cpu(), ~torch.isfinite(y32).cpu()
    assert torch.equal(nf32, want_bad)                                        # the exact-f32 kernel: exactly the reached outputs
    if split_on():
        want_split = want_bad.clone()
        want_split[8, :] = True                                               # 3.4e38 > bf16 max: documented NaN row
        assert torch.equal(nf, want_split)
    ok = ~(want_bad | (torch.arange(m) == 8)[:, None])
    ref = a.double() @ w.double().T
    assert float(((y.double().cpu() - ref)[ok]).abs().max() / ref[ok].abs().max()) < 2e-6
    # overflow of the PRODUCT (1e30 * 1e30): non-finite in both
    a3, w3 = rnd(512, k, seed=33) * 1e30, rnd(n, k, seed=34) * 1e30
    a3 = a3.repeat(40, 1)
    y, y32, _ = _both(a3, w3)
    assert not bool(torch.isfinite(y).any()) or not split_on()
    assert float(torch.isfinite(y32).float().mean()) < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# training-step epilogues of the plain split GEMM (round 4): pre-activation stored next to act(u); result multiplied by act'(x)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("m,n,k", [(20480, 1024, 512), (5376, 512, 1024), (10240, 512, 512)])
def test_split_gemm_training_epilogues(m, n, k, act):
    """(a) Linear + GELU / SiLU in one launch, the pre-activation kept for the backward: u bit-identical to the plain product, y
    bit-identical to dsc_activation_f32(u); (b) the input-gradient GEMM applying the derivative of the consumer's activation,
    y = (dY . W) * act'(x) + residual: the product followed by dsc_activation_bwd_f32 and an add, to one rounding; both
    against f64.  With the exact-f32 arithmetic selected these launches are REJECTED (DSC_EINVAL), never run
    without their epilogue."""
    from diffuscene_amd import _lib, ops
    d = dev()
    a, w, b = rnd(m, k, seed=41).to(d), rnd(n, k, seed=42, scale=0.08).to(d), rnd(n, seed=43).to(d)
    (pl,) = ops.split_planes([(w, None, False)])
    u_ref = ops.gemm(a, w, b, w_planes=pl)
    y, u = torch.empty(m, n, device=d), torch.empty(m, n, device=d)
    g = ops.make_gemm_args(a, w, y, b, act_out=act, preact=u, w_planes=pl)
    assert ops.gemm_uses_split(g) == split_on()
    if not split_on():
        with pytest.raises(RuntimeError):
            ops.run_gemm(g)
        return
    ops.run_gemm(g)
    assert torch.equal(u, u_ref)
    assert torch.equal(y, ops.activation(u_ref, act))
    z = a.double() @ w.double().T + b.double()
    fz = F.gelu(z) if act == 1 else F.silu(z)
    assert rel(u, z) < 2e-6 and rel(y, fz) < 2e-6
    # (b) derivative epilogue: x = the saved pre-activation of an [m, n] activation, here u itself
    res = rnd(m, n, seed=44).to(d)
    prod = ops.gemm(a, w, None, w_planes=pl)
    want = ops.activation_bwd(u, prod, act) + res
    out = torch.empty(m, n, device=d)
    g2 = ops.make_gemm_args(a, w, out, None, residual=res, act_out=act, actgrad_x=u, w_planes=pl)
    ops.run_gemm(g2)
    assert rel(out, want) < 2e-7          # (one rounding apart at most: the epilogue may contract product * act' + residual into an FMA)
    zd = z.clone().requires_grad_(True)
    (F.gelu(zd) if act == 1 else F.silu(zd)).sum().backward()
    ref = (a.double() @ w.double().T) * zd.grad + res.double()
    assert rel(out, ref) < 3e-6, rel(out, ref)
    # accumulate in place (residual == y), as the plan's multi-consumer gradients do
    out2 = res.clone()
    ops.run_gemm(ops.make_gemm_args(a, w, out2, None, residual=out2, act_out=act, actgrad_x=u, w_planes=pl))
    assert torch.equal(out2, out)


def test_training_epilogues_are_rejected_on_the_exact_f32_kernel():
    """A launch that asks for an activation epilogue and does not qualify for the split kernel (no planes / too few rows / exact-f32
    arithmetic selected) fails with DSC_EINVAL."""
    from diffuscene_amd import _lib, ops
    d = dev()
    a, w = rnd(300, 512, seed=45).to(d), rnd(512, 512, seed=46, scale=0.1).to(d)
    (pl,) = ops.split_planes([(w, None, False)])
    y, u = torch.empty(300, 512, device=d), torch.empty(300, 512, device=d)
    with pytest.raises(RuntimeError):
        ops.run_gemm(ops.make_gemm_args(a, w, y, None, act_out=1, preact=u, w_planes=pl))          # 300 rows: too few blocks
    with pytest.raises(RuntimeError):
        ops.run_gemm(ops.make_gemm_args(a, w, y, None, act_out=1, actgrad_x=u))                    # no planes
    prev = _lib.set_gemm_arithmetic("f32")
    try:
        big = rnd(20480, 512, seed=47).to(d)
        yb, ub = torch.empty(20480, 512, device=d), torch.empty(20480, 512, device=d)
        with pytest.raises(RuntimeError):
            ops.run_gemm(ops.make_gemm_args(big, w, yb, None, act_out=2, preact=ub, w_planes=pl))
    finally:
        _lib.set_gemm_arithmetic(prev)
