"""Every forward kernel of csrc/blocks.hip against the float64 statements of oracle/blocks_ref.py, one entry point and one
dispatch branch at a time, at the smallest shapes at which each can still go wrong (tests/test_gpu_ops.py sees them dense, freshly
allocated and at product shapes, under one whole-tensor bound).  Launches go through the ops.* wrappers with out=.

The conventions are those of tests/test_gpu_train_kernels.py, whose Case, bounded and unit helpers are imported: every input with a
leading dimension is a column slice of a wider tensor, every output a slice of a wider tensor that holds NaN where the kernel must
write and 7.5 everywhere else; after each launch the owned elements are finite, the sentinel elements and the inputs bit-unchanged.
Every launch gets valid arguments only, except in the one refusals test.  Copies, LeakyReLU, the identity and table rows are
compared EXACTLY.  Everything else is held, per output tensor, to
    err = max over units ( max|got - ref64| / max|ref64| over the unit )  <=  max(4 * err_torch32, FLOOR),  FLOOR = 64 * 2^-24
where a unit is what one block or wave computes -- a weight row, a token row, a (scene, head) slab, the whole tensor for the
activations -- and err_torch32 is the same distance for the oracle evaluated in float32 on the CPU.  A unit whose float64 reference
vanishes (weight standardisation of one column, a constant row) is compared absolutely: |got| <= FLOOR * max|input|.  Every measured
err is printed and goes to $DSC_PARITY_LOG when it is set.  tests/test_blocks_ref_host.py asserts, on the CPU, what this module
assumes of its inputs.

FLOORS lists the output tensors whose floor is not the default one, with the measurement and the arithmetic that causes it; no floor
exceeds the tolerance tests/test_gpu_ops.py applies to the same operation (CAPS)."""
import numpy as np
import pytest
import torch

from oracle import blocks_ref as B
from test_gpu_train_kernels import DEV, F32, F64, FLOOR, SENT, Case, bits, bounded, check_all, exact, host, rows_, slabs, whole

pytestmark = pytest.mark.gpu

CAPS = {"weight_standardize": 2e-6, "layernorm": 2e-6, "linear_smallk": 2e-6, "linear_smallk_grouped": 2e-6, "attention": 3e-6,
        "linear_attention": 3e-6, "time_embedding": 5e-4}
# (entry point, tensor) -> raised floor = 2 x the worst err measured over this module's cases on the MI355X.  None is needed: the
# polynomial erf of dsc_gelu (worst err 4.2e-8) and the device sinf / cosf at 1500 rad (5.1e-8) stay far below the default floor, and
# the largest err under it is 1.1e-6 (attention, n = 128).
FLOORS = {}


def lib():
    from diffuscene_amd import _lib, ops
    return _lib, ops


def held(entry, tensor, case, got, ref64, t32, units=whole, scale=1.0):
    return bounded(entry, tensor, case, got, ref64, t32, units, scale, prefix="blocks_fwd", caps=CAPS, floors=FLOORS)


def sync():
    torch.cuda.synchronize()


def amax(*arrays):
    return float(max(np.abs(a).max() for a in arrays))


# ================================================================================================ dsc_attention_f32
def run_attention(scenes, n, large=False):
    _, ops = lib()
    d = B.attention_case(scenes, n, large)
    c = Case()
    qkv = c.inp(np.concatenate([d["q"], d["k"], d["v"]], 1))
    out = c.out(scenes * n, 128)
    assert qkv.stride(0) > 384 and out.stride(0) > 128
    ops.attention(qkv[:, :128], qkv[:, 128:256], qkv[:, 256:], scenes, n, B.SCALE, out=out)
    sync()
    case = "B%d n%d%s" % (scenes, n, " q x%g" % B.LARGE if large else "")
    c.check("attention " + case)
    a = (d["q"], d["k"], d["v"], scenes, n, B.SCALE)
    check_all([held("attention", "out", case, out, B.attention(*a, dtype=F64), B.attention(*a, dtype=F32), slabs(scenes, n), amax(d["v"]))])


@pytest.mark.parametrize("scenes,n", B.ATTN_N)
def test_attention(scenes, n):
    """dsc_attention_f32, attention_kernel: both sides of every block-size switch of dsc_attention_threads (256 threads up to 64, 320
    to 80, 384 to 96, 448 to 112, 512 above), of the second pass over the queries (128 | 129), one and two tokens, the largest scene;
    q | k | v column blocks of one buffer."""
    run_attention(scenes, n)


@pytest.mark.parametrize("scenes,n", B.ATTN_LARGE)
def test_attention_large_logits(scenes, n):
    """q scaled by 30: logits beyond 89, nearly one-hot rows; the row maximum must be the maximum over ALL keys, in the first pass
    (n = 17) and in the second (n = 129)"""
    run_attention(scenes, n, large=True)


# ================================================================================================ dsc_linear_attention_f32
def run_linear_attention(scenes, nq, nk, large=False):
    _, ops = lib()
    d = B.linear_attention_case(scenes, nq, nk, large)
    c = Case()
    if nq == nk:                                                    # self form: q | k | v slices of one buffer
        qkv = c.inp(np.concatenate([d["q"], d["k"], d["v"]], 1))
        q, k, v = qkv[:, :128], qkv[:, 128:256], qkv[:, 256:]
    else:                                                           # cross form: k | v slices of a [B nk, 256] buffer
        q = c.inp(d["q"])
        kv = c.inp(np.concatenate([d["k"], d["v"]], 1))
        k, v = kv[:, :128], kv[:, 128:]
    out = c.out(scenes * nq, 128)
    ops.linear_attention(q, k, v, scenes, nq, nk, B.SCALE, out=out)
    sync()
    case = "B%d nq%d nk%d%s" % (scenes, nq, nk, " q,k x%g" % B.LARGE if large else "")
    c.check("linear_attention " + case)
    a = (d["q"], d["k"], d["v"], scenes, nq, nk, B.SCALE)
    check_all([held("linear_attention", "out", case, out, B.linear_attention(*a, dtype=F64), B.linear_attention(*a, dtype=F32),
                    slabs(scenes, nq), amax(d["v"]))])


@pytest.mark.parametrize("scenes,nq,nk", B.LINATTN)
def test_linear_attention(scenes, nq, nk):
    """dsc_linear_attention_f32, linear_attention_kernel: one key, fewer keys than the 8 lanes of a channel and no multiple of them, nq
    on either side of the 64-query pass and of two passes (128 | 129), nq != nk with both above 64, three scenes, the largest scene;
    self form (nq = nk) and cross form."""
    run_linear_attention(scenes, nq, nk)


@pytest.mark.parametrize("scenes,nq,nk", B.LINATTN_LARGE)
def test_linear_attention_large_logits(scenes, nq, nk):
    """q and k scaled by 30: exp overflows unless the maximum of k is taken over all 8 lanes of a channel (and every token: nk = 9 leaves
    one lane with two) and that of q over the 4 lanes of a token"""
    run_linear_attention(scenes, nq, nk, large=True)


# ================================================================================================ dsc_layernorm_f32
def run_layernorm(m, with_residual, kind="random"):
    _, ops = lib()
    d = B.layernorm_case(m, kind)
    c = Case()
    x, g = c.inp(d["x"], 4, 4), c.inp(d["g"])
    res = c.inp(d["residual"], 8, 4) if with_residual else None
    y = c.out(m, B.C, 8, 8)
    lds = {t.stride(0) for t in (x, res, y) if t is not None}
    assert len(lds) == (3 if with_residual else 2) and all(ld % 4 == 0 for ld in lds)
    assert all(t.data_ptr() % 16 == 0 for t in (x, g, res, y) if t is not None)
    ops.layernorm(x, g, residual=res, out=y)
    sync()
    case = "m%d %s%s" % (m, kind, " residual" if with_residual else "")
    c.check("layernorm " + case)
    r = d["residual"] if with_residual else None
    ref = B.layernorm(d["x"], d["g"], r, dtype=F64)
    res_ = [held("layernorm", "y", case, y, ref, B.layernorm(d["x"], d["g"], r, dtype=F32), rows_, amax(d["x"]))]
    if kind == "constant":                                          # the normalised row vanishes: y = residual, or 0
        row = host(y)[B.ln_const_row(m)].astype(np.float64)
        want = d["residual"][B.ln_const_row(m)].astype(np.float64) if with_residual else 0.0
        assert np.abs(row - want).max() <= FLOOR * amax(d["x"]), "constant row: %g" % np.abs(row - want).max()
    check_all(res_)


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("m", B.LN_M)
def test_layernorm(m, with_residual):
    """dsc_layernorm_f32, layernorm512_kernel (one wave per row, four rows per block): one row, both sides of one block (3, 4, 5), three
    blocks; x, residual and y with three different leading dimensions"""
    run_layernorm(m, with_residual)


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("m,kind", B.LN_EDGES)
def test_layernorm_numerical_edges(m, kind, with_residual):
    """x = 50 +- 0.01 (the variance of a row whose mean dwarfs its spread), and one constant row among random ones (variance 0)"""
    run_layernorm(m, with_residual, kind)


# ================================================================================================ dsc_weight_standardize_f32
def run_ws(shapes, kind, what):
    _, ops = lib()
    c = Case()
    ws = B.ws_case(shapes, kind)
    sizes = [r * cc for r, cc in shapes]
    w = [v.view(s) for v, s in zip(c.pool(sizes, fill=ws), shapes)]
    o = [v.view(s) for v, s in zip(c.pool(sizes), shapes)]
    ops.weight_standardize(w, outs=o)
    sync()
    c.check("weight_standardize " + what)
    check_all([held("weight_standardize", "out", "%s item %d %dx%d" % (what, i, *shapes[i]), o[i], B.weight_standardize(a, dtype=F64),
                    B.weight_standardize(a, dtype=F32), rows_, amax(a)) for i, a in enumerate(ws)])


@pytest.mark.parametrize("rows,cols", B.WS_SINGLE)
def test_weight_standardize_single_items(rows, cols):
    """dsc_weight_standardize_f32, ws_kernel: one column (the reference vanishes), both sides of one element per thread (256) and of
    the eight a thread can hold (2048); the sentinel behind the last row catches a store at c = cols"""
    run_ws([(rows, cols)], "random", "single")


@pytest.mark.parametrize("cols", B.WS_EDGE_COLS)
def test_weight_standardize_constant_and_shifted_rows(cols):
    """row 0 constant (variance 0, rs = eps^-1/2, output 0), row 1 = 100 +- 0.01"""
    run_ws([(3, cols)], "edges", "edges")


def test_weight_standardize_ragged_row_counts_in_one_launch():
    """one launch whose grid has 70 rows: items of 1, 2, 3 and 7 rows next to two of 70, as runs of one pool -- a block past an item's
    own rows must not write (the next item's NaN run and the sentinel gaps lie behind it)"""
    _lib, _ = lib()
    assert len(B.WS_RAGGED) <= _lib.WS_MAX and (1, 5) in B.WS_RAGGED and (70, 256) in B.WS_RAGGED
    run_ws(B.WS_RAGGED, "random", "ragged")


def test_weight_standardize_more_items_than_one_launch_holds():
    """WS_MAX + 3 matrices in one ops.weight_standardize call: the wrapper issues two launches, every item is written once"""
    _lib, _ = lib()
    run_ws(B.ws_chunked_shapes(_lib.WS_MAX), "random", "chunked")


# ================================================================================================ dsc_linear_smallk_f32
def smallk_operands(c, d, with_bias, right=None):
    """x at column offset 1 of an odd-width buffer, w strided, bias a slice"""
    k = d["x"].shape[1]
    x = c.inp(d["x"], 1, 2 + k % 2 if right is None else right)
    assert x.stride(0) % 2 == 1 and x.storage_offset() == 1
    return x, c.inp(d["w"]), (c.inp(d["bias"]) if with_bias else None)


def run_smallk(m, k_in, n, act, with_bias):
    _, ops = lib()
    d = B.smallk_case(m, k_in, n)
    c = Case()
    x, w, bias = smallk_operands(c, d, with_bias)
    y = c.out(m, n, 3, 2)
    ops.linear_smallk(x, w, bias, act_out=B.ACTS[act], out=y)
    sync()
    case = "m%d k%d n%d %s%s" % (m, k_in, n, act, " bias" if with_bias else "")
    c.check("linear_smallk " + case)
    a = (d["x"], d["w"], d["bias"] if with_bias else None, B.ACTS[act])
    check_all([held("linear_smallk", "y", case, y, B.linear_smallk(*a, dtype=F64), B.linear_smallk(*a, dtype=F32), rows_,
                    amax(d["x"]) * amax(d["w"]))])


@pytest.mark.parametrize("m,k_in", B.SMALLK_CROSS)
def test_linear_smallk_depth_and_token_block(m, k_in):
    """dsc_linear_smallk_f32: k_in on both sides of the 8-wide weight prefetch (7, 8, 9) and at its last full group (63, 64), one input
    column; m on both sides of the 32-token block; n = 257 leaves one channel to the second trip of the 256-thread stride"""
    run_smallk(m, k_in, B.SMALLK_N, "gelu", True)


@pytest.mark.parametrize("n,act,with_bias", B.SMALLK_WIDTHS)
def test_linear_smallk_widths_activations_bias(n, act, with_bias):
    """n on both sides of the 256-thread stride, one channel, two full trips; each activation once; with and without bias"""
    run_smallk(33, 9, n, act, with_bias)


# ================================================================================================ dsc_linear_smallk_grouped_f32
def test_linear_smallk_grouped_items_equal_their_single_launches():
    """SMALLK_MAX items of different depth in one launch, outputs adjacent column blocks of one buffer: each bit-equal to its single
    launch and within the bound of the oracle"""
    _lib, ops = lib()
    assert len(B.SMALLK_GROUP_K) == _lib.SMALLK_MAX
    m, n = 33, B.SMALLK_N
    ds = [B.smallk_case(m, k, n, seed=i) for i, k in enumerate(B.SMALLK_GROUP_K)]
    c = Case()
    xbuf = c.inp(np.concatenate([d["x"] for d in ds], 1), 1, 2)
    assert xbuf.stride(0) % 2 == 1
    offs = np.cumsum([0] + B.SMALLK_GROUP_K)
    xs = [xbuf[:, offs[i]:offs[i + 1]] for i in range(len(ds))]
    ws, bs = [c.inp(d["w"]) for d in ds], [c.inp(d["bias"]) for d in ds]
    wide = c.out(m, n * len(ds))
    outs = [wide[:, i * n:(i + 1) * n] for i in range(len(ds))]
    ops.linear_smallk_grouped(xs, ws, bs, outs, act_out=B.ACT_GELU)
    singles = [c.out(m, n) for _ in ds]
    for x, w, b, y in zip(xs, ws, bs, singles):
        ops.linear_smallk(x, w, b, act_out=B.ACT_GELU, out=y)
    sync()
    c.check("linear_smallk_grouped")
    res = []
    for i, d in enumerate(ds):
        assert exact(outs[i], host(singles[i])), "item %d differs from its single launch" % i
        a = (d["x"], d["w"], d["bias"], B.ACT_GELU)
        res.append(held("linear_smallk_grouped", "y", "item %d k%d" % (i, B.SMALLK_GROUP_K[i]), outs[i], B.linear_smallk(*a, dtype=F64),
                        B.linear_smallk(*a, dtype=F32), rows_, amax(d["x"]) * amax(d["w"])))
    check_all(res)


# ================================================================================================ dsc_gather_columns_f32
GATHER = {"one span": (5, 40, 30, [(3, 7, 11)]),
          "four spans with gaps": (7, 100, 70, [(0, 1, 8), (32, 12, 25), (64, 37, 31), (96, 69, 1)]),
          "one row": (1, 100, 70, [(90, 0, 10), (0, 20, 3), (50, 40, 30)]),
          "covering": (9, 96, 65, [(0, 0, 8), (32, 8, 25), (64, 33, 32)]),
          "grid stride": (2049, 300, 270, [(0, 2, 8), (32, 12, 25), (64, 40, 32), (100, 75, 191)])}


@pytest.mark.parametrize("name", sorted(GATHER))
def test_gather_columns(name):
    """dsc_gather_columns_f32: one span and SMALLK_MAX spans, spans that leave gaps in the destination (the gaps keep their sentinel),
    one row, spans that cover the destination, and rows * total = 2049 * 256, one row more than the 2048 blocks of 256 threads hold
    (the grid stride); bit-equal to the slice copies"""
    _lib, ops = lib()
    rows, sw, dw, spans = GATHER[name]
    assert len(spans) <= _lib.SMALLK_MAX and (name != "grid stride" or rows * sum(w for _, _, w in spans) == 2048 * 256 + 256)
    src_h = B.noise((rows, sw), rows + sw)
    init = np.full((rows, dw), SENT, np.float32)
    for _, dc, w in spans:
        assert np.all(init[:, dc:dc + w] == SENT) and dc + w <= dw
        init[:, dc:dc + w] = np.nan
    c = Case()
    src = c.inp(src_h, 3, 2)
    dst = c.out(rows, dw, 5, 2, init=init)
    big, own = c.outs[-1]
    own[1:1 + rows, 5:5 + dw] = np.isnan(init)                      # the gaps belong to the sentinels
    assert (name == "covering") == bool(np.isnan(init).all())
    ops.gather_columns(dst, src, spans)
    sync()
    c.check("gather_columns " + name)
    got = host(dst)
    for sc, dc, w in spans:
        assert exact(got[:, dc:dc + w], src_h[:, sc:sc + w]), (name, sc, dc, w)


# ================================================================================================ dsc_activation_f32
@pytest.mark.parametrize("count", B.ACT_COUNTS)
@pytest.mark.parametrize("name", sorted(B.ACTS))
def test_activation(name, count):
    """dsc_activation_f32: identity and LeakyReLU(0.1) bit-equal; GELU (polynomial erf) and SiLU (expf and a division) bounded over the
    whole tensor, over the part without the special points (whose maximum of 90 would otherwise set the scale), and absolutely at
    the special points 0, +-1e-4, +-30, +-90; one thread, both sides of a block, and the grid-stride above 4096 blocks"""
    _, ops = lib()
    xh = B.activation_case(count)
    c = Case()
    x, y = c.inp(xh), c.out1(count)
    ops.activation(x, B.ACTS[name], out=y)
    sync()
    c.check("activation %s %d" % (name, count))
    ref, t32 = B.activation(xh, B.ACTS[name], dtype=F64), B.activation(xh, B.ACTS[name], dtype=F32)
    if name in ("none", "leaky"):
        assert exact(y, t32.numpy())
        return
    got = host(y)
    k = min(count, len(B.ACT_FWD_SPECIALS))
    assert np.isfinite(got[:k]).all()
    gap = np.abs(got[:k].astype(np.float64) - ref.numpy()[:k]).max()
    assert gap <= FLOOR * amax(xh), "special points: %g" % gap
    res = [held("activation " + name, "y", "count %d" % count, got, ref, t32, whole, amax(xh))]
    if count > k:
        res.append(held("activation " + name, "y without specials", "count %d" % count, got[k:], ref[k:], t32[k:], whole, amax(xh[k:])))
    check_all(res)


# ================================================================================================ dsc_time_embedding_f32
@pytest.mark.parametrize("with_table", [True, False])
@pytest.mark.parametrize("dim", B.TIME_DIMS)
def test_time_embedding(dim, with_table):
    """dsc_time_embedding_f32: t = 0 and table_rows - 1 are bit-equal to their table rows (a table of noise: not to be mistaken for
    computed values); t = table_rows, 1500 and -3 take the computed path, as every t does without a table; dim = 2 (one frequency),
    6, and 512 (two trips of the 256 threads); per row against sin / cos of the same float32 argument"""
    _, ops = lib()
    d = B.time_case(dim)
    nt, rows = len(d["t"]), B.TIME_TABLE_ROWS
    c = Case()
    freq = c.inp(d["freq"])
    table = c.pool([rows * dim], fill=[d["table"]])[0].view(rows, dim) if with_table else None
    out = c.pool([nt * dim])[0].view(nt, dim)
    t = torch.from_numpy(d["t"]).to(DEV)
    ops.time_embedding(t, dim, table, freq, out=out)
    sync()
    case = "dim%d %s" % (dim, "table" if with_table else "no table")
    c.check("time_embedding " + case)
    assert np.array_equal(host(t), d["t"])
    ref, t32 = B.time_embedding(d["t"], dim, d["freq"], dtype=F64), B.time_embedding(d["t"], dim, d["freq"], dtype=F32)
    first = 0
    if with_table:
        assert exact(host(out)[:2], d["table"][[0, rows - 1]]), "rows inside the table are not the table's"
        first = 2
    check_all([held("time_embedding", "out", case, host(out)[first:], ref[first:], t32[first:], rows_)])


# ================================================================================================ refusals
def test_documented_refusals_return_before_any_launch():
    """Every entry point returns its error code from the host checks in front of its launch, and every canary stays as it was: d != 512
    (ERANGE), a misaligned x and an odd leading dimension (EALIGN) of dsc_layernorm_f32; n = 161 (ERANGE) and a misaligned q (EALIGN) of
    both attentions; cols = 2049 (ERANGE) of dsc_weight_standardize_f32; k_in = 65 (ERANGE) of dsc_linear_smallk_f32; a zero-width span
    (EINVAL) of dsc_gather_columns_f32; an odd dim (EINVAL) of dsc_time_embedding_f32."""
    _lib, ops = lib()
    EINVAL, EALIGN, ERANGE = -1, -2, -3

    def refused(c, rec, want, what):
        name, args, _ = rec
        rc = _lib.fn(name)(*args, ops.stream_ptr())
        sync()
        assert rc == want, "%s: %s returned %d, expected %d" % (what, name, rc, want)
        for big, before in c.ins:
            assert (bits(host(big)) == bits(before)).all(), "%s: an input changed" % what
        for big, own in c.outs:
            h = host(big)
            assert np.isnan(h[own]).all() and (bits(h[~own]) == bits(np.float32(SENT))).all(), "%s: %s wrote to an output" % (what, name)

    ones = lambda *s: np.ones(s, np.float32)
    # LayerNorm
    c = Case()
    refused(c, ops.layernorm_rec(c.inp(ones(4, 256)), c.inp(ones(256)), c.out(4, 256)), ERANGE, "LayerNorm d 256")
    c = Case()
    x = c.inp(ones(4, 512), 1, 3)
    assert x.data_ptr() % 16 == 4 and x.stride(0) % 4 == 0
    refused(c, ops.layernorm_rec(x, c.inp(ones(512)), c.out(4, 512)), EALIGN, "LayerNorm misaligned x")
    c = Case()
    x = c.inp(ones(4, 512), 4, 1)
    assert x.data_ptr() % 16 == 0 and x.stride(0) % 2 == 1
    refused(c, ops.layernorm_rec(x, c.inp(ones(512)), c.out(4, 512)), EALIGN, "LayerNorm odd ld")
    # attentions
    for which in ("attention", "linear_attention"):
        for n, left, want, what in ((161, 4, ERANGE, "n 161"), (8, 1, EALIGN, "misaligned q")):
            c = Case()
            q, k, v = c.inp(ones(n, 128), left, 8 - left), c.inp(ones(n, 128)), c.inp(ones(n, 128))
            assert q.data_ptr() % 16 == (0 if left == 4 else 4) and q.stride(0) % 4 == 0
            out = c.out(n, 128)
            rec = (ops.attention_rec(q, k, v, out, 1, n, 0.5) if which == "attention" else
                   ops.linear_attention_rec(q, k, v, out, 1, n, n, 0.5))
            refused(c, rec, want, which + " " + what)
    # weight standardisation
    c = Case()
    w, o = c.pool([2 * 2049], fill=[ones(2, 2049)])[0].view(2, 2049), c.pool([2 * 2049])[0].view(2, 2049)
    refused(c, ops.weight_standardize_rec([(w, o)]), ERANGE, "weight standardisation cols 2049")
    # small-K
    c = Case()
    refused(c, ops.linear_smallk_rec(c.inp(ones(3, 65)), c.inp(ones(5, 65)), c.inp(ones(5)), c.out(3, 5)), ERANGE, "small-K k_in 65")
    # gather
    c = Case()
    refused(c, ops.gather_columns_rec(c.out(3, 20), c.inp(ones(3, 20)), [(0, 0, 4), (8, 8, 0)]), EINVAL, "gather zero-width span")
    # time embedding
    c = Case()
    t = torch.zeros(2, dtype=torch.int64, device=DEV)
    refused(c, ops.time_embedding_rec(t, 5, None, c.inp(ones(2)), c.pool([10])[0].view(2, 5)), EINVAL, "time embedding odd dim")
