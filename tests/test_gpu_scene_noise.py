"""GPU: per-scene seeds.

The kernel (dsc_scene_randn_f32 / dsc_scene_philox_u32) over per_scene in {1, 3, 4, 5, 744, 1365} x B in {1, 3, 67} x stream in {0, 1} x
draw in {0, 1, 2**32 + 5}, seeds including 0, 1, 2**32 and 2**63 - 1: the raw words equal the numpy definition (scene_noise.py) exactly,
the normals lie within the bound below of its float64 evaluation, every row is the single-scene launch of its seed, permuted seeds give
permuted rows, e does not depend on per_scene, nothing is written past ``out`` (aligned and one element off: both store paths), and the
draw number is read from the device counter.
Bound for the normals: 4 x the largest distance of the float32 numpy evaluation from the float64 one over the words of these cases --
computed here, not fixed in advance: the device is another float32 evaluation of the same words (the same rounding of u and theta, its
own logf / sinf / cosf).  DSC_PARITY_LOG=<file> records the measured distances.

The loops, on the tiny text model of tests/test_gpu_sampler_core.py (C = 62) at B = 3, N = 12 (per_scene = 744: dwordx4 stores) and
N = 21 (per_scene = 1302: scene bases off the 16-byte grid, dword stores), T = 3 / S in {1, 3}: for each of the eight loop kinds seeded
captured == seeded eager (torch.equal), a repeat is equal (counters re-armed), other seeds reuse the graph and differ, the device
generator is untouched (also by the capturing call), permuted seeds and inputs give permuted scenes, and scene b is the batch_size = 1
call with its seed and its own inputs (for the ragged loops at its own Pmax) -- the last two at the chain criterion 1e-4 norm-relative
(tests/test_gpu_wide.py), the GEMM dispatch of another batch size being free to differ in the last bits."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_cfg import GC, build_model, case_texts  # noqa: E402
from test_gpu_complete_ragged import build_wrapper, dev, rnd  # noqa: E402
from tools.make_golden_cfg import distance  # noqa: E402

QUIET = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731
CHAIN = 1e-4


@pytest.fixture(autouse=True)
def no_device_errors():
    from diffuscene_amd import _lib
    _lib.device_error_count(reset=True)
    yield
    assert _lib.device_error_count(reset=True) == 0


def _log(line):
    print(line)
    if os.environ.get("DSC_PARITY_LOG"):
        with open(os.environ["DSC_PARITY_LOG"], "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------------------------- the kernel
PER_SCENE = (1, 3, 4, 5, 744, 1365)
BATCHES = (1, 3, 67)
STREAMS = (0, 1)
DRAWS = (0, 1, 2 ** 32 + 5)
PMAX = 1368                                                                           # whole quads covering the longest scene
SENTINEL, MARGIN = 12345.0, 64


def _seeds(b):
    """b seeds: the edge values first (all four from b = 4 on; b = 1 takes the largest), then spread-out ones."""
    edge = [2 ** 63 - 1, 0, 1, 2 ** 32]
    return (edge + [(i * 0x9E3779B97F4A7C15 + 12345) % 2 ** 63 for i in range(max(b - 4, 0))])[:b]


_REF = {}


def _ref(seed, stream, draw):
    """(words, float32 normals, float64 normals) of the first PMAX elements, computed once per (seed, stream, draw)."""
    from diffuscene_amd.scene_noise import normals_from_words, philox_words
    k = (seed, stream, draw)
    if k not in _REF:
        w = philox_words(seed, stream, draw, PMAX)
        _REF[k] = (w, normals_from_words(w, np.float32), normals_from_words(w, np.float64))
    return _REF[k]


def _bound():
    """4 x the float32-to-float64 distance of the host definition over every word the cases below draw."""
    worst = 0.0
    for seed in sorted(set(_seeds(67) + _seeds(3) + _seeds(1))):
        for stream in STREAMS:
            for draw in DRAWS:
                _, z32, z64 = _ref(seed, stream, draw)
                worst = max(worst, float(np.abs(z32.astype(np.float64) - z64).max()))
    return 4.0 * worst, worst


def _i64(v):
    return torch.tensor([v], dtype=torch.int64, device=dev())


def test_words_and_normals_are_the_host_definition_at_every_case():
    from diffuscene_amd import ops
    bound, host = _bound()
    assert 0 < bound < 1e-3
    worst = 0.0
    for b in BATCHES:
        seeds = _seeds(b)
        assert len(seeds) == b and len(set(seeds)) == b and (b < 4 or {0, 1, 2 ** 32, 2 ** 63 - 1} <= set(seeds))
        sd = torch.tensor(seeds, dtype=torch.int64, device=dev())
        for stream in STREAMS:
            for draw in DRAWS:
                d = _i64(draw)
                refs = [_ref(s, stream, draw) for s in seeds]
                for p in PER_SCENE:
                    words = ops.scene_philox(sd, d, stream, (b, p)).cpu()
                    want = torch.from_numpy(np.stack([r[0][:p] for r in refs]).view(np.int32))
                    assert torch.equal(words, want), (b, p, stream, draw)
                    z = ops.scene_randn(sd, d, stream, (b, p))
                    assert z.dtype == torch.float32 and tuple(z.shape) == (b, p) and bool(torch.isfinite(z).all())
                    dist = float(np.abs(z.cpu().numpy().astype(np.float64) - np.stack([r[2][:p] for r in refs])).max())
                    worst = max(worst, dist)
                    assert dist <= bound, (b, p, stream, draw, dist, bound)
                    assert int(d.item()) == draw                                        # the counter is read, never written
    _log("scene noise kernel: device normals vs float64 definition, max abs %.3g (host float32 %.3g, bound %.3g)" % (worst, host, bound))


def test_rows_are_single_scene_launches_and_permuted_seeds_permute_the_rows():
    from diffuscene_amd import ops
    for b in (3, 67):
        seeds = _seeds(b)
        sd = torch.tensor(seeds, dtype=torch.int64, device=dev())
        perm = list(reversed(range(b)))
        for stream, draw in ((0, 0), (1, 2 ** 32 + 5)):
            d = _i64(draw)
            for p in PER_SCENE:
                z = ops.scene_randn(sd, d, stream, (b, p))
                for row in (range(b) if b == 3 else (0, 33, 66)):
                    alone = ops.scene_randn(sd[row:row + 1].contiguous(), d, stream, (1, p))
                    assert torch.equal(alone[0], z[row]), (b, p, row)
                zp = ops.scene_randn(sd[perm].contiguous(), d, stream, (b, p))
                assert torch.equal(zp, z[perm]), (b, p)
                assert torch.equal(ops.scene_philox(sd[perm].contiguous(), d, stream, (b, p)), ops.scene_philox(sd, d, stream, (b, p))[perm])
        # a 3-d shape is its flattened scene: e = row * C + c
        assert torch.equal(ops.scene_randn(sd, d, 1, (b, 21, 65)).view(b, -1), ops.scene_randn(sd, d, 1, (b, 1365)))
    twice = torch.tensor([7, 7, 8], dtype=torch.int64, device=dev())                  # repeated seeds: identical scenes
    z = ops.scene_randn(twice, _i64(3), 0, (3, 744))
    assert torch.equal(z[0], z[1]) and not torch.equal(z[0], z[2])


def test_the_element_index_does_not_depend_on_the_scene_length():
    from diffuscene_amd import ops
    sd = torch.tensor(_seeds(67), dtype=torch.int64, device=dev())
    d = _i64(1)
    long, short = ops.scene_randn(sd, d, 1, (67, 1365)), ops.scene_randn(sd, d, 1, (67, 5))
    assert torch.equal(long[:, :5], short)
    assert torch.equal(ops.scene_randn(sd, d, 1, (67, 744))[:, :4], ops.scene_randn(sd, d, 1, (67, 4)))
    assert not torch.equal(ops.scene_randn(sd, d, 0, (67, 5)), short)                   # the stream enters
    assert not torch.equal(ops.scene_randn(sd, _i64(2), 1, (67, 5)), short)             # and the draw


@pytest.mark.parametrize("offset", [0, 1])
def test_nothing_is_written_outside_out(offset):
    """``out`` inside a sentinel-filled buffer, on a 16-byte boundary and one element past it (the dword path at every per_scene)."""
    from diffuscene_amd import ops
    for b in BATCHES:
        sd = torch.tensor(_seeds(b), dtype=torch.int64, device=dev())
        for p in PER_SCENE:
            n = b * p
            for op, dtype, fill in ((ops.scene_randn, torch.float32, SENTINEL), (None, torch.int32, 0x5A5A5A5A)):
                buf = torch.full((MARGIN + offset + n + MARGIN,), fill, dtype=dtype, device=dev())
                out = buf[MARGIN + offset:MARGIN + offset + n].view(b, p)
                assert out.data_ptr() % 16 == 4 * offset
                if op is None:
                    from diffuscene_amd import _lib
                    _lib.check(_lib.fn("dsc_scene_philox_u32")(out.data_ptr(), sd.data_ptr(), _i64(1).data_ptr(), 1, b, p, ops.stream_ptr()),
                               "dsc_scene_philox_u32")
                    want = ops.scene_philox(sd, _i64(1), 1, (b, p))
                else:
                    op(sd, _i64(1), 1, (b, p), out=out)
                    want = op(sd, _i64(1), 1, (b, p))
                assert torch.equal(out, want), (b, p, offset)
                assert bool((buf[:MARGIN + offset] == fill).all()) and bool((buf[MARGIN + offset + n:] == fill).all()), (b, p, offset)


def test_the_draw_number_comes_from_the_device_counter():
    from diffuscene_amd import ops
    sd = torch.tensor(_seeds(3), dtype=torch.int64, device=dev())
    d = _i64(0)
    first = ops.scene_randn(sd, d, 0, (3, 1365))
    ops.add_scalar_i64(d, 1)                                                           # what a captured step does between two replays
    second = ops.scene_randn(sd, d, 0, (3, 1365))
    assert not torch.equal(first, second)
    assert torch.equal(first, ops.scene_randn(sd, _i64(0), 0, (3, 1365))) and torch.equal(second, ops.scene_randn(sd, _i64(1), 0, (3, 1365)))
    d.fill_(2 ** 32 + 5)
    words = ops.scene_philox(sd, d, 0, (3, 8)).cpu()
    assert torch.equal(words, torch.from_numpy(np.stack([_ref(s, 0, 2 ** 32 + 5)[0][:8] for s in _seeds(3)]).view(np.int32)))


def test_argument_checks_on_the_device():
    from diffuscene_amd import ops
    sd = torch.tensor(_seeds(3), dtype=torch.int64, device=dev())
    assert tuple(ops.scene_randn(sd, _i64(0), 0, (3, 0)).shape) == (3, 0)              # nothing to draw: no launch
    for bad in (lambda: ops.scene_randn(sd, _i64(0), 0, (2, 4)), lambda: ops.scene_randn(sd.int(), _i64(0), 0, (3, 4)),
                lambda: ops.scene_randn(sd, torch.zeros(2, dtype=torch.int64, device=dev()), 0, (3, 4)),
                lambda: ops.scene_randn(sd.cpu(), _i64(0), 0, (3, 4)), lambda: ops.scene_randn(sd, _i64(0), 0, (3, 4), out=torch.empty(3, 5, device=dev()))):
        with pytest.raises(RuntimeError, match="diffuscene_amd"):
            bad()
    with pytest.raises(RuntimeError, match="DSC_EINVAL"):
        ops.scene_randn(sd, _i64(0), -1, (3, 4))


# ------------------------------------------------------------------------------------------------------------------- the loops
B, T, T_STRIDED = 3, 3, 50
SEEDS, OTHER = (5, 2 ** 32 + 1, 2 ** 63 - 1), (6, 0, 1)
COUNTS, SCALES = (0, 2, 5), (0.0, 1.5, 3.0)
PERM = [2, 0, 1]
#         entry point                      class                 strided
LOOPS = {"gen_samples": ("_StepGraph", False),
         "gen_samples_ddim": ("_DDIMGraph", True),
         "complete_samples_ragged": ("_RaggedCompleteGraph", False),
         "complete_samples_ragged_ddim": ("_DDIMCompleteGraph", True),
         "inpaint_samples": ("_MaskedGraph", False),
         "inpaint_samples_ddim": ("_DDIMMaskedGraph", True),
         "gen_samples_guided": ("_GuidedStepGraph", False),
         "gen_samples_guided_ddim": ("_DDIMGuidedGraph", True)}
CASES = [(loop, n, s) for loop, (_, strided) in LOOPS.items() for n in (12, 21) for s in ((1, 3) if strided else (None,))]
_INPUTS = {}


def _model(strided, n, tmp_path):
    return build_model("v", T_STRIDED if strided else T, tmp_path, tag="scene_seeds", sample_num_points=n)


def _inputs(m, n):
    """The master inputs of the B = 3 batch at N = n: conditions, given values, mask."""
    key = (id(m), n)
    if key not in _INPUTS:
        room = torch.zeros(B, 1, 64, 64, device=dev())
        with torch.no_grad(), QUIET():
            cond, cross = m._sampling_conditions(room, n, dev(), text=case_texts()[:B])
        _INPUTS[key] = (cond, cross, rnd(B, n, GC, seed=601).clamp(-1, 1).to(dev()), (rnd(B, n, GC, seed=602) > 0.3).to(dev()))
    return _INPUTS[key]


def _run(m, loop, n, idx, seeds, graph, S=None, pmax=5, mask=None):
    """``loop`` on the scenes ``idx`` of the master batch, in that order, under ``seeds``; ``mask``: another master mask."""
    from diffuscene_amd.scene_noise import SceneNoise
    cond, cross, given, own_mask = _inputs(m, n)
    mask = own_mask if mask is None else mask
    kw = dict(clip_denoised=True) if S is None else dict(sampling_timesteps=S, ddim_sampling_eta=0.5)
    if loop.startswith("complete"):
        kw.update(partial_boxes=given[idx, :pmax].contiguous(), num_partial=[COUNTS[i] for i in idx])
    elif loop.startswith("inpaint"):
        kw.update(known=given[idx], mask=mask[idx])
    elif "guided" in loop:
        kw.update(guidance_scale=tuple(SCALES[i] for i in idx))
    with torch.no_grad(), QUIET():
        return getattr(m.diffusion, loop)((len(idx), n, GC), dev(), condition=None if cond is None else cond[idx].contiguous(),
                                          condition_cross=cross[idx].contiguous(), noise_fn=SceneNoise(list(seeds), dev()), graph=graph, **kw)


def _rel(a, b):
    return distance(a.cpu(), b.cpu())[0]


@pytest.mark.parametrize("loop,n,S", CASES)
def test_seeded_loops(loop, n, S, tmp_path):
    cls, strided = LOOPS[loop]
    m = _model(strided, n, tmp_path)
    gd = m.diffusion.diffusion
    all3 = [0, 1, 2]
    torch.manual_seed(97)
    state = torch.cuda.get_rng_state(dev())
    gd._graphs.clear()
    eager = _run(m, loop, n, all3, SEEDS, False, S)
    first = _run(m, loop, n, all3, SEEDS, True, S)                                       # this call captures
    g = next(iter(gd._graphs.values()))
    assert type(g).__name__ == cls and g.mode == "seeded" and len(gd._graphs) == 1
    assert torch.equal(torch.cuda.get_rng_state(dev()), state)                          # no draw from the device generator, capture included
    assert torch.equal(first, eager), (loop, n, S, float((first - eager).abs().max()))
    assert bool(torch.isfinite(first).all())
    again = _run(m, loop, n, all3, SEEDS, True, S)
    assert torch.equal(again, first)                                                    # the draw counters start over
    other = _run(m, loop, n, all3, OTHER, True, S)
    assert next(iter(gd._graphs.values())) is g and not torch.equal(other, first)       # seeds are no part of the cache key
    assert torch.equal(_run(m, loop, n, all3, OTHER, False, S), other)
    permuted = _run(m, loop, n, PERM, [SEEDS[i] for i in PERM], True, S)
    worst_perm = _rel(permuted, first[PERM])
    worst_alone = 0.0
    for b in all3:
        alone = _run(m, loop, n, [b], [SEEDS[b]], True, S, pmax=max(COUNTS[b], 1))      # the ragged loops: at the scene's own Pmax
        worst_alone = max(worst_alone, _rel(alone, first[b:b + 1]))
        if loop.startswith("complete"):
            assert torch.equal(alone[0, :COUNTS[b]], _inputs(m, n)[2][b, :COUNTS[b]])   # the given rows, restored
    assert torch.equal(torch.cuda.get_rng_state(dev()), state)
    _log("seeded %s N=%d S=%s: permuted batch norm-relative %.3g, batch_size 1 norm-relative %.3g" % (loop, n, S, worst_perm, worst_alone))
    assert worst_perm < CHAIN and worst_alone < CHAIN
    # the scenes differ from one another far beyond the criterion: it can tell a wrong seed or a wrong row
    assert _rel(first[1:2], first[0:1]) > 100 * CHAIN


@pytest.mark.parametrize("n", [12, 21])
@pytest.mark.parametrize("S", [None, 3])
def test_a_prefix_mask_is_the_ragged_completion_bit_for_bit_and_counts_do_not_leak(n, S, tmp_path):
    """complete_samples_ragged[_ddim] with counts (0, 2, 5) at Pmax = 5 against inpaint_samples[_ddim] with the whole-row prefix mask,
    under the same seeds: torch.equal (the given stream's element index is row * C + c in both); scene 1 against the same scene run
    alone with counts (2,) at Pmax = 2: the chain criterion."""
    m = _model(S is not None, n, tmp_path)
    sfx = "" if S is None else "_ddim"
    ragged = _run(m, "complete_samples_ragged" + sfx, n, [0, 1, 2], SEEDS, True, S)
    rows = torch.arange(n, device=dev())[None, :, None] < torch.tensor(COUNTS, device=dev())[:, None, None]
    for graph in (True, False):
        masked = _run(m, "inpaint_samples" + sfx, n, [0, 1, 2], SEEDS, graph, S, mask=rows.expand(B, n, GC))
        assert torch.equal(masked, ragged), (n, S, graph, float((masked - ragged).abs().max()))
    alone = _run(m, "complete_samples_ragged" + sfx, n, [1], [SEEDS[1]], True, S, pmax=2)
    r = _rel(alone, ragged[1:2])
    _log("seeded ragged completion N=%d S=%s: scene 1 of counts (0, 2, 5) vs alone with counts (2,), norm-relative %.3g" % (n, S, r))
    assert r < CHAIN


def test_the_wrapper_keywords(tmp_path):
    """generate_layout_batched(scene_seeds=range(3)) scene by scene against generate_layout with batch_seeds=arange(i, i + 1) once
    ``honour_batch_seeds`` is set -- what the reference's scripts pass --, ignored batch_seeds, and the completion / in-painting entry
    points under seeds."""
    n = 12
    m = _model(False, n, tmp_path)
    texts = case_texts()[:B]
    room = torch.zeros(B, 1, 64, 64, device=dev())
    given = _inputs(m, n)[2]
    with torch.no_grad(), QUIET():
        batched = m.generate_layout_batched(room, n, GC, B, text=texts, scene_seeds=range(B), keep_empty=True, clip_denoised=True)
        assert len(batched) == B
        torch.manual_seed(3)
        plain = m.generate_layout(room[:1], n, GC, batch_size=1, text=texts[:1], keep_empty=True)
        torch.manual_seed(3)
        ignored = m.generate_layout(room[:1], n, GC, batch_size=1, text=texts[:1], keep_empty=True, batch_seeds=torch.arange(0, 1))
        assert all(torch.equal(plain[k], ignored[k]) for k in plain)
        m.honour_batch_seeds = True
        try:
            worst = 0.0
            for i in range(B):
                one = m.generate_layout(room[:1], n, GC, batch_size=1, text=texts[i:i + 1], keep_empty=True, clip_denoised=True,
                                        batch_seeds=torch.arange(i, i + 1))
                assert sorted(one) == sorted(batched[i])
                worst = max(worst, max(_rel(one[k], batched[i][k]) for k in one))
        finally:
            del m.honour_batch_seeds
        _log("generate_layout_batched(scene_seeds=range(3)) vs per-scene honoured batch_seeds: norm-relative %.3g" % worst)
        assert worst < CHAIN
        state = torch.cuda.get_rng_state(dev())
        un, _ = build_wrapper("uncond", tmp_path, time_num=T)                           # completion: a model without text
        runs = [un.complete_scene_batched(room, n, GC, [given[0, :2], given[1, :0], given[2, :5]], scene_seeds=s, keep_empty=True)
                for s in ((1, 2, 3), (1, 2, 3), (1, 2, 4))]
        runs += [m.inpaint_scene_batched(room, n, GC, given, m.attribute_mask([1, 0, 3], ("sizes", "class_labels"), B, n), text=texts,
                                         scene_seeds=s, keep_empty=True, sampling_timesteps=2, ddim_sampling_eta=1.0)
                 for s in ((1, 2, 3), (1, 2, 3), (1, 2, 4))]
        assert torch.equal(torch.cuda.get_rng_state(dev()), state)
    for same, again, other in (runs[:3], runs[3:]):
        for b in range(B):
            assert all(torch.equal(same[b][k], again[b][k]) for k in same[b])
        assert not all(torch.equal(same[2][k], other[2][k]) for k in same[2])           # the scene whose seed changed
    with pytest.raises(ValueError, match="scene_seeds"):
        m.generate_layout_batched(room, n, GC, B, text=texts, scene_seeds=[0, 1])
