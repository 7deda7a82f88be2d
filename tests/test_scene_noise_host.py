"""Per-scene seeds on the host: the numpy definition of the noise (diffuscene_amd/scene_noise.py) against the published Philox4x32-10
known answers and its first moments, the two new C symbols, ``ops.scene_seeds`` on every accepted form and every refusal, and -- over the
recording fakes of tools/trace_eager_loops.py, which run the eager loops on the CPU -- the (stream, draw) sequence a SceneNoise issues in
each of the twelve eager loops, and what ``batch_seeds`` / ``honour_batch_seeds`` / ``scene_seeds`` do to the wrapper's trace."""
import contextlib
import io
import json
import os
import re
import runpy
import sys

import numpy as np
import pytest
import torch

from oracle import weights as W
from oracle.make_golden_wrapper import network_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsc_scene_randn_f32", "dsc_scene_philox_u32")
QUIET = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731


# ------------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox4x32_10_reproduces_the_published_known_answers(counter, key, want):
    from diffuscene_amd.scene_noise import philox4x32_10
    got = philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert " ".join("%08x" % v for v in got) == want


def test_the_counter_layout_and_the_batched_form_are_the_scalar_one():
    """philox_words(seed, stream, draw, count)[e] is word e & 3 of the block (e >> 2, stream, draw lo, draw hi) under (seed lo, seed hi)."""
    from diffuscene_amd.scene_noise import philox4x32_10, philox_words
    seed, stream, draw = 2 ** 63 - 1, 1, 2 ** 32 + 5
    w = philox_words(seed, stream, draw, 11)
    assert w.shape == (11,) and w.dtype == np.uint32
    for e in (0, 3, 4, 10):
        block = philox4x32_10(np.array([e >> 2, 1, 5, 1], dtype=np.uint64), np.array([0xffffffff, 0x7fffffff], dtype=np.uint64))
        assert w[e] == block[e & 3]
    assert np.array_equal(philox_words(seed, stream, draw, 1365)[:11], w)              # e does not depend on the count


def test_moments_of_the_reference_normals():
    """Each statistic within five standard errors: n = 2**22 gives the bounds 2.4e-3, 3.5e-3, 2.4e-2, 2.4e-3."""
    from diffuscene_amd.scene_noise import reference_normals
    n = 2 ** 22
    z = reference_normals(1234, 0, 0, n)
    assert z.dtype == np.float64 and z.shape == (n,) and np.isfinite(z).all()
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2 - 3.0
    lag1 = (z[:-1] * z[1:]).mean()
    print("mean %.3g var-1 %.3g excess kurtosis %.3g lag-1 %.3g" % (mean, var - 1, kurt, lag1))
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(kurt) < 5 * np.sqrt(96 / n)
    assert abs(lag1) < 5 / np.sqrt(n)


def test_float32_is_the_float64_definition_up_to_rounding_and_never_infinite():
    from diffuscene_amd.scene_noise import normals_from_words, reference_normals
    z64, z32 = reference_normals(7, 1, 3, 2 ** 16), reference_normals(7, 1, 3, 2 ** 16, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32.astype(np.float64) - z64).max() < 1e-4
    assert np.array_equal(reference_normals(7, 1, 3, 5), z64[:5])                     # a prefix: e alone indexes the stream
    # the edge words: u == 2**-25 (the largest rho) and, in float32, u rounded to 1 (rho == 0): finite either way
    edge = np.array([0, 0, 0xffffffff, 0xffffffff, 0xffffffff, 0, 0, 0xffffffff], dtype=np.uint32)
    for dt in (np.float32, np.float64):
        z = normals_from_words(edge, dt)
        assert np.isfinite(z).all() and np.abs(z).max() < 6.0


# ------------------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_library_exports_the_new_symbols():
    from diffuscene_amd import _lib, ops, sampler, scene_noise
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dsc_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, "%s not declared in include/diffuscene_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), "%s not exported / bound" % name
    for name in ("scene_randn", "scene_philox", "scene_seeds"):
        assert callable(getattr(ops, name))
    assert callable(scene_noise.SceneNoise) and sampler.SEEDED == "seeded"


def test_the_launchers_check_their_arguments_before_any_launch():
    """Null pointers, negative counts and a stream beyond 32 bits: DSC_EINVAL (-1); an empty draw: 0 and no launch (no device here);
    per_scene beyond 2**32 or a grid beyond 2**31 - 1 blocks: DSC_ERANGE (-3)."""
    from diffuscene_amd import _lib
    p = 4096                                                                          # any non-null address: never dereferenced on the host
    for name in NEW_SYMBOLS:
        f = _lib.fn(name)
        assert f(None, p, p, 0, 1, 4, None) == -1 and f(p, None, p, 0, 1, 4, None) == -1 and f(p, p, None, 0, 1, 4, None) == -1
        assert f(p, p, p, -1, 1, 4, None) == -1 and f(p, p, p, 2 ** 32, 1, 4, None) == -1
        assert f(p, p, p, 0, -1, 4, None) == -1 and f(p, p, p, 0, 1, -4, None) == -1
        assert f(p, p, p, 0, 0, 4, None) == 0 and f(p, p, p, 1, 3, 0, None) == 0
        assert f(p, p, p, 0, 1, 2 ** 32 + 1, None) == -3 and f(p, p, p, 0, 2 ** 40, 2 ** 32, None) == -3


# ------------------------------------------------------------------------------------------------------------------- ops.scene_seeds
def test_scene_seeds_normalises_every_accepted_form():
    from diffuscene_amd import ops
    big = 2 ** 63 - 1
    for value, want in (([0, 1, 2], [0, 1, 2]), ((5, 5, 5), [5, 5, 5]), (range(3), [0, 1, 2]), (range(7, 10), [7, 8, 9]),
                        ([0, 2 ** 32, big], [0, 2 ** 32, big]), (np.array([3, 1, 2]), [3, 1, 2]), (np.arange(3, dtype=np.int32), [0, 1, 2]),
                        ([np.int64(4), np.uint8(1), 2], [4, 1, 2]), (torch.tensor([9, 8, 7]), [9, 8, 7]),
                        (torch.arange(3, dtype=torch.int32), [0, 1, 2]), (torch.tensor([big, 0, 1]), [big, 0, 1])):
        out = ops.scene_seeds(value, 3, "cpu")
        assert out.dtype == torch.int64 and tuple(out.shape) == (3,) and out.is_contiguous()
        assert out.tolist() == want, (value, out)
    assert ops.scene_seeds(torch.arange(4, 5), 1, "cpu").tolist() == [4]              # what the reference's call sites pass
    assert ops.scene_seeds([], 0, "cpu").tolist() == []


@pytest.mark.parametrize("bad", [[True, False, True], torch.tensor([True, False, True]), [0.0, 1.0, 2.0], [0, 1.5, 2], torch.zeros(3),
                                 np.zeros(3), [0, 1], [0, 1, 2, 3], torch.arange(2), torch.zeros(3, 1, dtype=torch.int64), [-1, 0, 1],
                                 [0, 1, 2 ** 63], torch.tensor([0, -5, 1]), np.array([0, 1, 2 ** 63], dtype=np.uint64), None, 7, "abc",
                                 ["a", "b", "c"], [[0], [1], [2]], [None, 0, 1], np.array([True, False, True])])
def test_scene_seeds_refuses_everything_else(bad):
    from diffuscene_amd import ops
    with pytest.raises(ValueError, match="scene_seeds"):
        ops.scene_seeds(bad, 3, "cpu")


# ------------------------------------------------------------------------------------------------------------------- the eager loops
_PATCHED = ("p_sample", "ddim_step", "ddim_advance", "cfg_combine", "complete_overwrite", "complete_overwrite_ragged", "masked_overwrite")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    """tools/trace_eager_loops.py, run in this process: its recording fakes stay installed over ``ops`` and GaussianDiffusion.tables for
    this module's tests and are taken out again afterwards.  -> the tool's globals (EV, rec, denoise, the loop inputs)."""
    from diffuscene_amd import ops
    from diffuscene_amd.networks import diffusion_ddpm as D
    saved = {n: getattr(ops, n) for n in _PATCHED}
    saved_tables, argv, path = D.GaussianDiffusion.tables, sys.argv, list(sys.path)
    out = tmp_path_factory.mktemp("trace") / "eager.json"
    try:
        sys.argv = ["trace_eager_loops.py", ROOT, str(out)]
        with QUIET():
            g = runpy.run_path(os.path.join(ROOT, "tools", "trace_eager_loops.py"))
        sys.argv = argv
        real = ops.scene_randn

        def scene_randn(seeds, draw, stream, shape, out=None):
            g["rec"]("scene_randn", seeds.tolist(), int(stream), int(draw), tuple(shape))
            gen = torch.Generator().manual_seed(int(draw) * 2 + int(stream))
            return torch.randn(tuple(shape), generator=gen) + seeds.float()[:, None, None]
        ops.scene_randn = scene_randn
        yield g
        ops.scene_randn = real
    finally:
        sys.argv, sys.path[:] = argv, path
        D.GaussianDiffusion.tables = saved_tables
        for n, f in saved.items():
            setattr(ops, n, f)


def _events(g, fn):
    ev = g["EV"]
    n0 = len(ev)
    with QUIET():
        res = fn()
    got = [list(e) for e in ev[n0:]]
    del ev[n0:]
    return got, res


def _draws(events):
    return [(e[2], e[3], e[4]) for e in events if e[0] == "scene_randn"]


def _gd(g, T):
    D = g["D"]
    return D.GaussianDiffusion(g["cfg"], D.get_betas("linear", 1e-4, 0.02, T), "mse", "v", "fixedsmall", False, False, None)


def test_scene_noise_issues_the_documented_stream_and_draw_numbers_in_every_eager_loop(tool):
    from diffuscene_amd.scene_noise import SceneNoise
    g = tool
    B, N, C = g["shape"]
    shape, cond, cross, given, mask, denoise = g["shape"], g["cond"], g["cross"], g["given"], g["mask"], g["denoise"]
    sub = (B, N, 5)                                                                    # translation + angle: the arrange loops
    T, S = 3, 3
    nf = SceneNoise([11, 22], "cpu")
    free_t = lambda sh: [(0, k, sh) for k in range(T + 1)]                                                          # noqa: E731
    free_s = lambda sh: [(0, k, sh) for k in range(S)]                                                              # noqa: E731
    given_t = lambda gs: [(0, 0, shape)] + [d for k in range(T) for d in ((1, k, gs), (0, k + 1, shape))]           # noqa: E731
    given_s = lambda gs: [(0, 0, shape)] + [d for k in range(S) for d in ((1, k, gs), (0, k + 1, shape))][:-1]      # noqa: E731
    kw = dict(sampling_timesteps=S, ddim_sampling_eta=0.5)
    loops = [
        ("p_sample_loop", T, lambda gd: gd.p_sample_loop(denoise, shape, "cpu", cond, None, noise_fn=nf), free_t(shape)),
        ("trajectory", T, lambda gd: gd.p_sample_loop_trajectory(denoise, shape, "cpu", 2, cond, None, noise_fn=nf), free_t(shape)),
        ("guided", T, lambda gd: gd.p_sample_loop_guided(denoise, shape, "cpu", cond, cross, 2.0, noise_fn=nf), free_t(shape)),
        ("arrange", T, lambda gd: gd.p_sample_loop_arrange(denoise, shape, "cpu", cond, None, noise_fn=nf, input_boxes=given), free_t(sub)),
        ("dense", T, lambda gd: gd.p_sample_loop_complete(denoise, shape, "cpu", cond, None, noise_fn=nf, partial_boxes=given[:, :2]),
         given_t((B, 2, C))),
        ("ragged", T, lambda gd: gd.p_sample_loop_complete_ragged(denoise, shape, "cpu", cond, None, noise_fn=nf, partial_boxes=given[:, :4],
                                                                   num_partial=[0, 3]), given_t((B, 4, C))),
        ("ragged pmax=N", T, lambda gd: gd.p_sample_loop_complete_ragged(denoise, shape, "cpu", cond, None, noise_fn=nf, partial_boxes=given,
                                                                          num_partial=[2, N]), given_t(shape)),
        ("masked", T, lambda gd: gd.p_sample_loop_masked(denoise, shape, "cpu", cond, None, noise_fn=nf, known=given, mask=mask),
         given_t(shape)),
        ("ddim", 20, lambda gd: gd.ddim_sample_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, **kw), free_s(shape)),
        ("ddim all", 20, lambda gd: gd.ddim_sample_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, return_all_timesteps=True, **kw),
         free_s(shape)),
        ("guided ddim", 20, lambda gd: gd.ddim_guided_loop(denoise, shape, "cpu", cond, cross, (0.0, 3.0), noise_fn=nf, **kw), free_s(shape)),
        ("arrange ddim", 20, lambda gd: gd.ddim_arrange_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, input_boxes=given, **kw), free_s(sub)),
        ("ragged ddim", 20, lambda gd: gd.ddim_complete_ragged_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, partial_boxes=given[:, :4],
                                                                     num_partial=[0, 3], **kw), given_s((B, 4, C))),
        ("masked ddim", 20, lambda gd: gd.ddim_masked_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, known=given, mask=mask, **kw),
         given_s(shape)),
    ]
    for name, steps, fn, want in loops:                                                 # ONE SceneNoise: every loop re-arms it
        gd = _gd(g, steps)
        ev, _ = _events(g, lambda: fn(gd))
        assert _draws(ev) == want, name
        assert all(e[1] == [11, 22] for e in ev if e[0] == "scene_randn")
        assert not any(e[0] == "draw" for e in ev)
    with pytest.raises(ValueError, match="2 seeds"):
        _gd(g, T).p_sample_loop(denoise, (3, N, C), "cpu", None, None, noise_fn=nf)


def _wrapper(g, tmp_path):
    """The unconditional wrapper on the CPU over the tool's fakes: T = 3, the tool's denoiser in place of the HIP one."""
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    cfg = network_config("uncond", str(stats), 20)
    with QUIET():
        m = DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, None, cfg)
    m.diffusion._denoise = g["denoise"]
    m.diffusion.diffusion.num_timesteps = 3                                            # the loops' step count; the tables keep 20 rows
    m.diffusion.diffusion.tables("cpu")                                                # the one upload: not an event of a later run
    m.delete_empty_per_scene = lambda samples, keep_empty=False: samples               # its compaction is a device kernel
    m.delete_empty_from_network_samples = lambda samples, device="cpu", keep_empty=False: samples
    return m.eval()


def test_batch_seeds_is_ignored_unless_honoured_and_then_it_is_scene_seeds(tool, tmp_path):
    g = tool
    m = _wrapper(g, tmp_path)
    N, C = 12, int(m.config["point_dim"])
    room = torch.zeros(2, 1, 64, 64)

    def run(fn, **kw):
        torch.manual_seed(5)
        ev, res = _events(g, lambda: fn(room, N, C, batch_size=2, **kw))
        return ev, res, torch.get_rng_state()

    assert type(m).honour_batch_seeds is False
    for fn, extra in ((m.sample, {}), (m.generate_layout, {}), (m.generate_layout_batched, {}),
                      (m.generate_layout_batched, dict(sampling_timesteps=2, ddim_sampling_eta=0.5))):
        plain = run(fn, **extra)
        ignored = run(fn, batch_seeds=torch.arange(2), **extra)
        assert ignored[0] == plain[0] and torch.equal(ignored[1], plain[1]) and torch.equal(ignored[2], plain[2])
        assert not _draws(plain[0])
        seeded = run(fn, scene_seeds=range(2), **extra)
        assert _draws(seeded[0]) and all(e[1] == [0, 1] for e in seeded[0] if e[0] == "scene_randn")
        assert [e for e in seeded[0] if e[0] != "scene_randn"] == plain[0]              # the same launches around other noise
        torch.manual_seed(5)
        torch.randn((2, N, C))
        assert torch.equal(seeded[2], torch.get_rng_state())                            # sample()'s CPU draw is kept, and is the only one
        m.honour_batch_seeds = True
        try:
            honoured = run(fn, batch_seeds=torch.arange(2), **extra)
            still_plain = run(fn, **extra)                                              # batch_seeds=None: nothing to honour
            both = run(fn, batch_seeds=torch.arange(2), scene_seeds=[1, 0], **extra)    # scene_seeds wins
        finally:
            del m.honour_batch_seeds
        assert honoured[0] == seeded[0] and torch.equal(honoured[1], seeded[1])
        assert still_plain[0] == plain[0] and torch.equal(still_plain[1], plain[1])
        assert all(e[1] == [1, 0] for e in both[0] if e[0] == "scene_randn")
    # bad seeds are refused before anything is drawn or computed
    torch.manual_seed(5)
    state = torch.get_rng_state()
    n0 = len(g["EV"])
    for bad in ([0], [0, 1, 2], [0.5, 1.0], [True, False], [-1, 0], 3):
        for fn in (m.sample, m.generate_layout, m.generate_layout_batched, m.generate_layout_progressive):
            with pytest.raises(ValueError, match="scene_seeds"):
                fn(room, N, C, batch_size=2, scene_seeds=bad)
    assert torch.equal(torch.get_rng_state(), state) and len(g["EV"]) == n0


def test_every_entry_point_takes_the_keyword():
    import inspect
    from diffuscene_amd.networks.diffusion_scene_layout_ddpm import DiffusionSceneLayout_DDPM as M
    for name in ("sample", "generate_layout", "generate_layout_progressive", "generate_layout_batched", "complete_scene", "arrange_scene",
                 "complete_scene_batched", "arrange_scene_batched", "inpaint_scene_batched"):
        p = inspect.signature(getattr(M, name)).parameters
        assert p["scene_seeds"].default is None and p["batch_seeds"].default is None, name
