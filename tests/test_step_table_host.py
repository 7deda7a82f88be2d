"""The two tables the sampling stack is laid out from, on the host: ops.STEP_ENTRY -- (strided, given, guided) -> entry point and
parameter order, what ops.step_rec marshals by -- against the bound signatures and the independent statement of
tests/test_step_args_host.py; and the spec each public loop of GaussianDiffusion hands to its dispatcher against the front end of
sampler.py that the method called when each was written out.  No device."""
import ctypes

import pytest
import torch

from test_step_args_host import ENTRY_POINTS

# public loop -> the captured loop it hands over to
FRONT_ENDS = {"p_sample_loop": "graph_sample_loop", "p_sample_loop_complete": "graph_sample_loop", "p_sample_loop_arrange": "graph_sample_loop",
              "ddim_sample_loop": "graph_ddim_sample_loop", "ddim_arrange_loop": "graph_ddim_sample_loop",
              "p_sample_loop_complete_ragged": "graph_complete_ragged_loop", "ddim_complete_ragged_loop": "graph_ddim_complete_ragged_loop",
              "p_sample_loop_masked": "graph_masked_loop", "ddim_masked_loop": "graph_ddim_masked_loop",
              "p_sample_loop_guided": "graph_guided_loop", "ddim_guided_loop": "graph_ddim_guided_loop",
              "p_sample_loop_masked_guided": "graph_masked_guided_loop", "ddim_masked_guided_loop": "graph_ddim_masked_guided_loop"}


def test_the_step_table_holds_ten_bound_entry_points_in_the_order_of_the_header():
    from diffuscene_amd import _lib, ops
    assert set(ops.STEP_ENTRY) == {(s, g, c) for s in (False, True) for g in (None, "rows", "mask") for c in (False, True)} \
        - {(False, "rows", True), (True, "rows", True)}
    names = [name for name, _ in ops.STEP_ENTRY.values()]
    assert len(set(names)) == 10 and set(names) == {n for n in ENTRY_POINTS if "overwrite" not in n}
    for (strided, given, guided), (name, params) in ops.STEP_ENTRY.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(params) + 1 == len(argtypes), name                           # + the stream
        assert params == [a.rstrip("?") for a in ENTRY_POINTS[name].split()], name
        assert ("S" in params) == strided and ("scale" in params) == guided, name
        assert ("counts" in params, "mask" in params) == (given == "rows", given == "mask"), name
        for p, ty in zip(params, argtypes):                                     # sizes and flags are ints, everything else a pointer
            assert (ty is ctypes.c_void_p) == (p not in ("mean_type", "clip", "b", "inner", "n", "pmax", "c", "S", "T")), (name, p)


@pytest.mark.parametrize("strided", [False, True])
def test_guided_completion_has_no_kernel_and_says_so(strided):
    from diffuscene_amd import ops
    x = torch.zeros(2, 3, 4)
    time = dict(strided=(x, x, x, x), tables=(x,) * 4) if strided else dict(t=x, tables=(x,) * 5)
    with pytest.raises(ValueError, match="given=rows, guided=True"):            # refused before any operand is looked at
        ops.step_rec(x, x, x, x, 0, rows=(x, x, x), q=(x, x), scale=x, **time)
    with pytest.raises(ValueError, match="given=rows and mask"):
        ops.step_rec(x, x, x, x, 0, rows=(x, x, x), mask=(x, x, x), q=(x, x), **time)
    with pytest.raises(ValueError, match="takes no x_dup"):
        ops.step_rec(x, x, x, x, 0, x_dup=x, **time)
    with pytest.raises(ValueError, match="takes no x0_out"):
        ops.step_rec(x, x, x, x, 0, mask=(x, x, x), q=(x, x), x0_out=x, **time)


def test_every_public_loop_hands_its_spec_to_the_front_end_it_called_before(monkeypatch, capsys):
    from diffuscene_amd import sampler
    from diffuscene_amd.networks import diffusion_ddpm as dd
    seen = []

    def record(self, what, denoise_fn, shape, device, condition, condition_cross, noise_fn, graph, strided=None, given=None, scale=None,
               **kw):
        seen.append((what, dd.front_end_name(strided is not None, given and given[0], scale is not None)))
        return torch.zeros(shape)
    monkeypatch.setattr(dd.GaussianDiffusion, "_loop", record)
    gd = object.__new__(dd.GaussianDiffusion)
    gd.num_timesteps, gd.betas = 1000, [0.0] * 1000
    gd.translation_dim, gd.size_dim, gd.angle_dim, gd.bbox_dim = 3, 3, 2, 8
    shape = (1, 2, 10)
    x = torch.zeros(shape)
    extra = {"guided": dict(guidance_scale=2.0), "complete": dict(partial_boxes=x[:, :1]), "ragged": dict(num_partial=[1]),
             "masked": dict(known=x, mask=x > 0), "arrange": dict(input_boxes=x)}
    for loop, front in FRONT_ENDS.items():
        kw = {k: v for key, d in extra.items() if key in loop for k, v in d.items()}
        getattr(gd, loop)(None, shape, "cpu", None, None, **kw)
        what, name = seen.pop()
        assert not seen and name == front and callable(getattr(sampler, name)), (loop, name)
        assert what == (loop if loop != "ddim_arrange_loop" else "ddim_sample_loop")
    assert set(FRONT_ENDS.values()) == {n for n in vars(sampler) if n.startswith("graph_") and n.endswith("_loop")}
    assert len(set(FRONT_ENDS.values())) == 10
