#!/usr/bin/env python
"""Canonical dump of every library call a captured sampling loop makes, to compare two trees launch for launch and argument for argument.

Wraps _lib.fn, then for each case calls the loop's front end in sampler three times in one process -- the first call builds the plans,
warms up and captures, the second and third run the cached graph -- and writes every call into the library in order, in the line format
of tools/launch_lists.py: pointer arguments as ``s<k>+<byte offset>``, k numbering the device allocations by first appearance in launch
order (the live blocks of the caching allocator: the draws and x_T of a loop are temporaries that no object keeps).  Replays of a
captured graph make no call; what a graph holds is what its capture recorded.

The cases: the ten loops and the dense-prefix completion behind complete_samples at B = 2, N = 12 on the text configuration -- three
steps for the T-step loops, S = 1 and S = 3 for the strided ones, ``fused`` both ways where the loop takes it, under each noise mode
(randn, replay, seeded).

    python tools/loop_launches.py OUTDIR

writes OUTDIR/<case>.txt and OUTDIR/SHA256SUMS.  Run it in two trees and compare the SHA256SUMS files.  Only names that both trees have
are used: the graph_*_loop front ends with their arguments of the day they were written."""
import gc
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from launch_lists import Storages, fmt_step  # noqa: E402
from diffuscene_amd import _lib, sampler  # noqa: E402
from diffuscene_amd.scene_noise import SceneNoise  # noqa: E402

B, STEPS, PMAX, ETA = 2, 3, 5, 0.5
MODES = ("randn", "replay", "seeded")
#       front end                          strided  given     guided  takes fused=
ROWS = [("graph_sample_loop",               False,  None,     False,  False),
        ("graph_sample_loop",               False,  "dense",  False,  False),
        ("graph_ddim_sample_loop",          True,   None,     False,  False),
        ("graph_complete_ragged_loop",      False,  "rows",   False,  True),
        ("graph_ddim_complete_ragged_loop", True,   "rows",   False,  True),
        ("graph_masked_loop",               False,  "mask",   False,  False),
        ("graph_ddim_masked_loop",          True,   "mask",   False,  False),
        ("graph_guided_loop",               False,  None,     True,   True),
        ("graph_ddim_guided_loop",          True,   None,     True,   True),
        ("graph_masked_guided_loop",        False,  "mask",   True,   True),
        ("graph_ddim_masked_guided_loop",   True,   "mask",   True,   True)]


class Blocks(Storages):
    """Storages over the live blocks of the caching allocator, looked up again whenever something was allocated or freed."""

    def __init__(self, device):
        super().__init__()
        self.device, self.version = device, None

    def refresh(self):
        stats = torch.cuda.memory_stats(self.device)
        version = (stats["allocation.all.allocated"], stats["allocation.all.freed"])
        if version == self.version:
            return
        self.version, self.spans = version, {}
        for seg in torch.cuda.memory_snapshot():
            at = seg["address"]
            for blk in seg["blocks"]:
                if blk["state"].startswith("active"):
                    self.spans[at] = blk["size"]
                at += blk["size"]
        self.bases = sorted(self.spans)

    def name(self, ptr, what):
        try:
            return super().name(ptr, what)
        except SystemExit:                          # not device memory of the allocator: no stable name, and no reason to stop a capture
            self.unknown += 1
            return "?"

    unknown = 0


def record_calls(lines, st):
    """_lib.fn hands out recording wrappers from here on (launch plans keep what it returns)."""
    real, wrapped = _lib.fn, {}

    def fn(name):
        if name not in wrapped:
            f = real(name)

            def call(*args):
                st.refresh()
                lines.append(fmt_step(name, args[:-1], st))
                return f(*args)
            call.__name__ = name
            wrapped[name] = call
        return wrapped[name]
    _lib.fn = fn
    return real


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def run_case(front, strided, given, guided, fused, S, mode, model, dev):
    """-> the text of one case."""
    spec = dict(bench.CONFIGS["text"], batch=B)
    shape, cond, cross, _, _ = bench.sampling_inputs(spec, model, dev, seed=0)
    _, N, C = shape
    dp, gd = model.diffusion, model.diffusion.diffusion
    steps = S if strided else STEPS
    head = [cond, cross]
    if guided:
        head = list(gd._guided_inputs(shape, dev, cond, cross, (0.0, 3.0), front))
    kw = {}
    pshape = None
    boxes = rnd(*shape, seed=11).clamp(-1, 1).to(dev)
    if given == "dense":
        kw["partial_boxes"] = boxes[:, :PMAX].contiguous()
        pshape = (B, PMAX, C)
    elif given == "rows":
        kw["partial_boxes"], kw["counts"] = gd._ragged_inputs(shape, dev, boxes[:, :PMAX].contiguous(), [0, PMAX], front)
        pshape = (B, PMAX, C)
    elif given == "mask":
        kw["known"], kw["mask"] = gd._masked_inputs(shape, dev, boxes, rnd(*shape, seed=12) > 0.3, front)
        pshape = shape
    if fused is not None:
        kw["fused"] = fused
    main = rnd(steps + (0 if strided else 1), *shape, seed=13).to(dev)
    part = None if pshape is None else rnd(steps, *pshape, seed=14).to(dev)
    sched = (S, ETA) if strided else (True, STEPS)
    lines = []
    st = Blocks(dev)
    real = record_calls(lines, st)
    try:
        for call in ("capture", "cached", "cached again"):
            lines.append("# %s" % call)
            if mode == "seeded":
                noise_fn = SceneNoise([7, 2 ** 40 + 3], dev)
            elif mode == "replay":
                noise_fn = (sampler.NoiseReplay if given in (None, "dense") else sampler.RaggedNoiseReplay)(main, part)
            else:
                noise_fn = torch.randn
            torch.manual_seed(0)
            with torch.no_grad():
                out = getattr(sampler, front)(gd, dp._denoise, shape, dev, *head, *sched, noise_fn=noise_fn, **kw)
            lines.append("# -> %s finite=%s" % (tuple(out.shape), bool(torch.isfinite(out).all())))
    finally:
        _lib.fn = real
    (g,) = gd._graphs.values()
    lines.append("# class %s graph=%s final=%s unnamed pointers=%d" % (type(g).__name__, g.graph is not None, g.final is not None,
                                                                       st.unknown))
    gd._graphs.clear()
    model.diffusion.model.engine(dev).plans.clear()         # every case builds its plan anew, through the recording wrappers
    del g
    return "\n".join(lines) + "\n"


def main():
    outdir = sys.argv[1]
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda:0")
    model, _ = bench.build_model(dict(bench.CONFIGS["text"], batch=B), dev)
    sums = []
    for front, strided, given, guided, has_fused in ROWS:
        for S in ((1, 3) if strided else (None,)):
            for fused in ((True, False) if has_fused else (None,)):
                for mode in MODES:
                    label = front[len("graph_"):] + ("_dense" if given == "dense" else "") + ("" if S is None else "_S%d" % S) \
                        + ("" if fused is None else "_fused%d" % fused) + "_" + mode
                    text = run_case(front, strided, given, guided, fused, S, mode, model, dev)
                    with open(os.path.join(outdir, label + ".txt"), "w") as f:
                        f.write(text)
                    sums.append("%s  %s.txt  %d calls" % (hashlib.sha256(text.encode()).hexdigest(), label,
                                                          sum(1 for ln in text.splitlines() if not ln.startswith("#"))))
                    print(sums[-1], flush=True)
                    gc.collect()
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
    with open(os.path.join(outdir, "SHA256SUMS"), "w") as f:
        f.write("\n".join(sums) + "\n")


if __name__ == "__main__":
    main()
