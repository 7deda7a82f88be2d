#!/usr/bin/env python
"""Canonical dump of the launch lists the planners produce, to compare two trees launch for launch and argument for argument.

For each of the five BASELINE configurations, at B = 2 and at its BASELINE batch, under both GEMM arithmetics, builds the sampling plans
(DenoiserEngine.prepare, time_table both ways) and the TrainPlan on HipBackend -- nothing is launched beyond what plan construction
itself launches -- and writes every recorded step (pre_steps / steps, fwd / bwd) as one line:

* pointer arguments and pointer fields (known from _lib.SIGNATURES and the ctypes _fields_) as ``s<k>+<byte offset>``: k numbers the
  storages reachable from the plan, the engine and the model by first appearance in launch order; NULL is ``0``; a pointer into no
  known storage is an error;
* structs and host arrays field by field; the device tables of the grouped launches are read back and decoded with the same structs.

    python tools/launch_lists.py OUTDIR [config ...]

writes OUTDIR/<arithmetic>_<config>_B<batch>.txt and OUTDIR/SHA256SUMS.  Run it in two trees and compare the SHA256SUMS files.
Only attributes that both trees have are used."""
import bisect
import ctypes as C
import hashlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from diffuscene_amd import _lib  # noqa: E402
from diffuscene_amd._lib import SS_NONE, SS_PER_SLOT, SS_PER_TOKEN  # noqa: E402
from diffuscene_amd.train_plan import HipBackend, TrainPlan  # noqa: E402

# (entry point) -> [(index of the table pointer, index of its item count, item struct | "i32x2")] of the grouped launches
TABLES = {"dsc_gemm_tn_grouped_f32": [(0, 1, _lib.TnGroup)],
          "dsc_gemm_tn_grouped_split_f32": [(0, 1, _lib.TnGroup), (3, 4, "i32x2")],
          "dsc_colsum_grouped_f32": [(0, 1, _lib.ColsumItem)]}


class Storages:
    """The storages reachable from the roots, numbered by first appearance among the pointers resolved."""

    def __init__(self, *roots):
        self.spans, self.by_ptr, self.number = {}, {}, {}
        seen, todo = set(), list(roots)
        while todo:
            o = todo.pop()
            if o is None or isinstance(o, (int, float, str, bytes, bool, C.Structure, C.Array, type)) or id(o) in seen:
                continue
            seen.add(id(o))
            if isinstance(o, torch.Tensor):
                st = o.untyped_storage()
                if st.nbytes():
                    self.spans[st.data_ptr()] = max(self.spans.get(st.data_ptr(), 0), st.nbytes())
                    self.by_ptr.setdefault(o.data_ptr(), o)
                todo += [getattr(o, "_base", None), getattr(o, "_dsc_fragment", None)]
            elif isinstance(o, (list, tuple, set, frozenset)):
                todo += list(o)
            elif isinstance(o, dict):
                todo += list(o.values())
            elif isinstance(o, types.FunctionType):
                todo += [c.cell_contents for c in (o.__closure__ or ()) if _filled(c)]
            elif isinstance(o, types.MethodType):
                todo.append(o.__self__)
            elif isinstance(o, torch.nn.Module):
                todo += list(o.parameters(recurse=False)) + list(o.buffers(recurse=False)) + list(vars(o).values())
            elif hasattr(o, "__dict__") and type(o).__module__.split(".")[0] in ("diffuscene_amd", "bench", "__main__"):
                todo += list(vars(o).values())
        self.bases = sorted(self.spans)

    def name(self, ptr, what):
        if not ptr:
            return "0"
        i = bisect.bisect_right(self.bases, ptr) - 1
        if i < 0 or ptr >= self.bases[i] + self.spans[self.bases[i]]:
            raise SystemExit("launch_lists: %s: pointer %#x lies in no storage reachable from the plan" % (what, ptr))
        base = self.bases[i]
        k = self.number.setdefault(base, len(self.number))
        return "s%d+%d" % (k, ptr - base)

    def read(self, ptr, nbytes):
        t = self.by_ptr[ptr]
        return t.contiguous().view(-1).view(torch.uint8)[:nbytes].cpu().numpy().tobytes()


def _filled(cell):
    try:
        cell.cell_contents
        return True
    except ValueError:
        return False


def fmt_struct(s, st, what):
    out = []
    for fname, ftype in s._fields_:
        v = getattr(s, fname)
        out.append("%s=%s" % (fname, st.name(v, "%s.%s" % (what, fname)) if ftype is C.c_void_p else repr(v)))
    return "{" + " ".join(out) + "}"


def fmt_step(name, args, st):
    argtypes = _lib.SIGNATURES[name][1][:-1]              # (the stream is not part of a recorded step)
    if len(argtypes) != len(args):
        raise SystemExit("launch_lists: %s recorded with %d arguments, the C ABI takes %d" % (name, len(args), len(argtypes)))
    out = []
    for i, (ty, a) in enumerate(zip(argtypes, args)):
        what = "%s arg %d" % (name, i)
        if ty is C.c_void_p:
            out.append(st.name(a, what))
        elif isinstance(ty, type) and issubclass(ty, C._Pointer):
            if a is None:
                out.append("0")
                continue
            obj = getattr(a, "_obj", a)                   # ctypes.byref(struct) keeps the struct in ._obj
            items = list(obj) if isinstance(obj, C.Array) else [obj]
            out.append("[" + " ".join(fmt_struct(x, st, what) if isinstance(x, C.Structure) else repr(x) for x in items) + "]")
        else:
            out.append(repr(a))
    for pi, ci, item in TABLES.get(name, ()):
        if not args[pi]:
            continue
        if item == "i32x2":
            raw = st.read(args[pi], 8 * args[ci])
            vals = (C.c_int32 * (2 * args[ci])).from_buffer_copy(raw)
            out.append("table%d=[%s]" % (pi, " ".join(str(v) for v in vals)))
        else:
            arr = (item * args[ci]).from_buffer_copy(st.read(args[pi], C.sizeof(item) * args[ci]))
            out.append("table%d=[%s]" % (pi, " ".join(fmt_struct(x, st, "%s table" % name) for x in arr)))
    return "%s(%s)" % (name, ", ".join(out))


def dump_steps(title, steps, st, lines):
    lines.append("# %s: %d launches" % (title, len(steps)))
    for s in steps:
        if isinstance(s, dict):
            s = s["step"]
        lines.append(fmt_step(s[0].__name__, s[1], st))


def train_signature(spec, model, cond, cross):
    """What train_step.loss_step hands to PlanRunner.plan_for for this configuration."""
    ctx_mode, ctx_dim, ctx_param = SS_NONE, 0, None
    if cond is not None:
        ctx_dim = cond.shape[-1]
        if cond.stride(0) == 0:
            ctx_mode, ctx_param = SS_PER_SLOT, getattr(model, "positional_embedding", None)
        else:
            ctx_mode = SS_PER_TOKEN
    L, text_dim = (cross.shape[1], cross.shape[2]) if cross is not None else (0, 0)
    return ctx_mode, ctx_dim, L, text_dim, ctx_param


def dump_config(name, batch, dev):
    spec = dict(bench.CONFIGS[name], batch=batch)
    model, _ = bench.build_model(spec, dev)
    (B, N, _), cond, cross, _, _ = bench.sampling_inputs(spec, model, dev, seed=0)
    net = model.diffusion.model
    lines = []
    eng = net.engine(dev)
    for tt in (False, True):
        plan = eng.prepare(B, N, cond, cross, time_table=tt)
        st = Storages(plan, eng, model, cond, cross)
        dump_steps("sampling time_table=%d pre_steps" % tt, plan.pre_steps, st, lines)
        dump_steps("sampling time_table=%d steps" % tt, plan.steps, st, lines)
    ctx_mode, ctx_dim, L, text_dim, ctx_param = train_signature(spec, model, cond, cross)
    if ctx_param is not None and tuple(ctx_param.shape) != (N, ctx_dim):
        ctx_param = None
    be = HipBackend(dev)
    tp = TrainPlan(net, model._dsc_flat, model.diffusion.diffusion, B, N, ctx_mode, ctx_dim, L, text_dim, be, ctx_param=ctx_param,
                   grad_scale=1.0 / B)
    st = Storages(tp, be, model)
    dump_steps("train fwd", tp.fwd, st, lines)
    dump_steps("train bwd", tp.bwd, st, lines)
    return "\n".join(lines) + "\n"


def main():
    outdir = sys.argv[1]
    names = sys.argv[2:] or ["living80", "bedroom21", "text", "arrange", "complete"]
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device("cuda:0")
    sums = []
    for arith in ("split", "f32"):
        _lib.set_gemm_arithmetic(arith)
        for name in names:
            for batch in (2, bench.CONFIGS[name]["batch"]):
                label = "%s_%s_B%d" % (arith, name, batch)
                text = dump_config(name, batch, dev)
                with open(os.path.join(outdir, label + ".txt"), "w") as f:
                    f.write(text)
                sums.append("%s  %s.txt  %d launches" % (hashlib.sha256(text.encode()).hexdigest(), label,
                                                        sum(1 for ln in text.splitlines() if not ln.startswith("#"))))
                print(sums[-1], flush=True)
                torch.cuda.empty_cache()
    with open(os.path.join(outdir, "SHA256SUMS"), "w") as f:
        f.write("\n".join(sums) + "\n")


if __name__ == "__main__":
    main()
