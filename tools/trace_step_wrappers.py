"""The argument lists that the eight step wrappers of ops.py hand to their dsc_* symbols, without a GPU: CPU tensors, a recording _lib.
Pointers are recorded by operand name, so the order and the value of every argument can be read; bad calls record the exception type
and text, and that nothing was launched before it.

    python tools/trace_step_wrappers.py <checkout root> <out.json>

Run it on two checkouts and compare the files (pointers of tensors that a wrapper allocates itself differ from run to run)."""
import os, sys, json
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch
from diffuscene_amd import ops, _lib
assert ops.__file__.startswith(root)

def _dev(t, name="tensor", dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("not a tensor: %s" % name)
    if t.dtype != dtype:
        raise RuntimeError("diffuscene_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
    return t
ops._dev = _dev
ops.stream_ptr = lambda: "STREAM"
NAMES = {}
CALLS = []
def fn(sym):
    def call(*a):
        CALLS.append([sym] + [NAMES.get(x, x) if isinstance(x, int) and x > 4096 else x for x in a])
        return 0
    return call
_lib.fn = fn
_lib.check = lambda rc, name: None

B, N, C, S, T = 2, 5, 7, 4, 30
g = torch.Generator().manual_seed(0)
def mk(name, *shape, dtype=torch.float32):
    t = torch.randn(*shape, generator=g).to(dtype) if dtype.is_floating_point else torch.zeros(*shape, dtype=dtype)
    NAMES[t.data_ptr()] = name
    return t
x, mo, noise, given, gn, out, x0o, dup = (mk(n, B, N, C) for n in ("x", "mo", "noise", "given", "gn", "out", "x0o", "dup"))
mo2 = mk("mo2", 2 * B, N, C)
mask = mk("mask", B, N, C, dtype=torch.uint8)
counts = mk("counts", B, dtype=torch.int64)
scale = mk("scale", B)
t = mk("t", B, dtype=torch.int64)
step = mk("step", 1, dtype=torch.int64)
times, times_next = mk("times", S, dtype=torch.int64), mk("times_next", S, dtype=torch.int64)
coef = mk("coef", 3, S)
for r in range(3):
    NAMES[coef[r].data_ptr()] = "coef%d" % r
tabs = {n: mk(n, T) for n in ("ca", "cb", "c1", "c2", "sigma", "recip", "recipm1", "sa", "sb")}
ca, cb, c1, c2, sigma, recip, recipm1, sa, sb = tabs.values()

def attempt(what, f):
    n0 = len(CALLS)
    try:
        r = f()
        CALLS.append(["ok", what, NAMES.get(r.data_ptr(), "fresh")])
    except Exception as e:
        assert len(CALLS) == n0, "launched before refusing"
        CALLS.append(["refused", what, type(e).__name__, str(e)])

for A, Bc in ((ca, cb), (None, None)):
    for o in (None, out):
        post, dd = (A, Bc, c1, c2, sigma), (times, times_next, coef, A, Bc, recip, recipm1)
        attempt("p_sample", lambda: ops.p_sample(x, mo, noise, t, *post, 2, True, out=o, x0_out=x0o if o is not None else None))
        attempt("ddim_step", lambda: ops.ddim_step(x, mo, noise, step, *dd, 1, out=o, x0_out=x0o if o is None else None))
        attempt("p_sample_inpaint", lambda: ops.p_sample_inpaint(x, mo, noise, given, gn, counts, t, *post, sa, sb, 0, False, out=o))
        attempt("ddim_inpaint_step", lambda: ops.ddim_inpaint_step(x, mo, noise, given, gn, counts, step, *dd, sa, sb, 2, out=o))
        attempt("p_sample_masked", lambda: ops.p_sample_masked(x, mo, noise, given, gn, mask, t, *post, sa, sb, 2, True, out=o))
        attempt("ddim_masked_step", lambda: ops.ddim_masked_step(x, mo, noise, given, gn, mask, step, *dd, sa, sb, 2, out=o))
        attempt("p_sample_cfg", lambda: ops.p_sample_cfg(x, mo2, scale, noise, t, *post, 2, True, out=o, x_dup=dup if o is not None else None, x0_out=x0o if o is not None else None))
        attempt("ddim_cfg_step", lambda: ops.ddim_cfg_step(x, mo2, scale, noise, step, *dd, 2, out=o, x_dup=dup if o is not None else None, x0_out=x0o if o is None else None))
# refusals
post, dd = (ca, cb, c1, c2, sigma), (times, times_next, coef, ca, cb, recip, recipm1)
bad_tn, bad_coef, bad_mo, bad_out = torch.zeros(S + 1, dtype=torch.int64), torch.zeros(2, S), torch.zeros(B, N, C + 1), torch.zeros(B, C, N).transpose(1, 2)
short = torch.zeros(T - 1)
nc_x0 = torch.zeros(B, C, N).transpose(1, 2)
def strided(name, f, **kw):
    for what, rep in (("times_next", dict(tn=bad_tn)), ("coef", dict(cf=bad_coef)), ("step dtype", dict(st=torch.zeros(1))), ("times nc", dict(tm=torch.zeros(2 * S, dtype=torch.int64)[::2]))):
        a = dict(st=step, tm=times, tn=times_next, cf=coef); a.update(rep)
        attempt(name + " bad " + what, lambda: f(a["st"], a["tm"], a["tn"], a["cf"]))
strided("ddim_step", lambda st, tm, tn, cf: ops.ddim_step(x, mo, noise, st, tm, tn, cf, ca, cb, recip, recipm1, 2))
strided("ddim_inpaint_step", lambda st, tm, tn, cf: ops.ddim_inpaint_step(x, mo, noise, given, gn, counts, st, tm, tn, cf, ca, cb, recip, recipm1, sa, sb, 2))
strided("ddim_masked_step", lambda st, tm, tn, cf: ops.ddim_masked_step(x, mo, noise, given, gn, mask, st, tm, tn, cf, ca, cb, recip, recipm1, sa, sb, 2))
strided("ddim_cfg_step", lambda st, tm, tn, cf: ops.ddim_cfg_step(x, mo2, scale, noise, st, tm, tn, cf, ca, cb, recip, recipm1, 2))
for m_, n_, o_, tag in ((bad_mo, noise, None, "model_out shape"), (mo, bad_mo, None, "noise shape"), (mo, noise, bad_out, "out nc"), (mo, noise, torch.zeros(B, N, C + 1), "out shape")):
    attempt("p_sample " + tag, lambda: ops.p_sample(x, m_, n_, t, *post, 2, True, out=o_))
    attempt("ddim_step " + tag, lambda: ops.ddim_step(x, m_, n_, step, *dd, 2, out=o_))
    attempt("p_sample_inpaint " + tag, lambda: ops.p_sample_inpaint(x, m_, n_, given, gn, counts, t, *post, sa, sb, 2, True, out=o_))
    attempt("ddim_inpaint_step " + tag, lambda: ops.ddim_inpaint_step(x, m_, n_, given, gn, counts, step, *dd, sa, sb, 2, out=o_))
    attempt("p_sample_masked " + tag, lambda: ops.p_sample_masked(x, m_, n_, given, gn, mask, t, *post, sa, sb, 2, True, out=o_))
    attempt("ddim_masked_step " + tag, lambda: ops.ddim_masked_step(x, m_, n_, given, gn, mask, step, *dd, sa, sb, 2, out=o_))
    attempt("p_sample_cfg " + tag, lambda: ops.p_sample_cfg(x, mo2 if m_ is mo else m_, scale, n_, t, *post, 2, True, out=o_))
    attempt("ddim_cfg_step " + tag, lambda: ops.ddim_cfg_step(x, mo2 if m_ is mo else m_, scale, n_, step, *dd, 2, out=o_))
for tag, kw in (("x0_out shape", dict(x0_out=torch.zeros(B, N, C + 1))), ("x0_out nc", dict(x0_out=nc_x0))):
    attempt("p_sample_cfg " + tag, lambda: ops.p_sample_cfg(x, mo2, scale, noise, t, *post, 2, True, **kw))
    attempt("ddim_cfg_step " + tag, lambda: ops.ddim_cfg_step(x, mo2, scale, noise, step, *dd, 2, **kw))
# table rows that disagree
attempt("p_sample rows", lambda: ops.p_sample(x, mo, noise, t, ca, cb, c1, short, sigma, 2, True))
attempt("ddim_step rows", lambda: ops.ddim_step(x, mo, noise, step, times, times_next, coef, ca, cb, recip, short, 2))
attempt("p_sample_inpaint rows", lambda: ops.p_sample_inpaint(x, mo, noise, given, gn, counts, t, *post, sa, short, 2, True))
attempt("ddim_inpaint_step rows", lambda: ops.ddim_inpaint_step(x, mo, noise, given, gn, counts, step, *dd, short, sb, 2))
attempt("p_sample_masked rows", lambda: ops.p_sample_masked(x, mo, noise, given, gn, mask, t, *post, sa, short, 2, True))
attempt("ddim_masked_step rows", lambda: ops.ddim_masked_step(x, mo, noise, given, gn, mask, step, *dd, short, sb, 2))
attempt("p_sample_cfg rows", lambda: ops.p_sample_cfg(x, mo2, scale, noise, t, short, cb, c1, c2, sigma, 2, True))
attempt("ddim_cfg_step rows", lambda: ops.ddim_cfg_step(x, mo2, scale, noise, step, times, times_next, coef, ca, short, recip, recipm1, 2))
json.dump(CALLS, open(sys.argv[2], "w"), indent=0)
print(len(CALLS), "records;", sum(c[0] == "refused" for c in CALLS), "refusals")
