"""The launch sequence of the twelve eager loops of diffusion_ddpm.py, without a GPU: the loops run on the CPU over recording fakes of
the ops they launch (the fakes compute, so the outputs are comparable too).  Each noise_fn call (size, its type, dtype, device as passed),
model call, table upload, op call (operand shapes, timesteps, counts, step counter), what was printed, whether the caller's draws were
written to, and the first complaint about a set of bad arguments are recorded.

    python tools/trace_eager_loops.py <checkout root> <out.json>

Run it on two checkouts and compare the files: equal files mean equal draw protocol, launch order, outputs, prints and refusals."""
import os, sys, json, io, contextlib, hashlib
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch
from diffuscene_amd import ops
from diffuscene_amd.networks import diffusion_ddpm as D
assert D.__file__.startswith(root), D.__file__

EV = []
def sh(t):
    return None if t is None else (tuple(t.shape) if isinstance(t, torch.Tensor) else t)
def rec(name, *a):
    EV.append([name] + [sh(x) if isinstance(x, torch.Tensor) or x is None else x for x in a])

def tables(self, device):
    tb = self._dev.get("cpu")
    if tb is None:
        rec("tables_upload")
        tb = {n: getattr(self, n).clone() for n in self._TABLE_NAMES}
        self._dev["cpu"] = tb
    return tb
D.GaussianDiffusion.tables = tables

def p_sample(x_t, model_out, noise, t, ca, cb, c1, c2, sigma, mean_type, clip, out=None, x0_out=None):
    rec("p_sample", x_t, model_out, noise, t.tolist(), ca is not None, mean_type, bool(clip), out is not None, x0_out is not None)
    return 0.9 * x_t - 0.1 * model_out + 0.01 * (t[:, None, None] + 1) * noise
def ddim_step(x_t, model_out, noise, step, times, times_next, coef, ca, cb, a, b, mean_type, out=None, x0_out=None):
    k = int(step)
    rec("ddim_step", x_t, model_out, noise, k, times.tolist(), times_next.tolist(), [round(float(v), 6) for v in coef[:, k]], noise is x_t, mean_type)
    return 0.8 * x_t - 0.2 * model_out + (0.0 if times_next[k] < 0 else 0.05 * noise)
def ddim_advance(step, times, t):
    rec("ddim_advance", int(step))
    step += 1
    t.fill_(int(times[int(step)]))
    return t
def cfg_combine(mo, scale, out=None):
    rec("cfg_combine", mo, scale.tolist())
    b = mo.shape[0] // 2
    return mo[b:] + scale[:, None, None] * (mo[:b] - mo[b:])
def complete_overwrite(x, partial, noise, t, sa, sb):
    rec("complete_overwrite", x, partial, noise, t.tolist())
    x[:, :partial.shape[1]] = partial * 0.5 + noise * 0.1 * (t[:, None, None] + 1)
    return x
def complete_overwrite_ragged(x, partial, noise, counts, t, sa, sb):
    rec("complete_overwrite_ragged", x, partial, noise, counts.tolist(), t.tolist())
    for b, c in enumerate(counts.tolist()):
        x[b, :c] = partial[b, :c] * 0.5 + noise[b, :c] * 0.1 * (t[b] + 1)
    return x
def masked_overwrite(x, known, noise, mask, t, sa, sb):
    rec("masked_overwrite", x, known, noise, int(mask.sum()), t.tolist())
    x.copy_(torch.where(mask != 0, known * 0.5 + noise * 0.1 * (t[:, None, None] + 1), x))
    return x
for f in (p_sample, ddim_step, ddim_advance, cfg_combine, complete_overwrite, complete_overwrite_ragged, masked_overwrite):
    setattr(ops, f.__name__, f)

def denoise(x, t, c, cc):
    rec("model", x, t.tolist(), c, cc)
    return torch.tanh(x) * 0.5 + (0 if cc is None else cc.mean()) if x.shape[0] == t.shape[0] else None

class Noise:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.made = []
    def __call__(self, size=None, dtype=None, device=None):
        rec("draw", tuple(size), type(size).__name__, str(dtype), repr(device))
        n = torch.randn(tuple(size), generator=self.g)
        self.made.append((n, n.clone()))
        return n

B, N, C = 2, 6, 62
cfg = dict(objectness_dim=0, class_dim=22, angle_dim=2, objfeat_dim=32)
OUT = {}
def digest(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()[:16]
def run(name, mt, fn):
    gd = D.GaussianDiffusion(cfg, D.get_betas("linear", 1e-4, 0.02, 3 if "ddim" not in name else 20), "mse", mt, "fixedsmall", False, False, None)
    nf = Noise(7)
    EV.append(["== " + name + " " + mt])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = fn(gd, nf)
    EV.append(["stdout", buf.getvalue()])
    EV.append(["buffers_untouched", all(torch.equal(a, b) for a, b in nf.made)])
    EV.append(["x_T_is_draw0", (res[0] if isinstance(res, list) else res) is nf.made[0][0]])
    OUT[name + "." + mt] = [digest(r) for r in res] if isinstance(res, list) else digest(res)
    EV.append(["attrs", getattr(gd, "ddim_sampling_eta", None), getattr(gd, "sampling_timesteps", None)])

g = torch.Generator().manual_seed(3)
shape = (B, N, C)
cond = torch.randn(B, N, 8, generator=g)
cross = torch.randn(B, 4, 8, generator=g)
given = torch.randn(B, N, C, generator=g)
mask = torch.rand(B, N, C, generator=g) > 0.5
for mt in ("v", "eps", "x0"):
    for kr in (False, True):
        run("p_sample_loop kr=%s" % kr, mt, lambda gd, nf: gd.p_sample_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, clip_denoised=not kr, keep_running=kr))
    run("trajectory", mt, lambda gd, nf: gd.p_sample_loop_trajectory(denoise, shape, "cpu", 2, cond, None, noise_fn=nf))
    for S in (1, 3):
        run("ddim S=%d" % S, mt, lambda gd, nf: gd.ddim_sample_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=S, ddim_sampling_eta=0.5))
        run("ddim all S=%d" % S, mt, lambda gd, nf: gd.ddim_sample_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=S, ddim_sampling_eta=0.5, return_all_timesteps=True))
        run("guided ddim S=%d" % S, mt, lambda gd, nf: gd.ddim_guided_loop(denoise, shape, "cpu", cond, cross, (0.0, 3.0), noise_fn=nf, sampling_timesteps=S, ddim_sampling_eta=0.3))
        for pmax, counts in ((1, [0, 1]), (N, [2, N])):
            run("ragged ddim S=%d pmax=%d" % (S, pmax), mt, lambda gd, nf: gd.ddim_complete_ragged_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=S, ddim_sampling_eta=0.5, partial_boxes=given[:, :pmax], num_partial=counts))
        run("masked ddim S=%d" % S, mt, lambda gd, nf: gd.ddim_masked_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=S, ddim_sampling_eta=0.5, known=given, mask=mask))
        run("arrange ddim S=%d" % S, mt, lambda gd, nf: gd.ddim_arrange_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=S, ddim_sampling_eta=0.5, input_boxes=given))
    run("guided", mt, lambda gd, nf: gd.p_sample_loop_guided(denoise, shape, "cpu", cond, cross, 2.0, noise_fn=nf))
    run("guided stride0 cond", mt, lambda gd, nf: gd.p_sample_loop_guided(denoise, shape, "cpu", cond[:1].expand(B, -1, -1), cross, 2.0, noise_fn=nf))
    for pmax in (1, N):
        run("dense pmax=%d" % pmax, mt, lambda gd, nf: gd.p_sample_loop_complete(denoise, shape, "cpu", cond, None, noise_fn=nf, partial_boxes=given[:, :pmax]))
        run("ragged pmax=%d" % pmax, mt, lambda gd, nf: gd.p_sample_loop_complete_ragged(denoise, shape, "cpu", cond, None, noise_fn=nf, partial_boxes=given[:, :pmax], num_partial=[0, pmax]))
    run("masked", mt, lambda gd, nf: gd.p_sample_loop_masked(denoise, shape, "cpu", cond, None, noise_fn=nf, known=given, mask=mask[:, :, 0]))
    run("arrange", mt, lambda gd, nf: gd.p_sample_loop_arrange(denoise, shape, "cpu", cond, None, noise_fn=nf, input_boxes=given))
# refusals: type and text of the first complaint
def refusal(name, fn):
    gd = D.GaussianDiffusion(cfg, D.get_betas("linear", 1e-4, 0.02, 20), "mse", "v", "fixedsmall", False, False, None)
    n0 = len(EV)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn(gd, Noise(1))
        r = "no refusal"
    except Exception as e:
        r = type(e).__name__ + ": " + str(e)
    del EV[n0:]
    EV.append(["refusal", name, r])
refusal("ddim S=0", lambda gd, nf: gd.ddim_sample_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=0))
refusal("ragged ddim S=0 and no boxes", lambda gd, nf: gd.ddim_complete_ragged_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=0))
refusal("ragged ddim no boxes", lambda gd, nf: gd.ddim_complete_ragged_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=3))
refusal("ragged no boxes", lambda gd, nf: gd.p_sample_loop_complete_ragged(denoise, shape, "cpu", cond, None, noise_fn=nf))
refusal("ragged bad pmax", lambda gd, nf: gd.p_sample_loop_complete_ragged(denoise, shape, "cpu", cond, None, noise_fn=nf, partial_boxes=torch.zeros(B, N + 1, C), num_partial=[0, 0]))
refusal("ragged bad count", lambda gd, nf: gd.p_sample_loop_complete_ragged(denoise, shape, "cpu", cond, None, noise_fn=nf, partial_boxes=given, num_partial=[0, N + 1]))
refusal("ragged ddim bad count", lambda gd, nf: gd.ddim_complete_ragged_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=3, partial_boxes=given, num_partial=[0, N + 1]))
refusal("masked no known", lambda gd, nf: gd.p_sample_loop_masked(denoise, shape, "cpu", cond, None, noise_fn=nf))
refusal("masked ddim S=0 no known", lambda gd, nf: gd.ddim_masked_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=0))
refusal("masked ddim bad mask", lambda gd, nf: gd.ddim_masked_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=3, known=given, mask=mask.float()))
refusal("guided no cross", lambda gd, nf: gd.p_sample_loop_guided(denoise, shape, "cpu", cond, None, 2.0, noise_fn=nf))
refusal("guided ddim S=0 no cross", lambda gd, nf: gd.ddim_guided_loop(denoise, shape, "cpu", cond, None, 2.0, noise_fn=nf, sampling_timesteps=0))
refusal("guided ddim bad scale", lambda gd, nf: gd.ddim_guided_loop(denoise, shape, "cpu", cond, cross, float("inf"), noise_fn=nf, sampling_timesteps=3))
refusal("arrange ddim S=0 no boxes", lambda gd, nf: gd.ddim_arrange_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=0))
refusal("arrange ddim no boxes", lambda gd, nf: gd.ddim_arrange_loop(denoise, shape, "cpu", cond, None, noise_fn=nf, sampling_timesteps=3))
refusal("dense no boxes", lambda gd, nf: gd.p_sample_loop_complete(denoise, shape, "cpu", cond, None, noise_fn=nf))
refusal("list shape plain", lambda gd, nf: gd.p_sample_loop(denoise, list(shape), "cpu", cond, None, noise_fn=nf))
json.dump({"events": EV, "outputs": OUT}, open(sys.argv[2], "w"), indent=0)
print(len(EV), "events,", len(OUT), "runs")
