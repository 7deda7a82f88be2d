"""The multistep DPM-Solver++(2M) solver of INTEGRATION.md 9, restated in torch on the host, and a toy model with an exact solution.

The statement (``correct``): at pair k with history weight e, for every free element -- float32 up to the clamped x0, float64 after it,
one rounding --
    m = mo, or u + w (c - u) from the two halves of a guided 2 B output;  x0raw = predict_x0(x_t, m);  x0c = clamp(x0raw, -1, 1);
    D = x0c + e (x0c - hist);  d = x0raw - D;  mean type x0: m' = m - d;  eps / v: m' = m + d / Bc (Bc == 0: unchanged);  hist = x0c.
e == 0 leaves mo as it is and does not read hist; the last pair leaves hist as it is; a given element is left alone everywhere.

The toy: data x0 ~ N(MU, SD^2) elementwise.  With alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t) the exact denoiser is
eps(x, t) = sigma_t (x - alpha_t MU) / (alpha_t^2 SD^2 + sigma_t^2) and the exact probability-flow solution
x_t = alpha_t MU + sqrt(alpha_t^2 SD^2 + sigma_t^2) z with z fixed along a trajectory.  ``chain`` runs the strided loop on it -- DDIM at
eta = 0, or the solver -- in a dtype of the caller's choice; the clamp is never active on this toy (|D| <= 0.32 at S = 20)."""
import numpy as np
import torch

MU, SD = 0.2, 0.1
EPS, X0, V = 0, 1, 2


def betas(T=1000, lo=1e-4, hi=0.02):
    return np.linspace(lo, hi, T, dtype=np.float64)


def pairs(S, T=1000):
    """The (t, t_next) pairs of the strided schedule: float32 linspace from -1 to T - 1, truncated, reversed; the last ends at -1."""
    times = list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))
    return list(zip(times[:-1], times[1:]))


def weights(prs, abar):
    """e_0 = 0, e_k = h_k / (2 h_{k-1}) for 1 <= k <= S - 2, e_{S-1} = 0, h_k = lambda(t'_k) - lambda(t_k), lambda = 1/2 ln(abar / (1 - abar)):
    float64 numpy, the closed form written out pair by pair."""
    abar = np.asarray(abar, dtype=np.float64)
    lam = lambda t: 0.5 * (np.log(abar[t]) - np.log1p(-abar[t]))  # noqa: E731
    S = len(prs)
    e = np.zeros(S, dtype=np.float64)
    for k in range(1, S - 1):
        h_k = lam(prs[k][1]) - lam(prs[k][0])
        h_prev = lam(prs[k - 1][1]) - lam(prs[k - 1][0])
        e[k] = h_k / (2.0 * h_prev)
    return e


def tables(S, T=1000, abar=None):
    """The per-pair float64 scalars of the chain for the linear schedule: A, Bc (x0 = A x - Bc eps), an = sqrt(abar_next),
    cn = sqrt(1 - abar_next), the toy's alpha, sigma at t, and the history weights e."""
    abar = np.cumprod(1.0 - betas(T)) if abar is None else np.asarray(abar, dtype=np.float64)
    prs = pairs(S, T)
    t = np.array([p[0] for p in prs])
    tn = np.array([max(p[1], 0) for p in prs])
    last = np.array([p[1] < 0 for p in prs])
    tab = dict(A=np.sqrt(1.0 / abar[t]), Bc=np.sqrt(1.0 / abar[t] - 1.0), an=np.where(last, 0.0, np.sqrt(abar[tn])),
               cn=np.where(last, 0.0, np.sqrt(1.0 - abar[tn])), alpha=np.sqrt(abar[t]), sigma=np.sqrt(1.0 - abar[t]), e=weights(prs, abar))
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in tab.items()}, prs


def toy_eps(x, alpha, sigma):
    """The exact denoiser of the toy, in x's dtype; one rounding per operation, in this order."""
    var = alpha * alpha * (SD * SD) + sigma * sigma
    return sigma * (x - alpha * MU) / var


def toy_exact(z, alpha, sigma):
    """The exact probability-flow state at (alpha, sigma) of the trajectory z (float64)."""
    return alpha * MU + np.sqrt(alpha * alpha * SD * SD + sigma * sigma) * z


def chain(tab, z, solver, dtype=torch.float64):
    """The strided loop on the toy from x_T = toy_exact(z) in ``dtype`` (the tables are rounded to it first): per pair the model call,
    [the solver's correction of its output,] the eta = 0 DDIM step on it.  -> (the S + 1 states, the largest |D| met)."""
    tb = {k: v.to(dtype) for k, v in tab.items()}
    S = tb["A"].numel()
    x = toy_exact(z.double(), float(tab["alpha"][0]), float(tab["sigma"][0])).to(dtype)
    states, hist, dmax = [x], None, 0.0
    for k in range(S):
        A, Bc, an, cn, e = (tb[n][k] for n in ("A", "Bc", "an", "cn", "e"))
        m = toy_eps(x, tb["alpha"][k], tb["sigma"][k])
        raw = A * x - Bc * m
        x0c = raw.clamp(-1, 1)
        if solver and float(e) != 0.0:
            D = x0c + e * (x0c - hist)
            dmax = max(dmax, float(D.abs().max()))
            m = m + (raw - D) / Bc
        hist = x0c
        x0 = (A * x - Bc * m).clamp(-1, 1)
        x = x0 if k == S - 1 else x0 * an + cn * m
        states.append(x)
    return states, dmax


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def correct(x_t, mo, hist, e, A, Bc, mean_type, scale=None, given=None, last=False):
    """The statement of the module docstring on host float32 tensors: x_t, hist (B, ...), mo (B, ...) or (2 B, ...) under ``scale`` (B,),
    e / A / Bc float32 scalars (0-dim tensors or floats holding float32 values), ``given`` a bool tensor of x_t's shape or None.
    -> (mo', hist')."""
    B = hist.shape[0]
    f32 = lambda v: torch.as_tensor(v, dtype=torch.float32)  # noqa: E731
    e, A, Bc = f32(e), f32(A), f32(Bc)
    c, u = (mo, None) if scale is None else (mo[:B], mo[B:])
    if scale is None:
        m = c
    else:
        w = scale.reshape((B,) + (1,) * (hist.dim() - 1))
        m = u + w * (c - u)
    raw = m if mean_type == X0 else A * x_t - Bc * m
    x0c = raw.clamp(-1, 1)
    free = torch.ones_like(hist, dtype=torch.bool) if given is None else ~given
    if last:
        return mo.clone(), hist.clone()
    new_hist = torch.where(free, x0c, hist)
    if float(e) == 0.0 or (mean_type != X0 and float(Bc) == 0.0):
        return mo.clone(), new_hist
    x0d = x0c.double()
    D = x0d + e.double() * (x0d - hist.double())
    d = raw.double() - D
    delta = -d if mean_type == X0 else d / Bc.double()
    halves = [torch.where(free, (h.double() + delta).float(), h) for h in ((c,) if scale is None else (c, u))]
    return torch.cat(halves, dim=0), new_hist
