"""The float64 oracle, the rooms, the input generator and the margin condition of the floor-plan steering tests (tests/test_walls_host.py
on the CPU, tests/test_gpu_walls.py on the device).  Not a test module.

The oracle is the definition of INTEGRATION.md 9 written in torch: a brute-force distance field over the inside pixels of the mask,
rounded once to float32; the nine footprint points of every box of the clamped x0 estimate (sizes and angle detached); the bilinear
lookup with its quadratic continuation outside the image; the energy over valid boxes and autograd for its gradient."""
import functools

import torch

import steer_oracle as S

BBOX, CLASSES, C12, EMPTY, BOUNDS = S.BBOX, S.CLASSES, S.C12, S.EMPTY, S.BOUNDS
PIXEL_MARGIN = 1e-6                # pixels: every sample point keeps this distance from every integer u or v (the clamp bounds among them)
LOGIT_MARGIN = 1e-4                # the validity logit, normalised units
A9 = torch.tensor([-1., -1., -1., 0., 0., 0., 1., 1., 1.], dtype=torch.float64)         # the nine points in (a, b) order
B9 = torch.tensor([-1., 0., 1., -1., 0., 1., -1., 0., 1.], dtype=torch.float64)


def pixel_centres(h, w, side):
    """(x (w,), z (h,)) of the pixel centres, float64: the image covers [-side, side] along its columns (x) and its rows (z)."""
    s = float(torch.tensor(side, dtype=torch.float32))
    dx, dz = 2.0 * s / w, 2.0 * s / h
    return -s + (torch.arange(w, dtype=torch.float64) + 0.5) * dx, -s + (torch.arange(h, dtype=torch.float64) + 0.5) * dz


def room(kind, h, w, side, seed=0):
    """One (h, w) float32 mask, 1 inside.  'L': the square |x|, |z| < 2 without its quadrant x, z > 0; 'rect': |x| < 1.5, |z| < 1;
    'full' / 'none' / 'pixel' (one inside pixel) / 'random' (one pixel in three)."""
    x, z = pixel_centres(h, w, side)
    X, Z = x[None, :].expand(h, w), z[:, None].expand(h, w)
    if kind == "L":
        m = (X.abs() < 2) & (Z.abs() < 2) & ~((X > 0) & (Z > 0))
    elif kind == "rect":
        m = (X.abs() < 1.5) & (Z.abs() < 1.0)
    elif kind == "full":
        m = torch.ones(h, w, dtype=torch.bool)
    elif kind == "none":
        m = torch.zeros(h, w, dtype=torch.bool)
    elif kind == "pixel":
        m = torch.zeros(h, w, dtype=torch.bool)
        m[h // 3, (2 * w) // 3] = True
    else:
        m = torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) < 1 / 3
    return m.float()


def rooms(h, w, side):
    """(3, 1, h, w): a room per scene -- the L, the rectangle, the L mirrored in x."""
    return torch.stack([room("L", h, w, side), room("rect", h, w, side), room("L", h, w, side).flip(-1)])[:, None].contiguous()


def field(mask, side):
    """mask (..., h, w), inside iff > 0.5 -> the field of the definition, (..., h, w) float32: half the squared distance, metres^2, from
    each pixel centre to the nearest inside one by brute force in float64, rounded once; 0 where the mask has no inside pixel."""
    lead, (h, w) = mask.shape[:-2], mask.shape[-2:]
    s = float(torch.tensor(side, dtype=torch.float32))
    dx, dz = 2.0 * s / w, 2.0 * s / h
    out = torch.zeros(mask.reshape(-1, h, w).shape, dtype=torch.float32)
    ii, jj = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    for b, m in enumerate(mask.reshape(-1, h, w)):
        inside = m > 0.5
        if not bool(inside.any()):
            continue
        i_in, j_in = ii[inside], jj[inside]
        for r in range(h):                                                      # one image row at a time: (w, inside pixels)
            d2 = ((r - i_in)[None, :] * dz) ** 2 + ((jj[r][:, None] - j_in[None, :]) * dx) ** 2
            out[b, r] = (0.5 * d2.min(dim=1).values).float()
    return out.reshape(*lead, h, w)


def points(x, bounds=BOUNDS):
    """Clamped x0 (B, N, C) float64 -> (px, pz) (B, N, 9), metres: centre_xz + R (a sx, b sz), R the rotation about y by the (cos, sin)
    channels over their hypot (a zero pair: angle 0).  Gradient flows through the centre only."""
    bd = torch.tensor(bounds, dtype=torch.float32).double()
    c_lo, c_hi, s_lo, s_hi = bd[0:3], bd[3:6], bd[6:9], bd[9:12]
    ctr = (x[..., 0:3] + 1) / 2 * (c_hi - c_lo) + c_lo
    siz = ((x[..., 3:6] + 1) / 2 * (s_hi - s_lo) + s_lo).detach()
    c, s = x[..., 6].detach(), x[..., 7].detach()
    hyp = torch.hypot(c, s)
    safe = torch.where(hyp > 0, hyp, torch.ones_like(hyp))
    c, s = torch.where(hyp > 0, c / safe, torch.ones_like(c)), torch.where(hyp > 0, s / safe, torch.zeros_like(s))
    lx, lz = A9 * siz[..., 0:1], B9 * siz[..., 2:3]
    px = ctr[..., 0:1] + (c[..., None] * lx - s[..., None] * lz)
    pz = ctr[..., 2:3] + (s[..., None] * lx + c[..., None] * lz)
    return px, pz


def pixel_coords(px, pz, h, w, side):
    s = float(torch.tensor(side, dtype=torch.float32))
    dx, dz = 2.0 * s / w, 2.0 * s / h
    return (px + s) / dx - 0.5, (pz + s) / dz - 0.5, dx, dz


def point_energy(px, pz, fld, side):
    """e(p) of the definition for points (B, N, 9) over the float32 field (B or 1, h, w)."""
    h, w = fld.shape[-2:]
    B = px.shape[0]
    F = fld.double().expand(B, h, w)
    u, v, dx, dz = pixel_coords(px, pz, h, w, side)
    uc, vc = u.clamp(0, w - 1), v.clamp(0, h - 1)
    j0, i0 = uc.detach().floor().clamp(max=w - 2).long(), vc.detach().floor().clamp(max=h - 2).long()
    fu, fv = uc - j0, vc - i0
    bi = torch.arange(B)[:, None, None].expand_as(j0)
    f00, f01, f10, f11 = F[bi, i0, j0], F[bi, i0, j0 + 1], F[bi, i0 + 1, j0], F[bi, i0 + 1, j0 + 1]
    bil = f00 * (1 - fv) * (1 - fu) + f01 * (1 - fv) * fu + f10 * fv * (1 - fu) + f11 * fv * fu
    return bil + 0.5 * ((u - uc) * dx) ** 2 + 0.5 * ((v - vc) * dz) ** 2


def energy_grad(x0, mask, side, bounds=BOUNDS):
    """x0 (B, N, C), clamped here; mask (B or 1, 1, h, w) -> (E (B,), g (B, N, 3) = dE / d x0[:, :, 0:3] with a zero y column,
    outside (B,) = the number of valid boxes with a point of e > 0), float64."""
    x = x0.detach().double().clamp(-1, 1).requires_grad_(True)
    fld = field(mask[:, 0], side)
    e = point_energy(*points(x, bounds), fld, side)
    valid = x[..., EMPTY] < 0
    E = (e.sum(-1) / 9 * valid).sum(-1)
    g, = torch.autograd.grad(E.sum(), x)
    assert float(g[..., 1].abs().max()) == 0.0 and float(g[..., 3:].abs().max()) == 0.0
    return E.detach(), g[..., 0:3].detach(), (valid & (e.detach() > 0).any(-1)).sum(-1)


def step(x0, mask, side, w):
    """clamp(x0) - w[b] g in channels 0 and 2: the x0 the unchanged step forms after the launch, float64."""
    x = x0.detach().double().clamp(-1, 1)
    x[..., 0:3] -= torch.as_tensor(w, dtype=torch.float64).reshape(-1, 1, 1) * energy_grad(x0, mask, side)[1]
    return x


def margins(x0, h, w, side):
    """(the smallest distance in pixels of a sample point of a valid box from an integer u or v, the smallest |empty logit|)."""
    x = x0.detach().double().clamp(-1, 1)
    u, v, _, _ = pixel_coords(*points(x), h, w, side)
    valid = (x[..., EMPTY] < 0)[..., None].expand_as(u)
    d = torch.minimum((u - u.round()).abs(), (v - v.round()).abs())
    pix = float(d[valid].min()) if bool(valid.any()) else float("inf")
    return pix, float(x0[..., EMPTY].abs().min())


def assert_margins(x0, mask, side, what, want_outside=True):
    """The condition on the inputs: no decision of the point energy -- the cell, the clamp, validity -- hangs on a rounding.  With
    ``want_outside`` the batch must also hold a valid box with a point outside its room."""
    h, w = mask.shape[-2:]
    pix, logit = margins(x0, h, w, side)
    assert pix >= PIXEL_MARGIN and logit >= LOGIT_MARGIN, (what, pix, logit)
    if want_outside:
        assert int(energy_grad(x0, mask, side)[2].sum()) >= 1, (what, "no valid box with a point outside the room")


def outside_image(x0, h, w, side):
    """The number of sample points of valid boxes that lie outside the image."""
    x = x0.detach().double().clamp(-1, 1)
    u, v, _, _ = pixel_coords(*points(x), h, w, side)
    out = (u < 0) | (u > w - 1) | (v < 0) | (v > h - 1)
    return int((out & (x[..., EMPTY] < 0)[..., None]).sum())


def make_scenes(n, seed, b=3, c=C12, spread=1.0):
    """steer_oracle.make_scenes with the translations of its n <= 16 branch (+-0.25 there, +-0.75 m) widened to +-``spread``: centres
    over the whole +-3 m of BOUNDS, so that boxes reach outside the rooms; n > 16 already spans +-1.2 (some beyond the clamp)."""
    x = S.make_scenes(n, seed, b=b, c=c)
    if n <= 16:
        x[..., 0:3] = x[..., 0:3] * (spread / 0.25)
    return x.contiguous()


# (h, w, room_side) of the device tests; the last has sample points outside the image (2 m against the +-3 m of BOUNDS)
ROOMS = ((64, 64, 3.1), (16, 16, 3.1), (8, 12, 3.1), (16, 16, 2.0))


@functools.lru_cache(maxsize=None)
def case(n, seed, h, w, side):
    """(scenes, masks (3, 1, h, w), E, g, outside) of one device case, computed once; the margin condition is asserted here."""
    x, m = make_scenes(n, seed), rooms(h, w, side)
    assert_margins(x, m, side, (n, seed, h, w, side))
    return (x, m) + energy_grad(x, m, side)


rel_err = S.rel_err
