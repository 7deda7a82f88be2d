"""Per-scene noise: the definition on the host, and the noise_fn of the seeded loops.

``z = scene_normal(seed, stream, draw, e)`` is a pure function -- nothing of the batch size, of a scene's position in the batch or of
earlier calls enters, so scene b of a seeded call can be regenerated alone, a batch can be split over calls or devices, and the batched
entry points reproduce what per-scene calls produce:

  q = e >> 2, lane = e & 3
  (r0, r1, r2, r3) = Philox4x32-10 on the counter (q, stream, draw & 0xffffffff, draw >> 32) under the key
                     (seed & 0xffffffff, seed >> 32); the seed is an int64 read as 64 bits.  Multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
                     constants 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped after every round
  u_i = (r_i >> 8) * 2^-24 + 2^-25.  In float32 the product is exact and the sum is rounded to nearest even for r_i >> 8 >= 2^23
        (there u needs 25 bits): u lies in (0, 1], and u == 1 gives rho == 0, never an infinity.  In float64 u is exact, in (0, 1)
  lanes 0, 1: rho = sqrt(-2 log(u0)), theta = (float32)(2 pi) * u1, z0 = rho cos(theta), z1 = rho sin(theta); lanes 2, 3: (u2, u3)

Element index: e = row * C + c inside the scene's own (rows, C) block -- main stream (0): rows = N; given stream (1): rows = Pmax in the
prefix loops, N in the masked loops.  e does not depend on Pmax, so a scene's given-part noise does not depend on the other scenes'
counts, and a whole-row prefix mask draws what the ragged completion loop draws.
Draw numbering: main stream -- x_T is draw 0, the loop's k-th step draw is draw k (the masked-out one at t == 0 of the T-step loops
included); given stream -- the loop's j-th partial / known draw is draw j, from 0.

The device evaluates the float32 definition (csrc/diffusion.hip, dsc_scene_randn_f32); ``reference_normals`` evaluates it in numpy.
"""
import numpy as np
import torch

from . import ops

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF
MAIN, GIVEN = 0, 1                     # stream ids


def philox4x32_10(counter, key):
    """Philox4x32-10: ``counter`` (..., 4) and ``key`` (..., 2) of 32-bit words (broadcast against each other) -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def philox_words(seed, stream, draw, count):
    """The raw word r_(e & 3) of elements e = 0 .. count - 1: (count,) uint32."""
    seed, draw, count = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1), int(count)
    quads = (count + 3) // 4
    counter = np.empty((quads, 4), dtype=np.uint64)
    counter[:, 0] = np.arange(quads, dtype=np.uint64)
    counter[:, 1], counter[:, 2], counter[:, 3] = int(stream), draw & _MASK, draw >> 32
    return philox4x32_10(counter, np.array([seed & _MASK, seed >> 32], dtype=np.uint64)).reshape(-1)[:count]


def normals_from_words(words, dtype=np.float64):
    """Box-Muller over whole quads of raw words ((4 k,) uint32), every operation in ``dtype``."""
    dtype = np.dtype(dtype).type
    w = np.asarray(words, dtype=np.uint32).reshape(-1, 2)
    u = (w >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24) + dtype(2.0 ** -25)
    rho = np.sqrt(dtype(-2.0) * np.log(u[:, 0]))
    theta = dtype(np.float32(2.0 * np.pi)) * u[:, 1]
    return np.stack([rho * np.cos(theta), rho * np.sin(theta)], axis=-1).reshape(-1)


def reference_normals(seed, stream, draw, count, dtype=np.float64):
    """scene_normal(seed, stream, draw, e) for e = 0 .. count - 1, every floating-point operation in ``dtype``: float32 is the
    definition the device implements, float64 the yardstick its rounding is measured against."""
    count = int(count)
    words = philox_words(seed, stream, draw, 4 * ((count + 3) // 4))
    return normals_from_words(words, dtype)[:count]


class SceneNoise:
    """noise_fn (protocol of diffusion_ddpm.py: ``noise_fn(size=, dtype=, device=)``) that draws scene b's noise from ``seeds[b]`` alone:
    every call is one dsc_scene_randn_f32 launch with the (stream, draw) of the loop's documented draw order.  Call 0 is x_T (main
    draw 0); a loop without a given part then makes main draws 1, 2, ...; a loop with one alternates the way RaggedNoiseReplay does --
    given draw j, main draw j + 1 -- whatever the two shapes are.  The eager loops arm it (``arm``) when they start, so one object
    serves one loop after another; the captured loops read ``seeds`` only (their draws are counted on the device).
    ``seeds``: what ops.scene_seeds accepts for a batch of len(seeds), or its result.  Repeated seeds give identical scenes."""

    def __init__(self, seeds, device):
        if not (isinstance(seeds, torch.Tensor) and seeds.dtype == torch.int64 and seeds.dim() == 1
                and seeds.device == torch.device(device)):
            seeds = ops.scene_seeds(seeds, len(seeds), device)
        self.seeds, self.device = seeds.contiguous(), seeds.device
        self.arm(False)

    def arm(self, given=False):
        """Start a new loop; ``given``: the loop draws for a given part in front of every model call."""
        self.given, self.calls, self.next_draw = bool(given), 0, [0, 0]
        return self

    def __call__(self, size=None, dtype=None, device=None):
        size = tuple(size)
        if size[0] != self.seeds.shape[0]:
            raise ValueError("SceneNoise holds %d seeds, the loop draws for %d scenes" % (self.seeds.shape[0], size[0]))
        stream = GIVEN if self.given and self.calls % 2 == 1 else MAIN
        self.calls += 1
        return self._draw(stream, size)

    def main_draw(self, size=None, dtype=None, device=None):
        """One more draw of the main stream that does not take a turn of the alternation: the draw of a resampling jump."""
        return self._draw(MAIN, tuple(size))

    def _draw(self, stream, size):
        draw = torch.full((1,), self.next_draw[stream], dtype=torch.int64, device=self.device)
        self.next_draw[stream] += 1
        return ops.scene_randn(self.seeds, draw, stream, size)
