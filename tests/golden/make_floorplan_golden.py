"""Generator of tests/golden/floorplan_wrapper.npz (build container only: it needs the reference tree; CPU, about a minute).

    python tests/golden/make_floorplan_golden.py

The REAL reference ``DiffusionSceneLayout_DDPM`` (loaded through the unchanged oracle.ref_loader) with ``room_mask_condition: true``,
paired with the plain-torch encoder of tests/floorplan_oracle.py -- the reference wrapper takes its feature extractor as a constructor
argument, and the reference's own one needs torchvision.  Weights by seed, as the other wrapper goldens: the denoiser and the wrapper-level
tensors from oracle.make_golden_wrapper.wrapper_state_dict, the encoder from floorplan_oracle.init_state_dict(ENC_SEED).

Cases: ``room`` (the floor plan is the only per-object condition) and ``roominst`` (``room_mask_condition`` and ``instance_condition``
together: pins the concatenation order [room | instance]).  Recorded per case: the condition handed to the diffusion, ``get_loss`` under
a fixed seed (loss and logged parts), and a seeded ``sample`` chain of SAMPLE_T steps at B scenes.
"""
import contextlib
import copy
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import floorplan_oracle as FO  # noqa: E402
from oracle import weights as W  # noqa: E402
from oracle.make_golden_wrapper import network_config, wrapper_state_dict  # noqa: E402

B, N, SIDE, SAMPLE_T, LATENT, FEATURE = 2, 12, 32, 10, 64, 64
ENC_SEED, SEED_LOSS, SEED_SAMPLE = 11, 2234, 2236
CASES = ("room", "roominst")
ENC_PREFIX = "feature_extractor."


def room_network_config(case, stats_file, time_num=1000):
    """The uncond ``network`` section of the reference with the floor-plan condition switched on."""
    cfg = copy.deepcopy(network_config("uncond", stats_file, time_num))
    cfg["room_mask_condition"] = True
    cfg["latent_dim"] = LATENT
    cfg["instance_condition"] = case == "roominst"
    cfg["net_kwargs"]["instanclass_dim"] = LATENT + (128 if case == "roominst" else 0)
    return cfg


def room_masks(b=B, side=SIDE, seed=5):
    """(b, 1, side, side) float32 masks, 1 inside an axis-aligned room that differs per scene."""
    rng = np.random.RandomState(seed)
    m = np.zeros((b, 1, side, side), dtype=np.float32)
    for i in range(b):
        y0, x0 = rng.randint(1, side // 3, size=2)
        y1, x1 = rng.randint(2 * side // 3, side - 1, size=2)
        m[i, 0, y0:y1, x0:x1] = 1.0
    return torch.from_numpy(m)


def room_batch():
    x = W.synth_scene_batch(B, N, 22, 32, seed=91)
    return {"translations": x[:, :, 0:3].contiguous(), "sizes": x[:, :, 3:6].contiguous(), "angles": x[:, :, 6:8].contiguous(),
            "class_labels": x[:, :, 8:30].contiguous(), "objfeats_32": x[:, :, 30:].contiguous(), "room_layout": room_masks()}


def room_state_dict(module):
    """Seeded values for ``module.state_dict()``: the encoder's entries from the oracle's seed, the rest as the other wrapper goldens."""
    class _Rest:
        def state_dict(self):
            return {k: v for k, v in module.state_dict().items() if not k.startswith(ENC_PREFIX)}
    sd = wrapper_state_dict(_Rest())
    sd.update({ENC_PREFIX + k: v for k, v in FO.init_state_dict(1, FEATURE, ENC_SEED).items()})
    return sd


def main():
    from oracle.ref_loader import load_reference_package
    torch.set_num_threads(os.cpu_count() or 8)
    mod = load_reference_package()["diffusion_scene_layout_ddpm"]
    stats_file = os.path.join(tempfile.mkdtemp(), "dataset_stats.txt")
    with open(stats_file, "w") as f:
        json.dump(W.DATASET_STATS, f)
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {}

    def build(case, time_num):
        cfg = room_network_config(case, stats_file, time_num)
        with quiet:
            m = mod.DiffusionSceneLayout_DDPM(cfg["class_dim"] + 1, FO.OracleEncoder(1, FEATURE, seed=ENC_SEED), cfg)
        sd = room_state_dict(m)
        m.feature_extractor.load_state_dict({k[len(ENC_PREFIX):]: v for k, v in sd.items() if k.startswith(ENC_PREFIX)})
        missing, unexpected = m.load_state_dict({k: v for k, v in sd.items() if not k.startswith(ENC_PREFIX)}, strict=False)
        assert not unexpected and all(k.startswith(ENC_PREFIX) for k in missing), (missing, unexpected)
        return m, cfg

    for case in CASES:
        m, cfg = build(case, 1000)
        s = room_batch()
        seen = {}
        inner = m.diffusion.get_loss_iter

        def spy(data, noises=None, condition=None, condition_cross=None):
            seen["condition"] = condition.detach().clone()
            return inner(data, noises=noises, condition=condition, condition_cross=condition_cross)
        m.diffusion.get_loss_iter = spy
        torch.manual_seed(SEED_LOSS)
        with torch.no_grad():
            loss, parts = m.get_loss(s)
        m.diffusion.get_loss_iter = inner
        out[case + ".condition"] = seen["condition"].numpy()
        out[case + ".loss"] = np.float32(loss.item())
        for k, v in parts.items():
            out[case + ".part." + k] = np.float32(v.item())
        m, cfg = build(case, SAMPLE_T)
        torch.manual_seed(SEED_SAMPLE)
        with torch.no_grad(), quiet:
            y = m.sample(room_masks(), N, cfg["point_dim"], batch_size=B, clip_denoised=True)
        out[case + ".sample"] = y.numpy()
        print("%-8s loss %.6f  condition %s  sample |mean| %.5f" % (case, out[case + ".loss"], tuple(seen["condition"].shape),
                                                                     float(y.abs().mean())))
    path = os.path.join(HERE, "floorplan_wrapper.npz")
    np.savez_compressed(path, **out)
    print("written", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
