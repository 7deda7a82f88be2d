#!/usr/bin/env python
"""Write the weight EMA of a training run as a model checkpoint that ``generate_diffusion.py --weight_file`` loads.

    python tools/export_ema.py CONFIG EXPERIMENT_DIR EPOCH        -> EXPERIMENT_DIR/model_ema_XXXXX

``train_diffusion.py`` with ``training: {ema_decay: ...}`` saves the average inside ``opt_XXXXX`` (``state[i]["ema"]``).  This tool
builds the network of CONFIG on the CPU, loads ``model_XXXXX`` (buffers and frozen parameters come from it), and replaces every
trainable parameter by its average from ``opt_XXXXX`` (``diffuscene_amd.optim.ema_model_state``).  No GPU is needed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def export(config, experiment_dir, epoch):
    import torch
    from diffuscene_amd.networks import build_network
    from diffuscene_amd.optim import ema_model_state
    model_path = os.path.join(experiment_dir, "model_{:05d}".format(epoch))
    opt_path = os.path.join(experiment_dir, "opt_{:05d}".format(epoch))
    out_path = os.path.join(experiment_dir, "model_ema_{:05d}".format(epoch))
    # n_classes does not shape any parameter (the class width is config["network"]["class_dim"])
    network, _, _ = build_network(None, config["network"].get("class_dim", 21) + 1, config, model_path, device="cpu")
    state = ema_model_state(network, torch.load(opt_path, map_location="cpu"))
    torch.save(state, out_path)
    return out_path


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config", help="the YAML file the run was trained with")
    ap.add_argument("experiment_dir", help="directory holding model_XXXXX and opt_XXXXX")
    ap.add_argument("epoch", type=int)
    args = ap.parse_args(argv)
    import yaml
    with open(args.config) as f:
        config = yaml.safe_load(f)
    print("wrote", export(config, args.experiment_dir, args.epoch))


if __name__ == "__main__":
    main()
