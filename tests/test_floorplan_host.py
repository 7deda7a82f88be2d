"""CPU: the floor-plan encoder's host side -- construction through build_network, the state-dict contract with a reference checkpoint,
the refusals, and the float64 oracle's own frozen BN.  No kernel runs here."""
import copy

import pytest
import torch

from oracle import weights as W

import floorplan_oracle as FO

LATENT = 64


def room_config(instance=True, latent=LATENT, feature_size=64, input_channels=1, **fe):
    kw = dict(W.UNCOND_BEDROOM)
    kw["instanclass_dim"] = latent + (128 if instance else 0)
    net = {"type": "diffusion_scene_layout_ddpm", "net_type": "unet1d", "point_dim": 62, "latent_dim": latent,
           "room_mask_condition": True, "sample_num_points": 12, "objectness_dim": 0, "objfeat_dim": 32,
           "class_dim": 22, "angle_dim": 2, "learnable_embedding": True, "instance_condition": instance,
           "instance_emb_dim": 128,
           "diffusion_kwargs": dict(schedule_type="linear", beta_start=1e-4, beta_end=0.02, time_num=1000,
                                    loss_type="mse", model_mean_type="v", model_var_type="fixedsmall",
                                    loss_separate=True, loss_iou=False, train_stats_file=None),
           "net_kwargs": kw}
    feat = dict(name="resnet18", freeze_bn=True, input_channels=input_channels, feature_size=feature_size)
    feat.update(fe)
    return {"network": net, "feature_extractor": feat}


def test_build_network_constructs_a_floor_plan_conditioned_model():
    from diffuscene_amd.networks import build_network
    from diffuscene_amd.networks.feature_extractors import ResNet18
    net, train, val = build_network(62, 23, room_config())
    assert isinstance(net.feature_extractor, ResNet18) and net.feature_extractor.feature_size == 64
    assert net.fc_room_f.in_features == 64 and net.fc_room_f.out_features == LATENT
    # the reference's default for a config that leaves the key out is True: the same model
    cfg = room_config()
    del cfg["network"]["room_mask_condition"]
    net2, _, _ = build_network(62, 23, cfg)
    assert set(net2.state_dict()) == set(net.state_dict())
    assert callable(train) and callable(val)


@pytest.mark.parametrize("input_channels,feature_size", [(1, 64), (2, 128)])
def test_state_dict_is_the_reference_key_list(input_channels, feature_size):
    from diffuscene_amd.networks.feature_extractors import get_feature_extractor
    enc = get_feature_extractor("resnet18", freeze_bn=True, input_channels=input_channels, feature_size=feature_size)
    want = FO.key_shapes(input_channels, feature_size)
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == want
    assert len(want) == 1 + 4 + 8 * 10 + 3 * 5 + 4
    assert not any("num_batches_tracked" in k for k in want)
    buffers = {k for k, _ in enc.named_buffers()}
    params = {k for k, p in enc.named_parameters() if p.requires_grad}
    assert buffers == {k for k in want if k.endswith("running_mean") or k.endswith("running_var")}
    assert params == set(want) - buffers              # frozen-BN weight and bias are trainable, as in the reference
    assert enc.feature_size == feature_size


def test_initial_values_follow_the_reference_distributions():
    from diffuscene_amd.networks.feature_extractors import get_feature_extractor
    torch.manual_seed(0)
    sd = get_feature_extractor("resnet18", freeze_bn=True, input_channels=1, feature_size=64).state_dict()
    p = "_feature_extractor."
    for k, v in sd.items():
        if k.endswith("running_var"):
            assert torch.equal(v, torch.ones_like(v) + 1e-5)
        elif k.endswith("running_mean") or (k.endswith(".bias") and "fc." not in k):
            assert not v.any()
        elif k.endswith(".weight") and v.dim() == 1:
            assert torch.equal(v, torch.ones_like(v))
    w = sd[p + "layer3.0.conv2.weight"]                                   # Kaiming normal, fan_out, ReLU gain: std = sqrt(2 / (O k k))
    assert abs(float(w.std()) / (2.0 / (256 * 9)) ** 0.5 - 1.0) < 0.02
    w = sd[p + "conv1.weight"]                                            # torch's Conv2d default: U(-b, b), b = 1 / sqrt(fan_in)
    assert float(w.abs().max()) <= 1.0 / 7.0 and float(w.abs().max()) > 0.9 / 7.0
    w = sd[p + "fc.2.weight"]                                             # torch's Linear default: U(-b, b), b = 1 / sqrt(512)
    assert float(w.abs().max()) <= 512 ** -0.5 and float(w.abs().max()) > 0.95 * 512 ** -0.5


def test_state_dict_round_trips_between_oracle_and_module():
    from diffuscene_amd.networks.feature_extractors import get_feature_extractor
    enc = get_feature_extractor("resnet18", freeze_bn=True, input_channels=1, feature_size=64)
    oracle = FO.OracleEncoder(1, 64, seed=3)
    enc.load_state_dict(oracle.state_dict(), strict=True)
    for k, v in oracle.state_dict().items():
        assert torch.equal(enc.state_dict()[k], v), k
    other = FO.OracleEncoder(1, 64, seed=4)
    other.load_state_dict(copy.deepcopy(enc.state_dict()))
    x = torch.rand(2, 1, 16, 16)
    with torch.no_grad():
        assert torch.equal(other(x), oracle(x))


def test_refusals_name_the_key():
    from diffuscene_amd.networks import build_network
    from diffuscene_amd.networks.feature_extractors import get_feature_extractor
    with pytest.raises(NotImplementedError, match="alexnet"):
        get_feature_extractor("alexnet", freeze_bn=True)
    with pytest.raises(NotImplementedError, match="freeze_bn"):
        get_feature_extractor("resnet18", freeze_bn=False)
    with pytest.raises(NotImplementedError, match="alexnet"):
        build_network(62, 23, room_config(name="alexnet"))
    with pytest.raises(NotImplementedError, match="freeze_bn"):
        build_network(62, 23, room_config(freeze_bn=False))


def test_forward_refuses_bad_inputs_before_any_kernel():
    from diffuscene_amd.networks.feature_extractors import get_feature_extractor
    enc = get_feature_extractor("resnet18", freeze_bn=True, input_channels=1, feature_size=64)
    for bad in (torch.zeros(2, 1, 7, 16), torch.zeros(2, 1, 16, 257), torch.zeros(2, 2, 16, 16), torch.zeros(1, 16, 16),
                torch.zeros(2, 1, 16, 16, dtype=torch.float64)):
        with pytest.raises(ValueError):
            enc(bad)
    with pytest.raises(RuntimeError, match="HIP device"):               # a CPU tensor raises like the rest of the package
        enc(torch.zeros(2, 1, 16, 16))


def test_room_mask_batch_is_checked_before_anything_is_drawn():
    from diffuscene_amd.networks import build_network
    net, _, _ = build_network(62, 23, room_config())
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match="room_mask holds 2 rooms for a batch of 3"):
        net.generate_layout_batched(torch.zeros(2, 1, 16, 16), 12, 62, 3)
    with pytest.raises(ValueError, match="room_mask"):
        net.sample(torch.zeros(16, 16), 12, 62, batch_size=1)
    assert torch.equal(torch.random.get_rng_state(), state)


def test_plan_supported_keeps_refusing_the_model():
    from diffuscene_amd.networks import build_network
    from diffuscene_amd.train_step import plan_supported
    net, _, _ = build_network(62, 23, room_config())
    assert plan_supported(net) is False


def test_oracle_frozen_bn_at_construction_is_the_affine_map():
    sd = FO.fresh_state_dict(1, 64)
    x = torch.randn(2, 64, 3, 5, dtype=torch.float64)
    y = FO.frozen_bn(x, sd, "_feature_extractor.bn1.")
    assert torch.equal(y, x * torch.tensor(1.0 + 1e-5, dtype=torch.float64).rsqrt())
    sd = FO.init_state_dict(1, 64, seed=0, dtype=torch.float64)
    p = "_feature_extractor.layer2.0.downsample.1."
    x = torch.randn(2, 128, 3, 5, dtype=torch.float64)
    s = sd[p + "weight"] / sd[p + "running_var"].sqrt()
    want = (x - sd[p + "running_mean"].view(1, -1, 1, 1)) * s.view(1, -1, 1, 1) + sd[p + "bias"].view(1, -1, 1, 1)
    assert torch.allclose(FO.frozen_bn(x, sd, p), want, rtol=1e-13, atol=1e-13)
