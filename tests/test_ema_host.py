"""Weight EMA on the host (no kernel runs): the three C symbols, FusedAdam's unchanged face with EMA off and on, the refusals of
``ema_decay``, the warm-up sequence, checkpoint compatibility in both directions, ``ema_model_state`` on a CPU module,
``optimizer_factory`` with and without the keys, and tools/export_ema.py on files written here."""
import copy
import os
import re
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsc_adam_ema_step_f32", "dsc_ema_update_f32", "dsc_ema_swap_f32")


def _params():
    return [torch.nn.Parameter(torch.arange(12.0).reshape(3, 4)), torch.nn.Parameter(torch.ones(5))]


def test_header_declares_and_library_exports_the_new_symbols():
    from diffuscene_amd import _lib, optim
    hdr = open(os.path.join(ROOT, "include", "diffuscene_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dsc_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, "%s not declared in include/diffuscene_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(lib, name), "%s not exported / bound" % name
    assert len(_lib.SIGNATURES["dsc_adam_ema_step_f32"][1]) == len(_lib.SIGNATURES["dsc_adam_step_f32"][1]) + 2      # + ema, ema_decay
    assert "typedef struct dsc_optim_chunk {\n    float* param;\n    const float* grad;\n    float* exp_avg;\n    float* exp_avg_sq;\n" \
           "    int64_t count;\n} dsc_optim_chunk;" in hdr                                                            # unchanged
    for name in ("ParamEMA", "ema_model_state", "ema_decay_at"):
        assert callable(getattr(optim, name))


@pytest.mark.parametrize("kw", [{}, {"ema_decay": None}, {"ema_decay": 0.999}, {"ema_decay": 0.0, "ema_warmup": True}])
def test_fused_adam_keeps_torch_adams_face(kw):
    """The EMA settings are attributes: the group keys are torch.optim.Adam's whether the average is on or off, and a fresh optimizer
    has no state (so no EMA keys) either way."""
    from diffuscene_amd.optim import FusedAdam
    opt = FusedAdam(_params(), lr=2e-4, **kw)
    ref = torch.optim.Adam(_params(), lr=2e-4)
    assert set(opt.param_groups[0].keys()) == set(ref.param_groups[0].keys())
    sd = opt.state_dict()
    assert sd["state"] == {} and set(sd["param_groups"][0].keys()) == set(ref.state_dict()["param_groups"][0].keys())
    assert opt.ema_decay == kw.get("ema_decay") and opt.ema_warmup == kw.get("ema_warmup", False) and opt.ema_swapped is False
    ref.load_state_dict(sd)


def test_no_ema_state_keys_when_off():
    from diffuscene_amd.optim import FusedAdam
    ps = _params()
    opt = FusedAdam(ps, lr=1e-3)
    sd = torch.optim.Adam(ps, lr=1e-3).state_dict()
    sd["state"] = {i: {"step": torch.tensor(2.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)} for i, p in enumerate(ps)}
    with warnings.catch_warnings():
        warnings.simplefilter("error")                        # nothing to drop: no warning
        opt.load_state_dict(copy.deepcopy(sd))
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in opt.state_dict()["state"].values())
    with pytest.raises(RuntimeError, match="ema_decay=None"):
        opt.ema_swap()


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), "x"])
def test_ema_decay_outside_the_half_open_unit_interval_is_refused(bad):
    from diffuscene_amd.optim import FusedAdam, ParamEMA
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdam(_params(), ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        ParamEMA(_params(), bad)


def test_warmup_needs_a_decay():
    from diffuscene_amd.optim import FusedAdam
    with pytest.raises(ValueError, match="ema_warmup"):
        FusedAdam(_params(), ema_warmup=True)


@pytest.mark.parametrize("d", [0.9999, 0.5, 0.0])
def test_warmup_sequence(d):
    from diffuscene_amd.optim import ema_decay_at
    for k in range(21):
        assert ema_decay_at(d, True, k) == min(d, (1 + k) / (10 + k))
        assert ema_decay_at(d, False, k) == d
    assert ema_decay_at(0.9999, True, 0) == 0.1 and ema_decay_at(0.9999, True, 10 ** 6) == 0.9999


def _state_dict_with_ema(ps):
    sd = torch.optim.Adam(ps, lr=1e-3).state_dict()
    sd["state"] = {i: {"step": torch.tensor(3.0), "exp_avg": torch.full_like(p, 0.1), "exp_avg_sq": torch.full_like(p, 0.01),
                       "ema": p.detach() * 0.5, "ema_step": torch.tensor(3.0)} for i, p in enumerate(ps)}
    return sd


def test_checkpoint_with_the_average_loads_into_plain_torch_adam_which_steps():
    ps = _params()
    ref = torch.optim.Adam(ps, lr=1e-3)
    ref.load_state_dict(copy.deepcopy(_state_dict_with_ema(ps)))
    before = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad = torch.ones_like(p)
    ref.step()
    assert all(not torch.equal(p, b) for p, b in zip(ps, before))
    assert float(ref.state[ps[0]]["step"]) == 4.0


def test_checkpoint_with_the_average_into_fused_adam_without_ema_warns_once_and_drops_it():
    from diffuscene_amd.optim import FusedAdam
    ps = _params()
    opt = FusedAdam(ps, lr=1e-3)
    with pytest.warns(UserWarning, match="weight EMA") as rec:
        opt.load_state_dict(copy.deepcopy(_state_dict_with_ema(ps)))
    assert len(rec) == 1
    sd = opt.state_dict()
    assert len(sd["state"]) == 2 and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    assert float(sd["state"][0]["step"]) == 3.0


def test_checkpoint_round_trips_through_fused_adam_with_ema():
    from diffuscene_amd.optim import FusedAdam
    ps = _params()
    src = _state_dict_with_ema(ps)
    opt = FusedAdam(ps, lr=1e-3, ema_decay=0.9)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        opt.load_state_dict(copy.deepcopy(src))
    sd = opt.state_dict()
    for i, p in enumerate(ps):
        assert set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq", "ema", "ema_step"}
        assert torch.equal(sd["state"][i]["ema"], src["state"][i]["ema"]) and sd["state"][i]["ema"].shape == p.shape
        e = sd["state"][i]["ema_step"]
        assert e.dim() == 0 and e.dtype == torch.float32 and float(e) == 3.0
    # a checkpoint without the keys loads as well; the average then starts at the next step
    plain = copy.deepcopy(src)
    for st in plain["state"].values():
        del st["ema"], st["ema_step"]
    opt2 = FusedAdam(ps, lr=1e-3, ema_decay=0.9)
    opt2.load_state_dict(plain)
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in opt2.state_dict()["state"].values())


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(3, 2)
        self.frozen = torch.nn.Parameter(torch.full((4,), 7.0), requires_grad=False)
        self.b = torch.nn.Linear(2, 1, bias=False)
        self.register_buffer("table", torch.arange(5.0))


def test_ema_model_state_on_cpu():
    from diffuscene_amd.optim import FusedAdam, ema_model_state
    torch.manual_seed(0)
    m = _Tiny()
    trainable = [p for p in m.parameters() if p.requires_grad]                    # a.weight, a.bias, b.weight: the filter order
    assert [tuple(p.shape) for p in trainable] == [(2, 3), (2,), (1, 2)]
    sd = torch.optim.Adam(trainable, lr=1e-3).state_dict()
    avgs = [torch.full_like(p, float(i + 1)) for i, p in enumerate(trainable)]
    sd["state"] = {i: {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p), "ema": avgs[i],
                       "ema_step": torch.tensor(1.0)} for i, p in enumerate(trainable)}
    want = {k: v.clone() for k, v in m.state_dict().items()}
    out = ema_model_state(m, sd)
    assert list(out) == list(want)
    assert torch.equal(out["a.weight"], avgs[0]) and torch.equal(out["a.bias"], avgs[1]) and torch.equal(out["b.weight"], avgs[2])
    assert torch.equal(out["frozen"], want["frozen"]) and torch.equal(out["table"], want["table"])
    assert all(torch.equal(v, want[k]) for k, v in m.state_dict().items())        # the model itself is untouched
    out["a.weight"].zero_()
    assert torch.equal(avgs[0], torch.full((2, 3), 1.0))                          # ... and the result owns its storage
    _Tiny().load_state_dict(out)
    # a live optimizer gives the same
    live = FusedAdam(trainable, lr=1e-3, ema_decay=0.9)
    live.load_state_dict(copy.deepcopy(sd))
    out2 = ema_model_state(m, live)
    assert all(torch.equal(out2[k], v) for k, v in ema_model_state(m, sd).items())
    # a parameter without an average is named
    del sd["state"][1]["ema"]
    with pytest.raises(ValueError, match="a.bias"):
        ema_model_state(m, sd)
    with pytest.raises(ValueError, match="a.weight"):
        ema_model_state(m, FusedAdam(trainable, lr=1e-3, ema_decay=0.9))
    with pytest.raises(ValueError, match="holds 2 parameters"):
        ema_model_state(m, torch.optim.Adam(trainable[:2], lr=1e-3).state_dict())


def test_optimizer_factory_with_and_without_the_keys():
    from diffuscene_amd.networks import optimizer_factory
    from diffuscene_amd.optim import FusedAdam, ParamEMA
    for name, cls in (("Adam", FusedAdam), ("SGD", torch.optim.SGD), ("RAdam", torch.optim.RAdam)):
        plain = optimizer_factory({"optimizer": name, "lr": 1e-3}, iter(_params()))
        assert type(plain) is cls and not hasattr(plain, "ema") and "step" not in vars(plain)
        if name == "Adam":
            assert plain.ema_decay is None
        ps = _params()
        opt = optimizer_factory({"optimizer": name, "lr": 1e-3, "ema_decay": 0.9999, "ema_warmup": True}, iter(ps))     # (a filter object)
        assert type(opt) is cls and len(opt.param_groups[0]["params"]) == 2
        if name == "Adam":
            assert opt.ema_decay == 0.9999 and opt.ema_warmup is True and not hasattr(opt, "ema")
        else:
            assert isinstance(opt.ema, ParamEMA) and opt.ema.decay == 0.9999 and opt.ema.warmup is True
            assert all(a is b for a, b in zip(opt.ema.params, ps)) and opt.ema.swapped is False and "step" in vars(opt)
            for p in ps:
                p.grad = torch.ones_like(p)
            with pytest.raises(RuntimeError, match="no CPU fallback"):            # step() reaches the average: CPU tensors are refused
                opt.step()
        with pytest.raises(ValueError, match="ema_decay"):
            optimizer_factory({"optimizer": name, "ema_decay": 1.0}, iter(_params()))
        with pytest.raises(ValueError, match="ema_warmup"):
            optimizer_factory({"optimizer": name, "ema_warmup": True}, iter(_params()))


def test_param_ema_starts_as_a_copy_and_round_trips_its_state():
    from diffuscene_amd.optim import ParamEMA, ema_model_state
    ps = _params()
    ema = ParamEMA(iter(ps), 0.9, warmup=True)
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(ema.shadow, ps)) and ema.num_updates == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ema.update()
    sd = ema.state_dict()
    sd["shadow"] = [e + 1.0 for e in sd["shadow"]]
    sd["num_updates"] = 5
    other = ParamEMA(ps, 0.9, warmup=True)
    other.load_state_dict(sd)
    assert other.num_updates == 5 and all(torch.equal(e, p + 1.0) for e, p in zip(other.shadow, ps))
    with pytest.raises(ValueError, match="1 averages for 2"):
        other.load_state_dict({"num_updates": 0, "shadow": sd["shadow"][:1]})
    lin = torch.nn.Linear(4, 3)                                   # ema_model_state reads a ParamEMA (or an optimizer carrying one) too
    lin.weight.data, lin.bias.data = ps[0].data, torch.ones(3)
    got = ema_model_state(lin, ParamEMA(lin.parameters(), 0.5))
    assert torch.equal(got["weight"], ps[0]) and torch.equal(got["bias"], torch.ones(3))


def test_export_ema_writes_the_averaged_checkpoint(tmp_path):
    """tools/export_ema.py on files written here: model_XXXXX + opt_XXXXX -> model_ema_XXXXX, through build_network on the CPU."""
    import contextlib
    import io
    import json
    from oracle import weights as W
    from diffuscene_amd.networks import build_network
    from tools.export_ema import export
    stats = tmp_path / "dataset_stats.txt"
    stats.write_text(json.dumps(W.DATASET_STATS))
    net = {"type": "diffusion_scene_layout_ddpm", "net_type": "unet1d", "point_dim": 62, "latent_dim": 0, "room_mask_condition": False,
           "sample_num_points": 12, "objectness_dim": 0, "objfeat_dim": 32, "class_dim": 22, "angle_dim": 2, "learnable_embedding": True,
           "instance_condition": True, "instance_emb_dim": 128,
           "diffusion_kwargs": dict(schedule_type="linear", beta_start=1e-4, beta_end=0.02, time_num=1000, loss_type="mse",
                                    model_mean_type="v", model_var_type="fixedsmall", loss_separate=True, loss_iou=True,
                                    train_stats_file=str(stats)),
           "net_kwargs": dict(W.UNCOND_BEDROOM)}
    config = {"network": net}
    with contextlib.redirect_stdout(io.StringIO()):
        m, _, _ = build_network(None, 23, config, None, device="cpu")
    trainable = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    sd = torch.optim.Adam([p for _, p in trainable], lr=1e-3).state_dict()
    sd["state"] = {i: {"step": torch.tensor(1.0), "ema": p.detach() + 1.0, "ema_step": torch.tensor(1.0)} for i, (_, p) in enumerate(trainable)}
    torch.save(m.state_dict(), str(tmp_path / "model_00007"))
    torch.save(sd, str(tmp_path / "opt_00007"))
    with contextlib.redirect_stdout(io.StringIO()):
        out = export(config, str(tmp_path), 7)
    assert out == str(tmp_path / "model_ema_00007")
    got, raw = torch.load(out), m.state_dict()
    names = {n for n, _ in trainable}
    assert list(got) == list(raw) and names
    for k in raw:
        assert torch.equal(got[k], raw[k] + 1.0 if k in names else raw[k]), k
