"""The argument checks of the thirteen sampling-step launchers of csrc/diffusion.hip (the ten step kernels and the three overwrites), on
the host: no device.  A fake non-null address is never dereferenced before a launch, and every call here carries exactly one defect, so
every call returns before one.  The optional pointers (x0_out, x_dup, and ca / cb with mean type x0) need a launch to be seen: the GPU
tests pass them."""
import pytest

P = 4096                                                   # any non-null address
EINVAL, ERANGE = -1, -3
EPS, X0, V = 0, 1, 2
INTS = dict(mean_type=V, clip=1, b=2, inner=8, n=4, pmax=2, p=2, c=3, S=5, T=10)        # a valid set: pmax, p <= n

# name -> its parameters in the order of include/diffuscene_hip.h, without the stream.  A name of INTS is that integer, ``name?`` a
# pointer that may be NULL, ca / cb are required unless mean_type is x0, every other name is a required pointer.
_POST = "ca cb coef1 coef2 sigma"
_STRIDED = "step times times_next sqrt_alpha_next c_noise sigma ca cb sqrt_recip_ac sqrt_recipm1_ac"
_Q = "sqrt_ac sqrt_1mac"
ENTRY_POINTS = {
    "dsc_p_sample_f32": "x_t model_out noise t %s out x0_out? mean_type clip b inner T" % _POST,
    "dsc_ddim_step_f32": "x_t model_out noise %s out x0_out? mean_type b inner S T" % _STRIDED,
    "dsc_p_sample_inpaint_f32": "x_t model_out noise partial noise_p counts t %s %s out mean_type clip b n pmax c T" % (_POST, _Q),
    "dsc_ddim_inpaint_step_f32": "x_t model_out noise partial noise_p counts %s %s out mean_type b n pmax c S T" % (_STRIDED, _Q),
    "dsc_p_sample_masked_f32": "x_t model_out noise known noise_k mask t %s %s out mean_type clip b inner T" % (_POST, _Q),
    "dsc_ddim_masked_step_f32": "x_t model_out noise known noise_k mask %s %s out mean_type b inner S T" % (_STRIDED, _Q),
    "dsc_p_sample_cfg_f32": "x_t model_out scale noise t %s out x_dup? x0_out? mean_type clip b inner T" % _POST,
    "dsc_ddim_cfg_step_f32": "x_t model_out scale noise %s out x_dup? x0_out? mean_type b inner S T" % _STRIDED,
    "dsc_p_sample_masked_cfg_f32": "x_t model_out scale noise known noise_k mask t %s %s out x_dup? mean_type clip b inner T" % (_POST, _Q),
    "dsc_ddim_masked_cfg_step_f32": "x_t model_out scale noise known noise_k mask %s %s out x_dup? mean_type b inner S T" % (_STRIDED, _Q),
    "dsc_complete_overwrite_f32": "x partial noise t %s b n p c T" % _Q,
    "dsc_complete_overwrite_ragged_f32": "x partial noise counts t %s b n pmax c T" % _Q,
    "dsc_masked_overwrite_f32": "x known noise mask t %s b inner T" % _Q,
}


def _call(name, **defect):
    from diffuscene_amd import _lib
    params = [a.rstrip("?") for a in ENTRY_POINTS[name].split()]
    assert defect and set(defect) <= set(params), (name, defect)                        # never a fully valid call
    assert len(params) + 1 == len(_lib.SIGNATURES[name][1]), name                       # the table above against the bound signature
    return _lib.fn(name)(*[defect[a] if a in defect else INTS.get(a, P) for a in params], None)


assert len(ENTRY_POINTS) == 13


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_every_step_launcher_checks_its_arguments_before_any_launch(name):
    params = ENTRY_POINTS[name].split()
    required = [a for a in params if not a.endswith("?") and a not in INTS and a not in ("ca", "cb")]
    for a in required:                                                                  # every required pointer nulled in turn
        assert _call(name, **{a: None}) == EINVAL, (name, a)
    if "mean_type" in params:
        for mt in (-1, 3):
            assert _call(name, mean_type=mt) == EINVAL, (name, mt)
        for mt in (EPS, V):
            for a in ("ca", "cb"):
                assert _call(name, mean_type=mt, **{a: None}) == EINVAL, (name, mt, a)
    for a in params:                                                                    # every size at 0 (clip is a flag)
        if a in INTS and a not in ("mean_type", "clip"):
            assert _call(name, **{a: 0}) == EINVAL, (name, a)
    for a in ("pmax", "p"):                                                             # more given rows than rows
        if a in params:
            assert _call(name, **{a: INTS["n"] + 1}) == EINVAL, (name, a)
    assert _call(name, b=65536) == ERANGE, name                                         # blockIdx.y carries the scene
