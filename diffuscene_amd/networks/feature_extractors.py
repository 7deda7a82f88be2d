"""Floor-plan image encoder -- drop-in for scene_synthesis/networks/feature_extractors.py (``get_feature_extractor``, ``ResNet18``).

The reference wraps ``torchvision.models.resnet18`` (BatchNorm frozen into ``FrozenBatchNorm2d``, a ``conv1`` for the mask's channels, a
two-layer head).  This module is that network on this package's HIP kernels, forward and backward, with the state_dict keys a reference
checkpoint carries below ``_feature_extractor.``; torchvision is not needed.  The key list and the topology come from torchvision's
published module tree, not from an import of it.

Images travel channel-last, token-major ``[b * h * w][c]`` with their geometry ``(b, h, w)`` beside them -- the layout of every GEMM
operand of the package.  A convolution is a patch gather (dsc_conv_patches_f32), the exact-f32 GEMM and the fused frozen-BN / residual /
ReLU epilogue (dsc_frozen_bn_act_f32); its backward re-gathers the patches for the weight gradient (``ops.gemm_tn``) instead of keeping
them.  Nothing derived from a weight is cached: the (O, kh, kw, I) row form of a convolution weight and its K padding are redone on
every call, so optimizer steps, ``ema_weights()`` swaps and ``load_state_dict`` need no invalidation.

Not built (NotImplementedError naming the key): ``name: alexnet`` and ``freeze_bn: false`` (every shipped YAML says true).
"""
import math

import torch
import torch.nn as nn
from torch.autograd import Function

from .. import ops
from ..autograd_ops import LinearFn, _dense

MIN_SIDE, MAX_SIDE = 8, 256
STAGES = (64, 128, 256, 512)
K_CHUNK = 576           # longest K run one convolution GEMM accumulates (64 channels x 9 taps)


def _weight_rows(weight):
    """(O, I, kh, kw) -> [O][(ky, kx, i)] zero-padded to the patch row length (ops.conv_kpad): the W operand of the convolution GEMM."""
    o, i, k, _ = weight.shape
    rows = weight.permute(0, 2, 3, 1).reshape(o, k * k * i)
    kpad = ops.conv_kpad(i, k)
    if kpad == rows.shape[1]:
        return rows.contiguous()
    out = torch.zeros((o, kpad), device=weight.device, dtype=weight.dtype)
    out[:, :rows.shape[1]].copy_(rows)
    return out


def _row_invariant():
    """Outside autograd (sampling) the encoder's GEMMs are pinned row-invariant: a room encoded alone gives, bit for bit, the features it
    gives inside any batch, so one mask expanded over B layouts equals the mask repeated B times."""
    return not torch.is_grad_enabled()


def _conv_gemm(patches, rows):
    """patches @ rows.T with the K sum blocked: the exact-f32 GEMM adds its K terms one after the other, so the 1152- to 4608-long sums
    of stages 2 to 4 are taken K_CHUNK columns at a time and the partial products added (the blocked sum LinearFn.backward uses for its
    long reductions, and what a CPU BLAS does with its K loop); every launch keeps the caller's row-invariance."""
    k = patches.shape[1]
    if k <= K_CHUNK:
        return ops.gemm(patches, rows, row_invariant=_row_invariant())
    y = None
    for c0 in range(0, k, K_CHUNK):
        c1 = min(c0 + K_CHUNK, k)
        y = ops.gemm(patches[:, c0:c1], rows[:, c0:c1], residual=y, row_invariant=_row_invariant())
    return y


class ConvFn(Function):
    """y [b * ho * wo][O] = conv2d(x [b * h * w][I], weight (O, I, k, k)), no bias"""

    @staticmethod
    def forward(ctx, x, weight, geom, stride, pad):
        k = weight.shape[2]
        patches = ops.conv_patches(x, geom, k, stride, pad)
        y = _conv_gemm(patches, _weight_rows(weight))
        ctx.save_for_backward(x, weight)
        ctx.cfg = (geom, stride, pad)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        geom, stride, pad = ctx.cfg
        o, i, k, _ = weight.shape
        dyd = _dense(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dpatches = ops.gemm(dyd, ops.transpose(_weight_rows(weight)))          # [rows, kpad] = dy @ W
            dx = ops.conv_patches_bwd(dpatches, geom, i, k, stride, pad)
        if ctx.needs_input_grad[1]:
            patches = ops.conv_patches(x, geom, k, stride, pad)                    # gathered again, not kept since the forward
            dwr = ops.gemm_tn(patches, dyd)                                        # [O, kpad]
            dw = dwr[:, :k * k * i].reshape(o, k, k, i).permute(0, 3, 1, 2).contiguous()
        return dx, dw, None, None, None


class FrozenBNActFn(Function):
    """y = act(x * s + t (+ residual)), s = weight / sqrt(running_var), t = bias - running_mean * s; without a weight: y = act(x)"""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, residual, relu):
        y = ops.frozen_bn_act(x, weight, bias, running_mean, running_var, residual=residual, relu=relu)
        ctx.save_for_backward(x if weight is not None else None, y if relu else None, weight, running_mean, running_var)
        ctx.relu, ctx.has_res = relu, residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, running_mean, running_var = ctx.saved_tensors
        dyd = dy.contiguous()
        dx, dres, dw, db = ops.frozen_bn_act_bwd(dyd, y, x, weight, running_mean, running_var, relu=ctx.relu,
                                                 want_residual=ctx.has_res and ctx.relu)
        if ctx.has_res and not ctx.relu:
            dres = dy
        return dx, dw, db, None, None, dres, None


class MaxPoolFn(Function):
    """nn.MaxPool2d(3, 2, 1); the winners' window slots are kept for the backward gather"""

    @staticmethod
    def forward(ctx, x, geom):
        y, arg = ops.maxpool2d(x, geom)
        ctx.save_for_backward(arg)
        ctx.geom = geom
        ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, dy, _darg):
        arg, = ctx.saved_tensors
        return ops.maxpool2d_bwd(dy.contiguous(), arg, ctx.geom), None


class AvgPoolFn(Function):
    """nn.AdaptiveAvgPool2d((1, 1)) + flatten: [b * hw][c] -> [b][c]"""

    @staticmethod
    def forward(ctx, x, b):
        ctx.hw = x.shape[0] // b
        return ops.avgpool_rows(x, b)

    @staticmethod
    def backward(ctx, dy):
        return ops.avgpool_rows_bwd(dy.contiguous(), ctx.hw), None


def _nchw(rows, geom):
    """[b * h * w][c] -> (b, c, h, w), the reference's layout (records and tests only)."""
    b, h, w = geom
    return rows.reshape(b, h, w, rows.shape[1]).permute(0, 3, 1, 2)


def _out_geom(geom, k, stride, pad):
    b, h, w = geom
    return b, ops.conv_out_size(h, k, stride, pad), ops.conv_out_size(w, k, stride, pad)


class Conv2d(nn.Module):
    """Bias-free square convolution; ``weight`` keeps torch's (O, I, kh, kw) shape."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, default_init=False):
        super().__init__()
        self.kernel_size, self.stride, self.padding = kernel_size, stride, padding
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        if default_init:
            nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))                 # torch's Conv2d default (the reference's new conv1)
        else:
            nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")        # torchvision's ResNet.__init__

    def forward(self, x, geom):
        return (ConvFn.apply(x, self.weight, geom, self.stride, self.padding),
                _out_geom(geom, self.kernel_size, self.stride, self.padding))


class FrozenBatchNorm2d(nn.Module):
    """The reference's FrozenBatchNorm2d as ``from_batch_norm`` leaves a fresh BatchNorm2d: trainable weight 1 and bias 0, buffers
    running_mean 0 and running_var 1 + eps (eps is inside the buffer; the forward adds none)."""

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features = num_features
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features) + eps)

    def forward(self, x, residual=None, relu=False):
        return FrozenBNActFn.apply(x, self.weight, self.bias, self.running_mean, self.running_var, residual, relu)


def _note_relu(record, y, geom):
    if record is not None:
        record["relu"].append(_nchw(y.detach() > 0, geom) if geom is not None else y.detach() > 0)


class BasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 3, stride, 1)
        self.bn1 = FrozenBatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, 1, 1)
        self.bn2 = FrozenBatchNorm2d(planes)
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(Conv2d(inplanes, planes, 1, stride, 0), FrozenBatchNorm2d(planes))
        else:
            self.downsample = None

    def forward(self, x, geom, record=None):
        h, g = self.conv1(x, geom)
        h = self.bn1(h, relu=True)
        _note_relu(record, h, g)
        h, g = self.conv2(h, g)
        identity = x
        if self.downsample is not None:
            identity, _ = self.downsample[0](x, geom)
            identity = self.downsample[1](identity)
        h = self.bn2(h, residual=identity, relu=True)
        _note_relu(record, h, g)
        return h, g


class _ResNet(nn.Module):
    """torchvision's resnet18 module tree with the reference's conv1 and head."""

    def __init__(self, input_channels, feature_size):
        super().__init__()
        self.conv1 = Conv2d(input_channels, 64, 7, 2, 3, default_init=True)
        self.bn1 = FrozenBatchNorm2d(64)
        inplanes = 64
        for n, planes in enumerate(STAGES):
            stride = 1 if n == 0 else 2
            setattr(self, "layer%d" % (n + 1), nn.Sequential(BasicBlock(inplanes, planes, stride), BasicBlock(planes, planes, 1)))
            inplanes = planes
        self.fc = nn.Sequential(nn.Linear(512, 512), nn.ReLU(), nn.Linear(512, feature_size))

    def _linear(self, a, mod):
        if torch.is_grad_enabled():
            return LinearFn.apply(a, mod.weight, mod.bias, None, None)
        return ops.gemm(a, mod.weight, mod.bias, row_invariant=True)

    def forward(self, x, geom, record=None):
        h, g = self.conv1(x, geom)
        h = self.bn1(h, relu=True)
        _note_relu(record, h, g)
        h, arg = MaxPoolFn.apply(h, g)
        if record is not None:
            # the winners as torch.nn.functional.max_pool2d(return_indices=True) numbers them: iy * w + ix of the input plane, (b, c, ho, wo)
            _, hh, ww = g
            go = _out_geom(g, 3, 2, 1)
            slot = _nchw(arg, go).to(torch.int64)
            oy = torch.arange(go[1], device=arg.device).view(1, 1, -1, 1)
            ox = torch.arange(go[2], device=arg.device).view(1, 1, 1, -1)
            record["pool"] = (oy * 2 - 1 + slot // 3) * ww + (ox * 2 - 1 + slot % 3)
        g = _out_geom(g, 3, 2, 1)
        for n in range(1, 5):
            for block in getattr(self, "layer%d" % n):
                h, g = block(h, g, record)
        h = AvgPoolFn.apply(h, g[0])
        h = self._linear(h, self.fc[0])
        h = FrozenBNActFn.apply(h, None, None, None, None, None, True)
        _note_relu(record, h, None)
        return self._linear(h, self.fc[2])


class BaseFeatureExtractor(nn.Module):
    @property
    def feature_size(self):
        return self._feature_size


class ResNet18(BaseFeatureExtractor):
    """reference feature_extractors.py:19-44 with ``freeze_bn=True``.  ``forward(X)``: (B, input_channels, H, W) float32 on the HIP device,
    8 <= H, W <= 256 -> (B, feature_size).  ``_record``: set to ``{"relu": [], "pool": None}`` to have the next forward note every ReLU's
    mask (in forward order, the reference's layouts) and the max-pool's winner indices -- the decisions a float64 restatement needs to be
    compared on the same branch (tests)."""

    def __init__(self, freeze_bn, input_channels, feature_size):
        super().__init__()
        if not freeze_bn:
            raise NotImplementedError("feature_extractor.freeze_bn: false (batch-statistics BatchNorm2d) is not built; every shipped "
                                      "config freezes it (freeze_bn: true)")
        self._feature_size = int(feature_size)
        self._input_channels = int(input_channels)
        self._feature_extractor = _ResNet(self._input_channels, self._feature_size)
        self._record = None

    def forward(self, X):
        if not isinstance(X, torch.Tensor) or X.dim() != 4 or X.shape[0] < 1 or X.shape[1] != self._input_channels:
            raise ValueError("room mask must be a (B, %d, H, W) tensor, got %s"
                             % (self._input_channels, tuple(X.shape) if isinstance(X, torch.Tensor) else type(X).__name__))
        b, c, h, w = X.shape
        if not (MIN_SIDE <= h <= MAX_SIDE and MIN_SIDE <= w <= MAX_SIDE):
            raise ValueError("room mask sides must lie in [%d, %d], got %d x %d" % (MIN_SIDE, MAX_SIDE, h, w))
        if X.dtype != torch.float32:
            raise ValueError("room mask must be float32, got %s" % X.dtype)
        ops._dev(X, "room mask")
        rows = X.reshape(b * h * w, 1) if c == 1 else X.permute(0, 2, 3, 1).reshape(b * h * w, c)
        return self._feature_extractor(rows.contiguous(), (b, h, w), self._record)


def get_feature_extractor(name, freeze_bn=False, input_channels=1, feature_size=128):
    """reference :71-85 (which builds both networks and returns one; here only the one asked for is built)."""
    if name == "resnet18":
        return ResNet18(freeze_bn=freeze_bn, input_channels=input_channels, feature_size=feature_size)
    if name == "alexnet":
        raise NotImplementedError("feature_extractor.name: alexnet is not built (no shipped config uses it); use resnet18")
    raise KeyError(name)
