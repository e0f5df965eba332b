"""nn_layers/aspp.py on the HIP path: `ASPP(num_classes)` (512-channel trunks) and `ASPP_Bottleneck(num_classes)` (2048-channel
trunks) -- the DeepLabv3 heads of BASELINE configs[4].  Same constructor, attribute names and `state_dict()` as the reference;
Under torch.no_grad(): eval-mode BatchNorm (folded, together with the conv bias, into the producing kernel's epilogue).
In train() with gradients enabled: the reference's training forward (batch-statistics BatchNorm, running-statistics update)
on autograd nodes with HIP backward kernels.  eval() with gradients enabled (frozen-BN fine-tuning of the heads) is refused.

    out_1x1   = relu(bn(conv_1x1_1(x)))                       aspp.py:40 / :87
    out_3x3_k = relu(bn(conv_3x3_k(x))),  dilation 6, 12, 18  aspp.py:41-43 / :88-90      <- K13, the matrix-core kernel
    out_img   = interpolate(relu(bn(conv_1x1_2(avg_pool(x)))))  (a constant map: bilinear from 1x1)   :45-47 / :92-94
    out       = conv_1x1_4(relu(bn(conv_1x1_3(cat[...]))))     aspp.py:49-51 / :96-98

Inference: the five branches write straight into their channel slice of one (N,1280,H,W) buffer.
Training: each branch keeps its raw convolution output z (what the BatchNorm backward needs); the four convolutions of the
feature map are ONE autograd node (one data-gradient launch into one gx), torch.cat builds the concatenation.

Matrix mode (inference path only; `head.matrix_mode`, or `set_matrix_mode(model, mode)` for every head of a module tree):
    'fp32'    the default: exact fp32 on v_mfma_f32_32x32x2_f32, bit-identical to a head that never heard of the mode
    'bf16x3'  the four convolutions of the feature map and conv_1x1_3 split every fp32 operand into 2 bf16 planes and keep the 3
              products plane_i(w) * plane_j(x) with i + j < 2 on the bf16 matrix instruction, fp32 accumulation
    'bf16x6'  3 planes, the 6 products with i + j < 3: indistinguishable from float64 arithmetic at fp32 output precision
  Split rule: r_0 = v, plane_i = bf16_rne(r_i), r_{i+1} = r_i - float(plane_i).  Contract: inputs and weights finite and in the
  normal fp32 range (an infinity splits into an infinity and a NaN; magnitudes whose low planes would be bf16-subnormal lose
  them); the output is fp32; the summation order is fixed, so the same inputs give the same bits.  The pooled 1x1 (N pixels) and
  the classifier stay fp32, and so does the whole training path: _forward_train ignores the mode.
"""
import torch
from torch import nn

from . import autograd, ops
from .layers import bn_fold, cached
from .ops import Epi


MATRIX_MODES = {'fp32': 0, 'bf16x3': 2, 'bf16x6': 3}        # mode -> bf16 planes per operand (0: no split)


def _check_mode(mode):
    if mode not in MATRIX_MODES:
        raise ValueError('mspl_amd: matrix_mode %r (one of %s)' % (mode, ', '.join(repr(m) for m in MATRIX_MODES)))
    return mode


def set_matrix_mode(module, mode):
    """Set `matrix_mode` on every ASPP head found in `module`'s tree (the module itself included); returns how many there were."""
    _check_mode(mode)
    heads = [m for m in module.modules() if isinstance(m, _ASPPBase)]
    for m in heads:
        m.matrix_mode = mode
    return len(heads)


class _ASPPBase(nn.Module):
    _matrix_mode = 'fp32'

    def __init__(self, in_channels, num_classes):
        super().__init__()
        self.conv_1x1_1 = nn.Conv2d(in_channels, 256, kernel_size=1)
        self.bn_conv_1x1_1 = nn.BatchNorm2d(256)
        self.conv_3x3_1 = nn.Conv2d(in_channels, 256, kernel_size=3, stride=1, padding=6, dilation=6)
        self.bn_conv_3x3_1 = nn.BatchNorm2d(256)
        self.conv_3x3_2 = nn.Conv2d(in_channels, 256, kernel_size=3, stride=1, padding=12, dilation=12)
        self.bn_conv_3x3_2 = nn.BatchNorm2d(256)
        self.conv_3x3_3 = nn.Conv2d(in_channels, 256, kernel_size=3, stride=1, padding=18, dilation=18)
        self.bn_conv_3x3_3 = nn.BatchNorm2d(256)
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.conv_1x1_2 = nn.Conv2d(in_channels, 256, kernel_size=1)
        self.bn_conv_1x1_2 = nn.BatchNorm2d(256)
        self.conv_1x1_3 = nn.Conv2d(1280, 256, kernel_size=1)       # (1280 = 5*256)
        self.bn_conv_1x1_3 = nn.BatchNorm2d(256)
        self.conv_1x1_4 = nn.Conv2d(256, num_classes, kernel_size=1)

    @property
    def matrix_mode(self):
        return self._matrix_mode

    @matrix_mode.setter
    def matrix_mode(self, mode):
        self._matrix_mode = _check_mode(mode)

    def _packed(self, conv):
        return cached(conv, 'packed', [conv.weight], lambda: ops.pack_dense_weight(conv.weight))

    def _dense(self, x, conv, ep, out=None):
        """One dense convolution of the inference path in this head's matrix mode (exact fp32 where the split kernel does not fit)."""
        k, dil = conv.kernel_size[0], conv.dilation[0]
        planes = MATRIX_MODES[self._matrix_mode]
        if planes and ops.dense_conv_split_fits(conv.in_channels, conv.out_channels, k, planes):
            ws = cached(conv, 'packed_split%d' % planes, [conv.weight], lambda: ops.pack_dense_weight_split(conv.weight, planes))
            return ops.dense_conv_split(x, ws, k, dil, ep, out=out)
        return ops.dense_conv(x, self._packed(conv), k, dil, ep, out=out)

    def _epi(self, conv, bn, ctot=None, coff=0):
        """relu(bn(conv(x) + bias)) as scale / shift / alpha = 0: shift = bn_shift + bias * bn_scale.  Epilogue vectors are
        indexed by the DESTINATION channel: for a branch written into its slice of the concatenation they are laid out at
        that offset in a ctot-sized vector."""
        def build():
            scale, shift = bn_fold(bn)
            shift = shift + conv.bias * scale
            n = scale.numel()
            tot = n if ctot is None else ctot
            sc, sh = torch.ones(tot, device=scale.device), torch.zeros(tot, device=scale.device)
            sc[coff:coff + n] = scale
            sh[coff:coff + n] = shift
            return sc, sh, torch.zeros(tot, device=scale.device)
        sc, sh, zero = cached(bn, 'aspp_epi_%s_%d' % (ctot, coff), [bn.weight, bn.bias, bn.running_mean, bn.running_var, conv.bias], build)
        return Epi(sc, sh, zero)

    def _packs(self, conv):
        """(packed weight, callable giving the data-gradient pack) of a dense convolution, both cached per weight version."""
        return (self._packed(conv),
                lambda: cached(conv, 'packed_dgrad', [conv.weight], lambda: ops.pack_dense_weight_dgrad(conv.weight)))

    def _relu(self, z, bn):
        """relu(bn(z)) with batch statistics: PReLU with a constant zero slope, which takes no gradient."""
        zero = cached(bn, 'aspp_zero_alpha', [bn.weight], lambda: torch.zeros(bn.num_features, device=bn.weight.device))
        return autograd.bn_train_prelu(z, bn, alpha=zero)

    def _forward_train(self, feature_map):
        """nn_layers/aspp.py:40-51 / :87-98 in train(): saved activations are the feature map (once), the five z, the concatenation
        and conv_1x1_3's z."""
        H, W = feature_map.shape[2:]
        spatial = [(self.conv_1x1_1, self.bn_conv_1x1_1), (self.conv_3x3_1, self.bn_conv_3x3_1),
                   (self.conv_3x3_2, self.bn_conv_3x3_2), (self.conv_3x3_3, self.bn_conv_3x3_3)]
        zs = autograd.dense_conv_branches(feature_map, [c for c, _ in spatial], [self._packs(c) for c, _ in spatial])
        outs = [self._relu(z, bn) for z, (_, bn) in zip(zs, spatial)]
        img = autograd.adaptive_avgpool(feature_map, (1, 1))
        (zi,) = autograd.dense_conv_branches(img, [self.conv_1x1_2], [self._packs(self.conv_1x1_2)])
        outs.append(autograd.bilinear(self._relu(zi, self.bn_conv_1x1_2), (int(H), int(W))))
        cat = torch.cat(outs, 1)
        (z3,) = autograd.dense_conv_branches(cat, [self.conv_1x1_3], [self._packs(self.conv_1x1_3)])
        out = self._relu(z3, self.bn_conv_1x1_3)
        return autograd.conv_bias(out, self.conv_1x1_4)

    def forward(self, feature_map):
        if torch.is_grad_enabled():
            if not self.training:
                raise RuntimeError('mspl_amd: the ASPP heads are inference-only in eval() on the HIP path: frozen-BatchNorm '
                                   'fine-tuning of the heads is not supported (call under torch.no_grad(), or train() the head '
                                   'for batch-statistics training)')
            return self._forward_train(feature_map)
        return self._forward_infer(feature_map)

    def _forward_infer(self, feature_map):
        N, _, H, W = feature_map.shape
        cat = torch.empty((N, 1280, H, W), device=feature_map.device, dtype=torch.float32)
        self._dense(feature_map, self.conv_1x1_1, self._epi(self.conv_1x1_1, self.bn_conv_1x1_1, 1280, 0), out=(cat, 0))
        for i, (conv, bn) in enumerate([(self.conv_3x3_1, self.bn_conv_3x3_1), (self.conv_3x3_2, self.bn_conv_3x3_2),
                                        (self.conv_3x3_3, self.bn_conv_3x3_3)]):
            self._dense(feature_map, conv, self._epi(conv, bn, 1280, 256 * (i + 1)), out=(cat, 256 * (i + 1)))
        img = ops.adaptive_avgpool(feature_map, (1, 1))
        img = ops.dense_conv(img, self._packed(self.conv_1x1_2), 1, 1, self._epi(self.conv_1x1_2, self.bn_conv_1x1_2))
        ops.bilinear(img, (H, W), out=(cat, 1024))            # bilinear from a 1x1 map: the constant, whatever align_corners is
        out = self._dense(cat, self.conv_1x1_3, self._epi(self.conv_1x1_3, self.bn_conv_1x1_3))
        c4 = self.conv_1x1_4
        return ops.conv1x1(out, c4.weight, 1, Epi(shift=c4.bias))


def upsample_logits(logits, size):
    """The head's caller: F.upsample(output, size=(h, w), mode='bilinear') with the default align_corners=False
    (model/segmentation/deeplabv3.py:40)."""
    return ops.bilinear(logits, size, align_corners=False)


class ASPP(_ASPPBase):
    def __init__(self, num_classes):
        super().__init__(512, num_classes)


class ASPP_Bottleneck(_ASPPBase):
    def __init__(self, num_classes):
        super().__init__(4 * 512, num_classes)
