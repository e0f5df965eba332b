"""Inputs and float64 references for the softmax-family kernels at the logit magnitudes of a trained network (a helper, no tests).

`randn * 3` logits from two independent heads keep |logit| below 10 and the KL of order 1.  A trained network is elsewhere: one class
wins by tens of logits, the two heads agree, the KL is 1e-2 or less, and an exp / log formula whose terms have the size of the logits
loses its relative accuracy there.  `confident_logits` builds such inputs; the references are oracle.labels on `.double()` inputs; the
yardstick of every bound is the SAME oracle on the float32 inputs on the CPU against its float64 result (`err32`), never the code
under test.  tests/test_confident_cases.py holds the references themselves to the conditions the GPU tests rely on."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import labels as olab

MAGNITUDES = (3, 8, 20, 40)                 # the generator's; the training-side families take TRAIN_MAGNITUDES
TRAIN_MAGNITUDES = (8, 20, 40)
HEADS = ('agree', 'differ', 'same')
KLD_FLOOR = 2.0 ** -22                      # unit of the KL bounds: max(err32, KLD_FLOOR)
PROB_FLOOR = 2.0 ** -23                     # ... of the probability bound
MARGIN = 4                                  # |kernel - float64| <= MARGIN * unit (tests/test_gpu_confident_logits.py says why 4)
TIE_GAP_REL = 1e-4                          # a label is compared where the float64 top-two gap exceeds TIE_GAP_REL * magnitude
TIE_CAP = 0.01                              # at most this share of a case's pixels may be left out that way
# the bounds of tests/test_gpu_supervised_grad_parity.py for a loss and for a gradient tensor against float64
LOSS_TAU, GRAD_TAU_REL, GRAD_TAU_EL = 5e-6, 2e-4, 2.5e-4


def upsample(t, size):
    """The decoders' final resize (model/segmentation/espdnet_ue.py:301-302) in t's own precision; identity at equal sizes."""
    size = (int(size[0]), int(size[1]))
    return t if tuple(t.shape[-2:]) == size else F.interpolate(t, size=size, mode='bilinear', align_corners=True)


def _seed(N, C, size, magnitude, heads, seed):
    return 900001 + 7919 * seed + 101 * C + 13 * N + 31 * size[0] + 37 * size[1] + 1009 * int(magnitude) + 5 * HEADS.index(heads)


def confident_logits(N, C, size, magnitude, heads, seed, aux_size=None, target_size=None, ignore=None):
    """(pred (N,C)+size, aux (N,C)+aux_size, target (N,)+target_size int64) from a CPU torch.Generator.

    pred = (randn + onehot(winner)) * magnitude with a random winner class per pixel.  aux is made from pred at the aux head's own
    size (pred itself at equal sizes -- the default --, else pred resized to aux_size, bilinear with aligned corners, in float64):
      'agree'   0.8 * pred + 0.05 * randn       (a trained network: the KL is 1e-2 or less where the heads share a size)
      'differ'  0.8 * pred + 2.0 * randn
      'same'    pred + 3.0                      (identical softmaxes, true KL 0; needs aux_size == size)
    target: the winner (at target_size: of the nearest head pixel) on about 90 % of the pixels, a random class elsewhere; with
    `ignore` given, about 5 % of the pixels carry that value instead."""
    assert heads in HEADS
    size = (int(size[0]), int(size[1]))
    aux_size = size if aux_size is None else (int(aux_size[0]), int(aux_size[1]))
    target_size = size if target_size is None else (int(target_size[0]), int(target_size[1]))
    g = torch.Generator().manual_seed(_seed(N, C, size, magnitude, heads, seed))
    winner = torch.randint(0, C, (N,) + size, generator=g)
    pred = (torch.randn((N, C) + size, generator=g) + F.one_hot(winner, C).permute(0, 3, 1, 2).float()) * float(magnitude)
    base = pred if aux_size == size else upsample(pred.double(), aux_size).float()
    noise = torch.randn((N, C) + aux_size, generator=g)
    if heads == 'same':
        assert aux_size == size, "heads='same' needs both heads at one size"
        aux = pred + 3.0
    else:
        aux = 0.8 * base + (0.05 if heads == 'agree' else 2.0) * noise
    iy = torch.round(torch.linspace(0, size[0] - 1, target_size[0])).long()
    ix = torch.round(torch.linspace(0, size[1] - 1, target_size[1])).long()
    target = winner[:, iy][:, :, ix].clone()
    other = torch.rand((N,) + target_size, generator=g) >= 0.9
    target[other] = torch.randint(0, C, (N,) + target_size, generator=g)[other]
    void = torch.rand((N,) + target_size, generator=g) < 0.05
    if ignore is not None:
        target[void] = int(ignore)
    return pred.contiguous(), aux.contiguous(), target.contiguous()


def class_weights(C):
    return torch.linspace(0.5, 1.5, C) if C > 1 else torch.ones(1)


# ------------------------------------------------------------------ the label epilogue: KL map, probabilities, labels
def label_reference(pred, aux, size, magnitude):
    """Float64 get_output of the up-sampled heads and the float32 oracle's own error against it (the yardstick)."""
    with torch.no_grad():
        p64, a64 = upsample(pred.double(), size), upsample(aux.double(), size)
        prob64, kld64 = olab.get_output(p64, a64)
        prob32, kld32 = olab.get_output(upsample(pred, size), upsample(aux, size))
        o64 = p64 + 0.5 * a64
        top = torch.sort(o64, dim=1, descending=True)[0]
        gap = top[:, 0] - top[:, 1] if o64.shape[1] > 1 else torch.full_like(top[:, 0], float('inf'))
    sure = gap > TIE_GAP_REL * float(magnitude)
    return {'kld64': kld64, 'kld32': kld32, 'err32': float((kld32.double() - kld64).abs().max()),
            'prob64': prob64, 'perr32': float((prob32.double() - prob64).abs().max()),
            'labels64': o64.argmax(1).to(torch.uint8), 'sure': sure, 'excluded': int((~sure).sum()),
            'main32': upsample(pred, size), 'aux32': upsample(aux, size)}


def kld_unit(ref):
    return max(ref['err32'], KLD_FLOOR)


def _centred_parts(m, a):
    """float32 numpy: (T1, S1, S2, M1, M2) of the centred formula for logits (N,C,H,W), summed class by class like the kernels."""
    m, a = np.asarray(m, np.float32), np.asarray(a, np.float32)
    M1, M2 = m.max(1), a.max(1)
    S1 = np.zeros_like(M1); T1 = np.zeros_like(M1); S2 = np.zeros_like(M1)
    for c in range(m.shape[1]):
        d1, d2 = (m[:, c] - M1).astype(np.float32), (a[:, c] - M2).astype(np.float32)
        e1 = np.exp(d1).astype(np.float32)
        S1 = (S1 + e1).astype(np.float32)
        T1 = (T1 + (e1 * (d1 - d2).astype(np.float32)).astype(np.float32)).astype(np.float32)
        S2 = (S2 + np.exp(d2).astype(np.float32)).astype(np.float32)
    return T1, S1, S2, M1, M2


def kld_centred_f32(m, a):
    """The KL map formula of mspl_amd/csrc/labels.hip restated in numpy float32: T1/S1 - log S1 + log S2 with
    T1 = sum e1 * ((m - M1) - (a - M2)): every term is small wherever the softmax weight is not."""
    T1, S1, S2, _, _ = _centred_parts(m, a)
    return ((T1 / S1).astype(np.float32) - np.log(S1).astype(np.float32) + np.log(S2).astype(np.float32)).astype(np.float32)


def kld_raw_f32(m, a):
    """The formula labels.hip used before: T1/S1 - (M1 + log S1) + (M2 + log S2) with T1 = sum e1 * (m - a) -- three terms of the
    size of the logits that cancel."""
    m, a = np.asarray(m, np.float32), np.asarray(a, np.float32)
    M1, M2 = m.max(1), a.max(1)
    S1 = np.zeros_like(M1); T1 = np.zeros_like(M1); S2 = np.zeros_like(M1)
    for c in range(m.shape[1]):
        e1 = np.exp((m[:, c] - M1).astype(np.float32)).astype(np.float32)
        S1 = (S1 + e1).astype(np.float32)
        T1 = (T1 + (e1 * (m[:, c] - a[:, c]).astype(np.float32)).astype(np.float32)).astype(np.float32)
        S2 = (S2 + np.exp((a[:, c] - M2).astype(np.float32)).astype(np.float32)).astype(np.float32)
    lse1 = (M1 + np.log(S1).astype(np.float32)).astype(np.float32)
    lse2 = (M2 + np.log(S2).astype(np.float32)).astype(np.float32)
    return (((T1 / S1).astype(np.float32) - lse1).astype(np.float32) + lse2).astype(np.float32)


# (name, N, C, main size, aux size, output size, which heads).  The forms of mspl_label_epilogue_fwd the product build reaches:
#   lds_*      the LDS-staged kernel: exact-count instantiations (5, 13, 20), the predicated ones (3 -> 8, 11 -> 16, 21 -> 24); both heads
#              at the x2 size, so that `agree` and `same` are what they are for a trained network after the up-sampling too
#   wide_*     its 480-pixel-wide instantiations (staged strides 132 / 68): x2 and x4 heads
#   odd / id   an odd width with x2 / x4 heads; all three sizes equal
#   reg_*      the register kernel: staged rows wider than 256 columns do not fit the LDS form
#   gen_*      the general kernel: more than 24 classes; the probability / logit outputs are asked for by the test
_ADS = ('agree', 'differ', 'same')
_AD = ('agree', 'differ')
LABEL_SHAPES = [('lds_c%d' % C, 2, C, (8, 20), (8, 20), (16, 40), _ADS) for C in (5, 13, 20, 3, 11, 21)] + \
               [('wide_c%d' % C, 1, C, (8, 240), (4, 120), (16, 480), _AD) for C in (5, 13, 20)] + \
               [('odd_c5', 2, 5, (9, 22), (5, 11), (18, 44), _AD), ('odd_c11', 2, 11, (9, 22), (5, 11), (18, 44), _AD),
                ('id_c5', 2, 5, (17, 37), (17, 37), (17, 37), _ADS), ('id_c13', 1, 13, (17, 37), (17, 37), (17, 37), _ADS),
                ('reg_id_c5', 1, 5, (6, 260), (6, 260), (6, 260), _ADS), ('reg_c13', 1, 13, (12, 300), (6, 150), (12, 300), _AD),
                ('gen_c30', 1, 30, (9, 22), (5, 11), (18, 44), _AD), ('gen_id_c30', 1, 30, (16, 24), (16, 24), (16, 24), _ADS),
                ('gen_prob_c5', 2, 5, (9, 22), (9, 22), (18, 44), _ADS)]
LABEL_CASES = [(s[0], mag, h) for s in LABEL_SHAPES for mag in MAGNITUDES for h in s[6]]
_LABEL_SHAPE = dict((s[0], s) for s in LABEL_SHAPES)


def label_case_id(case):
    return '%s-m%d-%s' % case


def identity_size(name):
    """No up-sampling at all: the construction of the measurement that motivated the centred formula."""
    s = _LABEL_SHAPE[name]
    return s[3] == s[4] == s[5]


@functools.lru_cache(maxsize=None)
def label_case(case):
    """(pred, aux, output size, reference dict) of one LABEL_CASES entry; computed once, shared, never modified."""
    name, mag, heads = case
    _, N, C, ms, as_, size, _ = _LABEL_SHAPE[name]
    pred, aux, _ = confident_logits(N, C, ms, mag, heads, 0, aux_size=as_)
    return pred, aux, size, label_reference(pred, aux, size, mag)


# ------------------------------------------------------------------ the training and evaluation losses
def uest_reference(pred, aux, target, cw, ignore, size, dtype, out_scale=1.0):
    """uest_train_loss (criterion(pred + 0.5 aux, labels, kld) * 20 + kld.mean()) on the up-sampled heads in `dtype`:
    (loss, d loss / d up-sampled pred, d loss / d up-sampled aux, kld)."""
    p = upsample(pred.to(dtype), size).detach().requires_grad_()
    a = upsample(aux.to(dtype), size).detach().requires_grad_()
    loss = olab.uest_train_loss(p, a, target, cw.to(dtype), ignore_idx=ignore) * out_scale
    loss.backward()
    return float(loss.detach()), p.grad, a.grad


def kld_grad_reference(d1, d2, gk, dtype):
    """PixelwiseKLD forward and its backward for the upstream gradient gk (N,H,W)."""
    a, b = d1.detach().to(dtype).clone().requires_grad_(), d2.detach().to(dtype).clone().requires_grad_()
    k = olab.pixelwise_kld(a, b)
    k.backward(gk.to(dtype))
    return k.detach(), a.grad, b.grad


def weighted_ce_reference(pred, target, u, cw, ignore, mode, dtype):
    """(sums[0], sums[1], d loss / d pred, d loss / d u) of mspl_weighted_ce_fwd / _bwd with upstream gradient 1:
    sums[0] = sum_valid w[t] * nll * exp(-u), sums[1] = sum_valid w[t]; loss = sums[0] / (N*H*W) ('all') or / sums[1] ('weights')."""
    N, C, H, W = pred.shape
    x = pred.detach().to(dtype).clone().requires_grad_()
    uu = None if u is None else u.detach().to(dtype).clone().requires_grad_()
    valid = (target != ignore) & (target >= 0) & (target < C)
    t = torch.where(valid, target, torch.zeros_like(target))
    w = cw.to(dtype)[t] * valid.to(dtype)
    nll = F.cross_entropy(x, t, reduction='none')
    num = (nll * w * (torch.exp(-uu) if uu is not None else 1.0)).sum()
    den = w.sum()
    (num / (N * H * W) if mode == 'all' else num / den).backward()
    return float(num.detach()), float(den), x.grad, None if uu is None else uu.grad


def ce_sums_reference(x, target, cw, ignore, dtype=torch.float64):
    """(num, den) of nn.CrossEntropyLoss(weight, ignore_index) through F.cross_entropy(reduction='sum'), as
    tests/test_gpu_ce_meters._reference does; labels outside 0..C-1 count nowhere."""
    C = x.shape[1]
    tt = torch.where((target < 0) | (target >= C), torch.full_like(target, ignore), target)
    w = cw.to(dtype)
    num = float(F.cross_entropy(x.to(dtype), tt, weight=w, ignore_index=ignore, reduction='sum'))
    keep = tt[tt != ignore]
    return num, float(w[keep].sum())


def loss_error(got, ref64):
    """Relative error of a loss (absolute where the float64 loss is exactly 0: one class)."""
    return abs(got - ref64) / abs(ref64) if ref64 != 0.0 else abs(got - ref64)


def grad_errors(got, ref64):
    """(relative norm error, largest element error / largest element) of a gradient tensor against float64 (absolute errors where
    the float64 gradient is exactly 0: one class)."""
    got, ref64 = got.detach().cpu().double(), ref64.double()
    nrm, top = float(ref64.norm()), float(ref64.abs().max())
    if top == 0.0:
        d = float((got - ref64).abs().max())
        return d, d
    return float((got - ref64).norm()) / nrm, float((got - ref64).abs().max()) / top


# (name, N, C, main size, aux size, output size): the shapes of the loss families.  Full-resolution kernels take the first entries;
# the head-resolution ones the x2 / x4 heads of an (18, 44) label map, one per class count with its own code path.
FULL_SHAPES = [('full_c5', 2, 5, (18, 44)), ('full_c13', 1, 13, (18, 44))]
HEADS_SHAPES = [('heads_c%d' % C, 2, C, (9, 22), (5, 11), (18, 44)) for C in (1, 3, 5, 8, 13, 20)]
KLD_SHAPES = [('kld_c%d' % C, 2, C, (18, 44)) for C in (2, 5, 21)]
CE_SHAPES = [('ce_c5', 2, 5, (18, 44)), ('ce_c20', 1, 20, (18, 44))]
EVAL_SHAPES = [('eval_c%d' % C, 2, C, (9, 22), (5, 11), (18, 44)) for C in (5, 20)]


def grid(shapes, heads=_AD, magnitudes=TRAIN_MAGNITUDES):
    return [(s, mag, h) for s in shapes for mag in magnitudes for h in heads]


def grid_id(case):
    return '%s-m%d-%s' % (case[0][0], case[1], case[2])


@functools.lru_cache(maxsize=None)
def loss_case(case, out_scale=1.0):
    """One case of the fused uest loss (K11 and its head-resolution forms): inputs, class weights with the ignore class C - 1 (none at
    C = 1), and the float64 / float32 oracle results.  Computed once, shared, never modified."""
    shape, mag, heads = case
    name, N, C, ms = shape[:4]
    as_, size = (shape[4], shape[5]) if len(shape) > 4 else (ms, ms)
    ignore = C - 1 if C > 1 else None
    pred, aux, target = confident_logits(N, C, ms, mag, heads, 1, aux_size=as_, target_size=size, ignore=ignore)
    cw = class_weights(C)
    cwz = cw.clone()
    if ignore is not None:
        cwz[ignore] = 0.0
    r64 = uest_reference(pred, aux, target, cw, ignore, size, torch.float64, out_scale)
    r32 = uest_reference(pred, aux, target, cw, ignore, size, torch.float32, out_scale)
    return {'pred': pred, 'aux': aux, 'target': target, 'cw': cwz, 'size': size, 'ref64': r64, 'ref32': r32, 'C': C, 'N': N}


@functools.lru_cache(maxsize=None)
def kld_case(case):
    """One PixelwiseKLD case: both distributions, an upstream gradient in [0.5, 1.5), the KL reference of label_reference and the
    float64 / float32 oracle gradients.  `grad_unit`: the float32 oracle's largest absolute gradient error, floored at one float32
    rounding of the largest softmax term (2**-23 * max gk) -- the unit of the `same` cases, whose float64 gradients are themselves
    the rounding of aux = pred + 3 (1e-6 and below), so that a relative bound would compare noise with noise (the float32 oracle
    is off by 30 % to 200 % of them)."""
    (name, N, C, size), mag, heads = case
    d1, d2, _ = confident_logits(N, C, size, mag, heads, 2)
    gk = torch.rand((N,) + tuple(size), generator=torch.Generator().manual_seed(11)) + 0.5
    g64 = kld_grad_reference(d1, d2, gk, torch.float64)[1:]
    g32 = kld_grad_reference(d1, d2, gk, torch.float32)[1:]
    unit = max(max(float((a.double() - b).abs().max()) for a, b in zip(g32, g64)), 2.0 ** -23 * float(gk.max()))
    return {'d1': d1, 'd2': d2, 'gk': gk, 'ref': label_reference(d1, d2, size, mag), 'g64': g64, 'g32': g32, 'grad_unit': unit}


@functools.lru_cache(maxsize=None)
def wce_case(case, with_u, mode):
    """One weighted cross entropy case on pred + 0.5 aux with labels of every class and 5 % of 255 (ignored); u = the KL of the two
    heads (the uncertainty weight of the uest loss) or None; mode 'all' / 'weights' = the two normalisations."""
    (name, N, C, size), mag, heads = case
    pred, aux, tgt = confident_logits(N, C, size, mag, heads, 3, ignore=255)
    x = pred + 0.5 * aux
    cw = class_weights(C)
    with torch.no_grad():
        u = olab.pixelwise_kld(pred, aux).clamp_(min=0.0) if with_u else None
    return {'x': x, 'target': tgt, 'u': u, 'cw': cw, 'ref64': weighted_ce_reference(x, tgt, u, cw, 255, mode, torch.float64),
            'ref32': weighted_ce_reference(x, tgt, u, cw, 255, mode, torch.float32)}
