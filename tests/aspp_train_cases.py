"""Cases and sampling rules of the ASPP training golden (tests/golden/make_aspp_train_golden.py writes it with the reference's own
nn_layers/aspp.py in train(); tests/test_aspp_train_host.py and tests/test_gpu_aspp_train.py read it).  Weights, inputs and the
cotangent are regenerated from seeds by tests/synth.py: a 3x3 weight of the bottleneck head alone is 19 MB.

name -> (class name, num_classes, input shape, state-dict seed, input seed, cotangent seed)
  aspp_bottleneck_c20   10 x 14 map: dilation 18 leaves the map in both directions (eight dead taps), dilation 12 vertically only
                        (six dead taps: 12 < 14 columns), dilation 6 is partial everywhere
  aspp_c13              20 x 33 map: dilation 18 still reaches two rows; odd width, 1320 pixels are no multiple of a tile; N = 2 is the
                        smallest batch the image branch's BatchNorm (N values per channel) accepts
"""
import torch

ASPP_TRAIN_CASES = {
    'aspp_bottleneck_c20': ('ASPP_Bottleneck', 20, (2, 2048, 10, 14), 410, 411, 412),
    'aspp_c13': ('ASPP', 13, (2, 512, 20, 33), 413, 414, 415),
}

FULL_LIMIT = 8192          # a parameter gradient with at most this many elements is stored in full
SAMPLE = 4096              # else: this many seeded elements
X_SAMPLE = 8192            # elements of the input gradient that are stored (the whole tensor is 4.6 / 5.4 MB in float64)

# the convolutions in front of a batch-statistics BatchNorm: their bias gradient is mathematically zero
BN_FED_BIASES = ('conv_1x1_1.bias', 'conv_3x3_1.bias', 'conv_3x3_2.bias', 'conv_3x3_3.bias', 'conv_1x1_2.bias', 'conv_1x1_3.bias')
DILATIONS = {'conv_3x3_1.weight': 6, 'conv_3x3_2.weight': 12, 'conv_3x3_3.weight': 18}


def _gen(name, seed):
    import zlib
    g = torch.Generator()
    g.manual_seed((zlib.crc32(name.encode()) + 104729 * seed) & 0x7FFFFFFF)
    return g


def sample_index(name, shape, seed):
    """Flat indices (int64, into the contiguous tensor of `shape`) of the stored elements of gradient `name`, or None when the
    whole tensor is stored.  3x3 weights: 455 (co, ci) pairs per tap, nine taps, plus one more of the centre tap."""
    numel = 1
    for s in shape:
        numel *= int(s)
    if name == 'x':
        return torch.randperm(numel, generator=_gen(name, seed))[:X_SAMPLE].sort()[0]
    if numel <= FULL_LIMIT:
        return None
    g = _gen(name, seed)
    if len(shape) == 4 and shape[2] == 3:
        pairs = int(shape[0]) * int(shape[1])
        per = (SAMPLE - 1) // 9
        idx = [torch.randperm(pairs, generator=g)[:per + (1 if t == 4 else 0)] * 9 + t for t in range(9)]
        return torch.cat(idx).sort()[0]
    return torch.randperm(numel, generator=g)[:SAMPLE].sort()[0]


def dead_taps(dilation, H, W):
    """Taps (0..8, row-major) of a 3x3 convolution with padding = dilation whose shift leaves an H x W map for every pixel: their
    weight gradient is exactly zero."""
    return [t for t in range(9) if (t // 3 != 1 and dilation >= H) or (t % 3 != 1 and dilation >= W)]
