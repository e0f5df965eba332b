"""CPU tier of the split-bf16 matrix mode of the ASPP heads: the weight pack, the emulated oracle the GPU tests compare with, and
the `matrix_mode` plumbing.  No kernel is launched."""
import pytest
import torch
from torch import nn

from tests.split_cases import C_SPLIT, PLANES, SHAPES, problem, reference, split_planes


@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('k', [1, 3])
def test_pack_dense_weight_split(planes, k):
    from mspl_amd import ops
    _, w = problem((1, 64, 40, 4, 4, k, 1), 50 + k)
    pk = ops.pack_dense_weight_split(w, planes)
    assert pk.dtype == torch.bfloat16 and tuple(pk.shape) == (planes, k * k, 40, 64) and pk.is_contiguous()
    # layout: plane p is pack_dense_weight's permute of the p-th plane of w (that permute, restated: pack_dense_weight has no CPU path)
    for p, plane in enumerate(split_planes(w, planes)):
        assert torch.equal(pk[p].float(), plane.permute(2, 3, 0, 1).reshape(k * k, 40, 64))
    assert torch.equal(pk[0], w.to(torch.bfloat16).permute(2, 3, 0, 1).reshape(k * k, 40, 64))
    back = pk.double().sum(0).view(k, k, 40, 64).permute(2, 3, 0, 1)
    bound = {2: 2.0 ** -16, 3: 2.0 ** -24}[planes]
    assert torch.all((w.double() - back).abs() <= bound * w.double().abs())
    with pytest.raises(RuntimeError):
        ops.pack_dense_weight_split(w, 4)
    with pytest.raises(RuntimeError):
        ops.pack_dense_weight_split(w.double(), 2)


@pytest.mark.parametrize('index', range(len(SHAPES)))
def test_emulated_oracle_within_the_split_bound(index):
    ref = reference(index)
    for planes in PLANES:
        err = (ref['emu'][planes] - ref['true']).abs()
        frac = float((err / (C_SPLIT[planes] * ref['mag'])).max())
        print('%s planes %d: max error %.3e, %.3f of the bound' % (ref['shape'], planes, float(err.max()), frac))
        assert torch.all(err <= C_SPLIT[planes] * ref['mag'])
    # and the dropped cross term is visible: two planes are measurably worse than three
    assert float((ref['emu'][2] - ref['true']).abs().max()) > 16 * float((ref['emu'][3] - ref['true']).abs().max())


def test_fits_rule():
    from mspl_amd import ops
    assert ops.dense_conv_split_fits(2048, 256, 3, 2) and ops.dense_conv_split_fits(1280, 256, 1, 3) and ops.dense_conv_split_fits(32, 1, 1, 2)
    for Cin, Cout, k, planes in [(48, 16, 1, 2), (32, 16, 5, 2), (32, 16, 3, 1), (32, 16, 3, 4), (0, 16, 1, 2)]:
        assert not ops.dense_conv_split_fits(Cin, Cout, k, planes)


def test_matrix_mode_attribute_and_set_matrix_mode():
    from mspl_amd import aspp

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.trunk = nn.Conv2d(3, 8, 1)
            self.heads = nn.ModuleList([aspp.ASPP(num_classes=3), nn.Sequential(aspp.ASPP(num_classes=2))])

    net = Net()
    h0, h1 = net.heads[0], net.heads[1][0]
    assert h0.matrix_mode == h1.matrix_mode == 'fp32'
    keys = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert aspp.set_matrix_mode(net, 'bf16x3') == 2
    assert h0.matrix_mode == h1.matrix_mode == 'bf16x3'
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == keys
    assert aspp.set_matrix_mode(h1, 'bf16x6') == 1 and h0.matrix_mode == 'bf16x3' and h1.matrix_mode == 'bf16x6'
    h0.load_state_dict(aspp.ASPP(num_classes=3).state_dict())
    assert h0.matrix_mode == 'bf16x3'
    for bad in ('bf16', 'BF16X3', None, 3):
        with pytest.raises(ValueError):
            h0.matrix_mode = bad
        with pytest.raises(ValueError):
            aspp.set_matrix_mode(net, bad)
    assert h0.matrix_mode == 'bf16x3' and h1.matrix_mode == 'bf16x6'
    aspp.set_matrix_mode(net, 'fp32')
    assert h0.matrix_mode == h1.matrix_mode == 'fp32'
    assert aspp.set_matrix_mode(nn.Conv2d(3, 3, 1), 'bf16x3') == 0
