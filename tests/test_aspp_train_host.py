"""CPU tier of the ASPP training path: the golden's completeness, the data-gradient weight pack against ATen, and the routing of the
four training x grad combinations."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.aspp_train_cases import ASPP_TRAIN_CASES, BN_FED_BIASES, DILATIONS, SAMPLE, dead_taps, sample_index
from tests.conftest import GOLDEN

META = json.load(open(os.path.join(GOLDEN, 'aspp_train.json')))


@pytest.mark.parametrize('name', sorted(ASPP_TRAIN_CASES))
def test_golden_has_every_state_dict_key(name, golden):
    from mspl_amd import aspp
    cls, ncls, shp, sd_seed = ASPP_TRAIN_CASES[name][:4]
    m = getattr(aspp, cls)(num_classes=ncls)
    ref = golden('aspp_train_' + name)
    params = dict(m.named_parameters())
    for k, v in m.state_dict().items():
        stem, _, leaf = k.rpartition('.')
        if k in params:
            idx = sample_index(k, tuple(v.shape), sd_seed)
            assert ref['g__' + k].shape == (tuple(v.shape) if idx is None else (SAMPLE,)), k
            rec = META[name]['g__' + k]
            assert ('abs' in rec) == (k in BN_FED_BIASES), k
            if k in BN_FED_BIASES:          # mathematically zero: rounding level in the float64 record
                assert rec['scale'] < 1e-9, k
        else:
            key = {'running_mean': 'rm__', 'running_var': 'rv__', 'num_batches_tracked': 'nbt__'}[leaf] + stem
            assert ref[key].shape == tuple(v.shape), k
            if leaf == 'num_batches_tracked':
                assert ref[key] == 1
    for k in ('logits', 'gx', 'gx_chansum', 'gx_pixsum'):
        assert k in ref and np.all(np.isfinite(ref[k]))
    assert ref['logits'].shape == (shp[0], ncls) + tuple(shp[2:])
    assert all(os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20 for f in os.listdir(GOLDEN) if f.startswith('aspp_train'))


@pytest.mark.parametrize('name', sorted(ASPP_TRAIN_CASES))
def test_samples_cover_all_taps_and_dead_taps_are_zero(name, golden):
    cls, ncls, shp, sd_seed = ASPP_TRAIN_CASES[name][:4]
    ref = golden('aspp_train_' + name)
    Cin, H, W = shp[1:]
    dead_total = 0
    for k, dil in DILATIONS.items():
        idx = sample_index(k, (256, Cin, 3, 3), sd_seed)
        assert idx.numel() == SAMPLE and idx.unique().numel() == SAMPLE and int(idx.max()) < 256 * Cin * 9
        taps = idx % 9
        assert sorted(taps.unique().tolist()) == list(range(9)) and int(torch.bincount(taps).min()) >= 400
        g = ref['g__' + k]
        for t in range(9):
            on_tap = g[(taps == t).numpy()]
            if t in dead_taps(dil, H, W):
                dead_total += 1
                assert np.all(on_tap == 0.0) and ref['tapsum__' + k][t] == 0.0 and ref['tapnorm__' + k][t] == 0.0
            else:
                assert np.any(on_tap != 0.0) and ref['tapnorm__' + k][t] > 0.0
    assert dead_total == {'aspp_bottleneck_c20': 14, 'aspp_c13': 0}[name]


@pytest.mark.parametrize('shape', [(5, 4, 3, 2, 6, 7), (3, 2, 1, 1, 4, 5), (2, 3, 3, 4, 5, 4)])
def test_pack_dense_weight_dgrad_against_aten(shape):
    """conv2d of gy with the unpacked data-gradient pack == what conv2d autograd (and conv_transpose2d) give for the input."""
    from mspl_amd import ops
    Cout, Cin, k, dil, H, W = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, Cin, k, k, generator=g)
    gy = torch.randn(2, Cout, H, W, generator=g, dtype=torch.float64)
    pad = dil * (k // 2)
    F.conv2d(x, w.double(), None, 1, pad, dil).backward(gy)
    wt = ops.pack_dense_weight_dgrad(w)
    assert tuple(wt.shape) == (k * k, Cin, Cout) and wt.is_contiguous()
    wp = ops.pack_dense_weight(w) if w.is_cuda else w.permute(2, 3, 0, 1).reshape(k * k, Cout, Cin)
    for t in range(k * k):
        assert torch.equal(wt[t], wp[k * k - 1 - t].t())
    got = F.conv2d(gy, ops.unpack_dense_weight(wt, k).double(), None, 1, pad, dil)
    torch.testing.assert_close(got, x.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(F.conv_transpose2d(gy, w.double(), None, 1, pad, 0, 1, dil), x.grad, rtol=1e-12, atol=1e-12)
    # unpack_dense_weight is the inverse permute of the forward pack, as a view
    back = ops.unpack_dense_weight(wp.contiguous(), k)
    assert torch.equal(back, w) and back._base is not None


def test_mode_table(monkeypatch):
    """train() with grad -> the training forward; eval() with grad -> refused; both no_grad combinations -> today's inference code."""
    from mspl_amd import aspp
    monkeypatch.setattr(aspp._ASPPBase, '_forward_train', lambda self, x: 'train')
    monkeypatch.setattr(aspp._ASPPBase, '_forward_infer', lambda self, x: 'infer')
    m = aspp.ASPP(num_classes=3)
    x = torch.zeros(2, 512, 2, 2)
    m.train()
    assert m(x) == 'train'
    with torch.no_grad():
        assert m(x) == 'infer'
    m.eval()
    with pytest.raises(RuntimeError, match='inference-only'):
        m(x)
    with torch.no_grad():
        assert m(x) == 'infer'
    # nothing but self.training and the grad mode selects the path: a feature map that requires grad changes nothing
    m.train()
    with torch.no_grad():
        assert m(x.requires_grad_(True)) == 'infer'
