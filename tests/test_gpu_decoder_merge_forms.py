"""mspl_decoder_merge_fwd at the seams of its loop structure (tests/decoder_merge_cases.py: trip counts 1, 2, odd and even per
form and SPLIT, column blocks, plane counts, gate values) against the float64 formula and against the three launches it
replaces.  Needs a real MI355X: run with `-m gpu`.

Bounds are those of tests/test_gpu_decoder_merge.py: both evaluations are fp32 evaluations of one expression whose last step
is a sum of <= 64 products, held to EDGE_REL = (64 + 16) * 2^-23 ~= 1e-5 of the largest |value| of the output, and the fused
launch's error may not exceed twice the chain's on the same inputs.  A wrong buffer, a skipped or repeated group, a wrong halo
column or plane offset is an error of order 1.
"""
import pytest
import torch

from tests import decoder_merge_cases as dmc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _chain(c, groups):
    from mspl_amd import ops
    from mspl_amd.ops import Epi
    H, W = c['enc'].shape[2:]
    pw = ops.conv3x3(c['enc'], c['w3'], groups, ep=Epi(c['es'], c['eb'], c['ea'], gate=c['gate']))
    m = ops.bilinear(c['bu'], (H, W), Epi(c['bs'], c['bb'], c['ba'], pre_add=pw))
    return ops.conv1x1(m, c['wp'], 1, Epi(c['ps'], c['pb'], c['pa']))


def _fused(c):
    from mspl_amd import ops
    return ops.decoder_merge(c['enc'], c['bu'], c['w3'], (c['es'], c['eb'], c['ea']), c['gate'], (c['bs'], c['bb'], c['ba']),
                             c['wp'], (c['ps'], c['pb'], c['pa']))


@pytest.mark.parametrize('name', dmc.IDS)
def test_seam_case(name):
    case = dmc.CASES[dmc.IDS.index(name)]
    d, groups, ref = dmc.case_data(name)
    c = {k: v.to(DEV) for k, v in d.items()}
    scale = float(ref.abs().max())
    chain = _chain(c, groups)
    fused = _fused(c)
    torch.cuda.synchronize()
    ec = float((chain.cpu().double() - ref).abs().max())
    print('%s: chain %.3e of max |ref| = %.3f' % (name, ec / scale, scale))
    assert ec <= dmc.EDGE_REL * scale                               # the yardstick's own check
    if not dmc.geometry(case)['fused']:
        assert fused is None, 'a shape outside the fused set must be declined'      # and the chain has served it above
        return
    assert fused is not None, 'a fused shape was declined'
    assert fused.shape == (case.N, case.P, case.H, case.W)
    ef = float((fused.cpu().double() - ref).abs().max())
    print('%s: fused %.3e' % (name, ef / scale))
    assert ef <= dmc.EDGE_REL * scale
    assert ef <= 2.0 * ec
    # batch: the middle image alone gives the bits it has inside the batch of three
    one = _fused({k: (v[1:2].contiguous() if k in ('enc', 'bu', 'gate') else v) for k, v in c.items()})
    assert one is not None and torch.equal(one, fused[1:2])


def test_declined_shape_is_served_by_the_chain():
    """4 -> 3 groups are no fused form: ops.decoder_merge declines (nothing is launched) and the three launches meet the bound."""
    case = dmc.Case('declined_64to48', 3, 64, 48, 16, 8, 60, None, None, None, None, 4999)
    assert not dmc.geometry(case)['fused']
    d, groups = dmc.inputs(case)
    ref = dmc.formula(d, groups)
    c = {k: v.to(DEV) for k, v in d.items()}
    assert _fused(c) is None
    chain = _chain(c, groups)
    assert float((chain.cpu().double() - ref).abs().max()) <= dmc.EDGE_REL * float(ref.abs().max())
