"""The head of a DownSampler block as one launch (mspl_down_head_fwd: proj_1x1 + BatchNorm + PReLU, the 3x3 / s2 average pool with
the block's epilogue, and the plane sums of the input, from one read of the input) against (a) the launches it replaces
(mspl_conv1x1_fwd and mspl_avgpool3x3s2_psum_fwd; the strided K2 and the expansion follow either way) and (b) the reference
formula in torch float64 on the CPU (oracle.net.downsampler).  Needs a real MI355X: run with `-m gpu`.

Bounds.  The pooled half of the output repeats the pool kernel operation by operation: bit-identical, asserted.  Channels
[nin, nout) differ from (a) only through the reduced tensor, a sum of <= 64 fp32 products per value that (a) forms on the matrix
cores (small batches) or in the same ascending order on the vector unit (batch 16: bit-identical, asserted): the largest error
against (b), relative to the largest |output|, must not exceed TWICE that of (a) on the same inputs (the bound of
tests/test_gpu_decoder_merge.py).  Plane sums: every input value passes through at most d fp32 additions (3 in the eight-column
tree, 1 for the second row, 7 across the wave, 2 across the waves, nblk - 1 across the workgroups of a plane, done in float64
here), so |sum - exact| <= d * 2^-24 * sum |x| to first order; 1 % is allowed for the higher-order terms.
"""
import json
import os

import pytest
import torch

from oracle import net as onet
from tests.conftest import GOLDEN
from tests.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = json.load(open(os.path.join(GOLDEN, 'state_dict_keys.json')))
R_LIM = {32: 13, 128: 11, 256: 9}                 # level2_0 / level3_0 / level4_0 of ESPDNet(-UE) s = 2.0 (models.py)
# input sizes of the three blocks for 288x480, 256x480 and 512x1024 images
SIZES = {32: ((144, 240), (128, 240), (256, 512)), 128: ((72, 120), (64, 120), (128, 256)), 256: ((36, 60), (32, 60), (64, 128))}
BLOCKS = ((32, 128), (128, 256), (256, 512))


def _block(nin, nout, reinf, seed=31):
    from mspl_amd import layers
    m = torch.nn.ModuleDict({'d': layers.DownSampler(nin, nout, k=4, r_lim=R_LIM[nin], reinf=reinf)})
    sd = synth_state_dict(m.state_dict(), seed)
    m.load_state_dict(sd)
    return m.to(DEV).eval()['d'], sd


def _ref64(sd, nin, x, image):
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return onet.downsampler(x.double(), sd64, 'd', R_LIM[nin], None if image is None else image.double())


def _run(block, x, image, fused, monkeypatch):
    """(output, plane-sum partials) of the block with the head launch on or off."""
    from mspl_amd import layers
    monkeypatch.setattr(layers, '_FUSED_DOWN_HEAD', fused)
    xd = x.to(DEV)
    with torch.no_grad():
        out = block(xd, None if image is None else image.to(DEV))
    sums = layers._recall_plane_sums(xd)
    assert sums is not None
    torch.cuda.synchronize()
    return out.cpu(), sums.cpu()


def _rel_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _head_on(nin, nout, H, W):
    from mspl_amd import ops
    return ops.down_head_fits((1, nin, H, W), (nout - nin) // 4, 4)


CASES = [(2, nin, nout, h, w, reinf, False) for nin, nout in BLOCKS for h, w in SIZES[nin] for reinf in (True, False)]
# batch 16 at the label pass's size: the chain's projection is the vector-unit kernel there (k ascending): whole output bit-identical
CASES += [(16, 32, 128, 144, 240, True, True), (16, 128, 256, 72, 120, True, True), (16, 32, 128, 144, 240, False, True)]


@pytest.mark.parametrize('N,nin,nout,H,W,reinf,bitwise', CASES)
def test_block_vs_chain_and_float64(N, nin, nout, H, W, reinf, bitwise, monkeypatch):
    block, sd = _block(nin, nout, reinf)
    x = synth_input((N, nin, H, W), 100 + nin + W)
    image = synth_input((N, 3, H, W), 200 + W) if reinf else None          # one pool away from the block's output size
    fused, fsum = _run(block, x, image, True, monkeypatch)
    chain, csum = _run(block, x, image, False, monkeypatch)
    ref = _ref64(sd, nin, x, image)
    assert fused.shape == (N, nout, H // 2, W // 2)
    scale = float(ref.abs().max())                                         # errors are relative to the largest |output|
    ef = float((fused[:, nin:].double() - ref[:, nin:]).abs().max()) / scale
    ec = float((chain[:, nin:].double() - ref[:, nin:]).abs().max()) / scale
    ep = float((fused[:, :nin].double() - ref[:, :nin]).abs().max()) / scale
    print('down_head N=%d %d->%d %dx%d reinf=%d head=%d: expansion half fused %.3e chain %.3e, pooled half %.3e (relative to max |out| = %.3f)'
          ' bit-identical: whole %s' % (N, nin, nout, H, W, reinf, _head_on(nin, nout, H, W), ef, ec, ep, scale, torch.equal(fused, chain)))
    assert torch.equal(fused[:, :nin], chain[:, :nin])                     # the pooled half: bit-identical
    assert ef <= 2.0 * ec
    if bitwise:
        assert _head_on(nin, nout, H, W)
        assert torch.equal(fused, chain)
    # plane sums: fixed-order partials, within the summation bound of the float64 sums
    xs = x.double()
    exact, mag = xs.sum((2, 3)).reshape(-1), xs.abs().sum((2, 3)).reshape(-1)
    for name, s in (('fused', fsum), ('chain', csum)):
        d = 3 + 1 + 7 + 2 + s.shape[1]
        err = (s.double().sum(1) - exact).abs()
        worst = float((err / mag).max())
        print('   plane sums %s: %d slots, worst |err| / sum|x| %.3e (bound %.3e)' % (name, s.shape[1], worst, d * 2.0 ** -24 * 1.01))
        assert worst <= d * 2.0 ** -24 * 1.01


@pytest.mark.parametrize('nin,nout,H,W', [(32, 128, 144, 240), (128, 256, 72, 120)])
def test_two_runs_are_bit_identical(nin, nout, H, W, monkeypatch):
    block, _ = _block(nin, nout, True)
    x, image = synth_input((4, nin, H, W), 5), synth_input((4, 3, H, W), 6)
    assert _head_on(nin, nout, H, W)
    a, asum = _run(block, x, image, True, monkeypatch)
    b, bsum = _run(block, x, image, True, monkeypatch)
    assert torch.equal(a, b) and torch.equal(asum, bsum)


@pytest.mark.parametrize('nin,nout,H,W', [(32, 128, 144, 240), (128, 256, 72, 120), (32, 128, 6, 520), (128, 256, 10, 24)])
def test_head_launch_against_its_two_launches(nin, nout, H, W):
    """The head launch alone, batch 16: the reduced tensor against mspl_conv1x1_fwd (bit-identical where that call takes the
    vector-unit kernel; otherwise within 2x its error against float64), the pooled channels and the plane-sum partials against
    mspl_avgpool3x3s2_psum_fwd's DownSampler form (same slot layout, bit-identical).  The last two shapes have a half-empty last
    workgroup and rows shorter / longer than a wave."""
    from mspl_amd import ops
    from mspl_amd.ops import Epi
    N, n = 16, (nout - nin) // 4
    g = torch.Generator().manual_seed(nin + W)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, wp = rn(N, nin, H, W), rn(n, nin // 4) * (4.0 / nin) ** 0.5
    ps, pb, pa = rn(n), rn(n) * 0.5, rn(n) * 0.5
    sc, sh, al, rw = rn(nout), rn(nout) * 0.5, rn(nout) * 0.5, rn(nout, 3) * 0.3
    rr = rn(N, 3, H // 2, W // 2)
    c = [t.to(DEV) for t in (x, wp, ps, pb, pa, sc, sh, al, rw, rr)]
    xd, wpd, psd, pbd, pad, scd, shd, ald, rwd, rrd = c
    canary = 12345.0
    out = torch.full((N, nout, H // 2, W // 2), canary, device=DEV)
    out0 = torch.full_like(out, canary)
    ep = Epi(scd, shd, ald, reinf_r=rrd, reinf_w=rwd)
    r, sums = ops.down_head(xd, wpd, psd, pbd, pad, 4, ep, out)
    r0 = ops.conv1x1(xd, wpd, 4, Epi(psd, pbd, pad))
    _, sums0 = ops.avgpool3x3s2(xd, ep, out=(out0, 0), plane_sums=True)
    torch.cuda.synchronize()
    assert bool((out[:, nin:] == canary).all())                            # only channels [0, nin) are written
    assert torch.equal(out, out0)
    assert sums.shape == sums0.shape and torch.equal(sums, sums0)
    ref = torch.einsum('gmk,ngkp->ngmp', wp.double().view(4, n // 4, nin // 4), x.double().view(N, 4, nin // 4, H * W)).reshape(N, n, H, W)
    ref = ref * ps.double().view(1, -1, 1, 1) + pb.double().view(1, -1, 1, 1)
    ref = torch.where(ref > 0, ref, ref * pa.double().view(1, -1, 1, 1))
    ef, ec = _rel_err(r.cpu(), ref), _rel_err(r0.cpu(), ref)
    same = torch.equal(r, r0)
    print('down_head %d->%d %dx%d: reduced tensor fused %.3e, conv1x1 %.3e, bit-identical %s' % (nin, n, H, W, ef, ec, same))
    assert ef <= 2.0 * ec
    if 16 * 4 * -(-(H * W // 4) // 256) >= 400:                            # mspl_conv1x1_fwd's rule for its vector-unit kernel
        assert same


@pytest.mark.parametrize('nin,nout,H,W', [(32, 128, 144, 240), (128, 256, 72, 120)])
def test_batch_independence(nin, nout, H, W, monkeypatch):
    """Image i of a batch of 16 equals the same image run alone, bit for bit (launch shapes never depend on N)."""
    from mspl_amd import layers, ops
    block, _ = _block(nin, nout, True)
    x, image = synth_input((16, nin, H, W), 9), synth_input((16, 3, H, W), 10)
    monkeypatch.setattr(layers, '_FUSED_DOWN_HEAD', True)
    i = 11
    with torch.no_grad():
        xd, imd = x.to(DEV), image.to(DEV)
        full = block(xd, imd)
        fsum = layers._recall_plane_sums(xd)
        x1, im1 = xd[i:i + 1].contiguous(), imd[i:i + 1].contiguous()
        one = block(x1, im1)
        osum = layers._recall_plane_sums(x1)
        # the head launch on its own as well (the strided K2 and the expansion are today's launches)
        pj = block.eesp.proj_1x1
        sc, sh, rw = block._epilogue_vectors(False)
        ep = ops.Epi(sc, sh, block.act.weight)
        pscale, pshift = layers.bn_fold(pj.bn)
        o16, o1 = torch.zeros_like(full), torch.zeros_like(one)
        r16, _ = ops.down_head(xd, pj.conv.weight, pscale, pshift, pj.act.weight, 4, ep, o16)
        r1, _ = ops.down_head(x1, pj.conv.weight, pscale, pshift, pj.act.weight, 4, ep, o1)
    assert torch.equal(r16[i:i + 1], r1) and torch.equal(o16[i:i + 1], o1)
    assert torch.equal(fsum.view(16, nin, -1)[i], osum.view(nin, -1))
    assert torch.equal(full[i:i + 1], one)


@pytest.mark.parametrize('nin,nout,H,W', [(128, 256, 8, 44), (32, 128, 37, 240), (256, 512, 36, 60), (32, 128, 16, 244)])
def test_rejected_shapes_take_todays_launches(nin, nout, H, W, monkeypatch):
    """352-pixel-wide images (44 columns at level 3), odd heights, widths off the 8-column strip grid and the level-4 block (16
    reduced channels per group) are declined by mspl_down_head_fits: DownSampler.forward runs the projection and the pool as two
    launches, with exactly their result."""
    from mspl_amd import ops
    assert not _head_on(nin, nout, H, W)
    block, sd = _block(nin, nout, True)
    x = synth_input((2, nin, H, W), 3)
    image = synth_input((2, 3, H, W), 4)
    calls = []
    real = ops.down_head
    monkeypatch.setattr(ops, 'down_head', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    a, asum = _run(block, x, image, True, monkeypatch)
    b, bsum = _run(block, x, image, False, monkeypatch)
    assert not calls
    assert torch.equal(a, b) and torch.equal(asum, bsum)
    print('rejected %d->%d %dx%d: error against float64 %.3e' % (nin, nout, H, W, _rel_err(a, _ref64(sd, nin, x, image))))


@pytest.mark.parametrize('shape', [(1, 3, 64, 1024), (2, 3, 48, 512), (2, 3, 96, 160)])
def test_model_head_launch_on_and_off(shape, monkeypatch):
    """ESPDNet-UE (s = 2.0, 20 classes) with the head launch on and off: both meet the CPU oracle within 2e-4 (+ 1e-4 relative, the
    tolerance of tests/test_gpu_parity.py's model test); the label agreement between the two is reported."""
    from mspl_amd import layers, ops
    from tests.test_gpu_parity import _build_model
    m = _build_model('espdnetue', 2.0, 20, 'city')
    sd = synth_state_dict(KEYS['espdnetue_s2.0_c20'], 21)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    x = synth_input(shape, 77)
    calls = []
    real = ops.down_head
    monkeypatch.setattr(ops, 'down_head', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        monkeypatch.setattr(layers, '_FUSED_DOWN_HEAD', True)
        main, aux = m(x.to(DEV))
        assert len(calls) == 2                                    # level2_0 and level3_0; level4_0 keeps its launches
        monkeypatch.setattr(layers, '_FUSED_DOWN_HEAD', False)
        main0, aux0 = m(x.to(DEV))
        assert len(calls) == 2
        rmain, raux = onet.espdnet_ue_forward(sd, x)
    for a in (main, main0):
        torch.testing.assert_close(a.cpu(), rmain, rtol=1e-4, atol=2e-4)
    for a in (aux, aux0):
        torch.testing.assert_close(a.cpu(), raux, rtol=1e-4, atol=2e-4)
    agree = float((main.argmax(1) == main0.argmax(1)).float().mean())
    print('head launch on vs off %s: max |d logit| %.3e, label agreement %.6f' % (shape, float((main - main0).abs().max()), agree))
