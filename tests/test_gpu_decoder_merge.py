"""The head of a decoder stage as one launch (mspl_decoder_merge_fwd: grouped 3x3 of the skip + BN + PReLU + gate, x2 bilinear
up-merge + BN + PReLU, projection 1x1 + BN + PReLU) against (a) the three launches it replaces and (b) the same formula in torch
float64 on the CPU.  Needs a real MI355X: run with `-m gpu`.

Bound of the op-level checks: both (a) and the fused launch are fp32 evaluations of the same expression whose last step is a sum
of <= 64 products, at most in another order, so the fused launch's largest error against (b), relative to the largest |value| of
the output, must not exceed TWICE that of (a) on the same inputs.  Where (a)'s projection runs on the vector unit
(conv1x1_thin_kernel: the 32 -> P projection at 144x240 from batch 16 on) the fused launch walks the channels in the same order
and must be bit-identical.  Edge regions hold too few values for a ratio of two maxima to mean anything; they are held to
(64 + 16) * 2^-23 ~= 1e-5 of the largest |value| instead: 64 products plus the ~16 roundings each term carries from the 3x3, the
bilinear blend and the two BN + PReLU epilogues.  A wrong padding, clamp or halo column is an error of order 1.
"""
import ctypes
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import net as onet
from tests.conftest import GOLDEN
from tests.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = json.load(open(os.path.join(GOLDEN, 'state_dict_keys.json')))
EDGE_REL = 1e-5


def _inputs(N, Cin, Cout, P, H, W, seed, gate=None):
    g = torch.Generator().manual_seed(seed)
    groups = math.gcd(Cin, Cout)

    def rn(*shape, s=1.0):
        return torch.randn(*shape, generator=g) * s
    d = {
        'enc': rn(N, Cin, H, W), 'bu': rn(N, Cout, H // 2, W // 2),
        'w3': rn(Cout, Cin // groups, 3, 3, s=1.0 / math.sqrt(9 * Cin // groups)),
        # BN constants and PReLU slopes of both signs
        'es': rn(Cout), 'eb': rn(Cout, s=0.5), 'ea': rn(Cout, s=0.5),
        'bs': rn(Cout), 'bb': rn(Cout, s=0.5), 'ba': rn(Cout, s=0.5),
        'wp': rn(P, Cout, s=1.0 / math.sqrt(Cout)),
        'ps': rn(P), 'pb': rn(P, s=0.5), 'pa': rn(P, s=0.5),
    }
    if gate is None:
        d['gate'] = torch.sigmoid(rn(N, Cout))
    else:
        d['gate'] = torch.full((N, Cout), float(gate))
    return d, groups


def _prelu(v, alpha):
    return torch.where(v > 0, v, v * alpha.view(1, -1, 1, 1))


def _ref64(d, groups):
    t = {k: v.double() for k, v in d.items()}
    H, W = t['enc'].shape[2:]
    pw = F.conv2d(t['enc'], t['w3'], padding=1, groups=groups)
    pw = _prelu(pw * t['es'].view(1, -1, 1, 1) + t['eb'].view(1, -1, 1, 1), t['ea']) * t['gate'][:, :, None, None]
    up = F.interpolate(t['bu'], size=(H, W), mode='bilinear', align_corners=True)
    m = _prelu((pw + up) * t['bs'].view(1, -1, 1, 1) + t['bb'].view(1, -1, 1, 1), t['ba'])
    pr = torch.einsum('pc,nchw->nphw', t['wp'], m)
    return _prelu(pr * t['ps'].view(1, -1, 1, 1) + t['pb'].view(1, -1, 1, 1), t['pa'])


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


def _run(N, Cin, Cout, P, H, W, seed, gate=None):
    d, groups = _inputs(N, Cin, Cout, P, H, W, seed, gate)
    c = {k: v.to(DEV) for k, v in d.items()}
    fused = _fused(c)
    assert fused is not None, 'shape (%d,%d) P=%d %dx%d was not fused' % (Cin, Cout, P, H, W)
    chain = _chain(c, groups)
    torch.cuda.synchronize()
    return fused.cpu(), chain.cpu(), _ref64(d, groups)


def _rel_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


# the nine (channel pair, width family) stage shapes of the bench workloads (480-, 512- and 1024-wide inputs) at N = 2,
# the 32 -> 32 stage at N = 16 (there the chain's projection is conv1x1_thin_kernel: bit-identity), P = 2 / 6 / 10
CASES = [(2, cin, cout, 16, h, w, False)
         for (cin, cout), sizes in (((32, 32), ((144, 240), (128, 256), (256, 512))),
                                    ((128, 48), ((72, 120), (64, 128), (128, 256))),
                                    ((256, 64), ((36, 60), (32, 64), (64, 128))))
         for h, w in sizes]
CASES += [(16, 32, 32, 16, 144, 240, True), (16, 32, 32, 10, 144, 240, True),
          (2, 32, 32, 2, 144, 240, False), (2, 32, 32, 6, 144, 240, False), (2, 32, 32, 10, 144, 240, False)]


@pytest.mark.parametrize('N,Cin,Cout,P,H,W,bitwise', CASES)
def test_fused_vs_chain_and_float64(N, Cin, Cout, P, H, W, bitwise):
    fused, chain, ref = _run(N, Cin, Cout, P, H, W, 1000 + Cin + P + W + N)
    ef, ec = _rel_err(fused, ref), _rel_err(chain, ref)
    print('decoder_merge N=%d %d->%d P=%d %dx%d: fused %.3e  chain %.3e  (relative to max |out| = %.3f)'
          % (N, Cin, Cout, P, H, W, ef, ec, float(ref.abs().max())))
    assert fused.shape == (N, P, H, W)
    assert ef <= 2.0 * ec
    if bitwise:
        assert torch.equal(fused, chain)


@pytest.mark.parametrize('Cin,Cout,H,W', [
    (32, 32, 6, 60),        # two row pairs per wave, three row pairs: the last wave is half empty
    (32, 32, 10, 120),      # one row pair per wave, 60 of 64 lanes
    (32, 32, 8, 240),       # two column blocks: halo columns fetched by the edge lanes
    (32, 32, 4, 130),       # 65 lanes of work in two blocks of 33: dead lanes inside the second block
    (128, 48, 6, 120), (128, 48, 4, 132),
    (256, 64, 6, 60), (256, 64, 4, 16), (256, 64, 10, 24),
])
@pytest.mark.parametrize('gate', [None, 0.0, 1.0])
def test_edges(Cin, Cout, H, W, gate):
    fused, chain, ref = _run(3, Cin, Cout, 16, H, W, 7 + H + W, gate)
    scale = float(ref.abs().max())
    assert float((chain.double() - ref).abs().max()) <= EDGE_REL * scale          # the yardstick itself
    for name, sl in (('first row', (slice(None), slice(None), slice(0, 1))), ('last row', (slice(None), slice(None), slice(H - 1, H))),
                     ('first column', (Ellipsis, slice(0, 1))), ('last column', (Ellipsis, slice(W - 1, W)))):
        err = float((fused[sl].double() - ref[sl]).abs().max())
        assert err <= EDGE_REL * scale, '%s: %.3e against %.3e' % (name, err, EDGE_REL * scale)
    err = float((fused.double() - ref).abs().max())
    assert err <= EDGE_REL * scale


@pytest.mark.parametrize('Cin,Cout,H,W', [(32, 32, 144, 240), (32, 32, 16, 60), (128, 48, 72, 120), (256, 64, 36, 60)])
def test_batch_independence(Cin, Cout, H, W):
    """An image's result does not depend on the batch it travels in (the launch shape is chosen per image, never by N)."""
    d, _ = _inputs(5, Cin, Cout, 16, H, W, 11)
    c = {k: v.to(DEV) for k, v in d.items()}
    full = _fused(c)
    one = _fused({k: (v[3:4].contiguous() if k in ('enc', 'bu', 'gate') else v) for k, v in c.items()})
    assert torch.equal(full[3:4], one)


def test_output_buffer_canary():
    """The launch writes N*P*H*W floats and nothing around them (odd tile counts: dead lanes and a half-empty last wave)."""
    from mspl_amd import _native as nat
    N, Cin, Cout, P, H, W = 3, 32, 32, 16, 6, 130
    d, groups = _inputs(N, Cin, Cout, P, H, W, 5)
    c = {k: v.to(DEV).contiguous() for k, v in d.items()}
    n, pad = N * P * H * W, 4096
    buf = torch.full((pad + n + pad,), 12345.0, device=DEV)
    out = buf[pad:pad + n]
    assert out.data_ptr() % 16 == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = nat.lib.mspl_decoder_merge_fwd(p(c['enc']), p(c['bu']), p(c['w3']), p(c['es']), p(c['eb']), p(c['ea']), p(c['gate']),
                                        p(c['bs']), p(c['bb']), p(c['ba']), p(c['wp']), p(c['ps']), p(c['pb']), p(c['pa']),
                                        N, Cin, Cout, P, H, W, p(out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    nat.check(rc)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 12345.0).all()) and bool((buf[pad + n:] == 12345.0).all())
    ref = _ref64(d, groups)
    assert _rel_err(out.view(N, P, H, W).cpu(), ref) <= EDGE_REL


@pytest.mark.parametrize('Cin,Cout,P,H,W', [(64, 48, 16, 8, 32), (32, 32, 32, 8, 32), (32, 32, 16, 8, 32)])
def test_unsupported_shapes_take_the_three_launches(Cin, Cout, P, H, W):
    """Group shapes and projection widths outside the fused set are declined by the library (nothing is launched) and the stage
    runs conv3x3, bilinear and conv1x1 with the result the unfused modules give.  The last case IS a fused shape: the same helper
    then returns the fused result."""
    from mspl_amd import layers, models, ops
    m = torch.nn.ModuleDict({
        'merge': layers.EfficientPWConv(Cin, Cout),
        'br': torch.nn.Sequential(torch.nn.BatchNorm2d(Cout), torch.nn.PReLU(Cout)),
        'pyr': layers.EfficientPyrPool(in_planes=Cout, proj_planes=P, out_planes=24)})
    m.load_state_dict(synth_state_dict(m.state_dict(), 55))
    m = m.to(DEV).eval()
    merge, br, pyr = m['merge'], m['br'], m['pyr']
    enc, bu = synth_input((2, Cin, H, W), 3).to(DEV), synth_input((2, Cout, H // 2, W // 2), 4).to(DEV)
    supported = (Cin, Cout, P) == (32, 32, 16)
    with torch.no_grad():
        assert layers.decoder_stage_fusable(merge, enc, pyr) == supported
        gate = merge.gate(enc)
        proj = layers.decoder_stage_fused(merge, enc, gate, bu, br, pyr)
        assert (proj is not None) == supported
        want = pyr(layers.decoder_merge(merge(enc), bu, br))
        got = models._SegBase._decode_stage((merge, br, pyr), enc, gate, bu)        # handed a gate: fused, or declined -> three launches
    if supported:
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5)
    else:
        assert torch.equal(got, want)


@pytest.mark.parametrize('shape', [(1, 3, 64, 1024), (2, 3, 48, 512), (2, 3, 96, 160)])
def test_model_fused_and_unfused_decoder_stages(shape, monkeypatch):
    """ESPDNet-UE (s = 2.0, 20 classes, P = 16) with the fused decoder stages on and off: both meet the CPU oracle at the tolerance
    of test_model_wide_inputs_fused_and_fallback (2e-4 + 1e-4 relative), and they agree with each other within a quarter of the
    4e-4 that two results 2e-4 from the oracle may be apart: the fused stages only reorder three sums of <= 64 fp32 products
    (relative 64 * 2^-24 ~= 4e-6 of the stage's largest value each), which the three pyramid blocks that follow do not amplify
    by anything near 25x.  Label agreement between the two is reported."""
    from mspl_amd import layers
    from tests.test_gpu_parity import _build_model
    m = _build_model('espdnetue', 2.0, 20, 'city')
    sd = synth_state_dict(KEYS['espdnetue_s2.0_c20'], 21)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    x = synth_input(shape, 77)
    calls = []
    real = layers.ops.decoder_merge
    monkeypatch.setattr(layers.ops, 'decoder_merge', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        main, aux = m(x.to(DEV))
        assert len(calls) == 3                                    # every stage of this model is a fused shape
        monkeypatch.setattr(layers, '_FUSED_DEC_MERGE', False)
        main0, aux0 = m(x.to(DEV))
        assert len(calls) == 3
        rmain, raux = onet.espdnet_ue_forward(sd, x)
    for a in (main, main0):
        torch.testing.assert_close(a.cpu(), rmain, rtol=1e-4, atol=2e-4)
    for a in (aux, aux0):
        torch.testing.assert_close(a.cpu(), raux, rtol=1e-4, atol=2e-4)
    torch.testing.assert_close(main, main0, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(aux, aux0, rtol=1e-4, atol=1e-4)
    agree = float((main.argmax(1) == main0.argmax(1)).float().mean())
    print('fused vs unfused decoder stages %s: max |d logit| %.3e, label agreement %.6f'
          % (shape, float((main - main0).abs().max()), agree))
