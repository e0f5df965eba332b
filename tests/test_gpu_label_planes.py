"""The label epilogue that computes both heads' final 1x1 classifier from the heads' planes (ops.label_epilogue_planes,
mspl_label_epilogue_planes_fwd) against the chain it replaces: ops.conv1x1 of each head, then ops.label_epilogue[_hist].

The planes form sums a logit as the chain's 1x1 kernels do (k ascending, fused multiply-adds, then the bias), for the main and
for the aux head, so labels, KL map and histogram are asserted BIT-IDENTICAL to the chain in every case.  Independently of that,
every case is also held against a float64 evaluation of the formula on the CPU: labels equal wherever the float64 top-2 margin
exceeds 1e-4 * max|o| (at most 1 % of the pixels may be excluded by that rule), the histogram equals the bincount of the labels
written, and the KL error against float64 is at most twice the chain's own.
"""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (C, Hm, Wm, Ha, Wa, H, W, N)
CASES = {
    'wide480': (13, 6, 240, 3, 120, 12, 480, 1),       # the 480-wide instantiation, 16-byte rows
    'rows4_c5': (5, 8, 12, 4, 6, 16, 24, 2),           # 4-byte aux rows
    'rows4_c13': (13, 8, 12, 4, 6, 16, 24, 2),
    'blocks2_c20': (20, 9, 130, 5, 65, 18, 260, 2),    # two column blocks, odd sizes, a ragged last band
}


def _heads(case, P=16, seed=0, aux=True):
    """N(0,1) planes, N(0,0.25) weights, N(0,1) bias (the distribution the float64 exclusion rate was checked for)."""
    C, Hm, Wm, Ha, Wa, H, W, N = case
    g = torch.Generator().manual_seed(1234 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    main = (r(N, P, Hm, Wm), r(C, P, 1, 1) * 0.5, r(C))
    auxh = (r(N, P, Ha, Wa), r(C, P, 1, 1) * 0.5, r(C)) if aux else None
    return main, auxh


def _dev(head):
    return None if head is None else tuple(t.to(DEV) for t in head)


def _f64(main, aux, size):
    """float64 on the CPU: logits of both heads, bilinear (align_corners) to `size`, o = main + 0.5 aux, KL(main || aux)."""
    def up(head):
        planes, w, b = (t.double() for t in head)
        lo = torch.einsum('cp,nphw->nchw', w.flatten(1), planes) + b.view(1, -1, 1, 1)
        return F.interpolate(lo, size=size, mode='bilinear', align_corners=True)
    m = up(main)
    a = up(aux) if aux is not None else None
    o = m if a is None else m + 0.5 * a
    top2 = torch.topk(o, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4 * float(o.abs().max())
    kl = torch.zeros_like(o[:, 0])
    if a is not None:
        lm, la = F.log_softmax(m, 1), F.log_softmax(a, 1)
        kl = (lm.exp() * (lm - la)).sum(1)
    return o.argmax(1), clear, kl


def _chain(main, aux, size, C, lut=None, want_kld=True, with_hist=True):
    from mspl_amd import ops
    lm = ops.conv1x1(main[0], main[1], 1, ops.Epi(shift=main[2]))
    la = None if aux is None else ops.conv1x1(aux[0], aux[1], 1, ops.Epi(shift=aux[2]))
    if not with_hist:
        return ops.label_epilogue(lm, la, size, lut=lut, want_kld=want_kld), None
    hist = torch.zeros(C, dtype=torch.int64, device=DEV)
    return ops.label_epilogue_hist(lm, la, size, hist, C, lut=lut, want_kld=want_kld), hist


def _planes(main, aux, size, C, lut=None, want_kld=True, with_hist=True):
    from mspl_amd import ops
    assert ops.label_epilogue_planes_fits(main, aux, size)
    hist = torch.zeros(C, dtype=torch.int64, device=DEV) if with_hist else None
    return ops.label_epilogue_planes(main, aux, size, hist, C if with_hist else 0, lut=lut, want_kld=want_kld), hist


def _check(case, P=16, aux=True, lut=None, want_kld=True, with_hist=True, seed=0):
    C, Hm, Wm, Ha, Wa, H, W, N = case
    main, auxh = _heads(case, P, seed, aux)
    dm, da = _dev(main), _dev(auxh)
    lut_d = None if lut is None else torch.tensor(lut, dtype=torch.uint8, device=DEV)
    want, hw = _chain(dm, da, (H, W), C, lut_d, want_kld, with_hist)
    got, hg = _planes(dm, da, (H, W), C, lut_d, want_kld, with_hist)
    ref_lab, clear, ref_kl = _f64(main, auxh, (H, W))
    if lut is not None:
        ref_lab = torch.tensor(lut, dtype=torch.int64)[ref_lab]
    lab = got['labels'].cpu().long()
    excluded = 1.0 - float(clear.float().mean())
    print('%s P=%d aux=%s: float64 margin rule excludes %.3f %% of the pixels; labels differing from the chain: %d'
          % (case, P, aux, 100 * excluded, int((got['labels'] != want['labels']).sum())))
    # against float64
    assert excluded <= 0.01
    assert torch.equal(lab[clear], ref_lab[clear])
    if with_hist:
        np.testing.assert_array_equal(hg.cpu().numpy(), np.bincount(lab.numpy().ravel(), minlength=C)[:C])
    else:
        assert hg is None
    if want_kld:
        e_got = float((got['kld'].cpu().double() - ref_kl).abs().max())
        e_chain = float((want['kld'].cpu().double() - ref_kl).abs().max())
        print('   KL map: max error against float64 %.3e (chain %.3e)' % (e_got, e_chain))
        assert e_got <= 2 * e_chain
    else:
        assert 'kld' not in got
    # against the chain: the same bits
    assert torch.equal(got['labels'], want['labels'])
    if want_kld:
        assert torch.equal(got['kld'], want['kld'])
    if with_hist:
        assert torch.equal(hg, hw)
    return dm, da, got


@pytest.mark.parametrize('name', sorted(CASES))
def test_planes_equal_the_chain(name):
    case = CASES[name]
    dm, da, got = _check(case)
    C, Hm, Wm, Ha, Wa, H, W, N = case
    if N > 1:
        # batch independence: image 1 of the batch equals the image alone, bit for bit
        from mspl_amd import ops
        one = lambda h: (h[0][1:2].contiguous(), h[1], h[2])
        solo = ops.label_epilogue_planes(one(dm), one(da), (H, W), None, 0, want_kld=True)
        assert torch.equal(solo['labels'][0], got['labels'][1]) and torch.equal(solo['kld'][0], got['kld'][1])


def test_planes_single_head():
    _check(CASES['rows4_c13'], aux=False, seed=1)
    _check(CASES['wide480'], aux=False, seed=2)


def test_planes_with_lut():
    from mspl_amd import uest
    _check(CASES['rows4_c13'], lut=[int(v) for v in uest.id_camvid_to_greenhouse], seed=3)


def test_planes_without_kl_map():
    _check(CASES['rows4_c13'], want_kld=False, seed=4)


def test_planes_without_histogram():
    _check(CASES['rows4_c13'], with_hist=False, seed=5)
    _check(CASES['blocks2_c20'], with_hist=False, want_kld=False, seed=6)


def test_planes_eight_planes():
    _check(CASES['rows4_c13'], P=8, seed=7)
    _check(CASES['wide480'], P=8, seed=8)


def test_declined_shapes():
    from mspl_amd import layers, ops, uest
    z = lambda *s: torch.zeros(*s, device=DEV)
    head = lambda P, C, h, w: (z(1, P, h, w), z(C, P, 1, 1), z(C))
    assert ops.label_epilogue_planes_fits(head(16, 13, 8, 12), head(16, 13, 4, 6), (16, 24))
    assert not ops.label_epilogue_planes_fits(head(32, 13, 8, 12), head(32, 13, 4, 6), (16, 24))       # P = 32
    assert not ops.label_epilogue_planes_fits(head(16, 25, 8, 12), head(16, 25, 4, 6), (16, 24))       # C = 25
    assert not ops.label_epilogue_planes_fits(head(6, 13, 8, 12), None, (16, 24))                      # P not a multiple of 4
    with pytest.raises(RuntimeError, match='planes form'):
        ops.label_epilogue_planes(head(32, 13, 8, 12), None, (16, 24))
    # a head with the final BN + PReLU has no bare classifier to hand over: it returns its activations as before
    with torch.random.fork_rng(devices=[]):              # (the modules draw their initial weights: leave the global stream alone)
        torch.manual_seed(0)
        pyr = layers.EfficientPyrPool(24, 16, 13, last_layer_br=True).to(DEV).eval()
        bare = layers.EfficientPyrPool(24, 16, 13, last_layer_br=False).to(DEV).eval()
        x = torch.randn(2, 24, 16, 24).to(DEV)
    with torch.no_grad():
        out = pyr(x, planes=True)
        assert isinstance(out, torch.Tensor) and torch.equal(out, pyr(x))
        planes = bare(x, planes=True)
        assert isinstance(planes, tuple) and tuple(planes[0].shape) == (2, 16, 16, 24)
        assert torch.equal(uest._head_logits(planes), bare(x))


# ---------------------------------------------------------------------------------------------------------------- model level
def _net(C):
    from mspl_amd import models
    from tests.synth import synth_state_dict
    a = argparse.Namespace(s=2.0, channels=3, num_classes=1000)
    ds = {13: 'camvid', 20: 'city'}[C]
    m = models.ESPDNetwithUncertaintyEstimation(a, classes=C, dataset=ds, fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), 11))
    return m.to(DEV).eval()


@pytest.mark.parametrize('C', [13, 20])
def test_self_label_pass_switch_on_equals_off(C, monkeypatch):
    """ESPDNet-UE s=2.0 on 2x3x64x96: the pass with the classifier folded into the epilogue (default) against the pass with the
    switch off -- eager, graphed (two replays) and pipelined; then with the library's `fits` answering no (today's launches
    from the planes).  Both heads' summation orders are reproduced: everything is bit-equal."""
    from mspl_amd import layers, ops, uest
    from tests.synth import synth_input
    m = _net(C)
    xs = [synth_input((2, 3, 64, 96), 40 + i).to(DEV) for i in range(4)]

    def eager_results():
        p = uest.SelfLabelPass(m, classes=C, device=DEV, use_graph=False)
        outs = [tuple(t.clone() for t in p(x)) for x in xs]
        return outs, p.hist.clone()

    monkeypatch.setattr(layers, '_FUSED_HEAD_CLASSIFIER', False)
    want, hist_want = eager_results()
    assert int(hist_want.sum()) == 4 * 2 * 64 * 96
    monkeypatch.setattr(layers, '_FUSED_HEAD_CLASSIFIER', True)
    calls = []
    real = ops.label_epilogue_planes
    monkeypatch.setattr(ops, 'label_epilogue_planes', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got, hist_got = eager_results()
    assert len(calls) == 4                                   # the new path really ran
    for (l1, k1), (l0, k0) in zip(got, want):
        assert torch.equal(l1, l0) and torch.equal(k1, k0)
    assert torch.equal(hist_got, hist_want)
    # graphed: two replays of the same batch equal the eager result and each other
    g = uest.SelfLabelPass(m, classes=C, device=DEV, use_graph=True)
    first = tuple(t.clone() for t in g(xs[0]))
    second = tuple(t.clone() for t in g(xs[0]))
    for a, b, c in zip(first, second, want[0]):
        assert torch.equal(a, b) and torch.equal(a, c)
    # pipelined
    plp = uest.PipelinedLabelPass(lambda: uest.SelfLabelPass(m, classes=C, device=DEV, use_graph=True), depth=2, group=2)
    outs = []
    for x in xs:
        o = plp(x)
        if o is not None:
            outs.append((o[0].clone(), o[1].clone()))
    outs += [(o[0].clone(), o[1].clone()) for o in plp.flush()]
    torch.cuda.synchronize()
    assert len(outs) == len(want)
    for (l1, k1), (l0, k0) in zip(outs, want):
        assert torch.equal(l1, l0) and torch.equal(k1, k0)
    assert torch.equal(plp.hist, hist_want)
    # the library declines: the classifier launches run from the planes, results unchanged
    monkeypatch.setattr(ops, 'label_epilogue_planes_fits', lambda *a: False)
    n = len(calls)
    back, hist_back = eager_results()
    assert len(calls) == n
    for (l1, k1), (l0, k0) in zip(back, want):
        assert torch.equal(l1, l0) and torch.equal(k1, k0)
    assert torch.equal(hist_back, hist_want)


def test_pseudo_label_pass_single_model_with_lut(monkeypatch):
    """PseudoLabelPass with one source model and its id LUT (no histogram in the epilogue): switch on == switch off."""
    from mspl_amd import layers, uest
    from tests.synth import synth_input
    m = _net(13)
    x = synth_input((2, 3, 64, 96), 50).to(DEV)
    monkeypatch.setattr(layers, '_FUSED_HEAD_CLASSIFIER', False)
    off = uest.PseudoLabelPass([m], ['camvid'], device=DEV)
    want, hist_want = off(x).clone(), off.hist.clone()
    monkeypatch.setattr(layers, '_FUSED_HEAD_CLASSIFIER', True)
    on = uest.PseudoLabelPass([m], ['camvid'], device=DEV)
    assert torch.equal(on(x), want) and torch.equal(on.hist, hist_want)
