"""The label epilogue in every kernel form and at every geometry seam (tests/label_cases.py; tests/test_label_cases.py proves from
the library's plan query which form each case reaches), and the cross-source label merge over every instantiation, against float64.

Labels: equal to the float64 first-max argmax on every clear pixel (top-2 margin above tau, at most 1 % of a case unclear -- both
decided by the reference alone).  KL map, probabilities, up-sampled logits: |kernel - float64| <= 4 * max(err32, floor), err32 the
float32 CPU evaluation's own error; every test prints the ratio it measured.  The forms against each other (histogram entry, planes
entry against the conv1x1 chain, an image alone against the image in its batch) and the whole merge: bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import label_cases as lc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LDS_NAMES = [c.name for c in lc.CASES if c.expect['form'] == 'lds']


def _dev_head(t, offset):
    if t is None:
        return None
    if not offset:
        d = t.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.zeros(t.numel() + 1, device=DEV)              # the head starts one float into the allocation
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _shape_of(main, aux, size):
    N, C, Hm, Wm = main.shape
    Ha, Wa = (0, 0) if aux is None else aux.shape[2:]
    return (N, C, Hm, Wm, Ha, Wa, size[0], size[1])


def _plan(main_d, aux_d, size, general=False):
    from mspl_amd import ops
    aligned = main_d.data_ptr() % 16 == 0 and (aux_d is None or aux_d.data_ptr() % 16 == 0)
    return ops.label_epilogue_plan(_shape_of(main_d, aux_d, size), general=general, aligned16=aligned)


def _labels_ok(what, labels, ref, lut=None):
    want = ref['labels'] if lut is None else torch.tensor(lut, dtype=torch.int64)[ref['labels']]
    got = labels.cpu().long()
    clear = ref['clear']
    bad = int((got[clear] != want[clear]).sum())
    assert bad == 0, '%s: %d clear pixels differ from the float64 argmax (%d of %d unclear)' % (what, bad, int((~clear).sum()), clear.numel())


def _value_ok(what, key, got, ref):
    err = float((got.cpu().double() - ref[key]).abs().max())
    bound = ref['bound'][key]
    print('%s %s: max error against float64 %.3e, float32 CPU error %.3e, ratio to the unit %.2f (bound %d)'
          % (what, key, err, ref['err32'][key], err / (bound / lc.MARGIN), lc.MARGIN))
    assert err <= bound, '%s %s: %.3e > %.3e' % (what, key, err, bound)


def _check_label_entries(what, main, aux, size, ref, offset=False):
    """The labels / KL entry with and without a LUT, the histogram entry where the LDS form takes the shape, each image alone."""
    from mspl_amd import ops
    md, ad = _dev_head(main, offset), _dev_head(aux, offset)
    N, C = main.shape[:2]
    plan = _plan(md, ad, size)
    got = ops.label_epilogue(md, ad, size, want_kld=True)
    _labels_ok(what, got['labels'], ref)
    _value_ok(what, 'kld', got['kld'], ref)
    if aux is None:
        assert float(got['kld'].abs().max()) == 0.0
    lut = lc.lut_of(C)
    lut_d = torch.tensor(lut, dtype=torch.uint8, device=DEV)
    mapped = ops.label_epilogue(md, ad, size, lut=lut_d, want_kld=True)
    _labels_ok(what + ' lut', mapped['labels'], ref, lut)
    assert torch.equal(mapped['labels'], lut_d[got['labels'].long()]) and torch.equal(mapped['kld'], got['kld'])
    only = ops.label_epilogue(md, ad, size)                                   # labels alone: the same labels
    assert torch.equal(only['labels'], got['labels']) and 'kld' not in only
    if plan['form'] == 'lds':
        assert ops.label_epilogue_hist_fits(md, ad, size)
        for lt, base in ((None, got), (lut_d, mapped)):
            start = torch.arange(3, 3 + C, dtype=torch.int64, device=DEV)
            hist = start.clone()
            fused = ops.label_epilogue_hist(md, ad, size, hist, C, lut=lt, want_kld=True)
            assert torch.equal(fused['labels'], base['labels']) and torch.equal(fused['kld'], base['kld'])
            counts = np.bincount(fused['labels'].cpu().numpy().ravel(), minlength=C)[:C]
            np.testing.assert_array_equal((hist - start).cpu().numpy(), counts)
    else:
        assert not ops.label_epilogue_hist_fits(md, ad, size)
        with pytest.raises(RuntimeError):
            ops.label_epilogue_hist(md, ad, size, torch.zeros(C, dtype=torch.int64, device=DEV), C)
    for n in range(N if N > 1 else 0):
        solo = ops.label_epilogue(md[n:n + 1].contiguous(), None if ad is None else ad[n:n + 1].contiguous(), size, want_kld=True)
        assert torch.equal(solo['labels'][0], got['labels'][n]) and torch.equal(solo['kld'][0], got['kld'][n]), 'image %d alone' % n
    return plan, got


def _check_general(what, main, aux, size, ref):
    """Probabilities and up-sampled logits asked for: the general kernel."""
    from mspl_amd import ops
    md, ad = _dev_head(main, False), _dev_head(aux, False)
    assert _plan(md, ad, size, general=True)['form'] == 'general'
    got = ops.label_epilogue(md, ad, size, want_prob=True, want_kld=True, want_logits=True)
    _labels_ok(what + ' general', got['labels'], ref)
    for key in ('main_up', 'prob', 'kld') + (('aux_up',) if aux is not None else ()):
        _value_ok(what + ' general', key, got[key], ref)
    assert ('aux_up' in got) == (aux is not None)
    return got


@pytest.mark.parametrize('name', lc.NAMES)
def test_label_forms_against_float64(name):
    case = lc.BY_NAME[name]
    main, aux, size, ref, _ = lc.problem(name)
    plan, got = _check_label_entries(name, main, aux, size, ref, case.offset)
    if case.offset:
        assert plan['form'] == 'lds' and plan['vec'] == 0
        aligned = _check_label_entries(name + ' aligned', main, aux, size, ref, False)
        assert aligned[0]['vec'] == 1                                         # both staging modes: the same bits
        assert torch.equal(aligned[1]['labels'], got['labels']) and torch.equal(aligned[1]['kld'], got['kld'])
    else:
        assert plan['form'] == case.expect['form']


@pytest.mark.parametrize('name', lc.NAMES)
def test_general_form_against_float64(name):
    main, aux, size, ref, _ = lc.problem(name)
    _check_general(name, main, aux, size, ref)


@pytest.mark.parametrize('name', lc.SINGLE_HEAD)
def test_single_head(name):
    main, aux, size, ref, _ = lc.problem(name, single_head=True)
    assert aux is None
    plan, got = _check_label_entries(name + ' 1 head', main, None, size, ref)
    assert float(got['kld'].abs().max()) == 0.0
    gen = _check_general(name + ' 1 head', main, None, size, ref)
    assert float(gen['kld'].abs().max()) == 0.0 and plan['nra'] == plan['pairs_aux'] == 0


@pytest.mark.parametrize('name,mag', lc.TRAINED)
def test_trained_magnitudes(name, mag):
    main, aux, size, ref, _ = lc.trained_problem(name, mag)
    what = '%s m%d' % (name, mag)
    plan, _ = _check_label_entries(what, main, aux, size, ref)
    assert plan['form'] == lc.BY_NAME[name].expect['form']
    _check_general(what, main, aux, size, ref)


@pytest.mark.parametrize('P', lc.PLANES_P)
@pytest.mark.parametrize('name', LDS_NAMES)
def test_planes_form(name, P):
    from mspl_amd import ops
    main, aux, size, ref = lc.planes_problem(name, P)
    C = main[1].shape[0]
    dm = tuple(t.to(DEV) for t in main)
    da = None if aux is None else tuple(t.to(DEV) for t in aux)
    assert ops.label_epilogue_planes_fits(dm, da, size), 'an LDS case the planes form declines'
    start = torch.arange(1, 1 + C, dtype=torch.int64, device=DEV)
    hist = start.clone()
    got = ops.label_epilogue_planes(dm, da, size, hist, C, want_kld=True)
    what = '%s P=%d' % (name, P)
    _labels_ok(what, got['labels'], ref)
    _value_ok(what, 'kld', got['kld'], ref)
    np.testing.assert_array_equal((hist - start).cpu().numpy(), np.bincount(got['labels'].cpu().numpy().ravel(), minlength=C)[:C])
    # the chain it replaces: the same bits
    lm = ops.conv1x1(dm[0], dm[1], 1, ops.Epi(shift=dm[2]))
    la = None if da is None else ops.conv1x1(da[0], da[1], 1, ops.Epi(shift=da[2]))
    chain = ops.label_epilogue(lm, la, size, want_kld=True)
    assert torch.equal(got['labels'], chain['labels']) and torch.equal(got['kld'], chain['kld'])


@pytest.mark.parametrize('name', lc.CANARY)
def test_output_canaries(name):
    """labels and kld inside larger buffers, 64 sentinel bytes on each side: ragged W must not spill a store over either end."""
    from mspl_amd import _native as nv
    from mspl_amd import ops
    main, aux, size, ref, _ = lc.problem(name)
    md, ad = main.to(DEV), aux.to(DEV)
    N, C, Hm, Wm, Ha, Wa, H, W = lc.BY_NAME[name].shape
    npx = N * H * W
    want = ops.label_epilogue(md, ad, size, want_kld=True)
    SENT = -1.2345e30
    lab = torch.full((npx + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    kld = torch.full((npx + 32,), SENT, dtype=torch.float32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    nv.check(nv.lib.mspl_label_epilogue_fwd(p(md), p(ad), N, C, Hm, Wm, Ha, Wa, H, W, None, p(lab, 64), None, p(kld, 64), None, None,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert bool((lab[:64] == 0xA5).all()) and bool((lab[64 + npx:] == 0xA5).all()), 'labels written outside (N, H, W)'
    assert bool((kld[:16] == SENT).all()) and bool((kld[16 + npx:] == SENT).all()), 'kld written outside (N, H, W)'
    assert torch.equal(lab[64:64 + npx].view(N, H, W), want['labels']) and torch.equal(kld[16:16 + npx].view(N, H, W), want['kld'])


# ---------------------------------------------------------------------------------------------------------------- the merge
def _merge(src_d, ncls, thresh, fill, start):
    from mspl_amd import ops
    hist = start.clone()
    out = ops.merge_labels(list(src_d), ncls, thresh, fill, hist)
    return out, hist - start


@pytest.mark.parametrize('S', lc.MERGE_S)
def test_merge_every_instantiation(S):
    """merge_labels_kernel<S, 8 | 16 | 32> against the contract in numpy, bit for bit: class counts on both sides of every NCLS
    instantiation, thresholds from 1 to S + 1, a counted and an uncounted fill, labels outside the classes, engineered ties, the
    vector path with its tail and (sources one byte into their buffer) the byte path."""
    from oracle import labels as olab
    for ncls in lc.MERGE_NCLS:
        start = torch.arange(5, 5 + ncls, dtype=torch.int64, device=DEV)
        for npix in lc.MERGE_NPIX:
            src = lc.merge_sources(S, ncls, npix)
            views = {'aligned': [torch.from_numpy(src[s]).to(DEV) for s in range(S)], 'byte offset': []}      # one allocation per source
            for s in range(S):
                buf = torch.zeros(npix + 1, dtype=torch.uint8, device=DEV)
                buf[1:] = views['aligned'][s]
                views['byte offset'].append(buf[1:])
            assert all(v.data_ptr() % 16 == 0 for v in views['aligned']) and all(v.data_ptr() % 16 == 1 for v in views['byte offset'])
            for thresh in lc.merge_thresholds(S):
                for fill in lc.MERGE_FILL:
                    want, want_hist = lc.merge_reference(src, ncls, thresh, fill)
                    if thresh == S + 1:
                        assert (want == fill).all()
                    if fill == olab.NO_AGREEMENT_CLASS and thresh <= S:
                        np.testing.assert_array_equal(want, olab.merge_outputs(src, ncls, int(thresh)))
                    for how, v in views.items():
                        if how == 'byte offset' and npix not in (17, 4099):
                            continue
                        out, hist = _merge(v, ncls, thresh, fill, start)
                        msg = 'S=%d ncls=%d npix=%d thresh=%d fill=%d %s' % (S, ncls, npix, thresh, fill, how)
                        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=msg)
                        np.testing.assert_array_equal(hist.cpu().numpy(), want_hist, err_msg=msg)


def test_merge_ties_take_the_first_maximum():
    """Two sources that never agree: every pixel is a 1 : 1 tie between two classes and the lower class must win, whichever source
    holds it; three sources 2 : 1 take the majority."""
    from mspl_amd import ops
    a = torch.tensor([3, 0, 7, 2, 31, 1] * 11, dtype=torch.uint8, device=DEV)
    b = torch.tensor([1, 4, 2, 7, 0, 30] * 11, dtype=torch.uint8, device=DEV)
    out = ops.merge_labels([a, b], 32, 1, 255)
    assert torch.equal(out, torch.minimum(a, b))
    assert torch.equal(ops.merge_labels([a, b, a], 32, 2, 255), a)
    assert bool((ops.merge_labels([a, b], 32, 2, 255) == 255).all())


def test_merge_grid_stride():
    """More 16-pixel chunks than 16384 workgroups of 256 threads hold: the only case that enters the kernel's grid-stride loop.
    Sources drawn on the device, reference by torch integer operations on the device (plumbing, independent of the kernel)."""
    from mspl_amd import ops
    npix, ncls, thresh, fill = lc.MERGE_BIG_NPIX, 5, 2, 4
    assert -(-(-(-npix // 16)) // 256) > 16384
    g = torch.Generator(device=DEV).manual_seed(5)
    src = [torch.randint(0, 7, (npix,), dtype=torch.uint8, device=DEV, generator=g) for _ in range(2)]      # 5, 6: outside the classes
    best = torch.zeros(npix, dtype=torch.uint8, device=DEV)
    bestc = torch.full((npix,), -1, dtype=torch.int8, device=DEV)
    for c in range(ncls):
        cn = (src[0] == c).to(torch.int8) + (src[1] == c).to(torch.int8)
        upd = cn > bestc                                                    # strictly greater: the first maximum stays
        best = torch.where(upd, torch.full_like(best, c), best)
        bestc = torch.where(upd, cn, bestc)
        del cn, upd
    want = torch.where(bestc < thresh, torch.full_like(best, fill), best)
    del best, bestc
    start = torch.arange(1, 1 + ncls, dtype=torch.int64, device=DEV)
    hist = start.clone()
    out = ops.merge_labels(src, ncls, thresh, fill, hist)
    assert torch.equal(out, want)
    counts = torch.stack([(want == c).sum() for c in range(ncls)])
    assert torch.equal(hist - start, counts) and int(counts.sum()) == npix         # fill = 4 is a counted class
    assert 0.05 < float((want != fill).double().mean()) < 0.5                      # both outcomes are there (both sources agree on 4 of 49 draws)
