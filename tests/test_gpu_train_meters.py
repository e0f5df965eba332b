"""mspl_uw_loss_heads_meters_fwd_bwd through the C ABI: the loss kernel at head resolution with the training loop's meters (the
three MIOU area histograms of the up-sampled main head, loss * batch size) taken inside it."""
import numpy as np
import pytest
import torch

from tests.synth import synth_input, synth_labels

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (N, C, main size, aux size, label size, K): the model's x2 / x4 heads; the predicated form for <= 8 classes; 13 and 20 classes on two
# column tiles with the second partly filled and a band shorter than TH; three images with K = C
CASES = [(2, 5, (16, 24), (8, 12), (32, 48), 4), (1, 3, (12, 20), (6, 10), (23, 39), 3), (1, 13, (8, 136), (4, 68), (16, 272), 12),
         (1, 20, (8, 136), (4, 68), (16, 272), 19), (3, 5, (24, 40), (12, 20), (48, 80), 5)]
IDS = ['n%dc%d_%dx%d_k%d' % (c[0], c[1], c[4][0], c[4][1], c[5]) for c in CASES]


def _inputs(case):
    N, C, ms, as_, size, K = case
    main = (synth_input((N, C) + ms, 700 + C) * 2).to(DEV)
    aux = (synth_input((N, C) + as_, 701 + C) * 2).to(DEV)
    tgt = synth_labels((N,) + size, C, 702 + C)            # every class id, the ignored one and (K < C) ids >= K included
    tgt[0, 0, :3] = 255                                    # void
    tgt[-1, -1, -2:] = C + 1                               # an id outside the model's classes (and >= K)
    tgt[0, 1, 0] = -1
    cw = torch.linspace(0.5, 1.5, C)
    cw[C - 1] = 0.0                                        # the ignored class
    return main, aux, tgt.to(DEV), cw.to(DEV)


def _plain(main, aux, tgt, cw, out_scale=1.0):
    from mspl_amd._native import check, lib
    from mspl_amd.ops import _p, _stream
    N, C, Hm, Wm = main.shape
    Ha, Wa = aux.shape[2:]
    H, W = tgt.shape[-2:]
    loss = torch.zeros(1, device=DEV)
    g = torch.empty((2, N, C, H, W), device=DEV)
    check(lib.mspl_uw_loss_heads_fwd_bwd(_p(main), _p(aux), _p(tgt), _p(cw), N, C, Hm, Wm, Ha, Wa, H, W, 20.0, out_scale, _p(loss),
                                         _p(g[0]), _p(g[1]), _stream()))
    return loss, g


def _meters(main, aux, tgt, cw, K, weight, areas, meter, out_scale=1.0):
    from mspl_amd._native import check, lib
    from mspl_amd.ops import _p, _stream
    N, C, Hm, Wm = main.shape
    Ha, Wa = aux.shape[2:]
    H, W = tgt.shape[-2:]
    loss = torch.zeros(1, device=DEV)
    g = torch.empty((2, N, C, H, W), device=DEV)
    check(lib.mspl_uw_loss_heads_meters_fwd_bwd(_p(main), _p(aux), _p(tgt), _p(cw), N, C, Hm, Wm, Ha, Wa, H, W, 20.0, out_scale, _p(loss),
                                                _p(g[0]), _p(g[1]), K, float(weight), _p(areas), _p(meter), _stream()))
    return loss, g


def _buffers(K):
    return torch.zeros(3 * K, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV)


def _expected_areas(main, tgt, K):
    """(areas (3K,), number of pixels whose top-2 margin of ops.bilinear's logits is below 1e-5)"""
    from mspl_amd import metrics, ops
    up = ops.bilinear(main, tuple(tgt.shape[-2:]))
    srt = torch.sort(up, dim=1, descending=True)[0]
    near = int(((srt[:, 0] - srt[:, 1]) < 1e-5).sum())
    return metrics.MIOU(K).areas(up, tgt).reshape(-1), near, up


def _assert_areas(got, want, near, pixels):
    """Equal when the up-sampled logits are bit-identical (the kernel's header says so); a build that contracted the two expressions
    differently could move only pixels with a near-tie, each by one count in two bins of a histogram."""
    assert near <= 1e-3 * pixels, 'the inputs have %d near-ties in %d pixels' % (near, pixels)
    K = got.numel() // 3
    d = (got.cpu() - want.cpu()).abs().reshape(3, K).sum(1)
    print('areas L1 difference per histogram', d.tolist(), 'near-ties', near)
    assert int(d.max()) <= 2 * near, (got.cpu().tolist(), want.cpu().tolist())


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_meters_form_of_the_loss_kernel(case):
    """Gradients bit-identical to the plain entry, the loss within the plain kernel's own bound (per-workgroup atomics land in any
    order), the areas those of the area kernel on the up-sampled main head, meter[0] = loss * meter_weight; a second call without
    zeroing doubles both."""
    N, C, ms, as_, size, K = case
    main, aux, tgt, cw = _inputs(case)
    l0, g0 = _plain(main, aux, tgt, cw)
    areas, meter = _buffers(K)
    l1, g1 = _meters(main, aux, tgt, cw, K, 7.0, areas, meter)
    assert torch.equal(g1, g0)
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    want, near, up = _expected_areas(main, tgt, K)
    _assert_areas(areas, want, near, N * size[0] * size[1])
    # the histograms are not trivially empty, and the label histogram is exactly the labels'
    t8 = (tgt & 255).cpu().numpy()
    assert areas[2 * K:].cpu().tolist() == [int((t8 == k).sum()) for k in range(K)]
    assert int(areas[:K].sum()) > 0 and int(areas[K:2 * K].sum()) >= int(areas[:K].sum())
    torch.testing.assert_close(meter[0].cpu(), (l0[0].double() * 7.0).cpu(), rtol=1e-5, atol=7e-6)
    assert float(meter[1]) == 0.0
    first = areas.clone()
    _meters(main, aux, tgt, cw, K, 7.0, areas, meter)
    assert torch.equal(areas, 2 * first)
    torch.testing.assert_close(meter[0].cpu(), (l0[0].double() * 14.0).cpu(), rtol=1e-5, atol=14e-6)


def test_exact_ties_take_the_lower_class():
    """Two classes carry identical low-resolution planes: their up-sampled logits tie exactly at every pixel and sit above the
    others, so torch.max's first maximum -- the lower id -- must be counted."""
    N, C, ms, as_, size, K = 2, 5, (16, 24), (8, 12), (32, 48), 4
    main, aux, tgt, cw = _inputs((N, C, ms, as_, size, K))
    main[:, 3] = main[:, 1]
    main[:, 1] += 10.0
    main[:, 3] += 10.0
    areas, meter = _buffers(K)
    _meters(main, aux, tgt, cw, K, 1.0, areas, meter)
    a = areas.cpu().reshape(3, K)
    valid = int(((tgt & 255) != 255).sum())
    assert a[1].tolist() == [0, valid, 0, 0]                     # every counted pixel predicts class 1 (bin 2), never class 3
    assert int(a[0, 1]) == int((tgt == 1).sum()) and a[0].sum() == a[0, 1]
    from mspl_amd import metrics, ops
    assert torch.equal(areas, metrics.MIOU(K).areas(ops.bilinear(main, size), tgt).reshape(-1))


def test_two_lanes_add_up_to_the_batch():
    """Two half-batch calls with out_scale = 0.5 and meter_weight = B into the same buffers = the full batch."""
    case = (4, 5, (16, 24), (8, 12), (32, 48), 4)
    main, aux, tgt, cw = _inputs(case)
    K, B = 4, 4
    full_a, full_m = _buffers(K)
    lf, _ = _meters(main, aux, tgt, cw, K, B, full_a, full_m)
    areas, meter = _buffers(K)
    parts = [_meters(main[i:i + 2].contiguous(), aux[i:i + 2].contiguous(), tgt[i:i + 2].contiguous(), cw, K, B, areas, meter, out_scale=0.5)[0]
             for i in (0, 2)]
    assert torch.equal(areas, full_a)
    torch.testing.assert_close(parts[0] + parts[1], lf, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(meter[0].cpu(), (lf[0].double() * B).cpu(), rtol=1e-5, atol=4e-6)
    torch.testing.assert_close(meter[0], full_m[0], rtol=1e-5, atol=4e-6)


def test_meters_entry_refuses_bad_arguments():
    main, aux, tgt, cw = _inputs(CASES[0])
    areas, meter = _buffers(4)
    for K in (0, 65):
        with pytest.raises(RuntimeError, match='uw_loss_heads_meters'):
            _meters(main, aux, tgt, cw, K, 1.0, areas, meter)
    with pytest.raises(RuntimeError, match='null pointer'):
        _meters(main, aux, tgt, cw, 4, 1.0, None, meter)
    assert int(areas.sum()) == 0


def test_autograd_spelling_fills_train_meters():
    """autograd.uw_loss_heads(..., meters=TrainMeters) and the three-step form of forward_loss fill the same accumulators."""
    from mspl_amd import autograd as ag, training
    case = CASES[0]
    main, aux, tgt, cw = _inputs(case)
    m = training.TrainMeters(4, DEV)
    loss = ag.uw_loss_heads(main.clone().requires_grad_(True), aux.clone().requires_grad_(True), tgt, cw, meters=m)
    loss.backward()
    m.count(2)
    want, near, up = _expected_areas(main, tgt, 4)
    m2 = training.TrainMeters(4, DEV)
    m2.add(up, tgt, loss, 2)
    m2.count(2)
    r, r2 = m.read(), m2.read()
    assert near == 0 and np.array_equal(r['areas'], r2['areas']) and r['steps'] == 1
    np.testing.assert_allclose(r['loss_avg'], float(loss), rtol=1e-5)
    np.testing.assert_allclose(r2['loss_avg'], float(loss), rtol=1e-6)
    np.testing.assert_allclose(r['union'], r['areas'][1] + r['areas'][2] - r['areas'][0] + 1e-6, rtol=0, atol=0)
    m.reset()
    assert int(m.areas.sum()) == 0 and float(m.meter.sum()) == 0.0 and m.steps == 0
