"""CPU tier of the NID term at head resolution: the committed fixture tests/golden/nid_heads.npz (the reference's NIDLoss on the
up-sampled head, float64) is reproduced by the project's own float64 oracle composition F.interpolate -> oracle.labels.nid_loss on
inputs regenerated from the case; the fixture meets the conditions its generator asserted; mspl_nid_heads_plan (a host function)
answers what the cases assume; and script._fast_path admits exactly the drop-in NIDLoss with one label bin per class."""
import argparse

import numpy as np
import pytest
import torch

from tests import nid_heads_cases as nc


@pytest.fixture(scope='module')
def fixture(golden):
    return golden('nid_heads')


@pytest.mark.parametrize('name', sorted(nc.NID_HEADS_CASES))
def test_oracle_composition_reproduces_the_fixture(name, fixture):
    case = nc.NID_HEADS_CASES[name]
    B, C, K, (Hm, Wm), (H, W), _ = case
    cam, main = nc.case_inputs(case)
    cam2, main2 = nc.case_inputs(case)
    assert torch.equal(cam, cam2) and torch.equal(main, main2)                      # deterministic inputs
    assert tuple(cam.shape) == (B, 3, H, W) and tuple(main.shape) == (B, C, Hm, Wm) and main.dtype == torch.float32
    loss, grad = nc.oracle_nid_at_heads(cam, main, K, C)
    np.testing.assert_allclose(float(loss), float(fixture[name + '.loss2']), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(grad.numpy(), fixture[name + '.grad'], rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize('name', sorted(nc.NID_HEADS_CASES))
def test_fixture_meets_the_generators_conditions(name, fixture):
    B, C, K, (Hm, Wm), (H, W), _ = nc.NID_HEADS_CASES[name]
    g = fixture[name + '.grad']
    Cl = min(C, K)
    assert g.shape == (B, C, Hm, Wm) and g.dtype == np.float64
    assert fixture[name + '.hist'].shape == (K * Cl + K + Cl,)
    nz = int((g != 0).sum())
    assert nz >= max(nc.NONZERO_MIN, nc.NONZERO_SHARE * g.size), nz
    assert float(fixture[name + '.gap_grad']) <= nc.GRAD_GAP_CAP * np.abs(g).max()
    assert all(float(fixture[name + '.gap_' + k]) >= 0.0 for k in ('loss', 'hist', 'grad'))


def test_near_ties_come_in_blocks_of_one_class_pair():
    """3 x 3 head blocks share one adjacent class pair at 2 and 2 + delta, |delta| of a few 1e-3."""
    main = nc.head_logits(2, 5, 9, 12, 0)
    top2 = torch.sort(main, dim=1, descending=True)
    margin = (top2[0][:, 0] - top2[0][:, 1])
    tied = margin < 6e-3
    assert 0.2 < float(tied.float().mean()) < 0.8
    pair = torch.sort(top2[1][:, :2], dim=1)[0]                      # (B, 2, Hm, Wm) class ids of the top two
    blocks = 0
    for b in range(2):
        for y0 in range(0, 9, 3):
            for x0 in range(0, 12, 3):
                if bool(tied[b, y0:y0 + 3, x0:x0 + 3].all()):        # (a lone pixel of a noise block may tie by chance)
                    blocks += 1
                    p = pair[b, :, y0:y0 + 3, x0:x0 + 3].reshape(2, -1)
                    assert bool((p[0] == p[0, 0]).all()) and bool((p[1] == p[0, 0] + 1).all())
    assert blocks >= 6
    assert float(tied.float().sum()) <= 9 * blocks + 4


def test_plan_of_the_cases_and_the_refused_shape():
    from mspl_amd import autograd as ag
    for name, (B, C, K, (Hm, Wm), (H, W), _) in list(nc.NID_HEADS_CASES.items()) + [nc.WIDE_CASE]:
        p = ag.nid_heads_plan(B, C, Hm, Wm, H, W, K)
        assert p is not None, name
        assert (p['band_rows'], p['band_cols']) == (nc.BAND_ROWS, nc.BAND_COLS)
        assert p['bands'] == -(-H // nc.BAND_ROWS) * -(-W // nc.BAND_COLS)
        assert 1 <= p['patch_rows'] <= min(Hm, nc.BAND_ROWS + 1) and 1 <= p['patch_cols'] <= (min(Wm, nc.BAND_COLS + 1) | 1)
        assert max(p['lds_fwd'], p['lds_bwd']) <= 128 * 1024 and p['fan'] >= 1
    # the seam cases sit where they say: one band against two
    plan = lambda n: ag.nid_heads_plan(*(nc.NID_HEADS_CASES[n][:2] + nc.NID_HEADS_CASES[n][3] + nc.NID_HEADS_CASES[n][4] + (nc.NID_HEADS_CASES[n][2],)))
    assert plan('band_cols_exact')['bands'] == 2 and plan('band_cols_plus1')['bands'] == 4
    assert plan('band_rows_exact')['bands'] == 1 and plan('band_rows_plus1')['bands'] == 2
    B, C, K, (Hm, Wm), (H, W) = nc.REFUSED_SHAPE
    assert ag.nid_heads_plan(B, C, Hm, Wm, H, W, K) is None
    assert ag.nid_heads_plan(2, 33, 8, 12, 16, 24, 16) is None and ag.nid_heads_plan(2, 5, 8, 12, 16, 24, 33) is None
    assert ag.nid_heads_plan(2, 32, 64, 64, 64, 64, 32) is None               # columns and patches beyond the LDS budget
    with pytest.raises(RuntimeError):
        ag.nid_heads_plan(0, 5, 8, 12, 16, 24, 16)


def test_committed_loop_cases_meet_the_generators_conditions(golden):
    """tests/golden/train_loop_nid.*: the shapes of the records, and the conditioning its generator asserted -- the reference's own
    float32 loops within the one-step loss bound of its float64 loop in both written averages, near share at most NEAR_CAP."""
    import json
    import os
    from tests.conftest import GOLDEN
    from tests import train_loop_nid_cases as lc
    g = golden('train_loop_nid')
    meta = json.load(open(os.path.join(GOLDEN, 'train_loop_nid.json')))
    assert sorted(meta) == sorted(lc.TRAIN_LOOP_NID_CASES) == ['loop_nid_32x48', 'loop_nid_64x96_tail']
    assert lc.TRAIN_LOOP_NID_CASES['loop_nid_32x48']['batches'] == (2, 2, 2) and lc.TRAIN_LOOP_NID_CASES['loop_nid_32x48']['phases'] == (1, 1)
    assert lc.TRAIN_LOOP_NID_CASES['loop_nid_64x96_tail']['batches'] == (4, 4, 2) and lc.TRAIN_LOOP_NID_CASES['loop_nid_64x96_tail']['train_lanes'] == 2
    for name, case in lc.TRAIN_LOOP_NID_CASES.items():
        steps, epochs = len(case['batches']), sum(case['phases'])
        rec = meta[name]['records']
        assert len(rec) == 8 * epochs and meta[name]['returned'] == [lc.WRITER_IDX0 + 1 + e for e in range(epochs)]
        assert g[name + '.loss'].shape == g[name + '.loss2'].shape == g[name + '.gap_loss'].shape == (epochs, steps)
        assert g[name + '.areas'].shape == (epochs, steps, 3, 4) and len(g[name + '.params_off']) > 500
        pixels = sum(case['batches']) * case['hw'][0] * case['hw'][1]
        assert g[name + '.near'].sum(axis=1).max() <= lc.NEAR_CAP * pixels
        for e in range(epochs):
            loss_avg, nid_avg = rec[8 * e][1], rec[8 * e + 1][1]
            assert rec[8 * e][0] == 'uest/train/loss' and rec[8 * e + 1][0] == 'uest/train/nid_loss'
            assert g[name + '.gap_loss_avg'][e] <= lc.LOSS_RTOL * abs(loss_avg) + lc.LOSS_ATOL
            assert g[name + '.gap_nid_avg'][e] <= lc.LOSS_RTOL * abs(nid_avg) + lc.LOSS_ATOL
            # the written averages are those of the per-step records: losses.update(loss, B), nid_losses.update(loss2, 1)
            b = np.asarray(case['batches'], dtype=np.float64)
            np.testing.assert_allclose(loss_avg, (g[name + '.loss'][e] * b).sum() / b.sum(), rtol=1e-12)
            np.testing.assert_allclose(nid_avg, g[name + '.loss2'][e].mean(), rtol=1e-12)
            assert nid_avg != 0.0


def test_fast_path_truth_table(monkeypatch):
    """NIDLoss with one label bin per class of the model: the graphed step.  A lambda, a subclass, other bins: the restated body."""
    from mspl_amd import losses, script
    model = argparse.Namespace(training=False, classes=5)
    args = argparse.Namespace(model='espdnetue', use_depth=False, use_uncertainty=True)
    crit = losses.UncertaintyWeightedSegmentationLoss(5, class_weights=torch.ones(5), device='cpu')
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    fast = lambda add: script._fast_path(model, crit, opt, args, add)

    class Sub(losses.NIDLoss):
        pass

    assert fast(None)
    assert fast(losses.NIDLoss(image_bin=32, label_bin=5))
    assert fast(losses.NIDLoss(image_bin=16, label_bin=5, bw_camera=0.01))
    assert not fast(lambda images, pred: pred.sum())
    assert not fast(Sub(image_bin=32, label_bin=5))
    assert not fast(losses.NIDLoss(image_bin=32, label_bin=4))
    assert not fast(losses.NIDLoss(image_bin=32, label_bin=6))
    monkeypatch.setattr(script, '_FORCE_RESTATED', True)
    assert not fast(losses.NIDLoss(image_bin=32, label_bin=5))
