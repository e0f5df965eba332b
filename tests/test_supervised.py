"""Supervised-loop pieces: batch-statistics BatchNorm, SGD with learning-rate groups, flooding, epoch-wise
schedules.  CPU: oracle and host logic against vectors from the reference's own modules; GPU: the HIP path against both."""
import argparse
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import train as otrain
from tests.cases import LR_CASES, SUPERVISED_CASE
from tests.conftest import GOLDEN
from tests.optim_shadow import StepAudit
from tests.synth import synth_input, synth_labels, synth_state_dict

KEYS = json.load(open(os.path.join(GOLDEN, 'state_dict_keys.json')))
BASE = ('base_net.',)
SEG = ('bu_dec_l1.', 'bu_dec_l2.', 'bu_dec_l3.', 'bu_dec_l4.', 'merge_enc_dec_l4.', 'merge_enc_dec_l3.', 'merge_enc_dec_l2.',
       'bu_br_l4.', 'bu_br_l3.', 'bu_br_l2.')


def _is_param(k):
    return not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))


def test_lr_schedules_vs_reference_tables():
    from mspl_amd import lr_scheduler
    tables = json.load(open(os.path.join(GOLDEN, 'lr_schedules.json')))
    assert len(tables) == len(LR_CASES)
    for (name, kw, epochs), want in zip(LR_CASES, tables):
        sch = getattr(lr_scheduler, name)(**copy.deepcopy(kw))
        assert [sch.step(e) for e in range(epochs)] == want, name


def test_oracle_supervised_step_vs_reference_golden(golden):
    c, g = SUPERVISED_CASE, golden('supervised_step')
    sd = synth_state_dict(KEYS['espdnetue_s%s_c%d' % (c['s'], c['classes'])], c['sd_seed'])
    names = [str(n) for n in g['names']]
    assert sorted(names) == sorted(k for k in sd if _is_param(k))
    groups = [([n for n in names if n.startswith(BASE)], c['lr']), ([n for n in names if n.startswith(SEG)], c['lr'] * c['lr_mult'])]
    x = synth_input(c['shape'], c['in_seed'])
    labels = synth_labels((c['shape'][0],) + c['shape'][2:], c['classes'], c['in_seed'])
    loss, grads, new, after = otrain.supervised_step(sd, groups, x, labels, None, c['ignore_idx'], c['momentum'], c['weight_decay'],
                                                     c['flood'])
    torch.testing.assert_close(loss, torch.from_numpy(g['loss']), rtol=1e-5, atol=1e-6)
    in_group = set(groups[0][0]) | set(groups[1][0])
    for n, gn, moved in zip(names, g['gnorm'], g['moved']):
        if n in in_group and gn >= 0:
            assert abs(float(grads[n].double().norm()) - gn) <= 2e-3 * gn + 1e-7, n
        if n not in in_group:
            assert not moved, n                      # aux_decoder, fusion gates, depth encoder: in no group, never stepped
    for i, k in enumerate(str(s) for s in g['keep']):
        torch.testing.assert_close(new[k], torch.from_numpy(g['after_%d' % i]), rtol=1e-4, atol=1e-6)
    for i, k in enumerate(str(s) for s in g['stats']):
        if not k.endswith('num_batches_tracked'):
            torch.testing.assert_close(after[k], torch.from_numpy(g['stat_%d' % i]), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_bn_batch_stats_kernel():
    from mspl_amd import autograd as ag
    g = torch.Generator().manual_seed(5)
    for shp, mean_off in [((4, 32, 32, 32), 0.0), ((2, 7, 5, 9), 3.0), ((16, 24, 64, 120), 50.0), ((1, 3, 256, 480), -7.0)]:
        z = (torch.randn(shp, generator=g) * 1.7 + mean_off).cuda().requires_grad_()
        bn = torch.nn.BatchNorm2d(shp[1]).cuda().train()
        ref = torch.nn.BatchNorm2d(shp[1]).cuda().double().train()     # fp64 reference: with |mean| >> std the fp32 library
        with torch.no_grad():                                           # kernel itself is off by ~1e-3 (E[x^2]-E[x]^2)
            bn.weight.copy_(torch.rand(shp[1], generator=g) + 0.5)
            bn.bias.copy_(torch.randn(shp[1], generator=g))
            ref.load_state_dict(bn.state_dict())
        gy = torch.randn(shp, generator=g).cuda()
        with torch.enable_grad():
            scale, shift = ag.bn_batch_stats(z, bn)
            y = ag.affine_prelu(z, scale, shift)
            y.backward(gy)
        z2 = z.detach().double().requires_grad_()
        y2 = ref(z2)
        y2.backward(gy.double())
        f = lambda t: t.float()
        torch.testing.assert_close(y, f(y2), rtol=2e-5, atol=1e-5 * (1 + abs(mean_off)))
        torch.testing.assert_close(z.grad, f(z2.grad), rtol=1e-4, atol=2e-5)
        # d gamma = (sum g*z - mean * sum g) * invstd is formed from fp32 channel sums: its error grows with |mean|/std
        torch.testing.assert_close(bn.weight.grad, f(ref.weight.grad), rtol=1e-4, atol=2e-3 + 2e-4 * abs(mean_off))
        torch.testing.assert_close(bn.bias.grad, f(ref.bias.grad), rtol=1e-4, atol=2e-3)
        torch.testing.assert_close(bn.running_mean, f(ref.running_mean), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(bn.running_var, f(ref.running_var), rtol=1e-5, atol=1e-6)
        assert int(bn.num_batches_tracked) == 1


BN_NODE_TWO_LAUNCH = {(16, 16, 72, 120), (4, 8, 144, 240), (8, 6, 75, 77)}      # the shapes that are there for the two-launch form


@pytest.mark.gpu
@pytest.mark.parametrize('shp,mean_off,with_res', [
    ((16, 24, 18, 30), 0.5, True), ((2, 7, 5, 9), 3.0, False), ((16, 8, 36, 60), -2.0, True),
    ((4, 32, 64, 120), 1.0, True), ((3, 5, 9, 15), 0.0, True), ((16, 16, 72, 120), 0.3, False),
    # the two-launch form WITH a residual (the gc + pointwise(p * z + q + gc) backward), and with planes that are not whole quads
    ((16, 16, 72, 120), 0.3, True), ((4, 8, 144, 240), -1.0, True), ((8, 6, 75, 77), 0.7, True), ((8, 6, 75, 77), 0.7, False)])
def test_bn_train_prelu_node(shp, mean_off, with_res):
    """autograd.bn_train_prelu (PReLU(BatchNorm_train(z) + residual), the supervised loop's node) against torch in fp64: the one-launch
    small-plane form (N * HW <= 40 960) and the two-launch form above it, with and without residual; the form a shape is there for is
    checked against the library's own rule."""
    from mspl_amd import autograd as ag
    from mspl_amd._native import lib
    assert ag._SMALL_BN and bool(lib.mspl_bn_train_small_fits(shp[0], shp[1], shp[2] * shp[3])) == (shp not in BN_NODE_TWO_LAUNCH)
    g = torch.Generator().manual_seed(6)
    C = shp[1]
    z = (torch.randn(shp, generator=g) * 1.3 + mean_off).cuda().requires_grad_()
    res = torch.randn(shp, generator=g).cuda().requires_grad_() if with_res else None
    al = (torch.rand(C, generator=g) * 0.3).cuda().requires_grad_()
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    ref = torch.nn.BatchNorm2d(C).cuda().double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g))
        ref.load_state_dict(bn.state_dict())
    gy = torch.randn(shp, generator=g).cuda()
    with torch.enable_grad():
        y = ag.bn_train_prelu(z, bn, al, res)
        y.backward(gy)
    z2 = z.detach().double().requires_grad_()
    r2 = res.detach().double().requires_grad_() if with_res else None
    a2 = al.detach().double().requires_grad_()
    u = ref(z2) + (r2 if with_res else 0.0)
    y2 = F.prelu(u, a2)
    y2.backward(gy.double())
    f = lambda t: t.float()
    torch.testing.assert_close(y, f(y2), rtol=2e-5, atol=2e-5 * (1 + abs(mean_off)))
    torch.testing.assert_close(z.grad, f(z2.grad), rtol=2e-4, atol=5e-5)
    if with_res:
        torch.testing.assert_close(res.grad, f(r2.grad), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(al.grad, f(a2.grad), rtol=1e-4, atol=2e-3)
    torch.testing.assert_close(bn.weight.grad, f(ref.weight.grad), rtol=1e-4, atol=2e-3 + 2e-4 * abs(mean_off))
    torch.testing.assert_close(bn.bias.grad, f(ref.bias.grad), rtol=1e-4, atol=2e-3)
    torch.testing.assert_close(bn.running_mean, f(ref.running_mean), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(bn.running_var, f(ref.running_var), rtol=1e-5, atol=1e-6)
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.gpu
def test_flat_sgd_matches_torch_sgd():
    from mspl_amd.supervised import FlatSGD
    g = torch.Generator().manual_seed(9)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in [(8, 3, 3, 3), (8,), (5, 7), (1,)]]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ref = torch.optim.SGD([{'params': qs[:2], 'lr': 0.01}, {'params': qs[2:], 'lr': 0.1}], lr=0.1, momentum=0.9, weight_decay=4e-5)
    opt = None
    for it in range(3):
        grads = [torch.randn(p.shape, generator=g).cuda() for p in ps]
        for p, q, gr in zip(ps, qs, grads):
            if opt is None:
                p.grad = gr.clone()
            else:
                p.grad.copy_(gr)
            q.grad = gr.clone()
        if opt is None:
            opt = FlatSGD([{'params': ps[:2], 'lr': 0.01}, {'params': ps[2:], 'lr': 0.1}], lr=0.1, momentum=0.9, weight_decay=4e-5)
        if it == 2:                                   # an epoch boundary: train_segmentation.py:356-359
            opt.param_groups[0]['lr'] = ref.param_groups[0]['lr'] = 0.005
        opt.step()
        ref.step()
        for p, q in zip(ps, qs):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        FlatSGD([{'params': ps[:2]}, {'params': ps[1:]}], lr=0.1)


@pytest.mark.gpu
def test_supervised_step_vs_reference_golden(golden):
    """One train_seg_ue iteration (batch-statistics BatchNorm, CrossEntropy, flooding, SGD groups) on the HIP path against the
    reference's golden step and the oracle."""
    from mspl_amd import losses, models, supervised
    c, g = SUPERVISED_CASE, golden('supervised_step')
    a = argparse.Namespace(s=c['s'], channels=3, num_classes=1000)
    m = models.ESPDNetwithUncertaintyEstimation(a, classes=c['classes'], dataset=c['dataset'], fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(KEYS['espdnetue_s%s_c%d' % (c['s'], c['classes'])], c['sd_seed']))
    m = m.cuda().train()
    x = synth_input(c['shape'], c['in_seed']).cuda()
    labels = synth_labels((c['shape'][0],) + c['shape'][2:], c['classes'], c['in_seed']).cuda()
    crit = losses.SegmentationLoss(n_classes=c['classes'], device='cuda', ignore_idx=c['ignore_idx'])
    # step by hand first (gradients), then through the helper on a fresh copy
    with torch.enable_grad():
        out = m(x)
        logits = out[0] + 0.5 * out[1]
        loss = supervised.flood(crit(logits, labels).mean(), c['flood'])
        loss.backward()
    torch.testing.assert_close(loss.detach().cpu(), torch.from_numpy(g['loss']), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(logits.detach().cpu()[:, :, ::4, ::4], torch.from_numpy(g['logits']), rtol=1e-3, atol=1e-3)
    params = dict(m.named_parameters())
    names = [str(n) for n in g['names']]
    for n, gn in zip(names, g['gnorm']):
        if gn < 0:
            assert params[n].grad is None, n
        else:
            got = float(params[n].grad.double().norm())
            assert abs(got - gn) <= 1e-2 * gn + 1e-5, (n, got, gn)
    with StepAudit(m) as audit:
        opt = supervised.FlatSGD(supervised.segmentation_param_groups(m, c['lr'], c['lr_mult']), lr=c['lr'] * c['lr_mult'],
                                 momentum=c['momentum'], weight_decay=c['weight_decay'])
        before = {n: p.detach().clone() for n, p in params.items()}
        opt.step()
        torch.cuda.synchronize()
        for n, moved in zip(names, g['moved']):
            assert bool((params[n].detach() != before[n]).any()) == bool(moved), n
        for i, k in enumerate(str(s) for s in g['keep']):
            torch.testing.assert_close(params[k].detach().cpu(), torch.from_numpy(g['after_%d' % i]), rtol=1e-3, atol=2e-5)
        sd = m.state_dict()
        for i, k in enumerate(str(s) for s in g['stats']):
            torch.testing.assert_close(sd[k].cpu(), torch.from_numpy(g['stat_%d' % i]), rtol=1e-4, atol=1e-5)
        # the helper: a second iteration runs, the loss moves, every BatchNorm has seen two batches
        loss2, out2, opt = supervised.train_seg_ue_step(m, x, labels, crit, opt)
    # both SGD iterations, every element of every tensor and momentum buffer, per group (train() mode: the statistics move)
    audit.check(m, frozen_buffers=False, label='supervised golden step')
    assert audit.steps == [(1, [c['lr'], c['lr'] * c['lr_mult']]), (2, [c['lr'], c['lr'] * c['lr_mult']])]
    assert torch.isfinite(loss2) and out2.shape == logits.shape and float(loss2) != float(loss.detach())
    assert int(sd['base_net.level1.bn.num_batches_tracked']) == 2
    # inference afterwards uses the UPDATED running statistics (caches keyed on the buffers' versions)
    m.eval()
    with torch.no_grad():
        y = m(x)[0]
    assert torch.isfinite(y).all()


@pytest.mark.gpu
def test_graphed_supervised_step_equals_eager():
    """The supervised iteration replayed as one hipGraph (running statistics advancing inside the graph) against eager steps."""
    from mspl_amd import losses, models, supervised
    c = SUPERVISED_CASE
    a = argparse.Namespace(s=c['s'], channels=3, num_classes=1000)
    x = synth_input((2, 3, 64, 96), 28).cuda()
    y = synth_labels((2, 64, 96), c['classes'], 28).cuda()
    crit = losses.SegmentationLoss(n_classes=c['classes'], device='cuda', ignore_idx=c['ignore_idx'])
    nets = []
    for _ in range(2):
        m = models.ESPDNetwithUncertaintyEstimation(a, classes=c['classes'], dataset=c['dataset'], fix_pyr_plane_proj=True)
        m.load_state_dict(synth_state_dict(KEYS['espdnetue_s%s_c%d' % (c['s'], c['classes'])], 5))
        nets.append(m.cuda().train())
    opt, eager = None, []
    with StepAudit(*nets) as audit:
        for _ in range(4):
            l, _, opt = supervised.train_seg_ue_step(nets[0], x, y, crit, opt)
            eager.append(float(l))
        gs = supervised.GraphedSupervisedStep(nets[1], x, y, crit)                   # eager step 1 + captured step 2
        graphed = [float(gs(x, y)[0]) for _ in range(2)]
    np.testing.assert_allclose(graphed, eager[2:], rtol=5e-4, atol=1e-6)
    for k, net in enumerate(nets):      # each run's own four SGD iterations per tensor, at that iteration's own gradient
        audit.check(net, frozen_buffers=False, label='graphed supervised net %d' % k)
        assert [r.step for r in audit.records_of(net)] == [1, 2, 3, 4]
    for (k, p), (_, q) in zip(nets[0].state_dict().items(), nets[1].state_dict().items()):
        # two runs of the same kernels: the float atomics of the weight-gradient / channel sums land in a different order, and the
        # coarsest BatchNorms normalise over a handful of values per channel (16 and 4 at 64 x 96), which amplifies that over the four
        # steps (seen at 32 x 48, 4 and 2 values: 1.1e-3 relative on a running_var).  The outcome is bimodal: a 1e-7 difference can flip
        # a discrete event (a PReLU sign near zero) in step 3, after which the two runs sit 2e-5 apart in the loss and up to 4e-4 in
        # single weights (tools/sup_graph_vs_eager.py, tools/sup_determinism4.py: eager vs eager shows the same two outcomes)
        np.testing.assert_allclose(q.float().cpu().numpy(), p.float().cpu().numpy(), rtol=2e-3, atol=1e-3, err_msg=k)
    assert int(nets[1].state_dict()['base_net.level1.bn.num_batches_tracked']) == 4


# ------------------------------------------------------------------ NIDLoss
from tests.cases import NID_CASES  # noqa: E402
from tests.synth import synth_nid_inputs  # noqa: E402


@pytest.mark.parametrize('name', sorted(NID_CASES))
def test_oracle_nid_vs_reference_golden(name, golden):
    from oracle import labels as olab
    shape, classes, K, seed = NID_CASES[name]
    cam, lab = synth_nid_inputs(shape, classes, seed)
    lab.requires_grad_()
    loss = olab.nid_loss(cam, lab, image_bin=K, label_bin=classes)
    loss.backward()
    g = golden('nid')
    torch.testing.assert_close(loss.detach(), torch.from_numpy(g[name + '.loss']), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lab.grad, torch.from_numpy(g[name + '.grad']), rtol=1e-3, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(NID_CASES))
def test_nid_loss_vs_reference_golden(name, golden):
    """NIDLoss forward value and gradient w.r.t. the label logits (soft histogram kernels) against the reference's own numbers.
    The gradient lives only where the soft-arg-max falls between two label bins and is amplified by beta/bw_label = 5e5 there:
    compared with a relative tolerance."""
    from mspl_amd import losses
    shape, classes, K, seed = NID_CASES[name]
    cam, lab = synth_nid_inputs(shape, classes, seed)
    lab_d = lab.cuda().requires_grad_()
    crit = losses.NIDLoss(image_bin=K, label_bin=classes)
    loss = crit(cam.cuda(), lab_d)
    loss.backward()
    g = golden('nid')
    torch.testing.assert_close(loss.detach().cpu(), torch.from_numpy(g[name + '.loss']), rtol=1e-4, atol=2e-4)
    ref = torch.from_numpy(g[name + '.grad'])
    got = lab_d.grad.cpu()
    assert int((ref != 0).sum()) > 10
    torch.testing.assert_close(got, ref, rtol=2e-2, atol=2e-4 * float(ref.abs().max()))
    with pytest.raises(RuntimeError, match='classes'):
        losses.NIDLoss(image_bin=K, label_bin=classes + 1)(cam.cuda(), lab_d)
