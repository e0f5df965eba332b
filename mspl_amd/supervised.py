"""The supervised source-model loop on the HIP path: what train_segmentation.py needs beyond the frozen-BN
uest step.

Reference surface mirrored (paths relative to the reference root):
  utilities/train_eval_seg.py:16-91     train_seg: the same loop for a model that returns ONE tensor (`--model espnetv2`, `espdnet`):
                                        loss = criterion(out, target).mean() [+ add_criterion(inputs, out)*weight], NO flooding
  utilities/train_eval_seg.py:164-225   train_seg_ue: model.train() (batch-statistics BatchNorm), loss =
                                        criterion(out + 0.5*aux, target).mean() [+ add_criterion(inputs, out)*weight],
                                        flooding `(loss - b).abs() + b` with b = 0.015 (:221), zero_grad/backward/step
  train_segmentation.py:241-253         torch.optim.SGD over 2-3 learning-rate groups (base net lr, segmentation head and
                                        depth encoder lr*lr_mult), momentum, weight_decay
  train_segmentation.py:353-362         per-epoch learning rates written into optimizer.param_groups[i]['lr']
  utilities/lr_scheduler.py             -> mspl_amd/lr_scheduler.py

Batch-statistics BatchNorm runs through mspl_amd.autograd.BNBatchStatsFn (statistics kernel + the existing affine/PReLU
kernels); `FlatSGD` keeps parameters, gradients and momentum buffers of all groups in three flat fp32 buffers laid out group
after group, so a step is one kernel per group and the multi-GPU exchange one all-reduce.
"""
import os

import torch

from . import autograd as ag
from . import layers
from ._native import check, lib
from .ops import _p, _stream
from .steps import FlatOptimizer, GraphedStep, run_step
from .training import TrainMeters

FLOOD_LEVEL = 0.015          # utilities/train_eval_seg.py:178


class FlatSGD(FlatOptimizer):
    """torch.optim.SGD semantics (momentum, L2 weight_decay, dampening 0, no Nesterov; parameters whose gradient is None
    are skipped) over torch-style parameter groups `[{'params': iterable, 'lr': float}, ...]`, laid out group after group in the
    flat buffers (steps.FlatOptimizer: built AFTER the first backward).  A parameter listed in two groups raises, as torch.optim
    does."""

    STATE = ('buf',)

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0):
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{'params': groups}]
        param_groups, seen, flat = [], set(), []
        for g in groups:
            ps = [p for p in g['params'] if p.requires_grad and p.grad is not None]
            for p in ps:
                if id(p) in seen:
                    raise ValueError('some parameters appear in more than one parameter group')
                seen.add(id(p))
            param_groups.append({'params': ps, 'lr': g.get('lr', lr), 'momentum': g.get('momentum', momentum),
                                 'weight_decay': g.get('weight_decay', weight_decay)})
            flat += ps
        super().__init__(flat)
        self.param_groups = param_groups
        first = 0
        for g in self.param_groups:
            g['_lo'], g['_hi'] = self.bucket.span(first, len(g['params']))
            first += len(g['params'])

    def reset(self, groups=None):
        """Start over as a fresh torch.optim.SGD would (train_segmentation.py builds one per run): zero momentum buffer and the
        first-step rule (buf = gradient) again.  groups: torch-style parameter groups in this optimizer's group order whose `lr`,
        `momentum` and `weight_decay` are taken over."""
        if groups is not None:
            groups = list(groups)
            if len(groups) != len(self.param_groups):
                raise ValueError('FlatSGD.reset: %d groups given, the optimizer has %d' % (len(groups), len(self.param_groups)))
            for g, src in zip(self.param_groups, groups):
                for k in ('lr', 'momentum', 'weight_decay'):
                    if k in src:
                        g[k] = src[k]
        super().reset()

    def same_partition(self, groups):
        """True when torch-style `groups` split this optimizer's parameters the way it was built: as many groups, and every
        parameter of group i listed in groups[i]."""
        groups = list(groups)
        if len(groups) != len(self.param_groups):
            return False
        return all(set(id(p) for p in mine['params']) <= set(id(p) for p in theirs['params'])
                   for mine, theirs in zip(self.param_groups, groups))

    def step(self):
        first = 1 if self.step_count == 0 else 0
        self.step_count += 1
        for g in self.param_groups:
            lo, hi = g['_lo'], g['_hi']
            if hi > lo:
                check(lib.mspl_sgd_step(_p(self.flat_p[lo:hi]), _p(self.flat_g[lo:hi]), _p(self.buf[lo:hi]), hi - lo, float(g['lr']),
                                        float(g['momentum']), float(g['weight_decay']), first, _stream()))
        layers.bump_param_epoch()


def segmentation_param_groups(model, lr, lr_mult, use_depth=False):
    """train_segmentation.py:244-250."""
    groups = [{'params': model.get_basenet_params(), 'lr': lr},
              {'params': model.get_segment_params(), 'lr': lr * lr_mult}]
    if use_depth:
        groups.append({'params': model.get_depth_encoder_params(), 'lr': lr * lr_mult})
    return groups


def set_epoch_learning_rates(optimizer, lr_base, lr_mult, use_depth=False):
    """train_segmentation.py:356-362 (including its depth-group rule: group 2 gets lr_base, not lr_base*lr_mult)."""
    optimizer.param_groups[0]['lr'] = lr_base
    if len(optimizer.param_groups) > 1:
        optimizer.param_groups[1]['lr'] = lr_base * lr_mult
    if use_depth:
        optimizer.param_groups[2]['lr'] = lr_base
    return lr_base, lr_base * lr_mult


def flood(loss, b=FLOOD_LEVEL):
    """utilities/train_eval_seg.py:221."""
    return (loss - b).abs() + b


_TWO_HEAD_SUM = os.environ.get('MSPL_TWO_HEAD_SUM', '1') != '0'


def two_head_outputs(model, inputs, depth=None):
    """`outputs[0] + 0.5 * outputs[1]` of the two-head model (train_eval_seg.py:185-187): through the low-resolution heads and
    autograd.TwoHeadSumFn when the model offers them (two launches instead of two up-samplings + a multiply + an add on full-size
    logits), the reference's three steps otherwise."""
    if _TWO_HEAD_SUM and hasattr(model, 'forward_lowres') and getattr(model, 'aux_layer', -1) >= 0:
        main, aux = model.forward_lowres(inputs, depth) if depth is not None else model.forward_lowres(inputs)
        if aux is not None and main.shape[1] == aux.shape[1]:
            return ag.two_head_sum(main, aux, inputs.shape[2:])
        out = (ag.bilinear(main, tuple(inputs.shape[2:])), ag.bilinear(aux, tuple(inputs.shape[2:])))
    else:
        out = model(inputs, depth) if depth is not None else model(inputs)
    return out[0] + 0.5 * out[1]


class SupervisedMeters(TrainMeters):
    """The per-epoch meters of train_seg_ue (utilities/train_eval_seg.py:166-175, 216-222, 240) on the device: training.TrainMeters
    as it stands (`areas` int64[3 K], `meter` float64[2] = [sum of flooded loss * batch size, sum of the additional loss], host step
    and image counts, `add()` for the paths the fused node does not cover, `read()` as the one sync of an epoch) plus `sums`, the
    float64[2] cross-entropy sums of the step in flight that autograd.flooded_ce_meters accumulates and clears.

    What MIOU is taken on differs from train(): here the SUMMED `main + 0.5 * aux` logits with K = num_classes - 1 (:175, :216),
    there the main head alone.  Meters are per rank: a multi-GPU run all-reduces gradients, not these sums."""

    def __init__(self, classes, device='cuda'):
        super().__init__(classes, device)
        self.sums = torch.zeros(2, dtype=torch.float64, device=device)

    def reset(self):
        super().reset()
        self.sums.zero_()


def _fused_loss(criterion, add_criterion, meters):
    """The settings autograd.flooded_ce_meters computes: the drop-in SegmentationLoss('ce') alone, with meters to fill."""
    from . import losses
    return meters is not None and add_criterion is None and type(criterion) is losses.SegmentationLoss


def _flat_sgd(model, param_groups, lr, lr_mult, use_depth, momentum, weight_decay):
    """The FlatSGD of a first step: over a caller's torch.optim.SGD groups when given (same parameters, same group order), over
    segmentation_param_groups otherwise."""
    if param_groups is None:
        groups = segmentation_param_groups(model, lr, lr_mult, use_depth)
    else:
        groups = [{'params': list(g['params']), 'lr': g['lr'], 'momentum': g.get('momentum', 0.0),
                   'weight_decay': g.get('weight_decay', 0.0)} for g in param_groups]
    return FlatSGD(groups, lr=lr * lr_mult, momentum=momentum, weight_decay=weight_decay)


def train_seg_ue_step(model, inputs, target, criterion, optimizer=None, depth=None, add_criterion=None, weight=1.0,
                      lr=0.009, lr_mult=10.0, momentum=0.9, weight_decay=4e-5, b=FLOOD_LEVEL, *, meters=None, param_groups=None):
    """One iteration of train_seg_ue (utilities/train_eval_seg.py:179-225) for a two-head model in train() mode.
    Returns (flooded loss, (main + 0.5*aux) logits detached -- what the reference hands to MIOU --, optimizer).  Pass
    optimizer=None on the first call: it is built after the first backward from segmentation_param_groups, or from
    `param_groups` (a caller's torch.optim.SGD groups: same parameters, same order) when given.  meters: a SupervisedMeters the
    iteration is added to -- inside the loss launches for SegmentationLoss('ce') without add_criterion, by meters.add() otherwise."""
    return run_step(model, optimizer, inputs.shape[0],
                    lambda: _two_head_loss(model, inputs, target, depth, criterion, add_criterion, weight, b, meters),
                    lambda: _flat_sgd(model, param_groups, lr, lr_mult, depth is not None, momentum, weight_decay), meters)


def _two_head_loss(model, inputs, target, depth, criterion, add_criterion, weight, b, meters, cw=None):
    """(flooded loss, `main + 0.5 * aux` logits) of one train_seg_ue iteration (utilities/train_eval_seg.py:185-221) with `meters`
    filled when given (the step count stays with the caller).  cw: the class-weight tensor the fused node reads (a graph passes its
    own static copy)."""
    outputs = two_head_outputs(model, inputs, depth)
    if _fused_loss(criterion, add_criterion, meters):
        if cw is None and criterion.class_wts is not None:
            cw = criterion.class_wts.to(outputs.device)
        return ag.flooded_ce_meters(outputs, target, cw, int(criterion.ignore_idx), b, meters), outputs
    loss = criterion(outputs, target).mean()
    loss2 = None
    if add_criterion is not None:
        loss2 = add_criterion(inputs, outputs) * weight
        loss = loss + loss2
    loss = flood(loss, b)
    if meters is not None:
        meters.add(outputs, target, loss, inputs.shape[0], extra=loss2)
    return loss, outputs


def _head_loss(model, criterion, add_criterion):
    """The settings autograd.ce_head_meters computes for a single-head model: the drop-in SegmentationLoss('ce') alone on a model
    that exposes its low-resolution head."""
    from . import losses
    return add_criterion is None and type(criterion) is losses.SegmentationLoss and criterion.loss_type == 'ce' and \
        hasattr(model, 'forward_lowres')


def _single_head_loss(model, inputs, target, depth, criterion, add_criterion, weight, meters, cw=None, ce_at_head=None):
    """(loss, logits) of one train_seg iteration (utilities/train_eval_seg.py:32-47; no flooding) with `meters` filled when given (the
    step count stays with the caller).  With SegmentationLoss('ce') alone the loss is taken from `forward_lowres(...)[0]` by
    autograd.ce_head_meters (ce_at_head: its `fused` argument; None = wherever the kernel fits) and `logits` is that low-resolution
    head; otherwise the reference's lines on the model's full-size output.  cw: the class-weight tensor the node reads (a graph
    passes its own static copy)."""
    from collections import OrderedDict
    if _head_loss(model, criterion, add_criterion):
        head = (model.forward_lowres(inputs, depth) if depth is not None else model.forward_lowres(inputs))[0]
        if cw is None and criterion.class_wts is not None:
            cw = criterion.class_wts.to(head.device)
        return ag.ce_head_meters(head, target, cw, int(criterion.ignore_idx), meters, fused=ce_at_head), head
    outputs = model(inputs, depth) if depth is not None else model(inputs)
    if isinstance(outputs, OrderedDict):
        outputs = outputs['out']
    loss = criterion(outputs, target).mean()
    loss2 = None
    if add_criterion is not None:
        loss2 = add_criterion(inputs, outputs) * weight
        loss = loss + loss2
    if meters is not None:
        meters.add(outputs, target, loss, inputs.shape[0], extra=loss2)
    return loss, outputs


def train_seg_step(model, inputs, target, criterion, optimizer=None, depth=None, add_criterion=None, weight=1.0,
                   lr=0.009, lr_mult=10.0, momentum=0.9, weight_decay=4e-5, *, meters=None, param_groups=None, ce_at_head=None):
    """One iteration of train_seg (utilities/train_eval_seg.py:28-69) for a model that returns one tensor (ESPNetv2Segmentation,
    ESPDNetSegmentation) in train() mode; there is no flooding.  Returns (loss, the logits the loss was taken on, detached -- the
    low-resolution head with SegmentationLoss('ce') alone, the full-size output otherwise --, optimizer).  optimizer, param_groups
    and meters as in train_seg_ue_step; ce_at_head as in _single_head_loss."""
    return run_step(model, optimizer, inputs.shape[0],
                    lambda: _single_head_loss(model, inputs, target, depth, criterion, add_criterion, weight, meters, ce_at_head=ce_at_head),
                    lambda: _flat_sgd(model, param_groups, lr, lr_mult, depth is not None, momentum, weight_decay), meters)


class GraphedSupervisedStep(GraphedStep):
    """train_seg_ue_step on steps.GraphedStep (the iteration is ~900 launches; the SGD kernels stay outside the graph, their
    learning rates change per epoch).  The eager iteration of the constructor consumes SGD's first-step rule.  BatchNorm running
    statistics and num_batches_tracked advance inside the graph.

    heads=1: the same skeleton around train_seg_step (a single-head model, no flooding: `b` is unused; the loss through
    _single_head_loss with `ce_at_head`)."""

    SNAPSHOT_BUFFERS = True          # train()-mode BatchNorm: the running statistics belong to the entry state

    def __init__(self, model, inputs, target, criterion, depth=None, lr=0.009, lr_mult=10.0, momentum=0.9, weight_decay=4e-5,
                 b=FLOOD_LEVEL, *, meters=None, consume_first_batch=True, param_groups=None, heads=2, ce_at_head=None):
        """meters: a SupervisedMeters captured inside the graph (the loss then goes through autograd.flooded_ce_meters); it is reset
        when the constructor returns.  param_groups: a caller's torch.optim.SGD groups to build FlatSGD from instead of
        segmentation_param_groups.  consume_first_batch=False: the construction batch only shapes the capture -- the constructor
        takes two SGD steps on it (the eager iteration, then the captured one), and a loop applies each batch exactly once, so
        everything that moved is put back to its value on entry: the parameters, every buffer of the model (BatchNorm
        running_mean, running_var and num_batches_tracked advance in train() mode), a zero momentum buffer and step count."""
        if heads not in (1, 2):
            raise ValueError('GraphedSupervisedStep: heads must be 1 or 2')
        self.model, self.criterion, self.b = model, criterion, b
        self.meters = meters
        self.heads, self.ce_at_head = heads, ce_at_head
        # the class weights the captured loss node reads: a copy of this object's own, refreshed by set_criterion
        self.cw = None
        if self._node_loss(criterion) and criterion.class_wts is not None:
            self.cw = criterion.class_wts.detach().to(inputs.device, torch.float32).clone()

        # (the eager iteration reads the caller's criterion, class weights included, and fills the meters)
        eager_step, kw = (train_seg_ue_step, {'b': b}) if heads == 2 else (train_seg_step, {'ce_at_head': ce_at_head})
        self._build([('inputs', inputs), ('target', target), ('depth', depth)],
                    lambda: eager_step(model, self.inputs, self.target, criterion, None, self.depth, None, 1.0, lr, lr_mult, momentum,
                                       weight_decay, meters=meters, param_groups=param_groups, **kw)[2], consume_first_batch)

    def _loss(self):
        if self.heads == 1:
            return _single_head_loss(self.model, self.inputs, self.target, self.depth, self.criterion, None, 1.0, self.meters,
                                     cw=self.cw, ce_at_head=self.ce_at_head)
        return _two_head_loss(self.model, self.inputs, self.target, self.depth, self.criterion, None, 1.0, self.b, self.meters, cw=self.cw)

    def _node_loss(self, criterion):
        """True when the captured loss is a node that reads this object's own class-weight tensor."""
        if self.heads == 1:
            return _head_loss(self.model, criterion, None)
        return _fused_loss(criterion, None, self.meters)

    def set_criterion(self, criterion):
        """Another criterion object of the same kind (a script that rebuilds it): its class weights are copied into the tensor the
        graph reads; anything the capture cannot follow raises."""
        if criterion is self.criterion:
            return
        if (self.heads == 2 and self.meters is None) or not self._node_loss(criterion) or not self._node_loss(self.criterion):
            raise RuntimeError('GraphedSupervisedStep: the step was captured with another criterion object')
        if int(criterion.ignore_idx) != int(self.criterion.ignore_idx) or (criterion.class_wts is None) != (self.cw is None):
            raise RuntimeError('GraphedSupervisedStep: the new criterion differs in ignore_idx or in having class weights')
        if self.cw is not None:
            self.cw.copy_(criterion.class_wts.to(self.cw.device, torch.float32))
        self.criterion = criterion

    def __call__(self, inputs, target, depth=None):
        if (depth is None) != (self.depth is None):
            raise RuntimeError('GraphedSupervisedStep: captured %s a depth batch, called %s one (the graph is fixed at construction)'
                               % (('without', 'with') if self.depth is None else ('with', 'without')))
        return super().__call__(inputs, target, depth)
