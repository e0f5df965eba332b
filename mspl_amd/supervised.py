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
from . import dist as mdist
from . import layers
from ._native import check, lib
from .ops import _p, _stream
from .training import TrainMeters

FLOOD_LEVEL = 0.015          # utilities/train_eval_seg.py:178


class FlatSGD:
    """torch.optim.SGD semantics (momentum, L2 weight_decay, dampening 0, no Nesterov; parameters whose gradient is None
    are skipped) over torch-style parameter groups `[{'params': iterable, 'lr': float}, ...]`.  Build it AFTER the first
    backward, like FlatAdam.  A parameter listed in two groups raises, as torch.optim does."""

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0):
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{'params': groups}]
        self.param_groups, seen, flat = [], set(), []
        for g in groups:
            ps = [p for p in g['params'] if p.requires_grad and p.grad is not None]
            for p in ps:
                if id(p) in seen:
                    raise ValueError('some parameters appear in more than one parameter group')
                seen.add(id(p))
            self.param_groups.append({'params': ps, 'lr': g.get('lr', lr), 'momentum': g.get('momentum', momentum),
                                      'weight_decay': g.get('weight_decay', weight_decay)})
            flat += ps
        if not flat:
            raise RuntimeError('FlatSGD: run one backward before constructing the optimizer (no parameter has a gradient)')
        self.bucket = mdist.GradBucket(flat, with_params=True)            # the flat layout shared with FlatAdam and the all-reduce
        self.flat_p, self.flat_g = self.bucket.flat_p, self.bucket.flat
        self.buf = torch.zeros_like(self.flat_p)
        first = 0
        for g in self.param_groups:
            g['_lo'], g['_hi'] = self.bucket.span(first, len(g['params']))
            first += len(g['params'])
        self.params = flat
        self.step_count = 0

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
        self.buf.zero_()
        self.step_count = 0

    def zero_grad(self):
        self.flat_g.zero_()

    def same_partition(self, groups):
        """True when torch-style `groups` split this optimizer's parameters the way it was built: as many groups, and every
        parameter of group i listed in groups[i]."""
        groups = list(groups)
        if len(groups) != len(self.param_groups):
            return False
        return all(set(id(p) for p in mine['params']) <= set(id(p) for p in theirs['params'])
                   for mine, theirs in zip(self.param_groups, groups))

    def reattach(self):
        """Make every parameter's .grad the view of the flat gradient buffer again (another optimizer's zero_grad() sets it to None
        and autograd then allocates a tensor of its own, which this optimizer would never read).  Raises when a parameter's storage
        no longer is its view of the flat parameter buffer (a model moved or re-created since)."""
        b = self.bucket
        for p, off in zip(b.params, b.offsets):
            if p.data_ptr() != b.flat_p.data_ptr() + 4 * off:
                raise RuntimeError('FlatSGD: a parameter no longer lives in the flat parameter buffer (the model was moved or its '
                                   'tensors replaced); build a new step')
            g = p.grad
            if g is None or g.data_ptr() != b.flat.data_ptr() + 4 * off:
                p.grad = b.flat[off:off + p.numel()].view_as(p)

    def all_reduce_grads(self):
        self.bucket.all_reduce()

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


def _sgd_groups(param_groups):
    """A caller's torch.optim.SGD groups as FlatSGD groups: same parameters, same group order."""
    return [{'params': list(g['params']), 'lr': g['lr'], 'momentum': g.get('momentum', 0.0),
             'weight_decay': g.get('weight_decay', 0.0)} for g in param_groups]


def train_seg_ue_step(model, inputs, target, criterion, optimizer=None, depth=None, add_criterion=None, weight=1.0,
                      lr=0.009, lr_mult=10.0, momentum=0.9, weight_decay=4e-5, b=FLOOD_LEVEL, *, meters=None, param_groups=None):
    """One iteration of train_seg_ue (utilities/train_eval_seg.py:179-225) for a two-head model in train() mode.
    Returns (flooded loss, (main + 0.5*aux) logits detached -- what the reference hands to MIOU --, optimizer).  Pass
    optimizer=None on the first call: it is built after the first backward from segmentation_param_groups, or from
    `param_groups` (a caller's torch.optim.SGD groups: same parameters, same order) when given.  meters: a SupervisedMeters the
    iteration is added to -- inside the loss launches for SegmentationLoss('ce') without add_criterion, by meters.add() otherwise."""
    if optimizer is not None:
        optimizer.zero_grad()
    tr = getattr(optimizer, 'transposer', None)
    with torch.enable_grad(), ag.grad_sinks(), (tr.active() if tr is not None else ag.collect_conv_weights()) as got:
        layers.prefold_frozen_bn(model)
        outputs = two_head_outputs(model, inputs, depth)
        if meters is None:
            loss = criterion(outputs, target).mean()
            if add_criterion is not None:
                loss = loss + add_criterion(inputs, outputs) * weight
            loss = flood(loss, b)
        else:
            loss = _metered_loss(criterion, outputs, target, inputs, add_criterion, weight, b, meters)
        loss.backward()
    if meters is not None:
        meters.count(inputs.shape[0])
    if optimizer is None:
        groups = _sgd_groups(param_groups) if param_groups is not None else segmentation_param_groups(model, lr, lr_mult, depth is not None)
        optimizer = FlatSGD(groups, lr=lr * lr_mult, momentum=momentum, weight_decay=weight_decay)
        optimizer.transposer = ag.WeightTransposer(got)      # (after FlatSGD: the parameters now live in its flat buffer)
    optimizer.all_reduce_grads()
    optimizer.step()
    return loss.detach(), outputs.detach(), optimizer


def _metered_loss(criterion, outputs, target, inputs, add_criterion, weight, b, meters, cw=None):
    """Loss of the iteration with `meters` filled (the step count stays with the caller).  cw: the class-weight tensor the fused node
    reads (a graph passes its own static copy)."""
    if _fused_loss(criterion, add_criterion, meters):
        if cw is None and criterion.class_wts is not None:
            cw = criterion.class_wts.to(outputs.device)
        return ag.flooded_ce_meters(outputs, target, cw, int(criterion.ignore_idx), b, meters)
    loss = criterion(outputs, target).mean()
    loss2 = None
    if add_criterion is not None:
        loss2 = add_criterion(inputs, outputs) * weight
        loss = loss + loss2
    loss = flood(loss, b)
    meters.add(outputs, target, loss, inputs.shape[0], extra=loss2)
    return loss


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
    if optimizer is not None:
        optimizer.zero_grad()
    tr = getattr(optimizer, 'transposer', None)
    with torch.enable_grad(), ag.grad_sinks(), (tr.active() if tr is not None else ag.collect_conv_weights()) as got:
        layers.prefold_frozen_bn(model)
        loss, outputs = _single_head_loss(model, inputs, target, depth, criterion, add_criterion, weight, meters, ce_at_head=ce_at_head)
        loss.backward()
    if meters is not None:
        meters.count(inputs.shape[0])
    if optimizer is None:
        groups = _sgd_groups(param_groups) if param_groups is not None else segmentation_param_groups(model, lr, lr_mult, depth is not None)
        optimizer = FlatSGD(groups, lr=lr * lr_mult, momentum=momentum, weight_decay=weight_decay)
        optimizer.transposer = ag.WeightTransposer(got)      # (after FlatSGD: the parameters now live in its flat buffer)
    optimizer.all_reduce_grads()
    optimizer.step()
    return loss.detach(), outputs.detach(), optimizer


class GraphedSupervisedStep:
    """train_seg_ue_step with zero_grad + forward + loss + backward replayed as ONE hipGraph (the iteration is ~900 launches);
    the gradient all-reduce and the SGD kernels (their learning rates change per epoch) stay outside.  The first call runs one
    eager iteration (reveals the gradient-bearing parameters, builds FlatSGD, consumes SGD's first-step rule) and captures;
    shapes are fixed at construction.  BatchNorm running statistics and num_batches_tracked advance inside the graph.

    heads=1: the same skeleton around train_seg_step (a single-head model, no flooding: `b` is unused; the loss through
    _single_head_loss with `ce_at_head`)."""

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
        entry = None
        if not consume_first_batch:
            entry = ([p.detach().clone() for p in model.parameters()], dict((n, t.detach().clone()) for n, t in model.named_buffers()))
        self.inputs = inputs.detach().clone()
        self.target = target.detach().clone()
        self.depth = None if depth is None else depth.detach().clone()
        if heads == 2:
            _, _, self.optimizer = train_seg_ue_step(model, self.inputs, self.target, criterion, None, self.depth, None, 1.0, lr, lr_mult,
                                                     momentum, weight_decay, b, meters=meters, param_groups=param_groups)
        else:
            _, _, self.optimizer = train_seg_step(model, self.inputs, self.target, criterion, None, self.depth, None, 1.0, lr, lr_mult,
                                                  momentum, weight_decay, meters=meters, param_groups=param_groups, ce_at_head=ce_at_head)
        # the class weights the captured loss node reads: a copy of this object's own, refreshed by set_criterion
        self.cw = None
        if self._node_loss(criterion) and criterion.class_wts is not None:
            self.cw = criterion.class_wts.detach().to(self.inputs.device, torch.float32).clone()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with layers.graph_capture(self.graph):
            self.optimizer.zero_grad()
            with torch.enable_grad(), ag.grad_sinks(), self.optimizer.transposer.active():
                layers.prefold_frozen_bn(model)
                if heads == 1:
                    self.loss, self.outputs = _single_head_loss(model, self.inputs, self.target, self.depth, criterion, None, 1.0, meters,
                                                                cw=self.cw, ce_at_head=ce_at_head)
                else:
                    self.outputs = two_head_outputs(model, self.inputs, self.depth)
                    if meters is None:
                        self.loss = flood(criterion(self.outputs, self.target).mean(), b)
                    else:
                        self.loss = _metered_loss(criterion, self.outputs, self.target, self.inputs, None, 1.0, b, meters, cw=self.cw)
                self.loss.backward()
        self._finish()                                  # the capture did not execute: run the iteration it recorded
        if entry is not None:
            with torch.no_grad():
                for p, p0 in zip(model.parameters(), entry[0]):       # (.data are views of the flat buffer by now: written in place)
                    p.copy_(p0)
                for n, t in model.named_buffers():
                    t.copy_(entry[1][n])
            self.optimizer.reset()
            layers.bump_param_epoch()
        if meters is not None:
            meters.reset()

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

    def _finish(self):
        self.graph.replay()
        self.optimizer.all_reduce_grads()
        self.optimizer.step()
        if self.meters is not None:
            self.meters.count(self.inputs.shape[0])
        return self.loss.detach(), self.outputs.detach()

    def __call__(self, inputs, target, depth=None):
        self.inputs.copy_(inputs)
        self.target.copy_(target)
        if self.depth is not None:
            self.depth.copy_(depth)
        return self._finish()
