"""What the training steps share (training.py: the uest step on FlatAdam; supervised.py: the source-model steps on FlatSGD):

  FlatOptimizer   parameters, gradients and optimizer state in flat fp32 buffers over one dist.GradBucket
  run_step        the eager step body: zero_grad, forward + loss + backward under the gradient sinks, all-reduce, optimizer step
  GraphedStep     the same step with zero_grad + forward + loss + backward replayed as a hipGraph
"""
import torch

from . import autograd as ag
from . import dist as mdist
from . import layers


class FlatOptimizer:
    """Base of FlatAdam and FlatSGD.  Build it AFTER the first backward: the parameters that received a gradient define the flat
    layout.  Parameter .data and .grad are re-pointed to views of `flat_p` / `flat_g` (values preserved).  A subclass names its
    per-element state buffers in STATE, fills `param_groups` (torch.optim spelling) and has the `step()`."""

    STATE = ()

    def __init__(self, params):
        try:
            self.bucket = mdist.GradBucket(params, with_params=True)      # the ONE flat layout: optimizers and all-reduce share it
        except RuntimeError:
            raise RuntimeError('%s: run one backward before constructing the optimizer (no parameter has a gradient)'
                               % type(self).__name__)
        self.params = self.bucket.params
        self.flat_p, self.flat_g = self.bucket.flat_p, self.bucket.flat
        for name in self.STATE:
            setattr(self, name, torch.zeros_like(self.flat_p))
        self.param_groups = []
        self.step_count = 0

    def zero_grad(self):
        self.flat_g.zero_()

    def all_reduce_grads(self):
        """Average gradients over the ranks: one collective on the flat bucket (RCCL over xGMI on GPUs)."""
        self.bucket.all_reduce()

    def reset(self):
        """Start over as a fresh torch.optim optimizer would: zero state buffers and step count."""
        for name in self.STATE:
            getattr(self, name).zero_()
        self.step_count = 0

    def reattach(self):
        """Make every parameter's .grad the view of the flat gradient buffer again (another optimizer's zero_grad() sets it to None
        and autograd then allocates a tensor of its own, which this optimizer would never read).  Raises when a parameter's storage
        no longer is its view of the flat parameter buffer (a model moved or re-created since)."""
        b = self.bucket
        for p, off in zip(b.params, b.offsets):
            if p.data_ptr() != b.flat_p.data_ptr() + 4 * off:
                raise RuntimeError('%s: a parameter no longer lives in the flat parameter buffer (the model was moved or its '
                                   'tensors replaced); build a new step' % type(self).__name__)
            g = p.grad
            if g is None or g.data_ptr() != b.flat.data_ptr() + 4 * off:
                p.grad = b.flat[off:off + p.numel()].view_as(p)


def run_step(model, optimizer, batch_size, loss_fn, make_optimizer, meters=None):
    """One eager optimisation step.  loss_fn() -> (loss, outputs or None) runs the forward pass; make_optimizer() builds the flat
    optimizer when `optimizer` is None: after the first backward, which reveals the gradient-bearing parameters.  meters: counts
    the step (the device sums are loss_fn's business).  Returns (loss, outputs, optimizer), tensors detached."""
    if optimizer is not None:
        optimizer.zero_grad()
    tr = getattr(optimizer, 'transposer', None)
    with torch.enable_grad(), ag.grad_sinks(), (tr.active() if tr is not None else ag.collect_conv_weights()) as got:
        layers.prefold_frozen_bn(model)
        loss, outputs = loss_fn()
        loss.backward()
    if meters is not None:
        meters.count(batch_size)
    if optimizer is None:
        optimizer = make_optimizer()
        optimizer.transposer = ag.WeightTransposer(got)      # (after the optimizer: the parameters now live in its flat buffer)
    optimizer.all_reduce_grads()
    optimizer.step()
    return loss.detach(), None if outputs is None else outputs.detach(), optimizer


class GraphedStep:
    """run_step with zero_grad + forward + loss + backward replayed as ONE hipGraph; the gradient all-reduce and the optimizer
    kernel stay outside, so the same object serves one rank and many, and hyper-parameters may change between calls.  The
    constructor runs one eager step (it reveals the gradient-bearing parameters and builds the flat optimizer), captures and runs
    the captured step; a call copies its batch into the static buffers and replays.  Shapes are fixed at construction.

    A subclass sets `model`, `meters` and whatever its loss reads, then calls `_build`.  It supplies `_loss()` -> (loss, outputs or
    None) on the static tensors -- a call returns the loss, or (loss, outputs) when there are outputs, detached -- and
    SNAPSHOT_BUFFERS: whether the model's buffers move with a step (BatchNorm in train() mode)."""

    SNAPSHOT_BUFFERS = False
    outputs = None

    def _build(self, static, eager, consume_first_batch):
        """static: [(attribute name, tensor or None)] in the argument order of a call, cloned into the buffers the graph reads.
        eager(): one eager step on them that returns the optimizer it built.  consume_first_batch=False: the construction batch
        only shapes the capture -- everything the two steps taken here moved is put back to its value on entry."""
        # (taken before the eager step re-points .data into the flat buffer)
        entry = None if consume_first_batch else dict((n, t.detach().clone()) for n, t in self._entry_state())
        for name, t in static:
            setattr(self, name, None if t is None else t.detach().clone())
        self._static = tuple(getattr(self, name) for name, _ in static)
        self.optimizer = eager()
        torch.cuda.synchronize()
        self._capture()
        self._finish()                                  # the capture did not execute: run the step it recorded
        if entry is not None:
            with torch.no_grad():
                for n, t in self._entry_state():        # (.data are views of the flat buffer by now: written in place)
                    t.copy_(entry[n])
            self.optimizer.reset()
            layers.bump_param_epoch()
        if self.meters is not None:
            self.meters.reset()

    def _entry_state(self):
        named = list(self.model.named_parameters())
        return named + list(self.model.named_buffers()) if self.SNAPSHOT_BUFFERS else named

    def _capture(self):
        self.graph = torch.cuda.CUDAGraph()
        with layers.graph_capture(self.graph):
            self.optimizer.zero_grad()
            with torch.enable_grad(), ag.grad_sinks(), self.optimizer.transposer.active():
                layers.prefold_frozen_bn(self.model)
                self.loss, self.outputs = self._loss()
                self.loss.backward()

    def _replay(self):
        self.graph.replay()

    def _finish(self):
        self._replay()
        self.optimizer.all_reduce_grads()
        self.optimizer.step()
        if self.meters is not None:
            self.meters.count(self._static[0].shape[0])
        return self.loss.detach() if self.outputs is None else (self.loss.detach(), self.outputs.detach())

    def __call__(self, *batch):
        for buf, t in zip(self._static, batch):
            if buf is not None:
                buf.copy_(t)
        return self._finish()
