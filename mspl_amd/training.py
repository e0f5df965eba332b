"""One uest self-training step on the HIP path (uest_seg_multi_os.py:958-1089, train()).

    (pred, aux) = model(images)                               # frozen BatchNorm (model.eval(), Appendix B-3)
    kld  = PixelwiseKLD()(pred, aux)                          # NOT detached
    loss = criterion(pred + 0.5*aux, labels, kld) * 20 + kld.mean()
    loss.backward(); optimizer.step()                         # Adam over model.parameters(), weight decay as L2

`uest_loss` is K11 (one fused forward+backward kernel); `FlatAdam` keeps every gradient-bearing parameter, its
gradient and the two Adam moments in four flat fp32 buffers, so the optimizer is ONE kernel and the multi-GPU
gradient exchange ONE all-reduce (mspl_amd.dist).  Parameters whose gradient stays None (depth encoder, fusion gates,
module_act of strided EESPs: 230 of 570 tensors) are left out, exactly like torch.optim.Adam skips them.
"""
import os

import torch

from . import autograd as ag
from . import layers
from ._native import check, lib
from .ops import _p, _stream
from .steps import FlatOptimizer, GraphedStep, run_step
from .streams import _concurrent_streams


def _device_class_weights(class_weights, device, ignore_idx):
    cw = class_weights.detach().to(device, torch.float32).clone()
    if ignore_idx is not None:
        cw[ignore_idx] = 0.0
    return cw


def uest_loss(pred, aux, labels, class_weights, ignore_idx=None, ce_scale=20.0):
    """criterion(pred + 0.5*aux, labels, kld)*ce_scale + kld.mean() with kld = PixelwiseKLD(pred, aux).
    class_weights: tensor of num_classes weights; class_weights[ignore_idx] is treated as 0 (the reference zeroes it
    in place at construction, loss_fns/segmentation_loss.py:152-153)."""
    return ag.uw_loss(pred, aux, labels, _device_class_weights(class_weights, pred.device, ignore_idx), ce_scale)


_LOSS_AT_HEADS = os.environ.get('MSPL_LOSS_HEADS', '1') != '0'      # A/B aid: 0 = up-sample both heads, then the loss


class TrainMeters:
    """The per-epoch meters of the reference's train() (uest_seg_multi_os.py:964-969, 1032-1037, 1050) kept on the device:
    `areas` int64[3 K] = [inter | pred | mask] summed over the steps (MIOU(num_classes=K).get_iou on the main head), `meter`
    float64[2] = [sum of loss * batch size, sum of the additional loss].  The loss kernel adds into both (forward_loss(...,
    meters=...)); the step and image counts are host integers.  `read()` is the one device-to-host copy and sync of an epoch.

    The sums are integers, where the reference sums float32 arrays (AverageMeter over numpy float32 histograms, which stop counting
    exactly past 2^24 pixels per class): a deliberate difference, invisible below that count."""

    def __init__(self, classes=4, device='cuda'):
        self.classes = int(classes)
        self.areas = torch.zeros(3 * self.classes, dtype=torch.int64, device=device)
        self.meter = torch.zeros(2, dtype=torch.float64, device=device)
        self.steps = 0
        self.images = 0

    def reset(self):
        self.areas.zero_()
        self.meter.zero_()
        self.steps = 0
        self.images = 0

    def count(self, batch_size):
        """One step of `batch_size` images went in (host side; the device sums are added by the kernels)."""
        self.steps += 1
        self.images += int(batch_size)

    def add(self, pred, labels, loss, batch_size, extra=None):
        """The same sums from a full-size main head and a loss tensor (the forms the heads kernel does not cover): the integer area
        kernel and device-side adds, no sync."""
        from .metrics import MIOU
        self.areas += MIOU(self.classes).areas(pred.detach(), labels).reshape(-1)
        self.meter[0] += loss.detach().double() * float(batch_size)
        if extra is not None:
            self.meter[1] += extra.detach().double()

    def read(self):
        """{'loss_avg', 'extra_sum', 'inter' [K], 'union' [K], 'steps'}: union = pred + mask - inter + steps * 1e-6 (the reference adds
        its epsilon once per step, segmentation_miou.py:41)."""
        import numpy as np
        a = self.areas.cpu().numpy().reshape(3, self.classes).astype(np.float64)       # (synchronises)
        m = self.meter.cpu().numpy()
        return {'loss_avg': float(m[0]) / max(1, self.images), 'extra_sum': float(m[1]), 'inter': a[0],
                'union': a[1] + a[2] - a[0] + self.steps * 1e-6, 'areas': a, 'steps': self.steps}


def _additional_loss(add_loss, images, main, pred, meters):
    """loss2 = add_loss(images, pred) (uest_seg_multi_os.py:1027-1030) and its two meter adds on the device: meter[1] += loss2
    (nid_losses.update(loss2.item(), 1)) and meter[0] += B * loss2 (losses.update(loss.item(), B) at :1037 sees the loss after `loss
    += loss2`).  A losses.NIDLoss takes the low-resolution main head `main` where its heads kernels cover the shape; otherwise (and
    for any other callable) the full-size `pred`, up-sampled here when only `main` is given."""
    from . import losses
    if main is not None and type(add_loss) is losses.NIDLoss and add_loss.heads_supported(images, main):
        loss2 = add_loss.at_heads(images, main)
    else:
        loss2 = add_loss(images, pred if pred is not None else ag.bilinear(main, tuple(images.shape[2:])))
    if meters is not None:
        l2 = loss2.detach().double()
        meters.meter[0] += l2 * float(images.shape[0])
        meters.meter[1] += l2
    return loss2


def forward_loss(model, images, labels, cw, ce_scale=20.0, out_scale=1.0, root=False, meters=None, add_loss=None, depth=None):
    """model forward + uest loss (uest_seg_multi_os.py:1010-1023) on device class weights `cw`.  A model that exposes its decoder
    outputs (`forward_lowres`: main at H/2, auxiliary at H/4) gets the loss taken at head resolution -- the up-sampling of
    espdnet_ue.py:301-302 happens inside the loss kernel (ag.uw_loss_heads), same value and gradients; any other model is called as
    the reference calls it and the loss takes its two full-size outputs.  meters: a TrainMeters that receives this batch's area
    histograms and loss * batch size (a lane passes out_scale = 1 / lanes and adds its share).

    add_loss: the additional loss of train(..., add_loss=...) (:1027-1030), added to the returned loss; a losses.NIDLoss is taken from
    the low-resolution main head too (NIDLoss.at_heads) where the plan of its kernels covers the shape.  It sees all images of a
    batch at one pixel position together, so it goes with out_scale = 1 only (no micro-batch lanes).

    depth: the (N,1,H,W) depth batch of an RGB-D model (model(x, x_d), espdnet_ue.py:186-270), or None."""
    if add_loss is not None and out_scale != 1.0:
        raise RuntimeError('mspl_amd.training.forward_loss: an additional loss couples the images of a batch; it cannot be split '
                           'into micro-batch lanes (out_scale = %g)' % out_scale)
    lowres = getattr(model, 'forward_lowres', None) if _LOSS_AT_HEADS else None
    main = None
    if lowres is not None:
        main, aux = lowres(images, depth) if depth is not None else lowres(images)
        if aux is None:
            raise RuntimeError('mspl_amd.training.forward_loss: %s returns one head; the uest loss needs the auxiliary head of a '
                               'two-head model' % type(model).__name__)
        if ag.uw_loss_heads_supported(main.shape[1]):
            loss = ag.uw_loss_heads(main, aux, labels, cw, ce_scale, out_scale, root, meters)
            if add_loss is not None:
                loss = loss + _additional_loss(add_loss, images, main, None, meters)
            return loss
        size = tuple(images.shape[2:])
        pred, aux = ag.bilinear(main, size), ag.bilinear(aux, size)
    else:
        pred, aux = model(images, depth) if depth is not None else model(images)
    loss = ag.uw_loss(pred, aux, labels, cw, ce_scale, out_scale, root)
    if meters is not None:      # the three-step form: the existing area kernel on the full-size main head, loss * B added on the device
        meters.add(pred, labels, loss, images.shape[0] / out_scale)
    if add_loss is not None:
        loss = loss + _additional_loss(add_loss, images, main, pred, meters)
    return loss


class FlatAdam(FlatOptimizer):
    """torch.optim.Adam semantics (lr, betas, eps, L2 weight_decay, bias correction) on flat buffers (steps.FlatOptimizer: built
    AFTER the first backward)."""

    STATE = ('m', 'v')

    def __init__(self, params, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        # torch.optim spelling: the reference's adjust_learning_rate writes optimizer.param_groups[0]['lr'] (:1325-1328)
        self.param_groups = [{'lr': lr, 'params': self.params}]

    @property
    def lr(self):
        return self.param_groups[0]['lr']

    @lr.setter
    def lr(self, value):
        self.param_groups[0]['lr'] = value

    def reset(self, lr=None, betas=None, eps=None, weight_decay=None):
        """Start over as a fresh torch.optim.Adam would: zero moments and step count; hyper-parameters given are taken over."""
        super().reset()
        given = {'lr': lr, 'betas': None if betas is None else tuple(betas), 'eps': eps, 'weight_decay': weight_decay}
        for name, value in given.items():
            if value is not None:
                setattr(self, name, value)

    def step(self):
        self.step_count += 1
        check(lib.mspl_adam_step(_p(self.flat_p), _p(self.flat_g), _p(self.m), _p(self.v), self.flat_p.numel(),
                                 float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                                 float(self.weight_decay), self.step_count, _stream()))
        layers.bump_param_epoch()       # the kernel wrote through raw pointers: invalidate folded-BN / packed-weight caches


def lr_poly(base_lr, iter_n, max_iter, power):
    """uest_seg_multi_os.py:1317-1321."""
    return base_lr * ((1 - float(iter_n) / max_iter) ** power)


def adjust_learning_rate(optimizer, i_iter, tot_iter, base_lr, power=0.0):
    """uest_seg_multi_os.py:1325-1328 (base_lr / power are script globals there: args.learning_rate, args.power)."""
    lr = lr_poly(base_lr, i_iter, tot_iter, power)
    optimizer.param_groups[0]['lr'] = lr
    return lr


def train_step(model, images, labels, class_weights, optimizer=None, ignore_idx=None, lr=5e-4, weight_decay=5e-4,
               ce_scale=20.0, meters=None, add_loss=None, depth=None):
    """One optimisation step; returns (loss tensor, optimizer).  Pass optimizer=None on the first call: it is built
    after the first backward (which reveals the gradient-bearing parameters).  meters: a TrainMeters the step is added to.
    add_loss: the additional loss of train(..., add_loss=...), see forward_loss.  depth: the depth batch of an RGB-D model."""
    def loss_fn():
        return forward_loss(model, images, labels, _device_class_weights(class_weights, images.device, ignore_idx), ce_scale,
                            meters=meters, add_loss=add_loss, depth=depth), None

    loss, _, optimizer = run_step(model, optimizer, images.shape[0], loss_fn,
                                  lambda: FlatAdam(model.parameters(), lr=lr, weight_decay=weight_decay), meters)
    return loss, optimizer


SETTLE_THRESHOLD = 0.55      # four lanes overlapping take 0.44-0.45 of the same graphs back to back; two lanes sharing a queue ~0.7


def settle_seating(serial_ms, first_ms, measure, new_candidate, attempts=3, threshold=SETTLE_THRESHOLD):
    """Decision logic of `GraphedTrainStep._settle_streams`, free of GPU calls.  `first_ms` is the time of all lanes on seating 0,
    `serial_ms` of the same graphs back to back on one stream; `new_candidate()` makes another seating and returns its index,
    `measure(index)` times it.  Returns {'seating', 'lanes_ms', 'settled', 'attempts'}: the first seating under `threshold` x serial,
    else -- after `attempts` candidates -- the fastest one seen with settled = False (the caller warns and reports it)."""
    best_ms, best = first_ms, 0
    used = 0
    while best_ms > threshold * serial_ms and used < attempts:
        k = new_candidate()
        used += 1
        ms = measure(k)
        if ms < best_ms:
            best_ms, best = ms, k
    return {'seating': best, 'lanes_ms': best_ms, 'settled': bool(best_ms <= threshold * serial_ms), 'attempts': used}


class GraphedTrainStep(GraphedStep):
    """train_step on steps.GraphedStep (the step is ~1400 launches of 5-100 us; eager issue from Python is slower than the GPU
    executes them).

    lanes = 1: ONE graph.  lanes = L > 1: the batch is cut into L micro-batches that run as L graphs on L streams AT THE SAME TIME
    (the kernels of a batch-16 step are too small to fill the chip; graphs on separate streams overlap, branches inside one
    graph did not).  Same step: BatchNorm is frozen, the loss is a plain mean over the pixels of the batch (K11: 1 / (N*H*W)), so
    each lane back-propagates loss_lane / L and every parameter-gradient kernel adds into the shared flat gradient buffer with
    atomics (autograd.grad_sinks); only the floating-point summation order differs.  A parameter whose gradient would go through
    autograd's (non-atomic) AccumulateGrad in a lane is refused at construction.

    add_loss: the additional loss of train(..., add_loss=...) (forward_loss), captured inside the graph.  With one the step runs
    lanes = 1 whatever is asked: NIDLoss's joint histogram sums the images of a batch per pixel position BEFORE its outer product, so
    it has cross terms between the images of a batch, and micro-batch lanes would compute another loss."""

    def __init__(self, model, images, labels, class_weights, ignore_idx=None, lr=5e-4, weight_decay=5e-4, ce_scale=20.0, lanes=1,
                 meters=None, consume_first_batch=True, add_loss=None, depth=None):
        """depth: the (N,1,H,W) depth batch of an RGB-D model: a static buffer after `labels`, sliced per lane like the images.  A
        step captured with depth must be called with depth and one captured without must not (the graph is one or the other).
        meters: a TrainMeters captured inside the graph(s) -- every lane adds into the same buffers; it is reset when the
        constructor returns.  consume_first_batch=False: the construction batch only shapes the capture -- the parameters are put
        back to their values on entry, both Adam moments, the step count and the meters are zeroed, so the first call is step 1 (a
        training loop applies each batch exactly once; the default applies the construction batch twice: an eager step, then the
        captured one)."""
        self.model, self.meters, self.add_loss = model, meters, add_loss
        self.cw = _device_class_weights(class_weights, images.device, ignore_idx)
        self.ce_scale = ce_scale
        self.lanes = lanes if (lanes > 1 and images.shape[0] % lanes == 0 and add_loss is None) else 1
        # (the eager step gets the caller's class weights and no meters; the capture reads this object's own `cw`)
        self._build([('images', images), ('labels', labels.to(torch.int64)), ('depth', depth)],
                    lambda: train_step(model, self.images, self.labels, class_weights, None, ignore_idx, lr, weight_decay, ce_scale,
                                       add_loss=add_loss, depth=self.depth)[1],
                    consume_first_batch)

    def _lane_loss(self, images, labels, out_scale=1.0, depth=None):
        return forward_loss(self.model, images, labels, self.cw, self.ce_scale, out_scale=out_scale, root=True, meters=self.meters,
                            add_loss=self.add_loss, depth=depth)

    def _loss(self):
        return self._lane_loss(self.images, self.labels, depth=self.depth), None

    def __call__(self, images, labels, depth=None):
        if (depth is None) != (self.depth is None):
            raise RuntimeError('GraphedTrainStep: captured %s a depth batch, called %s one (the graph is fixed at construction)'
                               % (('without', 'with') if self.depth is None else ('with', 'without')))
        return super().__call__(images, labels, depth)

    def _capture(self):
        if self.lanes == 1:
            return super()._capture()
        tr = self.optimizer.transposer
        # what every lane needs first: zeroed gradients, this step's transposed weights and folded BatchNorms (their tensors live
        # in this graph's pool, the lanes' graphs read them)
        self.graph = torch.cuda.CUDAGraph()
        with layers.graph_capture(self.graph):
            self.optimizer.zero_grad()
            tr.run()
            with torch.no_grad():
                layers.prefold_frozen_bn(self.model)
        b = self.images.shape[0] // self.lanes
        # streams that really run side by side (HIP multiplexes streams onto a few hardware queues; two lanes on one queue run one
        # after the other, and four serialised micro-batches are SLOWER than the one-graph step: 12.2 vs 9.0 ms, both seen in one
        # process with plain new streams, depending on how many streams existed before)
        self.streams = _concurrent_streams(self.lanes, self.images.device)
        self.lane_graphs, self.lane_losses = [], []
        stray = []
        # (a tensor hook sees None when the op accumulated into the sink itself, a tensor when autograd is about to add one)
        hooks = [p.register_hook(lambda g_: stray.append(1) if g_ is not None else None) for p in self.optimizer.params]
        try:
            for i, st in enumerate(self.streams):
                st.wait_stream(torch.cuda.current_stream())
                g = torch.cuda.CUDAGraph()
                with layers.graph_capture(g, stream=st):
                    with torch.enable_grad(), ag.grad_sinks(), tr.active(refresh=False):
                        loss = self._lane_loss(self.images[i * b:(i + 1) * b], self.labels[i * b:(i + 1) * b], 1.0 / self.lanes,
                                               None if self.depth is None else self.depth[i * b:(i + 1) * b])
                        loss.backward()
                self.lane_graphs.append(g)
                self.lane_losses.append(loss)
        finally:
            for h in hooks:
                h.remove()
        if stray:
            raise RuntimeError('GraphedTrainStep(lanes=%d): %d parameter gradients went through AccumulateGrad instead of an '
                               'atomic gradient sink; concurrent lanes would race on them' % (self.lanes, len(stray)))
        # the capture did not execute: the lanes read this step's transposed weights and BatchNorm folds from self.graph's pool,
        # so it runs once before the lanes are timed (they would otherwise run on uninitialised memory)
        self.graph.replay()
        self._settle_streams()

    def set_class_weights(self, class_weights, ignore_idx=None):
        """New class weights (a relabelling round, uest_seg_multi_os.py:527-530): copied into the tensor the graphs read."""
        self.cw.copy_(_device_class_weights(class_weights, self.cw.device, ignore_idx))

    def reset_optimizer(self, lr=None, betas=None, eps=None, weight_decay=None):
        """FlatAdam.reset (the script builds a new optimizer per round, :594-598)."""
        self.optimizer.reset(lr, betas, eps, weight_decay)

    def _lanes_ms(self, streams, reps=2):
        """Wall time of one replay of every lane graph, lane i on streams[i % len(streams)] (the gradients they add up are thrown away by
        the next step's zero fill)."""
        import time
        dev = self.images.device
        best = float('inf')
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            cur = torch.cuda.current_stream()
            ev = cur.record_event()
            for i, g in enumerate(self.lane_graphs):
                st = streams[i % len(streams)]
                st.wait_event(ev)
                with torch.cuda.stream(st):
                    g.replay()
            torch.cuda.synchronize(dev)
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best

    def _settle_streams(self, attempts=3):
        """The lanes must really overlap: measured on the captured graphs themselves.  `_concurrent_streams` picks streams with a spin
        kernel, and that has been seen to let two lanes share a hardware queue now and then (a 4-lane step of 10.6-11 ms instead of
        6.7: twice in ~25 processes) -- a replay may run on any stream, so the lanes are re-seated until all lanes together take
        clearly less than the same graphs back to back on one stream; the best seating seen is kept (`settle_seating` is the decision,
        a pure function of the timings: tests/test_host.py drives it with injected ones).  The lanes are timed on REAL data: the
        caller has replayed `self.graph` (zeroed gradients, this step's transposed weights and BatchNorm folds) before."""
        self._lanes_ms(self.streams, 1)                                  # warm-up
        serial = self._lanes_ms(self.streams[:1])
        pool = [self.streams]           # candidate stream sets: bounded, and the losers are dropped with this list

        def candidate():
            pool.append(_concurrent_streams(self.lanes, self.images.device))
            return len(pool) - 1

        # (four lanes that overlap take 0.44-0.45 of the serial time, two sharing a queue ~0.7; two lanes that overlap ~0.57)
        d = settle_seating(serial, self._lanes_ms(self.streams), lambda k: self._lanes_ms(pool[k]), candidate, attempts,
                           threshold=min(0.9, 1.0 / self.lanes + 0.3))
        self.streams = pool[d['seating']]
        self.lane_overlap = {'lanes_ms': round(d['lanes_ms'], 3), 'serial_ms': round(serial, 3), 'settled': d['settled'],
                             'attempts': d['attempts'], 'lanes': self.lanes}
        if not d['settled']:
            import warnings
            warnings.warn('GraphedTrainStep(lanes=%d): the lane graphs did not overlap after %d re-seatings (%.2f ms against %.2f ms '
                          'back to back); the step runs on the best seating seen' % (self.lanes, d['attempts'], d['lanes_ms'], serial))

    def _replay(self):
        self.graph.replay()
        if self.lanes > 1:
            cur = torch.cuda.current_stream()
            ev = cur.record_event()
            for st, g in zip(self.streams, self.lane_graphs):
                st.wait_event(ev)
                with torch.cuda.stream(st):
                    g.replay()
            for st in self.streams:
                cur.wait_stream(st)
            self.loss = torch.stack([l.detach() for l in self.lane_losses]).sum()
