"""CPU-side checks of what the training steps share (mspl_amd/steps.py): the flat layout both optimizers get from FlatOptimizer,
reattach() and reset() on each, the `step` seam the optimizer audit replaces, and forward_loss on a one-head model.  The optimizers
are built on CPU tensors after a backward through a three-parameter stand-in; no kernel is launched and step() never runs."""
import types

import pytest
import torch

from mspl_amd import steps, supervised, training


class StandIn(torch.nn.Module):
    """Three parameters; the 13-element one sits in front of a larger one, so the 4-float alignment padding is in the layout."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.slope = torch.nn.Parameter(torch.randn(13, generator=g))
        self.weight = torch.nn.Parameter(torch.randn(6, 13, generator=g))
        self.bias = torch.nn.Parameter(torch.randn(6, generator=g))

    def forward(self, x):
        return torch.nn.functional.linear(x * self.slope, self.weight, self.bias)


def _after_backward():
    m = StandIn()
    m(torch.ones(2, 13)).pow(2).mean().backward()
    return m


def _adam(m):
    return training.FlatAdam(m.parameters(), lr=1e-3)


def _sgd(m):
    return supervised.FlatSGD([{'params': [m.slope, m.weight], 'lr': 0.1}, {'params': [m.bias], 'lr': 1.0}], lr=0.1, momentum=0.9)


BUILD = {'adam': _adam, 'sgd': _sgd}


def test_both_optimizers_share_the_flat_layout():
    offsets = {}
    for kind, build in BUILD.items():
        m = _after_backward()
        before = [(p.detach().clone(), p.grad.detach().clone()) for p in m.parameters()]
        opt = build(m)
        assert isinstance(opt, steps.FlatOptimizer) and opt.params == list(m.parameters()) and opt.step_count == 0
        assert opt.flat_p is opt.bucket.flat_p and opt.flat_g is opt.bucket.flat
        for p, off, (p0, g0) in zip(opt.params, opt.bucket.offsets, before):
            assert p.data_ptr() == opt.flat_p.data_ptr() + 4 * off and p.grad.data_ptr() == opt.flat_g.data_ptr() + 4 * off
            assert torch.equal(p.detach(), p0) and torch.equal(p.grad, g0)          # values preserved by the re-pointing
        for name in opt.STATE:
            assert getattr(opt, name).shape == opt.flat_p.shape and not getattr(opt, name).any()
        offsets[kind] = list(opt.bucket.offsets)
    assert offsets['adam'] == offsets['sgd'] == [0, 16, 16 + 80]                    # 13 floats padded to 16
    assert BUILD['sgd'](_after_backward()).param_groups[0]['_hi'] == 96


@pytest.mark.parametrize('kind', sorted(BUILD))
def test_no_backward_no_optimizer(kind):
    with pytest.raises(RuntimeError, match='^%s: run one backward' % {'adam': 'FlatAdam', 'sgd': 'FlatSGD'}[kind]):
        BUILD[kind](StandIn())


@pytest.mark.parametrize('kind', sorted(BUILD))
def test_reattach(kind):
    m = _after_backward()
    opt = BUILD[kind](m)
    m.slope.grad = None
    m.bias.grad = torch.zeros(6)
    opt.reattach()
    b = opt.bucket
    assert all(p.grad.data_ptr() == b.flat.data_ptr() + 4 * off for p, off in zip(b.params, b.offsets))
    m.weight.data = torch.zeros(6, 13)
    with pytest.raises(RuntimeError, match='%s: a parameter no longer lives in the flat parameter buffer' % type(opt).__name__):
        opt.reattach()


def _dirty(opt):
    for name in opt.STATE:
        getattr(opt, name).fill_(1.0)
    opt.step_count = 3


def test_reset_adam():
    opt = _adam(_after_backward())
    _dirty(opt)
    opt.reset()
    assert not opt.m.any() and not opt.v.any() and opt.step_count == 0
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay) == (1e-3, (0.9, 0.999), 1e-8, 0.0)
    _dirty(opt)
    opt.reset(lr=0.25, betas=[0.5, 0.75])
    assert not opt.m.any() and not opt.v.any() and opt.step_count == 0
    assert (opt.lr, opt.param_groups[0]['lr'], opt.betas, opt.eps, opt.weight_decay) == (0.25, 0.25, (0.5, 0.75), 1e-8, 0.0)
    # GraphedTrainStep.reset_optimizer hands its arguments to it
    _dirty(opt)
    training.GraphedTrainStep.reset_optimizer(types.SimpleNamespace(optimizer=opt), 0.5, (0.1, 0.2), 1e-3, 0.125)
    assert not opt.m.any() and not opt.v.any() and opt.step_count == 0
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay) == (0.5, (0.1, 0.2), 1e-3, 0.125)


def test_reset_sgd():
    opt = _sgd(_after_backward())
    _dirty(opt)
    opt.reset()
    assert not opt.buf.any() and opt.step_count == 0 and [g['lr'] for g in opt.param_groups] == [0.1, 1.0]
    _dirty(opt)
    opt.reset([{'lr': 0.5, 'momentum': 0.8}, {'weight_decay': 0.25}])
    assert not opt.buf.any() and opt.step_count == 0
    assert [(g['lr'], g['momentum'], g['weight_decay']) for g in opt.param_groups] == [(0.5, 0.8, 0.0), (1.0, 0.9, 0.25)]
    with pytest.raises(ValueError, match='1 groups given, the optimizer has 2'):
        opt.reset([{'lr': 1.0}])


class StubOptimizer(object):
    def __init__(self, log):
        self.log = log

    def zero_grad(self):
        self.log.append('zero_grad')

    def all_reduce_grads(self):
        self.log.append('all_reduce')

    def step(self):
        self.log.append('step')


class StubSinks(object):
    """What autograd.collect_conv_weights / WeightTransposer.active hand to the step body."""

    def __init__(self, log, name):
        self.log, self.name = log, name

    def __enter__(self):
        self.log.append(self.name)
        return ['weights of ' + self.name]

    def __exit__(self, *exc):
        return False

    def active(self):
        return self


def test_run_step_calls_the_step_of_the_class(monkeypatch):
    """The optimizer audit replaces `step` on the subclass: run_step must reach it through the instance, after the all-reduce."""
    log = []
    monkeypatch.setattr(steps.layers, 'prefold_frozen_bn', lambda model: log.append('prefold'))
    monkeypatch.setattr(steps.ag, 'collect_conv_weights', lambda: StubSinks(log, 'collect'))
    monkeypatch.setattr(steps.ag, 'WeightTransposer', lambda got: ('transposer', got))

    class Sub(StubOptimizer):
        pass
    monkeypatch.setattr(Sub, 'step', lambda self: self.log.append('patched step'))
    counted = []
    meters = types.SimpleNamespace(count=counted.append)
    w = torch.nn.Parameter(torch.tensor([2.0]))

    def loss_fn():
        log.append('loss')
        return (w * 3.0).sum(), w * 1.0

    with torch.no_grad():                                   # (the body turns gradients on itself)
        loss, out, opt = steps.run_step(None, None, 7, loss_fn, lambda: Sub(log), meters)
    assert isinstance(opt, Sub) and opt.transposer == ('transposer', ['weights of collect'])
    assert log == ['collect', 'prefold', 'loss', 'all_reduce', 'patched step'] and counted == [7]
    assert float(loss) == 6.0 and not loss.requires_grad and not out.requires_grad and float(w.grad) == 3.0

    del log[:]
    opt.transposer = StubSinks(log, 'transposer')
    loss, out, again = steps.run_step(None, opt, 5, lambda: ((w * 3.0).sum(), None), None, None)
    assert again is opt and out is None and counted == [7]
    assert log == ['zero_grad', 'transposer', 'prefold', 'all_reduce', 'patched step']


def test_a_call_copies_replays_reduces_steps_and_counts():
    """GraphedStep.__call__ on stand-ins for the graph and the optimizer: the order of a replayed step, and what it returns."""
    log = []

    class Step(steps.GraphedStep):
        pass
    s = Step()
    s.graph = types.SimpleNamespace(replay=lambda: log.append('replay'))
    s.optimizer = StubOptimizer(log)
    s.meters = types.SimpleNamespace(count=lambda n: log.append(('count', n)))
    s._static = (torch.zeros(3, 2), torch.zeros(3), None)
    s.loss = torch.ones((), requires_grad=True) * 2.0
    got = s(torch.ones(3, 2), torch.full((3,), 7.0), None)
    assert log == ['replay', 'all_reduce', 'step', ('count', 3)]
    assert float(got) == 2.0 and not got.requires_grad
    assert bool((s._static[0] == 1).all()) and bool((s._static[1] == 7).all())
    s.outputs = torch.ones(3, requires_grad=True) * 1.0
    loss, outputs = s(torch.ones(3, 2), torch.zeros(3))
    assert not loss.requires_grad and not outputs.requires_grad and outputs.shape == (3,)


def test_forward_loss_refuses_a_one_head_model():
    class OneHead(torch.nn.Module):
        def forward_lowres(self, images):
            return images[:, :, ::2, ::2], None

    with pytest.raises(RuntimeError, match='forward_loss: OneHead returns one head'):
        training.forward_loss(OneHead(), torch.zeros(1, 5, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64), torch.ones(5))
