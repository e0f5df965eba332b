"""autograd.GradDst / GradDstGroup / GradDstPair: where a parameter gradient goes (bookkeeping only: CPU tensors, no launch)."""
import pytest
import torch

from mspl_amd import autograd as ag


def _param(shape=(6,), grad=True):
    p = torch.nn.Parameter(torch.randn(shape))
    if grad:
        p.grad = torch.full(shape, 3.0)
    return p


def _shares_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def test_sink_inside_the_scope_is_the_grad_buffer_itself():
    p = _param()
    with ag.grad_sinks():
        d = ag.GradDst(p)
    assert d.is_sink
    for zeroed in (True, False):
        assert d.buf(zeroed=zeroed) is p.grad
        assert bool((p.grad == 3.0).all())           # handing it out does not touch it
        assert d.result() is None


def test_forward_time_capture_survives_the_scope():
    p, q = _param(), _param()
    with ag.grad_sinks():
        d = ag.GradDst(p)
    outside = ag.GradDst(q)
    with ag.grad_sinks():
        # made outside, used inside: still no sink; made inside, used after the exit: still the sink
        assert not outside.is_sink and outside.buf(zeroed=True) is not q.grad
    assert d.is_sink and d.buf(zeroed=True) is p.grad and d.result() is None


def _non_contiguous():
    p = _param((4, 6), grad=False)
    p.grad = torch.zeros(6, 4).t()
    assert not p.grad.is_contiguous()
    return p


def _half_grad():
    p = torch.nn.Parameter(torch.randn(6, dtype=torch.float16))
    p.grad = torch.zeros(6, dtype=torch.float16)
    return p


def _no_sink_cases():
    return {'outside the scope': (_param(), False),
            'non-leaf': (_param() * 2.0, True),
            'no .grad yet': (_param(grad=False), True),
            'non-contiguous .grad': (_non_contiguous(), True),
            'non-float32 .grad': (_half_grad(), True),
            'requires no grad': (torch.randn(6), True),
            'scope disabled': (_param(), None)}


@pytest.mark.parametrize('case', sorted(_no_sink_cases()))
def test_no_sink_yields_a_fresh_tensor_that_is_the_result(case):
    p, inside = _no_sink_cases()[case]
    if inside is None:
        with ag.grad_sinks(enabled=False):
            d = ag.GradDst(p)
    elif inside:
        with ag.grad_sinks():
            d = ag.GradDst(p)
    else:
        d = ag.GradDst(p)
    assert not d.is_sink
    t = d.buf(zeroed=True)
    assert t.shape == p.shape and t.dtype == torch.float32 and t.device == p.device
    assert bool((t == 0).all())
    if p.is_leaf and p.grad is not None:
        assert not _shares_storage(t, p.grad)
    assert d.result() is t
    e = d.buf(zeroed=False)                          # overwrite semantics: any fresh tensor of the right shape
    assert e is not t and e.shape == p.shape and e.dtype == torch.float32
    assert d.result() is e
    assert d.result() is None                        # handed over once; the node does not keep it alive


def test_parameter_none_has_no_buffer_and_no_result():
    with ag.grad_sinks():
        d = ag.GradDst(None)
    assert not d.is_sink
    assert d.buf(zeroed=True) is None and d.buf(zeroed=False) is None
    assert d.result() is None


def _count_allocations(monkeypatch):
    calls = []
    for name in ('zeros', 'empty'):
        real = getattr(torch, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls.append((_name, a[0]))
            return _real(*a, **kw)
        monkeypatch.setattr(torch, name, counted)
    return calls


def test_group_makes_one_zeroed_allocation_for_the_members_without_a_sink(monkeypatch):
    gamma, beta, alpha = _param(), _param(grad=False), _param(grad=False)
    with ag.grad_sinks():
        g = ag.GradDstGroup(gamma, beta, alpha)
    calls = _count_allocations(monkeypatch)
    d_gamma, d_beta, d_alpha = g.bufs()
    assert calls == [('zeros', (3, 6))]
    assert d_gamma is gamma.grad
    assert d_beta.shape == (6,) and d_alpha.shape == (6,) and bool((d_beta == 0).all()) and bool((d_alpha == 0).all())
    assert _shares_storage(d_beta, d_alpha) and d_beta.data_ptr() != d_alpha.data_ptr()
    assert d_beta.data_ptr() == d_alpha.data_ptr() - 6 * 4       # row i belongs to member i
    r = g.results()
    assert r[0] is None and r[1] is d_beta and r[2] is d_alpha


def test_group_allocates_nothing_when_every_member_has_a_sink(monkeypatch):
    ps = [_param((5, 1, 3, 3)) for _ in range(4)]
    with ag.grad_sinks():
        g = ag.GradDstGroup(*ps)
    calls = _count_allocations(monkeypatch)
    bufs = g.bufs()
    assert calls == []
    assert all(b is p.grad for b, p in zip(bufs, ps))
    assert [v for v in g.ptrs()] == [p.grad.data_ptr() for p in ps]
    assert g.results() == [None] * 4


def test_group_skips_a_member_that_is_not_wanted(monkeypatch):
    scale, alpha = _param(), _param()
    with ag.grad_sinks():
        g = ag.GradDstGroup(scale, None, alpha)      # every wanted member has a sink: no allocation
    calls = _count_allocations(monkeypatch)
    assert [b is t for b, t in zip(g.bufs(), (scale.grad, None, alpha.grad))] == [True] * 3
    assert calls == [] and g.results() == [None] * 3
    g = ag.GradDstGroup(scale, None, alpha)          # outside the scope: one (3, C) accumulator, nothing for the None
    d_scale, d_shift, d_alpha = g.bufs()
    assert calls == [('zeros', (3, 6))]
    assert d_shift is None and _shares_storage(d_scale, d_alpha)
    r = g.results()
    assert r[0] is d_scale and r[1] is None and r[2] is d_alpha


def test_pair_is_direct_only_when_both_members_have_sinks():
    rows = torch.empty(4, 6)
    for has_gamma, has_beta in ((True, True), (True, False), (False, True), (False, False)):
        gamma, beta = _param(grad=has_gamma), _param(grad=has_beta)
        with ag.grad_sinks():
            pair = ag.GradDstPair(gamma, beta)
        direct, d_gamma, d_beta = pair.bufs(rows[0], rows[1])
        if has_gamma and has_beta:
            assert direct == 1 and pair.direct and d_gamma is gamma.grad and d_beta is beta.grad
            assert pair.results() == (None, None)
        else:
            assert direct == 0 and not pair.direct
            assert d_gamma.data_ptr() == rows[0].data_ptr() and d_beta.data_ptr() == rows[1].data_ptr()
            r = pair.results()
            assert r[0] is d_gamma and r[1] is d_beta
    gamma, beta = _param(), _param()
    pair = ag.GradDstPair(gamma, beta)               # outside the scope
    assert pair.bufs(rows[0], rows[1])[0] == 0
