"""layers.graph_capture: the garbage collector stays out of a stream capture.  A dead cycle that holds a CUDAGraph must be
finalised before the capture begins, never inside it (the runtime forbids freeing a graph's pool during a capture)."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


class _Cycle(object):
    """Garbage only the cyclic collector can free; records whether it was finalised and whether a capture was under way then."""
    log = []

    def __init__(self):
        self.me = self

    def __del__(self):
        _Cycle.log.append(torch.cuda.is_current_stream_capturing())


def test_collector_runs_before_the_capture_and_not_inside():
    from mspl_amd import layers
    assert gc.isenabled()
    _Cycle.log = []
    _Cycle()                                             # dead at once, but only the collector can tell
    x = torch.ones(64, device=DEV)
    g = torch.cuda.CUDAGraph()
    with layers.graph_capture(g):
        assert _Cycle.log == [False]                     # finalised on entry, outside the capture
        assert not gc.isenabled()
        _Cycle()
        junk = [[] for _ in range(5000)]                 # enough allocations to trip the automatic collector, were it on
        del junk
        y = x * 2
    assert gc.isenabled()
    gc.collect()
    assert _Cycle.log == [False, False]                  # the second one waited for the end of the capture
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, x * 2)


def test_collector_is_switched_back_on_after_a_failed_capture():
    from mspl_amd import layers
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ZeroDivisionError):
        with layers.graph_capture(g):
            1 / 0
    assert gc.isenabled() and not torch.cuda.is_current_stream_capturing()
    torch.cuda.synchronize()
