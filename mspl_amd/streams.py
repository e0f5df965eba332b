"""Streams that really run side by side: what every path that keeps several hipGraphs in flight asks for its lanes."""
import time

import torch


def _concurrent_streams(n, device, candidates=12, spin_cycles=400000):
    """n streams whose kernels really run side by side.  HIP multiplexes streams onto a few hardware queues (4 by default,
    GPU_MAX_HW_QUEUES); two streams on the same queue execute in order, and which queue a torch stream lands on depends on how
    many streams the process created before.  Measured, not assumed: a spin kernel on the candidate and on every stream
    chosen so far must take about as long as one spin, not the sum.  Falls back to plain new streams when no n-subset overlaps
    (e.g. GPU_MAX_HW_QUEUES=1)."""
    if n == 1 or not hasattr(torch.cuda, '_sleep'):
        return [torch.cuda.Stream(device=device) for _ in range(n)]

    def spin_ms(streams):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for st in streams:
            with torch.cuda.stream(st):
                torch.cuda._sleep(spin_cycles)
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) * 1e3

    pool = [torch.cuda.Stream(device=device) for _ in range(candidates)]
    # The spin kernel counts CYCLES: on an idle chip the first spins run at a low clock and take longer, and a baseline taken then makes
    # two serialised spins at the boosted clock look like one (seen as a four-lane train step of 11.8 ms instead of 7.5 ms: all lanes
    # on one queue).  So: clocks warmed up first, and the final choice VALIDATED against a baseline taken after it; a failed
    # validation repeats the selection.
    for _ in range(30):
        spin_ms(pool[:1])
    chosen = [pool[0]]
    for attempt in range(3):
        one = min(spin_ms(pool[:1]) for _ in range(3))
        chosen = [pool[0]]
        for st in pool[1:]:
            if len(chosen) == n:
                break
            if min(spin_ms(chosen + [st]) for _ in range(2)) < one * (1.0 + 0.5 * len(chosen)):
                chosen.append(st)
        if len(chosen) < n:
            break                                       # fewer hardware queues than lanes: nothing to validate
        together = min(spin_ms(chosen) for _ in range(3))
        alone = min(spin_ms(chosen[:1]) for _ in range(3))
        if together < 1.6 * alone:
            break
    while len(chosen) < n:
        chosen.append(torch.cuda.Stream(device=device))
    return chosen
