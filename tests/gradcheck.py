"""Per-tensor comparison of a training step's gradients with a float64 oracle, and the conditioning check of a case.

The global checks elsewhere in the suite (one tolerance scaled by the largest gradient of the whole network) cannot see the small
tensors: the smallest of the 340 uest gradients are 5e-6 .. 4e-4 of the largest one (PReLU slopes, BatchNorm affines, some 1x1
layers).  Here every tensor is held to its own scale: a relative norm error, and every element against the largest element of
ITS tensor, with a floor of 1e-12 of the global largest (so an all-zero reference tensor still compares).
"""
import numpy as np
import torch
import torch.nn.functional as F


def _np64(t):
    return t.detach().to('cpu', torch.float64).numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def grad_errors(got, ref, floor_rel=1e-12):
    """{name: (relative norm error, largest element error / largest reference element of the tensor)} over the tensors that have a
    reference gradient, plus the absolute floor.  got / ref: {name: tensor or None}."""
    ref64 = {n: _np64(r) for n, r in ref.items() if r is not None}
    gmax = max(float(np.abs(r).max()) for r in ref64.values())
    floor = floor_rel * gmax
    out = {}
    for n, r in ref64.items():
        g = _np64(got[n])
        assert g.shape == r.shape, '%s: shape %s, reference %s' % (n, g.shape, r.shape)
        d = g - r
        out[n] = (float(np.linalg.norm(d)) / max(float(np.linalg.norm(r)), floor),
                  float(np.abs(d).max()) / max(float(np.abs(r).max()), floor))
    return out, floor


def assert_grads_match(got, ref, tau_rel, tau_el, n_expected=None, floor_rel=1e-12, what=''):
    """Every gradient on its own: the same tensors have one (None on both sides or on neither), ||g - r|| <= tau_rel ||r||, and
    |g - r| <= tau_el max|r_tensor| + floor element by element.  Returns the worst (relative norm error, name) and (element error,
    name) for the record; on failure the message lists the worst tensors."""
    assert set(got) == set(ref), '%s: tensor sets differ: %s' % (what, sorted(set(got) ^ set(ref))[:8])
    odd = [n for n in ref if (got[n] is None) != (ref[n] is None)]
    assert not odd, '%s: gradient present on one side only: %s' % (what, odd[:8])
    if n_expected is not None:
        have = sum(1 for r in ref.values() if r is not None)
        assert have == n_expected, '%s: %d tensors with a gradient, expected %d' % (what, have, n_expected)
    errs, floor = grad_errors(got, ref, floor_rel)
    bad = []
    for n, (rel, el) in errs.items():
        r = ref[n]
        d = np.abs(_np64(got[n]) - _np64(r))
        el_ok = bool((d <= tau_el * float(np.abs(_np64(r)).max()) + floor).all())
        if rel > tau_rel or not el_ok:
            bad.append((max(rel / tau_rel, el / tau_el), n, rel, el, tuple(r.shape)))
    if bad:
        bad.sort(reverse=True)
        lines = ['  %-60s rel %.3g  el %.3g  %s' % (n, rel, el, shp) for _, n, rel, el, shp in bad[:10]]
        raise AssertionError('%s: %d of %d gradients off (tau_rel %g, tau_el %g):\n%s' % (what, len(bad), len(errs), tau_rel, tau_el,
                                                                                          '\n'.join(lines)))
    worst_rel = max((rel, n) for n, (rel, _) in errs.items())
    worst_el = max((el, n) for n, (_, el) in errs.items())
    return worst_rel, worst_el


class ActivationRecorder:
    """Records every input of F.prelu / F.relu while the oracle runs (installed with pytest's monkeypatch): the cases' conditioning.
    A PReLU input within float32 rounding of zero can take the other slope on the GPU, and on maps of a few pixels that moves a
    gradient by per cent -- a property of the case, not of a kernel."""

    def __init__(self, monkeypatch):
        self.inputs = []
        prelu, relu = F.prelu, F.relu

        def rec_prelu(x, weight):
            self.inputs.append(x.detach())
            return prelu(x, weight)

        def rec_relu(x, inplace=False):
            self.inputs.append(x.detach().clone())
            return relu(x, inplace=inplace)
        monkeypatch.setattr(torch.nn.functional, 'prelu', rec_prelu)
        monkeypatch.setattr(torch.nn.functional, 'relu', rec_relu)

    def near_kinks(self, max_plane=256, rel=1e-5):
        """[(index, shape, count)] of the recorded activation inputs with <= max_plane pixels per plane that hold an element within
        rel * rms(tensor) of zero."""
        out = []
        for i, x in enumerate(self.inputs):
            if x.dim() != 4 or x.shape[2] * x.shape[3] > max_plane:
                continue
            x = x.double()
            rms = float(x.pow(2).mean().sqrt())
            k = int((x.abs() < rel * rms).sum())
            if k:
                out.append((i, tuple(x.shape), k))
        return out
