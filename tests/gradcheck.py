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


SEG_PREFIXES = ('bu_dec_l1.', 'bu_dec_l2.', 'bu_dec_l3.', 'bu_dec_l4.', 'merge_enc_dec_l4.', 'merge_enc_dec_l3.', 'merge_enc_dec_l2.',
                'bu_br_l4.', 'bu_br_l3.', 'bu_br_l2.')


def supervised_groups(names, lr=0.009, lr_mult=10.0, use_depth=False):
    """The SGD groups of the supervised loop as oracle.train.supervised_step takes them: base net at lr, segmentation head (and, with
    a depth image, the depth encoder) at lr * lr_mult.  Every other parameter (auxiliary decoder, fusion gates, the depth encoder's
    blocks the RGB path borrows) is in no group of the loop: it goes into a last group with lr 0, so the oracle returns its gradient
    and leaves its value alone."""
    base = [n for n in names if n.startswith('base_net.')]
    seg = [n for n in names if n.startswith(SEG_PREFIXES)]
    dep = [n for n in names if n.startswith('depth_base_net.')] if use_depth else []
    taken = set(base) | set(seg) | set(dep)
    groups = [(base, lr), (seg, lr * lr_mult)] + ([(dep, lr * lr_mult)] if use_depth else [])
    return groups + [([n for n in names if n not in taken], 0.0)]


class BatchNormRecorder:
    """Records, for every F.batch_norm call while the oracle runs, the number of values per channel behind its running_var buffer
    and how often the buffer was used (keyed by the buffer's storage): what a test needs to restate the unbiased-variance factor
    n / (n - 1) for another batch size, and to know num_batches_tracked after the step (with a depth image the RGB and the depth
    branch share some blocks, whose BatchNorms then run twice per forward)."""

    def __init__(self, monkeypatch):
        self.count = {}
        batch_norm = F.batch_norm

        def rec(x, running_mean, running_var, *a, **k):
            calls = self.count.get(running_var.data_ptr(), (0, 0))[1]
            self.count[running_var.data_ptr()] = (x.numel() // x.shape[1], calls + 1)
            return batch_norm(x, running_mean, running_var, *a, **k)
        monkeypatch.setattr(torch.nn.functional, 'batch_norm', rec)

    def per_channel(self, after):
        """{running_var key: (values per channel, calls)} for the oracle's returned state dict."""
        return {k: self.count[v.data_ptr()] for k, v in after.items() if k.endswith('running_var') and v.data_ptr() in self.count}


def running_var_for_copies(before, after, n, copies, momentum=0.1):
    """running_var after one step on `copies` permuted copies of the batch, from the oracle's value for the batch alone (n values per
    channel): the biased batch variance is the same, the unbiased factor becomes copies * n / (copies * n - 1).  float64."""
    var_b = (after - (1 - momentum) * before) / (momentum * n / (n - 1.0))
    m = float(copies * n)
    return (1 - momentum) * before + momentum * var_b * (m / (m - 1.0))


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
