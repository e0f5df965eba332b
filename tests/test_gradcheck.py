"""CPU tier: the per-tensor gradient comparator (tests/gradcheck.py) has the power the global checks lack.  The float32 oracle's
gradients pass against the float64 oracle at the uest tolerances of tests/test_gpu_grad_parity.py; one mutation each -- the kind
of slip a kernel makes in a small tensor -- fails."""
import json
import os

import pytest
import torch

from oracle import train as otrain
from tests.cases import TRAIN_CASES
from tests.conftest import GOLDEN
from tests.gradcheck import ActivationRecorder, assert_grads_match
from tests.synth import synth_input, synth_labels, synth_state_dict

KEYS = json.load(open(os.path.join(GOLDEN, 'state_dict_keys.json')))
UEST_TAU_REL, UEST_TAU_EL = 1e-4, 1e-3


def _param_names(template):
    return [k for k in template if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]


@pytest.fixture(scope='module')
def oracle_grads():
    c = TRAIN_CASES['train_step_64x96']
    tmpl = KEYS['espdnetue_s%s_c%d' % (c['s'], c['classes'])]
    names = _param_names(tmpl)
    sd = synth_state_dict(tmpl, c['sd_seed'])
    x = synth_input(c['shape'], c['in_seed'])
    y = synth_labels((c['shape'][0],) + c['shape'][2:], c['classes'], c['in_seed'])
    out = {}
    for dt in (torch.float32, torch.float64):
        sdt = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
        _, g, _ = otrain.train_step(sdt, names, x.to(dt), y, torch.ones(c['classes'], dtype=dt), c['ignore_idx'])
        out[dt] = g
    return out[torch.float32], out[torch.float64]


def _check(got, ref):
    return assert_grads_match(got, ref, UEST_TAU_REL, UEST_TAU_EL, n_expected=340)


def test_float32_oracle_passes(oracle_grads):
    g32, g64 = oracle_grads
    (rel, _), (el, _) = _check(g32, g64)
    assert rel < 1e-5 and el < 1e-4           # (measured: 1.1e-6 and 1.6e-6 -- two orders below the tolerances)


def _smallest(ref, pred):
    """The name of the tensor with the smallest non-zero gradient norm among those matching pred: the hardest to see."""
    return min((float(r.norm()), n) for n, r in ref.items() if r is not None and float(r.norm()) > 0 and pred(n, r))[1]


def _prelu_zeroed(g, ref):
    n = _smallest(ref, lambda n, r: n.endswith('act.weight'))
    g[n] = torch.zeros_like(g[n])


def _bn_beta_doubled(g, ref):
    n = _smallest(ref, lambda n, r: n.endswith('bn.bias'))
    g[n] = g[n] * 2


def _dw_channels_swapped(g, ref):
    n = _smallest(ref, lambda n, r: 'spp_dw' in n and r.dim() == 4)
    r = ref[n]
    # the two output channels whose gradients differ most (a swap of two equal channels would be no error)
    d = [(float((r[i] - r[i + 1]).abs().max()), i) for i in range(r.shape[0] - 1)]
    i = max(d)[1]
    t = g[n].clone()
    t[[i, i + 1]] = t[[i + 1, i]]
    g[n] = t


def _one_by_one_scaled(g, ref):
    n = _smallest(ref, lambda n, r: r.dim() == 4 and r.shape[2:] == (1, 1))
    g[n] = g[n] * 1.01


def _moved_to_twin(g, ref):
    # the smallest tensor that has a twin of the same shape; the twin's gradient lands in its place
    best = None
    for n, r in ref.items():
        if r is None or float(r.norm()) == 0:
            continue
        twins = [m for m, s in ref.items() if m != n and s is not None and s.shape == r.shape]
        if twins and (best is None or float(r.norm()) < best[0]):
            best = (float(r.norm()), n, twins[0])
    _, n, m = best
    g[n] = g[m].clone()


@pytest.mark.parametrize('mutate', [_prelu_zeroed, _bn_beta_doubled, _dw_channels_swapped, _one_by_one_scaled, _moved_to_twin],
                         ids=['prelu_alpha_zeroed', 'bn_beta_doubled', 'dw_channels_swapped', 'conv1x1_scaled_1.01', 'moved_to_twin'])
def test_each_mutation_fails(oracle_grads, mutate):
    g32, g64 = oracle_grads
    g = dict(g32)
    mutate(g, g64)
    with pytest.raises(AssertionError, match='gradients off'):
        _check(g, g64)


def test_tensor_sets_must_agree(oracle_grads):
    g32, g64 = oracle_grads
    n = next(n for n, r in g64.items() if r is not None)
    g = dict(g32)
    g[n] = None
    with pytest.raises(AssertionError, match='one side only'):
        _check(g, g64)
    g = dict(g32)
    del g[n]
    with pytest.raises(AssertionError, match='sets differ'):
        _check(g, g64)


def test_activation_recorder_sees_near_kinks(monkeypatch):
    """The conditioning check of the GPU cases: it finds an activation input planted at zero on a small map, and ignores big maps."""
    rec = ActivationRecorder(monkeypatch)
    small, big = torch.randn(2, 4, 3, 5), torch.randn(1, 2, 32, 32)
    small[1, 2, 0, 3] = 0.0
    big[0, 1, 5, 5] = 0.0
    torch.nn.functional.prelu(small, torch.full((4,), 0.25))
    torch.nn.functional.relu(big)
    assert [(s, k) for _, s, k in rec.near_kinks()] == [((2, 4, 3, 5), 1)]


# ------------------------------------------------------------------ the supervised step (batch-statistics BatchNorm)
# The same proof for tests/test_gpu_supervised_grad_parity.py, with ITS constants: the float32 oracle's supervised gradients pass
# against float64 at the small-case tolerances, and the slips a batch-statistics kernel can make fail.
@pytest.fixture(scope='module')
def supervised_grads():
    """(float32 gradients, float64 gradients, run(dtype) for further float32 runs) of the smallest supervised case."""
    from tests import test_gpu_supervised_grad_parity as sup
    from tests.gradcheck import supervised_groups
    case = sup.CASES[sup.SMALLEST]
    m = case.model()
    names = [n for n, _ in m.named_parameters()]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y, _ = case.data()

    def run(dt):
        sdt = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
        return otrain.supervised_step(sdt, supervised_groups(names, sup.LR, sup.LR_MULT), x.to(dt), y, None, case.ignore_idx,
                                      sup.MOMENTUM, sup.WEIGHT_DECAY, sup.FLOOD)[1]
    return run(torch.float32), run(torch.float64), run


def _sup_check(got, ref):
    from tests import test_gpu_supervised_grad_parity as sup
    return assert_grads_match(got, ref, sup.SUP_TAU_REL, sup.SUP_TAU_EL, n_expected=340)


def test_float32_oracle_supervised_passes(supervised_grads):
    g32, g64, _ = supervised_grads
    _sup_check(g32, g64)


def test_supervised_statistics_as_constants_fail(supervised_grads, monkeypatch):
    """A backward that treats the batch mean and variance as constants (the direct path alone, no p * z + q term)."""
    from oracle import net as onet
    _, g64, run = supervised_grads

    def bn_detached(x, sd, p):
        assert onet.BN_MODE['training']
        mean = x.mean((0, 2, 3), keepdim=True).detach()
        var = x.var((0, 2, 3), unbiased=False, keepdim=True).detach()
        return (x - mean) / torch.sqrt(var + onet.BN_EPS) * sd[p + '.weight'].view(1, -1, 1, 1) + sd[p + '.bias'].view(1, -1, 1, 1)
    monkeypatch.setattr(onet, '_bn', bn_detached)
    with pytest.raises(AssertionError, match='gradients off'):
        _sup_check(run(torch.float32), g64)


def _bn_gamma_scaled(g, ref):
    n = _smallest(ref, lambda n, r: n.endswith(('bn.weight', 'cbr.1.weight', 'br.0.weight')))
    g[n] = g[n] * 1.01


def _small_negated(g, ref):
    n = _smallest(ref, lambda n, r: r.numel() <= 64)
    g[n] = -g[n]


@pytest.mark.parametrize('mutate', [_bn_gamma_scaled, _small_negated], ids=['bn_gamma_scaled_1.01', 'small_tensor_negated'])
def test_each_supervised_mutation_fails(supervised_grads, mutate):
    g32, g64, _ = supervised_grads
    g = dict(g32)
    mutate(g, g64)
    with pytest.raises(AssertionError, match='gradients off'):
        _sup_check(g, g64)


def test_supervised_tensor_sets_must_agree(supervised_grads):
    g32, g64, _ = supervised_grads
    n = next(n for n, r in g64.items() if r is not None)
    g = dict(g32)
    g[n] = None
    with pytest.raises(AssertionError, match='one side only'):
        _sup_check(g, g64)
