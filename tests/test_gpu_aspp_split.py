"""The ASPP heads in the opt-in split-bf16 matrix modes ('bf16x3', 'bf16x6') against the reference's own outputs
(tests/golden/aspp.npz) at the tolerance of test_aspp_heads_vs_reference_golden, and the mode's plumbing: back to 'fp32' bit for bit,
pack rebuilt after a weight edit, graph capture, and train() untouched by the mode."""
import pytest
import torch

from tests.cases import ASPP_CASES
from tests.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _head(name, mode='fp32'):
    from mspl_amd import aspp
    cls, ncls, shp, sd_seed, x_seed = ASPP_CASES[name]
    m = getattr(aspp, cls)(num_classes=ncls)
    m.matrix_mode = mode
    m.load_state_dict(synth_state_dict(m.state_dict(), sd_seed))
    return m.to(DEV).eval(), synth_input(shp, x_seed).to(DEV)


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16x6'])
@pytest.mark.parametrize('name', sorted(ASPP_CASES))
def test_split_modes_vs_reference_golden(name, mode, golden, monkeypatch):
    from mspl_amd import ops
    m, x = _head(name, mode)
    assert m.matrix_mode == mode                          # survived load_state_dict
    calls = []
    real = ops.dense_conv_split
    monkeypatch.setattr(ops, 'dense_conv_split', lambda *a, **k: (calls.append(a[1].shape[0]), real(*a, **k))[1])
    with torch.no_grad():
        y = m(x).cpu()
    assert calls == [{'bf16x3': 2, 'bf16x6': 3}[mode]] * 5          # the four convolutions of the feature map and conv_1x1_3
    ref = torch.from_numpy(golden('aspp')[name])
    print('%s %s: max |logit - reference| %.3e' % (name, mode, float((y - ref).abs().max())))
    torch.testing.assert_close(y, ref, rtol=1e-4, atol=5e-4)


def test_back_to_fp32_is_bit_identical_and_pack_follows_the_weights():
    name = 'aspp_c13'
    fresh, x = _head(name)
    m, _ = _head(name, 'bf16x3')
    with torch.no_grad():
        want = fresh(x)
        split = m(x)
        assert not torch.equal(split, want)               # the mode does something
        m.matrix_mode = 'fp32'
        assert torch.equal(m(x), want)
        m.matrix_mode = 'bf16x3'
        assert torch.equal(m(x), split)
        m.conv_3x3_1.weight[5, 7, 1, 1] += 0.25           # the centre tap: live at every pixel
        edited = m(x)
        assert not torch.equal(edited, split), 'the split pack was not rebuilt after the weight changed'
        m.load_state_dict(fresh.state_dict())
        assert m.matrix_mode == 'bf16x3' and torch.equal(m(x), split)


def test_graph_replay_equals_eager():
    m, x = _head('aspp_c13', 'bf16x3')
    with torch.no_grad():
        eager = m(x).clone()                              # also builds the packs and epilogue vectors outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = m(x)
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, eager)


def test_train_ignores_the_mode():
    """train() with gradients enabled: the same logits bit for bit whatever the mode (the training path stays exact fp32)."""
    outs = []
    for mode in ('fp32', 'bf16x3'):
        m, x = _head('aspp_c13', mode)
        m.train()
        outs.append(m(x).detach())
    assert torch.equal(outs[0], outs[1])
