"""The pyramid streaming kernel with its stencil tables read from memory (mspl_pyr_stream_tables_build +
mspl_pyrpool_fused_tab_fwd) against the unchanged mspl_pyrpool_fused_fwd, which computes the tables in every workgroup: same
inputs, bit-identical outputs, at every seam of the table path (tests/pyr_stream_cases.py; test_pyr_stream_plan.py proves from the
library's plan query that each case reaches its seam).  Both paths are also held to float64 with the standing per-kernel bound
2e-5 + 1e-4 |ref|, so that the float32 reference cannot hide an error the two share."""
import pytest
import torch

from tests import pyr_stream_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ATOL, RTOL = 2e-5, 1e-4
_MEMO = {}


def _setup(name):
    """Inputs on the device, the float64 reference and both paths' outputs of a case: computed once, shared, never modified."""
    if name not in _MEMO:
        from mspl_amd import ops
        _, N, P, h, w, s0, s1 = C.case(name)
        sizes = C.sizes_of(h, w, s0, s1)
        inp = C.make_inputs(N, P, h, w, sizes, seed=len(name))
        dev = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else {i: t.to(DEV) for i, t in v.items()} if isinstance(v, dict)
                   else v.to(DEV)) for k, v in inp.items()}
        tab = ops.pyr_stream_tables(h, w, sizes, DEV)
        assert tab is not None
        _MEMO[name] = dict(N=N, P=P, h=h, w=w, sizes=sizes, inp=inp, dev=dev, tab=tab, ref=C.reference(inp, sizes))
        _MEMO[name]['old'] = _run(_MEMO[name], None)
        _MEMO[name]['new'] = _run(_MEMO[name], tab)
    return _MEMO[name]


def _run(s, tab, x=None, down=None, out=None):
    from mspl_amd import ops
    d = s['dev']
    x = d['x'] if x is None else x
    down = d['down_e'] if down is None else down
    stage = [d['stage_w'][i] if i < 3 else None for i in range(5)]
    maps = [down.get(i) for i in range(5)]
    ep = ops.Epi(d['ep_scale'], d['ep_shift'], d['ep_alpha'])
    if out is not None:                      # a slice of a wider destination: the constants sit at the destination's channels
        dst, coff = out
        ctot = dst.shape[1]
        wide = [torch.full((ctot,), 7.0, device=DEV) for _ in range(3)]
        for t, v in zip(wide, (d['ep_scale'], d['ep_shift'], d['ep_alpha'])):
            t[coff:coff + s['P']] = v
        ep = ops.Epi(*wide)
    return ops.pyrpool_fused(x, s['sizes'], stage, maps, d['br_scale'], d['br_shift'], d['br_alpha'], d['merge_w'], ep, out=out,
                             tables=tab)


@pytest.mark.parametrize('name', [c[0] for c in C.CASES])
def test_tables_path_is_bit_identical_and_close_to_float64(name):
    s = _setup(name)
    assert torch.equal(s['new'], s['old'])
    ref = s['ref']
    for path in ('old', 'new'):
        got = s[path].cpu().double()
        err = (got - ref).abs()
        print('%s %s: max |kernel - float64| %.3e' % (name, path, float(err.max())))
        assert bool((err <= ATOL + RTOL * ref.abs()).all()), (path, float(err.max()))


@pytest.mark.parametrize('name', ['pxl1_40x40', 'pxl2_two_blocks_20x126'])
def test_sliced_destination(name):
    """ctot > P, coff > 0: the slice equals the un-sliced result bit for bit on both paths, every other channel keeps its sentinel."""
    s = _setup(name)
    N, P, h, w = s['N'], s['P'], s['h'], s['w']
    coff, ctot = 3, P + 5
    for tab in (None, s['tab']):
        dst = torch.full((N, ctot, h, w), -123.25, device=DEV)
        _run(s, tab, out=(dst, coff))
        assert torch.equal(dst[:, coff:coff + P], s['old'])
        rest = torch.cat([dst[:, :coff], dst[:, coff + P:]], 1)
        assert bool((rest == -123.25).all())


def test_image_alone_equals_image_in_the_batch():
    """The batch decides the segment length (test_pyr_stream_plan.py: 40 rows for the whole batch, 6 for one image), never a row's
    arithmetic."""
    s = _setup(C.BATCH_CASE)
    for k in (0, 77, s['N'] - 1):
        one = _run(s, s['tab'], x=s['dev']['x'][k:k + 1].contiguous(),
                   down={i: t[k:k + 1].contiguous() for i, t in s['dev']['down_e'].items()})
        assert torch.equal(one[0], s['new'][k])


def test_table_of_another_geometry_is_refused():
    a, b = _setup('pxl1_40x40'), _setup('pxl1_24x62')
    dst = torch.full((a['N'], a['P'], a['h'], a['w']), 5.5, device=DEV)
    with pytest.raises(RuntimeError, match='tables were built for a 24x62 map'):
        _run(a, b['tab'], out=(dst, 0))
    with pytest.raises(RuntimeError, match='no geometry tables were built at'):
        _run(a, torch.zeros_like(a['tab']), out=(dst, 0))
    torch.cuda.synchronize()
    assert bool((dst == 5.5).all())


def test_two_builds_give_identical_bytes():
    from mspl_amd import ops
    for name in ('pxl1_40x40', 'pxl2_two_blocks_20x126'):
        s = _setup(name)
        again = ops.pyr_stream_tables(s['h'], s['w'], s['sizes'], DEV)
        assert again.data_ptr() != s['tab'].data_ptr() and torch.equal(again.view(torch.int32), s['tab'].view(torch.int32))


def _net():
    import argparse
    from mspl_amd import models
    from tests.synth import synth_state_dict
    a = argparse.Namespace(s=2.0, channels=3, num_classes=1000)
    m = models.ESPDNetwithUncertaintyEstimation(a, classes=13, dataset='camvid', fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    return m.cuda().eval()


def _tensors(out):
    return [out] if torch.is_tensor(out) else list(out)


def test_model_logits_with_and_without_tables(monkeypatch):
    """ESPDNet-UE s = 2.0, C = 13, 2 x 3 x 64 x 96: the table path on against off, eager and graphed with two replays."""
    from mspl_amd import layers
    from tests.synth import synth_input
    m = _net()
    x = synth_input((2, 3, 64, 96), 4).to(DEV)
    used = []
    real = layers.ops.pyr_stream_tables
    monkeypatch.setattr(layers.ops, 'pyr_stream_tables', lambda *a: used.append(a[:2]) or real(*a))
    out = {}
    for on in (False, True):
        monkeypatch.setattr(layers, '_PYR_STREAM_TABLES', on)
        with torch.no_grad():
            eager = [t.clone() for t in _tensors(m(x))]
            stat = x.clone()
            g = torch.cuda.CUDAGraph()
            with layers.graph_capture(g), layers.side_streams(False):       # (a linear graph: the lanes of a label pass capture like this)
                cap = _tensors(m(stat))
            reps = []
            for _ in range(2):
                g.replay()
                reps.append([t.clone() for t in cap])
        out[on] = (eager, reps)
    assert used, 'no pyramid of the model took the table path'
    for a, b in zip(out[True][0], out[False][0]):
        assert torch.equal(a, b)
    for rep in out[True][1] + out[False][1]:
        for a, b in zip(rep, out[False][0]):
            assert torch.equal(a, b)


def test_pipelined_label_pass_with_and_without_tables(monkeypatch):
    from mspl_amd import layers, uest
    g = torch.Generator().manual_seed(9)
    batches = [torch.randn((2, 3, 64, 96), generator=g).cuda() for _ in range(5)]
    got = {}
    for on in (False, True):
        monkeypatch.setattr(layers, '_PYR_STREAM_TABLES', on)
        m = _net()
        plp = uest.PipelinedLabelPass(lambda: uest.SelfLabelPass(m, classes=13, use_graph=True), depth=2, group=2)
        outs = []
        for b in batches:
            o = plp(b)
            if o is not None:
                outs.append((o[0].clone(), o[1].clone()))
        outs += [(o[0].clone(), o[1].clone()) for o in plp.flush()]
        torch.cuda.synchronize()
        got[on] = (outs, plp.hist.clone(), any('_mspl_pyr_tables' in mod.__dict__ and any(v is not None for v in mod.__dict__['_mspl_pyr_tables'].values())
                                               for mod in m.modules()))
    assert got[True][2] and not got[False][2]
    assert len(got[True][0]) == len(got[False][0]) == 5
    for (l1, k1), (l0, k0) in zip(got[True][0], got[False][0]):
        assert torch.equal(l1, l0) and torch.equal(k1, k0)
    assert torch.equal(got[True][1], got[False][1])
