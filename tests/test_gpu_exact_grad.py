"""The gradient kernels on the integer data of tests/exact_cases.py, through the C ABI (so that accumulate, split and null outputs can
be chosen): every output tensor must EQUAL the float64 reference element for element -- no tolerance, no allowance of mismatches --
and a second call must give the same bits.  tests/test_exact_cases.py proves on the CPU that the data make every summation order
exact and that each case reaches the kernel form and chunk / band seam it is in the table for."""
import ctypes

import pytest
import torch

from tests import exact_cases as ec

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, misalign=False):
    """float32 on the GPU; misalign: starting one float into a larger buffer (4 bytes past 16-byte alignment)."""
    if t is None:
        return None
    if not misalign:
        d = t.to(DEV, torch.float32).contiguous()
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)
    d = buf[1:].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    return d


def _out(shape, pre=None, misalign=False):
    """An output buffer: what the case says it held before the call, or NaN where the kernel must overwrite."""
    return _dev(torch.full(tuple(shape), NAN, dtype=torch.float64) if pre is None else pre, misalign)


def _acc(shape, pre=None):
    """A buffer the kernel accumulates into: the case's integers, or zeros."""
    return _dev(torch.zeros(tuple(shape), dtype=torch.float64) if pre is None else pre)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def run_conv_wgrad(cfg, p, lib, check):
    N, Cin, Cout, G, H, W, K, s = cfg['shape']
    mis = bool(cfg.get('misalign'))
    x, gy = _dev(p['x'], mis), _dev(p['gy'], mis)
    gw = _out((Cout, Cin // G, K, K), p.get('pre_gw'))
    check(lib.mspl_conv_bwd_weight(_p(gy), _p(x), N, Cin, Cout, G, H, W, K, s, 1, int('pre_gw' in p), _p(gw), _stream()))
    return {'gw': gw}


def run_conv_dgrad(cfg, p, lib, check):
    N, Cin, Cout, G, H, W, K, s = cfg['shape']
    gy, w = _dev(p['gy']), _dev(p['w'])
    gx = _out((N, Cin, H, W), p.get('pre_gx'))
    check(lib.mspl_conv_bwd_data(_p(gy), _p(w), N, Cin, Cout, G, H, W, K, s, 1, int('pre_gx' in p), _p(gx), _stream()))
    return {'gx': gx}


def run_eesp_dw(cfg, p, lib, check):
    N, n, H, W = cfg['shape']
    gs, x, w4 = _dev(p['gs']), _dev(p['x']), _dev(p['w4'])
    gx = _out((N, n, H, W), misalign=bool(cfg.get('misalign_gx')))
    gw = _acc((4, n, 3, 3), p.get('pre_gw'))
    check(lib.mspl_eesp_dw_bwd(_p(gs), _p(x), _p(w4), (ctypes.c_int32 * 4)(*cfg['dil']), cfg['stride'], N, n, H, W, _p(gx),
                               _ptrs([gw[k] for k in range(4)]), _stream()))
    return {'gx': gx, 'gw': gw}


def run_eesp_fused(cfg, p, lib, check):
    N, n, H, W = cfg['shape']
    d = {k: _dev(p.get(k)) for k in ('z', 'gy', 'w4', 'scale', 'shift', 'alpha', 'mean', 'inv', 'c', 'pscale', 'pshift', 'palpha', 'pmean', 'pinv')}
    x = _dev(ec.fused_x(p))
    tail = cfg['tail']
    o = {'gx': _out((N, n, H, W)), 'gw': _acc((4, n, 3, 3), p.get('pre_gw'))}
    for name in ('gscale', 'gshift', 'galpha'):
        o[name] = _acc((4 * n,), p.get('pre_' + name))
        if tail:
            o['gp' + name[1:]] = _acc((n,), p.get('pre_gp' + name[1:]))
    dil = (ctypes.c_int32 * 4)(*cfg['dil'])
    assert lib.mspl_eesp_bwd_fused_fits(N, n, H, W, dil)
    check(lib.mspl_eesp_bwd_fused(_p(d['z']), _p(d['gy']), _p(x), _p(d['w4']), dil, _p(d['scale']), _p(d['shift']), _p(d['alpha']), _p(d['mean']),
                                  _p(d['inv']), N, n, H, W, _p(o['gx']), _ptrs([o['gw'][k] for k in range(4)]), _p(o['gscale']), _p(o['gshift']),
                                  _p(o['galpha']), _p(d['c']), _p(d['pscale']), _p(d['pshift']), _p(d['palpha']), _p(d['pmean']), _p(d['pinv']),
                                  _p(o.get('gpscale')), _p(o.get('gpshift')), _p(o.get('gpalpha')), _stream()))
    return o


def run_hff_bn(cfg, p, lib, check):
    N, n, HW = cfg['shape']
    d = {k: _dev(p.get(k)) for k in ('z', 'gy', 'scale', 'shift', 'alpha', 'mean', 'inv')}
    o = {'out': _out((4, N, n, HW)), 'gscale': _acc((4 * n,)), 'gshift': _acc((4 * n,)), 'galpha': _acc((4 * n,))}
    check(lib.mspl_hff_bn_prelu_suffix_bwd(_p(d['z']), _p(d['gy']), _p(d['scale']), _p(d['shift']), _p(d['alpha']), _p(d['mean']), _p(d['inv']),
                                           N, n, HW, _p(o['out']), _p(o['gscale']), _p(o['gshift']), _p(o['galpha']), _stream()))
    return o


def run_hff_sum(cfg, p, lib, check):
    N, n, HW = cfg['shape']
    g, out = _dev(p['g']), _out((4, N, n, HW))
    check(lib.mspl_hff_suffix_sum(_p(g), N, n, HW, _p(out), _stream()))
    return {'out': out}


def run_affine(cfg, p, lib, check):
    N, C, HW = cfg['shape']
    d = {k: _dev(p.get(k)) for k in ('c', 'pre_add', 'residual', 'gy', 'scale', 'shift', 'alpha', 'mean', 'inv')}
    o = {'gz': _out((N, C, HW)), 'gc': _out((N, C, HW)), 'gscale': _acc((C,)), 'gshift': _acc((C,)), 'galpha': _acc((C,))}
    head = [_p(d[k]) for k in ('c', 'pre_add', 'residual', 'gy', 'scale', 'shift', 'alpha')]
    tail = [N, C, HW] + [_p(o[k]) for k in ('gz', 'gc', 'gscale', 'gshift', 'galpha')] + [_stream()]
    if cfg['mean_inv']:
        check(lib.mspl_bn_prelu_bwd(*head, _p(d['mean']), _p(d['inv']), *tail))
    else:
        check(lib.mspl_affine_prelu_bwd(*head, *tail))
    return o


def run_down_tail(cfg, p, lib, check):
    N, nin, C, HW = cfg['shape']
    d = {k: _dev(p.get(k)) for k in ('a', 'b', 'reinf', 'gy', 'alpha')}
    o = {'ga': _out((N, nin, HW)), 'gb': _out((N, C - nin, HW)), 'galpha': _acc((C,))}
    if cfg['reinf']:
        o['greinf'] = _out((N, C, HW))
    check(lib.mspl_down_tail_bwd(_p(d['a']), _p(d['b']), _p(d['reinf']), _p(d['gy']), _p(d['alpha']), N, nin, C, HW, _p(o['ga']), _p(o['gb']),
                                 _p(o.get('greinf')), _p(o['galpha']), _stream()))
    return o


def run_wgrad_batch(cfg, p, lib, check):
    probs = cfg['problems']
    n = len(probs)
    gy, x = [_dev(p['gy%d' % i]) for i in range(n)], [_dev(p['x%d' % i]) for i in range(n)]
    gw = [_acc(None, p['pre_gw%d' % i]) for i in range(n)]
    rs = [_dev(p.get('rowscale%d' % i)) for i in range(n)]
    rsp = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in rs])
    ints = lambda k: (ctypes.c_int32 * n)(*[q[k] for q in probs])          # noqa: E731
    check(lib.mspl_conv1x1_wgrad_batch(_ptrs(gy), _ptrs(x), _ptrs(gw), rsp, ints(0), ints(1), ints(2), ints(3), ints(4), n, _stream()))
    return {'gw%d' % i: gw[i] for i in range(n)}


def run_dense(cfg, p, lib, check):
    from tests.test_gpu_dense_conv_grad import _dgrad, _wgrad
    N, Cin, Cout, H, W, k, dil = cfg['shape']
    x, w, gy = _dev(p['x']), _dev(p['w']), _dev(p['gy'])
    dw, db = _wgrad(gy, x, k, dil, cfg['split'])
    if Cout % 32:
        return {'dw': dw, 'db': db}
    return {'dw': dw, 'db': db, 'gx': _dgrad([gy], [w], [k], [dil], Cin), 'gx_acc': _dgrad([gy], [w], [k], [dil], Cin, out=_dev(p['pre_gx']))}


def run_sums(cfg, p, lib, check):
    planes, HW, n = cfg['shape']
    srcs = [_dev(p['src%d' % k]) for k in range(n)]
    pc, v = _dev(p['pc']), _dev(p['v'])
    o = {'sum_n': _out((planes, HW)), 'sum_n_planes': _out((planes, HW)), 'plane_dot': _out((planes,)), 'plane_sum': _out((planes,)),
         'broadcast': _out((planes, HW)), 'broadcast_acc': _dev(p['pre'])}
    check(lib.mspl_sum_n(_ptrs(srcs), n, planes * HW, _p(o['sum_n']), _stream()))
    check(lib.mspl_sum_n_planes(_ptrs(srcs), n, _p(pc), 0.5, planes, HW, _p(o['sum_n_planes']), _stream()))
    check(lib.mspl_plane_dot(_p(srcs[0]), _p(srcs[1]), planes, HW, _p(o['plane_dot']), _stream()))
    check(lib.mspl_plane_dot(_p(srcs[0]), None, planes, HW, _p(o['plane_sum']), _stream()))
    check(lib.mspl_plane_broadcast(_p(v), planes, HW, 0.5, 0, _p(o['broadcast']), _stream()))
    check(lib.mspl_plane_broadcast(_p(v), planes, HW, 0.5, 1, _p(o['broadcast_acc']), _stream()))
    return o


def run_pyr_merge(cfg, p, lib, check):
    from tests.test_gpu_pyramid_grad import run_pyr_merge as run
    return run(cfg['shape'], p, lib, check, pre=0.0)


RUN = {'conv_wgrad': run_conv_wgrad, 'conv_dgrad': run_conv_dgrad, 'eesp_dw': run_eesp_dw, 'eesp_fused': run_eesp_fused, 'hff_bn': run_hff_bn,
       'hff_sum': run_hff_sum, 'affine': run_affine, 'down_tail': run_down_tail, 'wgrad_batch': run_wgrad_batch, 'dense': run_dense,
       'sums': run_sums, 'pyr_merge': run_pyr_merge}


def _where(case, name, idx):
    """The band / chunk / image an element of an output with a pixel axis falls in, from the library's own plan."""
    cfg = case.cfg
    if case.op == 'eesp_fused' and name == 'gx':
        bands, rows = ec.fused_bands(cfg['shape'], cfg['dil'])
        return 'image %d channel %d band %d of %d (rows %d..%d), row %d' % (idx[0], idx[1], idx[2] // rows, bands, idx[2] // rows * rows,
                                                                            min(cfg['shape'][2], (idx[2] // rows + 1) * rows) - 1, idx[2])
    if case.op == 'pyr_merge' and name == 'gt':
        return 'branch %d image %d channel %d row %d (band %d) column %d (tile %d)' % (tuple(idx[:4]) + (idx[3] // 16, idx[4], idx[4] // 64))
    if case.op in ('hff_bn', 'hff_sum') and name == 'out':
        return 'branch %d image %d channel %d pixel %d of %d' % (tuple(idx) + (cfg['shape'][2],))
    return ''


def _plan_text(case):
    cfg = case.cfg
    if case.op == 'conv_wgrad':
        N, Cin, Cout, G, H, W, K, s = cfg['shape']
        form, parts, ngroups = ec.wgrad_plan(cfg['shape'], not cfg.get('misalign'))
        total = N * ec.conv_out(H, K, s) * ec.conv_out(W, K, s)
        return 'form %d, %d parts of the %d output pixels (%d per part, %d per image; %d 64-pixel groups)' % (
            form, parts, total, -(-total // parts), total // N, ngroups)
    if case.op == 'eesp_dw':
        return '%d weight-gradient chunks' % ec.dw_chunks(cfg['shape'], cfg['stride'])
    if case.op == 'eesp_fused':
        return '%d bands of %d rows' % ec.fused_bands(cfg['shape'], cfg['dil'])
    return ''


def _assert_equal(case, name, got, ref):
    g = got.detach().cpu().double()
    assert g.shape == ref.shape, '%s %s: shape %s, reference %s' % (case.id, name, tuple(g.shape), tuple(ref.shape))
    if torch.equal(g, ref):
        return
    bad = torch.nonzero(~(g == ref))              # NaN (never written) counts as different
    lines = ['%s %s: %d of %d elements differ from the float64 reference; %s' % (case.id, name, len(bad), ref.numel(), _plan_text(case))]
    for idx in bad[:8].tolist():
        t = tuple(idx)
        lines.append('  %s: got %r want %r (difference %r) %s' % (t, float(g[t]), float(ref[t]), float(g[t] - ref[t]), _where(case, name, t)))
    raise AssertionError('\n'.join(lines))


@pytest.mark.parametrize('cid', [c.id for c in ec.CASES])
def test_exact(cid):
    from mspl_amd._native import check, lib
    case = ec.BY_ID[cid]
    p, ref = ec.inputs(case), ec.reference64(cid)
    got = RUN[case.op](case.cfg, p, lib, check)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a device fault: nothing more is started on this GPU
        pytest.exit('%s: %s' % (cid, e), returncode=3)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for name in sorted(ref):
        _assert_equal(case, name, got[name], ref[name])
    again = RUN[case.op](case.cfg, p, lib, check)
    torch.cuda.synchronize()
    for name in sorted(ref):
        assert torch.equal(again[name], got[name]), '%s %s: a second call gives other bits' % (cid, name)
