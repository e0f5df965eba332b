"""Tensor-level wrappers of the C ABI (forward ops).

PyTorch is plumbing only here: it owns device memory (caching allocator) and the stream.  Every wrapper
checks device/dtype/contiguity on the host before a pointer reaches a kernel, allocates the output with
torch.empty, and launches on torch's current stream so the calls are capturable by torch.cuda.graph().
"""
import ctypes
import math

import torch

from . import _native as nat
from ._native import Epilogue, check, lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('mspl_amd: %s must be a CUDA (ROCm) tensor; there is no CPU path' % name)
    if t.dtype != torch.float32:
        raise RuntimeError('mspl_amd: %s must be float32, got %s' % (name, t.dtype))
    if not t.is_contiguous():
        t = t.contiguous()
    return t


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _vec(t, n, name):
    if t is None:
        return None
    t = _f32(t, name)
    if t.numel() != n:
        raise RuntimeError('mspl_amd: %s has %d elements, expected %d' % (name, t.numel(), n))
    return t


class Epi:
    """Python mirror of mspl_epilogue_t (see include/mspl_hip.h for the exact order of operations)."""
    __slots__ = ('scale', 'shift', 'alpha', 'pre_add', 'residual', 'reinf_r', 'reinf_w', 'gate', 'raw_out')

    def __init__(self, scale=None, shift=None, alpha=None, pre_add=None, residual=None, reinf_r=None,
                 reinf_w=None, gate=None, raw_out=None):
        self.scale, self.shift, self.alpha = scale, shift, alpha
        self.pre_add, self.residual = pre_add, residual
        self.reinf_r, self.reinf_w, self.gate = reinf_r, reinf_w, gate
        self.raw_out = raw_out          # convolutions only: a tensor of the destination's shape that also receives the bare result


# Launch-shape preference of the calls issued by this THREAD (mspl_epilogue_t.flags / MSPL_LAUNCH_*): per call, carried in every
# epilogue struct -- the library itself holds no mutable state (rounds 1-2 flipped a process-wide switch around every lane launch).
import threading
_LAUNCH = threading.local()


class launch_flags(object):
    """with launch_flags(throughput=True): every op issued by this thread asks for launch shapes that favour steady-state
    efficiency over the latency of a lone launch (PipelinedLabelPass captures its lanes like this).  Results never change."""

    def __init__(self, throughput=False, k2_stream=None):
        self.value = nat.LAUNCH_THROUGHPUT if throughput else 0
        if k2_stream is not None:       # False: never the streaming form of the stride-2 depthwise launch; True: whenever the shape allows
            self.value |= nat.LAUNCH_K2_STREAM_FORCE if k2_stream else nat.LAUNCH_K2_STREAM_OFF

    def __enter__(self):
        self.prev = getattr(_LAUNCH, 'flags', 0)
        _LAUNCH.flags = self.value
        return self

    def __exit__(self, *exc):
        _LAUNCH.flags = self.prev


def current_launch_flags():
    return getattr(_LAUNCH, 'flags', 0)


def _build(ep, out, coff, N, C, hw):
    """Validate an Epi against the destination tensor `out` (N, ctot, ...) and build the C struct."""
    ctot = out.shape[1]
    if coff < 0 or coff + C > ctot:
        raise RuntimeError('mspl_amd: channel slice [%d,%d) outside destination with %d channels' % (coff, coff + C, ctot))
    s = Epilogue()
    s.struct_size = ctypes.sizeof(Epilogue)
    s.flags = current_launch_flags()
    s.out_ctot, s.out_coff = ctot, coff
    keep = []
    if ep is not None:
        for f in ('scale', 'shift', 'alpha'):
            v = _vec(getattr(ep, f), ctot, f)
            keep.append(v)
            setattr(s, f, None if v is None else v.data_ptr())
        for f in ('pre_add', 'residual'):
            v = getattr(ep, f)
            if v is not None:
                v = _f32(v, f)
                if v.numel() != N * ctot * hw:
                    raise RuntimeError('mspl_amd: %s shape %s does not match destination %s' % (f, tuple(v.shape), tuple(out.shape)))
                keep.append(v)
                setattr(s, f, v.data_ptr())
        if ep.reinf_r is not None:
            r = _vec(ep.reinf_r, N * 3 * hw, 'reinf_r')
            w = _vec(ep.reinf_w, ctot * 3, 'reinf_w')
            keep += [r, w]
            s.reinf_r, s.reinf_w = r.data_ptr(), w.data_ptr()
        if ep.gate is not None:
            g = _vec(ep.gate, N * ctot, 'gate')
            keep.append(g)
            s.gate = g.data_ptr()
        if ep.raw_out is not None:
            r = ep.raw_out
            if not r.is_cuda or r.dtype != torch.float32 or not r.is_contiguous() or r.numel() != N * C * hw or coff != 0 or ctot != C:
                raise RuntimeError('mspl_amd: raw_out must be a contiguous float32 CUDA tensor of the (un-sliced) destination shape')
            keep.append(r)
            s.raw_out = r.data_ptr()
    return s, keep


def _dest(out, shape, like):
    if out is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32), 0
    dst, coff = out
    if (dst.shape[0],) + tuple(dst.shape[2:]) != (shape[0],) + tuple(shape[2:]) or not dst.is_contiguous() \
            or dst.dtype != torch.float32 or not dst.is_cuda:
        raise RuntimeError('mspl_amd: destination %s incompatible with result %s' % (tuple(dst.shape), tuple(shape)))
    return dst, coff


def eesp_dw_hff(x, w4, dil, stride, ep=None, out=None):
    """K2.  x (N,n,H,W), w4 (4,n,3,3) -> (N,4n,Ho,Wo); `out=(tensor, channel_offset)` writes a slice."""
    x, w4 = _f32(x, 'x'), _f32(w4, 'w4')
    N, n, H, W = x.shape
    if tuple(w4.shape) != (4, n, 3, 3):
        raise RuntimeError('mspl_amd: eesp_dw_hff weight %s, expected (4,%d,3,3)' % (tuple(w4.shape), n))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dst, coff = _dest(out, (N, 4 * n, Ho, Wo), x)
    s, keep = _build(ep, dst, coff, N, 4 * n, Ho * Wo)
    d = (ctypes.c_int32 * 4)(*[int(v) for v in dil])
    check(lib.mspl_eesp_dw_hff_fwd(_p(x), _p(w4), d, stride, N, n, H, W, ctypes.byref(s), _p(dst), _stream()))
    return dst


def eesp_proj_dw_hff_fits(shape, n, groups, dilations, stride):
    """True when K1 + K2 of an EESP block run as one launch for an input of `shape` (N,Cin,H,W)."""
    if stride != 1:
        return False
    N, Cin, H, W = [int(v) for v in shape]
    d = (ctypes.c_int32 * 4)(*[int(v) for v in dilations])
    return bool(lib.mspl_eesp_proj_dw_hff_fits(N, Cin, int(n), int(groups), H, W, d, current_launch_flags()))


def eesp_proj_dw_hff(x, wproj, pscale, pshift, palpha, w4, dilations, groups, ep=None, out=None):
    """K1 + K2 (stride 1): PReLU(BN(grouped 1x1(x))) -> four dilated depthwise 3x3 + HFF + cat + epilogue, one launch."""
    x = _f32(x, 'x')
    N, Cin, H, W = x.shape
    wproj = _f32(wproj, 'projection weight')
    n = wproj.shape[0]
    w4 = _vec(w4, 4 * n * 9, 'w')
    ps, pb, pa = _vec(pscale, n, 'pscale'), _vec(pshift, n, 'pshift'), _vec(palpha, n, 'palpha')
    dst, coff = _dest(out, (N, 4 * n, H, W), x)
    s, keep = _build(ep, dst, coff, N, 4 * n, H * W)
    d = (ctypes.c_int32 * 4)(*[int(v) for v in dilations])
    check(lib.mspl_eesp_proj_dw_hff_fwd(_p(x), _p(wproj), _p(ps), _p(pb), _p(pa), _p(w4), d, N, Cin, n, int(groups), H, W,
                                        ctypes.byref(s), _p(dst), _stream()))
    return dst


def eesp_dw_exp_fits(shape, dilations):
    """True when K2 + K3 of a stride-1 EESP block run as one launch for a reduced tensor of `shape` (N,n,H,W)."""
    N, n, H, W = [int(v) for v in shape]
    d = (ctypes.c_int32 * 4)(*[int(v) for v in dilations])
    return bool(lib.mspl_eesp_dw_exp_fits(N, n, H, W, d, current_launch_flags()))


def eesp_dw_exp_pack(w4, bscale, bshift, balpha, wexp, H, W, dilations):
    """The packed parameter block of mspl_eesp_dw_exp_fwd (depends on the weights only: cache it per weight version)."""
    w4 = _f32(w4, 'w4')
    n = w4.shape[1]
    if tuple(w4.shape) != (4, n, 3, 3):
        raise RuntimeError('mspl_amd: eesp_dw_exp weight %s, expected (4,%d,3,3)' % (tuple(w4.shape), n))
    bs, bb, ba = _vec(bscale, 4 * n, 'bscale'), _vec(bshift, 4 * n, 'bshift'), _vec(balpha, 4 * n, 'balpha')
    wexp = _vec(wexp, 4 * n * n, 'expansion weight')
    packed = torch.empty(int(lib.mspl_eesp_dw_exp_pack_floats(n)), device=w4.device, dtype=torch.float32)
    d = (ctypes.c_int32 * 4)(*[int(v) for v in dilations])
    check(lib.mspl_eesp_dw_exp_pack(_p(w4), _p(bs), _p(bb), _p(ba), _p(wexp), n, int(H), int(W), d, _p(packed), _stream()))
    return packed


def eesp_dw_exp_next_pack(w1):
    """The next block's proj_1x1 weight (n, n[, 1, 1]) in the operand order of mspl_eesp_dw_exp_next_fwd (cache it per weight version)."""
    w1 = _f32(w1, 'next projection weight')
    n = w1.shape[0]
    if w1.numel() != n * n:
        raise RuntimeError('mspl_amd: next projection weight %s, expected (%d,%d)' % (tuple(w1.shape), n, n))
    packed = torch.empty(int(lib.mspl_eesp_dw_exp_next_pack_floats(n)), device=w1.device, dtype=torch.float32)
    check(lib.mspl_eesp_dw_exp_next_pack(_p(w1), n, _p(packed), _stream()))
    return packed


def eesp_dw_exp(r, packed, dilations, ep, next_proj=None):
    """K2 + K3 of a stride-1 EESP block: r (N,n,H,W) -> (N,4n,H,W); ep carries conv_1x1_exp's folded BN, module_act's slope
    and the residual (the block's input).  next_proj = (packed weight, scale, shift, alpha) of the FOLLOWING block's proj_1x1: the
    launch then also returns that block's reduced tensor (N,n,H,W): (y, r_next)."""
    r = _f32(r, 'r')
    N, n, H, W = r.shape
    packed = _vec(packed, int(lib.mspl_eesp_dw_exp_pack_floats(n)), 'packed')
    dst = torch.empty((N, 4 * n, H, W), device=r.device, dtype=torch.float32)
    s, keep = _build(ep, dst, 0, N, 4 * n, H * W)
    d = (ctypes.c_int32 * 4)(*[int(v) for v in dilations])
    if next_proj is None:
        check(lib.mspl_eesp_dw_exp_fwd(_p(r), _p(packed), d, N, n, H, W, ctypes.byref(s), _p(dst), _stream()))
        return dst
    npk = _vec(next_proj[0], int(lib.mspl_eesp_dw_exp_next_pack_floats(n)), 'next_packed')
    ns, nb, na = _vec(next_proj[1], n, 'nscale'), _vec(next_proj[2], n, 'nshift'), _vec(next_proj[3], n, 'nalpha')
    rn = torch.empty((N, n, H, W), device=r.device, dtype=torch.float32)
    check(lib.mspl_eesp_dw_exp_next_fwd(_p(r), _p(packed), d, N, n, H, W, ctypes.byref(s), _p(dst), _p(npk), _p(ns), _p(nb), _p(na), _p(rn),
                                        _stream()))
    return dst, rn


def conv1x1(x, w, groups=1, ep=None, out=None):
    """K1/K3.  x (N,Cin,H,W), w (Cout,Cin/groups[,1,1])."""
    x, w = _f32(x, 'x'), _f32(w, 'w')
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    if w.numel() != Cout * (Cin // groups) or Cin % groups or Cout % groups:
        raise RuntimeError('mspl_amd: conv1x1 weight %s does not match Cin=%d groups=%d' % (tuple(w.shape), Cin, groups))
    dst, coff = _dest(out, (N, Cout, H, W), x)
    s, keep = _build(ep, dst, coff, N, Cout, H * W)
    check(lib.mspl_conv1x1_fwd(_p(x), _p(w), N, Cin, Cout, groups, H * W, ctypes.byref(s), _p(dst), _stream()))
    return dst


CONV1X1_FORMS = {nat.PW_FORM_THIN: 'thin', nat.PW_FORM_SMALL_K: 'small_k', nat.PW_FORM_SPLIT_K: 'split_k',
                 nat.PW_FORM_TILE_PIPELINED: 'pipe', nat.PW_FORM_REGISTER_WEIGHTS: 'areg', nat.PW_FORM_LDS_RING: 'ring'}
CONV1X1_TERMS = {'scale': nat.PW_TERM_SCALE, 'shift': nat.PW_TERM_SHIFT, 'alpha': nat.PW_TERM_ALPHA, 'pre_add': nat.PW_TERM_PRE_ADD,
                 'residual': nat.PW_TERM_RESIDUAL, 'reinf': nat.PW_TERM_REINF, 'gate': nat.PW_TERM_GATE, 'raw_out': nat.PW_TERM_RAW_OUT}
_PW_PLAN_FIELDS = ('MT', 'MTILES', 'NSUB', 'CH', 'KS', 'TILES', 'NG', 'MB', 'AR', 'WM', 'TPW', 'RING', 'VECW', 'LDS_BYTES', 'GRID_X',
                   'GRID_Y', 'GRID_Z')


def conv1x1_plan(shape, terms=(), ctot=0, x_align=16, w_align=16, out_align=16, operand_align=16, side_align=16):
    """The kernel form conv1x1 takes (mspl_conv1x1_fwd_plan, the launcher's own host function; no device call).
    shape: (N, Cin, Cout, groups, HW); terms: names of the epilogue operands present (CONV1X1_TERMS); ctot: channels of the
    destination (0: Cout); *_align: the power of two (<= 16) dividing the address of x / w / out, the per-pixel operands
    (pre_add, residual, reinf_r) and raw_out / gate.  -> dict form ('thin' / 'small_k' / 'split_k' / 'pipe' / 'areg' / 'ring') and
    the integers mt / mtiles / nsub / ch / ks / tiles / ng / mb / ar / wm / tpw / ring / vecw / lds_bytes / grid_x / grid_y / grid_z,
    0 where they do not apply to the form.  A shape the launcher refuses raises what the launcher raises."""
    out = (ctypes.c_int32 * nat.PW_PLAN_LEN)()
    mask = 0
    for t in terms:
        mask |= CONV1X1_TERMS[t]
    check(lib.mspl_conv1x1_fwd_plan(*[int(v) for v in shape], int(ctot), mask, int(x_align), int(w_align), int(out_align),
                                    int(operand_align), int(side_align), out))
    plan = {n.lower(): int(out[getattr(nat, 'PW_PLAN_' + n)]) for n in _PW_PLAN_FIELDS}
    plan['form'] = CONV1X1_FORMS[int(out[nat.PW_PLAN_FORM])]
    return plan


def conv3x3(x, w, groups=1, stride=1, shuffle_groups=0, ep=None, out=None):
    x, w = _f32(x, 'x'), _f32(w, 'w')
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    if tuple(w.shape[2:]) != (3, 3) or Cin % groups or Cout % groups or w.shape[1] != Cin // groups:
        raise RuntimeError('mspl_amd: conv3x3 weight %s does not match Cin=%d groups=%d' % (tuple(w.shape), Cin, groups))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dst, coff = _dest(out, (N, Cout, Ho, Wo), x)
    s, keep = _build(ep, dst, coff, N, Cout, Ho * Wo)
    check(lib.mspl_conv3x3_fwd(_p(x), _p(w), N, Cin, Cout, groups, H, W, stride, shuffle_groups, ctypes.byref(s),
                               _p(dst), _stream()))
    return dst


def pack_dense_weight(w):
    """(Cout, Cin, k, k) conv weight -> the tap-major (k*k, Cout, Cin) layout dense_conv reads (a permute copy)."""
    w = _f32(w, 'w')
    Cout, Cin, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(kh * kw, Cout, Cin).contiguous()


def dense_conv(x, w_packed, ksize, dilation=1, ep=None, out=None):
    """K13.  Dense 1x1 / dilated 3x3 convolution (padding = dilation) on the matrix cores; w_packed from pack_dense_weight."""
    x, w_packed = _f32(x, 'x'), _f32(w_packed, 'w_packed')
    N, Cin, H, W = x.shape
    taps = ksize * ksize
    if w_packed.dim() != 3 or w_packed.shape[0] != taps or w_packed.shape[2] != Cin:
        raise RuntimeError('mspl_amd: dense_conv packed weight %s does not match k=%d Cin=%d' % (tuple(w_packed.shape), ksize, Cin))
    Cout = w_packed.shape[1]
    dst, coff = _dest(out, (N, Cout, H, W), x)
    s, keep = _build(ep, dst, coff, N, Cout, H * W)
    check(lib.mspl_dense_conv_fwd(_p(x), _p(w_packed), N, Cin, Cout, H, W, ksize, int(dilation), ctypes.byref(s), _p(dst),
                                  _stream()))
    return dst


def pack_dense_weight_split(w, planes):
    """(Cout, Cin, k, k) fp32 conv weight -> (planes, k*k, Cout, Cin) bfloat16: the weight split into bf16 planes by the rule of
    mspl_dense_conv_split_fwd (plane_i = bf16_rne(r_i), r_{i+1} = r_i - float(plane_i), r_0 = w), each plane in the tap-major
    layout of pack_dense_weight.  Plain torch ops: works on CPU tensors too."""
    if not isinstance(w, torch.Tensor) or w.dim() != 4 or w.shape[2] != w.shape[3] or w.dtype != torch.float32:
        raise RuntimeError('mspl_amd: pack_dense_weight_split takes a float32 (Cout, Cin, k, k) weight')
    if planes not in (2, 3):
        raise RuntimeError('mspl_amd: pack_dense_weight_split: %r planes (2 or 3)' % (planes,))
    Cout, Cin, k, _ = w.shape
    r = w.detach().permute(2, 3, 0, 1).reshape(k * k, Cout, Cin)
    out = torch.empty((planes, k * k, Cout, Cin), device=w.device, dtype=torch.bfloat16)
    for p in range(planes):
        out[p] = r.to(torch.bfloat16)              # round to nearest even
        r = r - out[p].to(torch.float32)           # exact in fp32
    return out


def dense_conv_split_fits(Cin, Cout, ksize, planes):
    """True when mspl_dense_conv_split_fwd takes this convolution (never depends on N, H, W)."""
    return bool(lib.mspl_dense_conv_split_fits(int(Cin), int(Cout), int(ksize), int(planes)))


def dense_conv_split(x, w_split, ksize, dilation=1, ep=None, out=None):
    """K13 in split-bf16 arithmetic (the opt-in matrix mode of the ASPP heads): w_split from pack_dense_weight_split, whose plane
    count (2: bf16x3, 3: bf16x6) selects the mode.  Shapes, epilogue and `out=(tensor, coff)` as dense_conv."""
    x = _f32(x, 'x')
    if not isinstance(w_split, torch.Tensor) or not w_split.is_cuda or w_split.dtype != torch.bfloat16 or not w_split.is_contiguous():
        raise RuntimeError('mspl_amd: dense_conv_split weights must be a contiguous CUDA (ROCm) bfloat16 tensor from pack_dense_weight_split')
    N, Cin, H, W = x.shape
    taps = ksize * ksize
    if w_split.dim() != 4 or w_split.shape[1] != taps or w_split.shape[3] != Cin:
        raise RuntimeError('mspl_amd: dense_conv_split weight %s does not match k=%d Cin=%d' % (tuple(w_split.shape), ksize, Cin))
    planes, Cout = w_split.shape[0], w_split.shape[2]
    dst, coff = _dest(out, (N, Cout, H, W), x)
    s, keep = _build(ep, dst, coff, N, Cout, H * W)
    check(lib.mspl_dense_conv_split_fwd(_p(x), _p(w_split), N, Cin, Cout, H, W, ksize, int(dilation), planes, ctypes.byref(s), _p(dst),
                                        _stream()))
    return dst


def pack_dense_weight_dgrad(w):
    """(Cout, Cin, k, k) conv weight -> the (k*k, Cin, Cout) weights of its data gradient as a dense_conv of gy (stride 1,
    padding = dilation): transposed and tap-reversed, Wt[t][ci][co] = Wp[k*k - 1 - t][co][ci] (a permute copy)."""
    if w.dim() != 4 or w.shape[2] != w.shape[3] or w.dtype != torch.float32:
        raise RuntimeError('mspl_amd: pack_dense_weight_dgrad takes a float32 (Cout, Cin, k, k) weight, got %s %s' % (tuple(w.shape), w.dtype))
    Cout, Cin, k, _ = w.shape
    return w.flip(2, 3).permute(2, 3, 1, 0).reshape(k * k, Cin, Cout).contiguous()


def unpack_dense_weight(wp, ksize):
    """The inverse permute of pack_dense_weight, as a VIEW: (k*k, Cout, Cin) -> (Cout, Cin, k, k)."""
    taps, Cout, Cin = wp.shape
    return wp.view(ksize, ksize, Cout, Cin).permute(2, 3, 0, 1)


def dense_conv_wgrad(gy, x, ksize, dilation=1, want_bias=True, split=0, out_bias=None):
    """Weight and bias gradient of dense_conv: gy (N,Cout,H,W), x (N,Cin,H,W) -> (dw in the packed (k*k, Cout, Cin) layout, db (Cout,)
    or None).  split: pixel ranges (0: the library chooses); the workspace of a split comes from torch's allocator."""
    gy, x = _f32(gy, 'gy'), _f32(x, 'x')
    N, Cin, H, W = x.shape
    Cout = gy.shape[1]
    if (gy.shape[0],) + tuple(gy.shape[2:]) != (N, H, W):
        raise RuntimeError('mspl_amd: dense_conv_wgrad gy %s does not match x %s' % (tuple(gy.shape), tuple(x.shape)))
    args = (N, Cin, Cout, H, W, int(ksize), int(dilation), int(split))
    nbytes = int(lib.mspl_dense_conv_wgrad_workspace_bytes(*args))
    if nbytes < 0:
        check(nbytes)
    ws = torch.empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32) if nbytes else None
    dw = torch.empty((ksize * ksize, Cout, Cin), device=x.device, dtype=torch.float32)
    db = None
    if want_bias:
        db = out_bias if out_bias is not None else torch.empty(Cout, device=x.device, dtype=torch.float32)
    check(lib.mspl_dense_conv_wgrad(_p(gy), _p(x), *args, _p(ws), nbytes, _p(dw), _p(db), _stream()))
    return dw, db


def dense_conv_dgrad(gys, wts, ksizes, dilations, out=None):
    """Data gradient of 1..4 dense convolutions of one input in ONE launch: gx = sum_b dense_conv(gys[b], wts[b]) with wts[b] from
    pack_dense_weight_dgrad.  out: an existing (N,Cx,H,W) tensor to ADD to (else a fresh one is written)."""
    gys = [_f32(g, 'gy') for g in gys]
    wts = [_f32(w, 'wt_packed') for w in wts]
    n = len(gys)
    N, Cg, H, W = gys[0].shape
    Cx = wts[0].shape[1]
    for g, w, k in zip(gys, wts, ksizes):
        if tuple(g.shape) != (N, Cg, H, W) or tuple(w.shape) != (k * k, Cx, Cg):
            raise RuntimeError('mspl_amd: dense_conv_dgrad gy %s / weights %s do not match (N,%d,%d,%d) / (k*k,%d,%d)'
                               % (tuple(g.shape), tuple(w.shape), Cg, H, W, Cx, Cg))
    if out is None:
        gx = torch.empty((N, Cx, H, W), device=gys[0].device, dtype=torch.float32)
    else:
        gx, _ = _dest((out, 0), (N, Cx, H, W), gys[0])
        if gx.shape[1] != Cx:
            raise RuntimeError('mspl_amd: dense_conv_dgrad destination %s, expected %d channels' % (tuple(gx.shape), Cx))
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])              # noqa: E731
    ints = lambda vs: (ctypes.c_int32 * n)(*[int(v) for v in vs])                    # noqa: E731
    check(lib.mspl_dense_conv_dgrad(arr(gys), arr(wts), ints(ksizes), ints(dilations), n, N, Cg, Cx, H, W, int(out is not None), _p(gx),
                                    _stream()))
    return gx


def avgpool3x3s2(x, ep=None, out=None, plane_sums=False):
    """3x3 / stride 2 / pad 1 average pool (+ epilogue).  plane_sums=True: returns (pooled, partial sums (N*C, nblk) of x per
    plane) -- for a gate over the same tensor (gate_from_sums) without reading it again."""
    x = _f32(x, 'x')
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dst, coff = _dest(out, (N, C, Ho, Wo), x)
    s, keep = _build(ep, dst, coff, N, C, Ho * Wo)
    if not plane_sums:
        check(lib.mspl_avgpool3x3s2_fwd(_p(x), N, C, H, W, ctypes.byref(s), _p(dst), _stream()))
        return dst
    nblk = lib.mspl_avgpool3x3s2_psum_blocks(H, W)
    if nblk <= 0:
        check(nblk)
    sums = torch.empty((N * C, nblk), device=x.device, dtype=torch.float32)
    check(lib.mspl_avgpool3x3s2_psum_fwd(_p(x), N, C, H, W, ctypes.byref(s), _p(dst), _p(sums), _stream()))
    return dst, sums


def down_head_fits(shape, n, groups):
    """True when a DownSampler's projection and pool run as one launch for an input of `shape` (N,nin,H,W)."""
    N, nin, H, W = [int(v) for v in shape]
    return bool(lib.mspl_down_head_fits(N, nin, int(n), int(groups), H, W, current_launch_flags()))


def down_head(x, wproj, pscale, pshift, palpha, groups, ep, out):
    """Head of a DownSampler block from one read of x (N,nin,H,W): returns (r, sums) with r (N,n,H,W) = PReLU(BN(grouped
    1x1(x))) and sums (N*nin, nblk) the partial plane sums of x; channels [0, nin) of `out` (N,nout,H/2,W/2) receive the 3x3 / s2
    average pool through ep (scale, shift, alpha over all nout channels, optionally the reinforcement)."""
    x, wproj = _f32(x, 'x'), _f32(wproj, 'projection weight')
    N, nin, H, W = x.shape
    n = wproj.shape[0]
    if wproj.numel() != n * (nin // groups) or nin % groups or n % groups:
        raise RuntimeError('mspl_amd: down_head weight %s does not match nin=%d groups=%d' % (tuple(wproj.shape), nin, groups))
    ps, pb, pa = _vec(pscale, n, 'pscale'), _vec(pshift, n, 'pshift'), _vec(palpha, n, 'palpha')
    dst, coff = _dest((out, 0), (N, nin, H // 2, W // 2), x)
    s, keep = _build(ep, dst, coff, N, nin, (H // 2) * (W // 2))
    nblk = lib.mspl_down_head_psum_blocks(H, W)
    if nblk <= 0:
        check(nblk)
    r = torch.empty((N, n, H, W), device=x.device, dtype=torch.float32)
    sums = torch.empty((N * nin, nblk), device=x.device, dtype=torch.float32)
    check(lib.mspl_down_head_fwd(_p(x), _p(wproj), _p(ps), _p(pb), _p(pa), N, nin, n, int(groups), H, W, ctypes.byref(s), _p(r),
                                 _p(dst), _p(sums), _stream()))
    return r, sums


def gate_from_sums(plane_sums, w, hw):
    """sigmoid(W . sum_j plane_sums[:, j] / hw) -> (N, Cout): gap_gate without re-reading the tensor."""
    w = _f32(w, 'w')
    Cout = w.shape[0]
    Cin = w.numel() // Cout
    planes, nblk = plane_sums.shape
    N = planes // Cin
    if planes != N * Cin or plane_sums.dtype != torch.float32 or not plane_sums.is_contiguous():
        raise RuntimeError('mspl_amd: gate_from_sums: sums %s do not match Cin=%d' % (tuple(plane_sums.shape), Cin))
    gate = torch.empty((N, Cout), device=w.device, dtype=torch.float32)
    check(lib.mspl_gate_from_sums_fwd(_p(plane_sums), _p(w), N, Cin, Cout, nblk, int(hw), _p(gate), _stream()))
    return gate


def decoder_merge_shape_ok(Cin, Cout, P, H, W):
    """The shape rules of mspl_decoder_merge_fwd, for callers that plan their streams before the bottom-up tensor exists (the
    library has the last word: decoder_merge returns None for what it does not take)."""
    groups = math.gcd(Cin, Cout)
    cg, cob = Cin // groups, Cout // groups
    if H % 2 or W % 2 or H < 2 or W < 2 or P not in (2, 6, 10, 16) or Cout > 1024:
        return False
    return (cg, cob) in ((1, 1), (8, 3)) or ((cg, cob) == (4, 1) and groups >= 16 and W % 4 == 0 and 16 <= W <= 256 and H >= 4)


def decoder_merge(enc, bu, w3, e_epi, gate, b_epi, wp, p_epi):
    """Head of a decoder stage in one launch: PReLU(BN(wp . PReLU(BN(gate * PReLU(BN(grouped3x3(enc))) + upsample2(bu))))).
    enc (N,Cin,H,W), bu (N,Cout,H/2,W/2), w3 (Cout,Cin/gcd,3,3), gate (N,Cout), wp (P,Cout[,1,1]); e_epi / b_epi / p_epi: (scale,
    shift, alpha) of the expansion, of bu_br and of the projection.  Returns (N,P,H,W), or None when the shape is not a fused one
    (mspl_decoder_merge_fwd: MSPL_ERR_UNSUPPORTED, nothing launched): the caller then runs conv3x3, bilinear and conv1x1."""
    enc, bu, w3, wp = _f32(enc, 'enc'), _f32(bu, 'bu'), _f32(w3, 'w3'), _f32(wp, 'wp')
    N, Cin, H, W = enc.shape
    Cout, P = w3.shape[0], wp.shape[0]
    if tuple(bu.shape) != (N, Cout, H // 2, W // 2) or H % 2 or W % 2:
        return None
    groups = math.gcd(Cin, Cout)
    if tuple(w3.shape) != (Cout, Cin // groups, 3, 3) or wp.numel() != P * Cout:
        raise RuntimeError('mspl_amd: decoder_merge weights %s / %s do not match Cin=%d Cout=%d'
                           % (tuple(w3.shape), tuple(wp.shape), Cin, Cout))
    gate = _vec(gate, N * Cout, 'gate')
    es, eb, ea = [_vec(t, Cout, 'expansion epilogue') for t in e_epi]
    bs, bb, ba = [_vec(t, Cout, 'bu_br epilogue') for t in b_epi]
    ps, pb, pa = [_vec(t, P, 'projection epilogue') for t in p_epi]
    if any(t is None for t in (es, eb, ea, bs, bb, ba, ps, pb, pa)):
        return None
    dst = torch.empty((N, P, H, W), device=enc.device, dtype=torch.float32)
    rc = lib.mspl_decoder_merge_fwd(_p(enc), _p(bu), _p(w3), _p(es), _p(eb), _p(ea), _p(gate), _p(bs), _p(bb), _p(ba), _p(wp),
                                    _p(ps), _p(pb), _p(pa), N, Cin, Cout, P, H, W, _p(dst), _stream())
    if rc == nat.ERR_UNSUPPORTED:
        return None
    check(rc)
    return dst


def bilinear(x, size, ep=None, out=None, align_corners=True):
    """Bilinear resize to size=(Ho,Wo); align_corners=True is the ESPNet decoders' rule, False F.interpolate's default."""
    x = _f32(x, 'x')
    N, C, H, W = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    dst, coff = _dest(out, (N, C, Ho, Wo), x)
    s, keep = _build(ep, dst, coff, N, C, Ho * Wo)
    check(lib.mspl_bilinear_fwd(_p(x), N, C, H, W, Ho, Wo, 1 if align_corners else 0, ctypes.byref(s), _p(dst), _stream()))
    return dst


def adaptive_avgpool(x, size, ep=None, out=None):
    x = _f32(x, 'x')
    N, C, H, W = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    dst, coff = _dest(out, (N, C, Ho, Wo), x)
    s, keep = _build(ep, dst, coff, N, C, Ho * Wo)
    check(lib.mspl_adaptive_avgpool_fwd(_p(x), N, C, H, W, Ho, Wo, ctypes.byref(s), _p(dst), _stream()))
    return dst


def pointwise(x, ep, out=None):
    """Apply the epilogue elementwise (BatchNorm+PReLU blocks)."""
    x = _f32(x, 'x')
    N, C = x.shape[:2]
    hw = x[0, 0].numel()
    dst = torch.empty_like(x) if out is None else out
    s, keep = _build(ep, dst, 0, N, C, hw)
    check(lib.mspl_pointwise_fwd(_p(x), N, C, hw, ctypes.byref(s), _p(dst), _stream()))
    return dst


def pyrpool_merge(zcat, scale, shift, alpha, merge_w, out=None):
    """merge_layer.0's fold + PReLU, Shuffle(groups=nb) and merge_layer.2's grouped 3x3 over kept branch values zcat (N, nb*P, h, w);
    merge_w (P, nb, 3, 3).  Returns the bare convolution result (N, P, h, w)."""
    zcat, merge_w = _f32(zcat, 'zcat'), _f32(merge_w, 'merge_w')
    N, C, h, w = zcat.shape
    P, nb = merge_w.shape[:2]
    if C != P * nb or tuple(merge_w.shape[2:]) != (3, 3) or any(t.numel() != C for t in (scale, shift, alpha)):
        raise RuntimeError('mspl_amd: pyrpool_merge operands do not match: zcat %s merge_w %s' % (tuple(zcat.shape), tuple(merge_w.shape)))
    dst = torch.empty((N, P, h, w), device=zcat.device, dtype=torch.float32) if out is None else out
    check(lib.mspl_pyrpool_merge_fwd(_p(zcat), N, P, h, w, nb, _p(_f32(scale, 'scale')), _p(_f32(shift, 'shift')), _p(_f32(alpha, 'alpha')),
                                     _p(merge_w), _p(dst), _stream()))
    return dst


def gap_gate(x, w):
    """sigmoid(W . mean_hw(x)) -> (N, Cout)."""
    x, w = _f32(x, 'x'), _f32(w, 'w')
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    if w.numel() != Cout * Cin:
        raise RuntimeError('mspl_amd: gap_gate weight %s does not match Cin=%d' % (tuple(w.shape), Cin))
    ws = torch.empty((N, Cin), device=x.device, dtype=torch.float32)
    gate = torch.empty((N, Cout), device=x.device, dtype=torch.float32)
    check(lib.mspl_gap_gate_fwd(_p(x), _p(w), N, Cin, Cout, H * W, _p(ws), _p(gate), _stream()))
    return gate


def fusion_gate(z, rgb, depth):
    """FusionGate blend (nn_layers/fusion_gate.py:36-44): sigmoid(z)-weighted mix, or rgb + depth when z is None."""
    rgb, depth = _f32(rgb, 'rgb'), _f32(depth, 'depth')
    if rgb.shape != depth.shape or (z is not None and z.shape != rgb.shape):
        raise RuntimeError('mspl_amd: fusion_gate operands differ in shape: %s %s %s'
                           % (tuple(rgb.shape), tuple(depth.shape), None if z is None else tuple(z.shape)))
    out = torch.empty_like(rgb)
    check(lib.mspl_fusion_gate_fwd(None if z is None else _p(_f32(z, 'z')), _p(rgb), _p(depth), rgb.numel(), _p(out),
                                   _stream()))
    return out


def fusion_gate_conv_fits(N, C, HW):
    """True for the shapes mspl_fusion_gate_conv_fwd / _bwd_weight serve (the library's own predicate)."""
    return bool(lib.mspl_fusion_gate_conv_fits(int(N), int(C), int(HW)))


def fusion_gate_conv_plan(N, C, HW):
    """What mspl_fusion_gate_conv_fwd launches for a shape (mspl_fusion_gate_conv_plan, the launcher's own host function; no device
    call) -> dict form / rows / pixels / wave_pixels / lds_bytes / grid_x, or None for a shape it declines."""
    out = (ctypes.c_int32 * nat.FGC_PLAN_LEN)()
    rc = lib.mspl_fusion_gate_conv_plan(int(N), int(C), int(HW), out)
    if rc == nat.ERR_UNSUPPORTED:
        return None
    check(rc)
    return {n.lower(): int(out[getattr(nat, 'FGC_PLAN_' + n)]) for n in ('FORM', 'ROWS', 'PIXELS', 'WAVE_PIXELS', 'LDS_BYTES', 'GRID_X')}


def fusion_gate_conv_bwd_weight_plan(N, C, HW):
    """-> dict form / parts / ngroups of mspl_fusion_gate_conv_bwd_weight (wave s of a tile pair takes the 64-pixel groups s, s + parts,
    ... of the ngroups groups of the flattened (image, pixel group) range), or None for a shape it declines."""
    form, parts, ngroups = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.mspl_fusion_gate_conv_bwd_weight_plan(int(N), int(C), int(HW), ctypes.byref(form), ctypes.byref(parts), ctypes.byref(ngroups))
    if rc == nat.ERR_UNSUPPORTED:
        return None
    check(rc)
    return {'form': form.value, 'parts': parts.value, 'ngroups': ngroups.value}


def fusion_gate_conv(rgb, depth, w, keep_z=False):
    """The trainable FusionGate in one launch: out = rgb*g + depth*(1-g), g = sigmoid(w[:, :C] . rgb + w[:, C:] . depth); w (C, 2C[,1,1])
    as the module stores it.  Returns out -- (out, z) with keep_z, z the pre-sigmoid tensor the backward needs -- or None when the
    library declines the shape (MSPL_ERR_UNSUPPORTED, nothing launched): the caller then runs conv1x1 twice and fusion_gate."""
    rgb, depth, w = _f32(rgb, 'rgb'), _f32(depth, 'depth'), _f32(w, 'w')
    if rgb.shape != depth.shape or rgb.dim() != 4:
        raise RuntimeError('mspl_amd: fusion_gate_conv operands differ in shape: %s %s' % (tuple(rgb.shape), tuple(depth.shape)))
    N, C = rgb.shape[:2]
    HW = rgb.shape[2] * rgb.shape[3]
    if w.numel() != 2 * C * C or w.shape[0] != C:
        raise RuntimeError('mspl_amd: fusion_gate_conv weight %s does not match C=%d' % (tuple(w.shape), C))
    if not fusion_gate_conv_fits(N, C, HW):
        return None
    out = torch.empty_like(rgb)
    z = torch.empty_like(rgb) if keep_z else None
    rc = lib.mspl_fusion_gate_conv_fwd(_p(rgb), _p(depth), _p(w), N, C, HW, None if z is None else _p(z), _p(out), _stream())
    if rc == nat.ERR_UNSUPPORTED:
        return None
    check(rc)
    return (out, z) if keep_z else out


def pyr_down_prep_fits(shape, sizes):
    """True when pyr_down_prep can stage a row band of an (N,P,h,w) map with these branch sizes in LDS
    (else: adaptive_avgpool + conv3x3 per branch)."""
    nb = len(sizes)
    N, P, h, w = [int(v) for v in shape]
    if nb < 1 or nb > 4 or any(int(s[0]) > h or int(s[1]) > w for s in sizes):
        return False
    hs = (ctypes.c_int32 * nb)(*[int(s[0]) for s in sizes])
    ws = (ctypes.c_int32 * nb)(*[int(s[1]) for s in sizes])
    return lib.mspl_pyr_down_prep_lds_bytes(N, P, h, w, nb, hs, ws) > 0


def pyr_down_prep(x, sizes, stage_ws, keep_pooled=False):
    """K6 prologue: [dw3x3(adaptive_avg_pool2d(x, size_i)) for each low-resolution branch] in one launch.  keep_pooled=True (the
    training forward): returns (those maps, the pooled maps themselves)."""
    x = _f32(x, 'x')
    N, P, h, w = x.shape
    nb = len(sizes)
    hs = (ctypes.c_int32 * nb)(*[int(s[0]) for s in sizes])
    ws = (ctypes.c_int32 * nb)(*[int(s[1]) for s in sizes])
    sw, op, pp = (ctypes.c_void_p * nb)(), (ctypes.c_void_p * nb)(), (ctypes.c_void_p * nb)()
    outs, pools, keep = [], [], []
    for i in range(nb):
        t = _f32(stage_ws[i], 'stage weight')
        if t.numel() != P * 9:
            raise RuntimeError('mspl_amd: pyramid stage weight %s, expected (%d,1,3,3)' % (tuple(t.shape), P))
        keep.append(t)
        sw[i] = t.data_ptr()
        o = torch.empty((N, P, int(sizes[i][0]), int(sizes[i][1])), device=x.device, dtype=torch.float32)
        outs.append(o)
        op[i] = o.data_ptr()
        if keep_pooled:
            pools.append(torch.empty_like(o))
            pp[i] = pools[-1].data_ptr()
    if keep_pooled:
        check(lib.mspl_pyr_down_prep_train_fwd(_p(x), N, P, h, w, nb, hs, ws, sw, op, pp, _stream()))
        return outs, pools
    check(lib.mspl_pyr_down_prep_fwd(_p(x), N, P, h, w, nb, hs, ws, sw, op, _stream()))
    return outs


def pyrpool_stream_plan(shape, sizes):
    """What the register-streaming form of K6 decides for an (N,P,h,w) map with these branch sizes (mspl_pyrpool_stream_plan, the
    launcher's own host function): a dict taken / t0 / t1 / pxl / ncb / cbw / seg / nseg / waves / seg_inkernel / nseg_inkernel /
    waves_inkernel, every value 0 when the shapes are left to the other forms."""
    N, P, h, w = [int(v) for v in shape]
    nb = len(sizes)
    hs = (ctypes.c_int32 * nb)(*[int(s[0]) for s in sizes])
    ws = (ctypes.c_int32 * nb)(*[int(s[1]) for s in sizes])
    out = (ctypes.c_int32 * nat.PYR_STREAM_PLAN_LEN)()
    check(lib.mspl_pyrpool_stream_plan(N, P, h, w, nb, hs, ws, out))
    names = ('TAKEN', 'T0', 'T1', 'PXL', 'NCB', 'CBW', 'SEG', 'NSEG', 'WAVES', 'SEG_INKERNEL', 'NSEG_INKERNEL', 'WAVES_INKERNEL')
    return {n.lower(): int(out[getattr(nat, 'PYR_STREAM_PLAN_' + n)]) for n in names}


def pyr_stream_tables(h, w, sizes, device):
    """The geometry tables of K6's streaming form for an h x w map with these branch sizes (a float32 tensor for pyrpool_fused's
    `tables`), or None when that form does not cover the geometry.  One small launch on the current stream."""
    nb = len(sizes)
    hs = (ctypes.c_int32 * nb)(*[int(s[0]) for s in sizes])
    ws = (ctypes.c_int32 * nb)(*[int(s[1]) for s in sizes])
    nbytes = int(lib.mspl_pyr_stream_tables_bytes(int(h), int(w), nb, hs, ws))
    if nbytes <= 0:
        return None
    tab = torch.empty(nbytes // 4, device=device, dtype=torch.float32)
    check(lib.mspl_pyr_stream_tables_build(int(h), int(w), nb, hs, ws, _p(tab), nbytes, _stream()))
    return tab


def pyrpool_fused(x, sizes, stage_ws, down_es, br_scale, br_shift, br_alpha, merge_w, ep=None, out=None, tables=None):
    """K6.  x (N,P,h,w); sizes: [(hs,ws)] per branch; stage_ws / down_es: per-branch tensors or None.  tables: what
    pyr_stream_tables built for this geometry (same output bits, less work per launch), or None."""
    x = _f32(x, 'x')
    N, P, h, w = x.shape
    nb = len(sizes)
    merge_w = _f32(merge_w, 'merge_w')
    if tuple(merge_w.shape) != (P, nb, 3, 3):
        raise RuntimeError('mspl_amd: pyrpool merge weight %s, expected (%d,%d,3,3)' % (tuple(merge_w.shape), P, nb))
    hs = (ctypes.c_int32 * nb)(*[int(s[0]) for s in sizes])
    ws = (ctypes.c_int32 * nb)(*[int(s[1]) for s in sizes])
    keep = []
    sw, de = (ctypes.c_void_p * nb)(), (ctypes.c_void_p * nb)()
    for i in range(nb):
        if stage_ws[i] is not None:
            t = _f32(stage_ws[i], 'stage weight')
            if t.numel() != P * 9:
                raise RuntimeError('mspl_amd: pyrpool stage weight %s, expected (%d,1,3,3)' % (tuple(t.shape), P))
            keep.append(t)
            sw[i] = t.data_ptr()
        if down_es[i] is not None:
            t = _f32(down_es[i], 'down map')
            if tuple(t.shape) != (N, P, int(sizes[i][0]), int(sizes[i][1])):
                raise RuntimeError('mspl_amd: pyrpool low-res map %s does not match branch size %s' % (tuple(t.shape), sizes[i]))
            keep.append(t)
            de[i] = t.data_ptr()
    bs, bh, ba = _vec(br_scale, nb * P, 'br_scale'), _vec(br_shift, nb * P, 'br_shift'), _vec(br_alpha, nb * P, 'br_alpha')
    dst, coff = _dest(out, (N, P, h, w), x)
    s, k2 = _build(ep, dst, coff, N, P, h * w)
    if tables is not None and not (s.pre_add or s.residual or s.reinf_r or s.gate or s.raw_out):   # (the streaming form's epilogue)
        check(lib.mspl_pyrpool_fused_tab_fwd(_p(x), N, P, h, w, nb, hs, ws, sw, de, _p(bs), _p(bh), _p(ba), _p(merge_w),
                                             s.scale, s.shift, s.alpha, s.out_ctot, s.out_coff, s.flags, _p(dst), _p(tables),
                                             _stream()))
        return dst
    check(lib.mspl_pyrpool_fused_fwd(_p(x), N, P, h, w, nb, hs, ws, sw, de, _p(bs), _p(bh), _p(ba), _p(merge_w),
                                     ctypes.byref(s), _p(dst), _stream()))
    return dst


def label_epilogue(main, aux, size, lut=None, want_labels=True, want_prob=False, want_kld=False,
                   want_logits=False):
    """K8+K9.  Returns dict with any of labels (uint8 N,H,W), prob, kld, main_up, aux_up."""
    main = _f32(main, 'main')
    N, C, Hm, Wm = main.shape
    Ha = Wa = 0
    if aux is not None:
        aux = _f32(aux, 'aux')
        if aux.shape[0] != N or aux.shape[1] != C:
            raise RuntimeError('mspl_amd: aux logits %s do not match main %s' % (tuple(aux.shape), tuple(main.shape)))
        Ha, Wa = aux.shape[2:]
    H, W = int(size[0]), int(size[1])
    dev = main.device
    res = {}
    if lut is not None:
        if lut.dtype != torch.uint8 or not lut.is_cuda or lut.numel() < C:
            raise RuntimeError('mspl_amd: lut must be a CUDA uint8 tensor with >= %d entries' % C)
    if want_labels:
        res['labels'] = torch.empty((N, H, W), device=dev, dtype=torch.uint8)
    if want_prob:
        res['prob'] = torch.empty((N, C, H, W), device=dev, dtype=torch.float32)
    if want_kld:
        res['kld'] = torch.empty((N, H, W), device=dev, dtype=torch.float32)
    if want_logits:
        res['main_up'] = torch.empty((N, C, H, W), device=dev, dtype=torch.float32)
        if aux is not None:
            res['aux_up'] = torch.empty((N, C, H, W), device=dev, dtype=torch.float32)
    check(lib.mspl_label_epilogue_fwd(_p(main), _p(aux), N, C, Hm, Wm, Ha, Wa, H, W, _p(lut), _p(res.get('labels')),
                                      _p(res.get('prob')), _p(res.get('kld')), _p(res.get('main_up')),
                                      _p(res.get('aux_up')), _stream()))
    return res


def label_epilogue_hist_fits(main, aux, size):
    """True when label_epilogue_hist covers these head shapes (else: label_epilogue + merge_labels(S=1))."""
    N, C, Hm, Wm = [int(v) for v in main.shape]
    Ha, Wa = ([int(v) for v in aux.shape[2:]] if aux is not None else (0, 0))
    return bool(lib.mspl_label_epilogue_hist_fits(N, C, Hm, Wm, Ha, Wa, int(size[0]), int(size[1])))


LABEL_EPILOGUE_FORMS = ('general', 'register', 'lds')      # MSPL_LE_FORM_*
_LE_PLAN_FIELDS = ('VEC', 'NRM', 'NRA', 'WMS', 'WAS', 'LDS_BYTES', 'PAIRS_MAIN', 'PAIRS_AUX', 'CMAX', 'EXACT', 'WIDE480', 'BANDS',
                   'COLBLOCKS', 'ROWSLOTS')


def label_epilogue_plan(shape, general=False, aligned16=True):
    """The kernel form the label epilogue takes (mspl_label_epilogue_plan, the launcher's own host function; no device call).
    shape: (N, C, Hm, Wm, Ha, Wa, H, W), Ha = Wa = 0 without a second head; general: probabilities or up-sampled logits are
    asked for; aligned16: both heads' base pointers are 16-byte aligned.  -> dict form ('general' / 'register' / 'lds') and the
    integers vec / nrm / nra / wms / was / lds_bytes / pairs_main / pairs_aux / cmax / exact / wide480 / bands / colblocks /
    rowslots, 0 where they do not apply to the form."""
    out = (ctypes.c_int32 * nat.LE_PLAN_LEN)()
    check(lib.mspl_label_epilogue_plan(*[int(v) for v in shape], int(bool(general)), int(bool(aligned16)), out))
    plan = {n.lower(): int(out[getattr(nat, 'LE_PLAN_' + n)]) for n in _LE_PLAN_FIELDS}
    plan['form'] = LABEL_EPILOGUE_FORMS[int(out[nat.LE_PLAN_FORM])]
    return plan


def label_epilogue_hist(main, aux, size, hist, num_classes, lut=None, want_kld=False):
    """K8+K9 + class histogram in one launch (single-source pass).  Requires C <= min(24, num_classes) so that every label is a
    counted class -- then it equals label_epilogue followed by merge_labels(S=1, thresh=1).  Returns dict(labels[, kld])."""
    main = _f32(main, 'main')
    N, C, Hm, Wm = main.shape
    Ha = Wa = 0
    if aux is not None:
        aux = _f32(aux, 'aux')
        if aux.shape[0] != N or aux.shape[1] != C:
            raise RuntimeError('mspl_amd: aux logits %s do not match main %s' % (tuple(aux.shape), tuple(main.shape)))
        Ha, Wa = aux.shape[2:]
    H, W = int(size[0]), int(size[1])
    if hist.dtype != torch.int64 or not hist.is_cuda or hist.numel() < num_classes:
        raise RuntimeError('mspl_amd: hist must be a CUDA int64 tensor with >= num_classes entries')
    if lut is not None and (lut.dtype != torch.uint8 or not lut.is_cuda or lut.numel() < C):
        raise RuntimeError('mspl_amd: lut must be a CUDA uint8 tensor with >= %d entries' % C)
    res = {'labels': torch.empty((N, H, W), device=main.device, dtype=torch.uint8)}
    if want_kld:
        res['kld'] = torch.empty((N, H, W), device=main.device, dtype=torch.float32)
    nbytes = int(lib.mspl_label_epilogue_hist_workspace_bytes(N, H, W))
    ws = torch.empty(max(nbytes, 4), device=main.device, dtype=torch.uint8)         # per-workgroup partial histograms
    check(lib.mspl_label_epilogue_hist_fwd(_p(main), _p(aux), N, C, Hm, Wm, Ha, Wa, H, W, _p(lut), _p(res['labels']),
                                           _p(res.get('kld')), _p(hist), int(num_classes), _p(ws), nbytes, _stream()))
    return res


def _head_planes(head, what):
    """A head before its classifier, (planes (N,P,h,w), weight (C,P[,1,1]), bias (C)) -> checked fp32 tensors and (N, P, C, h, w)."""
    planes, weight, bias = head
    planes, weight, bias = _f32(planes, what + ' planes'), _f32(weight, what + ' weight'), _f32(bias, what + ' bias')
    N, P, h, w = [int(v) for v in planes.shape]
    C = int(weight.shape[0])
    if weight.numel() != C * P or bias.numel() != C:
        raise RuntimeError('mspl_amd: %s classifier %s / bias %s does not match %d planes' %
                           (what, tuple(weight.shape), tuple(bias.shape), P))
    return planes, weight, bias, (N, P, C, h, w)


def label_epilogue_planes_fits(main, aux, size):
    """True when label_epilogue_planes covers these heads; main / aux: (planes, weight, bias), aux may be None."""
    N, P, Hm, Wm = [int(v) for v in main[0].shape]
    C = int(main[1].shape[0])
    Ha, Wa = ([int(v) for v in aux[0].shape[2:]] if aux is not None else (0, 0))
    if aux is not None and (int(aux[0].shape[1]) != P or int(aux[1].shape[0]) != C):
        return False
    return bool(lib.mspl_label_epilogue_planes_fits(N, P, C, Hm, Wm, Ha, Wa, int(size[0]), int(size[1])))


def label_epilogue_planes(main, aux, size, hist=None, num_classes=0, lut=None, want_kld=False):
    """K8+K9 from the heads' planes: the final 1x1 classifier of both heads is computed inside the epilogue (the logits are never
    written).  main / aux: (planes (N,P,h,w), weight (C,P,1,1), bias (C)); aux may be None.  With hist: label_epilogue_hist's
    histogram contract.  Equals conv1x1 + label_epilogue[_hist] bit for bit.  Returns dict(labels[, kld])."""
    mp, mw, mbias, (N, P, C, Hm, Wm) = _head_planes(main, 'main')
    ap = aw = abias = None
    Ha = Wa = 0
    if aux is not None:
        ap, aw, abias, (Na, Pa, Ca, Ha, Wa) = _head_planes(aux, 'aux')
        if (Na, Pa, Ca) != (N, P, C):
            raise RuntimeError('mspl_amd: aux head (N=%d, P=%d, C=%d) does not match main (N=%d, P=%d, C=%d)' % (Na, Pa, Ca, N, P, C))
    H, W = int(size[0]), int(size[1])
    if hist is not None and (hist.dtype != torch.int64 or not hist.is_cuda or hist.numel() < num_classes):
        raise RuntimeError('mspl_amd: hist must be a CUDA int64 tensor with >= num_classes entries')
    if lut is not None and (lut.dtype != torch.uint8 or not lut.is_cuda or lut.numel() < C):
        raise RuntimeError('mspl_amd: lut must be a CUDA uint8 tensor with >= %d entries' % C)
    res = {'labels': torch.empty((N, H, W), device=mp.device, dtype=torch.uint8)}
    if want_kld:
        res['kld'] = torch.empty((N, H, W), device=mp.device, dtype=torch.float32)
    ws, nbytes = None, 0
    if hist is not None:
        nbytes = int(lib.mspl_label_epilogue_hist_workspace_bytes(N, H, W))
        ws = torch.empty(max(nbytes, 4), device=mp.device, dtype=torch.uint8)       # per-workgroup partial histograms
    check(lib.mspl_label_epilogue_planes_fwd(_p(mp), _p(mw), _p(mbias), _p(ap), _p(aw), _p(abias), N, P, C, Hm, Wm, Ha, Wa, H, W,
                                             _p(lut), _p(res['labels']), _p(res.get('kld')), _p(hist), int(num_classes), _p(ws),
                                             nbytes, _stream()))
    return res


def merge_labels(sources, num_classes, thresh, fill=4, hist=None):
    """K10.  sources: list of uint8 CUDA tensors of identical shape.  hist: uint64-as-int64 CUDA tensor of
    num_classes entries, accumulated into (caller zeroes), or None."""
    S = len(sources)
    if S < 1:
        raise RuntimeError('mspl_amd: merge_labels needs at least one source')
    src = []
    for t in sources:
        if t.dtype != torch.uint8 or not t.is_cuda:
            raise RuntimeError('mspl_amd: merge_labels sources must be CUDA uint8 tensors')
        if t.shape != sources[0].shape:
            raise RuntimeError('mspl_amd: merge_labels sources differ in shape')
        src.append(t.contiguous())
    out = torch.empty_like(src[0])
    if hist is not None and (hist.dtype != torch.int64 or not hist.is_cuda or hist.numel() < num_classes):
        raise RuntimeError('mspl_amd: hist must be a CUDA int64 tensor with >= num_classes entries')
    arr = (ctypes.c_void_p * S)(*[t.data_ptr() for t in src])
    check(lib.mspl_merge_labels_fwd(arr, S, out.numel(), num_classes, int(thresh), int(fill), _p(out), _p(hist),
                                    _stream()))
    return out
