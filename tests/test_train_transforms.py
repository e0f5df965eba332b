"""Device-side train augmentation (mspl_amd.io.TrainPreprocessor, train_transforms.hip): RandomScale / RandomCrop / Resize /
RandomFlip / Normalize | Tensorize of transforms/segmentation/data_transforms.py for a batch.

CPU: the library's LANCZOS / BILINEAR tables against the numpy restatement (tests/pil_train_ref.py), the restatement against the
vectors the reference's own classes produced with Pillow (tests/golden/make_golden_train_transforms.py) and against the Pillow
installed here, draw() against the reference's draws.  GPU: every case bit-exact against the golden and the restatement, forced
records for the edges, out= in place, the error paths.
"""
import hashlib
import random

import numpy as np
import pytest
import torch

from tests import pil_train_ref as ref
from tests.pil_train_ref import GOLDEN_N, TRAIN_CASES, case_images


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def _pre(name, **kw):
    from mspl_amd.io import TrainPreprocessor
    hs, ws, size, scale, crop, ign, norm = TRAIN_CASES[name][:7]
    return TrainPreprocessor(size=size, scale=scale, crop=crop, ignore_idx=ign, normalize=norm, **kw)


SIZES = [(480, 240), (480, 960), (360, 180), (360, 719), (61, 31), (37, 18), (47, 94), (29, 58), (256, 256), (5, 7), (7, 5),
         (90, 45), (1, 3), (300, 301)]


def test_abi_tables_match_restatement():
    from mspl_amd._native import FILTER_BILINEAR, FILTER_LANCZOS, check, lib
    for filt in (FILTER_LANCZOS, FILTER_BILINEAR):
        for n_in, n_out in SIZES:
            k = lib.mspl_resample_ksize_filter(n_in, n_out, filt)
            bounds, kk = np.zeros((n_out, 2), np.int32), np.zeros((n_out, k), np.int32)
            check(lib.mspl_resample_coeffs_filter(n_in, n_out, filt, bounds.ctypes.data, kk.ctypes.data))
            rb, rk = ref.precompute_coeffs(n_in, n_out, filt)
            assert k == rk.shape[1] and np.array_equal(bounds, rb) and np.array_equal(kk, rk), (filt, n_in, n_out)
            if filt == FILTER_BILINEAR:                  # the generalised builder is the existing one for BILINEAR
                assert k == lib.mspl_resample_ksize(n_in, n_out)
                ob, ok = np.zeros_like(bounds), np.zeros_like(kk)
                check(lib.mspl_resample_coeffs(n_in, n_out, ob.ctypes.data, ok.ctypes.data))
                assert np.array_equal(ob, bounds) and np.array_equal(ok, kk)
    assert lib.mspl_resample_ksize_filter(480, 240, FILTER_LANCZOS) == 13          # 0.5x: 13-tap windows
    _, kk = ref.precompute_coeffs(480, 240, ref.LANCZOS)
    assert (kk < 0).any()                                                           # negative taps: the sign-dependent rounding
    assert lib.mspl_resample_ksize_filter(10, 5, 7) < 0 and lib.mspl_resample_ksize_filter(0, 5, FILTER_LANCZOS) < 0
    b = np.zeros((5, 2), np.int32)
    with pytest.raises(RuntimeError, match='filter'):
        check(lib.mspl_resample_coeffs_filter(10, 5, 3, b.ctypes.data, b.ctypes.data))


@pytest.mark.parametrize('name', sorted(TRAIN_CASES))
def test_restatement_vs_reference_golden(name, golden):
    hs, ws, size, scale, crop, ign, norm, with_depth = TRAIN_CASES[name][:8]
    g = golden('train_transforms')
    for k, (rgb, label, depth) in enumerate(case_images(name, GOLDEN_N)):
        t, lt, dt = ref.train_transform(rgb, label, depth if with_depth else None, g[name + '.draws'][k], size, crop, ign, norm)
        assert np.array_equal(_sha(t), g[name + '.rgb_sha'][k]), (name, k)
        assert np.array_equal(_sha(lt), g[name + '.label_sha'][k]), (name, k)
        if with_depth:
            assert np.array_equal(_sha(dt), g[name + '.depth_sha'][k]), (name, k)
        if k == 0:
            assert np.array_equal(t[:, ::23, ::29], g[name + '.rgb_s'])
            assert np.array_equal(lt[::23, ::29].astype(np.uint8), g[name + '.label_s'])


def test_restatement_vs_live_pillow():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(9)
    for hs, ws, size in [(360, 480, (240, 180)), (360, 480, (960, 720)), (61, 47, (30, 61)), (37, 90, (45, 18)), (29, 37, (37, 30))]:
        img = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
        dep = rng.integers(0, 256, (hs, ws), dtype=np.uint8)
        lz = ref.resize_u8(img, size, ref.LANCZOS)
        assert np.array_equal(lz, np.asarray(Image.fromarray(img).resize(size, Image.LANCZOS))), (hs, ws, size)
        assert np.array_equal(ref.resize_u8(lz, (48, 40), ref.BILINEAR),
                              np.asarray(Image.fromarray(lz).resize((48, 40), Image.BILINEAR)))
        assert np.array_equal(ref.resize_u8(dep, size, ref.BILINEAR), np.asarray(Image.fromarray(dep).resize(size, Image.BILINEAR)))
        # an unchanged axis is skipped (a LANCZOS pass over an unchanged size is not the identity)
        one = (ws, size[1])
        assert np.array_equal(ref.resize_u8(img, one, ref.LANCZOS), np.asarray(Image.fromarray(img).resize(one, Image.LANCZOS)))


@pytest.mark.parametrize('name', sorted(TRAIN_CASES))
def test_draw_consumes_the_reference_draws(name, golden):
    hs, ws = TRAIN_CASES[name][:2]
    seed = TRAIN_CASES[name][8]
    g = golden('train_transforms')
    random.seed(seed)
    got = _pre(name).draw(GOLDEN_N, (ws, hs))
    assert np.array_equal(np.array([tuple(int(v) for v in d) for d in got], np.int32), g[name + '.draws'])
    assert random.random() == float(g[name + '.next'])


# ------------------------------------------------------------------ GPU
def _check_against_restatement(pre, imgs, params, x, y, d):
    W, H = pre.size
    for k, (rgb, label, depth) in enumerate(imgs):
        t, lt, dt = ref.train_transform(rgb, label, None if d is None else depth, params[k], (W, H), pre.crop, pre.ignore_idx,
                                        pre.normalize)
        assert np.array_equal(x[k].cpu().numpy(), t), k
        assert np.array_equal(y[k].cpu().numpy(), lt), k
        if d is not None:
            assert np.array_equal(d[k].cpu().numpy(), dt), k


def _stack(imgs):
    return [torch.from_numpy(np.stack([im[c] for im in imgs])) for c in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize('N', [GOLDEN_N, 16])
@pytest.mark.parametrize('name', sorted(TRAIN_CASES))
def test_device_bit_exact(name, N, golden):
    hs, ws, size, scale, crop, ign, norm, with_depth, seed = TRAIN_CASES[name][:9]
    g = golden('train_transforms')
    pre = _pre(name)
    imgs = case_images(name, N)
    rgb, lab, dep = _stack(imgs)
    random.seed(seed)
    x, y, d = pre(rgb, lab, dep if with_depth else None)                  # params=None: draw() with the module-level random
    if N == GOLDEN_N:
        assert random.random() == float(g[name + '.next'])
    random.seed(seed)
    params = pre.draw(N, (ws, hs))
    assert x.shape == (N, 3, size[1], size[0]) and x.dtype == torch.float32 and y.dtype == torch.int64
    assert (d is not None) == with_depth
    for k in range(GOLDEN_N):                                               # the first 8 draws are the golden's
        assert np.array_equal(_sha(x[k].cpu().numpy()), g[name + '.rgb_sha'][k]), k
        assert np.array_equal(_sha(y[k].cpu().numpy()), g[name + '.label_sha'][k]), k
        if with_depth:
            assert np.array_equal(_sha(d[k].cpu().numpy()), g[name + '.depth_sha'][k]), k
    _check_against_restatement(pre, imgs, params, x, y, d)


def _forced(Ws, Hs, W, H, crop):
    """Records for the edges: unchanged size, one axis only, the smallest and largest scale, odd pads, far corner, both flips."""
    from mspl_amd.io import TrainDraw
    recs = []
    shapes = [(Ws, Hs), (Ws, Hs + 7), (Ws - 5, Hs), (int(round(Ws * 0.5)), int(round(Hs * 0.5))), (Ws * 2, Hs * 2), (W - 5, H - 5),
              (W + 9, H + 4), (W - 2, H - 3)]
    for k, (sw, sh) in enumerate(shapes):
        flip = k % 2 == 1
        if not crop:
            recs.append(TrainDraw(sw, sh, 0, 0, 0, 0, flip))
            continue
        pw, ph = max(0, int((1 + W - sw) / 2)), max(0, int((1 + H - sh) / 2))
        far = k % 3 != 0                                                      # crop at the far corner or at the origin
        i, j = (sh + 2 * ph - H, sw + 2 * pw - W) if far else (0, 0)
        recs.append(TrainDraw(sw, sh, pw, ph, i, j, flip))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize('crop', [False, True])
def test_device_forced_edges(crop):
    from mspl_amd.io import TrainPreprocessor
    Hs, Ws, W, H = 45, 58, 50, 40
    pre = TrainPreprocessor(size=(W, H), scale=(0.5, 2.0), crop=crop, ignore_idx=7, normalize=True)
    recs = _forced(Ws, Hs, W, H, crop)
    assert any(r.pad_w % 2 == 1 for r in recs) or not crop
    from tests.synth import synth_image_u8
    imgs = [synth_image_u8(Hs, Ws, 900 + k) for k in range(len(recs))]
    rgb, lab, dep = _stack(imgs)
    x, y, d = pre(rgb, lab, dep, params=recs)
    _check_against_restatement(pre, imgs, recs, x, y, d)
    for k in range(len(recs)):                                              # N = 1, each record on its own
        x1, y1, d1 = pre(rgb[k:k + 1], lab[k:k + 1], dep[k:k + 1], params=recs[k:k + 1])
        assert torch.equal(x1[0], x[k]) and torch.equal(y1[0], y[k]) and torch.equal(d1[0], d[k])
    if crop:
        assert (y == 7).any()                                               # padded label pixels are ignore_idx


@pytest.mark.gpu
def test_out_in_place_and_no_label_or_depth():
    name = 'greenhouse_rgbd_tensorize_odd'
    hs, ws, size = TRAIN_CASES[name][:3]
    pre = _pre(name)
    imgs = case_images(name, 4)
    rgb, lab, dep = _stack(imgs)
    params = pre.draw(4, (ws, hs), rng=random.Random(5))
    W, H = size
    ox = torch.full((4, 3, H, W), -1.0, device='cuda')
    oy = torch.full((4, H, W), -1, dtype=torch.int64, device='cuda')
    od = torch.full((4, 1, H, W), -1.0, device='cuda')
    x, y, d = pre(rgb.cuda(), lab.cuda(), dep.cuda(), params=params, out=(ox, oy, od))
    assert x is ox and y is oy and d is od
    _check_against_restatement(pre, imgs, params, x, y, d)
    x2, y2, d2 = pre(rgb, params=params, out=torch.zeros_like(ox))
    assert y2 is None and d2 is None and torch.equal(x2, ox)


@pytest.mark.gpu
def test_error_paths():
    from mspl_amd.io import TrainDraw
    name = 'camvid_crop_small_pad'
    hs, ws, size = TRAIN_CASES[name][:3]
    pre = _pre(name)
    rgb, lab, dep = _stack(case_images(name, 2))
    with pytest.raises(RuntimeError, match='uint8'):
        pre(rgb.float())
    with pytest.raises(RuntimeError, match='does not match'):
        pre(rgb, lab[:1])
    with pytest.raises(RuntimeError, match='does not match'):
        pre(rgb, lab, dep[:, :, 1:])
    with pytest.raises(RuntimeError, match='records'):
        pre(rgb, lab, params=pre.draw(3, (ws, hs)))
    with pytest.raises(RuntimeError, match='out='):
        pre(rgb, lab, out=torch.empty(2, 3, 5, 5, device='cuda'))
    with pytest.raises(RuntimeError, match='out='):
        pre(rgb, lab, out=(None, torch.empty(2, size[1], size[0], dtype=torch.int32, device='cuda'), None))
    W, H = size
    bad = [TrainDraw(ws, hs, 10, 10, 0, 0, False), TrainDraw(ws, hs, 10, 10, 100, 0, False)]      # crop origin outside
    with pytest.raises(RuntimeError, match='crop origin'):
        pre(rgb, lab, params=bad)
    with pytest.raises(RuntimeError, match='smaller than the crop'):
        pre(rgb, lab, params=[TrainDraw(ws, hs, 0, 0, 0, 0, False)] * 2)
    with pytest.raises(RuntimeError, match='scaled size'):
        pre(rgb, lab, params=[TrainDraw(0, hs, 0, 0, 0, 0, False)] * 2)
    torch.cuda.synchronize()
    x, y, _ = pre(rgb, lab)                                                 # still usable after the errors
    assert x.shape == (2, 3, H, W)
