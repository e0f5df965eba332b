"""The resident target set on the device: mspl_train_transform_store_fwd (train transforms reading a FrameStore by slot, label maps
of their own size, source-label LUT), mspl_amd.io.FrameStore / ResidentTrainLoader and the label loop's label_sink.

Every transform output is compared bit for bit: against the contiguous entry point, against the numpy restatement of Pillow
(tests/pil_train_ref.py) and against what the reference's own classes produced (tests/golden/resident_transforms.npz, written by
tests/golden/make_golden_resident.py)."""
import argparse
import hashlib
import os
import random

import numpy as np
import pytest
import torch

from tests import pil_train_ref as ref
from tests.pil_train_ref import TRAIN_CASES
from tests.resident_cases import GOLDEN_N, RESIDENT_CASES, case_images, reference_transform, remap_lut
from tests.synth import synth_image_u8, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def _stack(imgs):
    return [torch.from_numpy(np.stack([im[c] for im in imgs])) for c in range(3)]


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v)


def _check_restatement(pre, imgs, params, got, scale_stage=True, lut=None):
    """imgs: [(rgb, label at its own size, depth)]; the label is remapped on the host first when a LUT went to the device."""
    x, y, d = got
    for k, (rgb, label, depth) in enumerate(imgs):
        lab = label if lut is None else lut[label]
        t, lt, dt = reference_transform(rgb, lab, None if d is None else depth, params[k], pre.size, scale_stage, pre.crop,
                                        pre.ignore_idx, pre.normalize)
        assert np.array_equal(x[k].cpu().numpy(), t), k
        assert np.array_equal(y[k].cpu().numpy(), lt), k
        if d is not None:
            assert np.array_equal(d[k].cpu().numpy(), dt), k


# ------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize('name', ['greenhouse_rgbd_tensorize_odd', 'crop_with_depth'])
def test_identity_slots_equal_the_contiguous_call(name, golden):
    from mspl_amd.io import TrainDraw, TrainPreprocessor
    hs, ws, size, scale, crop, ign, norm = TRAIN_CASES[name][:7]
    pre = TrainPreprocessor(size=size, scale=scale, crop=crop, ignore_idx=ign, normalize=norm)
    params = [TrainDraw(*[int(v) for v in d]) for d in golden('train_transforms')[name + '.draws']]
    rgb, lab, dep = [t.to(DEV) for t in _stack(ref.case_images(name, GOLDEN_N))]
    want = pre(rgb, lab, dep, params=params)                                          # mspl_train_transform_fwd
    _same(pre(rgb, lab, dep, params=params, slots=list(range(GOLDEN_N))), want)       # the store entry point, slot list 0..N-1
    _same(pre(rgb, lab, dep, params=params, slots=torch.arange(GOLDEN_N)), want)
    _same(pre(rgb, lab, dep, params=params, label_lut=np.arange(256, dtype=np.uint8)), want)      # ... with NULL slots (slot n = n)


# ------------------------------------------------------------------ 2. golden
@pytest.mark.parametrize('name', sorted(RESIDENT_CASES))
def test_golden_labels_of_another_size(name, golden):
    from mspl_amd.io import TrainPreprocessor
    hs, ws, hl, wl, size, scale, crop, ign, norm, with_depth, seed = RESIDENT_CASES[name][:11]
    g = golden('resident_transforms')
    pre = TrainPreprocessor(size=size, scale=scale, crop=crop, ignore_idx=ign, normalize=norm)
    imgs = case_images(name, GOLDEN_N)
    rgb, lab, dep = _stack(imgs)
    assert tuple(lab.shape[1:]) == (hl, wl) != (hs, ws)
    lut = remap_lut()
    random.seed(seed)
    x, y, d = pre(rgb, lab, dep if with_depth else None, label_lut=lut)              # params=None: draw() with the module-level random
    assert random.random() == float(g[name + '.next'])
    random.seed(seed)
    params = pre.draw(GOLDEN_N, (ws, hs))
    assert np.array_equal(np.array([tuple(int(v) for v in p) for p in params], np.int32), g[name + '.draws'])
    assert x.shape == (GOLDEN_N, 3, size[1], size[0]) and y.shape == (GOLDEN_N, size[1], size[0]) and (d is not None) == with_depth
    for k in range(GOLDEN_N):
        assert np.array_equal(_sha(x[k].cpu().numpy()), g[name + '.rgb_sha'][k]), k
        assert np.array_equal(_sha(y[k].cpu().numpy()), g[name + '.label_sha'][k]), k
        if with_depth:
            assert np.array_equal(_sha(d[k].cpu().numpy()), g[name + '.depth_sha'][k]), k
    _check_restatement(pre, imgs, params, (x, y, d), scale_stage=scale is not None, lut=lut)


# ------------------------------------------------------------------ 3. label seams
def test_label_seams():
    """The sizes at which the label path switches tables, on the odd_two_tiles sizes (frame 45x58, labels 24x40, output 40x80: two
    32x64 tiles each way), every record with and without the mirror."""
    from mspl_amd.io import TrainDraw, TrainPreprocessor
    hs, ws, hl, wl, size = RESIDENT_CASES['odd_two_tiles'][:5]
    W, H = size
    imgs = case_images('odd_two_tiles', 8)
    rgb, lab, dep = _stack(imgs)
    shapes = [(ws, hs),            # frame unscaled, label scaled
              (wl, hl),            # label unscaled, frame scaled
              (W, H),              # Resize is a copy
              (ws, hs + 15)]       # sw == Ws with sh != Hs
    recs = [TrainDraw(sw, sh, 0, 0, 0, 0, flip) for sw, sh in shapes for flip in (False, True)]
    pre = TrainPreprocessor(size=size, scale=(0.5, 2.0), crop=False, normalize=True)
    _check_restatement(pre, imgs, recs, pre(rgb, lab, dep, params=recs))
    # crop mode, padding on both axes: 23x30 padded by (9, 25) to 41x80, cropped at row 1
    sw, sh = 30, 23
    pw, ph = max(0, int((1 + W - sw) / 2)), max(0, int((1 + H - sh) / 2))
    assert pw > 0 and ph > 0 and sh + 2 * ph - H == 1
    crecs = [TrainDraw(sw, sh, pw, ph, 1, 0, flip) for flip in (False, True)]
    cpre = TrainPreprocessor(size=size, scale=(0.5, 2.0), crop=True, ignore_idx=255, normalize=True)
    got = cpre(rgb[:2], lab[:2], dep[:2], params=crecs)
    _check_restatement(cpre, imgs[:2], crecs, got)
    assert (got[1] == 255).sum() >= 2 * (H * W - sh * sw)


# ------------------------------------------------------------------ 4. slots
def test_slots_gather_and_range_check():
    from mspl_amd.io import TrainPreprocessor
    hs, ws, hl, wl, size = RESIDENT_CASES['odd_two_tiles'][:5]
    W, H = size
    rgb, lab, dep = [t.to(DEV) for t in _stack(case_images('odd_two_tiles', 7))]
    pre = TrainPreprocessor(size=size, scale=(0.5, 2.0))
    slots = [6, 0, 3, 3, 6]
    params = pre.draw(len(slots), (ws, hs), rng=random.Random(4))
    assert any((p.sw, p.sh) != (ws, hs) for p in params)
    idx = torch.tensor(slots, device=DEV)
    want = pre(rgb.index_select(0, idx), lab.index_select(0, idx), dep.index_select(0, idx), params=params)
    _same(pre(rgb, lab, dep, params=params, slots=slots), want)
    assert not torch.equal(want[0][2], want[0][3])                    # one slot twice, with its own draw each time
    for bad in ([0, 7, 1, 2, 3], [0, -1, 1, 2, 3]):
        out = (torch.full((5, 3, H, W), -7.0, device=DEV), torch.full((5, H, W), -7, dtype=torch.int64, device=DEV),
               torch.full((5, 1, H, W), -7.0, device=DEV))
        with pytest.raises(RuntimeError, match=r'mspl_hip \(-1\).*slot %d' % bad[1]):          # MSPL_ERR_BAD_SHAPE
            pre(rgb, lab, dep, params=params, slots=bad, out=out)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in out)                # nothing was launched


# ------------------------------------------------------------------ 5. offsets beyond 4 GiB
def test_slot_offsets_beyond_4_gib():
    from mspl_amd.io import TrainDraw, TrainPreprocessor
    free = torch.cuda.mem_get_info()[0]
    if free < 8e9:
        pytest.skip('a 4.4 GB store needs 8 GB of free device memory, %.1f GB are free' % (free / 1e9))
    S = 64
    frame = S * S * 3
    M = 358400                                                        # 4.404 GB
    first = 349526                                                    # the first slot whose byte offset is above 2^32
    assert (first - 1) * frame < 2 ** 32 < first * frame and (M - 1) * frame > 2 ** 32
    store = torch.empty((M, S, S, 3), dtype=torch.uint8, device=DEV)
    frames = torch.from_numpy(np.stack([synth_image_u8(S, S, 40 + k)[0] for k in range(3)])).to(DEV)
    slots = [0, first, M - 1]
    for k, s in enumerate(slots):
        store[s] = frames[k]
    pre = TrainPreprocessor(size=(48, 40), scale=(0.5, 2.0))
    recs = [TrainDraw(96, 96, 0, 0, 0, 0, False), TrainDraw(S, S, 0, 0, 0, 0, True), TrainDraw(40, 50, 0, 0, 0, 0, False)]
    got = pre(store, params=recs, slots=slots)
    want = pre(frames, params=recs, slots=[0, 1, 2])
    _same(got, want)
    _same(want, pre(frames, params=recs))
    del store
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 6. LUT
def test_label_lut_remaps_source_values_only():
    from mspl_amd.io import TrainDraw, TrainPreprocessor
    hs, ws, hl, wl, size = RESIDENT_CASES['crop_after_scale'][:5]
    W, H = size
    imgs = case_images('crop_after_scale', 4)
    rgb, lab, _ = _stack(imgs)
    lab[:, :3, :5] = 255                                              # source 255 inside the crop: must come out as 7
    lab[:, 3, :5] = 0
    lut = np.arange(256, dtype=np.uint8)
    lut[0], lut[255] = 1, 7
    pre = TrainPreprocessor(size=size, scale=(0.5, 2.0), crop=True, ignore_idx=255)
    recs = []
    for k, (sw, sh) in enumerate([(35, 27), (39, 31), (35, 27), (69, 54)]):
        pw, ph = max(0, int((1 + W - sw) / 2)), max(0, int((1 + H - sh) / 2))
        recs.append(TrainDraw(sw, sh, pw, ph, (sh + 2 * ph - H) // 2, (sw + 2 * pw - W) // 2, k % 2 == 1))
    got = pre(rgb, lab, params=recs, label_lut=lut)
    want = pre(rgb, torch.from_numpy(lut[lab.numpy()]), params=recs)  # remapped on the host first, no LUT
    _same(got, want)
    _check_restatement(pre, [(im[0], lab[k].numpy(), im[2]) for k, im in enumerate(imgs)], recs, got, lut=lut)
    y = got[1].cpu().numpy()
    assert (y == 7).any() and not (y == 0).any()
    pad = np.ones((H, W), bool)                                       # image 0: 27x35 padded by (7, 8) to 41x51, crop origin (0, 0)
    pad[7:7 + 27, 8:8 + 35] = False
    assert recs[0][2:6] == (8, 7, 0, 0) and (y[0][pad] == 255).all()  # the fill is ignore_idx, not lut[ignore_idx]


# ------------------------------------------------------------------ 7. loader order
def _synthetic_store(n, with_depth):
    from mspl_amd.io import FrameStore
    frames = [synth_image_u8(45, 58, 700 + k) for k in range(n)]
    labels = np.stack([synth_image_u8(24, 40, 800 + k)[1] for k in range(n)])
    names = ['/data/tgt/color/frame_%03d.jpg' % k for k in range(n)]
    return FrameStore.from_arrays(np.stack([f[0] for f in frames]), labels, np.stack([f[2] for f in frames]) if with_depth else None, names)


@pytest.mark.parametrize('shuffle,drop_last,depth', [(True, False, False), (True, True, False), (False, False, False), (True, False, True)])
def test_loader_order_and_rng_consumption(shuffle, drop_last, depth):
    """The batches of ResidentTrainLoader against a torch Dataset + DataLoader that transforms one image at a time."""
    from torch.utils.data import DataLoader, Dataset
    from mspl_amd.io import ResidentTrainLoader, TrainPreprocessor
    store = _synthetic_store(10, depth)
    pre = TrainPreprocessor(size=(48, 32), scale=(0.5, 2.0))
    lut = remap_lut()

    class PerImage(Dataset):
        def __len__(self):
            return len(store)

        def __getitem__(self, k):
            x, y, d = pre(store.rgb[k:k + 1], store.labels[k:k + 1], store.depth[k:k + 1] if depth else None,
                          params=pre.draw(1, (58, 45)), label_lut=lut)
            return (x[0], y[0], d[0], store.names[k], 0.25) if depth else (x[0], y[0], store.names[k], 0.25)

    def epoch(loader):
        torch.manual_seed(31)
        random.seed(32)
        batches = list(loader)
        return batches, torch.get_rng_state(), random.getstate()
    want, t_want, r_want = epoch(DataLoader(PerImage(), shuffle=shuffle, num_workers=0, batch_size=4, drop_last=drop_last))
    loader = ResidentTrainLoader(store, pre, 4, shuffle=shuffle, drop_last=drop_last, use_depth=depth, reg_weight=0.25, label_lut=lut)
    got, t_got, r_got = epoch(loader)
    assert len(got) == len(want) == len(loader) == (2 if drop_last else 3)
    assert torch.equal(t_got, t_want) and r_got == r_want
    for b, w in zip(got, want):
        assert len(b) == len(w) == (5 if depth else 4)
        assert b[0].dtype == torch.float32 and b[1].dtype == torch.int64 and b[0].is_cuda and b[1].is_cuda
        _same(b[:3 if depth else 2], w[:3 if depth else 2])
        assert list(b[-2]) == list(w[-2])
        assert b[-1].dtype == w[-1].dtype == torch.float64 and b[-1].is_cuda and torch.equal(b[-1].cpu(), w[-1].cpu())
    if shuffle:
        assert [n for b in got for n in b[-2]] != store.names[:len(got) * 4]
    else:
        assert [n for b in got for n in b[-2]] == store.names


# ------------------------------------------------------------------ 8. from_list
def test_from_list(tmp_path):
    from PIL import Image
    from mspl_amd.io import FrameStore
    rng = np.random.default_rng(8)
    arrays, lines = {'color': [], 'label': [], 'depth': []}, []
    for k in range(6):
        row = []
        for kind, shape in (('color', (45, 58, 3)), ('label', (24, 40)), ('depth', (45, 58))):
            a = rng.integers(0, 256, shape, dtype=np.uint8)
            p = str(tmp_path / ('%s_%d.png' % (kind, k)))
            Image.fromarray(a).save(p)
            arrays[kind].append(a)
            row.append(p)
        lines.append(','.join(row))
    lst = str(tmp_path / 'tgt.lst')
    open(lst, 'w').write('\n'.join(lines) + '\n')
    store = FrameStore.from_list(lst, use_depth=True)
    assert len(store) == 6 and store.names == [l.split(',')[0] for l in lines] and store.rgb.is_cuda
    assert np.array_equal(store.rgb.cpu().numpy(), np.stack(arrays['color']))
    assert np.array_equal(store.labels.cpu().numpy(), np.stack(arrays['label']))
    assert np.array_equal(store.depth.cpu().numpy(), np.stack(arrays['depth']))
    bare = FrameStore.from_list(lst, with_labels=False)
    assert bare.labels is None and bare.depth is None and torch.equal(bare.rgb, store.rgb)
    views = list(bare.frames(4))
    assert [len(v[-2]) for v in views] == [4, 2] and views[1][0].data_ptr() == bare.rgb[4:].data_ptr() and views[0][1] is None
    views = list(store.frames(4))
    assert len(views[0]) == 5 and views[1][2].data_ptr() == store.depth[4:].data_ptr()
    # budget: refused before any device allocation
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match='need %d bytes' % (6 * (45 * 58 * 4 + 24 * 40))):
        FrameStore.from_list(lst, use_depth=True, max_bytes=1)
    assert torch.cuda.memory_allocated() == before
    # a frame of another size
    Image.fromarray(rng.integers(0, 256, (46, 58, 3), dtype=np.uint8)).save(str(tmp_path / 'color_4.png'))
    with pytest.raises(RuntimeError, match=r'color_4\.png is 58x46.*58x45'):
        FrameStore.from_list(lst, use_depth=True)


# ------------------------------------------------------------------ 9. label pass into the store
def _model(classes, dataset, seed):
    from mspl_amd import models
    a = argparse.Namespace(s=2.0, channels=3, num_classes=1000)
    m = models.ESPDNetwithUncertaintyEstimation(a, classes=classes, dataset=dataset, fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed))
    return m


def _frames_only_store(n=6):
    from mspl_amd.io import FrameStore
    rgb = np.stack([synth_image_u8(45, 58, 900 + k)[0] for k in range(n)])
    return FrameStore.from_arrays(rgb, names=['/data/tgt/color/r_%d.jpg' % k for k in range(n)])


def _png_maps(save, store):
    from PIL import Image
    return np.stack([np.array(Image.open('%s/pred/%s.png' % (save, os.path.basename(n).rsplit('.', 1)[0])), np.uint8) for n in store.names])


@pytest.mark.parametrize('multi', [False, True])
def test_label_pass_writes_into_the_store(tmp_path, multi):
    from mspl_amd import uest
    from mspl_amd.io import Preprocessor
    store = _frames_only_store()
    pre = Preprocessor(size=(48, 32))
    if multi:
        ms = [_model(13, 'camvid', 61), _model(5, 'greenhouse', 63)]
        run = lambda **kw: uest.generate_pseudo_label_multi_model(ms, ['camvid', 'forest'], store.frames(4), str(tmp_path), transform=pre, **kw)
    else:
        m = _model(5, 'greenhouse', 71)
        run = lambda **kw: uest.generate_pseudo_label(m, store.frames(4), str(tmp_path), transform=pre, **kw)
    lst0, cw0 = run()                                                 # the list-file path alone
    maps0 = _png_maps(str(tmp_path), store)
    assert store.labels is None and not store.labelled.any()
    lst1, cw1 = run(label_sink=store.put_labels)
    assert lst1 == lst0 and torch.equal(cw1, cw0)
    assert store.labelled.all() and tuple(store.labels.shape) == (6, 32, 48) and store.labels.dtype == torch.uint8
    got = store.labels.cpu().numpy()
    assert np.array_equal(got, _png_maps(str(tmp_path), store))       # what the files hold ...
    assert np.array_equal(got, maps0) and len(np.unique(got)) > 1     # ... and what the call without a sink wrote
    with pytest.raises(KeyError, match='not a frame'):
        store.put_labels(['/data/tgt/color/other.jpg'], store.labels[:1])
    with pytest.raises(RuntimeError, match='maps of 47x32'):
        store.put_labels(store.names[:1], store.labels[:1, :, :47].contiguous())
    # names out of slot order: one gathered copy
    store.put_labels([store.names[4], store.names[1]], store.labels[[0, 5]].clone())
    after = store.labels.cpu().numpy()
    assert np.array_equal(after[4], got[0]) and np.array_equal(after[1], got[5]) and np.array_equal(after[[0, 2, 3, 5]], got[[0, 2, 3, 5]])


# ------------------------------------------------------------------ 10. one epoch
def test_one_epoch_of_script_train_from_the_store(tmp_path):
    """The drop-in train() on a ResidentTrainLoader with the settings of the graphed fast path: a smoke test of existing code on the
    new iterable (2 iterations of 3 images), not a parity test."""
    from mspl_amd import losses, script, training, uest
    from mspl_amd.io import Preprocessor, ResidentTrainLoader, TrainPreprocessor
    store = _frames_only_store()
    m = _model(5, 'greenhouse', 71).to(DEV).eval()
    uest.generate_pseudo_label(m, store.frames(4), str(tmp_path), transform=Preprocessor(size=(48, 32)), label_sink=store.put_labels)
    loader = ResidentTrainLoader(store, TrainPreprocessor(size=(48, 32), scale=(0.5, 2.0)), 3, label_lut=remap_lut())
    assert len(loader) == 2
    crit = losses.UncertaintyWeightedSegmentationLoss(5, class_weights=torch.tensor([0.0, 6.31, 3.78, 3.18, 7.64]), ignore_idx=4, device=DEV)
    opt = torch.optim.Adam(m.parameters(), lr=5e-4, weight_decay=5e-4)
    args = argparse.Namespace(model='espdnetue', use_depth=False, use_uncertainty=True, use_traversable=False, learning_rate=5e-4, power=0.9)

    class Writer(object):
        records = []

        def add_scalar(self, tag, value, idx):
            self.records.append((tag, float(value), int(idx)))
    assert script._fast_path(m, crit, opt, args, None)
    before = [p.detach().clone() for p in m.parameters()]
    idx = script.train(loader, m, crit, DEV, None, opt, 6.0, 0, 0, args, None, None, None, 7, None, Writer(), None)
    assert idx == 8
    meters = m.__dict__['_mspl_train_loop']['meters']
    assert meters.images == 6 and meters.steps == 2
    assert isinstance(m.__dict__['_mspl_train_loop']['step'], training.GraphedTrainStep) and len(opt.state) == 0
    assert len(Writer.records) == 8 and all(np.isfinite(r[1]) and r[2] == 7 for r in Writer.records)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
