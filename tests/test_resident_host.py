"""Host side of the resident target set (mspl_amd.io.FrameStore / ResidentTrainLoader, the label loop's label_sink): the new C ABI
symbol, the FrameStore.from_list errors that happen before any device work, and the label loop's sink ordering with a stub pass.
No GPU: every from_list call here must fail before it touches the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.resident_cases import GOLDEN_N, RESIDENT_CASES, case_images, reference_transform, remap_lut


def test_store_symbol_is_declared_and_bound():
    from mspl_amd import _native
    name = 'mspl_train_transform_store_fwd'
    assert name in _native.SIGNATURES
    P, I = ctypes.c_void_p, ctypes.c_int
    # rgb label depth | M N Hs Ws Hl Wl H W crop scale_stage ignore_idx | recs_host recs_dev slots_host slots_dev lut mean std ws |
    # max_sh max_sw | out_rgb out_label out_depth stream
    want = [P] * 3 + [I] * 11 + [P] * 8 + [I] * 2 + [P] * 4
    fn = getattr(_native.lib, name)
    assert list(fn.argtypes) == want and fn.restype is ctypes.c_int
    # the contiguous call keeps its signature, the record its size, the ABI its revision (only a symbol was added)
    assert len(_native.lib.mspl_train_transform_fwd.argtypes) == 21
    assert ctypes.sizeof(_native.TrainRec) == 112


@pytest.mark.parametrize('name', sorted(RESIDENT_CASES))
def test_restatement_vs_reference_golden(name, golden):
    """The numpy restatement the GPU tests compare against, against what the reference's own classes produced (the fixture)."""
    import hashlib
    hs, ws, hl, wl, size, scale, crop, ign, norm, with_depth = RESIDENT_CASES[name][:10]
    g = golden('resident_transforms')
    sha = lambda a: np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
    lut = remap_lut()
    for k, (rgb, label, depth) in enumerate(case_images(name, GOLDEN_N)):
        t, lt, dt = reference_transform(rgb, lut[label], depth if with_depth else None, g[name + '.draws'][k], size, scale is not None,
                                        crop, ign, norm)
        assert np.array_equal(sha(t), g[name + '.rgb_sha'][k]), (name, k)
        assert np.array_equal(sha(lt), g[name + '.label_sha'][k]), (name, k)
        if with_depth:
            assert np.array_equal(sha(dt), g[name + '.depth_sha'][k]), (name, k)
        if k == 0:
            assert np.array_equal(t[:, ::23, ::29], g[name + '.rgb_s'])
            assert np.array_equal(lt[::23, ::29].astype(np.uint8), g[name + '.label_s'])


# ------------------------------------------------------------------ FrameStore.from_list: errors before any device work
def _write_set(tmp, n=3, frame=(9, 12), label=(5, 7), depth_mode='L', odd=None):
    """n frames / labels / depth maps as PNG files and their list file; odd = (kind, index): that file gets another size."""
    from PIL import Image
    rng = np.random.default_rng(3)
    lines = []
    for k in range(n):
        paths = {}
        for kind, (h, w), mode in (('color', frame, 'RGB'), ('label', label, 'L'), ('depth', frame, depth_mode)):
            if odd == (kind, k):
                h += 1
            if mode == 'RGB':
                im = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            elif mode == 'L':
                im = Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8))
            else:
                im = Image.fromarray(rng.integers(0, 60000, (h, w)).astype(np.uint16))         # a 16-bit depth map
            paths[kind] = os.path.join(str(tmp), '%s_%d.png' % (kind, k))
            im.save(paths[kind])
        lines.append('%s,%s,%s' % (paths['color'], paths['label'], paths['depth']))
    lst = os.path.join(str(tmp), 'set.lst')
    with open(lst, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return lst


def _no_device(monkeypatch):
    """Any upload would go through FrameStore.from_arrays: make it fail the test."""
    from mspl_amd import io as mio

    def boom(*a, **k):
        raise AssertionError('FrameStore.from_list reached the device')
    monkeypatch.setattr(mio.FrameStore, 'from_arrays', classmethod(boom))


def test_from_list_missing_file(tmp_path, monkeypatch):
    pytest.importorskip('PIL.Image')
    from mspl_amd import io as mio
    _no_device(monkeypatch)
    lst = _write_set(tmp_path)
    os.remove(os.path.join(str(tmp_path), 'label_1.png'))
    with pytest.raises(FileNotFoundError, match='label_1.png'):
        mio.FrameStore.from_list(lst)
    with pytest.raises(FileNotFoundError, match='label_1.png'):
        mio.FrameStore.from_list(lst, use_depth=True)
    os.remove(os.path.join(str(tmp_path), 'depth_2.png'))
    with pytest.raises(FileNotFoundError, match='depth_2.png'):
        mio.FrameStore.from_list(lst, use_depth=True, with_labels=False)


@pytest.mark.parametrize('kind', ['color', 'label', 'depth'])
def test_from_list_size_mismatch_names_the_file_and_both_sizes(tmp_path, monkeypatch, kind):
    pytest.importorskip('PIL.Image')
    from mspl_amd import io as mio
    _no_device(monkeypatch)
    lst = _write_set(tmp_path, odd=(kind, 2))
    h, w = (5, 7) if kind == 'label' else (9, 12)
    with pytest.raises(RuntimeError, match=r'%s_2\.png is %dx%d, the first one \(.*%s_0\.png\) is %dx%d' % (kind, w, h + 1, kind, w, h)):
        mio.FrameStore.from_list(lst, use_depth=True, workers=2)


def test_from_list_budget(tmp_path, monkeypatch):
    pytest.importorskip('PIL.Image')
    from mspl_amd import io as mio
    _no_device(monkeypatch)
    lst = _write_set(tmp_path)
    need = 3 * (9 * 12 * 4 + 5 * 7)
    with pytest.raises(RuntimeError, match='need %d bytes' % need):
        mio.FrameStore.from_list(lst, use_depth=True, max_bytes=need - 1)
    with pytest.raises(RuntimeError, match='need %d bytes' % (3 * 9 * 12 * 3)):
        mio.FrameStore.from_list(lst, with_labels=False, max_bytes=1)


def test_from_list_16_bit_depth_without_cv2(tmp_path, monkeypatch):
    pytest.importorskip('PIL.Image')
    import sys
    from mspl_amd import io as mio
    _no_device(monkeypatch)
    monkeypatch.setitem(sys.modules, 'cv2', None)          # `import cv2` raises ImportError, wherever OpenCV is installed
    lst = _write_set(tmp_path, depth_mode='I;16')
    with pytest.raises(RuntimeError, match=r'depth_0\.png.*OpenCV'):
        mio.FrameStore.from_list(lst, use_depth=True, workers=1)


# ------------------------------------------------------------------ the label loop's sink
class _StubPass:
    """PipelinedLabelPass's interface with one batch in flight and no GPU (as tests/test_dist_cpu.py's)."""

    def __init__(self):
        self.hist = torch.zeros(5, dtype=torch.int64)
        self._held = None

    def reset(self):
        self.hist.zero_()

    def _label(self, images):
        lab = (images.sum(1).round().to(torch.int64) % 5).to(torch.uint8)
        self.hist += torch.bincount(lab.flatten().to(torch.int64), minlength=5)
        return lab

    def __call__(self, images):
        out, self._held = self._held, self._label(images)
        return out

    def flush(self):
        if self._held is not None:
            out, self._held = self._held, None
            yield out


def _batches():
    g = torch.Generator().manual_seed(5)
    out, k = [], 0
    for n in (2, 3, 1):
        names = ['/data/color/frame_%03d.jpg' % (k + i) for i in range(n)]
        out.append((torch.rand(n, 3, 8, 12, generator=g) * 4, None, names, None))
        k += n
    return out


@pytest.mark.parametrize('fn', ['generate_pseudo_label', 'generate_pseudo_label_multi_model'])
def test_sink_is_called_once_per_batch_before_the_writers_submit(tmp_path, monkeypatch, fn):
    from mspl_amd import io as mio, uest
    batches = _batches()
    events = []
    submit = mio.LabelWriter.submit

    def logged(self, names, labels, stream=None):
        events.append(('submit', list(names)))
        return submit(self, names, labels, stream=stream)
    monkeypatch.setattr(mio.LabelWriter, 'submit', logged)
    got = []

    def sink(names, maps, stream):
        events.append(('sink', list(names)))
        got.append((list(names), maps.clone(), stream))
    call = (lambda **kw: uest.generate_pseudo_label(None, iter(batches), str(tmp_path / 'a'), writer_workers=2, **kw)) \
        if fn == 'generate_pseudo_label' else \
        (lambda **kw: uest.generate_pseudo_label_multi_model(None, None, iter(batches), str(tmp_path / 'a'), writer_workers=2, **kw))
    lst, w = call(_label_pass=_StubPass(), label_sink=sink)
    want = []
    for b in batches:
        want += [('sink', list(b[2])), ('submit', list(b[2]))]
    assert events == want
    stub = _StubPass()
    for (names, maps, stream), b in zip(got, batches):
        assert stream is None and maps.dtype == torch.uint8 and torch.equal(maps, stub._label(b[0]))
    # without a sink: the same list file and weights
    events[:] = []
    lst2, w2 = call(_label_pass=_StubPass())
    assert lst2 == lst and torch.equal(w, w2) and [e[0] for e in events] == ['submit'] * len(batches)


def test_sink_is_refused_with_more_than_one_rank(tmp_path, monkeypatch):
    from mspl_amd import dist as mdist, uest
    monkeypatch.setattr(mdist, 'world', lambda: (0, 2))
    with pytest.raises(RuntimeError, match='disjoint batches'):
        uest.generate_pseudo_label(None, iter(_batches()), str(tmp_path / 'b'), _label_pass=_StubPass(), label_sink=lambda *a: None)
    assert not os.path.exists(str(tmp_path / 'b'))         # refused before anything was written
