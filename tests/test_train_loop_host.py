"""CPU-side checks of the drop-in train() loop: its signature and opt-in binding, the committed fixture's own conditions, and the
package's independence from the oracle.  No kernel is launched."""
import inspect
import json
import os
import re

import numpy as np

from mspl_amd import script
from tests.conftest import GOLDEN, ROOT
from tests.train_loop_cases import NEAR_CAP, TRAIN_LOOP_CASES, WRITER_IDX0, reference_areas

REFERENCE_SIGNATURE = ['trainloader', 'model', 'criterion', 'device', 'interp', 'optimizer', 'tot_iter', 'round_idx', 'epoch_idx', 'args',
                       'logger', 'metric', 'class_encoding', 'writer_idx', 'class_weights', 'writer', 'add_loss']
FIVE = ['generate_pseudo_label', 'generate_pseudo_label_multi_model', 'get_output', 'merge_outputs', 'update_image_list']
TAGS = ['uest/train/loss', 'uest/train/nid_loss', 'uest/train/mean_IoU', 'uest/train/traversable_plant_IoU',
        'uest/train/other_plant_mean_IoU', 'uest/train/artificial_object_mean_IoU', 'uest/train/ground_mean_IoU',
        'uest/train/learning_rate']


def test_train_has_the_reference_signature():
    ns = {}
    script.patch_script(ns, train=True)
    for fn in (script.train, ns['train']):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == REFERENCE_SIGNATURE
        assert [p.default for p in sig.parameters.values()][-3:] == [None, None, None]
        assert all(p.default is inspect.Parameter.empty for p in list(sig.parameters.values())[:14])


def test_binding_is_opt_in():
    ns = {}
    assert script.patch_script(ns) == FIVE and 'train' not in ns
    ns = {}
    assert script.patch_script(ns, train=True) == sorted(FIVE + ['train']) and callable(ns['train'])
    from mspl_amd import dropin
    sig = inspect.signature(dropin.install_dropin)
    assert list(sig.parameters) == ['force', 'script', 'train_loops'] and sig.parameters['train_loops'].default is False


def test_fixture_satisfies_its_conditions():
    g = dict(np.load(os.path.join(GOLDEN, 'train_loop.npz'), allow_pickle=False))
    meta = json.load(open(os.path.join(GOLDEN, 'train_loop.json')))
    assert sorted(meta) == sorted(TRAIN_LOOP_CASES)
    for name, case in TRAIN_LOOP_CASES.items():
        epochs, steps = sum(case['phases']), len(case['batches'])
        pixels = sum(case['batches']) * case['hw'][0] * case['hw'][1]
        assert g[name + '.areas'].shape == (epochs, steps, 3, 4) and g[name + '.loss'].shape == (epochs, steps)
        near = g[name + '.near']
        assert near.shape == (epochs, steps) and near.sum(axis=1).max() <= NEAR_CAP * pixels
        rec = meta[name]['records']
        assert [r[0] for r in rec] == TAGS * epochs
        assert [r[2] for r in rec] == [WRITER_IDX0 + e for e in range(epochs) for _ in TAGS]
        assert meta[name]['returned'] == [WRITER_IDX0 + e + 1 for e in range(epochs)]
        for e in range(epochs):
            # the scalars are the reference's formulas on the stored areas and losses (float32 sums there, integers here)
            a = g[name + '.areas'][e].sum(0).astype(np.float64)
            iou = a[0] / (a[1] + a[2] - a[0] + steps * 1e-6 + 1e-10)
            want = [iou.mean() * 100 if case['use_traversable'] else iou[[1, 2, 3]].mean() * 100] + list(iou)
            np.testing.assert_allclose([r[1] for r in rec[8 * e + 2:8 * e + 7]], want, rtol=1e-5)
            w = np.asarray(case['batches'], dtype=np.float64)
            np.testing.assert_allclose(rec[8 * e][1], (g[name + '.loss'][e] * w).sum() / w.sum(), rtol=1e-12)
            assert rec[8 * e + 1][1] == 0.0
        assert len(g[name + '.params_off']) == 571 and all((name + '.params_%d' % p) in g for p in range(len(case['phases'])))


def test_reference_areas_rule():
    """The integer restatement of segmentation_miou.py:28-41 the generator checks the reference's histograms with."""
    pred = np.array([0, 1, 2, 3, 4, 0, 1, 3])
    tgt = np.array([0, 1, 3, 3, 4, 255, 4, 2])
    a = reference_areas(pred, tgt, 4)
    assert a.tolist() == [[1, 1, 0, 1], [1, 2, 1, 2], [1, 1, 1, 2]]       # class id 4 (value 5) and the void pixel count nowhere


def test_package_never_imports_the_oracle():
    pat = re.compile(r'^\s*(from|import)\s+(oracle|tests)\b', re.M)
    pkg = os.path.join(ROOT, 'mspl_amd')
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith('.py'):
            assert not pat.search(open(os.path.join(pkg, fn)).read()), fn
