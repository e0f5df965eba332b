"""bench.py's contract: a plain run times exactly --steps steps once and prints the headline alone; --dump-outputs writes what
the timed path returned for its last batch.  The benchmark runs in a fresh child process, as it is run for measurements."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'repeats', 'config'}


def test_plain_run_times_the_steps_and_dumps_the_last_batch(tmp_path):
    d = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                        '--dump-outputs', str(d)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert HEADLINE <= set(line), sorted(line)
    assert line['steps'] == 3 and line['repeats'] == 1 and line['unit'] == 'images/s' and line['dtype'] == 'f32'
    assert line['higher_is_better'] is True and line['ms_per_step'] > 0
    assert abs(line['value'] - 16 * 1000.0 / line['ms_per_step']) <= 0.01 * line['value']
    # everything beyond the headline belongs to --full
    assert not {'roofline', 'single_in_flight', 'three_source', 'train_step', 'cpu_baseline', 'path_roofline'} & set(line)

    labels, kld = np.load(d / 'labels.npy'), np.load(d / 'kld.npy')
    assert labels.dtype == np.float32 and kld.dtype == np.float32
    assert labels.shape == kld.shape == (16, 288, 480)

    # the same seeded weights and batch through one graphed pass with the lanes' launch flags: the lanes are bit-identical to it
    # (tests/test_gpu_fullsize.py::test_pipelined_label_pass_equals_single_lane)
    from mspl_amd import models, ops, uest
    from tests.synth import synth_state_dict
    a = argparse.Namespace(s=2.0, channels=3, num_classes=1000)
    m = models.ESPDNetwithUncertaintyEstimation(a, classes=13, dataset='camvid', fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), 0))
    x = torch.randn((16, 3, 288, 480), generator=torch.Generator().manual_seed(1234)).cuda()
    ref = uest.SelfLabelPass(m, classes=13, device='cuda', use_graph=True)
    with ops.launch_flags(throughput=True):
        lab, kl = ref(x)
    torch.cuda.synchronize()
    assert np.array_equal(labels, lab.float().cpu().numpy())
    assert np.array_equal(kld, kl.cpu().numpy())
