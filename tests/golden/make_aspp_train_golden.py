#!/usr/bin/env python3
"""Generate tests/golden/aspp_train_<case>.npz and aspp_train.json by running the REFERENCE's own nn_layers/aspp.py in train() on
the CPU, once in float64 (the record) and once in float32 (the yardstick: its error against float64 is stored per quantity, and the
GPU test holds the HIP path within 4x of it).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_aspp_train_golden.py <path of the reference checkout>

One forward and one backward per case, loss = sum(logits * G) for a seeded cotangent G (no loss kernel involved).  Only data is
written; weights, inputs and G come from seeds (tests/synth.py), the stored elements of large tensors from
tests/aspp_train_cases.sample_index.

Per case the .npz holds (float64):
    logits                       in full
    gx, gx_chansum, gx_pixsum    input gradient: seeded sample, its sum over channels (N,H,W), its sum over (n,y,x) per channel
    g__<parameter>               gradient in full (<= 8192 elements) or the seeded sample
    tapsum__<w>, tapnorm__<w>    3x3 weights: per-tap sum and L2 norm of the whole gradient
    rm__<bn>, rv__<bn>, nbt__<bn>  running statistics and num_batches_tracked after the step
and aspp_train.json, per case and quantity: 'err' = max |float32 - float64| / max |float64| over what is stored ('abs' for the
bias gradients in front of a BatchNorm, whose float64 value is rounding-level zero: the float32 reference's max |gradient|), and
'scale' = max |float64|.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])

from tests.aspp_train_cases import ASPP_TRAIN_CASES, BN_FED_BIASES, sample_index  # noqa: E402
from tests.synth import synth_input, synth_state_dict  # noqa: E402
from nn_layers import aspp as ref_aspp  # noqa: E402

torch.set_num_threads(8)


def run(case, dtype):
    cls, ncls, shp, sd_seed, x_seed, g_seed = case
    m = getattr(ref_aspp, cls)(num_classes=ncls)
    m.load_state_dict(synth_state_dict(m.state_dict(), sd_seed))
    m = m.to(dtype).train()
    x = synth_input(shp, x_seed).to(dtype).requires_grad_(True)
    logits = m(x)
    G = synth_input(tuple(logits.shape), g_seed).to(dtype)
    (logits * G).sum().backward()
    q = {'logits': logits.detach(), 'gx': None, 'gx_chansum': x.grad.sum(1), 'gx_pixsum': x.grad.sum((0, 2, 3))}
    idx = sample_index('x', tuple(shp), x_seed)
    q['gx'] = x.grad.reshape(-1)[idx]
    for k, p in m.named_parameters():
        idx = sample_index(k, tuple(p.shape), sd_seed)
        q['g__' + k] = p.grad if idx is None else p.grad.reshape(-1)[idx]
        if p.dim() == 4 and p.shape[2] == 3:
            q['tapsum__' + k] = p.grad.sum((0, 1)).reshape(9)
            q['tapnorm__' + k] = p.grad.pow(2).sum((0, 1)).sqrt().reshape(9)
    for k, b in m.named_buffers():
        stem, _, leaf = k.rpartition('.')
        q[{'running_mean': 'rm__', 'running_var': 'rv__', 'num_batches_tracked': 'nbt__'}[leaf] + stem] = b.detach()
    return {k: v.detach().double().numpy() for k, v in q.items()}


def main():
    meta = {}
    for name, case in sorted(ASPP_TRAIN_CASES.items()):
        q64, q32 = run(case, torch.float64), run(case, torch.float32)
        meta[name] = {}
        for k in sorted(q64):
            if k.startswith('nbt__'):
                assert np.array_equal(q64[k], q32[k])
                continue
            scale = float(np.abs(q64[k]).max())
            if k.startswith('g__') and k[3:] in BN_FED_BIASES:
                meta[name][k] = {'abs': float(np.abs(q32[k]).max()), 'scale': scale}
            else:
                meta[name][k] = {'err': float(np.abs(q32[k] - q64[k]).max() / scale), 'scale': scale}
        path = os.path.join(HERE, 'aspp_train_%s.npz' % name)
        np.savez_compressed(path, **q64)
        print('wrote %s (%.1f KiB)' % (path, os.path.getsize(path) / 1024))
    with open(os.path.join(HERE, 'aspp_train.json'), 'w') as f:
        json.dump(meta, f, sort_keys=True, indent=1)


if __name__ == '__main__':
    main()
