"""Shape rules of the DownSampler head launch (mspl_down_head_fits / mspl_down_head_psum_blocks): host-side logic, no GPU."""
import os

import pytest

from mspl_amd import _native as nat
from mspl_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (nin, n) of level2_0 / level3_0 / level4_0 of ESPDNet(-UE) s = 2.0 and their input sizes for 288x480, 256x480 and 512x1024 images
@pytest.mark.parametrize('nin,n,sizes,fits', [
    (32, 24, ((144, 240), (128, 240), (256, 512)), True),
    (128, 32, ((72, 120), (64, 120), (128, 256)), True),
    (256, 64, ((36, 60), (32, 60), (64, 128)), False),          # 16 reduced channels per group: today's launches
])
def test_bench_shapes(nin, n, sizes, fits):
    for H, W in sizes:
        for N in (1, 16):
            assert ops.down_head_fits((N, nin, H, W), n, 4) == fits


@pytest.mark.parametrize('shape,n,groups', [
    ((2, 128, 8, 44), 32, 4),          # a 352-pixel-wide image at level 3: rows off the 8-column strip grid
    ((2, 32, 37, 240), 24, 4),         # odd height
    ((2, 32, 16, 244), 24, 4),
    ((2, 32, 16, 240), 24, 2),         # other group counts
    ((2, 32, 16, 240), 16, 4),         # 4 reduced channels per group
    ((2, 512, 16, 240), 32, 4),        # 128 input channels per group
    ((2, 32, 0, 240), 24, 4),
])
def test_rejected(shape, n, groups):
    assert not ops.down_head_fits(shape, n, groups)


def test_does_not_depend_on_batch_or_launch_flags():
    for N in (1, 2, 16, 64):
        with ops.launch_flags(throughput=True):
            assert ops.down_head_fits((N, 32, 144, 240), 24, 4)
        assert ops.down_head_fits((N, 32, 144, 240), 24, 4)


@pytest.mark.parametrize('H,W', [(144, 240), (72, 120), (256, 512), (128, 256), (6, 520), (10, 24)])
def test_psum_blocks_match_the_pool_launch(H, W):
    """Same strip split as mspl_avgpool3x3s2_psum_fwd: one slot per 256 strips of four pooled outputs."""
    want = -(-((H // 2) * (W // 8)) // 256)
    assert nat.lib.mspl_down_head_psum_blocks(H, W) == want
    assert nat.lib.mspl_avgpool3x3s2_psum_blocks(H, W) == want


def test_psum_blocks_rejects_what_fits_rejects():
    assert nat.lib.mspl_down_head_psum_blocks(37, 240) < 0
    assert nat.lib.mspl_down_head_psum_blocks(16, 244) < 0


def test_declared_in_the_header():
    text = open(os.path.join(ROOT, 'include', 'mspl_hip.h')).read()
    for name in ('mspl_down_head_fits', 'mspl_down_head_psum_blocks', 'mspl_down_head_fwd'):
        assert name in nat.SIGNATURES and ('int %s(' % name) in text
