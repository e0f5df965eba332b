"""Case list of the decoder merge kernel's loop seams (mspl_amd/csrc/decoder_merge.hip) and the float64 formula the cases are
held to.  Shared by tests/test_decoder_merge_cases.py (CPU tier: the list reaches the forms it names) and
tests/test_gpu_decoder_merge_forms.py (the kernel against the formula).

The kernel walks the groups of the skip connection's grouped 3x3 with two named register buffers: the depthwise and the 4 -> 1
forms alternate them per group (an odd number of groups per wave leaves the two-step loop after its first step), the 8 -> 3 form
alternates them per pair of input channels inside a group.  SPLIT = 4 gives each of a workgroup's four waves a quarter of the
groups.  Rows wider than 128 columns are cut into column blocks, whose edge lanes load their halo column (a form of its own).
Every case names the form, the SPLIT and the groups per wave it is meant to reach; the CPU tier recomputes them from the
launcher's rules.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

EDGE_REL = 1e-5          # tests/test_gpu_decoder_merge.py: (64 + 16) * 2^-23 of the largest |value|

Case = collections.namedtuple('Case', 'name N Cin Cout P H W form split gpw gate seed')

FORMS = {(1, 1): 'dw', (8, 3): '8to3', (4, 1): '4to1'}


def _base():
    out = []

    def add(form, cin, cout, h, w, split, gpw, P=16, gate=None, tag=''):
        name = '%s_%dto%d_%dx%d_P%d%s' % (form, cin, cout, h, w, P, tag)
        out.append(Case(name, 3, cin, cout, P, h, w, form, split, gpw, gate, 5000 + len(out)))

    # depthwise, one wave per tile: 1, 2, 3, 5 groups (odd and even trip counts, the shortest ones included); 4x132 is two
    # column blocks of 33 lanes: edge-lane loads, dead lanes inside the second block
    for h, w in ((8, 60), (4, 132)):
        for c in (1, 2, 3, 5):
            add('dw', c, c, h, w, 1, c)
    # depthwise, four waves per tile (small map, G % 4 == 0): 1, 3, 2 groups per wave
    for c, gpw in ((4, 1), (12, 3), (8, 2)):
        add('dw', c, c, 6, 20, 4, gpw)
    # 8 -> 3, four waves per tile: 1, 3, 4 groups per wave (the last in two column blocks)
    add('8to3', 32, 12, 8, 60, 4, 1)
    add('8to3', 96, 36, 8, 60, 4, 3)
    add('8to3', 128, 48, 4, 132, 4, 4)
    # 8 -> 3, one wave per tile (G % 4 != 0): 5 groups in one wave
    add('8to3', 40, 15, 8, 60, 1, 5)
    # 4 -> 1, four waves per tile: 4 and 5 groups per wave
    for h, w in ((4, 16), (6, 60)):
        add('4to1', 64, 16, h, w, 4, 4)
        add('4to1', 80, 20, h, w, 4, 5)
    # 4 -> 1, one wave per tile: 17 groups
    add('4to1', 68, 17, 4, 16, 1, 17)
    # 4 -> 1 in two column blocks (the edge-lane form of the four-channel fetch)
    add('4to1', 80, 20, 4, 132, 4, 5)
    # plane counts on one odd-trip case of each form
    for P in (2, 6, 10):
        add('dw', 3, 3, 8, 60, 1, 3, P=P)
        add('8to3', 96, 36, 8, 60, 4, 3, P=P)
        add('4to1', 80, 20, 4, 16, 4, 5, P=P)
    # gate 0 and 1 on one case of each form (the random gate is every other case)
    for gate in (0.0, 1.0):
        add('dw', 5, 5, 4, 132, 1, 5, gate=gate, tag='_gate%d' % gate)
        add('8to3', 96, 36, 8, 60, 4, 3, gate=gate, tag='_gate%d' % gate)
        add('4to1', 80, 20, 6, 60, 4, 5, gate=gate, tag='_gate%d' % gate)
    return out


CASES = _base()
IDS = [c.name for c in CASES]


def geometry(c):
    """The launcher's plan for a case (decoder_merge_try / dm_launch): group shape, lanes per row pair, column blocks, waves per
    (image, column block), SPLIT and groups per wave; 'fused' is False where the library declines the shape."""
    G = math.gcd(c.Cin, c.Cout)
    cg, cob = c.Cin // G, c.Cout // G
    fused = c.H % 2 == 0 and c.W % 2 == 0 and c.H >= 2 and c.W >= 2 and c.P in (2, 6, 10, 16) and c.Cout <= 1024
    fused = fused and ((cg, cob) in ((1, 1), (8, 3))
                       or ((cg, cob) == (4, 1) and G >= 16 and c.W % 4 == 0 and 16 <= c.W <= 256 and c.H >= 4))
    lprt = c.W // 2
    ncb = -(-lprt // 64)
    lpr = -(-lprt // ncb)
    sub = 64 // lpr
    rpw = -(-(c.H // 2) // sub)
    split = 4 if (cg > 1 or ncb * rpw < 64) and G % 4 == 0 else 1
    return dict(cg=cg, cob=cob, G=G, ncb=ncb, lpr=lpr, sub=sub, rpw=rpw, split=split, gpw=G // split, fused=fused)


def inputs(c, N=None):
    """Inputs of a case, generated as tests/test_gpu_decoder_merge.py::_inputs does (slopes and BN constants of both signs)."""
    N = c.N if N is None else N
    g = torch.Generator().manual_seed(c.seed)
    groups = math.gcd(c.Cin, c.Cout)

    def rn(*shape, s=1.0):
        return torch.randn(*shape, generator=g) * s
    d = {
        'enc': rn(N, c.Cin, c.H, c.W), 'bu': rn(N, c.Cout, c.H // 2, c.W // 2),
        'w3': rn(c.Cout, c.Cin // groups, 3, 3, s=1.0 / math.sqrt(9 * c.Cin // groups)),
        'es': rn(c.Cout), 'eb': rn(c.Cout, s=0.5), 'ea': rn(c.Cout, s=0.5),
        'bs': rn(c.Cout), 'bb': rn(c.Cout, s=0.5), 'ba': rn(c.Cout, s=0.5),
        'wp': rn(c.P, c.Cout, s=1.0 / math.sqrt(c.Cout)),
        'ps': rn(c.P), 'pb': rn(c.P, s=0.5), 'pa': rn(c.P, s=0.5),
    }
    if c.gate is None:
        d['gate'] = torch.sigmoid(rn(N, c.Cout))
    else:
        d['gate'] = torch.full((N, c.Cout), float(c.gate))
    return d, groups


def _prelu(v, alpha):
    return torch.where(v > 0, v, v * alpha.view(1, -1, 1, 1))


def formula(d, groups, dtype=torch.float64):
    """proj = prelu(bn(Wp . prelu(bn(gate * prelu(bn(grouped3x3(enc))) + bilinear2x(bu))))) in the given precision."""
    t = {k: v.to(dtype) for k, v in d.items()}
    H, W = t['enc'].shape[2:]
    pw = F.conv2d(t['enc'], t['w3'], padding=1, groups=groups)
    pw = _prelu(pw * t['es'].view(1, -1, 1, 1) + t['eb'].view(1, -1, 1, 1), t['ea']) * t['gate'][:, :, None, None]
    up = F.interpolate(t['bu'], size=(H, W), mode='bilinear', align_corners=True)
    m = _prelu((pw + up) * t['bs'].view(1, -1, 1, 1) + t['bb'].view(1, -1, 1, 1), t['ba'])
    pr = torch.einsum('pc,nchw->nphw', t['wp'], m)
    return _prelu(pr * t['ps'].view(1, -1, 1, 1) + t['pb'].view(1, -1, 1, 1), t['pa'])


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(inputs, groups, float64 reference) of a case: computed once, shared by every test that needs it, never modified."""
    c = CASES[IDS.index(name)]
    d, groups = inputs(c)
    return d, groups, formula(d, groups)
