"""The label epilogue's geometries and kernel forms as a table, with the float64 reference every check compares against, and the
plain definition of the cross-source label merge.  Shared by tests/test_label_cases.py (no GPU) and tests/test_gpu_label_forms.py.
Nothing here touches the code under test (a helper, no tests).

The label epilogue (mspl_amd/csrc/labels.hip) has three kernel forms chosen by shape -- the general kernel, the register form and
the LDS-staged form with six class-count instantiations, two staging widths and compile-time strides for 480-wide outputs -- and
accepts any (Hm, Wm), (Ha, Wa) -> (H, W).  Each case names the form and the seam it is meant to reach; test_label_cases.py holds
the library's plan query to that, so a change of the launcher's rules that moves a case elsewhere fails there, not silently.

Reference, all float64 on the CPU: bilinear (align_corners=True) resize of both heads, o = main + 0.5 aux (o = main, KL = 0 with one
head), first-max argmax, optional id LUT, softmax probabilities, KL(main || aux) by log-softmax.  The same formulas in float32 on
the CPU give err32, each output's yardstick: |kernel - float64| <= MARGIN * max(err32, floor).

Label rule: a pixel is CLEAR when its float64 top-2 margin exceeds tau = max(1e-4 * max|o64|, 4 * max|o32 - o64|); on clear pixels
the label must equal the float64 argmax; at most UNCLEAR_CAP of a case's pixels may be unclear.  The second term of tau is there for
resizes by ratios float32 cannot hold (down-scaling 96 -> 40 rows: the float32 source position is off by 1e-6 of a pixel, the logits
by 2.4e-4).  The cap is a condition on the data: reference() walks SEEDS until the reference alone meets it."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import confident_cases as CC

MARGIN = 4                       # the margin of the softmax-family and pyramid audits (tests/test_gpu_confident_logits.py)
KLD_FLOOR, PROB_FLOOR = CC.KLD_FLOOR, CC.PROB_FLOOR
TAU_REL = 1e-4
UNCLEAR_CAP = 0.01
SEEDS = tuple(range(7, 7 + 8))   # seed 7 meets the cap for every case below; the walk is there for cases added later
LDS_64K = 64 * 1024

# shape: (N, C, Hm, Wm, Ha, Wa, H, W), Ha = Wa = 0: one head.  expect: what mspl_label_epilogue_plan must say for the labels / KL
# entry with aligned pointers (form, and for the LDS form vec, cmax, exact, wide480, big = more than 64 KB of LDS, any further
# field by name).  offset: the heads are views one float into a larger buffer (the pointers alone switch 16-byte staging off).
Case = collections.namedtuple('Case', 'name shape expect why offset', defaults=(False,))


def _lds(vec, cmax, exact, wide480=0, big=False, **more):
    return dict(form='lds', vec=vec, cmax=cmax, exact=exact, wide480=wide480, big=big, **more)


def _reg(cmax, **more):
    return dict(form='register', cmax=cmax, **more)


CASES = [
    Case('reg_same_res', (2, 5, 64, 300, 32, 150, 64, 300), _reg(8, colblocks=2, rowslots=64), 'register form, 2 column blocks, unaligned aux rows'),
    Case('reg_down', (1, 13, 96, 520, 48, 260, 40, 260), _reg(16, rowslots=40), 'register form, down-scaling, H % 4 == 0'),
    Case('reg_ragged_61', (2, 5, 64, 300, 32, 150, 61, 300), _reg(8, rowslots=64), "register form's padding row slots: 3"),
    Case('reg_ragged_62', (2, 5, 64, 300, 32, 150, 62, 300), _reg(8, rowslots=64), "register form's padding row slots: 2"),
    Case('reg_ragged_63', (2, 5, 64, 300, 32, 150, 63, 300), _reg(8, rowslots=64), "register form's padding row slots: 1"),
    Case('w257', (1, 13, 6, 257, 3, 129, 6, 257), _reg(16, colblocks=2), 'register form one column past the LDS limit'),
    Case('w256_edge', (1, 13, 6, 256, 3, 128, 6, 256), _lds(1, 13, 1, big=True, wms=256), 'LDS, wms = 256 (one pair per wave step), > 64 KB'),
    Case('lds_x3_odd', (2, 13, 11, 29, 6, 15, 31, 85), _lds(0, 13, 1, bands=8), 'LDS, 4-byte staging, x3, ragged last band'),
    Case('lds_nonint', (1, 20, 15, 70, 8, 35, 39, 181), _lds(0, 20, 1), 'LDS, EXACT<20>, non-integer ratio'),
    Case('lds_x8', (1, 5, 5, 33, 3, 17, 33, 257), _lds(0, 5, 1, colblocks=2), 'LDS, EXACT<5>, x8 (one source pair per band), second block of 1 column'),
    Case('lds_down2', (1, 5, 40, 64, 20, 32, 20, 32), _lds(1, 5, 1), 'LDS, down-scaling (rows skipped in a band)'),
    Case('same_res_small', (1, 13, 12, 100, 12, 100, 12, 100), _lds(1, 13, 1), 'LDS, ratio 1 for both heads'),
    Case('lds_1row', (1, 8, 1, 16, 1, 8, 7, 64), _lds(1, 8, 0, nrm=1, nra=1), 'one source row'),
    Case('lds_1col', (2, 16, 12, 1, 6, 1, 24, 1), _lds(0, 16, 0, wms=4, was=4), 'one source and output column'),
    Case('H1', (1, 13, 3, 40, 2, 20, 1, 80), _lds(1, 13, 1, bands=1, rowslots=4), 'one output row'),
    Case('wm_not4_aux4', (2, 13, 9, 30, 5, 16, 18, 60), _lds(0, 13, 1), 'main rows unaligned, aux rows aligned: 4-byte staging of both'),
    Case('unaligned_base', (1, 5, 40, 64, 20, 32, 20, 32), _lds(1, 5, 1), 'vec = 0 from the pointers alone', True),
    Case('wide480_c5', (1, 5, 10, 240, 5, 120, 19, 480), _lds(1, 5, 1, 1, wms=132, was=68), '<5, exact, 132, 68>, ragged last band'),
    Case('wide480_c13_1head', (1, 13, 6, 240, 0, 0, 12, 480), _lds(1, 13, 1, 1, wms=132), '<13, exact, 132, 68> with one head'),
    Case('wide480_c20_N3', (3, 20, 6, 240, 3, 120, 10, 478), _lds(1, 20, 1, 1, wms=132, was=68), '<20, exact, 132, 68>, W % 4 != 0, ragged last band'),
    Case('c24_two_blocks', (1, 24, 9, 130, 5, 65, 18, 260), _lds(0, 24, 0, big=True, wms=132, colblocks=2), '<24> with wms = 132 by rounding, > 64 KB'),
    Case('lds_big_64k', (1, 24, 24, 128, 12, 64, 48, 256), _lds(1, 24, 0, big=True), '> 64 KB tile, 16-byte staging'),
    Case('pairs_4080_1head', (1, 17, 240, 4, 0, 0, 2, 3), _lds(1, 24, 0, pairs_main=4080, pairs_aux=0),
         'largest pair index below the 4096 guard at the tightest C, one head'),
    Case('pairs_4080_2heads', (1, 17, 160, 4, 80, 4, 2, 3), _lds(1, 24, 0, pairs_main=2720, pairs_aux=1360),
         'the same 4080 pairs over two heads (the 4-byte staging decodes one index over both)'),
    Case('pairs_over', (1, 17, 700, 4, 350, 4, 13, 4), _reg(24), 'the 4096 guard sends it to the register form'),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
TRAINED = [(n, m) for n in ('lds_nonint', 'reg_down') for m in CC.TRAIN_MAGNITUDES]      # the second data set
CANARY = ('lds_x3_odd', 'lds_x8', 'w257', 'wide480_c20_N3')
SINGLE_HEAD = ('lds_x3_odd', 'reg_same_res', 'lds_nonint')      # LDS, register, and (with probabilities asked for) the general form
PLANES_P = (4, 8, 12, 16)


def two_heads(case):
    return case.shape[4] > 0


def lut_of(C):
    """An id LUT that maps several classes to one id (4 ids): a wrong class with the same id is all it can hide."""
    return [(3 * c + 1) % 4 for c in range(C)]


def upsample(t, size):
    return t if tuple(t.shape[-2:]) == tuple(size) else F.interpolate(t, size=tuple(size), mode='bilinear', align_corners=True)


def _formulas(main, aux, size):
    """The definition in the tensors' own precision: (main_up, aux_up or None, o, prob, kl)."""
    m = upsample(main, size)
    a = None if aux is None else upsample(aux, size)
    o = m if a is None else m + 0.5 * a
    kl = torch.zeros_like(o[:, 0])
    if a is not None:
        lm, la = F.log_softmax(m, 1), F.log_softmax(a, 1)
        kl = (lm.exp() * (lm - la)).sum(1)
    return m, a, o, F.softmax(o, 1), kl


def ulp32(v):
    return float(np.spacing(np.float32(v)))


def reference_of(main, aux, size):
    """main / aux: float32 CPU heads (aux may be None).  -> dict: float64 outputs, labels64 (first maximum), clear, unclear share,
    tau, err32 and bound per output.  Decided by the two CPU evaluations alone."""
    with torch.no_grad():
        m64, a64, o64, p64, k64 = _formulas(main.double(), None if aux is None else aux.double(), size)
        m32, a32, o32, p32, k32 = _formulas(main, aux, size)
    top = torch.sort(o64, dim=1, descending=True)[0]
    gap = top[:, 0] - top[:, 1] if o64.shape[1] > 1 else torch.full_like(top[:, 0], float('inf'))
    tau = max(TAU_REL * float(o64.abs().max()), 4 * float((o32.double() - o64).abs().max()))
    clear = gap > tau
    labels64 = torch.from_numpy(np.argmax(o64.numpy(), axis=1))            # np.argmax: the first maximum
    labels32 = torch.from_numpy(np.argmax(o32.numpy(), axis=1))
    err = {'kld': float((k32.double() - k64).abs().max()), 'prob': float((p32.double() - p64).abs().max()),
           'main_up': float((m32.double() - m64).abs().max()),
           'aux_up': 0.0 if a64 is None else float((a32.double() - a64).abs().max())}
    floor = {'kld': KLD_FLOOR, 'prob': PROB_FLOOR, 'main_up': ulp32(m64.abs().max()),
             'aux_up': 0.0 if a64 is None else ulp32(a64.abs().max())}
    return {'main_up': m64, 'aux_up': a64, 'o': o64, 'prob': p64, 'kld': k64, 'labels': labels64, 'labels32': labels32,
            'clear': clear, 'unclear': 1.0 - float(clear.double().mean()), 'tau': tau, 'err32': err,
            'bound': {k: MARGIN * max(err[k], floor[k]) for k in err}}


def _randn_heads(case, seed):
    N, C, Hm, Wm, Ha, Wa, H, W = case.shape
    g = torch.Generator().manual_seed(1000 * seed + NAMES.index(case.name))
    main = torch.randn(N, C, Hm, Wm, generator=g) * 2
    aux = torch.randn(N, C, Ha, Wa, generator=g) * 2 if two_heads(case) else None
    return main, aux


def _walk(make, size, what):
    for seed in SEEDS:
        main, aux = make(seed)
        ref = reference_of(main, aux, size)
        if ref['unclear'] <= UNCLEAR_CAP:
            return main, aux, ref, seed
    raise AssertionError('%s: no seed of %s keeps the unclear pixels under %g' % (what, SEEDS, UNCLEAR_CAP))


@functools.lru_cache(maxsize=None)
def problem(name, single_head=False):
    """(main, aux, size, reference, seed) of a case with `randn * 2` heads; computed once, shared, never modified."""
    case = BY_NAME[name]

    def make(seed):
        main, aux = _randn_heads(case, seed)
        return main, (None if single_head else aux)
    main, aux, ref, seed = _walk(make, case.shape[6:], name)
    return main, aux, tuple(case.shape[6:]), ref, seed


@functools.lru_cache(maxsize=None)
def trained_problem(name, magnitude):
    """The same for heads at a trained network's logit magnitudes (confident_cases.confident_logits, heads that agree)."""
    case = BY_NAME[name]
    N, C, Hm, Wm, Ha, Wa, H, W = case.shape

    def make(seed):
        return CC.confident_logits(N, C, (Hm, Wm), magnitude, 'agree', seed, aux_size=(Ha, Wa))[:2]
    main, aux, ref, seed = _walk(make, (H, W), '%s-m%d' % (name, magnitude))
    return main, aux, (H, W), ref, seed


def _classify(head):
    planes, w, b = head
    return torch.einsum('cp,nphw->nchw', w.flatten(1), planes) + b.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def planes_problem(name, P):
    """Heads as the P planes in front of their 1x1 classifier: N(0,1) planes, N(0,0.25) weights, N(0,1) bias (the distribution of
    tests/test_gpu_label_planes.py).  -> ((planes, weight, bias) per head, size, reference); the float64 logits come from the
    float64 planes, the float32 ones from a float32 classifier on the CPU."""
    case = BY_NAME[name]
    N, C, Hm, Wm, Ha, Wa, H, W = case.shape

    def heads(seed):
        g = torch.Generator().manual_seed(5000 * seed + 16 * NAMES.index(name) + P)
        r = lambda *s: torch.randn(*s, generator=g)
        main = (r(N, P, Hm, Wm), r(C, P, 1, 1) * 0.5, r(C))
        aux = (r(N, P, Ha, Wa), r(C, P, 1, 1) * 0.5, r(C)) if two_heads(case) else None
        return main, aux

    for seed in SEEDS:
        main, aux = heads(seed)
        with torch.no_grad():
            dbl = lambda h: None if h is None else _classify(tuple(t.double() for t in h))
            sgl = lambda h: None if h is None else _classify(h)
            r64 = _formulas(dbl(main), dbl(aux), (H, W))
            r32 = _formulas(sgl(main), sgl(aux), (H, W))
        o64, o32 = r64[2], r32[2]
        top = torch.sort(o64, dim=1, descending=True)[0]
        tau = max(TAU_REL * float(o64.abs().max()), 4 * float((o32.double() - o64).abs().max()))
        clear = (top[:, 0] - top[:, 1]) > tau
        unclear = 1.0 - float(clear.double().mean())
        if unclear <= UNCLEAR_CAP:
            err = float((r32[4].double() - r64[4]).abs().max())
            return main, aux, (H, W), {'labels': torch.from_numpy(np.argmax(o64.numpy(), axis=1)), 'clear': clear, 'unclear': unclear,
                                       'labels32': torch.from_numpy(np.argmax(o32.numpy(), axis=1)),
                                       'kld': r64[4], 'err32': {'kld': err}, 'bound': {'kld': MARGIN * max(err, KLD_FLOOR)}}
    raise AssertionError('%s P=%d: no seed keeps the unclear pixels under %g' % (name, P, UNCLEAR_CAP))


# ---------------------------------------------------------------------------------------------------------------- the merge
def merge_reference(src, ncls, thresh, fill):
    """mspl_merge_labels_fwd's contract in numpy.  src: (S, npix) uint8.  Per pixel the count of every class < ncls (labels >= ncls
    vote for nothing), the first maximum, `fill` where the winning count is < thresh; histogram of the output over classes < ncls."""
    src = np.asarray(src)
    counts = np.stack([(src == c).sum(axis=0) for c in range(ncls)])        # (ncls, npix)
    out = counts.argmax(axis=0).astype(np.uint8)                            # np.argmax: the first maximum
    out[counts.max(axis=0) < thresh] = fill
    return out, np.bincount(out, minlength=256)[:ncls].astype(np.int64)


MERGE_S = tuple(range(1, 9))
MERGE_NCLS = (5, 8, 9, 13, 16, 17, 21, 32)          # both sides of the NCLS = 8 / 16 / 32 instantiations
MERGE_FILL = (4, 255)                               # one the histogram counts, one it does not
MERGE_NPIX = (1, 15, 16, 17, 4099)
MERGE_BIG_NPIX = 16384 * 256 * 16 + 4099            # one chunk row past the 16384-workgroup cap: the only grid-stride case


def merge_thresholds(S):
    return sorted({1, (S + 1) // 2, S, S + 1})      # S + 1: everything is `fill`


def merge_sources(S, ncls, npix, seed=0):
    """(S, npix) uint8: uniform labels over the classes, 15 % labels outside them (ncls..255), and engineered ties every third pixel
    (the sources split evenly between a high and a low class, the high one first: the first maximum -- the LOWER class -- must win)."""
    rng = np.random.RandomState(977 * seed + 31 * S + ncls + npix % 1009)
    src = rng.randint(0, ncls, size=(S, npix)).astype(np.uint8)
    out = rng.rand(S, npix) < 0.15
    src[out] = rng.randint(ncls, 256, size=int(out.sum())).astype(np.uint8)
    if S >= 2:
        tie = np.arange(npix) % 3 == 0
        lo = rng.randint(0, ncls - 1, size=npix)
        hi = lo + 1 + rng.randint(0, ncls, size=npix) % (ncls - 1 - lo)
        for s in range(S - S % 2):                  # an even number of sources split in two; an odd last one keeps its random label
            src[s, tie] = (hi if s < (S - S % 2) // 2 else lo)[tie].astype(np.uint8)
    return src
