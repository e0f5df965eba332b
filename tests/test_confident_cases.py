"""The references of tests/confident_cases.py alone meet every condition tests/test_gpu_confident_logits.py relies on, so that a
failure there is the kernel's: the float32 oracle stays inside the project's loss / gradient bounds at these magnitudes, the centred
KL formula of labels.hip (restated in numpy float32) stays within 2x the float32 oracle's own error where the formula it replaced
exceeds 4x, and the label comparison leaves out less than its cap of near-ties."""
import numpy as np
import pytest

from tests import confident_cases as cc


@pytest.mark.parametrize('case', cc.grid(cc.FULL_SHAPES + cc.HEADS_SHAPES), ids=cc.grid_id)
def test_float32_oracle_loss_and_gradients_inside_the_project_bounds(case):
    r = cc.loss_case(case)
    l64, gp64, ga64 = r['ref64']
    l32, gp32, ga32 = r['ref32']
    lerr = cc.loss_error(l32, l64)
    errs = [cc.grad_errors(gp32, gp64), cc.grad_errors(ga32, ga64)]
    print('%s: loss %.9g, float32 error %.2e; gradients rel %.2e / %.2e, element %.2e / %.2e'
          % (cc.grid_id(case), l64, lerr, errs[0][0], errs[1][0], errs[0][1], errs[1][1]))
    assert lerr <= cc.LOSS_TAU
    assert max(e[0] for e in errs) <= cc.GRAD_TAU_REL and max(e[1] for e in errs) <= cc.GRAD_TAU_EL


@pytest.mark.parametrize('case', cc.grid(cc.KLD_SHAPES, heads=cc.HEADS), ids=cc.grid_id)
def test_float32_oracle_kld_gradients(case):
    r = cc.kld_case(case)
    errs = [cc.grad_errors(a, b) for a, b in zip(r['g32'], r['g64'])]
    top = max(float(g.abs().max()) for g in r['g64'])
    print('%s: float32 oracle gradients rel %.2e / %.2e, element %.2e / %.2e; largest float64 element %.2e, unit %.2e'
          % (cc.grid_id(case), errs[0][0], errs[1][0], errs[0][1], errs[1][1], top, r['grad_unit']))
    if case[2] == 'same':
        assert top <= 4e-6 and r['grad_unit'] <= 4e-6          # gradients of a KL that is zero: rounding of aux = pred + 3
    else:
        assert max(e[0] for e in errs) <= cc.GRAD_TAU_REL and max(e[1] for e in errs) <= cc.GRAD_TAU_EL


@pytest.mark.parametrize('mode', ['all', 'weights'])
@pytest.mark.parametrize('with_u', [True, False], ids=['u', 'nou'])
@pytest.mark.parametrize('case', cc.grid(cc.CE_SHAPES), ids=cc.grid_id)
def test_float32_oracle_weighted_ce(case, with_u, mode):
    r = cc.wce_case(case, with_u, mode)
    (n64, d64, gp64, gu64), (n32, d32, gp32, gu32) = r['ref64'], r['ref32']
    errs = [cc.grad_errors(gp32, gp64)] + ([cc.grad_errors(gu32, gu64)] if with_u else [])
    print('%s: sums %.9g / %.9g, float32 error %.2e / %.2e; gradients rel %s element %s'
          % (cc.grid_id(case), n64, d64, abs(n32 - n64) / n64, abs(d32 - d64) / d64, ['%.2e' % e[0] for e in errs], ['%.2e' % e[1] for e in errs]))
    assert abs(n32 - n64) <= cc.LOSS_TAU * n64 and abs(d32 - d64) <= 4 * 2.0 ** -23 * d64
    assert max(e[0] for e in errs) <= cc.GRAD_TAU_REL and max(e[1] for e in errs) <= cc.GRAD_TAU_EL


@pytest.mark.parametrize('case', cc.LABEL_CASES, ids=cc.label_case_id)
def test_kl_formulas_against_the_float32_oracle(case):
    """Centred formula: within 2x max(err32, 2**-22) of float64 on every case.  The formula labels.hip used before: beyond 4x on the
    `agree` and `same` cases at magnitudes of 8 and above without up-sampling (the construction of the measurement that motivated
    the change; 5x to 40x there, and 3.8x to 32x where both heads are up-sampled from one size.  With x2 / x4 heads of random
    per-pixel logits `agree` no longer means a small KL after the up-sampling, and the float32 interpolation weights alone move
    the KL by more than either formula)."""
    name, mag, heads = case
    pred, aux, size, ref = cc.label_case(case)
    unit = cc.kld_unit(ref)
    k64 = ref['kld64'].numpy()
    centred = float(np.abs(cc.kld_centred_f32(ref['main32'].numpy(), ref['aux32'].numpy()).astype(np.float64) - k64).max()) / unit
    raw = float(np.abs(cc.kld_raw_f32(ref['main32'].numpy(), ref['aux32'].numpy()).astype(np.float64) - k64).max()) / unit
    print('%s: err32 %.2e, KL up to %.3g; centred %.2f units, before %.2f units' % (cc.label_case_id(case), ref['err32'], k64.max(), centred, raw))
    assert centred <= 2.0
    if heads in ('agree', 'same') and mag >= 8 and cc.identity_size(name):
        assert raw > 4.0
    if heads == 'same':
        assert float(np.abs(k64).max()) <= cc.KLD_FLOOR          # the true KL of identical softmaxes (aux = pred + 3 rounds)


@pytest.mark.parametrize('case', cc.LABEL_CASES, ids=cc.label_case_id)
def test_label_comparison_leaves_out_less_than_its_cap(case):
    pred, aux, size, ref = cc.label_case(case)
    pixels = ref['sure'].numel()
    print('%s: %d of %d pixels within %g * magnitude of a tie' % (cc.label_case_id(case), ref['excluded'], pixels, cc.TIE_GAP_REL))
    assert ref['excluded'] <= cc.TIE_CAP * pixels


def test_generator_is_what_it_says():
    pred, aux, tgt = cc.confident_logits(2, 5, (16, 24), 20, 'agree', 0, ignore=255)
    win = pred.argmax(1)
    valid = tgt != 255
    assert 0.03 < float((~valid).float().mean()) < 0.07
    assert float((tgt[valid] == win[valid]).float().mean()) > 0.35           # chance is 0.2: the drawn winner leads by one sigma only
    assert float(pred.abs().max()) > 60 and float((aux - 0.8 * pred).abs().max()) < 0.3
    again = cc.confident_logits(2, 5, (16, 24), 20, 'agree', 0, ignore=255)
    assert all(bool((a == b).all()) for a, b in zip((pred, aux, tgt), again))
    p2, a2, t2 = cc.confident_logits(1, 5, (9, 22), 8, 'differ', 0, aux_size=(5, 11), target_size=(18, 44))
    assert a2.shape == (1, 5, 5, 11) and t2.shape == (1, 18, 44) and int(t2.min()) >= 0 and int(t2.max()) < 5
    ps, as_, _ = cc.confident_logits(1, 5, (4, 6), 40, 'same', 0)
    assert bool((as_ == ps + 3.0).all())
    with pytest.raises(AssertionError):
        cc.confident_logits(1, 5, (4, 6), 40, 'same', 0, aux_size=(2, 3))
