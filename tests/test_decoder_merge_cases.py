"""CPU tier of the decoder merge kernel's seam cases (tests/decoder_merge_cases.py): the list reaches the kernel forms, SPLIT
values and trip-count parities it names, by the launcher's own rules, and the yardstick is sound for the cases' seeds: a plain
fp32 evaluation of the formula with torch on the CPU stays within EDGE_REL of the float64 one.
"""
import math

import pytest
import torch

from tests import decoder_merge_cases as dmc


@pytest.mark.parametrize('name', dmc.IDS)
def test_case_reaches_its_form(name):
    c = dmc.CASES[dmc.IDS.index(name)]
    g = dmc.geometry(c)
    assert g['fused'], 'every listed case is a fused shape'
    assert dmc.FORMS[(g['cg'], g['cob'])] == c.form                 # gcd(Cin, Cout) gives the (CG, COB) pair
    # the launcher's SPLIT rule: (CG > 1 or ncb * rpw < 64) and G % 4 == 0
    assert g['split'] == (4 if (g['cg'] > 1 or g['ncb'] * g['rpw'] < 64) and g['G'] % 4 == 0 else 1) == c.split
    assert g['G'] % g['split'] == 0
    assert g['gpw'] == c.gpw and g['gpw'] % 2 == c.gpw % 2          # groups per wave: the stated count and parity
    assert c.N == 3 and c.H <= 16


def test_list_covers_every_seam():
    seen = {(c.form, c.split, c.gpw % 2) for c in dmc.CASES}
    for form in ('dw', '8to3', '4to1'):
        for split in (1, 4):
            assert (form, split, 1) in seen, (form, split, 'odd')
        assert any(c.form == form and c.gpw % 2 == 0 for c in dmc.CASES), (form, 'even')
        assert {c.P for c in dmc.CASES if c.form == form} == {2, 6, 10, 16}
        assert {c.gate for c in dmc.CASES if c.form == form} == {None, 0.0, 1.0}
        assert any(c.form == form and dmc.geometry(c)['ncb'] > 1 for c in dmc.CASES), (form, 'column blocks')
    assert {c.gpw for c in dmc.CASES if c.form == 'dw' and c.split == 1} == {1, 2, 3, 5}
    assert len(set(dmc.IDS)) == len(dmc.IDS) and len({c.seed for c in dmc.CASES}) == len(dmc.CASES)


def test_shapes_outside_the_fused_set_are_planned_as_declined():
    c = dmc.CASES[0]
    assert not dmc.geometry(c._replace(Cin=64, Cout=48))['fused']          # 4 -> 3 groups
    assert not dmc.geometry(c._replace(P=32))['fused']
    assert not dmc.geometry(c._replace(Cin=64, Cout=16, W=18))['fused']    # 4 -> 1 needs W % 4 == 0
    assert not dmc.geometry(c._replace(Cin=32, Cout=8, W=16, H=4))['fused']  # 4 -> 1 needs 16 groups


def test_inputs_are_those_of_the_existing_test():
    from tests import test_gpu_decoder_merge as ref
    for c in dmc.CASES[::5]:
        mine, groups = dmc.inputs(c)
        theirs, groups2 = ref._inputs(c.N, c.Cin, c.Cout, c.P, c.H, c.W, c.seed, c.gate)
        assert groups == groups2 == math.gcd(c.Cin, c.Cout)
        for k in theirs:
            assert torch.equal(mine[k], theirs[k]), k
        assert torch.equal(dmc.formula(mine, groups), ref._ref64(theirs, groups2))


@pytest.mark.parametrize('name', dmc.IDS)
def test_fp32_restatement_within_bound(name):
    d, groups, ref = dmc.case_data(name)
    got = dmc.formula(d, groups, torch.float32)
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    print('%s: fp32 restatement %.3e of max |ref| = %.3f' % (name, err / scale, scale))
    assert scale > 0 and err <= dmc.EDGE_REL * scale
