"""The integer-operand harness (exactint.py) and the CPU-side conditions of
test_gpu_exact_integers.py's cases: the references are exact (2^24 bound, fp32 == fp64) and the
rounding cases discriminate - a truncating store, a double rounding and a bf16 half-K partial each
change at least 1 % of the expected elements.  No GPU: these are conditions on the inputs."""
import pytest
import torch

import exactint as E
import test_gpu_exact_integers as T


def test_rne_and_trunc_on_known_values():
    v = torch.tensor([256.0, 257.0, 258.0, 259.0, -257.0, -259.0, 513.0, 514.0, 515.0, 0.75])
    assert E.rne(v).tolist() == [256.0, 256.0, 258.0, 260.0, -256.0, -260.0, 512.0, 512.0, 516.0, 0.75]
    assert E.trunc(v).tolist() == [256.0, 256.0, 258.0, 258.0, -256.0, -258.0, 512.0, 512.0, 512.0, 0.75]
    c = E.bf16_census(v)
    assert c["inexact"] == pytest.approx(0.7)    # +-257, +-259, 513, 514, 515
    assert c["ties"] == pytest.approx(0.5)       # +-257, +-259 (spacing 2) and 514 (spacing 4)
    assert c["trunc_ne_rne"] == pytest.approx(0.3)                                   # 259, -259, 515


def test_bound_refuses_inexact_ranges():
    E.assert_exact_bound(4608, 4, 2)
    with pytest.raises(AssertionError):
        E.assert_exact_bound(4608, 64, 64)
    with pytest.raises(AssertionError):   # a reference that could not tell the wrong roundings apart
        E.assert_discriminates(E.ints((64, 64), 100, torch.Generator().manual_seed(0)))


def test_wrong_references_are_what_they_say():
    ref, add, half = torch.tensor([300.0, 301.0]), torch.tensor([-44.0, 1.0]), torch.tensor([257.0, 100.0])
    w = E.wrong_references(ref + add, half=half, addend=add)
    assert E.rne(ref + add).tolist() == [256.0, 302.0]
    assert w["double_rounded"].tolist() == [256.0, 300.0]    # bf16(301) = 300, + 1 = 301 -> 300 (tie to even)
    assert w["half_k_bf16"].tolist() == [255.0, 302.0]       # bf16(257) = 256: the sum loses one


_FWD_CASES = sorted({(r[0], r[2]) for r in T.FWD_ROWS})   # every distinct (shape, magnitudes), whatever the knobs


@pytest.mark.parametrize("shape,mags", _FWD_CASES, ids=lambda v: None)
def test_forward_rows_are_valid_and_discriminate(shape, mags):
    c = T.conv_case(shape, mags, rounding=shape in T.SPLITK, check64=shape == T.FWD_ROWS[0][0])
    assert float(c["y"].abs().max()) < E.LIMIT and float(c["dx"].abs().max()) < E.LIMIT
    assert min(c["census"][k]["inexact"] for k in ("y", "dx")) >= 0.01   # every row pins the store's rounding
    if shape in T.SPLITK:
        assert min(min(f.values()) for f in c["fractions"].values()) >= 0.01


@pytest.mark.parametrize("shape,mags,amag", T.MASKED_ROWS, ids=lambda v: None)
def test_addend_rows_discriminate_double_rounding(shape, mags, amag):
    for seed in (1, 2):
        assert T._addend_case(shape, mags, amag, seed)["fractions"]["double_rounded"] >= 0.01


@pytest.mark.parametrize("shape,mags", T.AFFINE_SHAPES, ids=lambda v: None)
def test_affine_rows_discriminate(shape, mags):
    p = T._affine_case(shape, mags, torch.device("cpu"))
    assert all(E.frac_ne(p["one"][k], p["two"][k]) >= 0.01 for k in T.AFF_CASES)
