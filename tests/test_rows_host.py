"""The threshold rows of test_rows_bits_gpu.py are what they claim (tests/_rows_cases.py), shown in numpy without a GPU:
`fires` rows meet tiny * 8 == nonzero exactly, `holds` rows stay 16 below it with two entries at exactly 0.5 once scaled, and
each of the slips the GPU cases are meant to catch would flip the guard's answer on one of the two rows."""

import numpy as np
import pytest

from _rows_cases import EDGE, FAR, KINDS, WIDTHS, guard_counts, guard_fires, threshold_row


@pytest.mark.parametrize("signed", (False, True))
@pytest.mark.parametrize("d", WIDTHS)
def test_threshold_rows_meet_the_rule_exactly(d, signed):
    fires, holds = (threshold_row(d, k, signed) for k in KINDS)
    tiny, nz = guard_counts(fires)
    assert tiny > 0 and tiny * 8 == nz and guard_fires(fires)
    assert d - nz >= 8 and int((fires == 0).sum()) == d - nz          # zeros are there to be (wrongly) counted
    tiny_h, nz_h = guard_counts(holds)
    assert nz_h == nz and tiny_h == tiny - 2 and tiny_h * 8 < nz and not guard_fires(holds)
    assert int((np.abs(holds) == EDGE).sum()) == 2 and int((np.abs(fires) == FAR).sum()) == tiny
    assert float(np.abs(fires).max()) == float(np.abs(holds).max()) == 1.0


@pytest.mark.parametrize("d", WIDTHS)
def test_each_slip_flips_one_of_the_rows(d):
    fires, holds = (threshold_row(d, k) for k in KINDS)
    tiny, nz = guard_counts(fires)
    assert not tiny * 8 > nz                                          # `>` for `>=`: the fires row no longer fires
    assert not tiny * 8 >= d                                          # zeros counted as nonzero: neither
    xs = np.abs(holds) * np.float32(2.0 ** 13)
    tiny_le = int(((xs != 0) & (xs <= np.float32(0.5))).sum())        # `<= 0.5` for `< 0.5`: the holds row fires
    assert tiny_le == tiny and tiny_le * 8 >= nz


@pytest.mark.parametrize("d", WIDTHS)
def test_signed_rows_sum_to_zero_in_every_aligned_group_of_four(d):
    for kind in KINDS:
        row = threshold_row(d, kind, signed=True)
        assert d % 4 == 0 and not row.reshape(-1, 4).sum(axis=1).any()
        assert np.array_equal(np.abs(row), threshold_row(d, kind))
