"""The grouped aggregates (csrc/kernels/agg.hip) through each of their five
regimes -- single group, LDS, sorted runs, global atomics, radix-partitioned --
against tests/groupby_ref.py: every operator in launches of eight aggregates
and of one, with and without a validity mask, over int64 and int32 extremes
(sums crossing 2^63 and 2^64 both ways, MIN / MAX equal to the states'
identities, sign-extended bit operations), non-finite and denormal f64, NaN of
either sign under MIN / MAX, group ids outside [0, ngroups), empty and
all-NULL groups. Integers compare exactly, f64 MIN / MAX as values, an f64 SUM
within the any-order bound gamma_(t-1) * sum|x|. The checker asserts the regime
from the kernels' own thresholds. Cases live in tests/groupby_cases.py
(tests/test_groupby_ref.py runs them on the torch CPU path). Runs on a real
MI355X."""
import pytest

import groupby_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("nagg", [8, 1])
@pytest.mark.parametrize("regime", C.REGIMES)
def test_grouped_aggregate_edges(gpu_device, regime, nagg, masked, monkeypatch):
    C.check_agg(regime, nagg, masked, gpu_device, monkeypatch)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_having_general_kernel_edges(gpu_device, masked, monkeypatch):
    """The run-folding sorted_having_kernel has a fold path of its own: the
    sorted regime's rows, their group ids as keys, every operator."""
    C.check_having_general(masked, gpu_device, monkeypatch)
