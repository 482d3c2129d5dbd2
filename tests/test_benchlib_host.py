"""tools/benchlib.py without a device: the compile command it reads from the Makefile carries each file's own switches,
the remark parser's rows, and the two statistics the bench tools publish.  Nothing is compiled here: make runs dry."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib as BL  # noqa: E402


@pytest.mark.parametrize("source, has, lacks", [
    ("dpc_knn.hip", ["-ffp-contract=off"], ["-fno-slp-vectorize"]),
    ("dpc_chamfer.hip", ["-fno-slp-vectorize"], ["-ffp-contract=off"]),
    ("dpc_winding.hip", [], ["-ffp-contract=off", "-fno-slp-vectorize"]),
])
def test_compile_command_is_the_makefiles(source, has, lacks):
    argv = BL.compile_command(source)
    assert "--offload-arch=gfx950" in argv and argv[argv.index("-c") + 1] == source
    assert all(flag in argv for flag in has) and not any(flag in argv for flag in lacks)
    assert not any(arg.startswith("-Rpass") for arg in argv)


REMARKS = """\
dpc_x.hip:10:1: remark: Function Name: _Z9k_pm_fillPdi [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     TotalSGPRs: 10 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     VGPRs: 4 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:10:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:20:1: warning: unused variable 'n' [-Wunused-variable]
dpc_x.hip:30:1: remark: Function Name: _Z9k_pm_scanILi0EEvPi [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:30:1: remark:     TotalSGPRs: 49 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:30:1: remark:     VGPRs: 36 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:30:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:30:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:30:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:30:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:30:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:30:1: remark:     LDS Size [bytes/block]: 68 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark: Function Name: _ZN12_GLOBAL__N_15k_absEPf [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark:     TotalSGPRs: 102 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark:     VGPRs: 128 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark:     AGPRs: 16 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark:     ScratchSize [bytes/lane]: 24 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark:     Occupancy [waves/SIMD]: 3 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark:     SGPRs Spill: 2 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark:     VGPRs Spill: 6 [-Rpass-analysis=kernel-resource-usage]
dpc_x.hip:40:1: remark:     LDS Size [bytes/block]: 24576 [-Rpass-analysis=kernel-resource-usage]
"""


def test_usage_rows_of_three_kernels():
    """A plain kernel, a template instantiation (its `void` and its parameters dropped) and one in an anonymous namespace
    with spills; lines that are not resource remarks are passed over."""
    assert BL.usage_rows(REMARKS) == [
        "k_pm_fill                          vgpr=4    agpr=0    sgpr=10   sgpr_spill=0    vgpr_spill=0    scratch=0     occ=8  lds=0",
        "k_pm_scan<0>                       vgpr=36   agpr=0    sgpr=49   sgpr_spill=0    vgpr_spill=0    scratch=0     occ=8  lds=68",
        "k_abs                              vgpr=128  agpr=16   sgpr=102  sgpr_spill=2    vgpr_spill=6    scratch=24    occ=3  lds=24576",
    ]


def test_the_two_medians():
    assert BL.stats([3, 1, 2, 10]) == [2.5, 1, 10]            # np.median: the mean of the middle two
    assert BL.stats([1.23456, 1.0, 2.0], digits=2) == [1.23, 1.0, 2.0]
    assert BL.stats([1.23456], digits=None) == [1.23456] * 3
    assert BL.upper_median([1, 2, 3, 10]) == 3                # the event windows': the upper of the middle two
    assert BL.upper_median([5, 1, 3]) == 3


def test_share_of_a_peak():
    assert BL.share(4.0e9, 1.0, BL.HBM_PEAK, 4) == 0.5 and BL.share(4.0e9, None, BL.HBM_PEAK, 4) is None
