"""The spectrum-region kernels keep their registers: ss_spectrum_regions.hip cross-compiled for gfx950 with the resource-usage remark
(device only, no GPU needed), as tests/test_loudness_regions_resources.py does for the loudness regions — the three kernels use no
scratch and spill nothing, and k_spectrum_regions, whose loop is k_spectrum_stats' own, uses no LDS and holds as many waves per
SIMD as k_spectrum_stats does.  The kernel that reduces whole streams is the yardstick, so no number is fixed in advance:
ss_spectrum_stats.hip is compiled by the same function with the same flags in the same fixture.  (The region kernels have a file of
their own because tests/test_spectrum_stats_abi.py holds ss_spectrum_stats.hip to its three kernels; what the two files share is
ss_spectrum_stats_dev.h.)"""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

NEW = ["k_spectrum_regions", "k_spectrum_regions_combine", "k_spectrum_region_groups"]


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    regions, stats = dict(_resources("ss_spectrum_regions.hip")), dict(_resources("ss_spectrum_stats.hip"))
    assert sorted(regions) == sorted(NEW) and "k_spectrum_stats" in stats
    return {**stats, **regions}


@pytest.mark.parametrize("name", NEW)
def test_region_kernels_use_no_scratch(kernels, name):
    x = kernels[name]
    assert int(x["ScratchSize [bytes/lane]"]) == 0 and int(x["VGPRs Spill"]) == 0 and int(x["SGPRs Spill"]) == 0, x


def test_the_sweep_uses_no_lds_and_keeps_the_stats_kernels_occupancy(kernels):
    x, yardstick = kernels["k_spectrum_regions"], kernels["k_spectrum_stats"]
    print("k_spectrum_regions:", x, "\nk_spectrum_stats:", yardstick)
    assert int(x["LDS Size [bytes/block]"]) == 0, x
    assert int(x["Occupancy [waves/SIMD]"]) >= int(yardstick["Occupancy [waves/SIMD]"]), (x, yardstick)
