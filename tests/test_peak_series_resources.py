"""The peak kernels keep their registers: ss_peak_series.hip cross-compiled for gfx950 with the resource-usage remark (device only,
no GPU needed), as tests/test_loudness_regions_resources.py does for the region gate — every form of k_peak_series, k_region_peaks
and k_group_peaks uses no scratch and spills nothing, and k_peak_series leaves room for four workgroups of 256 threads on a CU's
registers (128 VGPRs a lane) beside its static LDS."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

SERIES = ["k_peak_series<12, 3>", "k_peak_series<24, 1>", "k_peak_series<0, 0>"]


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_peak_series.hip"))


@pytest.mark.parametrize("name", SERIES + ["k_region_peaks", "k_group_peaks"])
def test_peak_kernels_use_no_scratch(kernels, name):
    assert name in kernels, sorted(kernels)
    x = kernels[name]
    assert int(x["ScratchSize [bytes/lane]"]) == 0 and int(x["VGPRs Spill"]) == 0 and int(x["SGPRs Spill"]) == 0, x


@pytest.mark.parametrize("name", SERIES)
def test_peak_series_fits_four_workgroups_a_cu(kernels, name):
    x = kernels[name]
    assert int(x["VGPRs"]) <= 128 and int(x["LDS Size [bytes/block]"]) <= 2 * 1024, x      # (static LDS: the words, the taps)
