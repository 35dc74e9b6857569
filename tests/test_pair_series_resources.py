"""The pair kernels keep their registers: ss_pair_series.hip cross-compiled for gfx950 with the resource-usage remark (device only,
no GPU needed), as tests/test_peak_series_resources.py does for the peak kernels — both forms of k_pair_series, k_region_pairs and
k_group_pairs use no scratch and spill nothing.  The series kernel stages nothing: its static LDS is the four waves' partial sums
(128 bytes), and at 64 VGPRs or fewer a CU's registers hold eight workgroups of 256 threads, the most its wave slots take (DESIGN.md
section 3.3.4)."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

SERIES = ["k_pair_series<true>", "k_pair_series<false>"]


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_pair_series.hip"))


@pytest.mark.parametrize("name", SERIES + ["k_region_pairs", "k_group_pairs"])
def test_pair_kernels_use_no_scratch(kernels, name):
    assert name in kernels, sorted(kernels)
    x = kernels[name]
    assert int(x["ScratchSize [bytes/lane]"]) == 0 and int(x["VGPRs Spill"]) == 0 and int(x["SGPRs Spill"]) == 0, x


@pytest.mark.parametrize("name", SERIES)
def test_pair_series_fills_the_wave_slots(kernels, name):
    x = kernels[name]
    assert int(x["VGPRs"]) <= 64 and int(x["LDS Size [bytes/block]"]) <= 128, x
