"""The region kernels keep their registers: ss_loudness.hip cross-compiled for gfx950 with the resource-usage remark (device only,
no GPU needed), as tests/test_kernel_resources.py does for the time-domain and spectrum files — k_region_gate and k_group_eval use
no scratch, and k_region_gate's 1024-thread workgroup fits its register budget."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_loudness.hip"))


@pytest.mark.parametrize("name", ["k_region_gate", "k_group_eval"])
def test_region_kernels_use_no_scratch(kernels, name):
    assert name in kernels, sorted(kernels)
    x = kernels[name]
    assert int(x["ScratchSize [bytes/lane]"]) == 0 and int(x["VGPRs Spill"]) == 0 and int(x["SGPRs Spill"]) == 0, x


def test_region_gate_fits_a_1024_thread_workgroup(kernels):
    x = kernels["k_region_gate"]
    assert int(x["VGPRs"]) <= 128 and int(x["LDS Size [bytes/block]"]) <= 17 * 1024, x
