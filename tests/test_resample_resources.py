"""The resampler's kernels keep their registers: ss_resample.hip cross-compiled for gfx950 with the resource-usage remark (device
only, no GPU needed), as tests/test_apply_gain_resources.py does for the gain kernels — no instantiation of k_resample* uses scratch
or spills.  The register-taps form holds a phase's taps per lane: up to 80 of them within 128 VGPRs (four waves per SIMD), up to 128
within 168 (three)."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

EXPECTED = ["k_resample_reg<80, 1>", "k_resample_reg<80, 2>", "k_resample_reg<128, 1>", "k_resample_reg<128, 2>",
            "k_resample_lds<1>", "k_resample_lds<2>", "k_resample_lds<0>", "k_resample_direct"]


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_resample.hip"))


def test_every_instantiation_is_listed(kernels):
    assert sorted(k for k in kernels if k.startswith("k_resample")) == sorted(EXPECTED)


@pytest.mark.parametrize("name", EXPECTED)
def test_resample_kernels_use_no_scratch(kernels, name):
    x = kernels[name]
    assert int(x["ScratchSize [bytes/lane]"]) == 0 and int(x["VGPRs Spill"]) == 0 and int(x["SGPRs Spill"]) == 0, x


def test_register_taps_keep_their_occupancy(kernels):
    for name, most in (("k_resample_reg<80, 1>", 128), ("k_resample_reg<80, 2>", 128), ("k_resample_reg<128, 1>", 168), ("k_resample_reg<128, 2>", 168)):
        assert int(kernels[name]["VGPRs"]) <= most, (name, kernels[name])
