"""The gain kernels keep their registers: ss_apply_gain.hip cross-compiled for gfx950 with the resource-usage remark (device only, no
GPU needed), as tests/test_pair_series_resources.py does for the pair kernels — both forms of k_apply_gain and k_f32_to_pcm use no
scratch and spill nothing.  The sweep stages nothing (no LDS at all), and at 64 VGPRs or fewer a CU's registers hold eight
workgroups of 256 threads of the stereo form, the most its wave slots take."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

SWEEP = ["k_apply_gain<true>", "k_apply_gain<false>"]


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_apply_gain.hip"))


@pytest.mark.parametrize("name", SWEEP + ["k_f32_to_pcm"])
def test_gain_kernels_use_no_scratch(kernels, name):
    assert name in kernels, sorted(kernels)
    x = kernels[name]
    assert int(x["ScratchSize [bytes/lane]"]) == 0 and int(x["VGPRs Spill"]) == 0 and int(x["SGPRs Spill"]) == 0, x


def test_stereo_sweep_fills_the_wave_slots(kernels):
    x = kernels["k_apply_gain<true>"]
    assert int(x["VGPRs"]) <= 64 and int(x["LDS Size [bytes/block]"]) == 0, x
