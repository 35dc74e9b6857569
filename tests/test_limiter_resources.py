"""The limiter kernels keep their registers: ss_limiter.hip cross-compiled for gfx950 with the resource-usage remark (device only,
no GPU needed), as tests/test_apply_gain_resources.py does for the gain kernels — every instantiation of k_limit_detect and
k_limit_apply uses no scratch and spills nothing.  The detector's static LDS is the tile's r_q words and a few words beside them;
the sweep's LDS is all dynamic (the curve form's reach, sized per call), so its static part stays a few words (DESIGN.md section
3.3.6)."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

DETECT = ["k_limit_detect<12, 3>", "k_limit_detect<24, 1>", "k_limit_detect<0, 0>"]
APPLY = ["k_limit_apply<true>", "k_limit_apply<false>"]


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_limiter.hip"))


def test_every_instantiation_is_there(kernels):
    assert sorted(kernels) == sorted(DETECT + APPLY), sorted(kernels)


@pytest.mark.parametrize("name", DETECT + APPLY)
def test_limiter_kernels_use_no_scratch(kernels, name):
    assert name in kernels, sorted(kernels)
    x = kernels[name]
    assert int(x["ScratchSize [bytes/lane]"]) == 0 and int(x["VGPRs Spill"]) == 0 and int(x["SGPRs Spill"]) == 0, x


def test_static_lds(kernels):
    for name in DETECT:
        assert 4096 * 4 <= int(kernels[name]["LDS Size [bytes/block]"]) <= 4096 * 4 + 256, (name, kernels[name])
    for name in APPLY:
        assert int(kernels[name]["LDS Size [bytes/block]"]) <= 64, (name, kernels[name])
