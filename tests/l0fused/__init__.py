"""Host (CPU) build of the fused level 0's math, for tests/test_l0_fused_host.py.

TEST TOOLING ONLY -- see l0fused_host.cpp.  Built on demand with the ROCm
clang (host target) and TBG_BOUNDS_CHECK, which aborts on any violated value
bound (as tests/hostcheck does for the rest of the device math).
"""
from tests import twin_build


def build():
    return twin_build.build("l0fused")


def lib():
    return twin_build.lib("l0fused")
