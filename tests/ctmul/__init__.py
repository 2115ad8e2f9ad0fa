"""Host (CPU) build of the hardened signer's ladder, for tests/test_ctmul_host.py.

TEST TOOLING ONLY -- see ctmul_host.cpp.  Built on demand with the ROCm
clang (host target) and TBG_BOUNDS_CHECK, which aborts on any violated value
bound (as tests/l0tail does for the fused level 0's S role).
"""
from tests import twin_build


def build():
    return twin_build.build("ctmul")


def lib():
    return twin_build.lib("ctmul")
