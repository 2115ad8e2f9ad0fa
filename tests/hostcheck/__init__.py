"""Host (CPU) build of the engine's device math, for the CPU test suite.

TEST TOOLING ONLY -- see hostcheck.cpp.  Built on demand with the ROCm clang
(host target) and TBG_BOUNDS_CHECK, which aborts on any violated value bound.
"""
from tests import twin_build


def build():
    return twin_build.build("hostcheck")


def lib():
    return twin_build.lib("hostcheck")
