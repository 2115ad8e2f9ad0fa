"""Host (CPU) build of the hexad's direct line product, for
tests/test_hex_line_direct_host.py.

TEST TOOLING ONLY -- see hexline_host.cpp.  Built on demand with the ROCm
clang (host target) and TBG_BOUNDS_CHECK, which aborts on any violated value
bound (as tests/hostcheck does for the rest of the device math).
"""
from tests import twin_build


def build():
    return twin_build.build("hexline")


def lib():
    return twin_build.lib("hexline")
