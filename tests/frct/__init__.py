"""Host (CPU) builds of the fixed-schedule Fr arithmetic (charon_amd/csrc/bls_frct.h)
for tests/test_frct_host.py: the shared library (frct_host.cpp) and the
stand-alone sanitizer program (frct_main.cpp, its own main()).

TEST TOOLING ONLY -- see the two sources.  Built on demand with the ROCm
clang (host target); the library with TBG_BOUNDS_CHECK as tests/ctmul builds
its own, the program with -fsanitize=address,undefined.  The program is run
as a subprocess: nothing sanitized is loaded into Python.
"""
import ctypes

from tests import twin_build


def _signatures(h):
    p, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    h.frh_ops.restype = i
    h.frh_ops.argtypes = [i, p, p, u, p]
    h.frh_horner.restype = i
    h.frh_horner.argtypes = [p, u, u, p, p, p]
    h.frh_combine.restype = i
    h.frh_combine.argtypes = [p, p, u, p, p]
    h.frh_count_kinds.restype = u
    h.frh_count_kinds.argtypes = []
    h.frh_count_op.restype = i
    h.frh_count_op.argtypes = [i, p, p, p, p]
    h.frh_count_horner.restype = i
    h.frh_count_horner.argtypes = [p, u, u, p, p, p, p]
    h.frh_count_combine.restype = i
    h.frh_count_combine.argtypes = [p, p, u, p, p, p]


def build():
    return twin_build.build("frct")


def build_sanitized():
    """The stand-alone program under AddressSanitizer and UBSan (host code only)."""
    return twin_build.build("frct_main")


def lib():
    return twin_build.lib("frct", _signatures)
