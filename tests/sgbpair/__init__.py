"""Host (CPU) build of the batched subgroup test's paired schedule, for
tests/test_sgb_pair_host.py.

TEST TOOLING ONLY -- see sgbpair_host.cpp.  Built on demand with the ROCm
clang (host target) and TBG_BOUNDS_CHECK, which aborts on any violated value
bound (as tests/hostcheck does for the rest of the device math).
"""
import ctypes

from tests import twin_build


def _signatures(h):
    h.sp_code.restype = ctypes.c_uint32
    h.sp_code.argtypes = [ctypes.c_int32, ctypes.c_int32]
    h.sp_group.restype = ctypes.c_int
    h.sp_group.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                           ctypes.POINTER(ctypes.c_int), ctypes.c_char_p]
    h.sp_reference.restype = ctypes.c_int
    h.sp_reference.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p]


def build():
    return twin_build.build("sgbpair")


def lib():
    return twin_build.lib("sgbpair", _signatures)
