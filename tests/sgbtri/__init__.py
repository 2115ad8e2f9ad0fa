"""Host (CPU) build of the batched subgroup test's triple schedule, for
tests/test_sgb_tri_host.py.

TEST TOOLING ONLY -- see sgbtri_host.cpp.  Built on demand with the ROCm
clang (host target) and TBG_BOUNDS_CHECK, which aborts on any violated value
bound (as tests/hostcheck does for the rest of the device math).
"""
import ctypes

from tests import twin_build


def _signatures(h):
    h.st_code.restype = ctypes.c_uint32
    h.st_code.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    h.st_group.restype = ctypes.c_int
    h.st_group.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                           ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    h.st_reference.restype = ctypes.c_int
    h.st_reference.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p]


def build():
    return twin_build.build("sgbtri")


def lib():
    return twin_build.lib("sgbtri", _signatures)
