"""Host (CPU) build of the fused level 0's per-duty key side, for
tests/test_l0_straus_host.py.

TEST TOOLING ONLY -- see l0straus_host.cpp.  Built on demand with the ROCm
clang (host target) and TBG_BOUNDS_CHECK, which aborts on any violated value
bound (as tests/hostcheck does for the rest of the device math).
"""
import ctypes

from tests import twin_build


def _signatures(h):
    p, i = ctypes.c_void_p, ctypes.c_int
    h.ls_digits.restype = None
    h.ls_digits.argtypes = [p, ctypes.c_uint32, p]
    h.ls_duty.restype = i
    h.ls_duty.argtypes = [ctypes.c_char_p, i, p, p, p, i, i, ctypes.POINTER(i), ctypes.c_char_p]
    h.ls_reference.restype = i
    h.ls_reference.argtypes = [ctypes.c_char_p, i, p, p, p, i, ctypes.c_char_p]


def build():
    return twin_build.build("l0straus")


def lib():
    return twin_build.lib("l0straus", _signatures)
