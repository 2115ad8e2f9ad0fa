"""Host (CPU) build of level 0's message sums (bls_l0msg.h), for
tests/test_l0msg_host.py.

TEST TOOLING ONLY -- see l0msg_host.cpp.  Built on demand with the ROCm
clang (host target) and TBG_BOUNDS_CHECK, which aborts on any violated value
bound (as tests/hostcheck does for the rest of the device math).
"""
import ctypes

from tests import twin_build


def _signatures(h):
    p, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    h.lm_consts.restype = None
    h.lm_consts.argtypes = [p]
    h.lm_passes.restype = u
    h.lm_passes.argtypes = [u]
    h.lm_plan.restype = i
    h.lm_plan.argtypes = [p, p, p, u, p, p, p, p, p, p]
    h.lm_run.restype = i
    h.lm_run.argtypes = [ctypes.c_char_p, p, u, p, u, i, ctypes.c_char_p, p, ctypes.POINTER(i)]


def build():
    return twin_build.build("l0msg")


def lib():
    return twin_build.lib("l0msg", _signatures)
