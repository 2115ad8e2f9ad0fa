"""Device (gfx950) unit harness for the H(m)-lines kernel's body (px_h_lines).

TEST TOOLING ONLY -- see devcheck_hlines.hip.  Built the way tests/devcheck
is: the engine's compiler and common flags plus the per-unit flags
charon_amd/_native.py gives k_verify.hip (the unit that holds k_lines_h),
checked by the same return-address guard, linked with a version script that
exports the dch_* entries only.  Never loaded by charon_amd.
"""
import ctypes

from tests import twin_build


def _signatures(L):
    L.dch_sticky_error.restype = ctypes.c_int
    L.dch_sticky_error.argtypes = []
    L.dch_lines.restype = ctypes.c_int
    L.dch_lines.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                            ctypes.c_uint32]


def build():
    """Compile the harness for gfx950 if the library is stale; raises without hipcc."""
    return twin_build.build("devcheck_hlines")


def lib():
    return twin_build.lib("devcheck_hlines", _signatures)
