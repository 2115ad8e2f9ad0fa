"""Device (gfx950) unit harness for the hexad's line steps (hex_line_at_v,
hex_line_folded).

TEST TOOLING ONLY -- see tests/devcheck/devcheck_hexline.hip, the kernel
file, which lives beside the other device unit kernels; this package builds
it into a library of its own.  Built the way tests/devcheck is: the engine's
compiler and common flags plus the per-unit flags charon_amd/_native.py gives
k_miller_hex.hip (the unit whose kernels run these steps most), checked by
the same return-address guard, linked with a version script that exports the
dcx_* entries only.  Never loaded by charon_amd.
"""
import ctypes

from tests import twin_build


def _signatures(L):
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.dcx_sticky_error.restype = ctypes.c_int
    L.dcx_sticky_error.argtypes = []
    L.dcx_hex_line.restype = ctypes.c_int
    L.dcx_hex_line.argtypes = [ctypes.c_int, u32p, u32p, u32p, u32p, ctypes.c_uint32, ctypes.c_uint32]


def build():
    """Compile the harness for gfx950 if the library is stale; raises without hipcc."""
    return twin_build.build("devcheck_hexline")


def lib():
    return twin_build.lib("devcheck_hexline", _signatures)
