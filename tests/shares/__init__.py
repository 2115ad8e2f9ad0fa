"""Host (CPU) build of the share calls' workspace walk (work_host.cpp) for
tests/test_shares_abi.py.

TEST TOOLING ONLY -- see the source.  Built on demand with the ROCm clang
(host target), as tests/feldman builds its own walk: it only reads the HIP
headers' types.
"""
import ctypes

from tests import twin_build


def _signatures(h):
    p, q = ctypes.c_void_p, ctypes.c_uint64
    h.shw_max_sections.restype = ctypes.c_uint32
    h.shw_max_sections.argtypes = []
    h.shw_split.restype = ctypes.c_int
    h.shw_split.argtypes = [q, q, q, q, q, p, p, p, p, p, p, p]
    h.shw_combine.restype = ctypes.c_int
    h.shw_combine.argtypes = [q, q, q, p, p, p, p, p, p, p]
    h.shw_keyed_secret.restype = ctypes.c_int
    h.shw_keyed_secret.argtypes = [ctypes.c_int, q, q, p, p]


def build():
    return twin_build.build("shares")


def lib():
    return twin_build.lib("shares", _signatures)
