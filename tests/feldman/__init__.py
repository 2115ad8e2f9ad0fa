"""Host (CPU) builds for the Feldman commitment evaluation: the evaluation
itself (feldman_host.cpp, for tests/test_feldman_host.py) and the workspace of
tbg_eval_commitments (work_host.cpp, for tests/test_feldman_abi.py).

TEST TOOLING ONLY -- see the two sources.  Built on demand with the ROCm
clang (host target); the evaluation with TBG_BOUNDS_CHECK, which aborts on any
violated value bound (as tests/ctmul does for the hardened signer's ladder),
the workspace walk as tests/plan builds its own (it only reads the HIP
headers' types).
"""
import ctypes

from tests import twin_build


def _signatures(h):
    p, u = ctypes.c_void_p, ctypes.c_uint32
    h.fvh_eval.restype = ctypes.c_int
    h.fvh_eval.argtypes = [p, p, u, p, p, u, p, p, p]
    h.fvh_mul.restype = ctypes.c_int
    h.fvh_mul.argtypes = [ctypes.c_char_p, u, p]


def _work_signatures(h):
    p, q = ctypes.c_void_p, ctypes.c_uint64
    h.fvw_max_sections.restype = ctypes.c_uint32
    h.fvw_max_sections.argtypes = []
    h.fvw_work.restype = ctypes.c_int
    h.fvw_work.argtypes = [q, q, q, q, p, p, p, p]


def build():
    twin_build.build("feldman_work")
    return twin_build.build("feldman")


def lib():
    return twin_build.lib("feldman", _signatures)


def work_lib():
    return twin_build.lib("feldman_work", _work_signatures)
