"""Host (CPU) build of the launch plan and the arena section table
(charon_amd/csrc/tbls_plan.h) and of the one-shot calls' workspaces
(tbls_work.h), for tests/test_plan_host.py, and of the fallback lists' pass
schedule and grid-stride loops (tbls_launch.h), for tests/test_fb_passes_host.py.

TEST TOOLING ONLY -- see plan_host.cpp.  Built on demand with the ROCm clang
(host target); the header makes no HIP runtime call, it only reads the HIP
headers' types.
"""
import ctypes

from tests import twin_build


def _signatures(h):
    p, i, u, q, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    h.pl_max_sections.restype = u
    h.pl_max_sections.argtypes = []
    h.pl_layout.restype = i
    h.pl_layout.argtypes = [p, u, q, p, u, p, u, p, p, p, p]
    h.pl_bind.restype = i
    h.pl_bind.argtypes = [p, u, q, p, u, p, u, q, q, q, p, p, p]
    h.pl_shape_fits.restype = i
    h.pl_shape_fits.argtypes = [u, u, u, u, u, u]
    h.pl_l0_shape.restype = None
    h.pl_l0_shape.argtypes = [q, u, i, u, u, u, u, p, u, p]
    h.pl_sgb_plan.restype = i
    h.pl_sgb_plan.argtypes = [d, p]
    h.pl_fb_small.restype = u
    h.pl_fb_small.argtypes = []
    h.pl_lines_words.restype = u
    h.pl_lines_words.argtypes = []
    h.pl_fb_cover.restype = i
    h.pl_fb_cover.argtypes = [u, u, u, u, i, i, p, u, p, q, p, p]
    h.pl_max_work_sections.restype = u
    h.pl_max_work_sections.argtypes = []
    h.pl_work.restype = i
    h.pl_work.argtypes = [u, p, q, p, p, p, p]


def build():
    return twin_build.build("plan")


def lib():
    return twin_build.lib("plan", _signatures)
