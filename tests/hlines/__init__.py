"""Host (CPU) build of the H(m)-lines kernel's projective Miller steps, for
tests/test_hlines_host.py (and the expected words of tests/test_gpu_hlines.py).

TEST TOOLING ONLY -- see hlines_host.cpp.  Built on demand with the ROCm
clang (host target) and TBG_BOUNDS_CHECK, which aborts on any violated value
or limb bound of the lazy sums (as tests/hostcheck does for the rest of the
device math).
"""
import ctypes

from tests import twin_build

N_LINES = 68
LINE_WORDS = 3 * 2 * 14
LINES_WORDS = N_LINES * LINE_WORDS


def aff192(q):
    """An affine G2 point of the oracle ((x0, x1), (y0, y1)) as the twin reads it."""
    return b"".join(v.to_bytes(48, "big") for v in (q[0][0], q[0][1], q[1][0], q[1][1]))


def b2f(b):
    return (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:96], "big"))


def h_of(msg):
    """H(m) by the engine's own hash-to-G2 (host build), as an oracle point."""
    out = ctypes.create_string_buffer(192)
    assert lib().hl_hash(msg, len(msg), out) == 0
    return (b2f(out.raw[:96]), b2f(out.raw[96:]))


def _signatures(h):
    c, i, u, p = ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p
    for name, args in {"hl_hash": [c, u, c], "hl_steps": [c, i, c, c, c], "hl_words": [c, p],
                       "hl_pairing": [c, c, i, c], "hl_verify": [c, c, u, c]}.items():
        fn = getattr(h, name)
        fn.restype = ctypes.c_int
        fn.argtypes = args
    h.hl_words.restype = None


def build():
    return twin_build.build("hlines")


def lib():
    return twin_build.lib("hlines", _signatures)
