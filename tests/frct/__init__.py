"""Host (CPU) builds of the fixed-schedule Fr arithmetic (charon_amd/csrc/bls_frct.h)
for tests/test_frct_host.py: the shared library (frct_host.cpp) and the
stand-alone sanitizer program (frct_main.cpp, its own main()).

TEST TOOLING ONLY -- see the two sources.  Built on demand with the ROCm
clang (host target); the library with TBG_BOUNDS_CHECK as tests/ctmul builds
its own, the program with -fsanitize=address,undefined.  The program is run
as a subprocess: nothing sanitized is loaded into Python.
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "frct_host.cpp")
LIB = os.path.join(HERE, "libfrct_host.so")
MAIN_SRC = os.path.join(HERE, "frct_main.cpp")
MAIN = os.path.join(HERE, "frct_main_san")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "charon_amd", "csrc")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def _stale(srcs, out):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    deps = list(srcs) + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return any(os.path.getmtime(d) > t for d in deps)


def _cxx():
    cxx = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    return cxx if os.path.exists(cxx) else "clang++"


def _compile(src, out, flags):
    tmp = out + ".%d.tmp" % os.getpid()
    subprocess.check_call([_cxx(), "-O1", "-std=c++17", "-DTBG_BOUNDS_CHECK", "-Wno-pass-failed"] + flags + [src, "-o", tmp])
    os.replace(tmp, out)


def build():
    if _stale([SRC], LIB):
        _compile(SRC, LIB, ["-fPIC", "-shared"])
    return LIB


def build_sanitized():
    """The stand-alone program under AddressSanitizer and UBSan (host code only)."""
    if _stale([SRC, MAIN_SRC], MAIN):
        _compile(MAIN_SRC, MAIN, SAN_FLAGS)
    return MAIN


_lib = None


def lib():
    global _lib
    if _lib is None:
        h = ctypes.CDLL(build())
        p, u, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        h.frh_ops.restype = i
        h.frh_ops.argtypes = [i, p, p, u, p]
        h.frh_horner.restype = i
        h.frh_horner.argtypes = [p, u, u, p, p, p]
        h.frh_combine.restype = i
        h.frh_combine.argtypes = [p, p, u, p, p]
        h.frh_count_kinds.restype = u
        h.frh_count_kinds.argtypes = []
        h.frh_count_op.restype = i
        h.frh_count_op.argtypes = [i, p, p, p, p]
        h.frh_count_horner.restype = i
        h.frh_count_horner.argtypes = [p, u, u, p, p, p, p]
        h.frh_count_combine.restype = i
        h.frh_count_combine.argtypes = [p, p, u, p, p, p]
        _lib = h
    return _lib
