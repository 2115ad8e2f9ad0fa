"""Host (CPU) build of the share calls' workspace walk (work_host.cpp) for
tests/test_shares_abi.py.

TEST TOOLING ONLY -- see the source.  Built on demand with the ROCm clang
(host target), as tests/feldman builds its own walk: it only reads the HIP
headers' types.
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "work_host.cpp")
LIB = os.path.join(HERE, "libshares_work.so")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "charon_amd", "csrc")


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build():
    if _stale():
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        cxx = os.path.join(rocm, "llvm", "bin", "clang++")
        if not os.path.exists(cxx):
            cxx = "clang++"
        tmp = LIB + ".%d.tmp" % os.getpid()
        subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-pass-failed", "-D__HIP_PLATFORM_AMD__",
                               "-I" + os.path.join(rocm, "include"), SRC, "-o", tmp])
        os.replace(tmp, LIB)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        h = ctypes.CDLL(build())
        p, q = ctypes.c_void_p, ctypes.c_uint64
        h.shw_max_sections.restype = ctypes.c_uint32
        h.shw_max_sections.argtypes = []
        h.shw_split.restype = ctypes.c_int
        h.shw_split.argtypes = [q, q, q, q, q, p, p, p, p, p, p, p]
        h.shw_combine.restype = ctypes.c_int
        h.shw_combine.argtypes = [q, q, q, p, p, p, p, p, p, p]
        h.shw_keyed_secret.restype = ctypes.c_int
        h.shw_keyed_secret.argtypes = [ctypes.c_int, q, q, p, p]
        _lib = h
    return _lib
