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
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "feldman_host.cpp")
LIB = os.path.join(HERE, "libfeldman_host.so")
WORK_SRC = os.path.join(HERE, "work_host.cpp")
WORK_LIB = os.path.join(HERE, "libfeldman_work.so")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "charon_amd", "csrc")


def _stale(src, lib_path):
    if not os.path.exists(lib_path):
        return True
    t = os.path.getmtime(lib_path)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src, lib_path, flags):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cxx = os.path.join(rocm, "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = "clang++"
    tmp = lib_path + ".%d.tmp" % os.getpid()
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-pass-failed"] + flags + [src, "-o", tmp])
    os.replace(tmp, lib_path)


def build():
    if _stale(SRC, LIB):
        _compile(SRC, LIB, ["-DTBG_BOUNDS_CHECK"])
    if _stale(WORK_SRC, WORK_LIB):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        _compile(WORK_SRC, WORK_LIB, ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include")])
    return LIB


_lib = None
_work = None


def lib():
    global _lib
    if _lib is None:
        h = ctypes.CDLL(build())
        p, u = ctypes.c_void_p, ctypes.c_uint32
        h.fvh_eval.restype = ctypes.c_int
        h.fvh_eval.argtypes = [p, p, u, p, p, u, p, p, p]
        h.fvh_mul.restype = ctypes.c_int
        h.fvh_mul.argtypes = [ctypes.c_char_p, u, p]
        _lib = h
    return _lib


def work_lib():
    global _work
    if _work is None:
        build()
        h = ctypes.CDLL(WORK_LIB)
        p, q = ctypes.c_void_p, ctypes.c_uint64
        h.fvw_max_sections.restype = ctypes.c_uint32
        h.fvw_max_sections.argtypes = []
        h.fvw_work.restype = ctypes.c_int
        h.fvw_work.argtypes = [q, q, q, q, p, p, p, p]
        _work = h
    return _work
