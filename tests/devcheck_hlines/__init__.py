"""Device (gfx950) unit harness for the H(m)-lines kernel's body (px_h_lines).

TEST TOOLING ONLY -- see devcheck_hlines.hip.  Built the way tests/devcheck
is: the engine's compiler and common flags plus the per-unit flags
charon_amd/_native.py gives k_verify.hip (the unit that holds k_lines_h),
checked by the same return-address guard, linked with a version script that
exports the dch_* entries only.  Never loaded by charon_amd.
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "devcheck_hlines.hip")
LIB = os.path.join(HERE, "libdevcheck_hlines.so")
MAP = os.path.join(HERE, "devcheck_hlines.map")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "charon_amd", "csrc")
UNIT = "k_verify.hip"

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-Wno-unused-result",
         "-Wno-unused-value"]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    from charon_amd import _native
    deps = [SRC, MAP, os.path.abspath(__file__), os.path.abspath(_native.__file__)]  # (the last two hold the flags)
    deps += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build():
    """Compile the harness for gfx950 if the library is stale; raises without hipcc."""
    if _stale():
        from charon_amd import _native
        hipcc = _native._hipcc()  # raises: a stale library is an error, never a skip
        obj = os.path.splitext(SRC)[0] + ".o"
        subprocess.check_call([hipcc] + FLAGS + list(_native.UNIT_FLAGS.get(UNIT, ())) + ["-c", SRC, "-o", obj])
        _native.check_return_address(obj)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-Bsymbolic",
                               "-Wl,--version-script=" + MAP, obj, "-o", LIB + ".tmp"])
        os.replace(LIB + ".tmp", LIB)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        L.dch_sticky_error.restype = ctypes.c_int
        L.dch_sticky_error.argtypes = []
        L.dch_lines.restype = ctypes.c_int
        L.dch_lines.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                                ctypes.c_uint32]
        _lib = L
    return _lib
