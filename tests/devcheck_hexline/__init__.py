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
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(os.path.dirname(HERE), "devcheck", "devcheck_hexline.hip")
LIB = os.path.join(HERE, "libdevcheck_hexline.so")
MAP = os.path.join(HERE, "devcheck_hexline.map")
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "charon_amd", "csrc")
UNIT = "k_miller_hex.hip"

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
        obj = os.path.join(HERE, "devcheck_hexline.o")
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
        u32p = ctypes.POINTER(ctypes.c_uint32)
        L.dcx_sticky_error.restype = ctypes.c_int
        L.dcx_sticky_error.argtypes = []
        L.dcx_hex_line.restype = ctypes.c_int
        L.dcx_hex_line.argtypes = [ctypes.c_int, u32p, u32p, u32p, u32p, ctypes.c_uint32, ctypes.c_uint32]
        _lib = L
    return _lib
