"""TEST HELPER: the one place that runs g++ / gcc for test code — the host builds of the kernel headers and the shims over the
C++ mirrors (tests/host_sim), and the stand-alone programs. The compiler writes each output's dependency file (<out>.d, -MMD:
every file the source includes, system headers left out), and that list, not one kept by hand, decides whether an output is
stale. The command runs in the repository root on a root-relative source, so the paths in a .d file are root-relative and stay
valid when the tree is copied elsewhere with what was built."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
SIM = ["-O2", "-fwrapv", "-fPIC", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"]  # a kernel header built for the host
SIM_FP = SIM + ["-ffp-contract=off"]  # the floating-point ones: the bit-for-bit comparisons with the device depend on it
SHIM = ["-O2", "-std=c++17", "-Wall", "-fPIC"]  # a C++ mirror of host/ behind a C interface


def _stale(out):
    """No output, no readable .d file, or a file the .d file names that is missing or newer than the output"""
    try:
        t = os.path.getmtime(out)
        deps = open(out + ".d").read().replace("\\\n", " ").partition(":")[2].split()
        return not deps or any(os.path.getmtime(os.path.join(ROOT, p)) > t for p in deps)
    except OSError:
        return True


def compile(src, out, flags, libs=(), cc="g++"):
    """src -> out (both relative to tests/host_sim unless absolute) where out is stale -> whether it compiled. A compile that
    fails raises CalledProcessError and leaves no output behind that the next call would take for fresh."""
    src, out = os.path.join(SIM_DIR, src), os.path.join(SIM_DIR, out)
    if not _stale(out):
        return False
    for f in (out, out + ".d"):
        if os.path.exists(f):
            os.remove(f)
    subprocess.check_call([cc, *flags, "-MMD", "-MF", out + ".d", "-o", out, os.path.relpath(src, ROOT), *libs], cwd=ROOT)
    return True


def shared(src, out, flags, libs=()):
    compile(src, out, [*flags, "-shared"], libs)
    return ctypes.CDLL(os.path.join(SIM_DIR, out))


def library(pkg):
    """The arguments that link an output with the product's library and let it find that library when it is loaded"""
    libdir = os.path.dirname(os.path.abspath(pkg.lib_path()))
    return ["-L" + libdir, "-lalacgpu", "-Wl,-rpath," + libdir]
