"""How the tests compile the programs of tests/cpp/: one function for a program that runs kernel code on the host alone,
one for a caller linked against the library.  Each asserts that the compile succeeded and returns the program's path.  A
program whose compiler or flags differ from the usual ones passes the difference in; nothing here decides flags by name."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ocean-perception_amd")
LIBDIR = os.path.join(PKG, "lib")
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(PKG, "csrc")
HOST = os.path.join(PKG, "host")
CPP = os.path.join(ROOT, "tests", "cpp")

# AddressSanitizer + UBSan; a UBSan report ends the program
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def _compile(cmd, out):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def hipcc_host():
    """hipcc on HIP source with its host-only switch: what the *_body.hpp headers are compiled with for the CPU."""
    return (os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only")


def build_host_kernel(out, source, compiler=None, flags=("-O1", "-std=c++17", "-ffp-contract=off") + SANITIZE,
                      include=(INCLUDE, CSRC)):
    """tests/cpp/<source> -> out: a stand-alone program over csrc/ headers, no library.  By default through hipcc_host() with
    the sanitizers; `compiler`, `flags` and `include` replace the defaults whole."""
    cmd = [*(compiler or hipcc_host()), *flags, *("-I" + d for d in include), os.path.join(CPP, source), "-o", str(out)]
    return _compile(cmd, out)


def build_caller(out, source, flags=("-Wall", "-Wextra"), include_first=(), link=()):
    """tests/cpp/<source> -> out: a host caller of the C ABI and the C++ mirror, built by plain g++ (no HIP header in reach)
    and bound to the library in the tree.  `flags` replace the warning flags, `include_first` goes in front of the two
    include directories, `link` behind the library."""
    cmd = ["g++", "-std=c++17", "-O1", *flags, *("-I" + d for d in (*include_first, INCLUDE, HOST)), os.path.join(CPP, source),
           "-L" + LIBDIR, "-lvehicle_pm_gpu", "-Wl,-rpath," + LIBDIR, *link, "-o", str(out)]
    return _compile(cmd, out)
