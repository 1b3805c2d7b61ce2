"""CPU: the taps of the bicubic x2 kernels (camradepth_amd/csrc/bicubic_taps.h through tests/bicubic_taps_host.cpp) on the host.  For
n = 1 .. 12 the 2n x n forward matrix built from the forward taps equals torch's bicubic of the identity, the transpose's folded
weights are exactly its columns, and the "can be non-zero" predicate excludes no weight that is not zero.  Every value is a multiple
of 1/256, so all of it is compared with ==.  The same file as a stand-alone program built with AddressSanitizer and UBSan runs the
checks as a process of its own; no sanitizer goes into this one."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
SIZES = range(1, 13)


def compile_host(out, flags):
    return subprocess.run([CXX, "-std=c++17", "-O2", *flags, "-I", os.path.join(REPO, "camradepth_amd", "csrc"),
                           os.path.join(REPO, "tests", "bicubic_taps_host.cpp"), "-o", out], capture_output=True, text=True)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    lib = str(tmp_path_factory.mktemp("bicubic_taps") / "libbicubic_taps_host.so")
    r = compile_host(lib, ["-shared", "-fPIC"])
    assert r.returncode == 0, r.stderr[-2000:]
    so = ctypes.CDLL(lib)
    so.bt_check.restype = ctypes.c_int
    so.bt_check.argtypes = [ctypes.c_int]
    so.bt_matrix.restype = None
    so.bt_matrix.argtypes = [ctypes.c_int, ctypes.c_void_p]
    return so


def matrix(host, n):
    m = np.full((2 * n, n), 7.0, np.float32)
    host.bt_matrix(n, m.ctypes.data)
    return m


def test_forward_matrix_is_torchs_bicubic_of_the_identity(host):
    for n in SIZES:
        m = matrix(host, n)
        ref = F.interpolate(torch.eye(n, dtype=torch.float64).reshape(n, 1, 1, n).expand(n, 1, 2, n), scale_factor=(1, 2), mode="bicubic")
        assert ref.shape == (n, 1, 2, 2 * n)
        assert np.array_equal(m.astype(np.float64), ref[:, 0, 0].t().numpy()), n
        assert np.array_equal(m * 256, np.round(m * 256))                  # multiples of 1/256
        # eight candidates per input, and the borders no wider: outputs 2i - 3 .. 2i + 4
        o, i = np.nonzero(m)
        assert (o >= 2 * i - 3).all() and (o <= 2 * i + 4).all()


def test_folded_transpose_weights_are_the_columns(host):
    for n in SIZES:
        assert host.bt_check(n) == 0, n


def test_taps_under_sanitizers_as_a_process(tmp_path):
    """tests/bicubic_taps_host.cpp with AddressSanitizer and UBSan, a program of its own."""
    assert CXX is not None, "no host C++ compiler"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    base = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    flags = None
    for extra in (["-static-libasan"], ["-static-libsan"], []):         # a runtime linked into the program needs nothing of the loader
        if subprocess.run([CXX, *base, *extra, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0 and \
                subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            flags = base + extra
            break
    if flags is None:
        pytest.skip("the host compiler has no sanitizer runtime that links and starts here")
    exe = str(tmp_path / "bicubic_taps_main")
    r = compile_host(exe, flags)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
