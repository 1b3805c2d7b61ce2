"""CPU: the per-cell rule of the terrain map's kernels (camradepth_amd/csrc/terrain_cell.h through tests/terrain_cell_host.cpp) on the
host, over every cell of every call of tests/terrain_cases.py, against the values tests/terrain_ref.py wrote: the fused triple of
launch 4 from what the slot counted as and the call's observation, and step, slope2, state and hazard of launch 5 from the fused
window.  The same file as a stand-alone program built with AddressSanitizer and UBSan runs them as a process of its own; no
sanitizer goes into this one."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import terrain_cases, terrain_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = terrain_cases.all_cases()
CXX = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
I32_MIN = np.iinfo(np.int32).min
_WINDOWS = []


def windows():
    """Every map of every call of every case that was not skipped: its numbers, launch 4's inputs and the restatement's outputs in
    window order.  Made once."""
    if not _WINDOWS:
        for name, case in CASES.items():
            p = case["params"]
            _, step_max_q, slope2_max = terrain_ref.thresholds(p)
            state = terrain_ref.new_state(p)
            for call, f in enumerate(case["frames"]):
                r = terrain_ref.update(p, state, B=case["B"], **f)
                for m in range(p["M"]):
                    if not r["moved"][m]:
                        continue
                    known = r["weight"][m] != 0
                    _WINDOWS.append(dict(what=f"{name}, call {call}, map {m}", nx=p["nx"], ny=p["ny"], min_points=p["min_points"], w_max=p["w_max"],
                                         step_max_q=step_max_q, slope2_max=slope2_max,
                                         inputs=[r["before"][0, m], r["before"][1, m], r["before"][2, m], r["n"][m], r["lo"][m], r["hi"][m]],
                                         fused=[np.where(known, r["ground"][m], 0), np.where(known, r["top"][m], 0), r["weight"][m]],
                                         derived=[r[k][m] for k in ("step", "slope2", "state", "hazard")]))
    return _WINDOWS


def compile_host(out, flags):
    return subprocess.run([CXX, "-std=c++17", "-O2", *flags, "-I", os.path.join(REPO, "camradepth_amd", "csrc"),
                           os.path.join(REPO, "tests", "terrain_cell_host.cpp"), "-o", out], capture_output=True, text=True)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    lib = str(tmp_path_factory.mktemp("terrain_cell") / "libterrain_cell_host.so")
    r = compile_host(lib, ["-shared", "-fPIC"])
    assert r.returncode == 0, r.stderr[-2000:]
    so = ctypes.CDLL(lib)
    so.tch_fuse.restype = so.tch_derive.restype = None
    so.tch_fuse.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    so.tch_derive.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int32, ctypes.c_int64] + [ctypes.c_void_p] * 4
    return so


def test_the_windows_cover_every_branch_of_the_rule():
    ws = windows()
    assert len(ws) >= 60
    w, n, fused_w = (np.concatenate([np.ravel(x) for x in xs]) for xs in zip(*[(v["inputs"][0], v["inputs"][3], v["fused"][2]) for v in ws]))
    observed = n >= np.concatenate([np.full(v["nx"] * v["ny"], v["min_points"]) for v in ws])
    assert (observed & (w == 0)).any() and (observed & (w > 0)).any() and (~observed & (w > 0)).any() and (~observed & (w == 0)).any()
    assert ((n > 0) & ~observed).any() and (observed & (fused_w == w) & (w > 0)).any()             # too few rows; the weight at w_max
    states = np.concatenate([np.ravel(v["derived"][2]) for v in ws])
    assert set(np.unique(states).tolist()) == {0, 1, 2}
    assert any((np.asarray(v["inputs"][1]) < 0).any() for v in ws)                                   # negative grounds go through the floor division


def test_fuse_and_derive_on_the_host(host):
    for v in windows():
        cells = v["nx"] * v["ny"]
        ins = [np.ascontiguousarray(a, np.int32) for a in v["inputs"]]
        g, t, w = (np.full(cells, 77, np.int32) for _ in range(3))
        host.tch_fuse(cells, *(a.ctypes.data for a in ins), v["min_points"], v["w_max"], g.ctypes.data, t.ctypes.data, w.ctypes.data)
        for got, want, k in zip((g, t, w), v["fused"], ("ground", "top", "weight")):
            assert (got.reshape(v["nx"], v["ny"]) == want).all(), (v["what"], k)
        step, slope2 = np.full(cells, 77, np.int32), np.full(cells, 77, np.int64)
        state, hazard = np.full(cells, 77, np.uint8), np.full(cells, 77, np.uint8)
        host.tch_derive(v["nx"], v["ny"], g.ctypes.data, t.ctypes.data, w.ctypes.data, v["step_max_q"], v["slope2_max"], step.ctypes.data,
                        slope2.ctypes.data, state.ctypes.data, hazard.ctypes.data)
        for got, want, k in zip((step, slope2, state, hazard), v["derived"], ("step", "slope2", "state", "hazard")):
            assert got.dtype == want.dtype and (got.reshape(v["nx"], v["ny"]) == want).all(), (v["what"], k)


def test_the_rule_at_the_ends_of_its_range(host):
    """Heights of almost 2^24 quanta of either sign, weights up to 32767 and the largest thresholds: nothing leaves int64, and the
    results are Python's."""
    big = 2 ** 24 - 1
    rows = [(32767, -big, -big, 5, big, big, 32767), (32766, big, big, 5, -big, -big, 32767), (0, 123, 456, 0, 1, 2, 15), (3, -7, -7, 9, -8, -8, 15),
            (1, -1, 0, 2, -2, -1, 1), (32767, -big, big, 2, -big, big, 32767)]
    for w, g, t, n, lo, hi, w_max in rows:
        arrays = [np.array([v], np.int32) for v in (w, g, t, n, lo, hi)]
        out = [np.zeros(1, np.int32) for _ in range(3)]
        host.tch_fuse(1, *(a.ctypes.data for a in arrays), 2, w_max, *(a.ctypes.data for a in out))
        if n < 2:
            want = (g if w else 0, t if w else 0, w)
        elif w == 0:
            want = (lo, hi, 1)
        else:
            want = ((w * g + lo) // (w + 1), (w * t + hi) // (w + 1), min(w + 1, w_max))
        assert tuple(int(a[0]) for a in out) == want, (w, g, t, n, lo, hi)
    ground = np.array([[-big, big, -big], [big, -big, big], [-big, big, -big]], np.int32)
    weight, top = np.ones((3, 3), np.int32), ground.copy()
    for step_max_q, slope2_max, state in ((2 ** 30, 2 ** 62, 1), (2 * big, 2 ** 62, 1), (2 * big - 1, 2 ** 62, 2), (2 ** 30, 1, 1)):
        step, slope2, st, hz = np.zeros(9, np.int32), np.zeros(9, np.int64), np.zeros(9, np.uint8), np.zeros(9, np.uint8)
        host.tch_derive(3, 3, ground.ctypes.data, top.ctypes.data, weight.ctypes.data, step_max_q, slope2_max, *(a.ctypes.data for a in (step, slope2, st, hz)))
        assert (step == 2 * big).all() and slope2[4] == 0 and slope2[0] == 2 * (4 * big) ** 2 and st[4] == state
        assert hz[4] == (254 if state == 2 else 2 * big * 253 // step_max_q)
        assert st[0] == (1 if slope2_max == 2 ** 62 and state == 1 else 2)


def test_fuse_and_derive_under_sanitizers_as_a_process(tmp_path):
    """tests/terrain_cell_host.cpp with AddressSanitizer and UBSan, a program of its own, on every window."""
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
    lines = [str(len(windows()))]
    for v in windows():
        lines.append(f"{v['nx']} {v['ny']} {v['min_points']} {v['w_max']} {v['step_max_q']} {v['slope2_max']}")
        table = np.stack([np.ravel(a).astype(np.int64) for a in v["inputs"] + v["fused"] + v["derived"]], axis=1)
        lines += [" ".join(str(x) for x in row) for row in table.tolist()]
    (tmp_path / "windows.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "terrain_cell_main")
    r = compile_host(exe, flags)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, str(tmp_path / "windows.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
