"""CPU: the pick's comparison and the pose composition of the scan matcher's kernels (camradepth_amd/csrc/match_pick.h through
tests/match_pick_host.cpp) on the host, against the values tests/match_ref.py wrote for every match of tests/match_cases.py: the pick
over the candidates in natural and in shuffled order, T'[b][t] of every frame and turn and the pose that goes out, bit for bit.  The
same file as a stand-alone program built with AddressSanitizer and UBSan runs them as a process of its own; no sanitizer goes into
this one."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import match_cases, match_ref
from tests.occupancy_ref import per_frame, transformed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = match_cases.all_cases()
CXX = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
SEEDS = (0, 1, 0x9E3779B97F4A7C15)
_PROBLEMS = []


def problems():
    """-> (tables, poses): every map's score table with the restatement's pick, and every frame's (T, S, c, s, centre, dx, dy, cell)
    with T'[b][t] and T'[b][t] moved, for every turn (moved by the pick) and for the turn of the pick.  Made once."""
    if not _PROBLEMS:
        tables, poses = [], []
        for name, c in CASES.items():
            state = match_cases.state_of(name, c)
            for i, match in enumerate(c["matches"]):
                out, spec, kw, B, M = match_cases.match_of(c, state, i), match["spec"], match["kw"], c["B"], c["params"]["M"]
                n_xy, n_theta, cell = spec["n_xy"], spec["n_theta"], float(c["params"]["cell"])
                rot = match_ref.rot_table(n_theta, spec["d_theta"])
                T = match_ref.poses_of(kw.get("T"), B)
                S = np.stack(transformed(T, np.arange(B), per_frame(kw.get("sensor"), B)), axis=1)
                for m in range(M):
                    t, dx, dy = (int(v) for v in out["pick"][m])
                    tables.append(dict(what=f"{name}, match {i}, map {m}", n_xy=n_xy, n_theta=n_theta, table=out["scores"][m].reshape(-1),
                                       pick=(t + n_theta, dx, dy), score=int(out["score"][m])))
                    for b in (range(B) if M == 1 else [m]):
                        if not np.isfinite(T[b]).all() or not np.isfinite(S[0 if M == 1 else b]).all():
                            continue                                             # the payload of a NaN is not pinned
                        for tt in range(2 * n_theta + 1):
                            moved = out["T_c"][b, tt].copy()
                            moved[0, 3] = moved[0, 3] + np.float64(dx) * np.float64(cell)
                            moved[1, 3] = moved[1, 3] + np.float64(dy) * np.float64(cell)
                            poses.append(dict(what=f"{name}, match {i}, frame {b}, turn {tt}", T=T[b].reshape(-1), S=S[0 if M == 1 else b, :2],
                                              c=rot[tt, 0], s=rot[tt, 1], centre=int(tt == n_theta), dx=dx, dy=dy, cell=cell,
                                              candidate=out["T_c"][b, tt].reshape(-1), want=moved.reshape(-1),
                                              applied=out["pose"][b].reshape(-1) if tt == t + n_theta and not out["status"][m] & 15 else None))
        _PROBLEMS.append((tables, poses))
    return _PROBLEMS[0]


def compile_host(out, flags):
    return subprocess.run([CXX, "-std=c++17", "-O2", *flags, "-I", os.path.join(REPO, "camradepth_amd", "csrc"),
                           os.path.join(REPO, "tests", "match_pick_host.cpp"), "-o", out], capture_output=True, text=True)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    lib = str(tmp_path_factory.mktemp("match_pick") / "libmatch_pick_host.so")
    r = compile_host(lib, ["-shared", "-fPIC"])
    assert r.returncode == 0, r.stderr[-2000:]
    so = ctypes.CDLL(lib)
    so.mp_pick.restype = ctypes.c_longlong
    so.mp_pick.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]
    so.mp_pose.restype = None
    so.mp_pose.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                           ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    return so


def test_the_problems_cover_ties_guards_and_every_search_shape():
    tables, poses = problems()
    assert len(tables) >= 30 and len(poses) >= 100
    assert {(p["n_xy"] > 0, p["n_theta"] > 0) for p in tables} == {(True, True), (True, False), (False, True)}
    assert any((p["table"] == p["score"]).sum() > 1 for p in tables) and any((p["table"] == p["score"]).sum() == 1 for p in tables)
    assert any(not p["table"].any() for p in tables) and any(p["applied"] is not None and (p["dx"] or p["dy"]) for p in poses)


def test_the_pick_in_natural_and_in_shuffled_order(host):
    for p in problems()[0]:
        table = np.ascontiguousarray(p["table"], np.int64)
        for seed in SEEDS:
            pick = np.full(3, 99, np.int32)
            score = host.mp_pick(table.ctypes.data, p["n_xy"], p["n_theta"], seed, pick.ctypes.data)
            assert (tuple(pick.tolist()), score) == (p["pick"], p["score"]), (p["what"], seed)


def test_the_pose_composition_bit_for_bit(host):
    for p in problems()[1]:
        T, S = np.ascontiguousarray(p["T"]), np.ascontiguousarray(p["S"])
        candidate, out = np.full(12, 7.0), np.full(12, 7.0)
        host.mp_pose(T.ctypes.data, S.ctypes.data, p["c"], p["s"], p["centre"], p["dx"], p["dy"], p["cell"], candidate.ctypes.data, out.ctypes.data)
        assert candidate.tobytes() == p["candidate"].tobytes(), p["what"]
        assert out.tobytes() == p["want"].tobytes(), p["what"]
        if p["applied"] is not None:
            assert out.tobytes() == p["applied"].tobytes(), p["what"]
        if p["centre"]:
            assert candidate.tobytes() == T.tobytes(), p["what"]


def test_pick_and_pose_under_sanitizers_as_a_process(tmp_path):
    """tests/match_pick_host.cpp with AddressSanitizer and UBSan, a program of its own, on a share of the problems."""
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
    tables, poses = problems()
    tables, poses = tables[::2], poses[::5]
    lines = [str(len(tables))]
    for p in tables:
        lines += [f"{p['n_xy']} {p['n_theta']}", " ".join(str(int(v)) for v in p["table"]), " ".join(str(v) for v in p["pick"])]
    lines.append(str(len(poses)))
    for p in poses:
        lines += [" ".join(float(v).hex() for v in p["T"]),
                  f"{float(p['S'][0]).hex()} {float(p['S'][1]).hex()} {float(p['c']).hex()} {float(p['s']).hex()} {p['centre']} {p['dx']} {p['dy']} "
                  f"{float(p['cell']).hex()}", " ".join(float(v).hex() for v in p["want"])]
    (tmp_path / "problems.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "match_pick_main")
    r = compile_host(exe, flags)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
