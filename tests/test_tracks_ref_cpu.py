"""CPU: tests/tracks_ref.py, the Python restatement of crd_track_objects, held on every case of tests/tracks_cases.py and on seeded
random tie-heavy problems to an independent sorted-edge greedy loop, on the unambiguous problems to
scipy.optimize.linear_sum_assignment as well, and to the invariants of the ids and counts; and the host build of the kernel's
association body (camradepth_amd/csrc/track_assoc.h through tests/tracks_assoc_host.cpp) in natural and in shuffled thread order: the
same assignment and the same rounds.  A stand-alone program built with AddressSanitizer and UBSan runs the body as a process of its
own; no sanitizer goes into this one."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from tests import tracks_cases, tracks_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tracks_cases.all_cases()
CXX = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
_RUNS, _PROBLEMS = {}, []


def run_of(name):
    """The restatement's states and outputs of case `name`, frame by frame, computed once and left unchanged."""
    if name not in _RUNS:
        _RUNS[name] = tracks_ref.run_case(CASES[name])
    return _RUNS[name]


def problems():
    """Every association problem of every frame and map of the cases, then seeded random ones on a 0.5 lattice: dictionaries of pred,
    live, z, candidate, n, gate2, cap and the restatement's answer."""
    if _PROBLEMS:
        return _PROBLEMS
    for name, c in CASES.items():
        run = run_of(name)
        T, N, gate = c["spec"]["max_tracks"], c["N"], float(c["spec"]["gate"])
        for i, f in enumerate(c["frames"]):
            before = tracks_ref.new_state(c["M"], T) if i == 0 or f["reset"] else run[i - 1][0]
            for m in range(c["M"]):
                pred, live, z, candidate, n = tracks_ref.problem(before, m, f["centre"], f["info"])
                _PROBLEMS.append(dict(what=f"{name}, frame {i}, map {m}", pred=pred, live=live, z=z, candidate=candidate, n=n, gate2=gate * gate,
                                      cap=min(N, T) + 1))
    rng = np.random.default_rng(2024)
    for trial in range(60):
        T, N = (int(v) for v in rng.integers(1, 25, 2))
        side = int(rng.integers(2, 9))                                   # a small lattice: many equal distances
        pred = [(float(x), float(y)) for x, y in rng.integers(0, side, (T, 2)) * 0.5]
        z = [(float(x), float(y)) for x, y in rng.integers(0, side, (N, 2)) * 0.5]
        live = [bool(v) for v in rng.random(T) < 0.8]
        n = int(rng.integers(0, N + 1))
        candidate = [k < n and bool(rng.random() < 0.9) for k in range(N)]
        gate = float(rng.choice([0.5, 1.0, 1.5, 4.0]))
        _PROBLEMS.append(dict(what=f"random {trial}", pred=pred, live=live, z=z, candidate=candidate, n=n, gate2=gate * gate, cap=min(N, T) + 1))
    for p in _PROBLEMS:
        p["trk_obj"], p["obj_trk"], p["rounds"], p["guard"] = tracks_ref.associate(p["pred"], p["live"], p["z"], p["candidate"], p["gate2"], p["cap"])
    return _PROBLEMS


def edges_of(p):
    """(d2, t, k) of every pair within the gate, d2 written out anew."""
    edges = []
    for t, (px, py) in enumerate(p["pred"]):
        for k, (zx, zy) in enumerate(p["z"]):
            if p["live"][t] and p["candidate"][k]:
                dx, dy = zx - px, zy - py
                d2 = dx * dx + dy * dy
                if d2 <= p["gate2"]:
                    edges.append((d2, t, k))
    return edges


def test_the_rounds_are_the_sorted_greedy_assignment():
    ties = 0
    for p in problems():
        edges = edges_of(p)
        slot_of, row_of = {}, {}
        for d2, t, k in sorted(edges):
            if t not in row_of and k not in slot_of:
                row_of[t], slot_of[k] = k, t
        want_t = [row_of.get(t, -1) if p["live"][t] else -2 for t in range(len(p["live"]))]
        want_k = [slot_of.get(k, -1) if p["candidate"][k] else -2 for k in range(len(p["candidate"]))]
        assert (p["trk_obj"], p["obj_trk"]) == (want_t, want_k), p["what"]
        assert p["guard"] == 0 and 1 <= p["rounds"] <= min(len(row_of), p["cap"] - 1) + 1, p["what"]
        ties += len(edges) - len({d2 for d2, _, _ in edges})
    assert ties > 500                                                    # the problems are tie-heavy


def test_unambiguous_problems_agree_with_the_optimal_assignment():
    checked = pairs = 0
    for p in problems():
        edges = edges_of(p)
        if not edges or len({t for _, t, _ in edges}) != len(edges) or len({k for _, _, k in edges}) != len(edges):
            continue                                                    # a slot or a row with two candidates
        T, N = len(p["live"]), len(p["candidate"])
        big = 1e9
        cost = np.full((T, N), big)
        for d2, t, k in edges:
            cost[t, k] = d2
        rows, cols = linear_sum_assignment(cost)
        optimal = {(int(t), int(k)) for t, k in zip(rows, cols) if cost[t, k] < big}
        assert optimal == {(t, k) for t, k in enumerate(p["trk_obj"]) if k >= 0} == {(t, k) for _, t, k in edges}, p["what"]
        checked, pairs = checked + 1, pairs + len(edges)
    assert checked >= 20 and pairs >= 60


@pytest.mark.parametrize("name", list(CASES))
def test_invariants_frame_by_frame(name):
    c = CASES[name]
    T, N, M = c["spec"]["max_tracks"], c["N"], c["M"]
    born_total, live_before, ids_before, next_before = np.zeros(M, np.int64), np.zeros(M, np.int64), np.full((M, T), -1), np.zeros(M, np.int64)
    for i, (state, out) in enumerate(run_of(name)):
        if c["frames"][i]["reset"]:
            born_total[:], live_before[:], ids_before[:], next_before[:] = 0, 0, -1, 0
        info = out["info"]
        assert state["ids"].dtype == np.int64 and state["tracks"].dtype == np.int32 and state["pos"].dtype == np.float64
        assert out["track_of"].dtype == np.int32 and out["id_of"].dtype == np.int64 and info.dtype == np.int32 and info.shape == (M, 8)
        for m in range(M):
            n_live, n_matched, n_born, n_missed_out, n_left, n_overflow, rounds, guard = (int(v) for v in info[m])
            live = state["tracks"][m, :, 0] != 0
            ids = state["ids"][m]
            assert guard == 0 and 1 <= rounds <= min(N, T) + 1
            assert n_live == live.sum() == live_before[m] + n_born - n_missed_out - n_left
            born_total[m] += n_born
            assert state["next_id"][m] == born_total[m] == next_before[m] + n_born
            assert len(set(ids[live].tolist())) == n_live and (ids[~live] == -1).all() and (ids[live] >= 0).all() and (ids[live] < state["next_id"][m]).all()
            fresh = ids >= next_before[m]                               # born in this call: ids never used before, rank by rank
            assert fresh.sum() == n_born and sorted(ids[fresh].tolist()) == list(range(int(next_before[m]), int(state["next_id"][m])))
            assert (ids[live & ~fresh] == ids_before[m][live & ~fresh]).all()      # a track keeps its slot and its id
            free = ~live
            assert (state["tracks"][m, free] == np.array(tracks_ref.FREE_ROW)).all() and np.isnan(state["pos"][m, free]).all()
            assert np.isnan(state["vel"][m, free]).all() and not state["box"][m, free].any() and np.isfinite(state["pos"][m, live]).all()
            track_of, obj = out["track_of"][m], state["tracks"][m, :, 4]
            for k in np.flatnonzero(track_of >= 0):
                assert live[track_of[k]] and obj[track_of[k]] == k and out["id_of"][m, k] == ids[track_of[k]]
            for t in np.flatnonzero(live & (obj >= 0)):
                assert track_of[obj[t]] == t
            assert (out["id_of"][m][track_of < 0] == -1).all() and (track_of >= 0).sum() == (live & (obj >= 0)).sum()
            live_before[m], ids_before[m], next_before[m] = n_live, ids.copy(), state["next_id"][m]


def test_the_cases_place_what_they_are_meant_to():
    def info(name, i, m=0):
        return run_of(name)[i][1]["info"][m].tolist()

    assert info("empty table, first frame", 0) == [0, 0, 0, 0, 0, 0, 1, 0] and info("empty table, first frame", 1)[:3] == [1, 0, 1]
    static = run_of("one static object, six frames")
    assert [s["tracks"][0, 0, 0] for s, _ in static] == [1, 1, 2, 2, 2, 2] and [s["tracks"][0, 0, 2] for s, _ in static] == [1, 2, 3, 4, 5, 6]
    assert all(s["ids"][0, 0] == 0 and s["tracks"][0, 0, 5] == 5 for s, _ in static) and (static[5][0]["vel"][0, 0] == 0).all()
    moving = run_of("moving a cell per frame")
    speed = [s["vel"][0, 0, 0] for s, _ in moving]
    assert all(s["ids"][0, 0] == 0 for s, _ in moving) and abs(speed[-1] - 0.5) < 0.02 < abs(speed[3] - 0.5) and moving[-1][0]["vel"][0, 0, 1] == 0
    ties = run_of("exact ties of d2")
    assert ties[1][1]["track_of"][0, 0] == 0 and ties[1][1]["info"][0, :4].tolist() == [2, 1, 0, 0]              # the lower slot
    assert ties[2][1]["track_of"][0, :2].tolist() == [0, 1] and ties[2][1]["info"][0, 6] == 3                    # the lower row, then the rest
    assert ties[3][1]["track_of"][0, :3].tolist() == [1, 2, 0] and ties[3][1]["info"][0, 2] == 1
    gate = run_of("on the gate and the next double above")
    assert 4.0 + 2.0 ** -50 == np.nextafter(4.0, 5.0)
    assert gate[1][1]["track_of"][0, :2].tolist() == [0, 2] and gate[1][1]["id_of"][0, :2].tolist() == [0, 2] and gate[1][1]["info"][0, 1:3].tolist() == [1, 1]
    for P, NT in ((20, 32), (16, 16)):
        run = run_of(f"a displacement chain of {P} in {NT} slots")
        assert run[1][1]["info"][0].tolist() == [P, P, 0, 0, 0, 0, P + 1, 0]                                      # P = min(N, T): the cap, met exactly
        assert run[1][1]["track_of"][0, :P].tolist() == list(range(P)) and run[0][1]["info"][0, 6] == 1 and run[2][1]["info"][0, 6] == 2
    keep, drop = run_of("max_misses 2, gone for two frames"), run_of("max_misses 0, gone for two frames")
    assert [o["id_of"][0, 0] for _, o in keep] == [0, 0, 1, 1, 0, 0] and keep[3][0]["tracks"][0, 0, 3] == 2 and keep[4][0]["tracks"][0, 0, 3] == 0
    assert [o["id_of"][0, 0] for _, o in drop] == [0, 0, 1, 1, 2, 2] and drop[2][1]["info"][0, 3] == 1
    over = run_of("births beyond the free slots")
    assert over[0][1]["info"][0].tolist() == [4, 0, 4, 0, 0, 2, 1, 0] and over[1][1]["info"][0].tolist() == [4, 3, 1, 1, 0, 2, 2, 0]
    assert over[1][1]["track_of"][0, :6].tolist() == [0, 1, 2, 3, -1, -1] and over[1][0]["ids"][0].tolist() == [0, 1, 2, 4]
    ren = run_of("rows renumbered between frames")
    assert [o["id_of"][0, :3].tolist() for _, o in ren[:3]] == [[0, 1, 2], [2, 0, 1], [1, 2, 0]] and ren[3][1]["id_of"][0, :4].tolist() == [3, 0, 1, 2]
    shift = run_of("the origin shifts by (+1, -2) a frame")
    assert all(np.array_equal(s["box"], shift[0][0]["box"]) and np.array_equal(s["pos"], shift[0][0]["pos"], equal_nan=True) and
               np.array_equal(s["ids"], shift[0][0]["ids"]) for s, _ in shift)
    assert shift[0][0]["box"][0, 0].tolist() == [6, 6, 6, 6] and not np.array_equal(CASES["the origin shifts by (+1, -2) a frame"]["frames"][0]["objects"],
                                                                                    CASES["the origin shifts by (+1, -2) a frame"]["frames"][1]["objects"])
    coast = run_of("a coasting track leaves the window")
    assert [o["info"][0, 4] for _, o in coast] == [0, 0, 0, 0, 1, 0] and coast[3][0]["pos"][0, 0, 0] == 15.5 and coast[4][0]["ids"][0, 0] == -1
    nan = run_of("NaN centre rows inside n_objects")
    assert [o["id_of"][0, :3].tolist() for _, o in nan] == [[0, -1, 1], [-1, 0, 1], [0, 1, -1]] and all(o["info"][0, 2] == 0 for _, o in nan[1:])
    stale = run_of("stale rows behind n_objects")
    assert [o["info"][0, :3].tolist() for _, o in stale] == [[2, 0, 2], [2, 1, 0], [2, 0, 0], [2, 2, 0]]
    three = run_of("three maps with different histories")
    assert len({tuple(o["info"][m].tolist()) for _, o in three for m in range(3)}) > 6 and three[-1][0]["next_id"].tolist()[1] == 1
    assert len({int(s["next_id"][m]) for s, _ in three[-1:] for m in range(3)}) == 3
    reset = run_of("reset mid-sequence")
    assert [o["id_of"][0, :3].tolist() for _, o in reset] == [[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, -1]] and reset[2][1]["info"][0, 2] == 3
    crowd = run_of("a crowd on a lattice, two maps")
    assert sum(int(o["info"][:, 5].sum()) for _, o in crowd) > 0 and sum(int(o["info"][:, 3].sum()) for _, o in crowd) > 0
    assert max(int(o["info"][:, 6].max()) for _, o in crowd) >= 3


def compile_host(out, sources, flags):
    return subprocess.run([CXX, "-std=c++17", "-O2", *flags, "-I", os.path.join(REPO, "camradepth_amd", "csrc"),
                           *[os.path.join(REPO, "tests", s) for s in sources], "-o", out], capture_output=True, text=True)


@pytest.fixture(scope="module")
def host_assoc(tmp_path_factory):
    """tests/tracks_assoc_host.cpp as a plain shared library: the association body of the kernel, compiled for the host."""
    assert CXX is not None, "no host C++ compiler"
    lib = str(tmp_path_factory.mktemp("tracks_assoc") / "libtracks_assoc_host.so")
    r = compile_host(lib, ["tracks_assoc_host.cpp"], ["-shared", "-fPIC"])
    assert r.returncode == 0, r.stderr[-2000:]
    fn = ctypes.CDLL(lib).ta_associate
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6 + [ctypes.c_double, ctypes.c_int, ctypes.c_uint64] + [ctypes.c_void_p] * 3
    return fn


def arrays_of(p):
    px, py = (np.array([v[c] for v in p["pred"]], np.float64) for c in (0, 1))
    zx, zy = (np.array([v[c] for v in p["z"]], np.float64) for c in (0, 1))
    return px, py, np.array(p["live"], np.uint8), zx, zy, np.array(p["candidate"], np.uint8)


def test_the_association_body_in_natural_and_in_shuffled_order(host_assoc):
    for p in problems():
        px, py, live, zx, zy, candidate = arrays_of(p)
        for seed in (0, 1, 0x9E3779B97F4A7C15):
            trk_obj, obj_trk, rounds = np.full(len(live), 7, np.int32), np.full(len(candidate), 7, np.int32), np.zeros(1, np.int32)
            guard = host_assoc(len(live), len(candidate), p["n"], px.ctypes.data, py.ctypes.data, live.ctypes.data, zx.ctypes.data, zy.ctypes.data,
                               candidate.ctypes.data, p["gate2"], p["cap"], seed, trk_obj.ctypes.data, obj_trk.ctypes.data, rounds.ctypes.data)
            assert (trk_obj.tolist(), obj_trk.tolist(), int(rounds[0]), guard) == (p["trk_obj"], p["obj_trk"], p["rounds"], p["guard"]), (p["what"], seed)


def test_the_association_body_under_sanitizers_as_a_process(tmp_path):
    """tests/tracks_assoc_main.cpp with AddressSanitizer and UBSan, a program of its own, on the problems of two cases."""
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
    chosen = [p for p in problems() if p["what"].startswith(("a displacement chain of 20", "a crowd on a lattice"))]
    assert len(chosen) >= 10
    lines = [str(len(chosen))]
    for p in chosen:
        lines.append(f"{len(p['live'])} {len(p['candidate'])} {p['n']} {p['cap']} {float(p['gate2']).hex()}")
        lines += [f"{int(l)} {x.hex()} {y.hex()}" for l, (x, y) in zip(p["live"], p["pred"])]
        lines += [f"{int(c)} {x.hex()} {y.hex()}" if x == x and y == y else f"{int(c)} nan nan" for c, (x, y) in zip(p["candidate"], p["z"])]
        lines += [" ".join(str(v) for v in p["trk_obj"]) or "", " ".join(str(v) for v in p["obj_trk"]) or "", f"{p['rounds']} {p['guard']}"]
    (tmp_path / "problems.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "tracks_assoc_main")
    r = compile_host(exe, ["tracks_assoc_host.cpp", "tracks_assoc_main.cpp"], flags)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
