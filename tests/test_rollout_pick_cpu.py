"""CPU: the score and the pick's comparison of the local planner's kernels (camradepth_amd/csrc/rollout_pick.h through
tests/rollout_pick_host.cpp) on the host, against the records tests/rollout_ref.py wrote for every map of tests/rollout_cases.py and
against drawn records full of ties: the scores bit for bit, and the same pick over the records in natural and in shuffled order.  The
same file as a stand-alone program built with AddressSanitizer and UBSan runs them as a process of its own; no sanitizer goes into this
one."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rollout_cases, rollout_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
SEEDS = (0, 1, 0x9E3779B97F4A7C15)
ORDER = ("togo", "max_cost", "sum_cost", "slow", "turn")
_PROBLEMS = []


def expected(p):
    """The scores by the header's formula in Python integers, and the pick by the restatement's sort."""
    K, n_v, n_w, w = p["K"], p["n_v"], p["n_w"], p["weights"]
    end, worst, total, flags = (p["values"][:, i].astype(np.int64) for i in range(4))
    k = np.arange(K)
    scores = (w[0] * end if p["has_togo"] else 0) + w[1] * worst + w[2] * total + w[3] * (n_v - 1 - k // n_w) + w[4] * np.abs(k % n_w - (n_w - 1) // 2)
    valid = (flags & rollout_ref.VALID) != 0
    return scores.astype(np.int64), rollout_ref.pick_of(valid, scores, n_w) if valid.any() else -1


def problems():
    """Every map of the shared cases as records, and drawn records: few distinct values, so that every level of the order decides."""
    if not _PROBLEMS:
        out = []
        for name, case in rollout_cases.all_cases().items():
            want, s = rollout_cases.want_of(name), case["spec"]
            for m in range(case["scene"]["M"]):
                values = np.stack([want[k][m] for k in ("end_togo", "max_cost", "sum_cost", "flags")], axis=1).astype(np.int32)
                p = dict(what=f"{name}, map {m}", K=values.shape[0], n_v=s["v"][2], n_w=s["w"][1], weights=[s["weights"][k] for k in ORDER],
                         has_togo=int(case["togo"] is not None), values=np.ascontiguousarray(values))
                p["scores"], p["pick"] = expected(p)
                assert p["scores"].tolist() == want["scores"][m].tolist()
                if want["info"][m, 4] == 0:
                    assert p["pick"] == want["best"][m]
                out.append(p)
        rng = np.random.default_rng(5)
        for n_v, n_w, share, levels in ((1, 1, 1.0, 1), (4, 9, 1.0, 1), (4, 9, 0.5, 2), (64, 63, 0.3, 3), (7, 129, 0.0, 2), (63, 65, 0.01, 1),
                                        (5, 5, 0.5, 4), (2, 3, 1.0, 2)):
            K = n_v * n_w
            values = np.stack([rng.choice([3, 700, rollout_ref.UNREACHED], K), rng.integers(0, levels, K), rng.integers(0, levels, K) * 5,
                               np.where(rng.random(K) < share, 15, rng.choice([0, 1, 3, 7], K))], axis=1).astype(np.int32)
            for weights, has_togo in (([0, 0, 0, 0, 0], 0), ([1, 1, 1, 0, 0], 0), ([32767, 32767, 32767, 32767, 32767], 1), ([0, 2, 1, 5, 5], 1)):
                p = dict(what=f"drawn {n_v} x {n_w}, weights {weights}", K=K, n_v=n_v, n_w=n_w, weights=weights, has_togo=has_togo,
                         values=np.ascontiguousarray(values))
                p["scores"], p["pick"] = expected(p)
                out.append(p)
        _PROBLEMS.append(out)
    return _PROBLEMS[0]


def compile_host(out, flags):
    return subprocess.run([CXX, "-std=c++17", "-O2", *flags, "-I", os.path.join(REPO, "camradepth_amd", "csrc"),
                           os.path.join(REPO, "tests", "rollout_pick_host.cpp"), "-o", out], capture_output=True, text=True)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert CXX is not None, "no host C++ compiler"
    lib = str(tmp_path_factory.mktemp("rollout_pick") / "librollout_pick_host.so")
    r = compile_host(lib, ["-shared", "-fPIC"])
    assert r.returncode == 0, r.stderr[-2000:]
    so = ctypes.CDLL(lib)
    so.rp_pick.restype = ctypes.c_int
    so.rp_pick.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]
    return so


def test_the_problems_cover_ties_and_every_level_of_the_order():
    ps = problems()
    assert len(ps) >= 40 and any(p["pick"] < 0 for p in ps) and any(p["pick"] >= 0 for p in ps)
    tied = [p for p in ps if p["pick"] >= 0 and ((p["scores"] == p["scores"][p["pick"]]) & ((p["values"][:, 3] & 8) != 0)).sum() > 1]
    assert len(tied) >= 8 and any(p["scores"].max() > 2 ** 45 for p in ps)
    # the order itself, on three candidates of a 3 x 5 plan: a lower score, then the lesser turn, then the larger speed, then the lower k
    b = rollout_ref.better
    assert b((True, 1, 14), (True, 2, 7), 5) and b((True, 1, 7), (True, 1, 6), 5) and b((True, 1, 12), (True, 1, 7), 5)
    assert b((True, 1, 6), (True, 1, 8), 5) and b((True, 9, 0), (False, 0, 7), 5) and b((False, 5, 3), (False, 0, 4), 5)


def test_the_scores_and_the_pick_in_natural_and_in_shuffled_order(host):
    for p in problems():
        weights = np.asarray(p["weights"], np.int32)
        for seed in SEEDS:
            scores = np.full(p["K"], -7, np.int64)
            pick = host.rp_pick(p["values"].ctypes.data, p["K"], p["n_v"], p["n_w"], weights.ctypes.data, p["has_togo"], seed, scores.ctypes.data)
            assert pick == p["pick"] and scores.tolist() == p["scores"].tolist(), (p["what"], seed, pick, p["pick"])


def test_score_and_pick_under_sanitizers_as_a_process(tmp_path):
    """tests/rollout_pick_host.cpp with AddressSanitizer and UBSan, a program of its own, on a share of the problems."""
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
    ps = problems()[::2]
    lines = [str(len(ps))]
    for p in ps:
        lines += [f"{p['K']} {p['n_v']} {p['n_w']}", " ".join(str(w) for w in p["weights"]), str(p["has_togo"])]
        lines += [" ".join(str(int(v)) for v in row) + f" {int(s)}" for row, s in zip(p["values"], p["scores"])]
        lines.append(str(p["pick"]))
    (tmp_path / "problems.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "rollout_pick_main")
    r = compile_host(exe, flags)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, str(tmp_path / "problems.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
