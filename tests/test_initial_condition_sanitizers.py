"""The initial-condition core (include/mrs_tg_initial_condition.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer: compiled
with plain g++ through tests/host/initial_condition_harness.cpp, which runs the branch table of prepareInitialCondition
(the reference's src/mrs_trajectory_generation.cpp:506-614, :650-655) and the splice (:801-838) on exact-size heap blocks.
No sanitizer report, and every line equals this file's restatement of the reference."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "host", "initial_condition_harness.cpp")
INT32_MAX = 2**31 - 1


def _sat(q):
    """int(q) + 1 clamped to the int32 range"""
    if not q < 2147483647.0:
        return INT32_MAX
    if not q > -2147483649.0:
        return -2**31
    return int(q) + 1


def _k(offset):
    return _sat(math.ceil((offset * 0.50 - 0.01) / 0.2)) if math.isfinite(offset) else INT32_MAX


def _k2(age):
    return _sat(math.floor((age - 0.01) / 0.2))


def _pred(n):
    """HeapPrediction: row i, column c of array a = 100 a + i + c / 8"""
    return [np.array([[100.0 * a + i + c / 8.0 for c in range(4)] for i in range(n)]).reshape(n, 4) for a in range(4)]


POSE = [1.0, -2.0, 3.5, 0.7]
STATE = ([0.4, -0.2, 0.1, 0.05], [0.1, 0.2, -0.3, 0.01], [1.0, -1.0, 0.5, 0.2])
UAV = [0.25, -0.5, 0.0, -1.2]
AGES = [None, 1.0, float(np.nextafter(1.0, 2.0)), 0.3]


def expected_prepare(t, off, n_pred, dont, n_wp, u):
    if math.isnan(off):
        return None
    drop = int(off > 0.2 and n_wp >= 2)
    zero = [0.0] * 4
    none = [0, 0, 0, drop] + [0.0] * 17
    if dont:
        return none
    if AGES[t] is None or AGES[t] > 1.0:
        if not u:
            return none
        wp = list(UAV)
        wp[2] += 1.5
        return [1, 0, 0, drop] + wp + [UAV[3]] + zero * 3
    tracker = [1, 0, 0, drop] + POSE + [POSE[3]] + STATE[0] + STATE[1] + STATE[2]
    if off > 0.2:
        k = _k(off)
        tracker[2] = k
        if k > n_pred - 1:
            return tracker
        pos, vel, acc, jerk = (a[k].tolist() for a in _pred(n_pred))
        return [1, 1, k, drop] + pos + [pos[3]] + vel + acc + jerk
    return tracker


def expected_splice(k, age, n, cap):
    fill = [-1000.0 - i for i in range(4 * cap)]
    if math.isnan(age):
        return -1, None
    if k <= _k2(age) or k <= 0:
        return n, fill
    if k > 41:
        return -1, None
    if n + k > cap:
        return n + k, fill
    return n + k, _pred(41)[0][:k].ravel().tolist() + fill[:4 * n]


@pytest.fixture(scope="module")
def harness_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ic_san") / "initial_condition_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", HARNESS, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    return p.stdout.splitlines()


def test_branch_table_under_sanitizers(harness_output):
    lines = [ln.split() for ln in harness_output if ln.startswith("P ")]
    assert len(lines) == 4 * 9 * 2 * 2 * 2 * 2
    for f in lines:
        t, off, n_pred, dont, n_wp, u, rc = int(f[1]), float(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), int(f[8])
        exp = expected_prepare(t, off, n_pred, dont, n_wp, u)
        if exp is None:
            assert rc == -1, f
            continue
        assert rc == 0, f
        got = [int(x) for x in f[9:13]] + [float(x) for x in f[13:]]
        if got[0]:
            assert got == exp, (f, exp)
        else:
            assert got[:4] == exp[:4], (f, exp)


def test_splice_under_sanitizers(harness_output):
    lines = [ln.split() for ln in harness_output if ln.startswith("S ")]
    assert len(lines) == 7 * 9 * 2 * 2
    for f in lines:
        k, age, n, cap, ret = int(f[1]), float(f[2]), int(f[3]), int(f[4]), int(f[6])
        exp_ret, exp_buf = expected_splice(k, age, n, cap)
        assert ret == exp_ret, (f[:7], exp_ret)
        if ret >= 0:
            assert [float(x) for x in f[7:]] == exp_buf, f[:7]
    assert [ln for ln in harness_output if ln.startswith("E ")] == ["E -1 -1 -1"]
    assert harness_output[-1].startswith("OK ")
