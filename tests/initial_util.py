"""What the tests of the initial condition, the prepended waypoint and the prediction splice as plan steps share
(mrs_tg_plan_initial_condition, mrs_tg_plan_prepend_initial_condition, mrs_tg_plan_splice_prediction, csrc/mrs_tg_initial.hpp,
DESIGN.md section 11g): the arguments at which the two bins change, the branch table of prepareInitialCondition, numpy
restatements of the edit and of the splice's index maps, and the CPU harness tests/host/initial_harness.cpp."""
import itertools

import numpy as np

from tests import host_harness as hh

# MRS_TG_IC_* (include/mrs_tg.h) and the flags input of mrs_tg_plan_initial_condition
PREPEND, FROM_FUTURE, DROP_FIRST, FROM_TRACKER, FROM_UAV, FROM_PREDICTION, INVALID = 1, 2, 4, 8, 16, 32, 64
FLAG_TRACKER, FLAG_UAV, FLAG_DONT_PREPEND = 1, 2, 4
N_PRED = 41                                       # rows of an MPC prediction
SPLICE_N = (0, 1, 63, 64, 65, 128, 129)           # sample rows: around the chunk of 64 rows and two of them
SPLICE_K = (1, 2, 63, 64, 65, 130)                # prefix rows: below, at and above a chunk, above two


def _around(x):
    """x and its neighbouring doubles, two on each side (the offset at which a quotient is integral need not be a double)"""
    lo1 = np.nextafter(x, -np.inf)
    hi1 = np.nextafter(x, np.inf)
    return [float(v) for v in (np.nextafter(lo1, -np.inf), lo1, x, hi1, np.nextafter(hi1, np.inf))]


def offset_arguments():
    """the arguments the two bins are compared at: every bin edge m = 1 .. 45 of sample_offset (offset = 2 (0.2 m + 0.01)) and of
    splice_offset (age = 0.2 m + 0.01) with its neighbours, 0.2 with its neighbours, negative, huge and NaN arguments"""
    xs = []
    for m in range(0, 46):
        xs += _around(2.0 * (0.2 * m + 0.01)) + _around(0.2 * m + 0.01)
    xs += _around(0.2) + _around(0.0) + _around(0.01) + _around(0.02)
    xs += [-0.0, -0.05, -1.0, -17.3, -1.0e9, -1.0e300, 1.0e9, 4.294967296e8, 8.589934592e8, 1.0e300, float("inf"), float("-inf"),
           float("nan")]
    return xs


def offset_at_k(k):
    """an offset well inside the bin of sample_offset == k (k >= 2)"""
    return 2.0 * (0.2 * (k - 1.5) + 0.01)


def branch_table():
    """prepareInitialCondition's branch table as rows (tracker, age, uav, dont_prepend, offset, n_waypoints, n_pred): tracker
    command present / absent / stale at 1.0 and its neighbours, UAV state present / absent, dont_prepend, offset <= 0.2 or > 0.2
    with k <= n_pred - 1 or k = n_pred, one or two requested waypoints"""
    one = 1.0
    trackers = [(0, 0.0), (1, 0.1), (1, float(np.nextafter(one, 0.0))), (1, one), (1, float(np.nextafter(one, 2.0))), (1, 7.5)]
    # (offset, n_pred): at or below the threshold; above it inside the prediction (k = 7 <= 40); k = n_pred - 1; k = n_pred
    offsets = [(0.0, N_PRED), (0.2, N_PRED), (float(np.nextafter(0.2, 1.0)), N_PRED), (offset_at_k(7), N_PRED),
               (offset_at_k(7), 8), (offset_at_k(7), 7), (offset_at_k(7), 0)]
    rows = []
    for (tr, age), uav, dont, (off, n_pred), n_wp in itertools.product(trackers, (0, 1), (0, 1), offsets, (1, 2)):
        rows.append(dict(tracker=tr, age=age, uav=uav, dont=dont, offset=off, n_wp=n_wp, n_pred=n_pred))
    return rows


def expected_word(has_initial_condition, from_future, drop_first, source):
    """the decision word a public answer amounts to; source: FROM_TRACKER / FROM_UAV / FROM_PREDICTION of the waypoint, 0 none"""
    return (PREPEND if has_initial_condition else 0) | (FROM_FUTURE if from_future else 0) | (DROP_FIRST if drop_first else 0) | source


def prepend_numpy(vertex_offsets, waypoints, stop_at, decision, initial):
    """the edit of :649-672 on a packed batch -> (offsets [P + 1], rows, stop_at, source)"""
    vo = np.asarray(vertex_offsets, dtype=np.int64)
    rows, stops, source, off = [], [], [], [0]
    for p in range(vo.size - 1):
        idx = list(range(vo[p], vo[p + 1]))
        if decision[p] & DROP_FIRST and idx:
            idx = idx[1:]
        if decision[p] & PREPEND:
            rows.append(initial[p, 0])
            stops.append(0)
            source.append(-1)
        for v in idx:
            rows.append(waypoints[v])
            stops.append(stop_at[v])
            source.append(v)
        off.append(len(rows))
    return (np.array(off, dtype=np.int32), np.array(rows, dtype=np.float64).reshape(-1, 4), np.array(stops, dtype=np.uint8),
            np.array(source, dtype=np.int32))


def splice_cases():
    """(n, k, capacity) over SPLICE_N x SPLICE_K x {n + k, n + k - 1}"""
    return [(n, k, n + k - short) for n in SPLICE_N for k in SPLICE_K for short in (0, 1)]


# ---- the CPU harness -----------------------------------------------------------------------------------------------------------

def build_harness(tmp_path, sanitize=False):
    return hh.build("initial_harness.cpp", tmp_path, sanitize=sanitize)


def run_offsets(exe, xs):
    """-> [len(xs)][4] int64: sample_offset new, public, splice_offset new, public"""
    out = hh.run(exe, ["O %s\n" % repr(float(x)) for x in xs], len(xs))
    return np.array([[int(t) for t in line.split()] for line in out], dtype=np.int64)


def run_decisions(exe, rows):
    """-> per row dict(word, k, has, future, drop, k_public, source, rc)"""
    lines = ["D %d %s %d %d %s %d %d\n" % (r["tracker"], repr(float(r["age"])), r["uav"], r["dont"], repr(float(r["offset"])),
                                          r["n_wp"], r["n_pred"]) for r in rows]
    res = []
    for line in hh.run(exe, lines, len(rows)):
        new, old = line.split("|")
        word, k = (int(t) for t in new.split())
        has, future, drop, k_public, source, rc = (int(t) for t in old.split())
        res.append(dict(word=word, k=k, has=has, future=future, drop=drop, k_public=k_public, source=source, rc=rc))
    return res


def run_splices(exe, cases):
    """-> [len(cases)][3]: the public count, the walk's count, 1 where the buffers hold the same bytes"""
    out = hh.run(exe, ["S %d %d %d\n" % c for c in cases], len(cases))
    return np.array([[int(t) for t in line.split()] for line in out], dtype=np.int64)
