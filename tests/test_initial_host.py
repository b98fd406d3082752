"""The initial condition, the decision table and the splice's walk on the CPU: csrc/mrs_tg_initial.hpp (what the kernels of
mrs_tg_initial.hip run) compiled by g++ into tests/host/initial_harness.cpp NEXT TO the public host header
include/mrs_tg_initial_condition.hpp, the two asked the same questions: the bins at every edge, the whole branch table of
prepareInitialCondition, and the in-place chunk walk against memmove + memcpy.  Everything is exact.  No GPU."""
import numpy as np
import pytest

from tests import initial_util as iu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return iu.build_harness(tmp_path_factory.mktemp("initial"))


def _check_offsets(exe):
    xs = iu.offset_arguments()
    got = iu.run_offsets(exe, xs)
    assert np.array_equal(got[:, 0], got[:, 1]), [(x, a, b) for x, (a, b, _, _) in zip(xs, got) if a != b]
    assert np.array_equal(got[:, 2], got[:, 3]), [(x, a, b) for x, (_, _, a, b) in zip(xs, got) if a != b]
    # the arguments do what they are there for: every k of 1 .. 46 is met from both sides of its edge, the ends saturate
    assert set(range(1, 47)) <= set(got[:, 0].tolist()) and set(range(1, 47)) <= set(got[:, 2].tolist())
    edges = sum(1 for i in range(len(xs) - 1) if xs[i + 1] == np.nextafter(xs[i], np.inf) and got[i, 0] != got[i + 1, 0])
    assert edges >= 46, edges
    assert got[xs.index(1.0e300), 0] == 2 ** 31 - 1 and got[xs.index(-1.0e300), 0] == -2 ** 31
    assert got[-1, 0] == 2 ** 31 - 1 and got[-1, 2] == 2 ** 31 - 1 and np.isnan(xs[-1])


def _check_decisions(exe):
    rows = iu.branch_table()
    res = iu.run_decisions(exe, rows)
    seen = set()
    for r, q in zip(rows, res):
        assert q["rc"] == 0 and q["source"] >= 0, (r, q)
        assert q["word"] == iu.expected_word(q["has"], q["future"], q["drop"], q["source"]), (r, q)
        assert q["k"] == q["k_public"], (r, q)
        seen.add(q["word"])
    # every case of the table is met, with and without the dropped waypoint
    assert {0, iu.PREPEND | iu.FROM_TRACKER, iu.PREPEND | iu.FROM_UAV, iu.DROP_FIRST, iu.PREPEND | iu.FROM_TRACKER | iu.DROP_FIRST, iu.PREPEND | iu.FROM_UAV | iu.DROP_FIRST,
            iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION | iu.DROP_FIRST, iu.PREPEND | iu.FROM_FUTURE | iu.FROM_PREDICTION} <= seen
    # what the public function refuses, decide() marks invalid and nothing else
    nan = float("nan")
    bad = [dict(tracker=1, age=0.1, uav=1, dont=0, offset=nan, n_wp=2, n_pred=iu.N_PRED),
           dict(tracker=1, age=nan, uav=1, dont=0, offset=0.5, n_wp=2, n_pred=iu.N_PRED),
           dict(tracker=1, age=0.1, uav=1, dont=0, offset=0.5, n_wp=2, n_pred=65)]      # beyond the harness's pred_capacity of 64
    got = iu.run_decisions(exe, bad)
    assert [q["word"] for q in got] == [iu.INVALID] * 3 and [q["rc"] for q in got[:2]] == [-1, -1]
    # a NaN age of a tracker command that is absent is no error, on either side
    absent = iu.run_decisions(exe, [dict(tracker=0, age=nan, uav=1, dont=0, offset=0.5, n_wp=2, n_pred=iu.N_PRED)])[0]
    assert absent["rc"] == 0 and absent["word"] == iu.PREPEND | iu.FROM_UAV | iu.DROP_FIRST


def _check_splices(exe):
    cases = iu.splice_cases()
    assert len(cases) == 7 * 6 * 2
    got = iu.run_splices(exe, cases)
    for (n, k, cap), (count_public, count_walk, same) in zip(cases, got):
        assert count_public == n + k and count_walk == n + k and same == 1, (n, k, cap, count_public, count_walk, same)


def test_bins_agree_with_the_public_header_at_every_edge(harness):
    _check_offsets(harness)


def test_decide_is_the_public_branch_table(harness):
    _check_decisions(harness)


def test_chunk_walk_is_the_public_splice(harness):
    _check_splices(harness)


def test_harness_is_clean_under_the_sanitizers(tmp_path):
    exe = iu.build_harness(tmp_path, sanitize=True)
    _check_offsets(exe)
    _check_decisions(exe)
    _check_splices(exe)
