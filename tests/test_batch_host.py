"""The batch addressing on the CPU: csrc/mrs_tg_batch.hpp (path_of_segment, path_of_vertex, first_segment, segments_of,
first_vertex, path_at -- the map every kernel takes its path from) compiled by g++ into tests/host/batch_harness.cpp, every
segment, vertex and position of a batch against a linear scan of seg_offsets.  No GPU."""
import numpy as np
import pytest

from tests import host_harness as hh

# segment counts per path, and whether the BatchView is coded as uniform (uniform_S = S) or ragged (uniform_S = 0)
BATCHES = {
    "ragged": ([1, 3, 2, 1, 4], False),
    "ragged_longest_last": ([1, 1, 5], False),
    "uniform_3x2": ([2, 2, 2], True),
    "single_path_single_segment": ([1], True),
    "one_path_ragged_coded": ([3], False),   # the search with hi - lo = 1: the loop body never runs
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return hh.build("batch_harness.cpp", tmp_path_factory.mktemp("batch"))


def _lines(batches):
    lines = []
    for S, uniform in batches:
        offsets = np.concatenate([[0], np.cumsum(S)])
        order = np.argsort(-np.asarray(S), kind="stable")   # longest first, stable: the plan's order
        lines.append("%d %d %s %s\n" % (len(S), S[0] if uniform else 0, " ".join(map(str, offsets)), " ".join(map(str, order))))
    return lines


def _linear_scan(S):
    """what the harness prints, from one pass over seg_offsets per index"""
    offsets = np.concatenate([[0], np.cumsum(S)]).tolist()
    P = len(S)
    out = []
    for s in range(offsets[-1]):        # the path whose segments [offsets[p], offsets[p + 1]) hold s
        out.append(next(p for p in range(P) if offsets[p] <= s < offsets[p + 1]))
    for v in range(offsets[-1] + P):    # path p owns the vertices [offsets[p] + p, offsets[p + 1] + p + 1)
        out.append(next(p for p in range(P) if offsets[p] + p <= v < offsets[p + 1] + p + 1))
    for p in range(P):
        out += [offsets[p], offsets[p + 1] - offsets[p], offsets[p] + p]
    for p in np.argsort(-np.asarray(S), kind="stable").tolist():
        out += [p, offsets[p], offsets[p + 1] - offsets[p], offsets[p] + p]
    return out


def _check(exe, env=None):
    batches = list(BATCHES.values())
    got = hh.run(exe, _lines(batches), len(batches), env=env)
    for (name, (S, _)), line in zip(BATCHES.items(), got):
        assert [int(x) for x in line.split()] == _linear_scan(S), name
    return got


def test_every_segment_vertex_and_position_against_a_linear_scan(harness):
    _check(harness)


def test_uniform_and_ragged_coding_of_the_same_batch_agree(harness):
    a, b = hh.run(harness, _lines([([2, 2, 2], True), ([2, 2, 2], False)]), 2)
    assert a == b


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness):
    san = hh.build("batch_harness.cpp", tmp_path, sanitize=True)
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    assert _check(san, env=env) == _check(harness)
