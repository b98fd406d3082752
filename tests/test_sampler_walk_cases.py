"""The cases of tests/sampler_walk_util.py, without a GPU: the replay of the reference's walk gives the oracle's counts at
every capacity the GPU test uses, the oracle's values at the replayed (segment, time) lie within the Horner bound of the exact
ones, the host model of the kernel's chunking emits the replay's samples, and every case contains the edge it is named for
(so that an edit of a case cannot lose its edge unnoticed)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import sampler_walk_util as w

CASE_IDS = [c[0] for c in w.CASES]
LONG = 450   # paths with more samples are evaluated exactly on their first and last 70 only


@pytest.mark.parametrize("index", range(len(w.CASES)), ids=CASE_IDS)
def test_the_replay_counts_as_the_oracle_does(index):
    _, seg_times, dt, _ = w.CASES[index]
    coeffs = w.case_coeffs(index)
    top = max(w.case_capacities(index))
    all_samples, n_all = w.replay(seg_times, dt, top)
    for cap in w.case_capacities(index):
        samples, n = w.replay(seg_times, dt, cap)
        _, n_oracle = po.sample_trajectory(coeffs, seg_times, dt, 0, cap)
        assert n == n_oracle == min(n_all, cap + 1), (cap, n, n_oracle, n_all)
        assert len(samples) == n and samples == all_samples[:n]   # a smaller capacity cuts the same walk short
        model = w.chunk_model(seg_times, dt, cap)
        assert model["count"] == n and model["samples"] == samples, cap   # the chunked walk is the same walk
    # the counts-only call (capacity 0) reports "more than fit" = 1 for a path with a sample
    assert w.replay(seg_times, dt, 0)[1] == min(n_all, 1) == w.chunk_model(seg_times, dt, 0)["count"]


@pytest.mark.parametrize("dt", sorted({c[2] for c in w.CASES}))
def test_every_path_at_every_sampling_period_counts_as_the_oracle_does(dt):
    """the GPU test compares EVERY path with the replay at every case's dt and at all of that dt's capacities, as
    min(replay at the largest capacity, capacity + 1): the same figure from the oracle, for each such (path, dt, capacity)"""
    caps = w.dt_capacities(dt)
    assert caps[-1] == (w.TABLE_CAPACITY if dt == w.TABLE_DT else w.STANDARD_CAPACITIES[-1])
    for index, (name, seg_times, _, _) in enumerate(w.CASES):
        coeffs = w.case_coeffs(index)
        samples, n_all = w.replay(seg_times, dt, w.STANDARD_CAPACITIES[-1])
        assert len(samples) == n_all
        for cap in caps:
            _, n_oracle = po.sample_trajectory(coeffs, seg_times, dt, 0, cap)
            assert n_oracle == min(n_all, cap + 1), (name, dt, cap, n_oracle, n_all)
        assert w.chunk_model(seg_times, dt, caps[-1])["samples"] == samples[:caps[-1] + 1], (name, dt)


@pytest.mark.parametrize("index", range(len(w.CASES)), ids=CASE_IDS)
def test_the_oracles_values_lie_within_the_horner_bound_of_the_exact_ones(index):
    _, seg_times, dt, _ = w.CASES[index]
    coeffs = w.case_coeffs(index)
    cap = max(w.case_capacities(index))
    samples, n = w.replay(seg_times, dt, cap)
    values, n_oracle = po.sample_trajectory(coeffs, seg_times, dt, 0, cap)
    assert n_oracle == n
    rows = min(n, cap)
    check = range(rows) if rows <= LONG else list(range(70)) + list(range(rows - 70, rows))
    two_pi = 2 * w.pi_exact()
    worst = 0.0
    for k in check:
        seg, tau = samples[k]
        exact, bound = w.exact_state(coeffs[seg], tau, 0), w.horner_bound(coeffs[seg], tau, 0)
        for d in range(4):
            err = abs(Fraction(float(values[k, d])) - exact[d])
            if d == 3:   # the oracle's heading is not wrapped
                err = err % two_pi
                err = min(err, two_pi - err)
            assert err <= bound[d], (k, d, seg, tau, float(err), float(bound[d]))
            worst = max(worst, float(err / bound[d]))
    print("WALK CASE %s: %d samples, oracle order 0 at most %.3f of the bound" % (w.CASES[index][0], rows, worst))


@pytest.mark.parametrize("index", range(len(w.CASES)), ids=CASE_IDS)
def test_every_case_contains_its_edge(index):
    name, seg_times, dt, want = w.CASES[index]
    got = w.case_edges(seg_times, dt)
    assert want and {k: got[k] for k in want} == want, (name, got)


def test_the_edges_of_the_issue_are_all_somewhere():
    """each edge of the list is reached by at least one case, at one of the capacities the GPU test runs"""
    edges = [w.case_edges(c[1], c[2]) for c in w.CASES]
    for key in ("boundary_hits", "multi_carries", "zero_segments_passed", "past_end", "t_end_on_grid", "t_end_is_dt",
                "t_end_below_dt", "chunks_last_63", "full_chunks", "chunks_m_62_to_64", "flushes_at_192", "buffer_full_at_end",
                "misfit_flushes", "no_sample", "never_ends"):
        assert any(e[key] for e in edges), key
    # a capacity inside a chunk, on a chunk edge and on the buffer's edge; 193 parked samples = a flush of 192 and one more
    for cap, parked in ((16, [17]), (64, [65]), (191, [192]), (192, [192, 1]), (193, [192, 2])):
        m = w.chunk_model([60.0], 0.2, cap)
        assert m["count"] == cap + 1 and m["flushes"] == parked, (cap, m["flushes"])
    # the LDS route: 256 segments need more than the 64 KB a launch gets by default
    assert 8 * (256 * 41 + w.SAMPLE_BUFFER) + 2 * w.SAMPLE_BUFFER > 64 * 1024
    # the table-edge cases sit around the last entry of the smallest table (capacity + 80 = 1104 entries, A[1103] the last)
    assert w.TABLE_CAPACITY + 80 == 1104
    for name, seg_times, dt, want in w.CASES:
        if dt == w.TABLE_DT:
            n = want["samples"]
            assert (n - 1) * dt < seg_times[0] < n * dt
    acc = 0.0
    for k in range(1104):   # (13/32 and its multiples are exact: the table holds k dt itself)
        assert acc == k * w.TABLE_DT
        acc += w.TABLE_DT


def test_the_heading_passes_the_seam():
    """on at least three cases the unwrapped heading at the replayed samples crosses odd multiples of pi several times, and
    exact_state's order-0 heading is the value in (-pi, pi]"""
    pi = w.pi_exact()
    sweeping = 0
    for index, (name, seg_times, dt, _) in enumerate(w.CASES):
        coeffs = w.case_coeffs(index)
        assert np.all(np.isfinite(coeffs)) and np.all(coeffs != 0.0) and np.max(np.abs(coeffs)) <= 2e3
        assert np.any(coeffs > 0) and np.any(coeffs < 0)
        samples, n = w.replay(seg_times, dt, 500)
        turns = [math.floor((float(np.polyval(coeffs[seg, 3, ::-1], tau)) + math.pi) / (2 * math.pi)) for seg, tau in samples[:500]]
        crossings = sum(1 for a, b in zip(turns[:-1], turns[1:]) if a != b)
        sweeping += crossings >= 3
        for seg, tau in samples[:3] + samples[-3:]:
            y = w.exact_state(coeffs[seg], tau, 0)[3]
            assert -pi < y <= pi
            raw = sum(Fraction(float(c)) * Fraction(float(tau)) ** j for j, c in enumerate(coeffs[seg, 3]))
            assert ((raw - y) / (2 * pi)).denominator == 1
    assert sweeping >= 3, sweeping


def test_exact_state_and_the_bound_on_a_polynomial_known_in_closed_form():
    """(1 + t)^9 and its derivatives at dyadic t are exact rationals; the bound is gamma_{2 (9 - k) + 1} (1 + |t|)^(9 - k) 9!/(9-k)!"""
    c = np.zeros((4, 10))
    c[:] = [math.comb(9, j) for j in range(10)]
    c[1] *= -1.0
    for t in (0.0, 0.375, 2.5, 1e-3):
        tf = Fraction(float(t))
        for k in range(5):
            ff = math.factorial(9) // math.factorial(9 - k)
            v = w.exact_state(c, t, k)
            want = ff * (1 + tf) ** (9 - k)
            assert v[0] == want and v[1] == -want and v[2] == want
            if k > 0:
                assert v[3] == want
            n = 2 * (9 - k) + 1
            assert w.horner_bound(c, t, k)[0] == Fraction(n, 2 ** 53 - n) * want
    assert w.exact_state(c, 0.0, 0)[3] == 1 and abs(w.exact_state(c, 0.375, 0)[3] - (Fraction(11, 8) ** 9 - 6 * w.pi_exact())) == 0
    got = np.array([[float(x) for x in w.exact_state(c, 0.375, k)] for k in range(5)])
    assert np.max(w.state_errors(c, 0.375, got)) <= 0.5   # correctly rounded values: half an ulp against 9 .. 19 roundings
    got[2, 1] = np.nextafter(got[2, 1], np.inf)
    got[2, 1] += 30 * np.spacing(got[2, 1])
    r = w.state_errors(c, 0.375, got)
    assert r[2, 1] > 1.0 and np.sum(r > 1.0) == 1
    got[0, 0] = np.nan
    assert np.isinf(w.state_errors(c, 0.375, got)[0, 0])
