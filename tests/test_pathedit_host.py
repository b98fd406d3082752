"""csrc/mrs_tg_pathedit.hpp on the CPU (tests/host/pathedit_harness.cpp, plain g++ and once more under ASan + UBSan, a
stand-alone program): the thinning decision in the reference's serial loop, in the 64-candidate window a wavefront uses and
through policy::preprocess against the oracle's mto_preprocess_path; the mid-point rule against a restatement of optimize()'s
insertion loop as written, on the oracle's mto_interpolate_point; the backward sums against a restatement in Python floats in
the stated order.  Everything bit for bit; NaN is ordinary data here."""
import numpy as np
import pytest

from tests import pathedit_util as pu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return pu.build_harness(tmp_path_factory.mktemp("pathedit_host"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    return pu.build_harness(tmp_path_factory.mktemp("pathedit_host_san"), sanitize=True)


def _check_thinning(problems, got):
    for p, g in zip(problems, got):
        rows, stop = pu.oracle_thin(p)
        name = p["name"]
        assert np.array_equal(g["serial"], g["window"]), name           # the window is the serial loop
        assert pu.same_bits(p["waypoints"][g["serial"]], rows), name    # ... which is the oracle, rows and stop_at
        assert np.array_equal(p["stop_at"][g["serial"]], stop), name
        assert pu.same_bits(g["rows"], rows) and np.array_equal(g["stop_at"], stop), name   # policy::preprocess on top of it


def _seeded_thin_problems():
    rng = np.random.default_rng(2024)
    sizes = [2, 3, 4, 63, 64, 65, 66, 128, 129, 130, 256, 257] + [int(v) for v in rng.integers(2, 258, size=138)]
    problems = []
    for q, V in enumerate(sizes):
        for straight in (False, True):
            w = pu.random_clustered_path(rng, V, straight=straight)
            problems.append(pu.thin_problem(w, 0.05 if q % 3 else 0.5, stop_at=rng.integers(0, 2, V),
                                            straightener=(0.05, 0.2) if straight else None, name="seeded_%d_%d" % (q, straight)))
    return problems


def test_thinning_is_the_oracle_on_a_seeded_set(harness):
    problems = _seeded_thin_problems()
    assert len(problems) == 300
    got = pu.run_thin(harness, problems)
    _check_thinning(problems, got)
    dropped = sum(p["waypoints"].shape[0] - g["serial"].size for p, g in zip(problems, got))
    by_line = sum(p["waypoints"].shape[0] - g["serial"].size for p, g in zip(problems, got) if p["straightener"])
    assert dropped > 2000 and by_line > 1000, (dropped, by_line)


def test_thinning_fixed_cases(harness):
    cases = pu.fixed_thin_cases()
    problems = [p for p, _ in cases]
    got = pu.run_thin(harness, problems)
    _check_thinning(problems, got)
    for (p, kept), g in zip(cases, got):
        if kept is not None:
            assert g["window"].size == kept, (p["name"], g["window"].size, kept)
    nan_case = [g for (p, _), g in zip(cases, got) if p["name"] == "nan_kept"][0]
    assert 1 in nan_case["window"]      # the vertex with the NaN coordinate: every comparison with it is false


def test_window_jumps_end_where_they_are_placed(harness):
    rng = np.random.default_rng(5)
    problems, wanted = [], []
    for V, kept in pu.window_cases(rng):
        w, k = pu.path_from_kept(V, kept, rng)
        problems.append(pu.thin_problem(w, 5.0, stop_at=rng.integers(0, 2, V), name="window_%d_%s" % (V, kept)))
        wanted.append(k)
    got = pu.run_thin(harness, problems)
    _check_thinning(problems, got)
    for p, g, k in zip(problems, got, wanted):
        assert np.array_equal(g["window"], k), p["name"]


def _subdivide_problems():
    rng = np.random.default_rng(77)
    problems = [pu.subdivide_problem(pu.random_path(rng, 2), [1], fs, name="S1_unsafe_fs%d" % fs) for fs in (0, 1)]
    problems += [pu.subdivide_problem(pu.random_path(rng, 2), [0], 0, name="S1_safe")]
    w3 = pu.random_path(rng, 3)
    for fs in (0, 1):
        problems.append(pu.subdivide_problem(w3, [1, 0], fs, stop_at=[0, 1, 0], name="V3_first_unsafe_fs%d" % fs))
        problems.append(pu.subdivide_problem(w3, [1, 1], fs, stop_at=[0, 1, 0], name="V3_both_unsafe_fs%d" % fs))
    for S in (2, 7, 63, 64, 65, 128, 256):
        w = pu.random_path(rng, S + 1)
        stop = rng.integers(0, 2, S + 1)
        for pattern, flags in pu.flag_patterns(S, rng).items():
            for fs in (0, 1):
                problems.append(pu.subdivide_problem(w, flags, fs, stop_at=stop, name="S%d_%s_fs%d" % (S, pattern, fs)))
    seam = pu.seam_path()
    problems.append(pu.subdivide_problem(seam, np.ones(seam.shape[0] - 1), 1, name="seam"))
    return problems


def _check_subdivision(problems, got):
    for p, g in zip(problems, got):
        rows, stop = pu.reference_subdivide(p)
        assert pu.same_bits(g["rows"], rows), p["name"]
        assert np.array_equal(g["stop_at"], stop), p["name"]
        copies = g["inserted"] == 0
        assert np.array_equal(g["source"][copies], np.arange(p["waypoints"].shape[0])), p["name"]
        assert np.all(g["source"][1:][~copies[1:]] == g["source"][:-1][~copies[1:]]), p["name"]   # a mid-point follows its segment's first vertex
        assert not np.any(g["stop_at"][~copies])


def test_subdivision_is_the_reference_loop(harness):
    problems = _subdivide_problems()
    got = pu.run_subdivide(harness, problems)
    _check_subdivision(problems, got)
    by_name = {p["name"]: g for p, g in zip(problems, got)}
    assert by_name["S1_unsafe_fs0"]["rows"].shape[0] == 3       # V <= 2: the first segment is subdivided whatever the flag says
    assert by_name["V3_first_unsafe_fs0"]["rows"].shape[0] == 3 and by_name["V3_first_unsafe_fs1"]["rows"].shape[0] == 4
    assert by_name["V3_both_unsafe_fs0"]["rows"].shape[0] == 4   # (the size is tested before anything is inserted)
    assert by_name["S256_all_fs1"]["rows"].shape[0] == 513
    seam = by_name["seam"]["rows"]
    assert np.all((seam[:, 3][by_name["seam"]["inserted"] == 1] >= 0.0))   # radians::interp answers in [0, 2 pi)


def _vjp_problems():
    rng = np.random.default_rng(9)
    problems = []
    for S, pattern in [(1, "all"), (2, "alternating"), (5, "random"), (64, "all"), (65, "odd"), (256, "random"), (7, "none")]:
        V = S + 1
        flags = pu.flag_patterns(S, rng)[pattern]
        source, inserted = [], []
        for i in range(V):
            source.append(i), inserted.append(0)
            if i < S and flags[i]:
                source.append(i), inserted.append(1)
        up = pu.dyadic(rng, 4 * len(source)).reshape(-1, 4) * (1.0 + 2.0 ** -40)   # halves of these round
        problems.append(dict(n_in=V, source=np.array(source), inserted=np.array(inserted, dtype=np.uint8), upstream=up))
    for V, kept in [(2, [0, 1]), (6, [0, 2, 5]), (130, [0] + list(range(101, 130)))]:
        up = pu.dyadic(rng, 4 * len(kept)).reshape(-1, 4)
        problems.append(dict(n_in=V, source=np.array(kept), inserted=None, upstream=up))
    return problems


def test_backward_sums_in_the_stated_order(harness):
    problems = _vjp_problems()
    got = pu.run_vjp(harness, problems)
    zero_rows = 0
    for p, g in zip(problems, got):
        ref = pu.reference_vjp(p["n_in"], p["source"], p["inserted"], p["upstream"])
        assert pu.same_bits(g, ref)
        if p["inserted"] is None:
            dropped = np.setdiff1d(np.arange(p["n_in"]), p["source"])
            assert np.all(pu.bits(g[dropped]) == 0)      # +0.0, not -0.0
            zero_rows += dropped.size
    assert zero_rows > 100


def test_everything_once_more_under_sanitizers(harness_san):
    thin = [p for p, _ in pu.fixed_thin_cases()] + _seeded_thin_problems()[:40]
    _check_thinning(thin, pu.run_thin(harness_san, thin))
    sub = _subdivide_problems()
    _check_subdivision(sub, pu.run_subdivide(harness_san, sub))
    vjp = _vjp_problems()
    for p, g in zip(vjp, pu.run_vjp(harness_san, vjp)):
        assert pu.same_bits(g, pu.reference_vjp(p["n_in"], p["source"], p["inserted"], p["upstream"]))
