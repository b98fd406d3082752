"""The request's vertices and limits on the CPU: csrc/mrs_tg_request.hpp (what the kernels of mrs_tg_request.hip run) compiled by
g++ into tests/host/request_harness.cpp NEXT TO restatements of the reference's vertex lines and limit lines (the policy layer's
policy::build_vertices, a call of the header by now, is held to the vertex restatement too).  Vertices and limits are compared in bits; the backward passes against central differences of the
forward -- exact for every copy and for the fallback's one multiplication, and for the heading, whose forward rounds in its fmod
and additions, within the bound stated at HEADING_FD_BOUND.  No GPU."""
import numpy as np
import pytest

from tests import request_util as ru

# A heading of the forward is the raw heading plus a multiple of 2 pi, rounded in the unwrap's additions: each output heading is
# within a few ulps of its magnitude (below 64 here: ulp 1.4e-14) of the exact value.  A central difference with step 0.25
# divides the difference of two such values by 0.5, and an input heading reaches the two heading outputs (waypoint and value) of
# every vertex from its own on, at most 22 elements for the 11 vertices used, each weighted by an upstream of at most 5:
# 22 * 5 * 4 * 1.4e-14 / 0.5 < 2e-11.
HEADING_FD_BOUND = 2e-11


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ru.build_harness(tmp_path_factory.mktemp("request"))


def check_vertices(exe):
    problems = ru.vertex_problems()
    assert len(problems) == 8 * 3 * 2 * 2
    got = ru.run_vertices(exe, problems)
    bad = [(q["V"], q["d"], q["has"], g.tolist()) for q, g in zip(problems, got) if not g.all()]
    assert not bad, bad


def check_limits(exe):
    rows = ru.limits_table() + ru.edge_rows()
    assert len(rows) == 2 * 8 * 2 * 2 * 3 + 12
    branch, lim, ref = ru.run_limits(exe, rows)
    for r, w, a, b in zip(rows, branch, lim, ref):
        assert a.tobytes() == b.tobytes(), (r["name"], r["flags"], r["fallback"], a, b)
        assert w == r["expect"], (r["name"], r["flags"], r["fallback"], w, r["expect"])
        assert a.tobytes() == ru.expected_limits(r).tobytes(), (r["name"], a)
    seen = set(int(w) for w in branch)
    assert any(w & ru.OVERRIDE_REFUSED for w in seen) and any(w & ru.OVERRIDDEN and w & ru.FALLBACK for w in seen)
    # a NaN in an operand of can_change refuses the override; a NaN constraint follows the comparison as written
    nan_rows = []
    for k in range(6):
        r = dict(rows[0], flags=ru.REQ_OVERRIDE, has=1, fallback=0, o=ru.OVERRIDE.copy(), state=ru.state_block(**ru.BELOW))
        r["o"][k] = float("nan")
        nan_rows.append(r)
    r = dict(rows[0], flags=ru.REQ_OVERRIDE, has=1, fallback=0, o=ru.OVERRIDE.copy(), state=ru.state_block(**ru.BELOW))
    r["state"][1, 0] = float("nan")
    nan_rows.append(r)
    branch, lim, ref = ru.run_limits(exe, nan_rows)
    assert all(w & ru.OVERRIDE_REFUSED and not w & ru.OVERRIDDEN for w in branch), branch
    assert lim.tobytes() == ref.tobytes()


def check_backward(exe):
    rng = np.random.default_rng(21)
    problems = [ru.dyadic_vertex_problem(rng, V, d, has) for V in (2, 3, 4, 11) for d in (2, 3, 4) for has in (0, 1)]
    for q, (grad, fd) in zip(problems, ru.run_backward(exe, "G", problems)):
        V = q["V"]
        heading = np.zeros(V * 4 + 16, dtype=bool)
        heading[3:V * 4:4] = True
        heading[V * 4 + 3] = True            # the state's heading: the analytic gradient is zero
        assert np.array_equal(grad[~heading], fd[~heading]), (V, q["d"], q["has"])
        assert np.abs(grad[heading] - fd[heading]).max() <= HEADING_FD_BOUND, (V, np.abs(grad[heading] - fd[heading]).max())
        assert np.all(grad[V * 4:V * 4 + 4] == 0.0)
        if q["has"]:
            assert np.any(grad[V * 4 + 4:] != 0.0)
        else:
            assert np.all(grad[V * 4:] == 0.0)
    rows = ru.backward_limit_rows()
    for r, (grad, fd) in zip(rows, ru.run_backward(exe, "H", rows)):
        assert np.array_equal(grad, fd), (r["name"], r["flags"], r["fallback"], grad, fd)


def test_vertices_have_the_bytes_of_the_host_builder(harness):
    check_vertices(harness)


def test_limits_follow_the_reference_on_the_whole_branch_table(harness):
    check_limits(harness)


def test_backward_passes_equal_central_differences(harness):
    check_backward(harness)
