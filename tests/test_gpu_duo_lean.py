"""The lean instantiation of the grouped two-sided solve: same bits as the general one, and chosen exactly where its rule says.

`launch_solve_quad_group` (mrs_tg_quad.hip) sends a grouped dispatch to `solve_duo_group_kernel<WP, true>` when the plan is
whole-uniform -- one length for every path, even and at least 4, and the paths fill every wavefront (n_paths % 8 == 0) -- and
MRS_TG_DUO_UNIFORM, MRS_TG_DUO_STORE_THROUGH and MRS_TG_DUO_LEAN are on; everything else goes to `solve_duo_group_kernel<WP>` as
before.  The lean instantiation is the same arithmetic without activity predicates, clamps and the second store flavour, with
LDS and output addresses that walk by a per-lane stride: what can go wrong is an address or a missing predicate, so every case

  * compares coeffs, cost and status with np.array_equal between four roads over the same inputs: lean (all knobs on),
    MRS_TG_DUO_LEAN=0, MRS_TG_DUO_UNIFORM=0 (the predicated loops and separate pieces: the road tests/test_gpu_duo_bits.py ties
    to recorded bits) and MRS_TG_DUO_STORE_THROUGH=0 -- no tolerance, nothing left out;
  * fills every output with a NaN bit pattern first, inside a larger allocation with guard zones: afterwards the guards are
    untouched and no pattern word is left inside;
  * reads the kernel trace under MRS_TG_TRACE_INSTANTIATIONS=1: `solve_duo_group_kernel<X, true>` on the lean road where the rule
    holds, `solve_duo_group_kernel<X>` on every other road and wherever it does not; and without that knob the family's name.

Shapes, the smallest that can still go wrong (min-snap): lengths 4 (the shortest with three exchange rows), 6, 10, 14 and 16 (either
side of the prologue's 16-element trip) and 24 (the longest routed); 8, 16 and 64 paths per batch (one, two and eight workgroups per
batch); groups of 1, 2, 3 and 16 batches (blockIdx.y at its ends, the last batch's pointers); positions from the value array and
from the waypoint array; moving starts in some wavefronts; one non-plain path (the general step inside the lean kernel); the
routing's negatives (odd lengths, lengths 2 and 3, 12 paths per batch, a ragged plan); and the headline's shape once.

Dispatches this small reach the two-sided kernels only below the saturated-device threshold: MRS_TG_DUO=1 and
MRS_TG_QUAD_MIN_PATHS=0, and the latter is read once per process -- so all cases run in ONE child process (this file as a script)
that writes each case's outcome, and the tests here read them (as tests/test_gpu_pipeline_shortcuts.py does for its knobs)."""
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

PATTERN64 = 0x7FF8DEADBEEF5A5A   # a quiet NaN no solve produces
PATTERN32 = 0x7FC0DEAD           # (status: a float NaN's bits, no status value)
# (MRS_TG_DUO_LEAN, MRS_TG_DUO_UNIFORM, MRS_TG_DUO_STORE_THROUGH); the first is the lean road, the third the reference road
ROADS = (("1", "1", "1"), ("0", "1", "1"), ("1", "0", "1"), ("1", "1", "0"))
LENGTHS, PATHS, GROUPS = (4, 6, 10, 14, 16, 24), (8, 16, 64), (1, 2, 3, 16)


def lean_rule(lengths, n_paths):
    """the launcher's rule, from the plan alone (the knobs are the road's)"""
    return len(set(lengths)) == 1 and lengths[0] >= 4 and lengths[0] % 2 == 0 and n_paths % 8 == 0


def _state(p):
    from mrs_uav_trajectory_generation_amd import problem as pr
    rng = pr.SplitMix64(93000 + p)
    return dict(heading=rng.uniform(-3.0, 3.0), velocity=[rng.uniform(-2.0, 2.0) for _ in range(4)],
                acceleration=[rng.uniform(-1.0, 1.0) for _ in range(4)], jerk=[rng.uniform(-1.0, 1.0) for _ in range(4)])


def _batch(lengths, seed, moving=(), stop=None):
    """one path per entry of lengths; moving: paths that start in motion; stop: (path, vertex) with velocity, acceleration and
    jerk constrained as well (a non-plain interior vertex)"""
    from mrs_uav_trajectory_generation_amd import problem as pr
    parts = []
    for p, S in enumerate(lengths):
        stop_at = None
        if stop is not None and stop[0] == p:
            stop_at = [v == stop[1] for v in range(S + 1)]
        parts.append(pr.build_vertices(pr.random_box_waypoints(S, seed + p), pr.SNAP, stop_at=stop_at,
                                       initial_state=_state(p) if p in moving else None))
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (len(parts), 1)))


def _cases():
    """name -> (lengths, group size, moving paths, (path, vertex) of a non-plain vertex or None)"""
    cases = {}
    for S in LENGTHS:
        for n in PATHS:
            for g in GROUPS:
                cases["S%d-P%d-G%d" % (S, n, g)] = ([S] * n, g, (), None)
    # wavefronts 1 and 4 wholly in motion, one path of wavefront 6; wavefronts 0, 2, 3, 5, 7 at rest
    cases["moving-starts"] = ([10] * 64, 2, tuple(range(8, 16)) + tuple(range(32, 40)) + (51,), None)
    cases["general-step"] = ([10] * 64, 2, (), (21, 4))   # path 21 (wavefront 2): vertex 4 with a second constraint
    for S in (5, 11, 2, 3):
        cases["negative-S%d" % S] = ([S] * 64, 2, (), None)
    cases["negative-12-paths"] = ([10] * 12, 3, (), None)
    cases["negative-ragged"] = (sorted([4, 6, 8, 10, 12, 10, 8, 6] * 3, reverse=True), 2, (), None)
    cases["headline"] = ([10] * 1024, 2, (), None)
    return cases


CASES = _cases()


# ---- the child process: every case, outcomes as JSON

class Guarded:
    """n elements inside an allocation of guard + n + guard, every word set to the pattern"""

    def __init__(self, shape, dtype, guard):
        import torch
        n = int(np.prod(shape))
        self.n, self.guard = n, guard
        self.bits = torch.int64 if dtype == torch.float64 else torch.int32
        self.pattern = PATTERN64 if dtype == torch.float64 else PATTERN32
        self.whole = torch.empty(guard + n + guard, dtype=dtype, device="cuda:0")
        self.view = self.whole[guard:guard + n].view(*shape)
        self.fill()

    def fill(self):
        self.whole.view(self.bits).fill_(self.pattern)

    def checked(self, what):
        """the inside as a host array, after: guards untouched, no pattern word left inside"""
        raw = self.whole.view(self.bits).cpu().numpy()
        g, n = self.guard, self.n
        assert np.all(raw[:g] == self.pattern), what + ": written in front of the buffer"
        assert np.all(raw[g + n:] == self.pattern), what + ": written behind the buffer"
        left = np.nonzero(raw[g:g + n] == self.pattern)[0]
        assert left.size == 0, "%s: %d words not written, the first at %d" % (what, left.size, left[0])
        return self.view.cpu().numpy().copy()


def _run_case(ctx, name):
    import torch
    from mrs_uav_trajectory_generation_amd import api, problem as pr
    lengths, group, moving, stop = CASES[name]
    batch = _batch(lengths, 7000 + 131 * len(lengths) + 17 * lengths[0], moving, stop)
    rule = lean_rule(lengths, batch.n_paths)
    plan = api.Plan(ctx, batch.seg_offsets)
    try:
        db = api.DeviceBatch(batch, "cuda:0")
        est = api.default_options(derivative_to_optimize=4, estimate_times=1)
        plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
                   limits=db.limits)
        torch.cuda.synchronize()
        # `group` batches of one plan: the same constraints at `group` sets of times, `group` sets of outputs
        times = [db.seg_times * (1.0 + 0.03 * j) for j in range(group)]
        g_coeff = max(lengths) * pr.N_DIM * pr.N_COEFF   # the longest path's coefficients
        outs = [(Guarded((batch.n_segments, pr.N_DIM, pr.N_COEFF), torch.float64, g_coeff),
                 Guarded((batch.n_paths,), torch.float64, 64), Guarded((batch.n_paths,), torch.int32, 64)) for _ in range(group)]
        for positions, flags in (("values", 0), ("waypoints", api.FLAG_POSITIONS_ARE_WAYPOINTS)):
            x = "true" if flags else "false"
            opt = api.default_options(derivative_to_optimize=4, flags=flags)
            calls = [plan.bind_solve(opt, db.fixed_mask, db.fixed_values, t, c.view, st.view, co.view, waypoints=db.waypoints)
                     for t, (c, co, st) in zip(times, outs)]
            got = {}
            for road in ROADS:
                os.environ["MRS_TG_DUO_LEAN"], os.environ["MRS_TG_DUO_UNIFORM"], os.environ["MRS_TG_DUO_STORE_THROUGH"] = road
                for o in outs:
                    for buf in o:
                        buf.fill()
                torch.cuda.synchronize()
                lean = rule and road == ROADS[0]
                for spell in ("1", "0"):   # (the same dispatch twice: the second overwrites the first with the same bytes)
                    os.environ["MRS_TG_TRACE_INSTANTIATIONS"] = spell
                    api.kernel_trace_reset()
                    api.RoundRobin(calls, grouped=True)(group)
                    want = "solve_duo_group_kernel<%s%s>" % (x, ", true" if lean and spell == "1" else "")
                    assert api.kernel_trace() == [want], (positions, road, spell, api.kernel_trace(), want)
                    if not lean:
                        break
                torch.cuda.synchronize()
                got[road] = [tuple(buf.checked("%s, road %s, batch %d, %s" % (positions, road, j, what))
                                   for buf, what in zip(o, ("coeffs", "cost", "status"))) for j, o in enumerate(outs)]
            want = got[ROADS[2]]
            # (a path of the general step may report a status of its own; every other path is solved)
            assert all(np.all(np.isfinite(c)) and np.all(np.isfinite(co)) for c, co, _ in want), positions
            for road in ROADS:
                for j, (a, b) in enumerate(zip(got[road], want)):
                    for what, u, v in zip(("coeffs", "cost", "status"), a, b):
                        assert np.array_equal(u, v), (positions, road, j, what, int(np.sum(u != v)))
            if group > 1:   # (the batches were solved at different times: an answer written to another batch's buffer would show)
                assert not np.array_equal(got[ROADS[0]][0][0], got[ROADS[0]][group - 1][0])
            assert np.all(got[ROADS[0]][group - 1][0][batch.n_segments - 1] != 0.0)
            if moving:   # the moving start went into the solution
                p = moving[0]
                assert np.allclose(got[ROADS[0]][0][0][batch.seg_offsets[p], :, 1], batch.fixed_values[batch.vertex_range(p)[0], 1],
                                   rtol=1e-9, atol=1e-12)
    finally:
        plan.close()


def _child(out_path):
    sys.path.insert(0, ROOT)
    from mrs_uav_trajectory_generation_amd import api
    ctx = api.Context(0)
    ctx.use_torch_stream()
    outcome = {}
    for name in CASES:
        try:
            _run_case(ctx, name)
            outcome[name] = "ok"
        except Exception:   # (an assertion's text, or the library's error: the parent shows it)
            outcome[name] = traceback.format_exc()
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(outcome, f)


# ---- the tests

@pytest.fixture(scope="module")
def outcomes(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("duo_lean") / "outcomes.json")
    env = dict(os.environ, MRS_TG_DUO="1", MRS_TG_QUAD_MIN_PATHS="0")
    for name in ("MRS_TG_DUO_LEAN", "MRS_TG_DUO_UNIFORM", "MRS_TG_DUO_STORE_THROUGH", "MRS_TG_TRACE_INSTANTIATIONS", "MRS_TG_QUAD_ENDS"):
        env.pop(name, None)
    subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, cwd=ROOT, timeout=600)
    with open(path) as f:
        return json.load(f)


def test_the_rule_of_the_cases():
    """(no GPU work: what the cases claim about the rule)"""
    assert all(lean_rule(CASES["S%d-P%d-G%d" % (S, n, g)][0], n) for S in LENGTHS for n in PATHS for g in GROUPS)
    assert lean_rule(CASES["moving-starts"][0], 64) and lean_rule(CASES["general-step"][0], 64)
    assert lean_rule(CASES["headline"][0], 1024)
    assert not any(lean_rule(CASES[k][0], len(CASES[k][0])) for k in CASES if k.startswith("negative"))
    assert len(set(CASES["negative-ragged"][0])) > 1 and len(CASES["negative-ragged"][0]) % 8 == 0


@pytest.mark.parametrize("name", list(CASES))
def test_lean_and_general_instantiation_same_bits_and_routed_by_the_rule(outcomes, name):
    assert outcomes[name] == "ok", outcomes[name]


if __name__ == "__main__":
    _child(sys.argv[1])
