"""What the tests of the heading along the direction of travel share (mrs_tg_plan_travel_heading, csrc/mrs_tg_heading.hpp,
DESIGN.md section 11f): a numpy restatement of getTrajectoryReference's override_heading_atan2
(src/mrs_trajectory_generation.cpp:1578-1603 of the reference), a torch restatement for the gradients, the named cases, and the
CPU harness tests/host/heading_harness.cpp.

The rows of a case are built directly, not by the optimiser: positions are cumulative sums of steps whose lengths come from
STEP_LENGTHS, every one at least 1e-3 m from the 0.05 m threshold, so that sqrt(dx dx + dy dy), std::hypot and both libms decide
alike and NO ROW IS LEFT OUT of any comparison."""
import math

import numpy as np

from tests import host_harness as hh

MIN_STEP = 0.05                                             # :1590
STEP_LENGTHS = (0.0, 0.01, 0.03, 0.049, 0.051, 0.2, 0.5)    # metres
SLOW = (0.0, 0.01, 0.03, 0.049)
MOVING = (0.051, 0.2, 0.5)

# The heading bound: the device's atan2 against the host's on bit-identical (dx, dy).  MEASURED_WORST is the worst absolute
# difference scripts/heading_cost.py --accuracy 1 found on an MI355X (profiles/heading_cost.txt): over the
# 4 075 520 rows of its larger batch in two draws and over 100 000 ratios dy/dx from 1e-300 to 1e300 in every quadrant (400 000
# operand pairs), against the C library's atan2 and against np.arctan2 alike: 4.44e-16 = 4 * 2^-53, one unit in the last place of
# a heading between 2 and 4 rad.  The factor 4 is there because the sweep does not visit every operand pair.  The bound, 16 *
# 2^-53, stays below the 64 * 2^-53 that DESIGN.md section 11d promises for the fallback sampler's headings.
MEASURED_WORST = 4.440892098500626e-16
HEADING_BOUND = 4.0 * MEASURED_WORST
GRAD_RTOL = 1e-13   # of the sum of the absolute terms of an entry: double rounding of fewer than 200 terms in another order


def travel_heading_numpy(samples, min_step=MIN_STEP, atan2=np.arctan2):
    """:1578-1603 for one path: samples [m][4] -> (heading [m], source [m] int32): one row after the other, np.arctan2, and the
    header's sqrt(dx dx + dy dy) for the decision; the last row keeps its heading and has source -1.  atan2=math.atan2 is the C
    library's function, the one tests/host/heading_harness.cpp calls: where numpy brings a vectorised arctan2 of its own (on
    CPUs with AVX-512) np.arctan2 is up to an ulp away from it, and only math.atan2 can be held to the harness's bits."""
    s = np.asarray(samples, dtype=np.float64).reshape(-1, 4)
    m = s.shape[0]
    heading = s[:, 3].copy()
    source = np.full(m, -1, dtype=np.int32)
    for i in range(m - 1):
        dx, dy = s[i + 1, 0] - s[i, 0], s[i + 1, 1] - s[i, 1]
        dist = np.sqrt(dx * dx + dy * dy)
        if dist < min_step and i > 0:
            heading[i], source[i] = heading[i - 1], source[i - 1]
        else:
            heading[i], source[i] = atan2(dy, dx), i
    return heading, source


def travel_heading_torch_grad(samples, upstream, source):
    """dL/dsamples [m][4] for L = sum(upstream * output rows) by torch's autograd: torch.atan2 on the steps gathered by the FIXED
    source index; the last row's heading passes through"""
    import torch
    s = torch.tensor(np.asarray(samples, dtype=np.float64).reshape(-1, 4), requires_grad=True)
    up = torch.tensor(np.asarray(upstream, dtype=np.float64).reshape(-1, 4))
    m = s.shape[0]
    if m == 0:
        return np.zeros((0, 4))
    if m == 1:
        return up.numpy().copy()
    idx = torch.as_tensor(np.asarray(source[:m - 1], dtype=np.int64))
    d = s[1:, :2] - s[:-1, :2]
    heading = torch.cat([torch.atan2(d[idx, 1], d[idx, 0]), s[m - 1:, 3]])
    out = torch.cat([s[:, :3], heading[:, None]], dim=1)
    (g,) = torch.autograd.grad((out * up).sum(), s)
    return g.numpy()


def grad_scale(samples, upstream, source):
    """the sum of the absolute terms of every entry of dL/dsamples [m][4]: what GRAD_RTOL is a fraction of"""
    s = np.asarray(samples, dtype=np.float64).reshape(-1, 4)
    up = np.abs(np.asarray(upstream, dtype=np.float64).reshape(-1, 4))
    m = s.shape[0]
    scale = up.copy()
    if m < 2:
        return scale
    scale[:m - 1, 3] = 0.0
    g_abs = np.zeros(m)
    np.add.at(g_abs, source[:m - 1], up[:m - 1, 3])
    with np.errstate(all="ignore"):
        d = s[1:, :2] - s[:-1, :2]
        r2 = d[:, 0] ** 2 + d[:, 1] ** 2
        t = np.where((r2 > 0)[:, None], np.abs(d[:, ::-1]) / r2[:, None] * g_abs[:m - 1, None], 0.0)   # (|dy|, |dx|) / r2 * G
    t[source[:m - 1] != np.arange(m - 1)] = 0.0
    scale[:m - 1, :2] += t
    scale[1:, :2] += t
    return scale


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _directions():
    """unit vectors over all four quadrants, exactly +-x and +-y among them"""
    out = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)]
    for deg in (17.0, 58.0, 112.0, 163.0, 197.0, 251.0, 289.0, 341.0):
        out.append((math.cos(math.radians(deg)), math.sin(math.radians(deg))))
    return np.array(out)


def rows_from_steps(lengths, seed):
    """[len(lengths) + 1][4] rows: positions are cumulative sums of steps of the given lengths in drawn directions, z and the
    sampled yaw drawn"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.float64)
    dirs = _directions()[rng.integers(0, 12, lengths.size)]
    rows = np.zeros((lengths.size + 1, 4))
    rows[0, :2] = rng.uniform(-3.0, 3.0, 2)
    rows[1:, :2] = rows[0, :2] + np.cumsum(dirs * lengths[:, None], axis=0)
    rows[:, 2] = rng.uniform(1.0, 4.0, lengths.size + 1)
    rows[:, 3] = rng.uniform(-3.0, 3.0, lengths.size + 1)
    return rows


def drawn_lengths(n_steps, seed, among=STEP_LENGTHS):
    return np.random.default_rng(1000 + seed).choice(np.asarray(among), size=max(n_steps, 0))


def path(rows, n_samples=None, status=1):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    return dict(rows=rows, n_samples=rows.shape[0] if n_samples is None else int(n_samples), status=int(status))


def drawn_path(n, seed, among=STEP_LENGTHS):
    if n == 0:
        return path(np.zeros((0, 4)))
    return path(rows_from_steps(drawn_lengths(n - 1, seed, among), seed))


def _run_path(n, slow_from, slow_to, seed):
    """n rows whose steps move, except those of the rows slow_from .. slow_to"""
    lengths = drawn_lengths(n - 1, seed, MOVING)
    lengths[slow_from:slow_to + 1] = drawn_lengths(slow_to + 1 - slow_from, seed + 1, SLOW)
    return path(rows_from_steps(lengths, seed))


def named_cases():
    """name -> list of paths (a batch)"""
    cases = {}
    for n in (0, 1, 2, 3, 64, 65, 128, 129, 130):
        cases["n%d" % n] = [drawn_path(n, n)]
    cases["slow_run_62_to_66"] = [_run_path(100, 62, 66, 201)]
    cases["slow_run_of_70_rows"] = [_run_path(200, 60, 129, 202)]            # rows 128, 129: the source is two chunks back
    cases["slow_from_row_1_to_the_end"] = [_run_path(150, 1, 148, 203)]
    zero_first = drawn_lengths(69, 204, SLOW)
    zero_first[0] = 0.0
    cases["zero_step_at_row_0_then_slow"] = [path(rows_from_steps(zero_first, 204))]
    cases["every_step_a_source"] = [drawn_path(130, 205, MOVING)]
    exact = np.array([[-0.3, 0.1, 1.0, 0.4], [0.0, 0.0, 1.0, 0.5], [0.05, 0.0, 1.0, 0.6], [0.05, 0.03, 1.0, 0.7],
                      [0.05, 0.23, 1.0, 0.8]])
    cases["step_of_exactly_the_threshold"] = [path(exact)]
    minus_pi = np.array([[0.0, 0.0, 1.0, 0.1], [-0.2, -0.0, 1.0, 0.2], [-0.4, 0.0, 1.0, 0.3], [-0.6, -0.0, 1.0, 0.4],
                         [-0.8, 0.0, 1.0, 0.5]])
    cases["negative_zero_dy_is_minus_pi"] = [path(minus_pi)]
    over = drawn_path(70, 206)
    over["n_samples"] = 71                                                   # capacity + 1: more rows than fit
    cases["count_of_capacity_plus_1"] = [over]
    cases["dead_path_between_live_ones"] = [drawn_path(40, 207), dict(drawn_path(70, 208), status=0), drawn_path(66, 209)]
    nan_path = _run_path(80, 41, 50, 210)
    nan_path["rows"][40, 0] = np.nan
    cases["not_a_number_in_a_middle_row"] = [nan_path]
    cases["five_paths"] = [drawn_path(3, 3), drawn_path(65, 65), _run_path(100, 62, 66, 201), drawn_path(130, 205, MOVING),
                           _run_path(200, 60, 129, 202)]
    return cases


def capacity_of(batch):
    """the capacity a batch is run at: room for every path's rows and three more -- except where a path reports more rows than it
    has (the overflow case), which is run at exactly its rows"""
    if any(p["n_samples"] > p["rows"].shape[0] for p in batch):
        return max(p["rows"].shape[0] for p in batch)
    return max(p["rows"].shape[0] for p in batch) + 3


def batch_arrays(batch, seed=0):
    """(samples [P][cap][4], n_samples [P] int32, status [P] int32, upstream [P][cap][4]) of a batch: the rows behind a path's
    own hold a sentinel that no result may depend on; the upstream is dyadic and covers every row"""
    cap = capacity_of(batch)
    P = len(batch)
    rng = np.random.default_rng(77 + seed)
    samples = 1.0e3 + rng.uniform(0.0, 1.0, (P, cap, 4))
    for q, p in enumerate(batch):
        samples[q, :p["rows"].shape[0]] = p["rows"]
    upstream = rng.integers(-128, 129, (P, cap, 4)) / 64.0
    n = np.array([p["n_samples"] for p in batch], dtype=np.int32)
    status = np.array([p["status"] for p in batch], dtype=np.int32)
    return samples, n, status, upstream


# ---- the CPU harness -----------------------------------------------------------------------------------------------------------

def build_harness(tmp_path, sanitize=False):
    return hh.build("heading_harness.cpp", tmp_path, sanitize=sanitize)


def run_harness(exe, batch, min_step=MIN_STEP, seed=0):
    """-> per path dict(m, source [m], heading [m], grad [m][4]) of the harness on batch_arrays(batch, seed)"""
    samples, n, status, upstream = batch_arrays(batch, seed)
    cap = samples.shape[1]
    lines = []
    for q in range(len(batch)):
        m = max(min(int(n[q]), cap), 0)
        lines.append("%d %d %d %s\n%s\n%s\n" % (n[q], cap, status[q], repr(float(min_step)), hh.fmt(samples[q, :m]),
                                                hh.fmt(upstream[q, :m])))
    out = []
    for line in hh.run(exe, lines, len(batch)):
        tok = line.split()
        m = int(tok[0])
        body = tok[1:1 + 2 * m]
        out.append(dict(m=m, source=np.array([int(t) for t in body[0::2]], dtype=np.int32),
                        heading=np.array([float(t) for t in body[1::2]], dtype=np.float64),
                        grad=np.array([float(t) for t in tok[1 + 2 * m:]], dtype=np.float64).reshape(m, 4)))
        assert len(tok) == 1 + 6 * m
    return out


same_bits, live_rows = hh.same_bits, hh.live_rows   # (a NaN equal to any NaN: two libms need not agree on a NaN's payload)


def grads_agree(got, want, scale):
    """|got - want| <= GRAD_RTOL * scale entry by entry; an entry that is not a number in one is not a number in the other"""
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = np.isnan(want) | (np.abs(got - want) <= GRAD_RTOL * scale)
    return bool(np.all(ok))
