"""What the tests of the mutual clearance within groups of paths share (mrs_tg_plan_mutual_clearance, csrc/mrs_tg_clearance.hpp,
DESIGN.md section 11i): the named cases, a numpy restatement of the forward (the same IEEE operations in the same order, so
it is held to the harness's bits), a torch restatement for the gradients on FIXED partners, and the CPU harness
tests/host/clearance_harness.cpp with its line grammar.

A case is a batch: dict(paths=[path, ...], groups=[size, ...], z_scale=...) with path = dict(rows [m][4], n_samples, status,
first_step).  The rows are built directly, not by the optimiser.  In the random cases the positions are drawn in a 20 m box and
tests/test_clearance_host.py asserts that on EVERY row the nearest and the second-nearest neighbour are more than 1e-9 apart
(relative), so no row has to be left out of any comparison; the tie cases are exact by construction."""
import numpy as np

from tests import host_harness as hh

EPS = 2.0 ** -52
GRAD_RTOL = 1e-13   # of the sum of the absolute terms of an entry (the family's bound: tests/heading_util.py)
BOX = 20.0
GAP = 1e-9          # the least relative gap between the nearest and the second-nearest neighbour in the random cases
ROW_COUNTS = (0, 1, 2, 63, 64, 65, 128, 129, 130)
GROUP_SIZES = (0, 1, 2, 3, 64, 65, 66)
STEP_OFFSETS = (1, 63, 64, 65)


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def path(rows, n_samples=None, status=1, first_step=0):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    return dict(rows=rows, n_samples=rows.shape[0] if n_samples is None else int(n_samples), status=int(status),
                first_step=int(first_step))


def drawn_rows(m, rng):
    """[m][4] rows in the box: a random walk of 0.4 m steps from a drawn start, so that neighbours change along a path"""
    rows = np.zeros((m, 4))
    if m:
        start = rng.uniform(0.0, BOX, 3)
        steps = rng.normal(0.0, 0.4, (m, 3))
        steps[0] = 0.0
        rows[:, :3] = np.clip(start + np.cumsum(steps, axis=0), 0.0, BOX)
        rows[:, 3] = rng.uniform(-3.0, 3.0, m)
    return rows


def case(paths, groups=None, z_scale=1.0):
    return dict(paths=list(paths), groups=[len(paths)] if groups is None else [int(g) for g in groups], z_scale=float(z_scale))


def drawn_case(rows_per_path, groups, seed, first_steps=None, z_scale=1.0):
    rng = np.random.default_rng(seed)
    paths = [path(drawn_rows(m, rng)) for m in rows_per_path]
    for q, f in enumerate(first_steps or ()):
        paths[q]["first_step"] = int(f)
    return case(paths, groups, z_scale)


def _exact_rows(points):
    """rows from exactly representable (x, y, z) triples, heading 0"""
    return np.array([[x, y, z, 0.0] for x, y, z in points])


def named_cases():
    """name -> case"""
    cases = {}
    for m in ROW_COUNTS:
        cases["rows_%d" % m] = drawn_case([m, m, m], None, 100 + m)
    over = drawn_case([70, 70], None, 171)
    for p in over["paths"]:
        p["n_samples"] = 71                                                   # capacity + 1: more rows than fit
    cases["count_of_capacity_plus_1"] = over
    for g in GROUP_SIZES:
        if g == 0:
            cases["group_of_0"] = drawn_case([9, 9], [0, 2], 200)             # (a plan needs a path: an empty group in front of one of 2)
        else:
            cases["group_of_%d" % g] = drawn_case([5] * g, [g], 200 + g)
    cases["groups_3_0_1_5"] = drawn_case([40, 70, 66, 30, 65, 64, 20, 67, 50], [3, 0, 1, 5], 300)
    for k in STEP_OFFSETS:
        cases["offset_%d" % k] = drawn_case([130, 130], None, 400 + k, first_steps=(0, k))
    cases["negative_offset"] = drawn_case([100, 100, 80], None, 470, first_steps=(-70, -3, 0))
    cases["extreme_first_steps"] = drawn_case([66, 66, 66], None, 471, first_steps=(2 ** 30, 2 ** 30 - 5, -2 ** 30))
    cases["never_overlap"] = drawn_case([100, 100], None, 472, first_steps=(0, 500))
    # an exact tie: the subject on the z axis, one neighbour 2^k in front and one 2^k behind along x, in every row
    z = [0.25 * r for r in range(6)]
    subject = _exact_rows([(0.0, 0.0, h) for h in z])
    plus = _exact_rows([(2.0 ** (r - 2), 0.0, h) for r, h in enumerate(z)])
    minus = _exact_rows([(-2.0 ** (r - 2), 0.0, h) for r, h in enumerate(z)])
    cases["exact_tie_lower_index_wins"] = case([path(subject), path(plus), path(minus)])
    cases["tie_between_a_path_in_front_and_one_behind"] = case([path(minus), path(subject), path(plus)])
    # coincident rows: paths 0 and 1 share their rows 2 .. 4; path 2 is metres away
    rng = np.random.default_rng(480)
    a = drawn_rows(8, rng)
    b = a + np.array([0.5, -0.25, 0.125, 0.0])
    b[2:5] = a[2:5]
    cases["coincident_rows"] = case([path(a), path(b), path(a + np.array([3.0, 3.0, 1.0, 0.0]))])
    # a NaN row in a neighbour: path 1 runs 0.5 m beside path 0, path 2 1.5 m beside it
    a = drawn_rows(12, np.random.default_rng(481))
    near, far = a + np.array([0.5, 0.0, 0.0, 0.0]), a + np.array([0.0, 1.5, 0.0, 0.0])
    near[5, 1] = np.nan
    cases["nan_row_in_a_neighbour"] = case([path(a), path(near), path(far)])
    sub = a.copy()
    sub[3, 2] = np.nan
    cases["nan_row_in_the_subject"] = case([path(sub), path(a + np.array([0.5, 0.0, 0.0, 0.0])), path(far)])
    dead = dict(path(np.full((12, 4), np.nan)), status=0)
    cases["dead_path_of_nan_rows_between_live_ones"] = case([path(a), dead, path(far)])
    # z_scale: B is 1 m beside the subject, A 1.5 m above it: 1.0 chooses B, 0.5 sees A at 0.75 m
    sub = _exact_rows([(0.0, 0.0, 1.0 + 0.125 * r) for r in range(5)])
    above = sub + np.array([0.0, 0.0, 1.5, 0.0])
    beside = sub + np.array([1.0, 0.0, 0.0, 0.0])
    cases["z_scale_1"] = case([path(sub), path(above), path(beside)], z_scale=1.0)
    cases["z_scale_half"] = case([path(sub), path(above), path(beside)], z_scale=0.5)
    # one row the partner of several paths at one step: path 2 in the middle, four paths around it, far from each other
    rng = np.random.default_rng(482)
    mid = drawn_rows(70, rng)
    around = [mid + np.array(o) + np.concatenate([rng.normal(0.0, 0.05, (70, 3)), np.zeros((70, 1))], axis=1)
              for o in ([1.1, 0.0, 0.0, 0.0], [-1.3, 0.0, 0.0, 0.0], [0.0, 1.2, 0.0, 0.0], [0.0, -1.4, 0.0, 0.0])]
    cases["a_row_that_is_partner_to_several_paths"] = case([path(around[0]), path(around[1]), path(mid), path(around[2]),
                                                            path(around[3])])
    # random: ragged rows, ragged starts, several groups
    rng = np.random.default_rng(490)
    cases["random_groups"] = drawn_case(rng.integers(1, 150, 16).tolist(), [5, 7, 4], 491,
                                        first_steps=rng.integers(-20, 21, 16).tolist())
    cases["random_one_group_z_scale_0_3"] = drawn_case(rng.integers(60, 140, 12).tolist(), None, 492,
                                                       first_steps=rng.integers(-10, 11, 12).tolist(), z_scale=0.3)
    return cases


RANDOM_CASES = ("random_groups", "random_one_group_z_scale_0_3")


def group_offsets_of(c):
    return np.concatenate([[0], np.cumsum(c["groups"])]).astype(np.int32)


def capacity_of(c):
    """the capacity a case is run at: room for every path's rows and three more -- except where a path reports more rows than
    it has (the overflow case), which is run at exactly its rows"""
    most = max([p["rows"].shape[0] for p in c["paths"]] + [1])
    return most if any(p["n_samples"] > p["rows"].shape[0] for p in c["paths"]) else most + 3


def batch_arrays(c, seed=0, capacity=None):
    """dict(samples [P][cap][4], n [P], status [P], first_step [P], group_offsets [G + 1], upstream [P][cap], z_scale) of a
    case: the rows behind a path's own hold a sentinel that no result may depend on; the upstream is dyadic and covers every
    row, the ones without a neighbour included"""
    cap = capacity_of(c) if capacity is None else int(capacity)
    P = len(c["paths"])
    rng = np.random.default_rng(77 + seed)
    samples = 1.0e3 + rng.uniform(0.0, 1.0, (P, cap, 4))
    for q, p in enumerate(c["paths"]):
        samples[q, :p["rows"].shape[0]] = p["rows"]
    upstream = rng.integers(-128, 129, (P, cap)) / 64.0
    return dict(samples=samples, n=np.array([p["n_samples"] for p in c["paths"]], dtype=np.int32),
                status=np.array([p["status"] for p in c["paths"]], dtype=np.int32),
                first_step=np.array([p["first_step"] for p in c["paths"]], dtype=np.int32),
                group_offsets=group_offsets_of(c), upstream=upstream, z_scale=c["z_scale"])


def combined_case(cases, z_scale):
    """all cases in one batch, a dead path of NaN rows between any two of them (a group of its own)"""
    paths, groups = [], []
    for i, c in enumerate(cases.values()):
        if i:
            paths.append(dict(path(np.full((7, 4), np.nan)), status=0))
            groups.append(1)
        paths += [dict(p) for p in c["paths"]]
        groups += c["groups"]
    return case(paths, groups, z_scale)


def rotated_case(c):
    """the same case with its first group moved behind the last: (case, for every path of the new batch its index in the old)"""
    off = group_offsets_of(c)
    k = int(off[1])
    order = list(range(k, len(c["paths"]))) + list(range(k))
    return case([c["paths"][q] for q in order], c["groups"][1:] + c["groups"][:1], c["z_scale"]), np.array(order)


# ---- the restatements ------------------------------------------------------------------------------------------------------------

def mutual_clearance_numpy(arr, second=False):
    """the forward on batch_arrays' dict with WELL-FORMED offsets -> dict(clearance [P][cap], partner [P][cap] int32,
    min_clearance [P], argmin [P][2] int32): per row the neighbours one after the other in increasing path index, a strict <
    from +inf; np.sqrt is correctly rounded like the C library's.  second=True adds `second` [P][cap]: the distance of the
    second-nearest neighbour (+inf without one), for the gap the random cases assert."""
    s, n, st, fs, off, kappa = arr["samples"], arr["n"], arr["status"], arr["first_step"], arr["group_offsets"], arr["z_scale"]
    P, cap = s.shape[:2]
    live = [live_rows(n[q], st[q], cap) for q in range(P)]
    clearance = np.full((P, cap), np.inf)
    partner = np.full((P, cap), -1, dtype=np.int32)
    runner_up = np.full((P, cap), np.inf)
    for g in range(len(off) - 1):
        for p in range(off[g], off[g + 1]):
            steps = int(fs[p]) + np.arange(live[p], dtype=np.int64)
            for j in range(off[g], off[g + 1]):
                if j == p:
                    continue
                rj = steps - int(fs[j])
                ok = (rj >= 0) & (rj < live[j])
                r = np.flatnonzero(ok)
                if not r.size:
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    dx = s[p, r, 0] - s[j, rj[r], 0]
                    dy = s[p, r, 1] - s[j, rj[r], 1]
                    dz = kappa * (s[p, r, 2] - s[j, rj[r], 2])
                    c = np.sqrt((dx * dx + dy * dy) + dz * dz)
                    wins = c < clearance[p, r]
                    if second:
                        loses = ~wins & (c < runner_up[p, r])
                        runner_up[p, r[wins]] = clearance[p, r[wins]]
                        runner_up[p, r[loses]] = c[loses]
                clearance[p, r[wins]] = c[wins]
                partner[p, r[wins]] = j
    min_clearance = np.full(P, np.inf)
    argmin = np.full((P, 2), -1, dtype=np.int32)
    for p in range(P):
        for r in range(live[p]):          # the first row strictly below every row in front of it
            if clearance[p, r] < min_clearance[p]:
                min_clearance[p], argmin[p] = clearance[p, r], (r, partner[p, r])
    out = dict(clearance=clearance, partner=partner, min_clearance=min_clearance, argmin=argmin)
    if second:
        out["second"] = runner_up
    return out


def _pairs(arr, partner):
    """the (p, r, q, rq) of every row whose partner entry is followed: in the row's group, not the row's path, a live row at
    the step"""
    n, st, fs, off = arr["n"], arr["status"], arr["first_step"], arr["group_offsets"]
    P, cap = partner.shape
    live = [live_rows(n[q], st[q], cap) for q in range(P)]
    out = []
    for g in range(len(off) - 1):
        for p in range(off[g], off[g + 1]):
            for r in range(live[p]):
                q = int(partner[p, r])
                if q < off[g] or q >= off[g + 1] or q == p:
                    continue
                rq = int(fs[p]) + r - int(fs[q])
                if 0 <= rq < live[q]:
                    out.append((p, r, q, rq))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def torch_clearance(torch, samples, pairs, z_scale):
    """c of the given (p, r, q, rq) pairs as a float64 torch expression of samples [P][cap][4] (differentiable)"""
    d = samples[pairs[:, 0], pairs[:, 1], :3] - samples[pairs[:, 2], pairs[:, 3], :3]
    return torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + (z_scale * d[:, 2]) ** 2)


def mutual_clearance_torch_grad(arr, partner):
    """(dL/dsamples [P][cap][4], the sum of the absolute terms of every entry [P][cap][4]) for L = sum(upstream * clearance) by
    torch's float64 autograd on the FIXED partners; coincident rows are left out (they contribute exactly 0 by contract)"""
    import torch
    s_np, up = arr["samples"], arr["upstream"]
    grad, scale = np.zeros_like(s_np), np.zeros_like(s_np)
    pairs = _pairs(arr, partner)
    if pairs.shape[0]:
        with np.errstate(invalid="ignore"):
            d = s_np[pairs[:, 0], pairs[:, 1], :3] - s_np[pairs[:, 2], pairs[:, 3], :3]
            d[:, 2] *= arr["z_scale"]
            c = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + d[:, 2] ** 2)
        pairs = pairs[c != 0.0]
    if pairs.shape[0]:
        idx = torch.as_tensor(pairs)
        s = torch.tensor(np.where(np.isnan(s_np), 0.0, s_np), requires_grad=True)   # (no pair touches a NaN row in the cases)
        g = torch.as_tensor(up[pairs[:, 0], pairs[:, 1]])
        (gt,) = torch.autograd.grad((torch_clearance(torch, s, idx, arr["z_scale"]) * g).sum(), s)
        grad = gt.numpy()
        d = s_np[pairs[:, 0], pairs[:, 1], :3] - s_np[pairs[:, 2], pairs[:, 3], :3]
        w = np.array([1.0, 1.0, arr["z_scale"] ** 2])
        c = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + (arr["z_scale"] * d[:, 2]) ** 2)
        t = np.abs(g.numpy())[:, None] * np.abs(d) * w / c[:, None]
        for k in range(3):
            np.add.at(scale[:, :, k], (pairs[:, 0], pairs[:, 1]), t[:, k])
            np.add.at(scale[:, :, k], (pairs[:, 2], pairs[:, 3]), t[:, k])
    return grad, scale


def term_bound(arr, partner):
    """16 eps |g| per contributing term, summed over the terms of every row [P][cap]: the own term and the term of every row
    that names this one"""
    up = np.abs(arr["upstream"])
    out = np.zeros(partner.shape)
    pairs = _pairs(arr, partner)
    if pairs.shape[0]:
        s = arr["samples"]
        d = s[pairs[:, 0], pairs[:, 1], :3] - s[pairs[:, 2], pairs[:, 3], :3]
        pairs = pairs[np.any(d != 0.0, axis=1)]
        t = 16.0 * EPS * up[pairs[:, 0], pairs[:, 1]]
        np.add.at(out, (pairs[:, 0], pairs[:, 1]), t)
        np.add.at(out, (pairs[:, 2], pairs[:, 3]), t)
    return out


# ---- the chain test's swarm ------------------------------------------------------------------------------------------------------

CHAIN_DT, CHAIN_CAPACITY, CHAIN_RADIUS = 0.2, 72, 2.0


def chain_batch():
    """The swarm of the chain test: four 4-segment paths that fly abreast along x, 1.0 to 1.3 m apart in y and a few decimetres
    in z, each with its own wiggle -- within the hinge radius of a neighbour on most rows, never closer than decimetres, and
    with no two neighbours at the same distance"""
    import math
    from mrs_uav_trajectory_generation_amd import problem as pr
    lanes, heights = (0.0, 1.0, 2.3, 3.3), (3.0, 3.4, 2.9, 3.5)
    parts = []
    for q in range(4):
        wp = [[-6.0 + 3.0 * k, lanes[q] + 0.3 * math.sin(1.3 * k + q), heights[q] + 0.1 * math.cos(0.7 * k + 2 * q), 0.0]
              for k in range(5)]
        parts.append(pr.build_vertices(np.array(wp), pr.SNAP))
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (len(parts), 1)))


# ---- the CPU harness -----------------------------------------------------------------------------------------------------------

def build_harness(tmp_path, sanitize=False):
    return hh.build("clearance_harness.cpp", tmp_path, sanitize=sanitize)


def run_harness(exe, arr, partner=None):
    """the harness on batch_arrays' dict (any offsets, well-formed or not; partner: the array the backward pass is driven by
    instead of the forward's) -> dict(clearance [P][cap], partner [P][cap], min_clearance [P], argmin [P][2], grad [P][cap][4])"""
    s = arr["samples"]
    P, cap = s.shape[:2]
    off = np.asarray(arr["group_offsets"])
    lines = ["%d %d %d %s %d\n" % (P, cap, off.size - 1, repr(float(arr["z_scale"])), 0 if partner is None else 1),
             _ints(off) + "\n", _ints(arr["n"]) + "\n", _ints(arr["status"]) + "\n", _ints(arr["first_step"]) + "\n",
             hh.fmt(s) + "\n", hh.fmt(arr["upstream"]) + "\n"]
    if partner is not None:
        lines.append(_ints(partner) + "\n")
    out = dict(clearance=np.zeros((P, cap)), partner=np.zeros((P, cap), dtype=np.int32), min_clearance=np.zeros(P),
               argmin=np.zeros((P, 2), dtype=np.int32), grad=np.zeros((P, cap, 4)))
    for q, line in enumerate(hh.run(exe, lines, P)):
        tok = line.split()
        assert len(tok) == 6 * cap + 3, (len(tok), cap)
        out["clearance"][q] = [float(t) for t in tok[:cap]]
        out["partner"][q] = [int(t) for t in tok[cap:2 * cap]]
        out["min_clearance"][q] = float(tok[2 * cap])
        out["argmin"][q] = [int(tok[2 * cap + 1]), int(tok[2 * cap + 2])]
        out["grad"][q] = np.array([float(t) for t in tok[2 * cap + 3:]]).reshape(cap, 4)
    return out


same_bits, live_rows, _ints = hh.same_bits, hh.live_rows, hh.ints


def grads_agree(got, want, scale):
    return hh.grads_agree(got, want, scale, GRAD_RTOL)
