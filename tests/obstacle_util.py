"""What the tests of the clearance from static obstacles share (mrs_tg_plan_obstacle_clearance, csrc/mrs_tg_obstacle.hpp,
DESIGN.md section 11j): the named cases, a numpy restatement of the forward (the same IEEE operations in the same order, so
it is held to the harness's bits), a torch restatement for the gradients on FIXED nearest obstacles, and the CPU harness
tests/host/obstacle_harness.cpp with its line grammar.

A case is a batch: dict(paths=[path, ...], obstacles [M][4], sets=[size, ...], path_set=[set, ...] or None, z_scale=...) with
path = dict(rows [m][4], n_samples, status).  The rows are built directly, not by the optimiser.  In the random cases the rows
and the obstacles are drawn in a 20 m box and tests/test_obstacle_host.py asserts that on EVERY row the nearest and the
second-nearest obstacle are more than 1e-9 apart (relative), so no row has to be left out of any comparison; the tie cases are
exact by construction, the one-ulp cases one ulp apart by construction, and the restatement asserts it."""
import numpy as np

from tests import host_harness as hh

EPS = 2.0 ** -52
GRAD_RTOL = 1e-13   # of the sum of the absolute terms of an entry (the family's bound: tests/clearance_util.py)
BOX = 20.0
GAP = 1e-9          # the least relative gap between the nearest and the second-nearest obstacle in the random cases
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)                      # the chunk seams (64) and the workgroup seams (256)
SET_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257)         # every unroll and tile seam of a power of two up to 256


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def path(rows, n_samples=None, status=1):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    return dict(rows=rows, n_samples=rows.shape[0] if n_samples is None else int(n_samples), status=int(status))


def drawn_rows(m, rng):
    """[m][4] rows: a random walk of 0.4 m steps from a start drawn in the box, so that the nearest obstacle changes along a path"""
    rows = np.zeros((m, 4))
    if m:
        start = rng.uniform(0.0, BOX, 3)
        steps = rng.normal(0.0, 0.4, (m, 3))
        steps[0] = 0.0
        rows[:, :3] = start + np.cumsum(steps, axis=0)
        rows[:, 3] = rng.uniform(-3.0, 3.0, m)
    return rows


def drawn_obstacles(m, rng, spheres=True):
    """[m][4] obstacles in the box: every other one a point (radius 0), the rest spheres of 0.1 .. 1.5 m"""
    ob = np.zeros((m, 4))
    ob[:, :3] = rng.uniform(0.0, BOX, (m, 3))
    if spheres:
        ob[1::2, 3] = rng.uniform(0.1, 1.5, ob[1::2].shape[0])
    return ob


def case(paths, obstacles, sets=None, path_set=None, z_scale=1.0):
    obstacles = np.asarray(obstacles, dtype=np.float64).reshape(-1, 4)
    return dict(paths=list(paths), obstacles=obstacles, sets=[obstacles.shape[0]] if sets is None else [int(g) for g in sets],
                path_set=None if path_set is None else [int(q) for q in path_set], z_scale=float(z_scale))


def drawn_case(rows_per_path, sets, seed, path_set=None, z_scale=1.0, spheres=True):
    rng = np.random.default_rng(seed)
    return case([path(drawn_rows(m, rng)) for m in rows_per_path], drawn_obstacles(int(sum(sets)), rng, spheres), sets, path_set,
                z_scale)


def _rows_at(points):
    """rows from exactly representable (x, y, z) triples, heading 0"""
    return np.array([[x, y, z, 0.0] for x, y, z in points])


def _ulp_pair(d):
    """(d, the next double above d)"""
    return float(d), float(np.nextafter(d, np.inf))


def named_cases():
    """name -> case"""
    cases = {}
    for m in ROW_COUNTS:
        cases["rows_%d" % m] = drawn_case([m, m], [9], 100 + m)
    over = drawn_case([70, 70], [6], 171)
    for p in over["paths"]:
        p["n_samples"] = 71                                                   # capacity + 1: more rows than fit
    cases["count_of_capacity_plus_1"] = over
    live = drawn_case([12, 12, 12], [6], 172)
    live["paths"][1] = dict(path(np.full((12, 4), np.nan)), status=0)
    cases["dead_path_of_nan_rows_between_live_ones"] = live
    for g in SET_SIZES:
        # rows scattered over the box, so that the nearest obstacle is all over the set; and row 0 of the second path a
        # centimetre beside the LAST obstacle, so that the last one wins somewhere
        c = drawn_case([66, 5], [g], 200 + g)
        rng = np.random.default_rng(250 + g)
        c["paths"][0]["rows"][:, :3] = rng.uniform(0.0, BOX, (66, 3))
        if g:
            c["paths"][1]["rows"][0, :3] = c["obstacles"][g - 1, :3] + [0.01, 0.0, 0.0]
        cases["set_of_%d" % g] = c
    # sets [3, 0, 1, 5]: two paths share set 0, one sees the empty set, one names no set (-1), one a set behind the last
    cases["sets_3_0_1_5"] = drawn_case([40, 70, 66, 30, 65, 20, 9], [3, 0, 1, 5], 300, path_set=[0, 0, 1, 2, 3, -1, 4])
    cases["sets_3_0_1_5_path_set_null"] = drawn_case([40, 70, 9], [3, 0, 1, 5], 301, path_set=None)
    # exact ties.  The rows climb the z axis; two points sit mirrored in x, so their c is the same double on every row, and on
    # row 0 (z = 0) it is the power of two itself
    climb = _rows_at([(0.0, 0.0, 0.25 * r) for r in range(6)])
    far = [0.0, 64.0, 0.0, 0.0]
    cases["exact_tie_lower_index_wins"] = case([path(climb)], [[4.0, 0.0, 0.0, 0.0], [-4.0, 0.0, 0.0, 0.0], far])
    cases["exact_tie_behind_a_farther_one"] = case([path(climb)], [far, [-0.5, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0]])
    rng = np.random.default_rng(310)
    filler = np.zeros((70, 4))
    filler[:, :3] = rng.uniform(40.0, 60.0, (70, 3))
    filler[3], filler[67] = [-2.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0]
    cases["exact_tie_64_obstacles_apart"] = case([path(climb)], filler)
    flat = _rows_at([(0.0, 0.25 * r, 0.0) for r in range(6)])                 # (row 0 at the origin)
    point, sphere = [2.0, 0.0, 0.0, 0.0], [-4.0, 0.0, 0.0, 2.0]               # on row 0: 2 - 0 == 4 - 2
    cases["tie_of_a_point_and_a_sphere_point_first"] = case([path(flat[:1])], [point, sphere, far])
    cases["tie_of_a_point_and_a_sphere_sphere_first"] = case([path(flat[:1])], [sphere, point, far])
    # one-ulp near-ties: the row at the origin, two points on the x axis whose distances are neighbouring doubles
    origin = _rows_at([(0.0, 0.0, 0.0)])
    for tag, d in (("small", 0.7500000000000003), ("large", 1.0e6 + 0.3)):
        lo, hi = _ulp_pair(d)
        cases["one_ulp_%s_nearer_first" % tag] = case([path(origin)], [[lo, 0.0, 0.0, 0.0], [-hi, 0.0, 0.0, 0.0], [0.0, 4.0e6, 0.0, 0.0]])
        cases["one_ulp_%s_nearer_second" % tag] = case([path(origin)], [[-hi, 0.0, 0.0, 0.0], [lo, 0.0, 0.0, 0.0], [0.0, 4.0e6, 0.0, 0.0]])
    # inside a sphere: the rows pass through a sphere of 3 m; a point 8 m away is never nearer
    through = _rows_at([(-4.0 + 0.5 * r, 0.25, 0.0) for r in range(17)])
    cases["inside_a_sphere"] = case([path(through)], [[0.0, 0.0, 0.0, 3.0], [0.0, 8.0, 0.0, 0.0]])
    # a row on a centre: row 2 of the path IS the centre of obstacle 1
    on = _rows_at([(1.0 + 0.5 * r, 2.0, 3.0) for r in range(5)])
    cases["row_on_a_centre"] = case([path(on)], [[9.0, 9.0, 9.0, 0.0], [2.0, 2.0, 3.0, 0.5], [-9.0, 0.0, 0.0, 0.25]])
    cases["radius_0_cloud"] = drawn_case([70, 33], [40], 320, spheres=False)
    # a NaN coordinate in the obstacle that would be nearest: the next one wins
    a = _rows_at([(0.0, 0.0, 1.0 + 0.125 * r) for r in range(8)])
    cases["nan_coordinate_in_an_obstacle"] = case([path(a)], [[0.25, np.nan, 1.0, 0.0], [0.0, 2.0, 1.0, 0.0], [0.0, 3.0, 1.0, 0.0]])
    sub = drawn_case([12, 12], [7], 330)
    sub["paths"][0]["rows"][3, 2] = np.nan
    sub["paths"][1]["rows"][0, 0] = np.nan
    cases["nan_in_a_row"] = sub
    # an infinite radius is ordinary data: -inf never wins (c = +inf), +inf always does (c = -inf)
    inf = drawn_case([9, 9], [2, 2], 340, path_set=[0, 1])
    inf["obstacles"][0, 3] = -np.inf
    inf["obstacles"][3, 3] = np.inf
    cases["infinite_radius"] = inf
    # z_scale: B is 1 m beside the rows, A 1.5 m above them: 1.0 chooses B, 0.5 sees A at 0.75 m
    sub = _rows_at([(0.125 * r, 0.0, 1.0) for r in range(5)])
    above, beside = sub[:, :3] + [0.0, 0.0, 1.5], sub[:, :3] + [0.0, 1.0, 0.0]
    ab = np.zeros((2, 4))
    ab[0, :3], ab[1, :3] = above[0], beside[0]
    cases["z_scale_1"] = case([path(sub[:1])], ab, z_scale=1.0)
    cases["z_scale_half"] = case([path(sub[:1])], ab, z_scale=0.5)
    # random: ragged rows, several sets, points and spheres
    rng = np.random.default_rng(390)
    cases["random_sets"] = drawn_case(rng.integers(1, 150, 12).tolist(), [40, 0, 97, 13], 391,
                                      path_set=rng.integers(0, 4, 12).tolist())
    cases["random_one_set_z_scale_0_3"] = drawn_case(rng.integers(60, 140, 6).tolist(), [300], 392, z_scale=0.3)
    return cases


RANDOM_CASES = ("random_sets", "random_one_set_z_scale_0_3")
ONE_ULP_CASES = tuple("one_ulp_%s_nearer_%s" % (a, b) for a in ("small", "large") for b in ("first", "second"))


def set_offsets_of(c):
    return np.concatenate([[0], np.cumsum(c["sets"])]).astype(np.int32)


def capacity_of(c):
    """the capacity a case is run at: room for every path's rows and three more -- except where a path reports more rows than
    it has (the overflow case), which is run at exactly its rows"""
    most = max([p["rows"].shape[0] for p in c["paths"]] + [1])
    return most if any(p["n_samples"] > p["rows"].shape[0] for p in c["paths"]) else most + 3


def batch_arrays(c, seed=0, capacity=None):
    """dict(samples [P][cap][4], n [P], status [P], obstacles [M][4], set_offsets [S + 1], path_set [P] or None, upstream
    [P][cap], z_scale) of a case: the rows behind a path's own hold a sentinel that no result may depend on; the upstream is
    dyadic and covers every row, the ones without an obstacle included"""
    cap = capacity_of(c) if capacity is None else int(capacity)
    P = len(c["paths"])
    rng = np.random.default_rng(77 + seed)
    samples = 1.0e3 + rng.uniform(0.0, 1.0, (P, cap, 4))
    for q, p in enumerate(c["paths"]):
        samples[q, :p["rows"].shape[0]] = p["rows"]
    upstream = rng.integers(-128, 129, (P, cap)) / 64.0
    return dict(samples=samples, n=np.array([p["n_samples"] for p in c["paths"]], dtype=np.int32),
                status=np.array([p["status"] for p in c["paths"]], dtype=np.int32),
                obstacles=np.ascontiguousarray(c["obstacles"], dtype=np.float64).reshape(-1, 4), set_offsets=set_offsets_of(c),
                path_set=None if c["path_set"] is None else np.array(c["path_set"], dtype=np.int32), upstream=upstream,
                z_scale=c["z_scale"])


def explicit_path_set(c):
    """the path_set of a case as a list: NULL written out as set 0 (no set at all where the case has none)"""
    return list(c["path_set"]) if c["path_set"] is not None else [0 if c["sets"] else -1] * len(c["paths"])


def combined_case(cases, z_scale):
    """all cases in one batch -- their obstacles one map, their sets one after the other -- with a dead path of NaN rows
    between any two of them"""
    paths, obstacles, sets, path_set = [], [np.zeros((0, 4))], [], []
    for i, c in enumerate(cases.values()):
        if i:
            paths.append(dict(path(np.full((7, 4), np.nan)), status=0))
            path_set.append(0)
        S = len(c["sets"])
        paths += [dict(p) for p in c["paths"]]
        path_set += [q + len(sets) if 0 <= q < S else -1 for q in explicit_path_set(c)]
        sets += c["sets"]
        obstacles.append(c["obstacles"])
    return case(paths, np.concatenate(obstacles), sets, path_set, z_scale)


def rotated_case(c):
    """the same case with its first path moved behind the last and its first set moved behind the last: (case, for every path
    of the new batch its index in the old, for every obstacle of the old map its index in the new)"""
    off = set_offsets_of(c)
    S, M, P = len(c["sets"]), int(off[-1]), len(c["paths"])
    k = int(off[1])
    ob_order = list(range(k, M)) + list(range(k))                    # new -> old
    new_of_old = np.argsort(np.array(ob_order, dtype=np.int64)) if M else np.zeros(0, dtype=np.int64)
    order = list(range(1, P)) + [0]
    ps = explicit_path_set(c)
    moved = [(q - 1) % S if 0 <= q < S else q for q in ps]
    rot = case([c["paths"][q] for q in order], c["obstacles"][ob_order], c["sets"][1:] + c["sets"][:1],
               [moved[q] for q in order], c["z_scale"])
    return rot, np.array(order), new_of_old


def path_bounds(arr, p):
    """(begin, end) of the obstacles path p sees, WELL-FORMED offsets assumed: empty where path_set names no set"""
    off = arr["set_offsets"]
    q = 0 if arr["path_set"] is None else int(arr["path_set"][p])
    return (int(off[q]), int(off[q + 1])) if 0 <= q < len(off) - 1 else (0, 0)


# ---- the restatements ------------------------------------------------------------------------------------------------------------

def obstacle_clearance_numpy(arr, second=False):
    """the forward on batch_arrays' dict with WELL-FORMED offsets -> dict(clearance [P][cap], nearest [P][cap] int32,
    min_clearance [P], argmin [P][2] int32): per row the obstacles of the path's set one after the other in increasing index, a
    strict < from +inf; np.sqrt is correctly rounded like the C library's.  second=True adds `second` [P][cap]: the c of the
    second-nearest obstacle (+inf without one), for the gaps the random and the one-ulp cases assert."""
    s, n, st, ob, kappa = arr["samples"], arr["n"], arr["status"], arr["obstacles"], arr["z_scale"]
    P, cap = s.shape[:2]
    live = [live_rows(n[q], st[q], cap) for q in range(P)]
    clearance = np.full((P, cap), np.inf)
    nearest = np.full((P, cap), -1, dtype=np.int32)
    runner_up = np.full((P, cap), np.inf)
    for p in range(P):
        begin, end = path_bounds(arr, p)
        m = live[p]
        x, y, z = s[p, :m, 0], s[p, :m, 1], s[p, :m, 2]
        for k in range(begin, end):
            with np.errstate(invalid="ignore", over="ignore"):
                dx = x - ob[k, 0]
                dy = y - ob[k, 1]
                dz = kappa * (z - ob[k, 2])
                c = np.sqrt((dx * dx + dy * dy) + dz * dz) - ob[k, 3]
                wins = c < clearance[p, :m]
                if second:
                    loses = ~wins & (c < runner_up[p, :m])
                    runner_up[p, :m][wins] = clearance[p, :m][wins]
                    runner_up[p, :m][loses] = c[loses]
            clearance[p, :m][wins] = c[wins]
            nearest[p, :m][wins] = k
    min_clearance = np.full(P, np.inf)
    argmin = np.full((P, 2), -1, dtype=np.int32)
    for p in range(P):
        for r in range(live[p]):          # the first row strictly below every row in front of it
            if clearance[p, r] < min_clearance[p]:
                min_clearance[p], argmin[p] = clearance[p, r], (r, nearest[p, r])
    out = dict(clearance=clearance, nearest=nearest, min_clearance=min_clearance, argmin=argmin)
    if second:
        out["second"] = runner_up
    return out


def _followed(arr, nearest):
    """the (p, r, k) of every row whose nearest entry is followed: a live row, the entry in the path's own set"""
    n, st = arr["n"], arr["status"]
    P, cap = nearest.shape
    out = []
    for p in range(P):
        begin, end = path_bounds(arr, p)
        for r in range(live_rows(n[p], st[p], cap)):
            k = int(nearest[p, r])
            if begin <= k < end:
                out.append((p, r, k))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def torch_clearance(torch, samples, obstacles, triples, z_scale):
    """c of the given (p, r, k) triples as a float64 torch expression of samples [P][cap][4] (differentiable):
    sqrt(dx^2 + dy^2 + (z_scale dz)^2) - radius"""
    o = obstacles[triples[:, 2]]
    d = samples[triples[:, 0], triples[:, 1], :3] - o[:, :3]
    return torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + (z_scale * d[:, 2]) ** 2) - o[:, 3]


def obstacle_clearance_torch_grad(arr, nearest):
    """(dL/dsamples [P][cap][4], the sum of the absolute terms of every entry [P][cap][4]) for L = sum(upstream * clearance) by
    torch's float64 autograd on the FIXED nearest obstacles; rows on a centre are left out (they contribute exactly 0 by
    contract).  A row has ONE term per coordinate, so the sum of the absolute terms is the term's own size."""
    import torch
    s_np, ob, up, kappa = arr["samples"], arr["obstacles"], arr["upstream"], arr["z_scale"]
    grad, scale = np.zeros_like(s_np), np.zeros_like(s_np)
    t = _followed(arr, nearest)
    if t.shape[0]:
        with np.errstate(invalid="ignore"):
            d = s_np[t[:, 0], t[:, 1], :3] - ob[t[:, 2], :3]
            d[:, 2] *= kappa
            dist = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + d[:, 2] ** 2)
        t = t[dist != 0.0]
    if t.shape[0]:
        s = torch.tensor(np.where(np.isnan(s_np), 0.0, s_np), requires_grad=True)   # (no followed entry touches a NaN row)
        o = torch.tensor(np.where(np.isnan(ob), 0.0, ob))                           # (... or an obstacle with a NaN)
        g = torch.as_tensor(up[t[:, 0], t[:, 1]])
        # (the radius takes no part in the gradient; an infinite one would make the LOSS infinite, so it is left out of it)
        o_finite = o.clone()
        o_finite[:, 3] = torch.where(torch.isfinite(o[:, 3]), o[:, 3], torch.zeros_like(o[:, 3]))
        (gt,) = torch.autograd.grad((torch_clearance(torch, s, o_finite, torch.as_tensor(t), kappa) * g).sum(), s)
        grad = gt.numpy()
        d = s_np[t[:, 0], t[:, 1], :3] - ob[t[:, 2], :3]
        w = np.array([1.0, 1.0, kappa ** 2])
        dist = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + (kappa * d[:, 2]) ** 2)
        scale[t[:, 0], t[:, 1], :3] = np.abs(g.numpy())[:, None] * np.abs(d) * w / dist[:, None]
    return grad, scale


# ---- the chain test's batch ------------------------------------------------------------------------------------------------------

CHAIN_DT, CHAIN_CAPACITY, CHAIN_RADIUS = 0.2, 72, 2.0


def chain_batch():
    """The batch of the chain test: three 4-segment paths that fly along x through a field of nine obstacles, (batch,
    obstacles [9][4]): points and small spheres 0.8 to 1.9 m beside, above and below the lanes, so that most rows are within
    the hinge radius of one of them, none closer than decimetres, and no two at the same distance"""
    import math
    from mrs_uav_trajectory_generation_amd import problem as pr
    lanes, heights = (0.0, 2.6, 5.1), (3.0, 3.4, 2.9)
    parts = []
    for q in range(3):
        wp = [[-6.0 + 3.0 * k, lanes[q] + 0.3 * math.sin(1.3 * k + q), heights[q] + 0.1 * math.cos(0.7 * k + 2 * q), 0.0]
              for k in range(5)]
        parts.append(pr.build_vertices(np.array(wp), pr.SNAP))
    obstacles = np.array([[-5.0, 1.2, 3.1, 0.0], [-2.1, -1.0, 3.3, 0.2], [0.4, 1.3, 2.6, 0.0], [3.2, -1.2, 3.2, 0.3],
                          [5.6, 1.1, 3.0, 0.0], [-3.6, 3.9, 3.6, 0.25], [1.1, 3.8, 2.7, 0.0], [4.3, 4.0, 4.4, 0.15],
                          [-0.7, 6.3, 2.2, 0.0]])
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (len(parts), 1))), obstacles


# ---- the CPU harness -----------------------------------------------------------------------------------------------------------

def build_harness(tmp_path, sanitize=False):
    return hh.build("obstacle_harness.cpp", tmp_path, sanitize=sanitize)


def run_harness(exe, arr, nearest=None):
    """the harness on batch_arrays' dict (any offsets and path_set, well-formed or not; nearest: the array the backward pass is
    driven by instead of the forward's) -> dict(clearance [P][cap], nearest [P][cap], min_clearance [P], argmin [P][2], grad
    [P][cap][4], spared [P]: the pairs whose square root obsq::cannot_win spares).  The harness itself exits with code 3 -- and
    hh.run fails -- where leaving those pairs out would change a minimum or an index."""
    s = arr["samples"]
    P, cap = s.shape[:2]
    off = np.asarray(arr["set_offsets"])
    ob = np.asarray(arr["obstacles"], dtype=np.float64).reshape(-1, 4)
    ps = arr["path_set"]
    lines = ["%d %d %d %d %s %d %d\n" % (P, cap, ob.shape[0], off.size - 1, repr(float(arr["z_scale"])), 0 if ps is None else 1,
                                         0 if nearest is None else 1),
             _ints(off) + "\n", ("" if ps is None else _ints(ps)) + "\n", _ints(arr["n"]) + "\n", _ints(arr["status"]) + "\n",
             hh.fmt(ob) + "\n", hh.fmt(s) + "\n", hh.fmt(arr["upstream"]) + "\n"]
    if nearest is not None:
        lines.append(_ints(nearest) + "\n")
    out = dict(clearance=np.zeros((P, cap)), nearest=np.zeros((P, cap), dtype=np.int32), min_clearance=np.zeros(P),
               argmin=np.zeros((P, 2), dtype=np.int32), grad=np.zeros((P, cap, 4)), spared=np.zeros(P, dtype=np.int64))
    for q, line in enumerate(hh.run(exe, lines, P)):
        tok = line.split()
        assert len(tok) == 6 * cap + 4, (len(tok), cap)
        out["clearance"][q] = [float(t) for t in tok[:cap]]
        out["nearest"][q] = [int(t) for t in tok[cap:2 * cap]]
        out["min_clearance"][q] = float(tok[2 * cap])
        out["argmin"][q] = [int(tok[2 * cap + 1]), int(tok[2 * cap + 2])]
        out["grad"][q] = np.array([float(t) for t in tok[2 * cap + 3:-1]]).reshape(cap, 4)
        out["spared"][q] = int(tok[-1])
    return out


same_bits, live_rows, _ints = hh.same_bits, hh.live_rows, hh.ints


def grads_agree(got, want, scale):
    return hh.grads_agree(got, want, scale, GRAD_RTOL)
