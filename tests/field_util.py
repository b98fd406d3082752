"""What the tests of the clearance from a voxel distance field share (mrs_tg_plan_field_clearance, csrc/mrs_tg_field.hpp,
DESIGN.md section 11k): the named cases, a numpy restatement of the forward and of the backward pass (the same correctly
rounded subtract, divide, multiply and add in the same order, so it is held to the harness's bits), a torch restatement of the
trilinear expression for the gradients on FIXED cells, `field_from_obstacles` (the exact section-11j clearance at every node of
a grid), and the CPU harness tests/host/field_harness.cpp with its line grammar.

A case is a batch: dict(paths=[path, ...], fields [F][nz][ny][nx], origin (3,), spacing (3,), path_field=[grid, ...] or None,
outside_value=...) with path = dict(rows [m][4], n_samples, status).  The rows are built directly, not by the optimiser."""
import numpy as np

from mrs_uav_trajectory_generation_amd import api
from tests import host_harness as hh
from tests import obstacle_util as ou

GRAD_RTOL = ou.GRAD_RTOL   # of the sum of the absolute terms of an entry (the family's bound, DESIGN.md sections 11i and 11j)
ROW_COUNTS = ou.ROW_COUNTS                                   # the chunk seams (64) and the workgroup seams (256)
DIMS = ((2, 2, 2), (2, 3, 5), (5, 4, 70))                    # nx, ny, nz: all three extents distinct, so a swapped stride shows
SPACINGS = ((0.25, 0.5, 1.0), (0.3, 0.7, 1.1))
ORIGIN = (-1.0, 2.0, 0.5)
path = ou.path
same_bits = ou.same_bits
grads_agree = ou.grads_agree
live_rows = ou.live_rows


# ---- geometry and fields ---------------------------------------------------------------------------------------------------------

def upper_corner(origin, spacing, dims):
    """the far corner's coordinates as the doubles origin + (n - 1) h"""
    return np.array([origin[a] + (dims[a] - 1) * spacing[a] for a in range(3)])


def node_coordinates(geometry):
    """[nz][ny][nx][3]: the position of every node, origin + (i hx, j hy, k hz), each product and sum rounded once"""
    nx, ny, nz = geometry.dims
    o, h = geometry.origin, geometry.spacing
    out = np.zeros((nz, ny, nx, 3))
    out[..., 0] = (o[0] + np.arange(nx) * h[0])[None, None, :]
    out[..., 1] = (o[1] + np.arange(ny) * h[1])[None, :, None]
    out[..., 2] = (o[2] + np.arange(nz) * h[2])[:, None, None]
    return out


def field_from_obstacles(obstacles, geometry, z_scale=1.0):
    """[nz][ny][nx]: the exact clearance of DESIGN.md section 11j at every node of the grid -- per node the obstacles one after
    the other in increasing index, sqrt((dx dx + dy dy) + dz dz) - radius with dz = z_scale (z - oz), a strict < from +inf --
    in chunks of grid layers.  What Plan.obstacle_clearance gives for the nodes as rows, in bits."""
    ob = np.asarray(obstacles, dtype=np.float64).reshape(-1, 4)
    nodes = node_coordinates(geometry)
    out = np.full(nodes.shape[:3], np.inf)
    for k0 in range(0, nodes.shape[0], 8):
        part = nodes[k0:k0 + 8]
        best = out[k0:k0 + 8]
        for q in range(ob.shape[0]):
            with np.errstate(invalid="ignore", over="ignore"):
                dx = part[..., 0] - ob[q, 0]
                dy = part[..., 1] - ob[q, 1]
                dz = z_scale * (part[..., 2] - ob[q, 2])
                c = np.sqrt((dx * dx + dy * dy) + dz * dz) - ob[q, 3]
                wins = c < best
            best[wins] = c[wins]
    return out


def drawn_fields(n_fields, dims, rng):
    nx, ny, nz = dims
    return rng.uniform(-2.0, 6.0, (n_fields, nz, ny, nx))


def drawn_rows(m, origin, spacing, dims, rng):
    """[m][4] rows: a random walk of steps of about a voxel from a start inside the grid, reflected nowhere -- most rows are
    inside, some stray out of it"""
    rows = np.zeros((m, 4))
    if m:
        lo, hi = np.array(origin), upper_corner(origin, spacing, dims)
        start = rng.uniform(lo, hi)
        steps = rng.normal(0.0, 0.6, (m, 3)) * np.array(spacing)
        steps[0] = 0.0
        walk = start + np.cumsum(steps, axis=0)
        # fold the walk back into a box slightly larger than the grid, so that most rows are inside and some are not
        span = (hi - lo) * 1.1
        folded = np.abs(np.mod(walk - lo + 0.05 * (hi - lo), 2.0 * span) - span)
        rows[:, :3] = lo - 0.05 * (hi - lo) + (span - folded)
        rows[:, 3] = rng.uniform(-3.0, 3.0, m)
    return rows


def case(paths, fields, origin=ORIGIN, spacing=SPACINGS[0], path_field=None, outside_value=np.inf):
    fields = np.ascontiguousarray(fields, dtype=np.float64)
    assert fields.ndim == 4
    return dict(paths=list(paths), fields=fields, origin=tuple(float(x) for x in origin), spacing=tuple(float(x) for x in spacing),
                path_field=None if path_field is None else [int(q) for q in path_field], outside_value=float(outside_value))


def drawn_case(rows_per_path, dims, seed, spacing=SPACINGS[1], n_fields=1, path_field=None, outside_value=np.inf, origin=ORIGIN):
    rng = np.random.default_rng(seed)
    fields = drawn_fields(n_fields, dims, rng)
    return case([path(drawn_rows(m, origin, spacing, dims, rng)) for m in rows_per_path], fields, origin, spacing, path_field,
                outside_value)


NAMED_DIMS, NAMED_SPACING = DIMS[1], SPACINGS[0]       # the grid of the named rows: powers of two, every face a dyadic number
NAMED_ROWS = {}                                        # name -> row index in named_rows()


def named_rows():
    """the rows of the contract's edge cases on the (2, 3, 5) grid of spacing (0.25, 0.5, 1.0) at origin (-1, 2, 0.5), as
    [m][4]; NAMED_ROWS gives every one's index"""
    lo, hi = np.array(ORIGIN), upper_corner(ORIGIN, NAMED_SPACING, NAMED_DIMS)
    mid = lo + np.array([0.0625, 0.125, 1.25])          # inside cell (0, 0, 1)
    rows, names = [], {}

    def add(name, xyz):
        names[name] = len(rows)
        rows.append([xyz[0], xyz[1], xyz[2], 0.5])

    add("on_node_0_0_0", lo)
    add("interior", mid)
    for a, axis in enumerate("xyz"):
        on = mid.copy()
        on[a] = hi[a]
        add("upper_face_" + axis, on)
        out = mid.copy()
        out[a] = np.nextafter(hi[a], np.inf)
        add("ulp_above_" + axis, out)
        out = mid.copy()
        out[a] = np.nextafter(lo[a], -np.inf)
        add("ulp_below_" + axis, out)
        on = mid.copy()
        on[a] = lo[a]
        add("lower_face_" + axis, on)
    add("far_corner", hi)
    add("interior_node_0_1_2", lo + np.array([0.0, 0.5, 2.0]))     # a node with a cell on either side in y and z
    add("nan_x", [np.nan, mid[1], mid[2]])
    add("nan_z", [mid[0], mid[1], np.nan])
    add("plus_inf_y", [mid[0], np.inf, mid[2]])
    add("minus_inf_x", [-np.inf, mid[1], mid[2]])
    add("huge_z", [mid[0], mid[1], 1.0e300])
    add("minus_huge_x", [-1.0e300, mid[1], mid[2]])
    NAMED_ROWS.clear()
    NAMED_ROWS.update(names)
    return np.array(rows)


def affine_field(dims, origin, spacing, coefficients):
    """[1][nz][ny][nx]: a + b x + c y + d z at every node"""
    a, b, c, d = coefficients
    g = api.FieldGeometry(origin, spacing, dims, 1)
    nodes = node_coordinates(g)
    return (a + b * nodes[..., 0] + c * nodes[..., 1] + d * nodes[..., 2])[None]


AFFINE = (0.5, 2.0, -0.25, 0.125)      # a, b, c, d: powers of two


def dyadic_rows(m, origin, spacing, dims, rng):
    """[m][4] rows inside the grid whose coordinates are multiples of 1/64: every operation of the lookup is exact on them"""
    lo, hi = np.array(origin), upper_corner(origin, spacing, dims)
    rows = np.zeros((m, 4))
    for a in range(3):
        rows[:, a] = rng.integers(int(lo[a] * 64), int(hi[a] * 64) + 1, m) / 64.0
    return rows


def named_cases():
    """name -> case"""
    cases = {}
    for m in ROW_COUNTS:
        cases["rows_%d" % m] = drawn_case([m, m], DIMS[2], 100 + m)
    over = drawn_case([70, 70], DIMS[2], 171)
    for p in over["paths"]:
        p["n_samples"] = 71                                                   # capacity + 1: more rows than fit
    cases["count_of_capacity_plus_1"] = over
    live = drawn_case([12, 12, 12], DIMS[1], 172)
    live["paths"][1] = dict(path(np.full((12, 4), np.nan)), status=0)
    cases["dead_path_of_nan_rows_between_live_ones"] = live
    for d, dims in enumerate(DIMS):
        for s, spacing in enumerate(SPACINGS):
            cases["grid_%dx%dx%d_spacing_%d" % (dims + (s,))] = drawn_case([66, 9], dims, 200 + 10 * d + s, spacing=spacing)
    # four grids: two paths share grid 0, one names no grid (-1), one a grid behind the last
    cases["fields_4"] = drawn_case([40, 70, 66, 30, 65, 20, 9], DIMS[1], 300, n_fields=4, path_field=[0, 0, 1, 2, 3, -1, 4])
    cases["fields_4_path_field_null"] = drawn_case([40, 70, 9], DIMS[1], 301, n_fields=4, path_field=None)
    # the named rows, against a random field, with every kind of outside_value
    rng = np.random.default_rng(310)
    named_field = drawn_fields(1, NAMED_DIMS, rng)
    for tag, outside in (("inf", np.inf), ("minus_1", -1.0), ("nan", np.nan)):
        cases["named_rows_outside_" + tag] = case([path(named_rows())], named_field, ORIGIN, NAMED_SPACING, outside_value=outside)
    # x = origin at -0.0: u = -0.0, which is inside (0 <= -0.0), in cell 0 with t = -0.0
    zero = np.array([[-0.0, 2.125, 1.75, 0.0], [0.0, 2.125, 1.75, 0.0]])
    cases["minus_zero_at_the_origin"] = case([path(zero)], drawn_fields(1, NAMED_DIMS, rng), (0.0, 2.0, 0.5), NAMED_SPACING)
    # the affine field on the power-of-two grid: everything exact
    cases["affine"] = case([path(dyadic_rows(200, ORIGIN, SPACINGS[0], DIMS[2], rng)), path(named_rows())],
                           affine_field(DIMS[2], ORIGIN, SPACINGS[0], AFFINE), ORIGIN, SPACINGS[0])
    # one +inf voxel, one NaN voxel: voxel (1, 1, 2) of a (5, 4, 70) grid; rows 0..7 sit in the cell whose LOW corner it is,
    # rows 8..15 in the cell whose far corner it is, the rest anywhere
    for tag, value in (("inf", np.inf), ("nan", np.nan)):
        c = drawn_case([90, 30], DIMS[2], 320)
        c["fields"][0, 2, 1, 1] = value
        o, h = np.array(ORIGIN), np.array(SPACINGS[1])
        r = c["paths"][0]["rows"]
        r[:8, :3] = o + (np.array([1, 1, 2]) + rng.uniform(0.1, 0.9, (8, 3))) * h
        r[8:16, :3] = o + (np.array([0, 0, 1]) + rng.uniform(0.1, 0.9, (8, 3))) * h
        cases["one_%s_voxel" % tag] = c
    # an outside row IS the path's minimum with cell -1
    cases["outside_minus_1_random"] = drawn_case([80, 65], DIMS[1], 330, outside_value=-1.0)
    cases["outside_minus_1_random"]["fields"] = np.abs(cases["outside_minus_1_random"]["fields"])     # (nothing inside is below it)
    cases["outside_nan_random"] = drawn_case([80, 65], DIMS[1], 331, outside_value=np.nan)
    # random: ragged rows, several grids
    rng = np.random.default_rng(390)
    cases["random_fields"] = drawn_case(rng.integers(1, 150, 12).tolist(), DIMS[2], 391, n_fields=3,
                                        path_field=rng.integers(0, 3, 12).tolist())
    return cases


def capacity_of(c):
    return ou.capacity_of(c)


def batch_arrays(c, seed=0, capacity=None):
    """dict(samples [P][cap][4], n [P], status [P], fields [F][nz][ny][nx], origin, spacing, path_field [P] or None, upstream
    [P][cap], outside_value) of a case: the rows behind a path's own hold a sentinel that no result may depend on; the upstream
    is dyadic and covers every row, the ones outside every grid included"""
    cap = capacity_of(c) if capacity is None else int(capacity)
    P = len(c["paths"])
    rng = np.random.default_rng(77 + seed)
    samples = 1.0e3 + rng.uniform(0.0, 1.0, (P, cap, 4))
    for q, p in enumerate(c["paths"]):
        samples[q, :p["rows"].shape[0]] = p["rows"]
    upstream = rng.integers(-128, 129, (P, cap)) / 64.0
    return dict(samples=samples, n=np.array([p["n_samples"] for p in c["paths"]], dtype=np.int32),
                status=np.array([p["status"] for p in c["paths"]], dtype=np.int32), fields=c["fields"], origin=c["origin"],
                spacing=c["spacing"], path_field=None if c["path_field"] is None else np.array(c["path_field"], dtype=np.int32),
                upstream=upstream, outside_value=c["outside_value"])


def arrays_geometry(arr):
    F, nz, ny, nx = arr["fields"].shape
    return api.FieldGeometry(arr["origin"], arr["spacing"], (nx, ny, nz), F)


def explicit_path_field(c):
    F = c["fields"].shape[0]
    return list(c["path_field"]) if c["path_field"] is not None else [0 if F else -1] * len(c["paths"])


def combined_case(cases, geometry_like, outside_value):
    """every case on the geometry of `geometry_like` in one batch -- their grids stacked in one array -- with a dead path of NaN
    rows between any two of them: (case, [(name, first path, first grid), ...])"""
    paths, fields, path_field, where = [], [], [], []
    F = 0
    ref = cases[geometry_like]
    for name, c in cases.items():
        if c["fields"].shape[1:] != ref["fields"].shape[1:] or c["spacing"] != ref["spacing"] or c["origin"] != ref["origin"]:
            continue
        if paths:
            paths.append(dict(path(np.full((7, 4), np.nan)), status=0))
            path_field.append(0)
        where.append((name, len(paths), F))
        own = c["fields"].shape[0]
        paths += [dict(p) for p in c["paths"]]
        path_field += [q + F if 0 <= q < own else -1 for q in explicit_path_field(c)]
        fields.append(c["fields"])
        F += own
    return case(paths, np.concatenate(fields), ref["origin"], ref["spacing"], path_field, outside_value), where


def rotated_case(c):
    """the same case with its first path moved behind the last and its first grid moved behind the last: (case, for every path
    of the new batch its index in the old, voxels per grid)"""
    F, P = c["fields"].shape[0], len(c["paths"])
    order = list(range(1, P)) + [0]
    pf = explicit_path_field(c)
    moved = [(q - 1) % F if 0 <= q < F else q for q in pf]
    rot = case([c["paths"][q] for q in order], np.concatenate([c["fields"][1:], c["fields"][:1]]), c["origin"], c["spacing"],
               [moved[q] for q in order], c["outside_value"])
    return rot, np.array(order), int(np.prod(c["fields"].shape[1:]))


def grid_of_path(arr, p):
    F = arr["fields"].shape[0]
    q = 0 if arr["path_field"] is None else int(arr["path_field"][p])
    return q if 0 <= q < F else -1


# ---- the restatements ------------------------------------------------------------------------------------------------------------

def _lerp(a, b, t):
    return a + t * (b - a)


def _corners(F, f, i, j, k):
    """v[I + 2 J + 4 K] of the cells with low corners (i, j, k) in grid f"""
    return [F[f, k + K, j + J, i + I] for K in (0, 1) for J in (0, 1) for I in (0, 1)]


def _gradient(v, t, h):
    gx = _lerp(_lerp(v[1] - v[0], v[3] - v[2], t[1]), _lerp(v[5] - v[4], v[7] - v[6], t[1]), t[2]) / h[0]
    gy = _lerp(_lerp(v[2] - v[0], v[3] - v[1], t[0]), _lerp(v[6] - v[4], v[7] - v[5], t[0]), t[2]) / h[1]
    gz = _lerp(_lerp(v[4] - v[0], v[5] - v[1], t[0]), _lerp(v[6] - v[2], v[7] - v[3], t[0]), t[1]) / h[2]
    return gx, gy, gz


def field_clearance_numpy(arr):
    """the forward on batch_arrays' dict -> dict(clearance [P][cap], cell [P][cap] int32, gradient [P][cap][4], min_clearance
    [P], argmin [P][2] int32): u = (x - o) / h, the inside test in double, i = min((int)u, n - 2), t = u - i, four lerps in x,
    two in y, one in z; the gradient differences first, lerps afterwards"""
    s, n, st, F = arr["samples"], arr["n"], arr["status"], arr["fields"]
    o, h = arr["origin"], arr["spacing"]
    dims = (F.shape[3], F.shape[2], F.shape[1])
    P, cap = s.shape[:2]
    clearance = np.full((P, cap), np.inf)
    cell = np.full((P, cap), -1, dtype=np.int32)
    gradient = np.zeros((P, cap, 4))
    min_clearance = np.full(P, np.inf)
    argmin = np.full((P, 2), -1, dtype=np.int32)
    for p in range(P):
        m = live_rows(n[p], st[p], cap)
        f = grid_of_path(arr, p)
        if f < 0 or m == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            u = [(s[p, :m, a] - o[a]) / h[a] for a in range(3)]
            inside = np.ones(m, dtype=bool)
            for a in range(3):
                inside &= (0.0 <= u[a]) & (u[a] <= float(dims[a] - 1))
            idx = [np.minimum(np.where(inside, u[a], 0.0).astype(np.int64), dims[a] - 2) for a in range(3)]
            t = [u[a] - idx[a].astype(np.float64) for a in range(3)]
            v = _corners(F, f, idx[0], idx[1], idx[2])
            c00, c10 = _lerp(v[0], v[1], t[0]), _lerp(v[2], v[3], t[0])
            c01, c11 = _lerp(v[4], v[5], t[0]), _lerp(v[6], v[7], t[0])
            c = _lerp(_lerp(c00, c10, t[1]), _lerp(c01, c11, t[1]), t[2])
            g = _gradient(v, t, h)
        clearance[p, :m] = np.where(inside, c, arr["outside_value"])
        cell[p, :m] = np.where(inside, ((f * dims[2] + idx[2]) * dims[1] + idx[1]) * dims[0] + idx[0], -1)
        for a in range(3):
            gradient[p, :m, a] = np.where(inside, g[a], 0.0)
        for r in range(m):          # the first row strictly below every row in front of it
            if clearance[p, r] < min_clearance[p]:
                min_clearance[p], argmin[p] = clearance[p, r], (r, cell[p, r])
    return dict(clearance=clearance, cell=cell, gradient=gradient, min_clearance=min_clearance, argmin=argmin)


def followed(arr, cell):
    """the (p, r, f, i, j, k) of every row whose cell entry is followed: a live row, the cell a low corner of the path's own
    grid"""
    F = arr["fields"]
    nx, ny, nz = F.shape[3], F.shape[2], F.shape[1]
    P, cap = cell.shape
    out = []
    for p in range(P):
        f = grid_of_path(arr, p)
        for r in range(live_rows(arr["n"][p], arr["status"][p], cap)):
            q = int(cell[p, r])
            if q < 0 or f < 0:
                continue
            i, rest = q % nx, q // nx
            j, rest = rest % ny, rest // ny
            k, cf = rest % nz, rest // nz
            if cf == f and i <= nx - 2 and j <= ny - 2 and k <= nz - 2:
                out.append((p, r, f, i, j, k))
    return np.array(out, dtype=np.int64).reshape(-1, 6)


def field_clearance_vjp_numpy(arr, cell):
    """dL/dsamples [P][cap][4] restated: g (the gradient recomputed at the recorded cell, t not clamped again)"""
    s, F, o, h, up = arr["samples"], arr["fields"], arr["origin"], arr["spacing"], arr["upstream"]
    grad = np.zeros_like(s)
    w = followed(arr, cell)
    if w.shape[0]:
        p, r, f, i, j, k = (w[:, a] for a in range(6))
        g = up[p, r]
        with np.errstate(invalid="ignore", over="ignore"):
            t = [(s[p, r, a] - o[a]) / h[a] - (i, j, k)[a].astype(np.float64) for a in range(3)]
            d = _gradient(_corners(F, f, i, j, k), t, h)
            for a in range(3):
                grad[p, r, a] = np.where(g == 0.0, 0.0, g * d[a])
    return grad


def torch_trilinear(torch, samples, fields, origin, spacing, w):
    """the clearance of the (p, r, f, i, j, k) rows of w as a float64 torch expression of samples [P][cap][4]
    (differentiable), gathered at those FIXED cells"""
    p, r, f, i, j, k = (w[:, a] for a in range(6))
    o = torch.as_tensor(np.array(origin))
    h = torch.as_tensor(np.array(spacing))
    u = (samples[p, r, :3] - o) / h
    t = u - torch.stack([i, j, k], dim=1).to(torch.float64)
    v = [fields[f, k + K, j + J, i + I] for K in (0, 1) for J in (0, 1) for I in (0, 1)]
    lerp = lambda a, b, x: a + x * (b - a)
    c00, c10 = lerp(v[0], v[1], t[:, 0]), lerp(v[2], v[3], t[:, 0])
    c01, c11 = lerp(v[4], v[5], t[:, 0]), lerp(v[6], v[7], t[:, 0])
    return lerp(lerp(c00, c10, t[:, 1]), lerp(c01, c11, t[:, 1]), t[:, 2])


def gradient_scale(arr, w):
    """[P][cap][4]: the sum of the absolute terms of every entry of dL/dsamples = g (d clearance / d coordinate): per
    coordinate the eight corner values, each with the absolute bilinear weight of the other two axes, over the spacing"""
    s, F, o, h, up = arr["samples"], arr["fields"], arr["origin"], arr["spacing"], arr["upstream"]
    scale = np.zeros_like(s)
    if w.shape[0]:
        p, r, f, i, j, k = (w[:, a] for a in range(6))
        t = [(s[p, r, a] - o[a]) / h[a] - (i, j, k)[a] for a in range(3)]
        v = np.abs(np.array(_corners(F, f, i, j, k)))                       # [8][rows]
        wt = [(np.abs(1.0 - t[a]), np.abs(t[a])) for a in range(3)]
        for a in range(3):
            b, c = [x for x in range(3) if x != a]
            total = np.zeros(w.shape[0])
            for K in (0, 1):
                for J in (0, 1):
                    for I in (0, 1):
                        bit = (I, J, K)
                        total += wt[b][bit[b]] * wt[c][bit[c]] * v[I + 2 * J + 4 * K]
            scale[p, r, a] = np.abs(up[p, r]) * total / h[a]
    return scale


def field_clearance_torch_grad(arr, cell):
    """(dL/dsamples [P][cap][4], the sum of the absolute terms of every entry) for L = sum(upstream * clearance) by torch's
    float64 autograd of the trilinear expression on the FIXED cells; for finite fields and finite followed rows"""
    import torch
    w = followed(arr, cell)
    grad = np.zeros_like(arr["samples"])
    if w.shape[0]:
        s = torch.tensor(np.where(np.isfinite(arr["samples"]), arr["samples"], 0.0), requires_grad=True)
        c = torch_trilinear(torch, s, torch.as_tensor(arr["fields"]), arr["origin"], arr["spacing"], torch.as_tensor(w))
        (gt,) = torch.autograd.grad((c * torch.as_tensor(arr["upstream"][w[:, 0], w[:, 1]])).sum(), s)
        grad = gt.numpy()
    return grad, gradient_scale(arr, w)


# ---- the chain test's batch and the nine spheres --------------------------------------------------------------------------------

CHAIN_DT, CHAIN_CAPACITY, CHAIN_RADIUS = ou.CHAIN_DT, ou.CHAIN_CAPACITY, ou.CHAIN_RADIUS
CHAIN_GEOMETRY = dict(origin=(-8.0, -3.0, 1.0), spacing=(0.5, 0.5, 0.5), dims=(33, 23, 9))     # covers the three lanes


def chain_batch():
    """(batch, obstacles [9][4], geometry, field [1][nz][ny][nx]): obstacle_util's chain batch with the field of its nine
    obstacles on a grid of half a metre that holds every sample"""
    batch, obstacles = ou.chain_batch()
    g = api.FieldGeometry(CHAIN_GEOMETRY["origin"], CHAIN_GEOMETRY["spacing"], CHAIN_GEOMETRY["dims"], 1)
    return batch, obstacles, g, field_from_obstacles(obstacles, g)[None]


NINE_SPHERES = np.array([[-0.5, 2.5, 1.0, 0.25], [0.25, 3.0, 2.5, 0.5], [-0.75, 2.25, 4.0, 0.125], [0.0, 3.5, 0.75, 0.0],
                         [-1.5, 2.75, 3.0, 0.375], [0.5, 1.5, 2.0, 0.25], [-0.25, 4.0, 5.0, 0.5], [-0.9, 3.1, 1.9, 0.0625],
                         [0.1, 2.1, 3.3, 0.2]])


# ---- the CPU harness -----------------------------------------------------------------------------------------------------------

def build_harness(tmp_path, sanitize=False):
    return hh.build("field_harness.cpp", tmp_path, sanitize=sanitize)


_ints = ou._ints


def run_harness(exe, arr, cell=None):
    """the harness on batch_arrays' dict (any path_field, well-formed or not; cell: the array the backward pass is driven by
    instead of the forward's) -> dict(clearance [P][cap], cell [P][cap], gradient [P][cap][4], min_clearance [P], argmin
    [P][2], grad [P][cap][4])"""
    s = arr["samples"]
    P, cap = s.shape[:2]
    F = np.asarray(arr["fields"], dtype=np.float64)
    pf = arr["path_field"]
    lines = ["%d %d %d %d %d %d\n" % (P, cap, F.shape[0], F.shape[3], F.shape[2], F.shape[1]),
             hh.fmt(list(arr["origin"]) + list(arr["spacing"]) + [arr["outside_value"]]) + "\n",
             "%d %d\n" % (0 if pf is None else 1, 0 if cell is None else 1),
             ("" if pf is None else _ints(pf)) + "\n", _ints(arr["n"]) + "\n", _ints(arr["status"]) + "\n",
             hh.fmt(F) + "\n", hh.fmt(s) + "\n", hh.fmt(arr["upstream"]) + "\n"]
    if cell is not None:
        lines.append(_ints(cell) + "\n")
    out = dict(clearance=np.zeros((P, cap)), cell=np.zeros((P, cap), dtype=np.int32), gradient=np.zeros((P, cap, 4)),
               min_clearance=np.zeros(P), argmin=np.zeros((P, 2), dtype=np.int32), grad=np.zeros((P, cap, 4)))
    for q, line in enumerate(hh.run(exe, lines, P)):
        tok = line.split()
        assert len(tok) == 10 * cap + 3, (len(tok), cap)
        out["clearance"][q] = [float(t) for t in tok[:cap]]
        out["cell"][q] = [int(t) for t in tok[cap:2 * cap]]
        out["gradient"][q] = np.array([float(t) for t in tok[2 * cap:6 * cap]]).reshape(cap, 4)
        out["min_clearance"][q] = float(tok[6 * cap])
        out["argmin"][q] = [int(tok[6 * cap + 1]), int(tok[6 * cap + 2])]
        out["grad"][q] = np.array([float(t) for t in tok[6 * cap + 3:]]).reshape(cap, 4)
    return out
