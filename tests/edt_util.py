"""What the tests of the distance field from an occupancy grid share (mrs_tg_field_from_occupancy, csrc/mrs_tg_edt.hpp, DESIGN.md
section 11l): the named occupancy patterns and the cases built from them, an independent numpy BRUTE FORCE of the definition --
per node the minimum of q = (wx di^2 + wy dj^2) + wz dk^2 over ALL nodes of the other class, the three products and two sums
rounded in that order; it knows no passes and no scan -- and the CPU harness tests/host/edt_harness.cpp with its line grammar.

A case is dict(dims (nx, ny, nz), spacing, z_scale, max_distance, signed, occupancy [F][nz][ny][nx] uint8, names [F]): the
patterns of one geometry stacked as the grids of one call, which never see each other."""
import numpy as np

from mrs_uav_trajectory_generation_amd import api
from tests import field_util as fu
from tests import host_harness as hh

ORIGIN = fu.ORIGIN                       # (-1, 2, 0.5): plays no part in the values
SPACINGS = fu.SPACINGS                   # (0.25, 0.5, 1.0): every product and sum exact; (0.3, 0.7, 1.1): every one rounded
Z_SCALES = (1.0, 0.5)
# nx, ny, nz: the chunk edges of the x pass (63, 64, 65, 130), the tile edges of the y and z passes (65 rows with 64 columns, 130
# rows with 32), a z extent of 70, and the smallest grid
SMALL_DIMS = ((2, 2, 2), (2, 3, 5), (5, 4, 70), (63, 2, 2), (64, 3, 2), (65, 2, 3), (130, 3, 2), (2, 65, 3), (3, 2, 130))
SPARSE_DIMS = (33, 31, 35)               # at density 0.02 only: several occupied voxels, most scans several steps long
SAME_BITS = fu.same_bits


def caps_for(spacing):
    """+inf, 1.0, and on the 0.25 grid 0.5: two voxels along x, a cap that is attained exactly"""
    return (np.inf, 1.0, 0.5) if spacing[0] == 0.25 else (np.inf, 1.0)


def geometry_of(c, n_fields=None):
    return api.FieldGeometry(ORIGIN, c["spacing"], c["dims"], c["occupancy"].shape[0] if n_fields is None else n_fields)


# ---- occupancy patterns -----------------------------------------------------------------------------------------------------------

def patterns(dims, seed=0, densities=(0.02, 0.2, 0.8, 0.98), only_random=False):
    """name -> [nz][ny][nx] uint8"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    out = {}
    zeros = lambda: np.zeros((nz, ny, nx), dtype=np.uint8)
    if not only_random:
        out["all_free"] = zeros()
        out["all_occupied"] = np.ones((nz, ny, nx), dtype=np.uint8)
        for q in range(8):
            g = zeros()
            g[(nz - 1) * (q >> 2 & 1), (ny - 1) * (q >> 1 & 1), (nx - 1) * (q & 1)] = 1
            out["corner_%d" % q] = g
        g = zeros()
        g[nz // 2, ny // 2, nx // 2] = 1
        out["middle"] = g
        for axis, name in ((2, "plane_x"), (1, "plane_y"), (0, "plane_z")):
            g = zeros()
            index = [slice(None)] * 3
            index[axis] = g.shape[axis] // 2
            g[tuple(index)] = 1
            out[name] = g
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        out["checkerboard"] = ((i + j + k) % 2).astype(np.uint8)
    for density in densities:
        out["random_%g" % density] = (rng.random((nz, ny, nx)) < density).astype(np.uint8)
    if not only_random:
        # the pattern of random_0.2 with the bytes 1, 7 and 255: all mean occupied
        out["bytes_1_7_255"] = out["random_0.2"] * rng.choice(np.array([1, 7, 255], dtype=np.uint8), (nz, ny, nx))
    return out


def stacked(dims, spacing, z_scale, max_distance, signed, grids):
    names = list(grids)
    return dict(dims=tuple(dims), spacing=tuple(spacing), z_scale=float(z_scale), max_distance=float(max_distance),
                signed=bool(signed), names=names, occupancy=np.ascontiguousarray(np.stack([grids[n] for n in names])))


def geometries():
    """(dims, spacing, z_scale, grids) of every geometry the cases are built on"""
    for d, dims in enumerate(SMALL_DIMS):
        for spacing in SPACINGS:
            for z_scale in Z_SCALES:
                yield dims, spacing, z_scale, patterns(dims, seed=100 + d)
    for spacing in SPACINGS:
        for z_scale in Z_SCALES:
            yield SPARSE_DIMS, spacing, z_scale, patterns(SPARSE_DIMS, seed=77, densities=(0.02,), only_random=True)


def all_cases():
    """every geometry with both modes and its caps"""
    for dims, spacing, z_scale, grids in geometries():
        for signed in (True, False):
            for cap in caps_for(spacing):
                yield stacked(dims, spacing, z_scale, cap, signed, grids)


def case_name(c):
    return "%dx%dx%d h=%s z_scale=%g cap=%g %s" % (c["dims"] + (c["spacing"], c["z_scale"], c["max_distance"],
                                                               "signed" if c["signed"] else "unsigned"))


# ---- the brute force --------------------------------------------------------------------------------------------------------------

def weights(spacing, z_scale):
    hx, hy, hz = (np.float64(x) for x in spacing)
    hz = np.float64(z_scale) * hz
    return hx * hx, hy * hy, hz * hz


def _nearest(targets, sources, w):
    """[T]: per target node (k, j, i) the minimum of q over the source nodes, +inf without sources"""
    out = np.full(len(targets), np.inf)
    if len(sources) == 0 or len(targets) == 0:
        return out
    step = max(1, 2_000_000 // len(sources))
    sk, sj, si = (sources[:, a][None, :] for a in range(3))
    for t0 in range(0, len(targets), step):
        part = targets[t0:t0 + step]
        dk, dj, di = (part[:, a][:, None] - s for a, s in enumerate((sk, sj, si)))
        q = (w[0] * (di * di).astype(np.float64) + w[1] * (dj * dj).astype(np.float64)) + w[2] * (dk * dk).astype(np.float64)
        out[t0:t0 + step] = q.min(axis=1)
    return out


def other_class_distances(grid, spacing, z_scale):
    """[nz][ny][nx]: D_occ at the free nodes and D_free at the occupied ones -- what the value at a node is made of -- each the
    minimum over every node of the other class of the one grid"""
    occupied = grid != 0
    occ, free = np.argwhere(occupied), np.argwhere(~occupied)
    w = weights(spacing, z_scale)
    out = np.empty(grid.shape)
    out[~occupied] = _nearest(free, occ, w)
    out[occupied] = _nearest(occ, free, w)
    return out


def field_of(distances, grid, max_distance, signed):
    """the value at every node from other_class_distances"""
    occupied = grid != 0
    root = np.minimum(np.sqrt(distances), max_distance)
    return np.where(occupied, -root if signed else 0.0, root)


_DISTANCES = {}


def brute_force(c):
    """[F][nz][ny][nx]: the definition on every grid of the case by itself (the distances are shared among the cases that differ
    in mode and cap only)"""
    out = np.empty(c["occupancy"].shape)
    for f, grid in enumerate(c["occupancy"]):
        key = (c["dims"], c["spacing"], c["z_scale"], grid.tobytes())
        if key not in _DISTANCES:
            _DISTANCES[key] = other_class_distances(grid, c["spacing"], c["z_scale"])
        out[f] = field_of(_DISTANCES[key], grid, c["max_distance"], c["signed"])
    return out


# ---- the CPU harness ---------------------------------------------------------------------------------------------------------------

def build_harness(tmp_path, sanitize=False):
    return hh.build("edt_harness.cpp", tmp_path, sanitize=sanitize)


def problem_lines(c):
    occ = c["occupancy"]
    nx, ny, nz = c["dims"]
    assert occ.shape[1:] == (nz, ny, nx) and occ.dtype == np.uint8
    return ["%d %d %d %d %d\n" % (occ.shape[0], nx, ny, nz, api.FIELD_SIGNED if c["signed"] else 0),
            hh.fmt(list(c["spacing"]) + [c["z_scale"], c["max_distance"]]) + "\n",
            " ".join(str(int(b)) for b in occ.reshape(-1)) + "\n"]


def run_harness(exe, cases):
    """the harness on a list of cases in one process -> a list of [F][nz][ny][nx]"""
    lines, grids = [], 0
    for c in cases:
        lines += problem_lines(c)
        grids += c["occupancy"].shape[0]
    out = iter(hh.run(exe, lines, grids))
    results = []
    for c in cases:
        occ = c["occupancy"]
        results.append(np.array([[float(t) for t in next(out).split()] for _ in range(occ.shape[0])]).reshape(occ.shape))
    return results
