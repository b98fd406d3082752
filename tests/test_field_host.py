"""The clearance from a voxel distance field and its backward pass on the CPU: csrc/mrs_tg_field.hpp (the inside test and cell
choice, the trilinear interpolant, the field's gradient, the cell's encoding and validation, the row gradient of
field_clearance_kernel / field_clearance_vjp_kernel) compiled by g++ into tests/host/field_harness.cpp, against the numpy
restatement of tests/field_util.py in BITS (both sides do the same correctly rounded subtract, divide, multiply and add) and
against torch's float64 autograd of the same trilinear expression gathered at the forward's cells (to 1e-13 of the sum of the
absolute terms); the closed form on an affine field; the Lipschitz bound against the exact clearance from nine spheres; the
exact zeros of the contract; the defensive rules on path_field and cell arrays that are not well-formed, also in a stand-alone
build of the same harness under AddressSanitizer and UndefinedBehaviorSanitizer, run as its own process; and the Python-side
host checks.  No GPU."""
import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api
from tests import field_util as fu
from tests import obstacle_util as ou


@pytest.fixture(scope="module")
def cases():
    return fu.named_cases()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return fu.build_harness(tmp_path_factory.mktemp("field"))


@pytest.fixture(scope="module")
def numpy_results(cases):
    """the restatement, once for all tests"""
    return {name: fu.field_clearance_numpy(fu.batch_arrays(c)) for name, c in cases.items()}


def _cell_ijk(c, cell):
    F, nz, ny, nx = c["fields"].shape
    return cell % nx, (cell // nx) % ny, (cell // (nx * ny)) % nz, cell // (nx * ny * nz)


def test_cases_have_the_properties_their_names_state(cases, numpy_results):
    res = numpy_results
    inside_rows = 0
    for m in fu.ROW_COUNTS:
        c, r = cases["rows_%d" % m], res["rows_%d" % m]
        assert [p["rows"].shape[0] for p in c["paths"]] == [m, m] and c["fields"].shape == (1, 70, 4, 5)
        assert np.all(r["cell"][:, m:] == -1) and np.all(r["clearance"][:, m:] == np.inf)
        inside_rows += int((r["cell"] >= 0).sum())
    assert inside_rows > 600
    r = res["rows_257"]
    assert np.any(r["cell"][:, :257] >= 0) and np.any(r["cell"][:, :257] == -1)        # most inside, some strayed out
    over = cases["count_of_capacity_plus_1"]
    assert all(p["n_samples"] == fu.capacity_of(over) + 1 for p in over["paths"])
    assert np.any(res["count_of_capacity_plus_1"]["cell"][:, -1] >= 0)                  # the last row of the capacity is live
    r, c = res["dead_path_of_nan_rows_between_live_ones"], cases["dead_path_of_nan_rows_between_live_ones"]
    assert [p["status"] for p in c["paths"]] == [1, 0, 1] and np.isnan(c["paths"][1]["rows"]).all()
    assert np.any(r["cell"][[0, 2], :12] >= 0) and np.all(r["cell"][1] == -1) and np.all(r["clearance"][1] == np.inf)
    assert np.all(r["argmin"][1] == -1)
    for dims in fu.DIMS:
        for s in range(2):
            c, r = cases["grid_%dx%dx%d_spacing_%d" % (dims + (s,))], res["grid_%dx%dx%d_spacing_%d" % (dims + (s,))]
            assert c["fields"].shape == (1, dims[2], dims[1], dims[0]) and c["spacing"] == fu.SPACINGS[s]
            assert (r["cell"] >= 0).sum() > 30
            i, j, k, f = _cell_ijk(c, r["cell"][r["cell"] >= 0].astype(np.int64))
            assert i.max() <= dims[0] - 2 and j.max() <= dims[1] - 2 and k.max() <= dims[2] - 2 and not f.any()
            assert i.min() >= 0 and j.min() >= 0 and k.min() >= 0
    c, r = cases["fields_4"], res["fields_4"]
    assert c["fields"].shape[0] == 4 and c["path_field"] == [0, 0, 1, 2, 3, -1, 4]
    per_grid = int(np.prod(c["fields"].shape[1:]))
    for q, f in enumerate(c["path_field"]):
        got = r["cell"][q][r["cell"][q] >= 0]
        if 0 <= f < 4:
            assert got.size > 5 and np.all(got // per_grid == f), q                      # two paths share grid 0
        else:
            assert got.size == 0 and np.all(r["clearance"][q] == np.inf) and np.all(r["argmin"][q] == -1), q
    c, r = cases["fields_4_path_field_null"], res["fields_4_path_field_null"]
    assert c["path_field"] is None and fu.batch_arrays(c)["path_field"] is None
    assert np.all(r["cell"] < per_grid) and np.any(r["cell"] >= 0)
    # the named rows
    rows = fu.named_rows()
    at = fu.NAMED_ROWS
    c, r = cases["named_rows_outside_inf"], res["named_rows_outside_inf"]
    nx, ny, nz = fu.NAMED_DIMS
    cell, grad = r["cell"][0], r["gradient"][0]
    assert cell[at["on_node_0_0_0"]] == 0 and r["clearance"][0, at["on_node_0_0_0"]] == c["fields"][0, 0, 0, 0]   # t = 0
    for a, axis in enumerate("xyz"):
        i, j, k, _ = _cell_ijk(c, int(cell[at["upper_face_" + axis]]))
        assert (i, j, k)[a] == fu.NAMED_DIMS[a] - 2, axis                           # the upper face: the LAST cell, t = 1
        assert cell[at["lower_face_" + axis]] >= 0, axis
        assert cell[at["ulp_above_" + axis]] == -1 and cell[at["ulp_below_" + axis]] == -1, axis
        assert rows[at["ulp_above_" + axis], a] == np.nextafter(rows[at["upper_face_" + axis], a], np.inf)
    assert cell[at["far_corner"]] == ((nz - 2) * ny + (ny - 2)) * nx + (nx - 2)
    assert r["clearance"][0, at["far_corner"]] == c["fields"][0, -1, -1, -1]           # every t = 1: the far voxel itself
    i, j, k, _ = _cell_ijk(c, int(cell[at["interior_node_0_1_2"]]))
    assert (i, j, k) == (0, 1, 2)                                                     # a node inside: the UPPER cell
    assert r["clearance"][0, at["interior_node_0_1_2"]] == c["fields"][0, 2, 1, 0]
    for name in ("nan_x", "nan_z", "plus_inf_y", "minus_inf_x", "huge_z", "minus_huge_x"):
        assert cell[at[name]] == -1 and r["clearance"][0, at[name]] == np.inf and not grad[at[name]].any(), name
    assert np.array_equal(cell == -1, np.isinf(r["clearance"][0]))
    # outside_value -1: an outside row IS the path's minimum, with cell -1; NaN: written as it is, never a minimum
    r = res["named_rows_outside_minus_1"]
    first_out = int(np.argmax(r["cell"][0, :rows.shape[0]] == -1))
    assert r["clearance"][0, first_out] == -1.0 and r["min_clearance"][0] in (-1.0, r["clearance"][0].min())
    r = res["outside_minus_1_random"]
    for q in range(2):
        assert r["min_clearance"][q] == -1.0 and r["argmin"][q, 1] == -1 and r["cell"][q, r["argmin"][q, 0]] == -1
        assert r["argmin"][q, 0] == int(np.argmax(r["clearance"][q] == -1.0))
    for name in ("named_rows_outside_nan", "outside_nan_random"):
        r = res[name]
        live = np.arange(r["cell"].shape[1])[None, :] < fu.batch_arrays(cases[name])["n"][:, None]
        assert np.all(np.isnan(r["clearance"][live & (r["cell"] == -1)])) and np.isfinite(r["min_clearance"]).all()
        assert np.all(r["argmin"][:, 1] >= 0)
    # -0.0 at the origin: inside, cell 0 along x, the same clearance as +0.0
    c, r = cases["minus_zero_at_the_origin"], res["minus_zero_at_the_origin"]
    assert np.signbit(c["paths"][0]["rows"][0, 0]) and r["cell"][0, 0] == r["cell"][0, 1] >= 0
    assert r["clearance"][0, 0] == r["clearance"][0, 1]
    # one +inf voxel: NaN where it is the low corner, not finite wherever the cell touches it, no other row touched
    for tag in ("inf", "nan"):
        c, r = cases["one_%s_voxel" % tag], res["one_%s_voxel" % tag]
        assert np.all(np.isnan(r["clearance"][0, :8])), tag
        i, j, k, _ = _cell_ijk(c, r["cell"].astype(np.int64))
        touches = (r["cell"] >= 0) & (np.abs(i - 0.5) < 1) & (np.abs(j - 0.5) < 1) & (np.abs(k - 1.5) < 1)
        assert touches[0, :16].all() and not np.isfinite(r["clearance"][touches]).any(), tag
        assert np.isfinite(r["clearance"][(r["cell"] >= 0) & ~touches]).all(), tag
        assert np.isfinite(r["min_clearance"]).all() and not touches[np.arange(2), r["argmin"][:, 0]].any(), tag
        clean = dict(c, fields=np.where(np.isfinite(c["fields"]), c["fields"], 0.0))
        ref = fu.field_clearance_numpy(fu.batch_arrays(clean))
        assert fu.same_bits(ref["clearance"][~touches], r["clearance"][~touches]), tag


def _check_case(name, c, got, want, torch_too=True):
    arr = fu.batch_arrays(c)
    P, cap = arr["samples"].shape[:2]
    assert fu.same_bits(got["clearance"], want["clearance"]), name
    assert np.array_equal(got["cell"], want["cell"]), name
    assert fu.same_bits(got["gradient"], want["gradient"]), name
    assert fu.same_bits(got["min_clearance"], want["min_clearance"]) and np.array_equal(got["argmin"], want["argmin"]), name
    assert fu.same_bits(got["grad"], fu.field_clearance_vjp_numpy(arr, want["cell"])), name
    # g * gradient_out and the backward pass: the same bits
    has = got["cell"] >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        product = np.where(arr["upstream"][..., None] == 0.0, 0.0, arr["upstream"][..., None] * got["gradient"][..., :3])
    assert fu.same_bits(got["grad"][..., :3][has], product[has]), name
    # exact zeros: column 3, the rows from n on, dead paths, rows without a cell
    assert not got["grad"][:, :, 3].any() and not got["gradient"][:, :, 3].any(), name
    for q in range(P):
        m = fu.live_rows(arr["n"][q], arr["status"][q], cap)
        assert not got["grad"][q, m:].any() and not got["gradient"][q, m:].any(), (name, q)
    assert not got["grad"][got["cell"] == -1].any() and not got["gradient"][got["cell"] == -1].any(), name
    if not torch_too or not np.isfinite(c["fields"]).all():
        return 0
    grad, scale = fu.field_clearance_torch_grad(arr, want["cell"])
    assert fu.grads_agree(got["grad"], grad, scale), name
    return int((scale[:, :, :3] > 0.0).sum())


def test_harness_is_the_restatement_in_bits_and_torchs_gradient(harness, cases, numpy_results):
    entries = 0
    for name, c in cases.items():
        entries += _check_case(name, c, fu.run_harness(harness, fu.batch_arrays(c)), numpy_results[name])
    assert entries > 5000                    # gradient entries that were held to torch's


def test_affine_field_is_reproduced_exactly(cases, numpy_results, harness):
    """a + b x + c y + d z with power-of-two coefficients on the power-of-two grid: every operation is exact, so the clearance
    IS the closed form and the gradient IS (b, c, d) at every inside row, the faces and the far corner included"""
    c = cases["affine"]
    got = fu.run_harness(harness, fu.batch_arrays(c))
    a, b, cc, d = fu.AFFINE
    inside = 0
    for q, p in enumerate(c["paths"]):
        rows = p["rows"]
        m = rows.shape[0]
        has = got["cell"][q, :m] >= 0
        want = a + b * rows[:, 0] + cc * rows[:, 1] + d * rows[:, 2]
        assert np.array_equal(got["clearance"][q, :m][has], want[has])
        assert np.all(got["gradient"][q, :m][has] == [b, cc, d, 0.0])
        inside += int(has.sum())
    assert inside >= 200 + 8 and np.all(got["cell"][0, :200] >= 0)


@pytest.mark.parametrize("z_scale", [1.0, 0.5])
@pytest.mark.parametrize("spacing", fu.SPACINGS)
def test_field_of_nine_spheres_is_within_a_cell_diagonal_of_the_exact_clearance(harness, spacing, z_scale):
    """The exact clearance d(x) of DESIGN.md section 11j is 1-Lipschitz in x (for z_scale <= 1: the weighted distance is no
    larger than the Euclidean one), and the interpolant at x is a convex combination (t in [0, 1]) of d at the eight corners,
    none farther from x than the cell's diagonal: |interpolant - d(x)| <= sqrt(hx^2 + hy^2 + hz^2), plus 1e-12 for rounding."""
    dims = (8, 6, 9)
    g = api.FieldGeometry(fu.ORIGIN, spacing, dims, 1)
    field = fu.field_from_obstacles(fu.NINE_SPHERES, g, z_scale)
    assert field.shape == (9, 6, 8) and np.isfinite(field).all() and field.min() < 0.0 < field.max()
    rng = np.random.default_rng(500)
    lo, hi = np.array(fu.ORIGIN), fu.upper_corner(fu.ORIGIN, spacing, dims)
    rows = np.zeros((300, 4))
    rows[:, :3] = rng.uniform(lo, hi, (300, 3))
    if spacing == fu.SPACINGS[0]:           # (dyadic spacing: the far faces are the doubles origin + (n - 1) h, and inside)
        rows[:8, :3] = [[(lo, hi)[b][a] for a, b in enumerate(bits)] for bits in np.ndindex(2, 2, 2)]  # the eight corners
    c = fu.case([fu.path(rows)], field[None], fu.ORIGIN, spacing)
    arr = fu.batch_arrays(c)
    got = fu.run_harness(harness, arr)
    exact = ou.obstacle_clearance_numpy(dict(arr, obstacles=fu.NINE_SPHERES, set_offsets=np.array([0, 9], dtype=np.int32),
                                             path_set=None, z_scale=z_scale))["clearance"]
    assert np.all(got["cell"][0, :300] >= 0)
    err = np.abs(got["clearance"][0, :300] - exact[0, :300])
    bound = np.sqrt(sum(h * h for h in spacing)) + 1e-12
    print("FIELD HOST: spacing %s z_scale %g: max |interpolant - exact| %.4f, bound %.4f" % (spacing, z_scale, err.max(), bound))
    assert np.all(err <= bound) and err.max() > 1e-6
    # on a node with t = 0 (every node but those of the upper faces, which are the last cell's t = 1) the field IS the exact
    # clearance, in bits
    nodes = fu.node_coordinates(g)[:-1, :-1, :-1].reshape(-1, 3)
    on = np.zeros((nodes.shape[0], 4))
    on[:, :3] = nodes
    arr = fu.batch_arrays(fu.case([fu.path(on)], field[None], fu.ORIGIN, spacing))
    if spacing == fu.SPACINGS[0]:                       # (dyadic spacing: a node's u is the integer, t = 0)
        assert fu.same_bits(fu.run_harness(harness, arr)["clearance"][0, :on.shape[0]], field[:-1, :-1, :-1].reshape(-1))


def test_holding_the_cell_fixed_matters(harness, cases):
    """a row on an interior node takes the UPPER cell; driven with the lower cell (where t = 1) the backward pass gives
    another gradient: the trilinear interpolant's gradient jumps across the face"""
    c = cases["named_rows_outside_inf"]
    arr = fu.batch_arrays(c)
    arr["upstream"][:] = 1.0
    at = fu.NAMED_ROWS["interior_node_0_1_2"]
    nx, ny, nz = fu.NAMED_DIMS
    fwd = fu.run_harness(harness, arr)
    upper = fwd["cell"].copy()
    assert upper[0, at] == (2 * ny + 1) * nx
    lower = upper.copy()
    lower[0, at] = (1 * ny + 0) * nx
    gu, gl = fu.run_harness(harness, arr, cell=upper)["grad"], fu.run_harness(harness, arr, cell=lower)["grad"]
    assert fu.same_bits(gu, fwd["grad"]) and fu.same_bits(gu[0, at], fwd["gradient"][0, at])
    assert np.all(gu[0, at, 1:3] != gl[0, at, 1:3]) and np.all(np.isfinite(gl[0, at]))
    assert fu.same_bits(gl, fu.field_clearance_vjp_numpy(arr, lower))
    assert fu.same_bits(np.delete(gu[0], at, axis=0), np.delete(gl[0], at, axis=0))


def test_exact_zeros_of_the_contract(harness, cases):
    # a zero upstream gives exactly 0, also on the +inf rows and against voxels that are not finite
    for name in ("random_fields", "fields_4", "named_rows_outside_inf", "one_inf_voxel", "one_nan_voxel"):
        a = fu.batch_arrays(cases[name])
        assert not fu.run_harness(harness, dict(a, upstream=np.zeros_like(a["upstream"])))["grad"].any(), name
    # rows without a cell get exactly 0 whatever the upstream is, infinite and NaN upstreams included
    a = fu.batch_arrays(cases["named_rows_outside_minus_1"])
    wild = a["upstream"].copy()
    wild[0, ::2], wild[0, 1::2] = np.inf, np.nan
    got = fu.run_harness(harness, dict(a, upstream=wild))
    assert not got["grad"][got["cell"] == -1].any() and (got["cell"] == -1).sum() > 10
    # a cell array of -1 gives exactly 0
    arr = fu.batch_arrays(cases["random_fields"])
    assert not fu.run_harness(harness, arr, cell=np.full(arr["upstream"].shape, -1))["grad"].any()


def _defensive_runs(exe, cases):
    """path_field and cell arrays that are not well-formed: the harness (and with it the header's grid_of_path and
    cell_of_path) reads nothing outside the fields array -- the sanitizers watch -- and gives exact zeros where the contract
    says so"""
    c = cases["fields_4"]
    arr = fu.batch_arrays(c)
    arr["upstream"][arr["upstream"] == 0.0] = 0.5
    P, cap = arr["samples"].shape[:2]
    F, nz, ny, nx = c["fields"].shape
    per_grid, total = nz * ny * nx, F * nz * ny * nx
    # path_field out of range: such a path sees nothing
    for bad in (np.full(P, -2 ** 31), np.full(P, 2 ** 31 - 1), np.full(P, 4), np.full(P, -1)):
        got = fu.run_harness(exe, dict(arr, path_field=bad.astype(np.int64)))
        assert np.all(got["cell"] == -1) and np.all(got["clearance"] == np.inf) and not got["grad"].any()
        assert not fu.run_harness(exe, dict(arr, path_field=bad.astype(np.int64)), cell=np.full((P, cap), 0))["grad"].any()
    # cell entries: -1, negative, beyond the array -> exactly 0 and no read
    for bad in (-1, -2, -2 ** 31, total, total + 5, 2 ** 31 - 1, total - 1):
        assert not fu.run_harness(exe, arr, cell=np.full((P, cap), bad))["grad"].any(), bad
    # the last node of an axis: not a low corner
    for i, j, k in ((nx - 1, 0, 0), (0, ny - 1, 0), (0, 0, nz - 1), (nx - 1, ny - 1, nz - 1)):
        for f in range(F):
            bad = ((f * nz + k) * ny + j) * nx + i
            assert not fu.run_harness(exe, arr, cell=np.full((P, cap), bad))["grad"].any(), (i, j, k, f)
    # a cell of somebody else's grid: grid 2 is path 3's own, nobody else's
    got = fu.run_harness(exe, arr, cell=np.full((P, cap), 2 * per_grid))
    assert got["grad"][3, :30].any() and not np.delete(got["grad"], 3, axis=0).any()
    # ... and the last low corner of the last grid is path 4's, and reads the array's last voxel
    last = ((3 * nz + nz - 2) * ny + ny - 2) * nx + nx - 2
    got = fu.run_harness(exe, arr, cell=np.full((P, cap), last))
    assert got["grad"][4, :65].any() and not np.delete(got["grad"], 4, axis=0).any()
    assert fu.same_bits(got["grad"], fu.field_clearance_vjp_numpy(arr, np.full((P, cap), last)))
    # no grid at all
    got = fu.run_harness(exe, dict(arr, fields=np.zeros((0, nz, ny, nx))), cell=np.full((P, cap), 0))
    assert np.all(got["cell"] == -1) and np.all(got["clearance"] == np.inf) and not got["grad"].any()


def test_defensive_rules(harness, cases):
    _defensive_runs(harness, cases)


def test_harness_is_clean_under_the_sanitizers(tmp_path, cases, numpy_results):
    """the same stand-alone program built with -fsanitize=address,undefined and run as its own process"""
    exe = fu.build_harness(tmp_path, sanitize=True)
    for name in ("rows_65", "grid_2x2x2_spacing_0", "grid_5x4x70_spacing_1", "fields_4", "fields_4_path_field_null",
                 "named_rows_outside_inf", "named_rows_outside_nan", "minus_zero_at_the_origin", "one_inf_voxel",
                 "random_fields"):
        _check_case(name, cases[name], fu.run_harness(exe, fu.batch_arrays(cases[name])), numpy_results[name], torch_too=False)
    _defensive_runs(exe, cases)


def test_host_field_geometry_is_checked():
    g = api.FieldGeometry((-1.0, 2.0, 0.5), (0.25, 0.5, 1.0), (5, 4, 70), 3)
    assert api.check_field_geometry((3, 70, 4, 5), g) is g and g.fields_shape() == (3, 70, 4, 5)
    s = g.as_struct()
    assert list(s.origin) == [-1.0, 2.0, 0.5] and list(s.spacing) == [0.25, 0.5, 1.0] and list(s.dims) == [5, 4, 70]
    assert s.n_fields == 3
    assert api.check_field_geometry((0, 2, 2, 2), api.FieldGeometry((0, 0, 0), (1, 1, 1), (2, 2, 2), 0)).n_fields == 0
    nan, inf = float("nan"), float("inf")
    for shape, bad in (((3, 70, 4, 5), api.FieldGeometry((0, 0, 0), (1, 1, 1), (70, 4, 5), 3)),      # nx and nz swapped
                       ((3, 70, 4, 5), api.FieldGeometry((0, 0, 0), (1, 1, 1), (5, 4, 70), 2)),
                       ((70, 4, 5), api.FieldGeometry((0, 0, 0), (1, 1, 1), (5, 4, 70), 1)),
                       ((1, 1, 4, 5), api.FieldGeometry((0, 0, 0), (1, 1, 1), (5, 4, 1), 1)),
                       ((1, 2, 2, 2), api.FieldGeometry((0, 0, 0), (1, 0.0, 1), (2, 2, 2), 1)),
                       ((1, 2, 2, 2), api.FieldGeometry((0, 0, 0), (1, 1, -1.0), (2, 2, 2), 1)),
                       ((1, 2, 2, 2), api.FieldGeometry((0, 0, 0), (nan, 1, 1), (2, 2, 2), 1)),
                       ((1, 2, 2, 2), api.FieldGeometry((0, 0, 0), (1, inf, 1), (2, 2, 2), 1)),
                       ((1, 2, 2, 2), api.FieldGeometry((0, nan, 0), (1, 1, 1), (2, 2, 2), 1)),
                       ((1, 2, 2, 2), api.FieldGeometry((inf, 0, 0), (1, 1, 1), (2, 2, 2), 1)),
                       ((0, 2, 2, 2), api.FieldGeometry((0, 0, 0), (1, 1, 1), (2, 2, 2), -1)),
                       ((2, 1024, 1024, 1024), api.FieldGeometry((0, 0, 0), (1, 1, 1), (1024, 1024, 1024), 2)),
                       ((1, 2, 2, 2), ((0, 0, 0), (1, 1, 1), (2, 2, 2), 1))):
        with pytest.raises(ValueError):
            api.check_field_geometry(shape, bad)
    with pytest.raises(ValueError):
        api.FieldGeometry((0, 0), (1, 1, 1), (2, 2, 2))
    # 2^31 - 1 voxels pass, one more does not
    api.check_field_geometry((1, 536870911, 2, 2), api.FieldGeometry((0, 0, 0), (1, 1, 1), (2, 2, 536870911), 1))
    with pytest.raises(ValueError):
        api.check_field_geometry((1, 536870912, 2, 2), api.FieldGeometry((0, 0, 0), (1, 1, 1), (2, 2, 536870912), 1))


def test_new_names_of_the_python_layer():
    assert api.CAP_FIELD_CLEARANCE == 262144 and api.CAP_FIELD_CLEARANCE == 2 * api.CAP_OBSTACLE_CLEARANCE
    assert (api.KERNEL_FIELD_CLEARANCE, api.KERNEL_FIELD_CLEARANCE_VJP) == (39, 40)
    assert {"mrs_tg_plan_field_clearance", "mrs_tg_plan_field_clearance_vjp"} <= set(api.EXPORTED_SYMBOLS)
    for name in ("field_clearance", "field_clearance_vjp"):
        assert callable(getattr(api.Plan, name))
    from mrs_uav_trajectory_generation_amd import autograd
    assert callable(autograd.field_clearance)
