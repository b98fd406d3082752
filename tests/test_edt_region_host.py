"""The update of a changed box of the distance field on the CPU (csrc/mrs_tg_edt_region.hpp through
tests/host/edt_region_harness.cpp): the plan -- reach, core, window, workspace -- against a restatement
of the definitions; the windowed passes, started from the old field, against the brute force of the NEW occupancy
(tests/edt_util.py, which knows no passes and no window) IN EVERY BIT; started from a sentinel-filled array, exactly the core
written; three overlapping updates in a row; a stack of two grids; the sanitizer build of the same stand-alone program; and
the Python layer's operand checks, which need no device."""
import os

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api
from tests import edt_region_util as ru
from tests import edt_util as eu
from tests import host_harness as hh


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ru.build_harness(tmp_path_factory.mktemp("edt_region"))


@pytest.fixture(scope="module")
def cases():
    return list(ru.all_cases())


def test_reach_core_and_window_are_the_definitions():
    inf = float("inf")
    seen = set()
    for dims in ((33, 31, 35), (20, 18, 16), (130, 3, 2), (5, 4, 70)):
        n = np.array(dims)
        for spacing in eu.SPACINGS:
            for z_scale in eu.Z_SCALES:
                for cap in (0.5, 1.0, 2.0, inf, 1e-3):
                    g = api.FieldGeometry(eu.ORIGIN, spacing, dims, 2)
                    for lo, hi in ((n // 2, n // 2), (n * 0, n * 0), (n - 1, n - 1), (n // 3, 2 * n // 3), (n * 0, n - 1)):
                        lo, hi = [int(x) for x in lo], [int(x) for x in hi]
                        got = api.field_update_query(g, lo, hi, field=1, z_scale=z_scale, max_distance=cap)
                        want = ru.expected_info(dims, spacing, z_scale, cap, lo, hi)
                        assert got == want, (dims, spacing, z_scale, cap, lo, hi, got, want)
                        seen.add((cap, tuple(got["reach"]), got["whole_grid"]))
                        assert (got["workspace_bytes"] == 0) == bool(got["whole_grid"])
                        for a in range(3):
                            assert 0 <= got["window_lo"][a] <= got["core_lo"][a] <= lo[a] <= hi[a] <= got["core_hi"][a] <= got["window_hi"][a] < dims[a]
    # a cap so small that every reach is 0: the core is the box, the window is the box
    assert all(r == (0, 0, 0) for cap, r, _ in seen if cap == 1e-3) and any(cap == 1e-3 for cap, _, _ in seen)
    assert all(whole == 1 for cap, _, whole in seen if cap == inf)
    assert {whole for cap, _, whole in seen if cap == 1.0} == {0, 1}
    # the named values
    g = api.FieldGeometry(eu.ORIGIN, (0.25, 0.5, 1.0), (33, 31, 35), 1)
    half = api.field_update_query(g, (16, 15, 17), (16, 15, 17), max_distance=0.5)
    assert half["reach"] == [2, 1, 0] and half["core_lo"] == [14, 14, 17] and half["core_hi"] == [18, 16, 17]
    assert half["window_lo"] == [12, 13, 17] and half["window_hi"] == [20, 17, 17] and half["whole_grid"] == 0
    assert half["workspace_bytes"] == 8 * 1 * 5 * 5
    whole = api.field_update_query(g, (16, 15, 17), (16, 15, 17))
    assert whole["whole_grid"] == 1 and whole["workspace_bytes"] == 0 and whole["reach"] == [32, 30, 34]
    assert whole["core_lo"] == [0, 0, 0] and whole["core_hi"] == [32, 30, 34]
    # the reach is where scan_line stops: w d^2 below T at the reach, at or above it one further
    for spacing in eu.SPACINGS:
        for cap in (0.5, 1.0, 2.0):
            T = np.nextafter(np.float64(cap) * np.float64(cap), np.inf)
            for w in eu.weights(spacing, 0.5):
                d = ru.reach(w, cap, 1024)
                assert w * np.float64(d * d) < T <= w * np.float64((d + 1) * (d + 1))


def test_the_cases_are_what_the_contract_names(cases):
    assert {rc["new"]["dims"] for rc in cases} == {(5, 4, 70), (65, 2, 3), (130, 3, 2), (2, 65, 3), (3, 2, 130), eu.SPARSE_DIMS}
    assert {rc["new"]["spacing"] for rc in cases} == set(eu.SPACINGS) and {rc["new"]["signed"] for rc in cases} == {True, False}
    assert {rc["new"]["max_distance"] for rc in cases} == {0.5, 1.0}
    names = {rc["box"] for rc in cases}
    assert names == {"middle_voxel", "face_x0", "straddle_64_128", "whole_grid", "nothing_changed"} | {"corner_%d" % q for q in range(8)}
    for rc in cases:
        old, new = rc["old"]["occupancy"], rc["new"]["occupancy"]
        (x0, y0, z0), (x1, y1, z1) = rc["lo"], rc["hi"]
        outside = np.ones(old.shape, dtype=bool)
        outside[rc["field"], z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = False
        assert np.array_equal(old[outside], new[outside]), ru.case_name(rc)
        nx, ny, nz = rc["new"]["dims"]
        info = ru.query(rc)
        if rc["box"] == "middle_voxel":
            assert rc["lo"] == rc["hi"] == (nx // 2, ny // 2, nz // 2)
        elif rc["box"].startswith("corner_"):
            q = int(rc["box"][-1])
            assert (x0 == 0 or x1 == nx - 1) and (y0 == 0 or y1 == ny - 1) and (z0 == 0 or z1 == nz - 1)
            assert ((x1 == nx - 1) == bool(q & 1) or nx == 2) and ((z1 == nz - 1) == bool(q & 4) or nz == 2)
        elif rc["box"] == "face_x0":
            assert x0 == 0
        elif rc["box"] == "straddle_64_128":
            assert nx == 130 and info["window_lo"][0] < 64 and info["window_hi"][0] >= 128 and not info["whole_grid"]
            assert info["core_lo"][0] < 64 and info["core_hi"][0] > 64       # the workspace's columns cross a chunk edge too
        elif rc["box"] == "whole_grid":
            assert rc["lo"] == (0, 0, 0) and rc["hi"] == (nx - 1, ny - 1, nz - 1) and info["whole_grid"] == 1
        else:
            assert np.array_equal(old, new)
    density = {rc["old"]["dims"]: rc["old"]["occupancy"].mean() for rc in cases}
    assert abs(density[eu.SPARSE_DIMS] - 0.02) < 0.01 and all(abs(v - 0.2) < 0.1 for k, v in density.items() if k != eu.SPARSE_DIMS)
    # both routes are among the cases
    assert {ru.query(rc)["whole_grid"] for rc in cases} == {0, 1}


def test_harness_is_the_brute_force_of_the_new_occupancy_and_writes_the_core_alone(harness, cases):
    old_fields = [eu.brute_force(rc["old"]) for rc in cases]
    got = ru.run_harness(harness, cases, old_fields)
    changed = at_cap = below_cap = windows = 0
    for rc, old_field, (info, updated, marked) in zip(cases, old_fields, got):
        name = ru.case_name(rc)
        c = rc["new"]
        want = eu.brute_force(c)
        assert info == ru.query(rc) == ru.expected_info(c["dims"], c["spacing"], c["z_scale"], c["max_distance"], rc["lo"], rc["hi"]), name
        assert eu.SAME_BITS(updated, want), name
        core = ru.core_mask(info, c["dims"], c["occupancy"].shape[0], rc["field"])
        # from a sentinel-filled array: the core holds the new field (no field value is the sentinel), nothing else is written
        assert eu.SAME_BITS(marked[core], want[core]) and np.all(marked[~core] == ru.SENTINEL), name
        assert not np.any(want == ru.SENTINEL)
        # outside the core the old field already is the new one
        assert eu.SAME_BITS(old_field[~core], want[~core]), name
        differs = old_field.view(np.int64) != want.view(np.int64)
        assert not differs[~core].any()
        changed += int(differs.sum())
        at_cap += int((differs & (np.abs(want) == c["max_distance"])).sum())
        below_cap += int((differs & (np.abs(want) < c["max_distance"])).sum())
        windows += 1 - info["whole_grid"]
    print("EDT REGION HOST: %d cases (%d through a window), %d core nodes changed their bits, %d of them to the cap, %d below it"
          % (len(cases), windows, changed, at_cap, below_cap))
    assert changed > 1000 and at_cap > 0 and below_cap > 0 and windows > len(cases) // 2


def test_three_overlapping_updates_end_in_the_full_rebuilds_bits(harness):
    dims = eu.SPARSE_DIMS
    for (spacing, z_scale), cap, signed in zip(ru.GEOMETRIES, (1.0, 1.0), (True, False)):
        grid = ru.old_grid(dims, 41)
        field = eu.brute_force(eu.stacked(dims, spacing, z_scale, cap, signed, {"g": grid}))
        start = field.copy()
        for step, (lo, hi) in enumerate((((10, 10, 10), (16, 15, 14)), ((14, 12, 12), (20, 18, 17)), ((8, 14, 13), (15, 20, 16)))):
            new = ru.changed_occupancy(grid, lo, hi, 50 + step)
            rc = ru.region_case(dims, spacing, z_scale, cap, signed, {"g": grid}, {"g": new}, 0, lo, hi, "step_%d" % step)
            (info, field, _), = ru.run_harness(harness, [rc], [field])
            assert not info["whole_grid"]
            grid = new
        rebuilt = eu.brute_force(eu.stacked(dims, spacing, z_scale, cap, signed, {"g": grid}))
        assert eu.SAME_BITS(field, rebuilt) and not eu.SAME_BITS(field, start)


def test_updating_grid_1_of_a_stack_of_two_leaves_grid_0_untouched(harness):
    dims = (5, 4, 70)
    a, b = ru.old_grid(dims, 7), ru.old_grid(dims, 8)
    lo, hi = (1, 1, 30), (3, 2, 36)
    b_new = ru.changed_occupancy(b, lo, hi, 9)
    for (spacing, z_scale), signed in zip(ru.GEOMETRIES, (True, False)):
        rc = ru.region_case(dims, spacing, z_scale, 1.0, signed, {"a": a, "b": b}, {"a": a, "b": b_new}, 1, lo, hi, "stack")
        old_field = eu.brute_force(rc["old"])
        (info, updated, marked), = ru.run_harness(harness, [rc], [old_field])
        want = eu.brute_force(rc["new"])
        assert eu.SAME_BITS(updated, want) and eu.SAME_BITS(updated[0], old_field[0]) and not eu.SAME_BITS(updated[1], old_field[1])
        core = ru.core_mask(info, dims, 2, 1)
        assert not core[0].any() and np.all(marked[0] == ru.SENTINEL) and np.all(marked[~core] == ru.SENTINEL)
        assert eu.SAME_BITS(marked[core], want[core])
        # grid 0 of the same geometry with the same box is another update: the harness addresses the grid it is told
        rc0 = ru.region_case(dims, spacing, z_scale, 1.0, signed, {"a": a, "b": b}, {"a": a, "b": b}, 0, lo, hi, "stack")
        (_, same, marked0), = ru.run_harness(harness, [rc0], [old_field])
        assert eu.SAME_BITS(same, old_field) and np.all(marked0[1] == ru.SENTINEL) and not np.all(marked0[0] == ru.SENTINEL)


def test_harness_is_clean_under_the_sanitizers(tmp_path, cases):
    """the same stand-alone program built with -fsanitize=address,undefined and run as its own process"""
    exe = ru.build_harness(tmp_path, sanitize=True)
    chosen = [rc for rc in cases if rc["new"]["dims"] in ((5, 4, 70), (130, 3, 2), (2, 65, 3), (3, 2, 130)) and rc["new"]["signed"]
              and rc["new"]["max_distance"] == 1.0 and rc["new"]["spacing"] == eu.SPACINGS[1]
              and rc["box"] in ("middle_voxel", "corner_7", "straddle_64_128", "whole_grid", "face_x0")]
    assert len(chosen) == 17
    old_fields = [eu.brute_force(rc["old"]) for rc in chosen]
    for rc, (info, updated, marked) in zip(chosen, ru.run_harness(exe, chosen, old_fields)):
        assert eu.SAME_BITS(updated, eu.brute_force(rc["new"])), ru.case_name(rc)


def test_operand_checks_need_no_device():
    g = api.FieldGeometry(eu.ORIGIN, (0.25, 0.5, 1.0), (5, 4, 7), 2)
    occ = torch.zeros((2, 7, 4, 5), dtype=torch.uint8)
    fields = torch.zeros((2, 7, 4, 5), dtype=torch.float64)
    nobody = object.__new__(api.Context)      # (no device, no library: the checks come first)
    nobody.device = 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(geometry=None), dict(geometry=api.FieldGeometry(eu.ORIGIN, (0.25, 0.5, 1.0), (7, 4, 5), 2)),
               dict(geometry=api.FieldGeometry(eu.ORIGIN, (0.25, 0.0, 1.0), (5, 4, 7), 2)),
               dict(z_scale=0.0), dict(z_scale=nan), dict(max_distance=0.0), dict(max_distance=nan),
               dict(occupancy=None), dict(occupancy=occ.numpy()), dict(fields=None), dict(fields=fields.float()),
               dict(lo=(0, 0), hi=(1, 1)), dict(lo=(2, 0, 0), hi=(1, 3, 6)), dict(lo=(-1, 0, 0)), dict(hi=(5, 3, 6)),
               dict(hi=(4, 4, 6)), dict(hi=(4, 3, 7)), dict(field=2), dict(field=-1), dict(lo=None),
               dict()):                     # well-formed, but not on a device
        args = dict(occupancy=occ, fields=fields, geometry=g, lo=(1, 1, 1), hi=(2, 2, 2), field=0, z_scale=1.0, max_distance=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            api.check_region_operands(**args)
        with pytest.raises(ValueError):
            nobody.field_update_region(**args)
    # what does not depend on the tensors is refused with its own words, by the query as well
    with pytest.raises(ValueError, match="field 2 is outside"):
        api.field_update_query(g, (1, 1, 1), (2, 2, 2), field=2)
    with pytest.raises(ValueError, match="axis 0 of the box"):
        api.field_update_query(g, (3, 1, 1), (2, 2, 2))
    with pytest.raises(ValueError, match="axis 2 of the box"):
        api.field_update_query(g, (1, 1, 1), (2, 2, 7))
    with pytest.raises(ValueError, match="no grid to update"):
        api.field_update_query(api.FieldGeometry(eu.ORIGIN, (0.25, 0.5, 1.0), (5, 4, 7), 0), (1, 1, 1), (2, 2, 2))
    with pytest.raises(ValueError, match="max_distance"):
        api.field_update_query(g, (1, 1, 1), (2, 2, 2), max_distance=-1.0)
    with pytest.raises(ValueError, match="at most %d" % api.FIELD_MAX_DIM):
        api.field_update_query(api.FieldGeometry(eu.ORIGIN, (1, 1, 1), (api.FIELD_MAX_DIM + 1, 2, 2), 1), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="on the device"):
        api.check_region_operands(occ, fields, g, (1, 1, 1), (2, 2, 2))


def test_the_library_refuses_a_bad_query_without_a_context():
    """mrs_tg_field_update_query itself: host only, the error text in the global last error"""
    L = api.load_library()
    info = api.FieldUpdateInfo()

    def call(geometry=api.FieldGeometry(eu.ORIGIN, (0.25, 0.5, 1.0), (5, 4, 7), 2), z_scale=1.0, max_distance=1.0, field=1,
             lo=(1, 1, 1), hi=(2, 2, 2), region=True, out=True):
        r = api.FieldRegion()
        r.field, r.lo[:], r.hi[:] = field, lo, hi
        return L.mrs_tg_field_update_query(api.C.byref(geometry.as_struct()) if geometry else None, z_scale, max_distance,
                                           api.C.byref(r) if region else None, api.C.byref(info) if out else None)

    assert call() == 0 and list(info.reach) == [4, 2, 1] and info.whole_grid == 0 and info.workspace_bytes > 0
    for bad in (dict(geometry=None), dict(region=False), dict(out=False), dict(field=2), dict(field=-1), dict(lo=(3, 1, 1)),
                dict(lo=(-1, 1, 1)), dict(hi=(2, 4, 2)), dict(hi=(2, 2, 7)), dict(z_scale=0.0), dict(max_distance=0.0),
                dict(max_distance=float("nan")), dict(geometry=api.FieldGeometry(eu.ORIGIN, (0.25, 0.5, 1.0), (5, 4, 7), 0)),
                dict(geometry=api.FieldGeometry(eu.ORIGIN, (0.25, 0.5, 1.0), (5, 1, 7), 2)),
                dict(geometry=api.FieldGeometry(eu.ORIGIN, (0.25, 0.5, 1.0), (5, 4, 1025), 2))):
        assert call(**bad) == -1 and len(L.mrs_tg_last_error(None)) > 0, bad


def test_new_names_of_the_python_layer():
    assert api.CAP_FIELD_UPDATE_REGION == 1048576 and api.CAP_FIELD_UPDATE_REGION == 2 * api.CAP_FIELD_FROM_OCCUPANCY
    assert api.capabilities() & api.CAP_FIELD_UPDATE_REGION
    assert "mrs_tg_field_update_query" in api.EXPORTED_SYMBOLS and "mrs_tg_field_update_region" in api.EXPORTED_SYMBOLS
    assert callable(api.Context.field_update_region) and callable(api.check_region_operands) and callable(api.field_update_query)
    assert api.C.sizeof(api.FieldRegion) == 28 and api.C.sizeof(api.FieldUpdateInfo) == 72
    header = open(os.path.join(hh.ROOT, "include", "mrs_tg.h")).read()
    assert "MRS_TG_CAP_FIELD_UPDATE_REGION = 1048576" in header
    assert "int mrs_tg_field_update_query(" in header and "int mrs_tg_field_update_region(" in header
    assert "typedef struct mrs_tg_field_region {" in header and "typedef struct mrs_tg_field_update_info {" in header
    assert "forty-two ids," in header and "0 .. 41" in header          # no kernel id was added: both routes are timed as 41
    region = open(os.path.join(os.path.dirname(api.__file__), "csrc", "mrs_tg_edt_region.hpp")).read()
    assert "inline RegionPlan plan_region(" in region and "inline int reach(" in region
