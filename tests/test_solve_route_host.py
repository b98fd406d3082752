"""The route of the fixed-times solve on the CPU: csrc/mrs_tg_solve_route.hpp (LDS footprints and budgets, the predicates,
route_solve) compiled by g++ into tests/host/solve_route_harness.cpp.  Checked here: every fixed-times and closing-solve row of
the committed routing table, both sides of every edge the header draws (the LDS edges found by a sweep over the segment count),
every routing knob of the fixed-times section of mrs_tg_knobs.hpp at a non-default value, and the same lines through an
AddressSanitizer + UndefinedBehaviorSanitizer build.  No GPU."""
import os
import re

import pytest

from tests import host_harness as hh
from tests import solve_route_util as sr
from tests.solve_route_util import CLOSING, FORCE_ROWS, FORCE_TILE, request

KB = 1024
BUDGET = {"rows": 144 * KB, "rows_pipeline": 144 * KB, "tile": 144 * KB, "quad": 80 * KB, "duo": 80 * KB, "lane": 0}
LDS_LIMIT = 160 * KB   # a compute unit's LDS


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return sr.build(tmp_path_factory.mktemp("solve_route"))


def _one(harness, env=None, **kw):
    n, S = kw.pop("n"), kw.pop("S")
    return sr.routes(harness, [request(n, S, **kw)], env)[0]


# ---- the committed table ----

TABLE = os.path.join(hh.ROOT, "profiles", "launch_layer_routing_table.md")
MELLINGER = {"Mellinger + sampling, min-snap": 4, "Mellinger + sampling, min-acceleration (the nodelet's default)": 2}


def _table_rows():
    rows = []
    with open(TABLE) as f:
        for line in f.read().splitlines()[2:]:
            batch, options, kernels = [c.strip() for c in line.strip().strip("|").split("|")]
            names = []
            for item in kernels.split(" → "):
                m = re.fullmatch(r"`([^`]+)`(?: \(x (\d+)\+?\))?", item)
                names += [m.group(1)] * int(m.group(2) or 1)
            rows.append((batch, options, names))
    return rows


def _shape(batch):
    m = re.match(r"(\d+) x (\d+)", batch)
    if m:
        return int(m.group(1)), int(m.group(2)), None
    m = re.match(r"(\d+) ragged (\d+)\.\.(\d+)", batch)   # any spread over the range gives the route of its longest path
    return int(m.group(1)), int(m.group(3)), 0


def test_the_committed_routing_table(harness):
    lines, expect = [], []
    for batch, options, names in _table_rows():
        n, S, uniform = _shape(batch)
        if options == "fixed times, min-snap":
            lines.append(request(n, S, uniform))
            expect.append((batch, options, 1, names))
        elif options == "fixed times, min-snap, materialised blocks":   # the kernel after the assembly
            assert names[0].startswith("assemble_blocks") and len(names) == 2
            lines.append(request(n, S, uniform, fused=0))
            expect.append((batch, options, 1, names[1:]))
        elif options == "fixed times, min-snap, grouped dispatch of 10 batches":
            lines.append(request(n, S, uniform, group=10))
            expect.append((batch, options, 1, names))
        elif options in MELLINGER:
            lines += sr.closing_requests(n, S, uniform, d=MELLINGER[options])
            expect.append((batch, options, 2, [k for k in names if k.startswith("solve_")]))
    # every shape of the table with its two fixed-times and two Mellinger rows; the grouped row where scripts/routing_table.py
    # asks for it (up to 15 segments)
    shapes = {batch for batch, _, _ in _table_rows()}
    short = {batch for batch in shapes if _shape(batch)[1] <= 15}
    assert len(shapes) == 27 and len(short) == 19 and len(expect) == 4 * len(shapes) + len(short), (len(shapes), len(short), len(expect))
    got = sr.routes(harness, lines)
    at = 0
    for batch, options, count, names in expect:
        r = got[at:at + count]
        at += count
        told = [sr.kernel_name(r[0])] if count == 1 else sr.closing_names(*r)
        assert told == names, (batch, options, told, names, r)


# ---- both sides of every edge ----

def test_the_size_edges(harness):
    def fam(**kw):
        return _one(harness, **kw)["family"]

    # MRS_TG_QUAD_MIN_PATHS' default
    assert fam(n=6143, S=10) == "rows" and fam(n=6144, S=10) == "duo"
    assert fam(n=6144, S=10, store=0) == "rows"       # no factor store: the four- and eight-lane kernels are not asked
    assert fam(n=614, S=10, group=10) == "rows" and fam(n=615, S=10, group=10) == "duo"   # paths of the whole dispatch
    # the two-sided bound: fewer than 1.25 quad wavefronts (16 paths) per SIMD
    last = (5 * 256 - 1) * 16
    assert fam(n=last, S=10) == "duo" and fam(n=last + 1, S=10) == "quad"
    assert fam(n=last // 16, S=10, group=16) == "duo" and fam(n=last // 16 + 1, S=10, group=16) == "quad"
    # ... at 64 compute units it lies below the size from which the four-lane kernel is asked at all: rows on both sides, and the
    # four-lane kernel where 256 compute units take the two-sided one (the bound itself: test_every_routing_knob, with the
    # four-lane size lowered)
    last64 = (5 * 64 - 1) * 16
    assert fam(n=last64, S=10, cus=64) == "rows" and fam(n=last64 + 1, S=10, cus=64) == "rows"
    assert fam(n=6144, S=10, cus=64) == "quad" and fam(n=6144, S=10, cus=256) == "duo"
    # paths per wavefront of the rows kernel
    for n, shared, sampling, ppw, rides in [(2048, 0, 0, 1, 0), (2049, 0, 0, 2, 0), (2048, 1, 0, 2, 0), (2049, 1, 0, 2, 0),
                                            (2048, 0, 1, 1, 1), (2049, 0, 1, 2, 0), (2048, 1, 1, 1, 1), (2049, 1, 1, 2, 0)]:
        r = _one(harness, n=n, S=10, shared=shared, sampling=sampling)
        assert (r["family"], r["per_workgroup"], r["sampling"], r["with_tail"]) == ("rows", ppw, rides, rides), (n, shared, sampling, r)
        assert r["grid_x"] == -(-n // ppw) and r["threads"] == 64
    # grouped: by the paths of the whole dispatch
    for n, g, ppw in [(1024, 1, 1), (1025, 1, 2), (256, 4, 1), (205, 5, 2), (64, 16, 1), (65, 16, 2)]:
        r = _one(harness, n=n, S=10, group=g)
        assert (r["family"], r["per_workgroup"], r["blocks_per_batch"], r["grid_x"]) == ("rows", ppw, -(-n // ppw), -(-n // ppw) * g), r
    # the pipeline in one launch, and the sampling that rides on a closing rows launch
    for n, S, names, rides in [(1024, 10, ["solve_rows_pipeline_kernel"], 1), (1025, 10, ["solve_rows_kernel<0>", "solve_rows_kernel<1>"], 1),
                               (1, 32, ["solve_rows_pipeline_kernel"], 1), (1, 33, ["solve_rows_kernel<0>", "solve_rows_kernel<1>"], 1),
                               (2048, 10, ["solve_rows_kernel<0>", "solve_rows_kernel<1>"], 1),
                               (2049, 10, ["solve_rows_kernel<0>", "solve_rows_kernel<1>"], 0)]:
        first, final = sr.routes(harness, sr.closing_requests(n, S))
        assert sr.closing_names(first, final) == names and final["sampling"] == rides and final["scales"] == 1, (n, S, first, final)
        if final["maxima_in_launch"]:
            assert (final["threads"], final["grid_x"], final["per_workgroup"]) == (128, n, 1), final
    # without samples wanted, and for paths with a position-free vertex (every stage a launch of its own)
    first, final = sr.routes(harness, sr.closing_requests(1024, 10, samples=False))
    assert final["maxima_in_launch"] == 1 and final["sampling"] == 0
    first, final = sr.routes(harness, sr.closing_requests(1024, 10, general=True))
    assert (final["family"], final["scales"], final["maxima_in_launch"], final["sampling"], final["with_tail"]) == ("rows", 0, 0, 0, 0)
    # the lane kernel (paths too long for a tile): four lanes per path until one lane per path fills the machine
    for n, fused, lanes in [(32768, 1, 4), (32769, 1, 1), (32769, 0, 4)]:
        r = _one(harness, n=n, S=256, fused=fused)
        assert (r["family"], r["lanes_per_path"], r["grid_x"], r["lds_bytes"]) == ("lane", lanes, -(-n * lanes // 64), 0), r
    # the tile kernel: 32-bit byte offsets into the blocks (800 bytes per segment and path), and the ragged size limits
    edge = 0xFFFFFFFF // (800 * 10)
    assert fam(n=edge, S=10, fused=0) == "tile" and fam(n=edge + 1, S=10, fused=0) == "lane"
    assert fam(n=edge + 1, S=200) == "tile"          # (fused: no blocks to address)
    assert fam(n=4096, S=200, uniform=0) == "tile" and fam(n=4097, S=200, uniform=0) == "lane"
    assert fam(n=8192, S=30, uniform=0, fused=0) == "tile" and fam(n=8193, S=30, uniform=0, fused=0) == "lane"
    assert fam(n=8193, S=30, fused=0) == "tile"      # uniform batches: at every size


def test_the_instantiation_rules(harness):
    # the lean instantiation of the grouped two-sided kernel: one even length of at least 4, every wavefront full
    for n, S, uniform, lean in [(1024, 4, None, 1), (1024, 10, None, 1), (1024, 2, None, 0), (1024, 5, None, 0), (1024, 4, 0, 0),
                                (1020, 4, None, 0), (1016, 4, None, 1)]:
        r = _one(harness, n=n, S=S, uniform=uniform, group=10)
        assert (r["family"], r["lean"], r["loop_bits"]) == ("duo", lean, 3), (n, S, uniform, r)
        assert (r["grid_x"], r["grid_y"], r["blocks_per_batch"], r["per_workgroup"]) == (-(-n // 8), 10, -(-n // 8), 8), r
        assert sr.kernel_name(r) == "solve_duo_group_kernel<false>"
        assert sr.kernel_name(r, True) == ("solve_duo_group_kernel<false, true>" if lean else "solve_duo_group_kernel<false>")
    assert _one(harness, n=6144, S=4)["lean"] == 0   # (a single launch has no lean instantiation)
    # end vertices with free slots: objective orders below snap, or the constrained-slots hint
    for d, slots, wp, name in [(4, 0, 0, "solve_duo_kernel<false>"), (4, 0, 1, "solve_duo_kernel<true>"),
                               (3, 0, 0, "solve_quad_kernel<false, true>"), (2, 0, 1, "solve_quad_kernel<true, true>"),
                               (4, 1, 0, "solve_quad_kernel<false, true>")]:
        r = _one(harness, n=6144, S=2, d=d, slots=slots, wp=wp)
        assert sr.kernel_name(r) == name and r["ends"] == (d < 4 or slots), (d, slots, wp, r)
    for d, slots, name in [(4, 0, "solve_quad_group_kernel<false>"), (2, 0, "solve_quad_group_kernel<false, true>"),
                           (4, 1, "solve_quad_group_kernel<false, true>")]:
        r = _one(harness, n=4096, S=2, d=d, slots=slots, group=10)
        assert sr.kernel_name(r) == name and r["grid_x"] == 256 * 10 and r["blocks_per_batch"] == 256, r
    # a family forced by the request (the diagnostic programs), whatever the size rules say
    r = _one(harness, n=20000, S=10, force=FORCE_ROWS)
    assert (r["family"], r["per_workgroup"]) == ("rows", 2)
    r = _one(harness, n=20000, S=10, force=FORCE_ROWS, maxima=1, sampling=1)
    assert (r["family"], r["sampling"], r["scales"]) == ("rows_pipeline", 1, 1)
    r = _one(harness, n=1, S=3, force=FORCE_TILE)
    assert (r["family"], r["fused"]) == ("tile", 1)
    assert _one(harness, n=0, S=0)["family"] == "none" and _one(harness, n=0, S=0, group=4)["family"] == "none"


# ---- the LDS edges, by a sweep over the segment count ----

LENGTHS = range(1, 257)


def _sweep(harness, env=None, **kw):
    """the routes of the same request at every length, each checked: LDS within the family's budget and a compute unit's LDS,
    the limit raised exactly when the launch needs more than the default 64 KB, the grid covers the batch"""
    n, group = kw["n"], max(kw.get("group", 0), 1)
    out = sr.routes(harness, [request(S=S, **kw) for S in LENGTHS], env)
    for S, r in zip(LENGTHS, out):
        if r["family"] == "none":    # a grouped dispatch of paths too long for the grouped kernels: refused, nothing to launch
            assert "group" in kw and r["grid_x"] == 0
            continue
        assert r["budget"] == BUDGET[r["family"]] and r["lds_limit"] == LDS_LIMIT, (S, r)
        assert r["lds_bytes"] <= r["budget"] <= LDS_LIMIT, (S, r)
        if r["family"] == "tile":
            assert r["raise_lds_to"] == r["budget"], (S, r)     # (the tile kernel's limit is always set)
        else:
            assert r["raise_lds_to"] == (r["budget"] if r["lds_bytes"] > 64 * KB else 0), (S, r)
        assert r["grid_x"] * r["grid_y"] * r["per_workgroup"] >= n * group, (S, r)
        assert r["grid_y"] == (group if r["family"] == "duo" else 1), (S, r)
    return dict(zip(LENGTHS, out))


def _last(routes, pred):
    """the last length of the leading run that satisfies pred (the edge: pred holds up to it and fails right behind it)"""
    L = 0
    while L + 1 in routes and pred(routes[L + 1]):
        L += 1
    assert 1 <= L < max(LENGTHS), L
    assert not pred(routes[L + 1])
    return L


def test_the_lds_edges(harness):
    def forced(S, force, **kw):
        return _one(harness, n=1, S=S, force=force, **kw)

    # the rows kernel, plain: behind its last length the same record would not fit the budget
    plain = _sweep(harness, n=1)
    rows_last = _last(plain, lambda r: r["family"] == "rows")
    assert forced(rows_last, FORCE_ROWS)["lds_bytes"] <= BUDGET["rows"] < forced(rows_last + 1, FORCE_ROWS)["lds_bytes"]
    assert plain[rows_last + 1]["family"] == "tile"
    # ... with the sampling on its launch (the staging copy of times and coefficients and the sample buffer)
    sampled = _sweep(harness, n=1, sampling=1)
    ride_last = _last(sampled, lambda r: r["sampling"] == 1)
    assert ride_last < rows_last and sampled[ride_last + 1]["family"] == "rows" and sampled[ride_last + 1]["with_tail"] == 0
    assert forced(ride_last, FORCE_ROWS, sampling=1)["lds_bytes"] <= BUDGET["rows"] < forced(ride_last + 1, FORCE_ROWS, sampling=1)["lds_bytes"]
    # ... as the closing solve: the same edge for the sampling that rides; behind it the solve still scales
    closing = _sweep(harness, n=2048, stage=CLOSING, scale=1, maxima=1, sampling=1)
    assert _last(closing, lambda r: r["sampling"] == 1) == ride_last
    assert closing[ride_last + 1]["scales"] == 1 and closing[ride_last + 1]["with_tail"] == 1
    assert _last(closing, lambda r: r["family"] == "rows") == rows_last and closing[rows_last + 1]["scales"] == 0
    # ... two paths per wavefront: one path where two would not fit
    two = _sweep(harness, n=4096)
    two_last = _last(two, lambda r: r["family"] == "rows" and r["per_workgroup"] == 2)
    assert two[two_last + 1]["family"] == "rows" and two[two_last + 1]["per_workgroup"] == 1 and two[two_last + 1]["grid_x"] == 4096
    assert 2 * forced(two_last, FORCE_ROWS)["lds_bytes"] <= BUDGET["rows"] < 2 * forced(two_last + 1, FORCE_ROWS)["lds_bytes"]
    grouped = _sweep(harness, n=1024, group=4)
    assert _last(grouped, lambda r: r["per_workgroup"] == 2) == two_last
    assert _last(grouped, lambda r: r["family"] == "rows") == rows_last and grouped[rows_last + 1]["family"] == "none"
    # the pipeline in one launch: its length rule (32) comes before its LDS
    pipeline = _sweep(harness, n=1, stage=CLOSING, scale=1, maxima=1, sampling=1)
    assert _last(pipeline, lambda r: r["family"] == "rows_pipeline") == 32
    assert forced(33, FORCE_ROWS, maxima=1, sampling=1)["lds_bytes"] <= BUDGET["rows"]
    # the four- and eight-lane kernels: one length rule, the four-lane record store
    duo = _sweep(harness, n=6144)
    quad_last = _last(duo, lambda r: r["family"] == "duo")
    assert duo[quad_last + 1]["family"] == "rows"
    quad = _sweep(harness, n=65536)
    assert _last(quad, lambda r: r["family"] == "quad") == quad_last
    assert quad[quad_last]["lds_bytes"] >= duo[quad_last]["lds_bytes"]      # (the larger of the two decides)
    per_segment = quad[quad_last]["lds_bytes"] - quad[quad_last - 1]["lds_bytes"]
    assert quad[quad_last]["lds_bytes"] + per_segment > BUDGET["quad"]
    for g in (_sweep(harness, n=1024, group=10), _sweep(harness, n=4096, group=10)):
        assert _last(g, lambda r: r["family"] in ("duo", "quad")) == quad_last
    # ... the instantiation that eliminates end vertices: two more records per path, so it stops earlier
    ends = _sweep(harness, n=6144, d=2)
    ends_last = _last(ends, lambda r: r["family"] == "quad" and r["ends"] == 1)
    assert ends_last < quad_last and ends[ends_last + 1]["family"] == "quad" and ends[ends_last + 1]["ends"] == 0
    assert ends[ends_last]["lds_bytes"] + (ends[ends_last]["lds_bytes"] - ends[ends_last - 1]["lds_bytes"]) > BUDGET["quad"]
    assert _last(ends, lambda r: r["family"] == "quad") == quad_last
    # the tile kernel: from the blocks at every length it takes, fused behind the rows kernel
    blocks = _sweep(harness, n=1, fused=0)
    tile_last = _last(blocks, lambda r: r["family"] == "tile")
    assert blocks[tile_last + 1]["family"] == "lane" and blocks[tile_last + 1]["lanes_per_path"] == 4
    assert forced(tile_last, FORCE_TILE)["per_workgroup"] >= 1 and forced(tile_last + 1, FORCE_TILE)["per_workgroup"] == 0
    assert rows_last < tile_last and all(plain[S]["family"] == "tile" for S in range(rows_last + 1, tile_last + 1))
    assert plain[tile_last + 1]["family"] == "lane"
    # tile size: what fits, at most eight paths; from more than four, halved (rounding down) while that leaves fewer than 512 tiles
    def halved(tp, n):
        while tp > 4 and -(-n // tp) < 512:
            tp //= 2
        return tp

    many = _sweep(harness, n=8192, fused=0)
    for S in range(1, tile_last + 1):
        r = many[S]
        assert r["family"] == "tile" and 1 <= r["per_workgroup"] <= 8 and r["threads"] == 256, (S, r)
        assert r["lds_bytes"] % r["per_workgroup"] == 0
        assert r["per_workgroup"] == min(8, BUDGET["tile"] // (r["lds_bytes"] // r["per_workgroup"])), (S, r)
        assert blocks[S]["per_workgroup"] == halved(r["per_workgroup"], 1), (S, blocks[S])


# ---- every routing knob of the fixed-times section, at a non-default value ----

# a probe per route the knobs can touch; `only` below names the probes a knob may change, every other line must not move
PROBES = {
    "one": request(1, 3),
    "one_sampled": request(1, 3, sampling=1),
    "one_closing": request(1, 3, stage=CLOSING, scale=1, maxima=1, sampling=1),
    "rows_4096": request(4096, 10),
    "rows_1023": request(1023, 10),
    "rows_1024": request(1024, 10),
    "sampled_1024": request(1024, 10, sampling=1),
    "closing_1024": request(1024, 10, stage=CLOSING, scale=1, maxima=1, sampling=1),
    "duo_6144": request(6144, 10),
    "duo_6144_wp": request(6144, 10, wp=1),
    "quad_65536": request(65536, 10),
    "ends_6144": request(6144, 10, d=2),
    "group_lean": request(1024, 10, group=10),
    "group_quad": request(4096, 10, group=10),
    "group_rows": request(64, 10, group=4),
    "tile_100": request(100, 200),
    "tile_101": request(101, 200),
    "blocks_1": request(1, 3, fused=0),
    "last64": request((5 * 64 - 1) * 16, 10, cus=64),
    "last64_1": request((5 * 64 - 1) * 16 + 1, 10, cus=64),
}


def _probe(harness, env):
    return dict(zip(PROBES, sr.routes(harness, list(PROBES.values()), env)))


@pytest.fixture(scope="module")
def defaults(harness):
    assert not [k for k, _, _ in KNOBS if k in os.environ]   # (the harness inherits the environment of the test run)
    return _probe(harness, None)


def _fields(r, **kw):
    return all(r[k] == v for k, v in kw.items())


KNOBS = [
    # MRS_TG_ROWS_KERNEL=0: the tile and lane kernels instead of the rows kernel, and no grouped dispatch of batches that are
    # the rows kernel's (the pipeline's one launch is a kernel of its own and stays)
    ("MRS_TG_ROWS_KERNEL", "0", dict(
        one=dict(family="tile", fused=1), one_sampled=dict(family="tile", sampling=0), rows_4096=dict(family="tile"),
        rows_1023=dict(family="tile"), rows_1024=dict(family="tile"), sampled_1024=dict(family="tile", sampling=0),
        last64=dict(family="tile"), last64_1=dict(family="tile"), group_rows=dict(family="none", grid_x=0))),
    # MRS_TG_ROWS_PIPELINE=0: the closing stages as separate launches
    ("MRS_TG_ROWS_PIPELINE", "0", dict(
        one_closing=dict(family="rows", with_tail=1, scales=1, sampling=1, maxima_in_launch=0, threads=64),
        closing_1024=dict(family="rows", with_tail=1, scales=1, sampling=1, maxima_in_launch=0, threads=64))),
    # MRS_TG_ROWS_PPW: paths per wavefront of the rows kernel, single and grouped (the pipeline keeps its one path)
    ("MRS_TG_ROWS_PPW", "2", dict(
        one=dict(per_workgroup=2, grid_x=1), one_sampled=dict(per_workgroup=2, grid_x=1, sampling=1), rows_1023=dict(per_workgroup=2, grid_x=512),
        rows_1024=dict(per_workgroup=2, grid_x=512), sampled_1024=dict(per_workgroup=2, grid_x=512, sampling=1),
        group_rows=dict(per_workgroup=2, blocks_per_batch=32, grid_x=128))),
    ("MRS_TG_ROWS_PPW", "1", dict(rows_4096=dict(per_workgroup=1, grid_x=4096), last64=dict(per_workgroup=1), last64_1=dict(per_workgroup=1))),
    # MRS_TG_QUAD_MIN_PATHS=1024: the four- and eight-lane kernels from 1024 paths per launch on.  The two precedence orders part
    # here: a fixed-times solve that samples keeps the rows kernel and its sampling, a closing solve goes to the eight-lane
    # kernel with the scaling and leaves the sampling to the sampler -- and the pipeline's one launch is not taken
    ("MRS_TG_QUAD_MIN_PATHS", "1024", dict(
        rows_4096=dict(family="duo"), rows_1024=dict(family="duo"),   # (sampled_1024: as by default, rows with its sampling)
        closing_1024=dict(family="duo", scales=1, sampling=0, maxima_in_launch=0, with_tail=1),
        last64=dict(family="duo"), last64_1=dict(family="quad"))),   # the two-sided bound at 64 compute units
    # MRS_TG_QUAD_ENDS=0: no instantiation that eliminates end vertices
    ("MRS_TG_QUAD_ENDS", "0", dict(ends_6144=dict(family="quad", ends=0))),
    # MRS_TG_DUO=0 never, =1 whenever the pattern allows (min-snap, fully constrained ends)
    ("MRS_TG_DUO", "0", dict(duo_6144=dict(family="quad", ends=0, wp=0), duo_6144_wp=dict(family="quad", ends=0, wp=1),
                              group_lean=dict(family="quad", lean=0, grid_x=640, grid_y=1))),
    ("MRS_TG_DUO", "1", dict(quad_65536=dict(family="duo", grid_x=8192), group_quad=dict(family="duo", lean=1, grid_x=512, grid_y=10))),
    # the two loop bits and the lean instantiation, which needs both
    ("MRS_TG_DUO_UNIFORM", "0", dict(duo_6144=dict(loop_bits=2), duo_6144_wp=dict(loop_bits=2), group_lean=dict(loop_bits=2, lean=0))),
    ("MRS_TG_DUO_STORE_THROUGH", "0", dict(duo_6144=dict(loop_bits=1), duo_6144_wp=dict(loop_bits=1), group_lean=dict(loop_bits=1, lean=0))),
    ("MRS_TG_DUO_LEAN", "0", dict(group_lean=dict(loop_bits=3, lean=0))),
    # MRS_TG_TRACE_INSTANTIATIONS: how the launcher spells a name, no route changes
    ("MRS_TG_TRACE_INSTANTIATIONS", "1", dict()),
    # MRS_TG_TILE_MAX_PATHS: the largest batch the tile kernel takes
    ("MRS_TG_TILE_MAX_PATHS", "100", dict(tile_101=dict(family="lane", lanes_per_path=4))),
    ("MRS_TG_TILE_MAX_PATHS", "0", dict(tile_100=dict(family="lane"), tile_101=dict(family="lane"), blocks_1=dict(family="lane", lanes_per_path=4, fused=0))),
]


def test_the_knobs_are_the_section_of_the_header():
    """every knob of the section "routing of the fixed-times solve" is in KNOBS, and no other"""
    with open(os.path.join(hh.ROOT, "mrs_uav_trajectory_generation_amd", "csrc", "mrs_tg_knobs.hpp")) as f:
        text = f.read()
    section = text.split("// ---- routing of the fixed-times solve ----")[1].split("// ---- routing of the nonlinear pipeline ----")[0]
    assert set(re.findall(r'env_\w+\("(MRS_TG_\w+)"', section)) == {k for k, _, _ in KNOBS}


@pytest.mark.parametrize("knob,value,only", KNOBS, ids=["%s=%s" % (k, v) for k, v, _ in KNOBS])
def test_every_routing_knob(harness, defaults, knob, value, only):
    got = _probe(harness, {knob: value})
    for name, r in got.items():
        if name in only:
            assert r != defaults[name] and _fields(r, **only[name]), (name, r, defaults[name])
        else:
            assert r == defaults[name], (name, r, defaults[name])


def test_the_probes_by_default(defaults):
    want = dict(one="solve_rows_kernel<0>", one_sampled="solve_rows_kernel<1>", one_closing="solve_rows_pipeline_kernel",
                rows_4096="solve_rows_kernel<0>", rows_1023="solve_rows_kernel<0>", rows_1024="solve_rows_kernel<0>",
                sampled_1024="solve_rows_kernel<1>", closing_1024="solve_rows_pipeline_kernel", duo_6144="solve_duo_kernel<false>",
                duo_6144_wp="solve_duo_kernel<true>", quad_65536="solve_quad_kernel<false>", ends_6144="solve_quad_kernel<false, true>",
                group_lean="solve_duo_group_kernel<false>", group_quad="solve_quad_group_kernel<false>", group_rows="solve_rows_group_kernel",
                tile_100="solve_tile_kernel<true>", tile_101="solve_tile_kernel<true>", blocks_1="solve_tile_kernel<false>",
                last64="solve_rows_kernel<0>", last64_1="solve_rows_kernel<0>")
    assert {k: sr.kernel_name(r) for k, r in defaults.items()} == want
    assert defaults["group_lean"]["lean"] == 1 and defaults["group_lean"]["loop_bits"] == 3 and defaults["duo_6144"]["loop_bits"] == 3


# ---- the same lines under AddressSanitizer + UndefinedBehaviorSanitizer ----

def test_the_sanitizer_build_prints_the_same(harness, tmp_path):
    san = sr.build(tmp_path, sanitize=True)
    lines = list(PROBES.values())
    for kw in (dict(n=1), dict(n=1, fused=0), dict(n=6144, d=2), dict(n=4096, group=10), dict(n=1, stage=CLOSING, scale=1, maxima=1, sampling=1)):
        lines += [request(S=S, **kw) for S in LENGTHS]
    lines += [request(1, 300, force=FORCE_TILE), request(1, 300, force=FORCE_ROWS, maxima=1, sampling=1), request(0, 0), request(0, 0, group=16),
              request(2 ** 31 - 1, 256), request(2 ** 31 - 1, 256, fused=0), request(2 ** 27, 10, group=16)]
    for env in (None, {"MRS_TG_QUAD_MIN_PATHS": "1024", "MRS_TG_ROWS_PPW": "2", "MRS_TG_DUO": "1"}):
        assert hh.run(san, lines, len(lines), env=env) == hh.run(harness, lines, len(lines), env=env)
