"""The route of the Mellinger outer loop on the CPU: csrc/mrs_tg_nonlinear_route.hpp (LDS footprints, the lane-group bins of a
plan, the predicates, route_nonlinear) compiled by g++ into tests/host/nonlinear_route_harness.cpp.  Checked here: every
Mellinger row of the committed routing table -- the whole launch list, not only the closing solves --, both sides of every edge
the header draws (group widths and LDS edges found by a sweep over the segment count and held to a plain restatement), every
knob of the nonlinear section of mrs_tg_knobs.hpp at a non-default value, the round-6 advisor's moving-start finding as it
stands today, and the same lines through an AddressSanitizer + UndefinedBehaviorSanitizer build.  No GPU."""
import os
import re

import pytest

from mrs_uav_trajectory_generation_amd import problem as pr
from tests import host_harness as hh
from tests import nonlinear_route_util as nr
from tests.nonlinear_route_util import request

KB = 1024
LDS_LIMIT, LDS_DEFAULT = 160 * KB, 64 * KB   # a compute unit's LDS; what a launch may ask for without raising the kernel's limit
RAGGED = [pr.ragged_segment_count(p) for p in range(8192)]   # the lengths of pr.random_batch(8192, "ragged", seed0=0), path by path


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return nr.build(tmp_path_factory.mktemp("nonlinear_route"))


def _one(harness, batch, env=None, **kw):
    return nr.routes(harness, [request(batch, **kw)], env)[0]


# ---- the committed table ----

TABLE = os.path.join(hh.ROOT, "profiles", "launch_layer_routing_table.md")
MELLINGER = {"Mellinger + sampling, min-snap": dict(d=4),
             "Mellinger + sampling, min-acceleration (the nodelet's default)": dict(d=2),
             "Mellinger + sampling, min-snap, stop_at / moving-start hint": dict(d=4, slots=1)}


def _batch(text):
    m = re.match(r"(\d+) x (\d+)", text)
    if m:
        return int(m.group(1)), int(m.group(2))
    assert re.match(r"8192 ragged 3\.\.30", text), text
    return RAGGED


def test_the_committed_routing_table(harness):
    """the table was printed on 256 compute units; a row ends on the sampler where the closing launch does not sample --
    plan_solve's launch, not launch_nonlinear's"""
    lines, expect = [], []
    with open(TABLE) as f:
        for line in f.read().splitlines()[2:]:
            batch, options, kernels = [c.strip() for c in line.strip().strip("|").split("|")]
            if options in MELLINGER:
                items = kernels.split(" → ")
                lines.append(request(_batch(batch), cus=256, **MELLINGER[options]))
                expect.append((batch, options, items[:-1] if items[-1] == "`sample_kernel<NDER>`" else items, items[-1]))
    assert len(expect) == 3 * 27, len(expect)
    assert sum(options.startswith("Mellinger + sampling, min-snap, stop_at") for _, options, _, _ in expect) == 27
    for (batch, options, items, last), r in zip(expect, nr.routes(harness, lines)):
        assert nr.compress(nr.kernel_names(r)) == items, (batch, options, nr.kernel_names(r), items)
        assert (last == "`sample_kernel<NDER>`") == (not r["tail_samples"]), (batch, options, r)


# ---- both sides of every edge ----

def test_the_dimension_split_and_the_regroup_rule(harness):
    def split(n, S, **kw):
        r = _one(harness, (n, S), **kw)
        return r["plan_dim_split"], r["dim_split"]

    for S in (1, 10, 12):
        assert split(2560, S) == (4, 4) and split(2561, S) == (1, 1), S
    for S in (13, 14, 15):
        assert split(1536, S) == (4, 4) and split(1537, S) == (1, 1), S
    assert split(1, 15) == (4, 4) and split(1, 16) == (1, 1)
    # the call goes back to lane groups at 13 to 15 segments for each of three reasons, and for none of them does not
    for S in (13, 14, 15):
        assert split(1024, S) == (4, 4)
        for why in (dict(d=3), dict(d=2), dict(slots=1), dict(moving=1)):
            assert split(1024, S, **why) == (4, 1), (S, why)
            assert split(1024, S, env={"MRS_TG_REGROUP": "0"}, **why) == (4, 4), (S, why)
    for why in (dict(d=2), dict(slots=1), dict(moving=1)):
        assert split(1024, 12, **why) == (4, 4) and split(1024, 16, **why) == (1, 1)
        assert _one(harness, (1024, 12), **why)["regroup_possible"] == 0 and _one(harness, (1024, 16), **why)["regroup_possible"] == 0
    assert _one(harness, (1024, 13))["regroup_possible"] == 1 and _one(harness, (1537, 13))["regroup_possible"] == 0
    # the shared-device hint is not the outer loop's
    assert split(1024, 14, shared=1) == (4, 4)


def _pow2ceil(x):
    return 1 << (x - 1).bit_length()


def _group_for(S, ds):      # lanes for the S + 1 time vectors, ds lanes each: a power of two from 4 to 64
    return min(64, max(4, _pow2ceil((S + 1) * ds)))


def _group_for_wide(S):     # from 13 segments on, the S + 4 lanes of the shared half sweeps
    return min(64, _pow2ceil(S + 4)) if S >= 13 else _group_for(S, 1)


def _group_for_ends(S, min_segments=2):   # every path of min_segments or more in S + 4 lanes, a wavefront in two passes up to 121
    if S < min_segments:
        return _group_for(S, 1)
    if S + 4 > 64:
        return 64 if S <= 121 else None
    return max(8, _pow2ceil(S + 4))


def _changes(width):
    """the lengths at which a width differs from the width one segment below"""
    return [S for S in sorted(width)[1:] if width[S] != width[S - 1]]


def test_the_group_widths(harness):
    lengths = range(1, 257)
    # lane groups (4096 paths: no dimension split at any length)
    got = nr.routes(harness, [request((4096, S)) for S in lengths])
    plain, wide, ends = {}, {}, {}
    for S, r in zip(lengths, got):
        assert r["plan_dim_split"] == 1 and len(r["bins"]) == 1 and len(r["wide_bins"]) == 1 and len(r["ends_bins"]) <= 1, (S, r)
        assert r["bins"][0][1:] == (0, 4096, S, S) and r["wide_bins"][0][1:] == (0, 4096, S, S), (S, r)
        plain[S], wide[S], ends[S] = r["bins"][0][0], r["wide_bins"][0][0], r["ends_bins"][0][0] if r["ends_bins"] else None
        assert r["wide_blocks"] == -(-4096 // (64 // wide[S])), (S, r)
    assert plain == {S: _group_for(S, 1) for S in lengths}
    assert wide == {S: _group_for_wide(S) for S in lengths}
    assert ends == {S: _group_for_ends(S) for S in lengths}
    assert _changes(plain) == [4, 8, 16, 32]
    assert _changes(wide) == [4, 8, 13, 29]
    assert _changes(ends) == [2, 5, 13, 29, 122]      # (61: a wavefront per path already, in two passes -- the kernel changes, below)
    # one lane per dimension (one path: the split at every length that has it)
    got = nr.routes(harness, [request((1, S)) for S in range(1, 16)])
    four = {S: r["bins"][0][0] for S, r in zip(range(1, 16), got)}
    for S, r in zip(range(1, 16), got):     # (the lane-group bins beside them only where a call may regroup)
        assert r["plan_dim_split"] == 4 and r["regroup_possible"] == (S >= 13), (S, r)
        assert (len(r["bins1"]), len(r["wide_bins"]), len(r["ends_bins"])) == ((1, 1, 1) if S >= 13 else (0, 0, 0)), (S, r)
    assert four == {S: _group_for(S, 4) for S in range(1, 16)} and _changes(four) == [2, 4, 8]
    # MRS_TG_ENDS_MIN_SEGMENTS (read once: a process of its own)
    got = nr.routes(harness, [request((4096, S)) for S in range(1, 9)], {"MRS_TG_ENDS_MIN_SEGMENTS": "4"})
    assert [r["ends_bins"][0][0] for r in got] == [_group_for_ends(S, 4) for S in range(1, 9)] == [4, 4, 4, 8, 16, 16, 16, 16]
    # the lean kernel by length, one path: shared half sweeps from 16 segments (below: the dimension split), in two passes from 61,
    # one-sided sweeps past 121; objective orders below snap regroup at 13 to 15 segments and take the free-end kernels
    snap = nr.routes(harness, [request((1, S)) for S in lengths])
    accel = nr.routes(harness, [request((1, S), d=2) for S in lengths])
    for S, a, b in zip(lengths, snap, accel):
        want = None if S <= 15 else "lean_shared" if S <= 60 else "lean_shared_ends_long" if S <= 121 else "lean"
        assert (a["lean_kernel"] if a["lean"] else None) == want, (S, a)
        want = None if S <= 12 else "lean_shared_ends" if S <= 60 else "lean_shared_ends_long" if S <= 121 else "lean_masked"
        assert (b["lean_kernel"] if b["lean"] else None) == want, (S, b)
        assert a["sweep_kernel"] == ("wave" if S <= 12 else "split" if S <= 15 else "compact"), (S, a)
        assert b["sweep_kernel"] == ("wave" if S <= 12 else "compact_masked"), (S, b)


def test_the_bin_limit(harness):
    """a launch's table holds five bins.  No batch gives nonlinear_host_plan more (there are five group widths), so the bins are
    given: with six the lean kernel is off and the sweeping launch does not fit -- the call is refused"""
    five, six = [60] * 2 + [50] * 2 + [40] * 2 + [30] * 2 + [20] * 2, [60] * 2 + [50] * 2 + [40] * 2 + [30] * 2 + [20] * 2 + [10] * 2
    a, b = _one(harness, five, as_bins=True), _one(harness, six, as_bins=True)
    assert len(a["bins"]) == 5 and (a["lean"], a["sweep_fits"]) == (1, 1) and len(a["lean_bins"]) == 5 and len(a["sweep_bins"]) == 5
    assert nr.outer_names(a) == ["optimize_lean_shared_kernel", "optimize_compact_kernel<false>"]
    assert len(b["bins"]) == 6 and (b["lean"], b["sweep_fits"]) == (0, 0) and nr.kernel_names(b) is None
    # the widest batch a plan builds: five bins, both launches
    r = _one(harness, [40] * 3 + [20] * 3 + [10] * 3 + [5] * 3 + [1] * 3)
    assert [b[0] for b in r["bins"]] == [64, 32, 16, 8, 4] and (r["lean"], r["sweep_fits"]) == (1, 1)
    assert [b[4] for b in r["sweep_bins"]] == [0, 3, 5, 6, 7] and r["sweep_blocks"] == 8    # block_begin: 1, 2, 4, 8, 16 paths per block


def test_the_wide_group_bound(harness):
    """wide groups while the launch over them has at most 8 blocks per resident wavefront (4 SIMDs x MRS_TG_LEAN_WAVES = 2 per
    compute unit): 14 segments, 32 lanes wide against 16 narrow, two paths per block"""
    for cus in (64, 256):
        last = 2 * 8 * cus * 4 * 2
        a, b = _one(harness, (last, 14), cus=cus), _one(harness, (last + 1, 14), cus=cus)
        assert a["wide_blocks"] == 8 * cus * 8 and b["wide_blocks"] == a["wide_blocks"] + 1
        assert (a["lean_bins"][0][0], a["lean_kernel"]) == (32, "lean_shared") and (b["lean_bins"][0][0], b["lean_kernel"]) == (16, "lean"), (a, b)
    assert _one(harness, (2 * 8 * 64 * 8 + 1, 14), cus=256)["lean_bins"][0][0] == 32      # (the bound is the device's)


def test_the_path_queue(harness):
    """one bin and more blocks than the caller's resident figure: the launch is what is resident, the rest is claimed"""
    for resident in (2048, 512, 7):      # (20 segments: lane groups at every size, two paths per block)
        a, b = _one(harness, (2 * resident, 20), resident=resident), _one(harness, (2 * resident + 1, 20), resident=resident)
        assert (a["queued"], a["lean_blocks"]) == (0, resident) and (b["queued"], b["lean_blocks"]) == (1, resident), (a, b)
        assert nr.outer_names(b)[0] == "set_queue_kernel" and nr.outer_names(a)[0] != "set_queue_kernel"
        assert b["sweep_blocks"] == resident + 1      # (the sweeping launch behind it is never queued)
    assert _one(harness, (65536, 10), resident=0)["queued"] == 0 and _one(harness, (65536, 10), resident=0)["lean_blocks"] == 16384
    two = _one(harness, [20] * 8192 + [10] * 8192, resident=2048)     # two bins: never queued
    assert len(two["lean_bins"]) == 2 and two["queued"] == 0 and two["lean_blocks"] == 4096 + 2048
    # the figure is the caller's: the knob is the launcher's to read, the header does not
    assert _one(harness, (65536, 10), env={"MRS_TG_LEAN_RESIDENT_BLOCKS": "0"})["queued"] == 1


def test_the_pair_launch(harness):
    """128 threads -- a partner wavefront per path -- only when every bin's group is 64 under the dimension split"""
    pair_bytes = (64 * 16 + 2) * 8     # the hand-over area of 16 doubles per lane, and the flags
    for S in (13, 14, 15):
        r = _one(harness, (1, S))
        assert (r["sweep_kernel"], r["sweep_threads"], r["sweep_bins"][0][0]) == ("split", 128, 64), r
        mixed = _one(harness, [S, 7])        # a second bin of 32 lanes: one wavefront per block
        assert (mixed["sweep_kernel"], mixed["sweep_threads"], [b[0] for b in mixed["sweep_bins"]]) == ("split", 64, [64, 32]), mixed
        assert r["sweep_lds"] == _sweep_bytes(64, S, True) + pair_bytes
        assert mixed["sweep_lds"] == max(_sweep_bytes(64, S, True), _sweep_bytes(32, 7, True))
    env = {"MRS_TG_WAVE_KERNEL": "0"}       # (up to 12 segments the wave kernel stands in front of the split kernel)
    assert [(_one(harness, (1, S), env)["sweep_threads"], _one(harness, (1, S), env)["sweep_bins"][0][0]) for S in (6, 7, 8, 12)] == \
        [(64, 32), (64, 32), (128, 64), (128, 64)]
    assert _one(harness, (1, 16))["sweep_threads"] == 64 and _one(harness, (4, 200))["sweep_threads"] == 64     # (lane groups: never)


# ---- the LDS formulas, by a sweep over the segment count ----

def _lean_bytes(group, S):          # per group x, g, xn, gn, dir, s[5], y[5] | rho[6] | tick state 5 | dp 4 S | staging 4 (S + 1) |
    return ((64 // group) * (15 * S + 6 + 5 + 4 * S + 4 * (S + 1) + 84 + 18) + 2 * 45) * 8     # hand-over 84 | moving start 18; 2 tables


def _group_doubles(S, extras):      # the same vectors | rho | tick state | vertices 22 (S + 1) | moving-start extras 160 | segments 38 S
    return 15 * S + 6 + 5 + 22 * (S + 1) + (160 if extras else 0) + 38 * S


def _sweep_bytes(group, S, split):
    return ((64 // group) * _group_doubles(S, split) + 36) * 8        # + the block constants


def _gradient_bytes(group, S, split):                                   # x, g | vertices | extras | segments; + the block constants
    return ((64 // group) * (2 * S + 22 * (S + 1) + (160 if split else 0) + 38 * S) + 36) * 8


def _first(pred, lengths):
    return next(S for S in lengths if pred(S))


def test_the_lds_edges(harness):
    lengths = range(1, 1025)
    got = dict(zip(lengths, nr.routes(harness, [request((1, S)) for S in lengths])))
    for S, r in got.items():
        split = r["dim_split"] == 4
        assert (r["lds_limit"], r["lds_default"]) == (LDS_LIMIT, LDS_DEFAULT)
        assert r["listed_lds"] == (_group_doubles(S, True) + 36) * 8, (S, r)
        assert r["gradient_lds"] == _gradient_bytes(r["bins"][0][0], S, r["plan_dim_split"] == 4), (S, r)
        if r["lean"]:
            assert r["lean_lds"] == _lean_bytes(r["lean_bins"][0][0], S) <= LDS_LIMIT, (S, r)
        if not r["wave"]:
            assert r["sweep_lds"] == _sweep_bytes(r["sweep_bins"][0][0], S, split) + ((64 * 16 + 2) * 8 if r["sweep_threads"] == 128 else 0), (S, r)
        assert r["sweep_fits"] == (r["sweep_lds"] <= LDS_LIMIT), (S, r)
    long = range(64, 1025)       # (a wavefront per path from 63 segments on: the formulas grow with every segment)
    # the sweeping launch: past 64 KB the launcher raises the kernel's limit, past 160 KB the call is refused
    s64, s160 = (_first(lambda S: _sweep_bytes(64, S, False) > lim, long) for lim in (LDS_DEFAULT, LDS_LIMIT))
    assert (s64, s160) == (109, 273)
    assert got[s64 - 1]["sweep_lds"] <= LDS_DEFAULT < got[s64]["sweep_lds"]
    assert got[s160 - 1]["sweep_fits"] == 1 and got[s160]["sweep_fits"] == 0 and all(got[S]["sweep_fits"] == 0 for S in range(s160, 1025))
    assert nr.kernel_names(got[s160 - 1]) is not None and nr.kernel_names(got[s160]) is None
    # the lean launch: past 160 KB it is not made (the sweeping launch has refused long before)
    l64, l160 = (_first(lambda S: _lean_bytes(64, S) > lim, long) for lim in (LDS_DEFAULT, LDS_LIMIT))
    assert (l64, l160) == (348, 882)
    assert got[l64 - 1]["lean_lds"] <= LDS_DEFAULT < got[l64]["lean_lds"]
    assert got[l160 - 1]["lean"] == 1 and all(got[S]["lean"] == 0 and got[S]["lean_lds"] == 0 for S in range(l160, 1025))
    # the gradient's launches and the kernels that take one listed path per workgroup
    g64, g160 = (_first(lambda S: _gradient_bytes(64, S, False) > lim, long) for lim in (LDS_DEFAULT, LDS_LIMIT))
    assert (g64, g160) == (132, 330)
    assert got[g64 - 1]["gradient_lds"] <= LDS_DEFAULT < got[g64]["gradient_lds"] and got[g160 - 1]["gradient_lds"] <= LDS_LIMIT < got[g160]["gradient_lds"]
    c64, c160 = (_first(lambda S: (_group_doubles(S, True) + 36) * 8 > lim, long) for lim in (LDS_DEFAULT, LDS_LIMIT))
    assert (c64, c160) == (107, 271)
    assert got[c64 - 1]["listed_lds"] <= LDS_DEFAULT < got[c64]["listed_lds"] and got[c160 - 1]["listed_lds"] <= LDS_LIMIT < got[c160]["listed_lds"]
    # several groups per wavefront: the widest launch of the lane groups, four paths of 15 segments in groups of 16
    r = _one(harness, (4096, 15))
    assert r["sweep_lds"] == _sweep_bytes(16, 15, False) and r["lean_lds"] == _lean_bytes(32, 15) and r["gradient_lds"] == _gradient_bytes(16, 15, False)


# ---- the flags of a call, and the closing ----

def test_the_flags_of_a_call(harness):
    base = _one(harness, (4096, 10))
    assert (base["estimate_in_kernel"], base["careful"], base["general"], base["closing"], base["tail_samples"]) == (1, 0, 0, "rows_tail", 0)
    assert _one(harness, (4096, 10), estimate=0)["estimate_in_kernel"] == 0
    assert nr.kernel_names(_one(harness, (4096, 10), estimate=0), estimate=False) == nr.kernel_names(base)
    for kw in (dict(careful=1), dict(general=1)):       # kernels that start from a copy of the times: the estimate is a launch in front
        r = _one(harness, (4096, 10), **kw)
        assert r["estimate_in_kernel"] == 0 and (r["careful"], r["general"]) == (kw.get("careful", 0), kw.get("general", 0))
        assert (r["lean_kernel"], r["sweep_kernel"], r["lean_bins"], r["sweep_bins"]) == \
            (base["lean_kernel"], base["sweep_kernel"], base["lean_bins"], base["sweep_bins"])
    r = _one(harness, (4096, 10), general=1)             # position-free paths: every closing stage a launch of its own
    assert (r["closing"], r["tail_samples"], r["final"]["scales"], r["final"]["maxima_in_launch"]) == ("separate", 0, 0, 0)
    assert _one(harness, (1, 33))["tail_samples"] == 1 and _one(harness, (1, 33), samples=0)["tail_samples"] == 0    # (few paths: it rides)
    assert [_one(harness, b)["closing"] for b in ((1024, 10), (1025, 10), (6144, 10), (4, 200))] == \
        ["rows_pipeline", "rows_tail", "quad_tail", "separate"]
    assert nr.kernel_names(_one(harness, (4, 200)), reference_status=True)[-3:] == \
        ["segment_maxima_scaling_kernel", "apply_scaling_kernel", "solve_tile_kernel<true>"]
    # the closing solves route by the compute units their request carries, the outer loop by the device's
    a, b = _one(harness, (8192, 14), cus=64, solve_cus=256), _one(harness, (8192, 14), cus=256, solve_cus=64)
    assert (a["lean_bins"][0][0], a["first"]["family"]) == (32, "duo") and (b["lean_bins"][0][0], b["first"]["family"]) == (32, "quad")
    assert _one(harness, (8193, 14), cus=64, solve_cus=256)["lean_bins"][0][0] == 16


# ---- the round-6 advisor's third finding ----

def test_the_moving_start_hint_changes_the_route_at_13_to_15_segments(harness):
    """The host policy route sees a moving start and says so; the device policy route cannot and never does.  Recorded as it
    stands: 1024 x 14 under min-snap takes the split kernel without the hint, and with it goes back to lane groups -- a lean
    kernel with the compact kernel behind it.  (With the hint alone the lean kernel is the one with only the shared half sweeps;
    the free-end kernel is what the constrained-slots hint adds.)"""
    without, with_hint = _one(harness, (1024, 14)), _one(harness, (1024, 14), moving=1)
    assert nr.outer_names(without) == ["optimize_split_kernel"]
    assert nr.outer_names(with_hint) == ["optimize_lean_shared_kernel", "optimize_compact_kernel<false>"]
    assert nr.outer_names(_one(harness, (1024, 14), slots=1)) == ["optimize_lean_shared_ends_kernel", "optimize_compact_kernel<false>"]
    assert nr.outer_names(_one(harness, (1024, 14), slots=1, moving=1)) == ["optimize_lean_shared_ends_kernel", "optimize_compact_kernel<false>"]
    assert without["first"] == with_hint["first"] and without["final"] == with_hint["final"]     # (the closing solves do not read it)
    for S in (12, 16):
        assert nr.kernel_names(_one(harness, (1024, S))) == nr.kernel_names(_one(harness, (1024, S), moving=1))


# ---- every knob of the nonlinear section, at a non-default value ----

SHORT = [30] * 100 + [3] * 100 + [2] * 100
# a probe per route the knobs can touch; `only` below names the probes a knob may change, every other line must not move
PROBES = {
    "one": request((1, 3)),
    "wave_1024": request((1024, 10)),
    "wave_2560": request((2560, 10)),
    "split_14": request((1024, 14)),
    "regroup_d2": request((1024, 14), d=2),
    "regroup_moving": request((1024, 14), moving=1),
    "lean_4096": request((4096, 10)),
    "ends_4096": request((4096, 10), d=2),
    "slots_4096": request((4096, 10), slots=1),
    "ragged": request(RAGGED),
    "ragged_d2": request(RAGGED, d=2),
    "short_d2": request(SHORT, d=2),
    "queued": request((65536, 10)),
    "long_80": request((1, 80)),
    "lean_200": request((4, 200)),
    "masked_200": request((4, 200), d=2),
    "wide_14": request((8192, 14)),
    "narrow_14": request((65536, 14)),
}
_GROUPS = ["regroup_d2", "regroup_moving", "lean_4096", "ends_4096", "slots_4096", "ragged", "ragged_d2", "short_d2", "queued", "long_80",
           "lean_200", "masked_200", "wide_14", "narrow_14"]      # the probes that run lane groups, and so a lean kernel


def _probe(harness, env):
    return dict(zip(PROBES, nr.routes(harness, list(PROBES.values()), env)))


@pytest.fixture(scope="module")
def defaults(harness):
    assert not [k for k, _, _ in KNOBS if k in os.environ]   # (the harness inherits the environment of the test run)
    return _probe(harness, None)


def _fields(r, **kw):
    return all(r[k] == v for k, v in kw.items())


KNOBS = [
    # MRS_TG_DIM_SPLIT_MAX_PATHS=0: no plan splits the dimensions -- lane groups and the lean kernels at every size (the probes that
    # regroup run what they ran, on a plan that has nothing to go back from)
    ("MRS_TG_DIM_SPLIT_MAX_PATHS", "0", dict(
        one=dict(plan_dim_split=1, lean=1, lean_kernel="lean_shared", sweep_kernel="compact"),
        wave_1024=dict(plan_dim_split=1, lean=1, lean_kernel="lean_shared", sweep_kernel="compact"),
        wave_2560=dict(plan_dim_split=1, lean=1, lean_kernel="lean_shared", sweep_kernel="compact"),
        split_14=dict(plan_dim_split=1, regroup_possible=0, lean=1, lean_kernel="lean_shared", sweep_kernel="compact", sweep_threads=64),
        regroup_d2=dict(plan_dim_split=1, regroup_possible=0, dim_split=1, lean_kernel="lean_shared_ends", sweep_kernel="compact_masked"),
        regroup_moving=dict(plan_dim_split=1, regroup_possible=0, dim_split=1, lean_kernel="lean_shared", sweep_kernel="compact"))),
    # MRS_TG_ENDS_MIN_SEGMENTS=4: paths of 2 and 3 segments keep their narrow groups in the free-end bins -- a fifth bin; the
    # min-snap launch over those bins no longer holds shared half sweeps only
    ("MRS_TG_ENDS_MIN_SEGMENTS", "4", dict(
        ragged=dict(lean_kernel="lean", lean_blocks=3586), ragged_d2=dict(lean_kernel="lean_shared_ends", lean_blocks=3586),
        short_d2=dict(lean_kernel="lean_shared_ends", lean_blocks=113))),
    # MRS_TG_LEAN=0: the sweeping kernel alone; =1: a lean kernel in front of the split kernel too (and in front of it the wave
    # kernel is not asked)
    ("MRS_TG_LEAN", "0", {k: dict(lean=0, lean_blocks=0, queued=0) for k in _GROUPS}),
    ("MRS_TG_LEAN", "1", dict(
        one=dict(lean=1, lean_kernel="lean_shared", wave=0, sweep_kernel="split", sweep_threads=64),
        wave_1024=dict(lean=1, lean_kernel="lean_shared", wave=0, sweep_kernel="split", sweep_threads=128),
        wave_2560=dict(lean=1, lean_kernel="lean_shared", queued=1, wave=0, sweep_kernel="split", sweep_threads=128),
        split_14=dict(lean=1, lean_kernel="lean_shared", sweep_kernel="split", sweep_threads=128))),
    # MRS_TG_LEAN_SHARED=0: one-sided sweeps only -- no wide groups, no free-end kernels; =1 differs from the default 2 inside the
    # mixed kernel alone (NonlinearParams::lean_shared), no route moves
    ("MRS_TG_LEAN_SHARED", "0", dict(
        regroup_d2=dict(lean_kernel="lean_masked"), regroup_moving=dict(lean_kernel="lean"), lean_4096=dict(lean_kernel="lean"),
        ends_4096=dict(lean_kernel="lean_masked"), slots_4096=dict(lean_kernel="lean"), ragged=dict(lean_kernel="lean"),
        ragged_d2=dict(lean_kernel="lean_masked"), short_d2=dict(lean_kernel="lean_masked"), queued=dict(lean_kernel="lean", queued=1),
        long_80=dict(lean_kernel="lean"), wide_14=dict(lean_kernel="lean", queued=0))),
    ("MRS_TG_LEAN_SHARED", "1", dict()),
    # MRS_TG_REGROUP=0: a call keeps the plan's dimension split
    ("MRS_TG_REGROUP", "0", dict(regroup_d2=dict(dim_split=4, lean=0, sweep_kernel="split", sweep_threads=128),
                                 regroup_moving=dict(dim_split=4, lean=0, sweep_kernel="split", sweep_threads=128))),
    # MRS_TG_LEAN_WIDE=0 never, =1 always the wide groups of a min-snap launch
    ("MRS_TG_LEAN_WIDE", "0", dict(regroup_moving=dict(lean_kernel="lean"), ragged=dict(lean_kernel="lean"),
                                   wide_14=dict(lean_kernel="lean", queued=0))),
    ("MRS_TG_LEAN_WIDE", "1", dict(narrow_14=dict(lean_kernel="lean_shared", queued=1))),
    # MRS_TG_LEAN_WIDE_ALL=0: only 13-15 and 29-30 segments move up, a ragged batch runs the mixed kernel over five bins
    ("MRS_TG_LEAN_WIDE_ALL", "0", dict(ragged=dict(lean_kernel="lean", lean_blocks=3478))),
    # MRS_TG_LEAN_RESIDENT_BLOCKS: the launcher reads it and passes the figure in (test_the_path_queue); the header does not
    ("MRS_TG_LEAN_RESIDENT_BLOCKS", "0", dict()),
    # MRS_TG_WAVE_KERNEL=0: the split kernel where the wave kernel ran
    ("MRS_TG_WAVE_KERNEL", "0", dict(one=dict(wave=0, sweep_kernel="split", sweep_threads=64),
                                     wave_1024=dict(wave=0, sweep_kernel="split", sweep_threads=128),
                                     wave_2560=dict(wave=0, sweep_kernel="split", sweep_threads=128))),
    # MRS_TG_MAXIMA_BOUNDS=0: every entry of the maxima searched, in every call
    ("MRS_TG_MAXIMA_BOUNDS", "0", {k: dict(certified_maxima=0) for k in PROBES}),
]


def test_the_knobs_are_the_section_of_the_header():
    """every knob of the section "routing of the nonlinear pipeline" is in KNOBS, and no other"""
    with open(os.path.join(hh.ROOT, "mrs_uav_trajectory_generation_amd", "csrc", "mrs_tg_knobs.hpp")) as f:
        text = f.read()
    section = text.split("// ---- routing of the nonlinear pipeline ----")[1].split("// ---- the C ABI's transfers and checks ----")[0]
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
    want = dict(one=["optimize_wave_kernel"], wave_1024=["optimize_wave_kernel"], wave_2560=["optimize_wave_kernel"],
                split_14=["optimize_split_kernel"],
                regroup_d2=["optimize_lean_shared_ends_kernel", "optimize_compact_kernel<true>"],
                regroup_moving=["optimize_lean_shared_kernel", "optimize_compact_kernel<false>"],
                lean_4096=["optimize_lean_shared_kernel", "optimize_compact_kernel<false>"],
                ends_4096=["optimize_lean_shared_ends_kernel", "optimize_compact_kernel<true>"],
                slots_4096=["optimize_lean_shared_ends_kernel", "optimize_compact_kernel<false>"],
                ragged=["optimize_lean_shared_kernel", "optimize_compact_kernel<false>"],
                ragged_d2=["optimize_lean_shared_ends_kernel", "optimize_compact_kernel<true>"],
                short_d2=["optimize_lean_shared_ends_kernel", "optimize_compact_kernel<true>"],
                queued=["set_queue_kernel", "optimize_lean_shared_kernel", "optimize_compact_kernel<false>"],
                long_80=["optimize_lean_shared_ends_long_kernel", "optimize_compact_kernel<false>"],
                lean_200=["optimize_lean_kernel", "optimize_compact_kernel<false>"],
                masked_200=["optimize_lean_masked_kernel", "optimize_compact_kernel<true>"],
                wide_14=["set_queue_kernel", "optimize_lean_shared_kernel", "optimize_compact_kernel<false>"],
                narrow_14=["set_queue_kernel", "optimize_lean_kernel", "optimize_compact_kernel<false>"])
    assert {k: nr.outer_names(r) for k, r in defaults.items()} == want
    assert all(r["certified_maxima"] == 1 and r["estimate_in_kernel"] == 1 for r in defaults.values())
    assert (defaults["wide_14"]["lean_bins"][0][0], defaults["narrow_14"]["lean_bins"][0][0]) == (32, 16)
    assert [len(defaults[k]["lean_bins"]) for k in ("ragged", "ragged_d2", "short_d2")] == [4, 4, 2]


# ---- the same lines under AddressSanitizer + UndefinedBehaviorSanitizer ----

def test_the_sanitizer_build_prints_the_same(harness, tmp_path):
    san = nr.build(tmp_path, sanitize=True)
    lines = list(PROBES.values())
    for kw in (dict(), dict(d=2), dict(slots=1, moving=1), dict(general=1, careful=1, estimate=0, samples=0)):
        lines += [request((1, S), **kw) for S in range(1, 301)]
    lines += [request((4096, S)) for S in range(1, 131)]
    lines += [request([60] * 2 + [50] * 2 + [40] * 2 + [30] * 2 + [20] * 2 + [10] * 2, as_bins=True), request((1, 1024)), request([], cus=64),
              request((0, 5)), request((2 ** 20, 10), cus=1, resident=1), request((2 ** 20, 3), cus=304, resident=0)]
    for env in (None, {"MRS_TG_DIM_SPLIT_MAX_PATHS": "100000", "MRS_TG_LEAN": "1", "MRS_TG_ENDS_MIN_SEGMENTS": "40", "MRS_TG_LEAN_WIDE_ALL": "0"}):
        assert hh.run(san, lines, 3 * len(lines), env=env) == hh.run(harness, lines, 3 * len(lines), env=env)
