"""The transfer plan of the one-call host interface on the CPU: csrc/mrs_tg_transfer.hpp (array table, classify, lay_out,
every_array_pinned, scan_constraints, count_position_mismatches_host, CopyList::add, route_hints) and policy_round_arena of csrc/mrs_tg_policy_host.hpp, compiled by g++ into
tests/host/transfer_harness.cpp.  The layout is checked exhaustively against its invariants inside the harness and, for named
cases, against a restatement here; the scans and the position check against brute force in numpy.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import host_harness as hh

# (segment counts per path, sample capacity)
BATCHES = {
    "one_path_one_segment": ([1], 0),
    "three_paths_1_2_4": ([1, 2, 4], 0),
    "64_paths_of_10_sampled": ([10] * 64, 256),
}
ARRAYS = ("waypoints", "mask", "values", "limits", "seg_times", "coeffs", "status", "cost", "n_samples", "samples")
INPUTS, OUTPUTS = ARRAYS[:4], ARRAYS[5:]
ABSENT, PINNED, PAGEABLE = 0, 1, 2


def _bytes(S, cap):
    P, nS = len(S), sum(S)
    nV = nS + P
    return dict(waypoints=nV * 4 * 8, mask=nV * 5, values=nV * 20 * 8, limits=P * 9 * 8, seg_times=nS * 8, coeffs=nS * 40 * 8,
                status=P * 4, cost=P * 8, n_samples=P * 4, samples=P * cap * 4 * 8)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return hh.build("transfer_harness.cpp", tmp_path_factory.mktemp("transfer"))


# ---- layout ----

def _up(n):
    return -(-n // 256) * 256


def _restated_layout(states, nbytes, stage_max):
    """what `layout` prints, from the rule in words: unstaged inputs, staged inputs, seg_times, staged outputs, unstaged outputs,
    every slot rounded up to 256 bytes, an unstaged output of no bytes given 8"""
    present = {a: states[a] != ABSENT and nbytes[a] > 0 for a in ARRAYS}
    pinned = {a: present[a] and states[a] == PINNED for a in ARRAYS}
    staged = {a: present[a] and not pinned[a] and nbytes[a] <= stage_max for a in ARRAYS}
    off, cursor = {}, 0
    for group, want_staged in ((INPUTS, False), (INPUTS, True), (("seg_times",), staged["seg_times"]), (OUTPUTS, True), (OUTPUTS, False)):
        if group == INPUTS and want_staged:
            span_begin = cursor
        if group == ("seg_times",):
            t_begin = cursor
        if group == OUTPUTS and not want_staged:
            span_end = cursor
        for a in group:
            if staged[a] == want_staged:
                off[a] = cursor
                cursor += _up(nbytes[a] if nbytes[a] or group is not OUTPUTS or want_staged else 8)
        if group == ("seg_times",):
            t_end = cursor
    in_span_end, out_span_begin = (t_end, t_begin) if staged["seg_times"] else (t_begin, t_end)
    out = []
    for a in ARRAYS:
        out += [int(staged[a]), off[a], off[a] - span_begin if staged[a] else -1]
    all_pinned = all(pinned[a] for a in ARRAYS if a != "limits" and present[a])
    return out + [span_begin, in_span_end, out_span_begin, span_end, max(cursor, 256), span_end - span_begin, int(all_pinned)]


def _named_cases():
    big = _bytes(*BATCHES["64_paths_of_10_sampled"])
    small = _bytes(*BATCHES["three_paths_1_2_4"])
    every = dict.fromkeys(ARRAYS, PAGEABLE)
    assert big["coeffs"] > 128 * 1024 > big["values"]
    no_samples = dict(small, samples=0)
    return {
        "all_pageable_small": (dict(every, n_samples=ABSENT, samples=ABSENT), no_samples, 256 * 1024),
        "all_pageable_coeffs_over_stage_max": (every, big, 128 * 1024),
        "all_pinned": (dict.fromkeys(ARRAYS, PINNED), big, 256 * 1024),
        "pinned_values_only": (dict(every, values=PINNED), big, 256 * 1024),
        # solve_batch_samples_only: no coefficients destination and no cost, their bytes as the batch implies
        "samples_only_no_coeffs_destination": (dict(every, coeffs=ABSENT, cost=ABSENT), big, 256 * 1024),
        "stage_max_0": (every, big, 0),
    }


def _layout_line(states, nbytes, stage_max):
    return "layout %d %s\n" % (stage_max, " ".join("%d %d" % (states[a], nbytes[a]) for a in ARRAYS))


def _check_named(exe, env=None):
    cases = _named_cases()
    got = hh.run(exe, [_layout_line(*c) for c in cases.values()], len(cases), env=env)
    for (name, case), line in zip(cases.items(), got):
        assert [int(x) for x in line.split()] == _restated_layout(*case), name
    return got


def test_named_layouts_against_their_restatement(harness):
    got = _check_named(harness)
    # and what the names promise: nothing staged at stage_max 0, zero copy's array half for all pinned only
    fields = {name: [int(x) for x in line.split()] for name, line in zip(_named_cases(), got)}
    f = fields["stage_max_0"]
    assert not any(f[0:30:3]) and f[-7] == f[-6] and f[-5] == f[-4]   # both spans empty
    assert [name for name, f in fields.items() if f[-1]] == ["all_pinned"]
    assert fields["all_pageable_coeffs_over_stage_max"][15] == 0 and all(fields["all_pageable_coeffs_over_stage_max"][0:15:3])


def _enumerate_lines():
    return ["enumerate %d %d %d\n" % (len(S), sum(S), cap) for S, cap in BATCHES.values()]


def test_every_combination_of_array_states_keeps_the_layout_invariants(harness):
    for name, line in zip(BATCHES, hh.run(harness, _enumerate_lines(), len(BATCHES))):
        states, *violations = [int(x) for x in line.split()]
        assert states == 3 * 4 ** 9, name     # seg_times is never absent
        assert violations == [0] * 9, (name, violations)


# ---- scan_constraints ----

def _plain_batch(S):
    """masks and values of paths with positions everywhere and every derivative slot free, at the ends as well: whatever a
    variant constrains is the only constrained slot of its batch"""
    so = np.concatenate([[0], np.cumsum(S)]).astype(int)
    nV = so[-1] + len(S)
    mask = np.zeros((nV, 5), dtype=np.uint8)
    mask[:, 0] = 1
    vals = np.zeros((nV, 5, 4))
    vals[:, 0] = np.arange(nV * 4).reshape(nV, 4) + 1.0
    return so, mask, vals


def _brute_force(so, mask, vals, derivative, want):
    P = len(so) - 1
    first = [so[p] + p for p in range(P)]
    interior = [v for p in range(P) for v in range(so[p] + p + 1, so[p + 1] + p)]
    general = bool(np.any(mask[:, 0] == 0))
    slots = derivative == 4 and bool(np.any(mask[interior, 1:] != 0)) if interior else False
    moving = bool(np.any((mask[first, 1:, None] != 0) & (vals[first, 1:] != 0.0)))
    return [int(general and want[0]), int(slots and want[1]), int(moving and want[2])]


def _scan_problems():
    problems = {}
    for bname, (S, _) in BATCHES.items():
        so, mask, vals = _plain_batch(S)
        last_first, last_end = so[-2] + len(S) - 1, so[-1] + len(S) - 1

        def variant(name, edit=None, derivative=4, want=(1, 1, 1)):
            m, v = mask.copy(), vals.copy()
            if edit:
                edit(m, v)
            problems["%s/%s" % (bname, name)] = (so, m, v, derivative, want)

        def free_last_vertex(m, v):
            m[last_end, 0] = 0

        def slot_at_first_interior_of_last_path(m, v):
            m[last_first + 1, 2] = 1

        def slots_at_the_ends_only(m, v):   # an end vertex never counts as a constrained interior slot; a non-zero
            m[last_first, 1:] = 1           # constrained value at the LAST vertex is no moving start either
            m[last_end, 1:] = 1
            v[last_end, 2, 1] = 0.75

        def moving_last_path(m, v):
            m[last_first, 3] = 1
            v[last_first, 3, 2] = -0.25

        def zero_valued_start(m, v):        # the same slot, constrained at zero: not a moving start
            m[last_first, 3] = 1

        def free_slot_with_a_value(m, v):   # a non-zero value in a slot that is not constrained: not a moving start
            v[last_first, 3, 2] = -0.25

        variant("plain")
        variant("position_free_last_vertex", free_last_vertex)
        if S[-1] > 1:                       # (a path of one segment has no interior vertex: three_paths starts with one)
            variant("interior_slot", slot_at_first_interior_of_last_path)
            variant("interior_slot_not_min_snap", slot_at_first_interior_of_last_path, derivative=3)
        variant("end_slot_only", slots_at_the_ends_only)
        variant("free_slot_with_a_value", free_slot_with_a_value)
        variant("moving_start_of_last_path", moving_last_path)
        variant("zero_valued_start", zero_valued_start)
        variant("everything_but_nothing_wanted", lambda m, v: (free_last_vertex(m, v), moving_last_path(m, v)), want=(0, 0, 0))
        for k in range(3):
            variant("only_scan_%d_wanted" % k, lambda m, v: (free_last_vertex(m, v), moving_last_path(m, v),
                                                             S[-1] > 1 and slot_at_first_interior_of_last_path(m, v)),
                    want=tuple(int(j == k) for j in range(3)))
    return problems


def _scan_line(so, mask, vals, derivative, want):
    return "scan %d %d %d %d %d %s %s %s\n" % (len(so) - 1, derivative, want[0], want[1], want[2], " ".join(map(str, so)),
                                               " ".join(map(str, mask.reshape(-1))), hh.fmt(vals))


def _check_scans(exe, env=None):
    problems = _scan_problems()
    got = hh.run(exe, [_scan_line(*p) for p in problems.values()], len(problems), env=env)
    for (name, p), line in zip(problems.items(), got):
        assert [int(x) for x in line.split()] == _brute_force(*p), name
    return got


def test_scan_constraints_against_brute_force(harness):
    got = dict(zip(_scan_problems(), _check_scans(harness)))
    # and the restatement itself says what the cases are there for
    for b in BATCHES:
        assert got[b + "/plain"] == "0 0 0" and got[b + "/position_free_last_vertex"] == "1 0 0"
        assert got[b + "/end_slot_only"] == "0 0 0" and got[b + "/zero_valued_start"] == "0 0 0"
        assert got[b + "/free_slot_with_a_value"] == "0 0 0"
        assert got[b + "/moving_start_of_last_path"] == "0 0 1"
    lines = {name: _scan_line(*p) for name, p in _scan_problems().items()}
    assert len(set(lines.values())) == len(lines)   # no variant repeats another problem
    assert "one_path_one_segment/interior_slot" not in got
    assert got["three_paths_1_2_4/interior_slot"] == "0 1 0" and got["three_paths_1_2_4/interior_slot_not_min_snap"] == "0 0 0"


# ---- count_position_mismatches_host: MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS checked on host arrays (mrs_tg_solve_batch) ----

def _text(x):
    """a double as text that reads back to the same bits, the sign bit of a NaN included (repr() drops it)"""
    x = float(x)
    if x != x:
        return "-nan" if np.array(x).view(np.uint64) >> np.uint64(63) else "nan"
    return repr(x)


def _mismatch_problems():
    """name -> (seg_offsets, waypoints, mask, values, the count the case is there for).  The criterion is
    position_mismatch_kernel's: position bit unset, or the four doubles of the constrained position not the waypoint's BITS"""
    problems = {}
    for bname, S in (("one_path_one_segment", [1]), ("ragged_1_2_4", [1, 2, 4]), ("64_paths_of_10", [10] * 64)):
        so, mask, vals = _plain_batch(S)
        wp = vals[:, 0].copy()
        nV = wp.shape[0]
        mid, last = nV // 2, nV - 1

        def variant(name, expected, edit=None):
            w, m, v = wp.copy(), mask.copy(), vals.copy()
            if edit:
                edit(w, m, v)
            problems["%s/%s" % (bname, name)] = (so, w, m, v, expected)

        def one_value(w, m, v):
            w[last, 3] = np.nextafter(w[last, 3], np.inf)       # one ulp, in the last double of the batch

        def one_bit(w, m, v):
            m[mid, 0] = 0

        def both_at_one_vertex(w, m, v):                        # a vertex counts once
            m[0, 0] = 0
            w[0, 1] += 1.0

        def other_slots_do_not_matter(w, m, v):                 # derivative slots and their values are not the statement's
            m[:, 1:] = 1
            v[:, 1:] = 7.0

        def nan_of_the_same_bits(w, m, v):                      # the solve reads the same bits from either array: no mismatch
            w[mid, 2] = v[mid, 0, 2] = np.nan

        def nan_in_the_waypoint_only(w, m, v):
            w[mid, 2] = np.nan

        def nan_of_the_other_sign(w, m, v):
            w[mid, 2], v[mid, 0, 2] = np.nan, -np.nan

        def zero_of_the_other_sign(w, m, v):
            w[0, 0], v[0, 0, 0] = 0.0, -0.0

        def every_vertex(w, m, v):
            m[:, 0] = 0

        variant("true_statement", 0)
        variant("one_value", 1, one_value)
        variant("one_unset_bit", 1, one_bit)
        variant("bit_and_value_at_one_vertex", 1, both_at_one_vertex)
        variant("other_slots_do_not_matter", 0, other_slots_do_not_matter)
        variant("nan_of_the_same_bits", 0, nan_of_the_same_bits)
        variant("nan_in_the_waypoint_only", 1, nan_in_the_waypoint_only)
        variant("nan_of_the_other_sign", 1, nan_of_the_other_sign)
        variant("zero_of_the_other_sign", 1, zero_of_the_other_sign)
        variant("every_vertex", nV, every_vertex)
    problems["empty_batch"] = (np.zeros(1, dtype=int), np.zeros((0, 4)), np.zeros((0, 5), dtype=np.uint8), np.zeros((0, 5, 4)), 0)
    return problems


def _mismatch_brute_force(so, wp, mask, vals, _):
    same_bits = np.ascontiguousarray(wp).view(np.uint64) == np.ascontiguousarray(vals[:, 0]).view(np.uint64)
    return int(np.sum((mask[:, 0] == 0) | ~same_bits.all(axis=1)))


def _mismatch_line(so, wp, mask, vals, _):
    return "mismatch %d %s %s %s %s\n" % (len(so) - 1, " ".join(map(str, so)), " ".join(_text(x) for x in wp.reshape(-1)),
                                          " ".join(map(str, mask.reshape(-1))), " ".join(_text(x) for x in vals.reshape(-1)))


def _check_mismatches(exe, env=None):
    problems = _mismatch_problems()
    got = hh.run(exe, [_mismatch_line(*p) for p in problems.values()], len(problems), env=env)
    for (name, p), line in zip(problems.items(), got):
        assert int(line) == _mismatch_brute_force(*p) == p[4], (name, line)
    return got


def test_position_mismatch_count_against_brute_force(harness):
    """zero mismatches, one value, one unset bit, NaNs (the kernel's answer: equal bits are equal), a ragged batch, an empty one"""
    got = dict(zip(_mismatch_problems(), _check_mismatches(harness)))
    assert got["empty_batch"] == "0" and got["ragged_1_2_4/true_statement"] == "0" and got["ragged_1_2_4/every_vertex"] == "10"
    lines = {name: _mismatch_line(*p) for name, p in _mismatch_problems().items()}
    assert len(set(lines.values())) == len(lines)   # no variant repeats another problem (the signs of NaN and zero reach the text)


# ---- policy_round_arena, CopyList ----

ARENA_SHAPES = [(1, 1, 0), (1, 1, 1), (3, 7, 16), (64, 640, 256)]


def _check_arena(exe, env=None):
    got = hh.run(exe, ["arena %d %d %d\n" % s for s in ARENA_SHAPES], len(ARENA_SHAPES), env=env)
    for (A, nS, cap), line in zip(ARENA_SHAPES, got):
        *offsets, total, in_bytes, block_samples, block_total = [int(x) for x in line.split()]
        nV = nS + A
        # results | mask | values | times | coefficients | cost | status | n_samples | rows | samples
        sizes = [block_samples - in_bytes, nV * 5, nV * 160, nS * 8, nS * 320, A * 8, A * 4, A * 4, A * 4, A * cap * 32]
        assert all(o % 256 == 0 for o in offsets + [total]), (A, nS, cap)
        assert offsets[0] == in_bytes                      # the arena starts with the block's input region, as in the block
        for (o, n), nxt in zip(zip(offsets, sizes), offsets[1:] + [total]):
            assert o + n <= nxt and nxt - (o + n) < 256, (A, nS, cap, o, n, nxt)   # disjoint, alignment padding only
        assert offsets[1] - offsets[0] == block_samples - in_bytes     # the results region has the size of the block's
        assert block_total - block_samples == total - offsets[-1]      # ... and so has the sample region
    return got


def test_policy_round_arena_is_aligned_disjoint_and_mirrors_the_block(harness):
    _check_arena(harness)


def test_a_full_copy_list_refuses_the_next_copy(harness):
    k_max, n, refused = [int(x) for x in hh.run(harness, ["copylist\n"], 1)[0].split()]
    assert n == k_max == 8 and refused == 1


# ---- route_hints: what a solve tells its launchers, from its option flags and what its caller saw of the first vertices ----

def _header_enum(prefix):
    """name -> value of every enumerator of include/mrs_tg.h that starts with `prefix`"""
    with open(os.path.join(hh.ROOT, "include", "mrs_tg.h")) as f:
        found = dict((name, int(value)) for name, value in re.findall(r"\b(%s\w+)\s*=\s*(-?\d+)" % prefix, f.read()))
    assert found, prefix
    return found


MELLINGER = "MRS_TG_TIME_ALLOC_MELLINGER"
# (time-allocation method by name, paths, longest path): the shape that is inside the window and its neighbours across each edge
HINT_INSIDE = (MELLINGER, 1536, 13)
HINT_EDGES = [((MELLINGER, 1536, 13), (MELLINGER, 1537, 13)), ((MELLINGER, 1536, 13), (MELLINGER, 1536, 12)),
              ((MELLINGER, 1536, 15), (MELLINGER, 1536, 16)), ((MELLINGER, 1, 15), (MELLINGER, 1, 16)),
              ((MELLINGER, 1, 13), (MELLINGER, 1, 12))]


def _hint_cases():
    """(flags, seen, method, paths, segments) of every case: every flag bit alone, none and all of them, on every shape; the
    shapes are the window's neighbours under Mellinger and the inside shape under every other method"""
    flags, methods = _header_enum("MRS_TG_FLAG_"), _header_enum("MRS_TG_TIME_ALLOC_")
    shapes = sorted(set(s for pair in HINT_EDGES for s in pair) | set((m, HINT_INSIDE[1], HINT_INSIDE[2]) for m in methods))
    every = 0
    for bit in flags.values():
        every |= bit
    return [(f, seen, methods[m], n, S) for f in [0, every] + sorted(flags.values()) for seen in (0, 1) for m, n, S in shapes]


def _check_hints(exe, env=None):
    flags, methods = _header_enum("MRS_TG_FLAG_"), _header_enum("MRS_TG_TIME_ALLOC_")
    shared, slots = flags["MRS_TG_FLAG_SHARED_DEVICE"], flags["MRS_TG_FLAG_CONSTRAINED_SLOTS"]
    assert len(set(flags.values())) == len(flags) and all(bit & (bit - 1) == 0 for bit in flags.values())   # one bit each
    cases = _hint_cases()
    got = hh.run(exe, ["hints %d %d %d %d %d\n" % c for c in cases], len(cases), env=env)
    wants = {}
    for (f, seen, method, n, S), line in zip(cases, got):
        h_shared, h_slots, h_moving, wanted = [int(x) for x in line.split()]
        # each of the two flags sets its own field and no other; every other bit of the header sets none
        assert (h_shared, h_slots) == (int(f & shared != 0), int(f & slots != 0)), (f, line)
        # a moving start: seen AND a shape inside wants_moving_starts' window -- whatever the flags are
        assert h_moving == int(seen and wanted), (f, seen, method, n, S, line)
        assert wants.setdefault((method, n, S), wanted) == wanted   # the window does not depend on flags or on `seen`
    # the cases lie on both sides of every edge of the window as wants_moving_starts draws it (move them when it moves)
    for inside, outside in HINT_EDGES:
        assert wants[(methods[inside[0]],) + inside[1:]] == 1 and wants[(methods[outside[0]],) + outside[1:]] == 0, (inside, outside)
    for name, m in methods.items():
        assert wants[(m,) + HINT_INSIDE[1:]] == int(name == MELLINGER), name
    return got


def test_route_hints_follow_their_flags_and_the_moving_start_window(harness):
    _check_hints(harness)


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness):
    san = hh.build("transfer_harness.cpp", tmp_path, sanitize=True)
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    assert _check_named(san, env=env) == _check_named(harness)
    assert _check_scans(san, env=env) == _check_scans(harness)
    assert _check_mismatches(san, env=env) == _check_mismatches(harness)
    assert _check_arena(san, env=env) == _check_arena(harness)
    assert _check_hints(san, env=env) == _check_hints(harness)
    assert hh.run(san, _enumerate_lines()[:2] + ["copylist\n"], 3, env=env) == hh.run(harness, _enumerate_lines()[:2] + ["copylist\n"], 3)
