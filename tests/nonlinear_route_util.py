"""What tests/test_nonlinear_route_host.py and tests/test_gpu_nonlinear_route.py share: the line grammar of
tests/host/nonlinear_route_harness.cpp (one request and its batch per line -> the host plan's bins, the fields of the
NonlinearRoute that route_nonlinear returns and the two closing solves' routes) and a restatement, from those fields, of the
kernel names launch_nonlinear notes, in launch order -- written from the names as profiles/launch_layer_routing_table.md and
include/mrs_tg.h spell them, not from the launcher's code.  The closing solves go by tests/solve_route_util.py."""
import itertools

from tests import host_harness as hh
from tests import solve_route_util as sr


def build(tmp_path, sanitize=False):
    return hh.build("nonlinear_route_harness.cpp", tmp_path, sanitize=sanitize)


def runs(lengths):
    """the batch as the harness reads it: run-length pairs (count, segments) of the lengths in the caller's path order"""
    return [(len(list(g)), int(S)) for S, g in itertools.groupby(lengths)]


def request(batch, d=4, slots=0, moving=0, shared=0, cus=256, resident=None, estimate=1, general=0, careful=0, samples=1, fused=1,
            store=1, wp=0, solve_cus=None, as_bins=False):
    """one input line.  batch: (paths, segments) of a uniform batch, or the lengths of every path in the caller's order.
    resident: the path queue's resident blocks (default: what the library passes on a device of `cus` compute units, two
    wavefronts per SIMD); solve_cus: the compute units the closing solves route by (default: cus); as_bins: every run of equal
    lengths (longest first) is made a bin of the plan as it stands"""
    pairs = [(int(batch[0]), int(batch[1]))] if isinstance(batch, tuple) else runs(batch)
    resident = cus * 4 * 2 if resident is None else resident
    v = [d, slots, moving, shared, cus, resident, estimate, general, careful, samples, fused, store, wp, cus if solve_cus is None else solve_cus,
         -len(pairs) if as_bins else len(pairs)] + [x for pair in pairs for x in pair]
    return " ".join(str(int(x)) for x in v) + "\n"


def _bins(text):
    return [] if text == "-" else [tuple(int(x) for x in b.split(":")) for b in text.split(",")]


_TEXT = ("lean_kernel", "sweep_kernel", "closing")
_BINS = ("bins", "bins1", "wide_bins", "ends_bins", "lean_bins", "sweep_bins")


def parse(line):
    """plan bins as (group, q_begin, q_count, max_S, min_S), launch bins as (group, q_begin, q_count, max_S, block_begin)"""
    r = {}
    for item in line.split():
        k, v = item.split("=")
        r[k] = v if k in _TEXT else _bins(v) if k in _BINS else int(v)
    return r


def routes(exe, lines, env=None):
    """per request the outer loop's route, with the closing solves' routes under "first" and "final" """
    out = hh.run(exe, lines, 3 * len(lines), env=env)
    got = []
    for i in range(0, len(out), 3):
        r = parse(out[i])
        r["first"], r["final"] = sr.parse(out[i + 1]), sr.parse(out[i + 2])
        got.append(r)
    return got


LEAN = {"lean": "optimize_lean_kernel", "lean_masked": "optimize_lean_masked_kernel", "lean_shared": "optimize_lean_shared_kernel",
        "lean_shared_ends": "optimize_lean_shared_ends_kernel", "lean_shared_ends_long": "optimize_lean_shared_ends_long_kernel"}
SWEEP = {"wave": "optimize_wave_kernel", "split": "optimize_split_kernel", "compact": "optimize_compact_kernel<false>",
         "compact_masked": "optimize_compact_kernel<true>"}


def outer_names(r, estimate=True):
    """the outer loop's launches: the estimate in front where the kernels do not compute it, the queue's counter, the lean kernel,
    the sweeping kernel; None where the call is refused (the sweeping launch does not fit)"""
    assert not r["careful"] and not r["general"]   # (their launches are counted by the batch, not restated here)
    names = ["estimate_times_kernel"] if estimate and not r["estimate_in_kernel"] else []
    if r["lean"]:
        names += (["set_queue_kernel"] if r["queued"] else []) + [LEAN[r["lean_kernel"]]]
    if not r["wave"] and not r["sweep_fits"]:
        return None
    return names + [SWEEP[r["sweep_kernel"]]]


def kernel_names(r, estimate=True, reference_status=False):
    """every launch of launch_nonlinear, in order"""
    names = outer_names(r, estimate)
    if names is None:
        return None
    if r["closing"] == "rows_pipeline":
        return names + sr.closing_names(r["first"], r["final"])
    first, final = sr.closing_names(r["first"], r["final"])
    names += [first, "segment_maxima_scaling_kernel" if r["certified_maxima"] else "segment_maxima9_kernel"]
    if r["closing"] == "separate":
        names += ["apply_scaling_kernel"] + ([] if reference_status else ["runaway_kernel"])
    return names + [final]


def compress(names):
    """as scripts/routing_table.py prints a row: names in first-launch order, a repeated one once with its count"""
    seen, order = {}, []
    for n in names:
        if n not in seen:
            order.append(n)
        seen[n] = seen.get(n, 0) + 1
    return ["`%s`%s" % (n, " (x %d)" % seen[n] if seen[n] > 1 else "") for n in order]
