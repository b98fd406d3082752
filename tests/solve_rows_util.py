"""solve_rows_kernel (csrc/mrs_tg_rows.hip) at the lengths where its schedule changes: the batches shared by
test_solve_rows_cases.py (CPU) and test_gpu_solve_rows_lengths.py (GPU), their oracle results, and a host statement of the
kernel's schedule and of the launcher's size rules.

schedule(), wavefronts(), path_doubles() and lds_bytes() are a hand-kept SECOND COPY of the kernel's and the launcher's integer
arithmetic (as chunk_model in sampler_walk_util.py is of the sampler's chunking).  They certify which edge a case reaches;
they are not a reference for any value.  An edit of the `nact` block, of RowSolve::run's start or of rows_lds_bytes needs the
same edit here, and test_solve_rows_cases.py then says which cases lost their edge."""
import functools

import numpy as np

from mrs_uav_trajectory_generation_amd import problem as pr
from oracle import pyoracle as po
from tests import util

# ---------------------------------------------------------------------------------------------------------------------
# the kernel's schedule, restated

VTX_REC, SEG_REC, N_DIM, N_COEFF = 88, 10, 4, 10     # kRVtxRec, kRSegRec, kD, kN
SAMPLE_BUFFER = 192                                  # kSampleBuffer
LDS_BUDGET = 144 * 1024                              # kRowsLdsBudget
LDS_DEFAULT = 64 * 1024                              # above it the launch raises its dynamic-LDS limit first
TAIL_MAX_PATHS = 2048                                # rows_tail_sampling_pays (mrs_tg_solve_route.hpp)


def schedule(S, mask_first, mask_last):
    """(mid, nact0, nact1) of a path of S segments whose first / last vertex have the fixed masks given ([5] each): the
    `nact` block of solve_rows_body.  Direction 0 eliminates the vertices [0, mid), direction 1 the vertices (mid, S]; an end
    vertex whose slots 1..4 are all constrained is left out."""
    mid = S // 2
    nact = []
    for length, mask in ((mid, mask_first), (S - mid, mask_last)):
        end_fixed = all(int(m) != 0 for m in np.asarray(mask).reshape(-1)[1:5])
        nact.append(length - 1 if (length > 0 and end_fixed) else length)
    return mid, nact[0], nact[1]


def first_built(nact, quad):
    """the distance of the vertex quad `quad` builds before the first step (RowSolve::run's w0; -1: none)"""
    w0 = -1
    if quad <= nact:
        w0 = nact - ((nact - quad) & 3)
    if quad == 0 and nact < 4:
        w0 = 0
    return w0


def path_schedule(batch, p):
    v0, v1 = batch.vertex_range(p)
    return schedule(int(batch.seg_offsets[p + 1] - batch.seg_offsets[p]), batch.fixed_mask[v0], batch.fixed_mask[v1 - 1])


def plan_order(seg_offsets):
    """the plan's order as DESIGN.md states it (longest first, stable).  Without a GPU there is no plan to ask; the GPU tests
    pass api.Plan.order to wavefronts() and assert that it is this."""
    return np.argsort(-np.diff(np.asarray(seg_offsets, dtype=np.int64)), kind="stable").astype(np.int32)


def wavefronts(batch, ppw, order=None):
    """per wavefront of a launch with `ppw` paths per wavefront: (its paths in the plan's order, its wmax).  The spare rows of a
    wavefront that holds one path repeat that path (store_ok = false), so its wmax is that path's own."""
    order = plan_order(batch.seg_offsets) if order is None else np.asarray(order)
    assert sorted(order.tolist()) == list(range(batch.n_paths))
    out = []
    for q0 in range(0, batch.n_paths, ppw):
        paths = tuple(int(p) for p in order[q0:q0 + ppw])
        out.append((paths, max(max(path_schedule(batch, p)[1:]) for p in paths)))
    return out


def path_doubles(S):
    """rows_path_doubles"""
    base = (S + 1) * VTX_REC + S * SEG_REC + S * N_DIM
    return base + (base & 1) + 2


def lds_bytes(Smax, ppw, sampling):
    """rows_lds_bytes (without the pipeline kernel's maxima)"""
    doubles = ppw * path_doubles(Smax)
    if sampling:
        doubles += ppw * Smax * (N_DIM * N_COEFF + 1) + SAMPLE_BUFFER + SAMPLE_BUFFER // 4 + 2
    return 8 * doubles


def route(Smax, n_paths, shared=False, sampling=False):
    """what route_solve (mrs_tg_solve_route.hpp) gives a fixed-times default solve of fewer than 6144 paths:
    dict(rows, ppw, tail, raised) -- rows False: the batch goes to the tile / lane kernels"""
    if lds_bytes(Smax, 1, False) > LDS_BUDGET:
        return dict(rows=False, ppw=0, tail=False, raised=False)
    tail = sampling and n_paths <= TAIL_MAX_PATHS and lds_bytes(Smax, 1, True) <= LDS_BUDGET
    ppw = 1 if (n_paths <= 2048 and not (shared and not tail)) else 2
    if lds_bytes(Smax, 2, tail) > LDS_BUDGET:
        ppw = 1
    return dict(rows=True, ppw=ppw, tail=tail, raised=lds_bytes(Smax, ppw, tail) > LDS_DEFAULT)


# ---------------------------------------------------------------------------------------------------------------------
# the batches

def lengths_batch(lengths, copies, d, seed0, moving=False, stop_every=0):
    """`copies` box-generator paths per entry of `lengths`, length by length in the order given.  Only patterns the adapter
    builds: rest-to-rest; moving=True: every path starts from a moving state; stop_every = n > 0: stop_at at every n-th
    interior vertex."""
    assert not (moving and stop_every)
    parts = []
    for S in lengths:
        for _ in range(copies):
            stop = None
            if stop_every:
                stop = [0 < i < S and i % stop_every == 0 for i in range(S + 1)]
            parts.append(pr.build_vertices(pr.random_box_waypoints(S, seed0 + len(parts)), d, stop_at=stop))
    batch = pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (len(parts), 1)), d)
    if moving:
        from tests.test_gpu_large_batches import _moving
        batch = _moving(batch)
    return batch


EVERY_LENGTH = tuple(range(1, 41))
SIZE_EDGE_LENGTHS = ((39, 17, 4), (79, 33, 5), (80, 33, 5), (89, 64, 2), (90, 65, 1), (179, 128, 65, 7), (180, 129, 7))
LONGEST_ROWS = (179, 128, 65, 7)
TAIL_LENGTHS = ((54, 9), (55, 9), (126, 63, 3), (127, 64, 3))
GROUP_LENGTHS = ((79, 33, 5), (80, 33, 5), (89, 64, 2), LONGEST_ROWS)
KINDS = ("rest", "moving", "stop")

# ("every", d, kind) | ("mixed", d) | ("edge", lengths, d, kind) | ("tail", lengths)
EVERY_KEYS = tuple(("every", d, kind) for d in (4, 3, 2) for kind in KINDS) + (("mixed", 4), ("mixed", 2))
EDGE_KEYS = tuple(("edge", lengths, d, kind) for lengths in SIZE_EDGE_LENGTHS for d, kind in ((4, "rest"), (2, "rest"), (4, "moving"))) + \
    (("edge", LONGEST_ROWS, 2, "moving"),)     # (for the alone-solves of test_gpu_solve_rows_lengths.py)
TAIL_KEYS = tuple(("tail", lengths) for lengths in TAIL_LENGTHS)
ALL_KEYS = EVERY_KEYS + EDGE_KEYS + TAIL_KEYS


def key_id(key):
    return "-".join("x".join(map(str, k)) if isinstance(k, tuple) else str(k) for k in key)


def _seed0(key):
    """one seed range per batch (a seed that breaks an oracle condition is replaced HERE, on the CPU)"""
    return 7_000_000 + 10_000 * ALL_KEYS.index(key)


def build(key):
    kind = key[0]
    if kind == "every":
        return lengths_batch(EVERY_LENGTH, 3, key[1], _seed0(key), moving=key[2] == "moving", stop_every=3 if key[2] == "stop" else 0)
    if kind == "mixed":
        return pr.random_mixed_batch(240, key[1], seed0=_seed0(key), max_segments=40)
    if kind == "edge":
        return lengths_batch(key[1], 3, key[2], _seed0(key), moving=key[3] == "moving")
    if kind == "tail":
        return lengths_batch(key[1], 3, 4, _seed0(key))
    raise KeyError(key)


# ---------------------------------------------------------------------------------------------------------------------
# the reference

def oracles(batch, times):
    """(double-precision oracle, 113-bit oracle) of the fixed-times solve over every path"""
    args = (batch.seg_offsets, batch.waypoints, batch.fixed_mask, batch.fixed_values, batch.limits, times)
    ref_d = po.solve_batch(*args, deriv=batch.derivative_to_optimize, n_threads=16)
    po.lib().mto_set_arithmetic(po.QUAD_PRECISION)
    try:
        ref_q = po.solve_batch(*args, deriv=batch.derivative_to_optimize, n_threads=16)
    finally:
        po.lib().mto_set_arithmetic(po.REFERENCE_ARITHMETIC)
    return ref_d, ref_q


def path_errors(c, ref, so):
    return np.array([util.coeff_error(c[a:b], ref[a:b]) for a, b in zip(so[:-1], so[1:])])


class Reference:
    """a batch, the oracle's Euclidean segment times, both oracle results at those times and e_o per path; read-only"""

    def __init__(self, batch):
        self.batch, self.times = batch, util.oracle_times(batch)
        self.ref_d, self.ref_q = oracles(batch, self.times)
        self.e_o = path_errors(self.ref_d["coeffs"], self.ref_q["coeffs"], batch.seg_offsets)
        for a in (self.times, self.e_o, self.ref_q["coeffs"], self.ref_q["cost"], self.ref_q["status"], self.ref_d["status"]):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)   # (the largest batch has 2460 segments)
def reference(key):
    return Reference(build(key))


def stats(e):
    return float(np.median(e)), float(np.percentile(e, 99)), float(np.max(e))
