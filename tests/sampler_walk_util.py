"""The sampler's walk (csrc/mrs_tg_sampling.hpp) at its segment, chunk, buffer, capacity and table edges: the reference's
loop replayed in Python floats, exact values of a sampled state with the bound a Horner chain may miss them by, a host model
of the kernel's chunking (to certify which edge an input reaches), and the case list shared by test_sampler_walk_cases.py
(CPU) and test_gpu_sampler_walk_edges.py (GPU).  No GPU and no oracle in here."""
import math
from fractions import Fraction

import numpy as np

from mrs_uav_trajectory_generation_amd.problem import SplitMix64

N_COEFF, N_DIM, N_ORDERS = 10, 4, 5
SAMPLE_BUFFER = 192          # kSampleBuffer
TABLE_DT = 13.0 / 32.0       # the table-edge cases' own sampling period: no other test builds a table for it
TABLE_CAPACITY = 1024        # capacity + 80 = the smallest table (1104 entries)
STANDARD_CAPACITIES = (16, 63, 64, 65, 191, 192, 193, 4200)
U = Fraction(1, 2 ** 53)     # unit roundoff of binary64

_PI_BITS = 320
_PI = None


def pi_exact():
    """pi as a rational, wrong by less than 2^-300"""
    global _PI
    if _PI is None:
        import mpmath
        with mpmath.workprec(_PI_BITS + 16):
            _PI = Fraction(int(mpmath.floor(mpmath.ldexp(mpmath.pi, _PI_BITS))), 2 ** _PI_BITS)
    return _PI


# ---------------------------------------------------------------------------------------------------------------------
# the reference's walk

def _walk(seg_times, dt, capacity):
    """Trajectory::evaluateRange (trajectory.cpp:93-151) with t_start = 0, in IEEE doubles, with the oracle's early stop at
    count > capacity.  Returns (samples, count, edges)."""
    T = [float(x) for x in seg_times]
    dt = float(dt)
    S = len(T)
    edges = dict(boundary_hits=0, multi_carries=0, longest_carry=0, zero_segments_passed=0, past_end=False,
                 t_end_on_grid=False, capacity_cut=False)
    t_end = 0.0
    for x in T:
        t_end += x
    accumulated = 0.0
    i = 0
    while i < S:
        accumulated += T[i]
        if accumulated > 0.0:
            break
        i += 1
    edges["zero_segments_passed"] += sum(1 for x in T[:i] if x == 0.0)
    if i >= S or 0.0 > accumulated:
        return [], 0, edges
    accumulated -= T[i]
    tin = 0.0 - accumulated
    samples = []
    count = 0
    carried = 0
    while accumulated < t_end:
        if tin > T[i]:
            tin = tin - T[i]
            i += 1
            carried += 1
            if i >= S:
                edges["past_end"] = True
                break
            if T[i] == 0.0:
                edges["zero_segments_passed"] += 1
            continue
        if carried >= 2:
            edges["multi_carries"] += 1
        edges["longest_carry"] = max(edges["longest_carry"], carried)
        carried = 0
        samples.append((i, tin))
        if tin == T[i]:
            edges["boundary_hits"] += 1
        count += 1
        tin += dt
        accumulated += dt
        if count > capacity:
            edges["capacity_cut"] = True
            break
    else:
        edges["t_end_on_grid"] = accumulated == t_end
    return samples, count, edges


def replay(seg_times, dt, capacity):
    """-> ([(segment, time_in_segment)], count); count = capacity + 1 means "more than fit" (that many entries are listed)"""
    samples, count, _ = _walk(seg_times, dt, capacity)
    return samples, count


def replay_edges(seg_times, dt, capacity):
    """which edges the reference's walk passes on this input: samples with time_in_segment == T_i, steps that carry the
    remainder through >= 2 segments, zero-length segments skipped or carried through, an exit because the segments ran out
    while accumulated < t_end, an exit with accumulated == t_end, a stop at the capacity"""
    return _walk(seg_times, dt, capacity)[2]


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's chunking, restated on the host (sample_path_walk): which chunk / buffer / capacity edge an input reaches

def chunk_model(seg_times, dt, capacity, parks=True):
    """-> dict(samples, count, chunks=[(segment, last, m)], flushes=[parked], ...).  The arithmetic that decides the chunking
    ((T_i - tin) * (1 / dt), repeated addition of dt) is the kernel's, in the same IEEE operations."""
    T = [float(x) for x in seg_times]
    dt = float(dt)
    S = len(T)
    t_end = 0.0
    for x in T:
        t_end += x
    inv_dt = 1.0 / dt
    # n_total = #{k : A[k] < t_end}; beyond capacity + 1 its value no longer matters (the lanes also stop at the capacity)
    n_total = 0
    if t_end == t_end:
        acc = 0.0
        while acc < t_end and n_total < capacity + 2:
            n_total += 1
            acc += dt
    i = 0
    acc = 0.0
    while i < S:
        acc += T[i]
        if acc > 0.0:
            break
        i += 1
    out = dict(samples=[], chunks=[], flushes=[], misfit_flushes=0, past_end=False)
    n = n_flushed = 0
    if i < S:
        tin, Ti = 0.0, T[i]
        while n < n_total:
            while tin > Ti:
                tin = tin - Ti
                i += 1
                if i >= S:
                    out["past_end"] = True
                    break
                Ti = T[i]
            if out["past_end"]:
                break
            room = (Ti - tin) * inv_dt
            last = int(room) + 2 if room < 61.0 else 63
            tj = [tin]
            for _ in range(last + 1):   # (one more than the lanes: lane `last` + dt restarts the next chunk)
                tj.append(tj[-1] + dt)
            m = 0
            while m <= last and n + m < n_total and not (tj[m] > Ti) and n + m <= capacity:
                m += 1
            assert m >= 1
            if parks:
                if n + m - n_flushed > SAMPLE_BUFFER:
                    out["flushes"].append(n - n_flushed)
                    out["misfit_flushes"] += (n - n_flushed) < SAMPLE_BUFFER
                    n_flushed = n
                out["samples"] += [(i, tj[j]) for j in range(m)]
            out["chunks"].append((i, last, m))
            n += m
            tin = tj[last + 1] if m == last + 1 else tj[m]
            if n > capacity:
                break
    out["flushes"].append(n - n_flushed)
    out["count"] = n
    return out


# ---------------------------------------------------------------------------------------------------------------------
# exact values and the Horner bound

def _ff(j, k):
    v = 1
    for q in range(k):
        v *= j - q
    return v


_FF = [[_ff(j, k) for j in range(N_COEFF)] for k in range(N_ORDERS)]


def _dyadic(x):
    """a finite double as (integer, exponent): x = integer * 2^exponent"""
    n, d = float(x).as_integer_ratio()
    return n, -(d.bit_length() - 1)


def _horner_int(ints, exps, t, order, absolute):
    """sum_j ff(j, order) c_j t^(j - order) (or of the absolute values) as (integer, exponent of 2); c_j = ints[j] * 2^exps[j]"""
    a, e = t if isinstance(t, tuple) else _dyadic(t)
    if absolute:
        a = abs(a)
    q = min(exps)
    ff = _FF[order]
    # c_j = n_j 2^q, t = a 2^e: the sum is 2^q sum_j ff n_j a^p 2^(e p), p = j - order; with e >= 0 an integer Horner chain in
    # a 2^e, with e < 0 one in a whose coefficients carry 2^(-e (deg - p))
    deg = N_COEFF - 1 - order
    acc = 0
    for j in range(N_COEFF - 1, order - 1, -1):
        nj = ints[j] << (exps[j] - q)
        if absolute:
            nj = abs(nj)
        term = ff[j] * nj
        if e >= 0:
            acc = acc * (a << e) + term
        else:
            acc = acc * a + (term << (-e * (deg - (j - order))))
    return acc, (q if e >= 0 else q + e * deg)


def _horner_exact(ints, exps, t, order, absolute):
    acc, scale = _horner_int(ints, exps, t, order, absolute)
    return Fraction(acc * (1 << scale), 1) if scale >= 0 else Fraction(acc, 1 << -scale)


def split_segment(coeffs_seg):
    """a segment's [4][10] coefficients as exact integers and exponents (what state_errors takes in place of the doubles)"""
    return _split(coeffs_seg)


def _split(coeffs_seg):
    c = np.asarray(coeffs_seg, dtype=np.float64).reshape(N_DIM, N_COEFF)
    return [tuple(zip(*(_dyadic(x) for x in c[d]))) for d in range(N_DIM)]


def wrap_exact(y):
    """a rational brought into (-pi, pi] by a multiple of 2 pi"""
    pi = pi_exact()
    k = math.ceil((y - pi) / (2 * pi))
    return y - 2 * pi * k


def exact_state(coeffs_seg, t, order):
    """the four dimensions' sum_j j!/(j-k)! c_j t^(j-k) of one segment ([4][10] coefficients) as exact rationals; the heading
    of order 0 reduced to (-pi, pi] (with pi wrong by < 2^-300)"""
    v = [_horner_exact(ints, exps, t, order, False) for ints, exps in _split(coeffs_seg)]
    if order == 0:
        v[3] = wrap_exact(v[3])
    return v


def gamma(n):
    return Fraction(n, 2 ** 53 - n)   # n u / (1 - n u)


def horner_bound(coeffs_seg, t, order):
    """gamma_{2 (9 - order) + 1} sum_j ff(j, order) |c_j| |t|^(j - order) per dimension: the bound of a Horner chain of degree
    9 - order (two roundings per step, or one where the step is fused) whose coefficients ff c are rounded once (Higham,
    Accuracy and Stability of Numerical Algorithms, section 5.1).  The heading of order 0 gets 2 u pi on top: its wrap is two
    fused multiply-adds whose results are at most pi."""
    g = gamma(2 * (N_COEFF - 1 - order) + 1)
    b = [g * _horner_exact(ints, exps, t, order, True) for ints, exps in _split(coeffs_seg)]
    if order == 0:
        b[3] += 2 * U * pi_exact()
    return b


def heading_limits(coeffs_path, segments, taus):
    """the largest |wrapped heading| of order 0 that wrap_heading may return at each sample (segments [n], taus [n]; coeffs_path
    [S][4][10]), as doubles.  The Horner value y has |y| <= (1 + gamma_19) M, M = sum_j |c_j| |t|^j; k = rint(fl(y fl(1 / 2 pi)))
    leaves |y - 2 pi k| <= pi + |y| (2 u + u^2); the two fused multiply-adds by the halves of 2 pi round twice more.  All of it
    is below pi (1 + 3 u) + 3 u M.  (M in doubles is right to 1e-15 of itself, far inside the step from 2 u to 3 u.)"""
    u = 2.0 ** -53
    a = np.abs(np.asarray(coeffs_path, dtype=np.float64)[np.asarray(segments, dtype=np.int64), 3, :])
    t = np.abs(np.asarray(taus, dtype=np.float64))
    m = np.zeros(t.shape)
    for j in range(N_COEFF - 1, -1, -1):
        m = m * t + a[:, j]
    return math.pi * (1.0 + 3.0 * u) + 3.0 * u * m


_GAMMA = [float(gamma(2 * (N_COEFF - 1 - k) + 1)) for k in range(N_ORDERS)]


def state_errors(coeffs_seg, t, got):
    """got [5][4] (doubles; or [1][4], order 0 alone) against exact_state: -> observed error / horner_bound as floats (inf where got is not
    finite; 0 where the error is 0); the heading of order 0 is compared modulo 2 pi.  A ratio is the correctly rounded quotient
    of two exact integers divided by the double nearest gamma: right to 2^-52, so a value at or below 1 - 2^-50 is inside the
    bound (what the tests assert)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, N_DIM).tolist()
    parts = coeffs_seg if isinstance(coeffs_seg, list) else _split(coeffs_seg)   # (a caller may split a segment once)
    ratios = np.zeros((len(got), N_DIM))
    t = _dyadic(t)
    for k in range(len(got)):
        g = _GAMMA[k]
        for d, (ints, exps) in enumerate(parts):
            if not math.isfinite(got[k][d]):
                ratios[k, d] = math.inf
                continue
            if k == 0 and d == 3:
                two_pi = 2 * pi_exact()
                err = abs(Fraction(got[k][d]) - _horner_exact(ints, exps, t, 0, False)) % two_pi
                err = min(err, two_pi - err)
                ratios[k, d] = float(err / (gamma(2 * N_COEFF - 1) * _horner_exact(ints, exps, t, 0, True) + 2 * U * pi_exact()))
                continue
            acc, scale = _horner_int(ints, exps, t, k, False)
            mag, _ = _horner_int(ints, exps, t, k, True)
            gn, ge = _dyadic(got[k][d])
            low = min(scale, ge)
            err = abs((gn << (ge - low)) - (acc << (scale - low)))
            ratios[k, d] = 0.0 if err == 0 else (math.inf if mag == 0 else err / (mag << (scale - low)) / g)
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# the cases

def _drawn(n, seed, lo=0.01, hi=0.6):
    rng = SplitMix64(seed)
    return [rng.uniform(lo, hi) for _ in range(n)]


def _table_edge(n):
    return [n * TABLE_DT - TABLE_DT / 2]   # (both terms and the difference are exact)


# name, seg_times, dt, and the edges the case is there for: {key of case_edges(): its count}.  The order is the batch's:
# long, short, long.
CASES = [
    ("drawn_256", _drawn(256, 9001), 0.2, dict(segments=256, samples=408, multi_carries=21, flushes_at_192=1, misfit_flushes=1)),
    ("tenths_dt_tenth", [0.1] * 30, 0.1, dict(samples=30, boundary_hits=29, t_end_on_grid=1)),
    ("tenths_dt_fifth", [0.1] * 30, 0.2, dict(samples=15, multi_carries=13, past_end=1)),
    ("quarters", [0.5, 0.25, 1.0, 0.25], 0.25, dict(samples=8, boundary_hits=3, t_end_on_grid=1)),
    ("sub_dt_middle", [1.0, 0.03, 0.04, 0.05, 1.0], 0.2, dict(samples=11, multi_carries=1, longest_carry=4)),
    ("zero_lengths", [0, 0, 1, 0, 1], 0.25, dict(samples=8, zero_segments_passed=3, boundary_hits=1, multi_carries=1)),
    ("chunk_61_to_66", [15.25, 15.5, 15.75, 16.0, 16.25, 16.5], 0.25,
     dict(samples=381, boundary_hits=5, chunks_last_63=6, full_chunks=3, chunks_m_62_to_64=6, misfit_flushes=2)),
    ("hundredths", [0.64, 0.63, 0.65], 0.01, dict(samples=192, chunks_last_63=3, full_chunks=2, buffer_full_at_end=1)),
    ("eight_of_50", [12.5] * 8, 0.25, dict(samples=400, boundary_hits=7, misfit_flushes=2)),
    ("drawn_121", _drawn(121, 9002), 0.2, dict(segments=121, samples=180, multi_carries=15)),
    ("millis_200", [1e-3] * 200, 0.2, dict(samples=2, longest_carry=199)),
    ("halves_dt_one", [0.5, 0.5], 1.0, dict(samples=1, t_end_on_grid=1, t_end_is_dt=1)),
    ("below_dt", [0.3, 0.3], 1.0, dict(samples=1, t_end_below_dt=1)),
    ("one_of_300", [60.0], 0.2, dict(samples=300, full_chunks=4, flushes_at_192=1)),
    ("no_sample", [0, 0], 0.2, dict(no_sample=1, zero_segments_passed=2)),
    ("nan_time", [0.5, float("nan"), 0.5], 0.2, dict(no_sample=1)),
    ("infinite_last", [0.5, float("inf")], 0.2, dict(never_ends=1)),
] + [("table_%d" % n, _table_edge(n), TABLE_DT, dict(samples=n)) for n in (1024, 1025, 1103, 1104, 1105, 3000)]

SWEEP_TURNS = 5   # how often the heading of a finite case goes round over the path


def case_coeffs(index):
    """[S][4][10] of case `index`: not solved, mixed signs, |c_j| ~ 10^(3 - 2 j / 3) (1e3 for c_0 down to 1e-3 for c_9) times a
    factor in [0.5, 2], divided by max(1, T)^j so that a long segment's polynomial stays of the size of its c_0.  The heading is
    a ramp of SWEEP_TURNS turns over the path (c_0 continuous from segment to segment, c_1 the rate) with the same family of
    higher coefficients 1e-3 times as large: it passes +-pi again and again."""
    name, seg_times, dt, _ = CASES[index]
    rng = SplitMix64(7700 + index)
    S = len(seg_times)
    finite = [t for t in seg_times if math.isfinite(t)]
    total = sum(finite) if len(finite) == S else 0.0
    rate = SWEEP_TURNS * 2 * math.pi / total if total > 0 else 1.0
    c = np.zeros((S, N_DIM, N_COEFF))
    start = 0.0
    for s, T in enumerate(seg_times):
        ref = max(1.0, T) if math.isfinite(T) else 1000.0
        for d in range(N_DIM):
            for j in range(N_COEFF):
                mag = 10.0 ** (3.0 - 2.0 * j / 3.0) * rng.uniform(0.5, 2.0) / ref ** j
                c[s, d, j] = mag if rng.uniform(0.0, 1.0) < 0.5 else -mag
        c[s, 3] *= 1e-3
        c[s, 3, 0] = -3.0 + rate * start
        c[s, 3, 1] = rate
        if math.isfinite(T):
            start += T
    return c


def case_edges(seg_times, dt, capacity=STANDARD_CAPACITIES[-1]):
    """the counts a case is asserted to have (test_sampler_walk_cases.py): the reference's walk's and the kernel's chunking's"""
    samples, count, e = _walk(seg_times, dt, capacity)
    m = chunk_model(seg_times, dt, capacity)
    t_end = 0.0
    for x in seg_times:
        t_end += float(x)
    e = dict(e)
    e.update(segments=len(seg_times), samples=count, no_sample=int(count == 0), never_ends=int(count == capacity + 1 and math.isinf(t_end)),
             t_end_on_grid=int(e["t_end_on_grid"]), t_end_below_dt=int(0.0 < t_end < dt), t_end_is_dt=int(t_end == dt), past_end=int(e["past_end"]),
             chunks_last_63=sum(1 for _, last, _m in m["chunks"] if last == 63),
             full_chunks=sum(1 for _, last, mm in m["chunks"] if mm == last + 1),
             chunks_m_62_to_64=sum(1 for _, _l, mm in m["chunks"] if 62 <= mm <= 64),
             flushes_at_192=sum(1 for f in m["flushes"][:-1] if f == SAMPLE_BUFFER),
             buffer_full_at_end=int(m["flushes"][-1] == SAMPLE_BUFFER), misfit_flushes=m["misfit_flushes"])
    return e


def case_capacities(index):
    """the capacities case `index` is sampled at on the GPU: the standard ones and its own N - 1, N, N + 1; the table-edge
    cases stay at or below TABLE_CAPACITY (a larger capacity would grow their table)"""
    _, seg_times, dt, _ = CASES[index]
    n = replay(seg_times, dt, STANDARD_CAPACITIES[-1] + 2)[1]
    caps = set(STANDARD_CAPACITIES) | {c for c in (n - 1, n, n + 1) if 1 <= c <= STANDARD_CAPACITIES[-1]}
    if dt == TABLE_DT:
        caps = {c for c in caps if c <= TABLE_CAPACITY} | {TABLE_CAPACITY - 1, TABLE_CAPACITY}
    return sorted(caps)


def dt_capacities(dt):
    """the capacities the GPU test samples the whole batch at with sampling period dt: those of every case whose dt it is"""
    caps = set()
    for i, c in enumerate(CASES):
        if c[2] == dt:
            caps |= set(case_capacities(i))
    return sorted(caps)
