#!/usr/bin/env python3
"""Generate tests/golden/refine_cases.json: 60-digit solutions of ill-conditioned linear QPs for MRS_TG_FLAG_REFINE.

The condition number of R_pp grows like (T_max / T_min)^(2d - 1) between neighbouring segments, so these paths put one short
segment among long ones.  Every case is solved by oracle/gen_golden.py's exact_solve (60-digit mpmath, the reference's
formulas) through its case_record; nothing of that module is changed.  Cases:

  * neighbour ratios of 50 and 100 (cond 1e12 .. 1e14) under d = 4, 3 and 2;
  * a 30- and a 60-segment path with one short segment;
  * interior stop_at vertices (velocity .. snap constrained to zero) next to a short segment;
  * a vertex whose position is free (MRS_TG_FLAG_GENERAL_PATTERNS);
  * free end derivatives (the last vertex constrains its position only);
  * "short_0p01_between_4s": a 0.01 s segment between 4 s ones ((T_max / T_min)^7 ~ 1e18): the refinement still converges
    (Cholesky is blind to the symmetric diagonal scaling behind most of that figure);
  * "guard_1em4_between_10s": a 1e-4 s segment between 10 s ones ((T_max / T_min)^7 ~ 1e35), where corrections solved in
    double stop lowering the residual before the solution is reached: the refinement's guard refuses such a step and keeps
    the previous iterate.  Beyond the 113-bit route's reach as well; the 60 digits of the fixture leave 25.

Run from the repo root:  python3 tests/golden/gen_refine_cases.py   (a few minutes: the 60-segment case dominates)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from mrs_uav_trajectory_generation_amd import problem as pr  # noqa: E402
from oracle.gen_golden import case_record, euclid_times  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "refine_cases.json")
GUARD_CASE = "guard_1em4_between_10s"


def short_segment_path(n_seg, seed, d, short_at, ratio, stop_at=None):
    """Box waypoints, Euclidean times, then segment `short_at` set to (mean of its neighbours) / ratio"""
    wp0 = pr.random_box_waypoints(n_seg, seed)
    wp, m, v = pr.build_vertices(wp0, d, stop_at=stop_at)
    t = [float(x) for x in euclid_times(wp, pr.DEFAULT_LIMITS)]
    nb = [t[i] for i in (short_at - 1, short_at + 1) if 0 <= i < n_seg]
    t[short_at] = float(np.mean(nb)) / ratio
    return wp, m, v, t


def cases():
    out = []
    for d in (4, 3, 2):
        for ratio in (50, 100):
            wp, m, v, t = short_segment_path(10, 100 + d, d, 4, ratio)
            out.append(case_record("ratio%d_d%d" % (ratio, d), wp, m, v, t, d))
    wp, m, v, t = short_segment_path(30, 130, 4, 17, 30)
    out.append(case_record("seg30_short", wp, m, v, t, 4))
    wp, m, v, t = short_segment_path(60, 160, 4, 41, 30)
    out.append(case_record("seg60_short", wp, m, v, t, 4))
    stop = [False] * 11
    stop[3] = stop[7] = True
    wp, m, v, t = short_segment_path(10, 170, 4, 5, 50, stop_at=stop)
    out.append(case_record("stop_at_interior", wp, m, v, t, 4))
    wp, m, v, t = short_segment_path(10, 180, 4, 6, 50)
    m = m.copy()
    v = v.copy()
    m[3, 0] = 0       # vertex 3 leaves its position free
    v[3, 0, :] = 0.0
    out.append(case_record("position_free_vertex", wp, m, v, t, 4))
    wp, m, v, t = short_segment_path(10, 190, 3, 8, 50)
    m = m.copy()
    v = v.copy()
    m[-1, 1:] = 0     # the end vertex constrains its position only
    v[-1, 1:, :] = 0.0
    out.append(case_record("free_end_derivatives", wp, m, v, t, 3))
    wp, m, v, _ = short_segment_path(6, 200, 4, 3, 1)
    t = [4.0, 4.0, 4.0, 0.01, 4.0, 4.0]
    out.append(case_record("short_0p01_between_4s", wp, m, v, t, 4))
    wp, m, v, _ = short_segment_path(4, 200, 4, 2, 1)
    t = [10.0, 10.0, 1e-4, 10.0]
    out.append(case_record(GUARD_CASE, wp, m, v, t, 4))
    return out


def main():
    cs = cases()
    with open(OUT, "w") as f:
        json.dump(dict(generator="tests/golden/gen_refine_cases.py", mp_dps=60, limits=pr.DEFAULT_LIMITS.tolist(), cases=cs), f)
    print("wrote", len(cs), "cases to", OUT)


if __name__ == "__main__":
    main()
