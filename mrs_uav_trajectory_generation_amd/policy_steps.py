"""The reference's optimize() (src/mrs_trajectory_generation.cpp:620-851) composed from plan steps, the waypoints on the device
from the request to the answer:

    thinning (Plan.preprocess_path) -> per round: heading unwrap (Plan.unwrap_headings), the vertices findTrajectory builds
    (:923-977, torch on the device, requests without an initial state), the Baca estimate (Plan.estimate_times_baca), the solve
    with its samples (Plan.solve), both gates (Plan.length_gate on the solve's status), the deviation scan (Plan.path_deviation),
    the mid-points of the unsafe segments (Plan.insert_midpoints), the plan of the next round.

With policy.fallback_sampling a round's solve and both gates give way to the reference's findTrajectoryFallback (:1215-1395),
from the steps that exist: the heading unwrap, the limits scaled by fallback_speed_factor and fallback_accel_factor, the Baca
estimate of that, and Plan.fallback_sample on the RAW waypoints with stop_at and fallback_stopping_time; a path is ok when its
rows fit the capacity; the deviation scan and the mid-points go on as before.  With policy.override_heading_atan2 the finished
samples get getTrajectoryReference's heading along the direction of travel (:1578-1603) where they are: ONE Plan.travel_heading
over samples_out in place, behind the rounds, on the device's success and n_samples.

Per round ONE readback: the offsets of the subdivided batch with the verdicts (a few words per path).  The rounds end as :729
does: round max_deviation_iterations is solved and not validated again.  mrs_tg_optimize_paths does not run through this module;
it is the same loop with the two edit stages on the host, and tests/test_gpu_pathedit_loop.py holds the two to the same answers.
Not here: initial states and a time budget (max_execution_time_s > 0 is refused)."""
import ctypes as C

import numpy as np
import torch

from . import api

_FLT_MAX = 3.4028234663852886e+38   # (double)FLT_MAX: a relaxed heading's limits (:1030-1038)
MAX_SEGMENTS = 256                  # MRS_TG_MAX_SEGMENTS: the longest path a plan takes


def _vertices(so, unwrapped, stop, d):
    """mask [sum V][5], values [sum V][5][4] as policy::build_vertices builds them without an initial state: every vertex
    constrains its position, the ends their derivatives 1 .. d to zero, a stop_at vertex between them its derivatives 1 .. 3"""
    dev = unwrapped.device
    n_v = unwrapped.shape[0]
    first = torch.as_tensor(so[:-1] + np.arange(so.size - 1), dtype=torch.int64, device=dev)
    last = torch.as_tensor(so[1:] + np.arange(so.size - 1), dtype=torch.int64, device=dev)
    end = torch.zeros(n_v, dtype=torch.bool, device=dev)
    end[first] = True
    end[last] = True
    mask = torch.zeros((n_v, 5), dtype=torch.uint8, device=dev)
    mask[:, 0] = 1
    mask[:, 1:d + 1] = end[:, None].to(torch.uint8)
    mask[:, 1:4] |= ((stop != 0) & ~end)[:, None].to(torch.uint8)
    vals = torch.zeros((n_v, 5, api.N_DIM), dtype=torch.float64, device=dev)
    vals[:, 0, :] = unwrapped
    return mask, vals


def optimize_paths(ctx, paths, limits=None, stop_flags=None, relax_heading=None, policy=None, sample_capacity=4096):
    """optimize() for a list of waypoint paths ([n][4] arrays, n >= 2) -> dict(success, n_samples, max_deviation, n_waypoints,
    iterations: numpy [P]; samples: a device tensor [P][sample_capacity][4], rows behind a path's n_samples are zero), the
    fields of api.optimize_paths."""
    from .problem import DEFAULT_LIMITS
    pol = policy or api.default_policy_options()
    P, cap = len(paths), int(sample_capacity)
    d, dt = int(pol.solver.derivative_to_optimize), float(pol.solver.sampling_dt)
    if pol.max_execution_time_s > 0:
        raise ValueError("policy_steps has no clock: a time budget (max_execution_time_s > 0) is not served")
    if not dt > 0 or not 2 <= d <= 4 or cap <= 0:
        raise ValueError("sampling_dt > 0, derivative_to_optimize in 2 .. 4 and sample_capacity > 0 are required")
    arrs = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 4) for p in paths]
    if any(a.shape[0] < 2 for a in arrs):
        raise ValueError("every path needs two waypoints")
    dev = torch.device("cuda", torch.cuda.current_device())
    stops = [np.zeros(a.shape[0], dtype=np.uint8) if stop_flags is None else np.asarray(stop_flags[p], dtype=np.uint8)
             for p, a in enumerate(arrs)]
    any_stop = any(bool(s[1:-1].any()) for s in stops)
    lim = np.ascontiguousarray(np.tile(DEFAULT_LIMITS, (P, 1)) if limits is None else limits, dtype=np.float64).reshape(P, 9).copy()
    if relax_heading is not None:
        lim[np.asarray(relax_heading, dtype=bool)[:, None] & np.isin(np.arange(9), (2, 5, 8))[None, :]] = _FLT_MAX
    success = np.zeros(P, dtype=np.int32)
    n_samples = np.zeros(P, dtype=np.int32)
    max_dev = np.zeros(P)
    n_wp = np.zeros(P, dtype=np.int32)
    iters = np.zeros(P, dtype=np.int32)
    samples_out = torch.zeros((P, cap, api.N_DIM), dtype=torch.float64, device=dev)
    if P == 0:
        return dict(success=success, n_samples=n_samples, samples=samples_out, max_deviation=max_dev, n_waypoints=n_wp,
                    iterations=iters)
    ctx.use_torch_stream()

    # ---- preprocessPath (:431-500) where the waypoints are
    so = np.concatenate([[0], np.cumsum([a.shape[0] - 1 for a in arrs])]).astype(np.int32)
    wp = torch.from_numpy(np.concatenate(arrs)).to(dev)
    stop = torch.from_numpy(np.concatenate(stops)).to(dev)
    plan = api.Plan(ctx, so)
    try:
        offsets = torch.empty(P + 1, dtype=torch.int32, device=dev)
        rows, stop_rows = torch.empty_like(wp), torch.empty_like(stop)
        plan.preprocess_path(wp, offsets, rows, min_waypoint_distance=pol.min_waypoint_distance, stop_at=stop,
                             straightener_enabled=bool(pol.path_straightener_enabled),
                             straightener_max_deviation=pol.path_straightener_max_deviation,
                             straightener_max_hdg_deviation=pol.path_straightener_max_hdg_deviation, stop_at_out=stop_rows)
        off = offsets.cpu().numpy().astype(np.int64)
    finally:
        plan.close()
    wp, stop = rows[:off[-1]], stop_rows[:off[-1]]
    ids = np.arange(P)                                   # the request every path of the round's batch answers
    so = (off - np.arange(P + 1)).astype(np.int32)
    n_wp[:] = np.diff(off)
    lim_d = torch.from_numpy(lim).to(dev)

    opt = api.Options.from_buffer_copy(pol.solver)
    opt.estimate_times = 1
    opt.sample_capacity = cap
    if pol.max_trajectory_len_factor > 0:                # the length gate is the reference's answer to a runaway (:1178-1199)
        opt.flags |= api.FLAG_REFERENCE_STATUS           # where its upper side runs; else the product's own rule (-4) answers
    if any_stop and d == 4:
        opt.flags |= api.FLAG_CONSTRAINED_SLOTS

    for rnd in range(int(pol.max_deviation_iterations) + 1):
        # a path subdivided beyond the longest one a plan takes fails on its own (the reference has no such limit)
        fits = np.diff(so) <= MAX_SEGMENTS
        if not fits.all():
            keep = np.flatnonzero(fits)
            vtx = np.concatenate([np.arange(so[a] + a, so[a + 1] + a + 1) for a in keep]) if keep.size else np.zeros(0, dtype=np.int64)
            vtx = torch.from_numpy(vtx).to(dev)
            wp, stop, lim_d = wp[vtx], stop[vtx], lim_d[torch.from_numpy(keep).to(dev)]
            so = np.concatenate([[0], np.cumsum(np.diff(so)[keep])]).astype(np.int32)
            ids = ids[keep]
        A = ids.size
        if A == 0:
            break
        last_round = rnd == int(pol.max_deviation_iterations)
        n_s, n_v = int(so[-1]), int(so[-1]) + A
        plan = api.Plan(ctx, so)
        try:
            unwrapped = torch.empty_like(wp)
            plan.unwrap_headings(wp.contiguous(), unwrapped)                                 # :925-936
            baca = torch.empty(n_s, dtype=torch.float64, device=dev)
            ns = torch.zeros(A, dtype=torch.int32, device=dev)
            samples = torch.zeros((A, cap, api.N_DIM), dtype=torch.float64, device=dev)
            if pol.fallback_sampling:                                                        # findTrajectoryFallback, :1215-1395
                lim_fb = lim_d.clone()
                lim_fb[:, 0:2] *= float(pol.fallback_speed_factor)
                lim_fb[:, 3:5] *= float(pol.fallback_accel_factor)
                plan.estimate_times_baca(unwrapped, lim_fb, baca)
                plan.fallback_sample(wp.contiguous(), baca, dt, cap, ns, samples, stop_at=stop.contiguous(),
                                     stopping_time=pol.fallback_stopping_time)
                ok = ns <= cap
            else:
                mask, vals = _vertices(so.astype(np.int64), unwrapped, stop, d)              # :923-977
                plan.estimate_times_baca(unwrapped, lim_d, baca)                             # initial_total_time_baca, :1048-1056
                times = torch.zeros(n_s, dtype=torch.float64, device=dev)
                coeffs = torch.empty((n_s, api.N_DIM, api.N_COEFF), dtype=torch.float64, device=dev)
                status = torch.zeros(A, dtype=torch.int32, device=dev)
                cost = torch.zeros(A, dtype=torch.float64, device=dev)
                plan.solve(opt, mask, vals, times, coeffs, status, cost=cost, waypoints=unwrapped, limits=lim_d, n_samples=ns,
                           samples=samples)
                verdict = torch.empty(A, dtype=torch.int32, device=dev)
                plan.length_gate(baca, ns, dt, max_factor=pol.max_trajectory_len_factor,
                                 min_factor=pol.min_trajectory_len_factor, status=status, verdict=verdict)   # :1138-1149, :1178-1199
                ok = (verdict == api.FIND_ACCEPTED) & (ns <= cap)
            worst = torch.zeros(A, dtype=torch.float64, device=dev)
            go_on = torch.zeros(A, dtype=torch.bool, device=dev)
            offsets = torch.zeros(A + 1, dtype=torch.int32, device=dev)
            if not last_round:
                seg_max = torch.empty(n_s, dtype=torch.float64, device=dev)
                plan.path_deviation(samples, ns, wp.contiguous(), first_segment=bool(pol.max_deviation_first_segment),
                                    status=ok.to(torch.int32), max_deviation=worst, segment_max=seg_max)   # :1401-1455
                path_of_segment = torch.repeat_interleave(torch.arange(A, device=dev),
                                                          torch.from_numpy(np.diff(so).astype(np.int64)).to(dev), output_size=n_s)
                unsafe = torch.zeros(A, dtype=torch.int32, device=dev).index_add_(0, path_of_segment,
                                                                                 (seg_max > pol.max_deviation).to(torch.int32)) > 0
                go_on = ok & unsafe if pol.check_deviation_enabled else go_on
                rows = torch.empty((n_v + n_s, api.N_DIM), dtype=torch.float64, device=dev)
                stop_rows = torch.empty(n_v + n_s, dtype=torch.uint8, device=dev)
                plan.insert_midpoints(wp.contiguous(), seg_max, pol.max_deviation, offsets, rows,
                                      first_segment=bool(pol.max_deviation_first_segment), stop_at=stop.contiguous(),
                                      active=go_on.to(torch.uint8), stop_at_out=stop_rows)   # :739-753
            # the round's one readback: the next batch's offsets and a few words per path
            words = torch.cat([offsets.to(torch.float64), ok.to(torch.float64), go_on.to(torch.float64), ns.to(torch.float64),
                               worst]).cpu().numpy()
        finally:
            plan.close()
        off = words[:A + 1].astype(np.int64)
        ok_h, go_h = words[A + 1:2 * A + 1] != 0, words[2 * A + 1:3 * A + 1] != 0
        ns_h, worst_h = words[3 * A + 1:4 * A + 1].astype(np.int32), words[4 * A + 1:]
        success[ids] = ok_h
        n_samples[ids] = np.where(ok_h, ns_h, 0)
        if not last_round:
            max_dev[ids[ok_h]] = worst_h[ok_h]
        done = np.flatnonzero(ok_h & ~go_h)
        if done.size:      # the finished paths' samples stay where they are: on the device
            samples_out[torch.from_numpy(ids[done]).to(dev)] = samples[torch.from_numpy(done).to(dev)]
        if last_round:
            break
        keep = np.flatnonzero(go_h)
        iters[ids[keep]] = rnd + 1
        n_wp[ids[keep]] = np.diff(off)[keep]
        if keep.size == 0:
            break
        vtx = torch.from_numpy(np.concatenate([np.arange(off[a], off[a + 1]) for a in keep])).to(dev)
        wp, stop, lim_d = rows[vtx], stop_rows[vtx], lim_d[torch.from_numpy(keep).to(dev)]
        so = np.concatenate([[0], np.cumsum(np.diff(off)[keep] - 1)]).astype(np.int32)
        ids = ids[keep]
    # a path that was still being subdivided when it outgrew a plan, or whose rounds ran out, keeps what the loop left it
    lost = np.setdiff1d(np.arange(P), np.flatnonzero(success))
    n_samples[lost] = 0
    if pol.override_heading_atan2:                       # getTrajectoryReference :1578-1603, where the samples are
        plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
        try:
            plan.travel_heading(samples_out, torch.from_numpy(n_samples).to(dev), status=torch.from_numpy(success).to(dev))
        finally:
            plan.close()
    return dict(success=success, n_samples=n_samples, samples=samples_out, max_deviation=max_dev, n_waypoints=n_wp,
                iterations=iters)
