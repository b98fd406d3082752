"""The reference's optimize() (src/mrs_trajectory_generation.cpp:620-851) composed from plan steps, the waypoints on the device
from the request to the answer:

    thinning (Plan.preprocess_path) -> per round: the vertices findTrajectory builds, their headings unwrapped from the initial
    state's (:923-977, Plan.request_vertices, one launch), the Baca estimate (Plan.estimate_times_baca), the solve
    with its samples (Plan.solve), both gates (Plan.length_gate on the solve's status), the deviation scan (Plan.path_deviation),
    the mid-points of the unsafe segments (Plan.insert_midpoints), the plan of the next round.

With policy.fallback_sampling a round's solve and both gates give way to the reference's findTrajectoryFallback (:1215-1395),
from the steps that exist: the heading unwrap, the limits scaled by fallback_speed_factor and fallback_accel_factor, the Baca
estimate of that, and Plan.fallback_sample on the RAW waypoints with stop_at and fallback_stopping_time; a path is ok when its
rows fit the capacity; the deviation scan and the mid-points go on as before.  With policy.override_heading_atan2 the finished
samples get getTrajectoryReference's heading along the direction of travel (:1578-1603) where they are: ONE Plan.travel_heading
over samples_out in place, behind the rounds, on the device's success and n_samples.

Where the trajectory starts comes in one of two ways.  initial_states= (as api.optimize_paths takes them): the first waypoint of
a path is its initial condition, the vertices fix velocity, acceleration and jerk there and the unwrap starts from the state's
heading.  initial= (the arrays of Plan.initial_condition and the prediction's age): prepareInitialCondition (:506-614) and the
edit of :649-672 run on the device in front of the thinning (Plan.initial_condition, Plan.prepend_initial_condition), a request of
ONE goal waypoint is the normal case, a path from the future is sampled at 0.2 s (:692-697; one solve has one sampling_dt, so
those paths run the rounds as a group of their own when the policy's sampling_dt is another), and behind the rounds and the
heading override the prediction is spliced in front where the samples are (Plan.splice_prediction, :801-840).  A path with fewer
than two vertices after the prepend or after the thinning fails ("the path is empty (after postprocessing)") and never reaches
a plan; an invalid decision, a prediction shorter than k and a spliced count above the capacity fail their request.

With policy.max_execution_time_s > 0 the host clock is read where each round starts, as mrs_tg_optimize_paths reads it: over
the budget (overtime(), :1730-1743) the round's still-active paths take the fallback sampler and succeed; otherwise the solve
runs under max_time_s = 2 * 0.95 * the time left (:899), and a path whose round's readback arrives after the deadline fails.

Per round ONE readback: the offsets of the subdivided batch with the verdicts (a few words per path).  The rounds end as :729
does: round max_deviation_iterations is solved and not validated again.  mrs_tg_optimize_paths does not run through this module;
it is the same loop with the two edit stages on the host, and tests/test_gpu_pathedit_loop.py holds the two to the same answers."""
import ctypes as C
import time

import numpy as np
import torch

from . import api

_FLT_MAX = 3.4028234663852886e+38   # (double)FLT_MAX: a relaxed heading's limits (:1030-1038)
MAX_SEGMENTS = 256                  # MRS_TG_MAX_SEGMENTS: the longest path a plan takes


FUTURE_SAMPLING_DT = 0.2            # sampling_dt of a path from the future (:692-697)


def _as_device(a, dtype, dev):
    """a numpy array or a device tensor -> a contiguous device tensor of dtype"""
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype).contiguous()


def _request_limits(ctx, pol, constraints, override, override_flags, state, P, dev):
    """[P][2][9]: findTrajectory's limits (:981-1038) and findTrajectoryFallback's (:1252-1299) of every request, one
    Plan.request_limits each, from constraints [P][12], override [P][6] and override_flags [P] (api.REQ_*)"""
    c = _as_device(constraints, torch.float64, dev).reshape(P, 12)
    flags = None if override_flags is None else _as_device(override_flags, torch.int32, dev).reshape(P)
    o = None if override is None else _as_device(override, torch.float64, dev).reshape(P, 6)
    if flags is None and o is not None:
        raise ValueError("override= needs override_flags= (api.REQ_OVERRIDE where it applies)")
    if flags is not None and o is None:
        if bool((flags & api.REQ_OVERRIDE).any()):
            raise ValueError("override_flags asks for an override: give override=")
        o = torch.zeros((P, 6), dtype=torch.float64, device=dev)
    has, rows = (None, None) if state is None else (state[0].to(torch.uint8).contiguous(), state[1].contiguous())
    both = torch.empty((2, P, 9), dtype=torch.float64, device=dev)
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))   # (the step takes the path count and the context from it)
    try:
        plan.request_limits(c, both[0], override=o, flags=flags, has_state=has, state=rows)
        plan.request_limits(c, both[1], override=o, flags=flags, has_state=has, state=rows, fallback=True,
                            speed_factor=float(pol.fallback_speed_factor), accel_factor=float(pol.fallback_accel_factor))
    finally:
        plan.close()
    return both.permute(1, 0, 2).contiguous()


def optimize_paths(ctx, paths, limits=None, stop_flags=None, relax_heading=None, policy=None, sample_capacity=4096,
                   initial_states=None, has_initial_state=None, initial=None, constraints=None, override=None,
                   override_flags=None):
    """optimize() for a list of waypoint paths ([n][4] arrays, n >= 2; n >= 1 with initial=) -> dict(success, n_samples,
    max_deviation, n_waypoints, iterations: numpy [P]; samples: a device tensor [P][sample_capacity][4], rows behind a path's
    n_samples are zero), the fields of api.optimize_paths.
    initial_states: per path None or dict(heading, velocity, acceleration, jerk) as api.optimize_paths takes it (has_initial_state
    [P], optional, switches single ones off): the path's first waypoint is its initial condition.
    initial: dict(flags [P] int32, tracker [P][4][4], tracker_age [P], uav_pose [P][4], takeoff_height, path_time_offset [P],
    prediction = (position, velocity, acceleration, jerk), each [P][pred_capacity][4], n_pred [P] int32, prediction_age [P]) of
    numpy arrays or device tensors, the arguments of Plan.initial_condition and Plan.splice_prediction: the initial condition is
    decided, prepended and spliced on the device.  With it the result also has decision and sample_offset (numpy [P]).
    constraints [P][12], override [P][6], override_flags [P] (api.REQ_OVERRIDE, api.REQ_RELAX_HEADING), in place of limits= and
    relax_heading=: the limits of the solve and of the fallback sampler are derived on the device as findTrajectory and
    findTrajectoryFallback derive them (Plan.request_limits, once each), the override tested against the initial state."""
    from .problem import DEFAULT_LIMITS
    if constraints is None and (override is not None or override_flags is not None):
        raise ValueError("override= and override_flags= go with constraints=")
    if constraints is not None and (limits is not None or relax_heading is not None):
        raise ValueError("constraints= and limits= / relax_heading= are two ways to give the limits: give one")
    pol = policy or api.default_policy_options()
    P, cap = len(paths), int(sample_capacity)
    d, dt = int(pol.solver.derivative_to_optimize), float(pol.solver.sampling_dt)
    t_begin = time.monotonic()
    if not dt > 0 or not 2 <= d <= 4 or cap <= 0:
        raise ValueError("sampling_dt > 0, derivative_to_optimize in 2 .. 4 and sample_capacity > 0 are required")
    if initial is not None and initial_states is not None:
        raise ValueError("initial_states and initial are two ways to say where the trajectory starts: give one")
    arrs = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 4) for p in paths]
    if any(a.shape[0] < (1 if initial is not None else 2) for a in arrs):
        raise ValueError("every path needs two waypoints" if initial is None else "every path needs a waypoint")
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
    budget = float(pol.max_execution_time_s)

    def elapsed():
        return time.monotonic() - t_begin

    def overtime():                                      # overtime() :1730-1743
        return budget > 0 and elapsed() > 0.95 * budget - 0.01

    wp = torch.from_numpy(np.concatenate(arrs)).to(dev)
    stop = torch.from_numpy(np.concatenate(stops)).to(dev)
    counts = np.array([a.shape[0] for a in arrs], dtype=np.int64)
    ids = np.arange(P)                                   # the request every path of a batch answers
    state = decision_h = k_h = None                      # (has [.] bool, rows [.][4][4]) of the batch's paths, on the device
    if initial_states is not None:
        rows_h, has_h = np.zeros((P, 4, 4)), np.zeros(P, dtype=bool)
        for p, st in enumerate(initial_states):
            if st is None or (has_initial_state is not None and not has_initial_state[p]):
                continue
            has_h[p] = True
            rows_h[p, 0, 3] = float(st["heading"])
            rows_h[p, 1], rows_h[p, 2], rows_h[p, 3] = st["velocity"], st["acceleration"], st["jerk"]
        state = (torch.from_numpy(has_h).to(dev), torch.from_numpy(rows_h).to(dev))
    if initial is not None:
        # ---- prepareInitialCondition (:506-614) and the edit of :649-672, where the waypoints are
        f64, i32 = torch.float64, torch.int32
        pred = tuple(_as_device(a, f64, dev) for a in initial["prediction"])
        n_pred = _as_device(initial["n_pred"], i32, dev)
        age = _as_device(initial["prediction_age"], f64, dev)
        vo = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
        decision = torch.empty(P, dtype=i32, device=dev)
        k_d = torch.empty(P, dtype=i32, device=dev)
        block = torch.empty((P, 4, 4), dtype=f64, device=dev)
        offsets = torch.empty(P + 1, dtype=i32, device=dev)
        rows = torch.empty((wp.shape[0] + P, api.N_DIM), dtype=f64, device=dev)
        stop_rows = torch.empty(wp.shape[0] + P, dtype=torch.uint8, device=dev)
        plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))   # (these steps take the path count and the context from it)
        try:
            plan.initial_condition(_as_device(initial["flags"], i32, dev), _as_device(initial["tracker"], f64, dev),
                                   _as_device(initial["tracker_age"], f64, dev), _as_device(initial["uav_pose"], f64, dev),
                                   float(initial["takeoff_height"]), _as_device(initial["path_time_offset"], f64, dev), vo, pred,
                                   n_pred, decision, k_d, block)
            plan.prepend_initial_condition(vo, wp, decision, block, offsets, rows, stop_at=stop, stop_at_out=stop_rows)
            words = torch.cat([offsets, decision, k_d]).cpu().numpy()
        finally:
            plan.close()
        off = words[:P + 1].astype(np.int64)
        decision_h, k_h = words[P + 1:2 * P + 1].astype(np.int32), words[2 * P + 1:].astype(np.int32)
        wp, stop, counts = rows[:off[-1]], stop_rows[:off[-1]], np.diff(off)
        state = ((decision & api.IC_PREPEND) != 0, block)
        counts = np.where(decision_h & api.IC_INVALID, 0, counts)     # an invalid decision fails its request

    def select(keep, first, n, wp, stop, lim_d, state):
        """the paths `keep` of a packed batch whose path a has the vertices first[a] .. first[a] + n[a] - 1"""
        vtx = np.concatenate([np.arange(first[a], first[a] + n[a]) for a in keep]) if keep.size else np.zeros(0, dtype=np.int64)
        vtx, keep_d = torch.from_numpy(vtx).to(dev), torch.from_numpy(keep).to(dev)
        return wp[vtx], stop[vtx], lim_d[keep_d], None if state is None else (state[0][keep_d], state[1][keep_d])

    lim_d = torch.from_numpy(lim).to(dev)
    if constraints is not None:                          # [P][2][9]: the solve's limits and the fallback sampler's
        lim_d = _request_limits(ctx, pol, constraints, override, override_flags, state, P, dev)
    if (counts < 2).any():                              # "the path is empty (after postprocessing)" :676-681
        first = np.concatenate([[0], np.cumsum(np.diff(off) if initial is not None else counts)])[:-1]
        keep = np.flatnonzero(counts >= 2)
        wp, stop, lim_d, state = select(keep, first, counts, wp, stop, lim_d, state)
        ids, counts = ids[keep], counts[keep]

    # ---- preprocessPath (:431-500) where the waypoints are
    A = ids.size
    if A:
        so = np.concatenate([[0], np.cumsum(counts - 1)]).astype(np.int32)
        plan = api.Plan(ctx, so)
        try:
            offsets = torch.empty(A + 1, dtype=torch.int32, device=dev)
            rows, stop_rows = torch.empty_like(wp), torch.empty_like(stop)
            plan.preprocess_path(wp.contiguous(), offsets, rows, min_waypoint_distance=pol.min_waypoint_distance,
                                 stop_at=stop.contiguous(), straightener_enabled=bool(pol.path_straightener_enabled),
                                 straightener_max_deviation=pol.path_straightener_max_deviation,
                                 straightener_max_hdg_deviation=pol.path_straightener_max_hdg_deviation, stop_at_out=stop_rows)
            off = offsets.cpu().numpy().astype(np.int64)
        finally:
            plan.close()
        wp, stop, counts = rows[:off[-1]], stop_rows[:off[-1]], np.diff(off)
        n_wp[ids] = counts
        if (counts < 2).any():
            keep = np.flatnonzero(counts >= 2)
            wp, stop, lim_d, state = select(keep, off[:-1], counts, wp, stop, lim_d, state)
            ids, counts = ids[keep], counts[keep]

    opt = api.Options.from_buffer_copy(pol.solver)
    opt.estimate_times = 1
    opt.sample_capacity = cap
    if pol.max_trajectory_len_factor > 0:                # the length gate is the reference's answer to a runaway (:1178-1199)
        opt.flags |= api.FLAG_REFERENCE_STATUS           # where its upper side runs; else the product's own rule (-4) answers
    if any_stop and d == 4:
        opt.flags |= api.FLAG_CONSTRAINED_SLOTS

    # one solve has one sampling_dt: the paths from the future (0.2 s, :692-697) run the rounds as a group of their own
    groups = [(np.arange(ids.size), dt)]
    if decision_h is not None and dt != FUTURE_SAMPLING_DT:
        future = (decision_h[ids] & api.IC_FROM_FUTURE) != 0
        groups = [(np.flatnonzero(~future), dt), (np.flatnonzero(future), FUTURE_SAMPLING_DT)]
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    for members, group_dt in groups:
        if members.size == 0:
            continue
        if members.size == ids.size:
            g_wp, g_stop, g_lim, g_state = wp, stop, lim_d, state
        else:
            g_wp, g_stop, g_lim, g_state = select(members, first, counts, wp, stop, lim_d, state)
        g_so = np.concatenate([[0], np.cumsum(counts[members] - 1)]).astype(np.int32)
        _rounds(ctx, pol, opt, group_dt, cap, d, ids[members], g_so, g_wp, g_stop, g_lim, g_state, elapsed, overtime,
                dict(success=success, n_samples=n_samples, max_dev=max_dev, n_wp=n_wp, iters=iters, samples=samples_out))
    # a path that was still being subdivided when it outgrew a plan, or whose rounds ran out, keeps what the loop left it
    lost = np.setdiff1d(np.arange(P), np.flatnonzero(success))
    n_samples[lost] = 0
    result = dict(success=success, n_samples=n_samples, samples=samples_out, max_deviation=max_dev, n_waypoints=n_wp,
                  iterations=iters)
    if pol.override_heading_atan2 or initial is not None:
        plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
        try:
            ns_d, ok_d = torch.from_numpy(n_samples).to(dev), torch.from_numpy(success).to(dev)
            if pol.override_heading_atan2:               # getTrajectoryReference :1578-1603, where the samples are
                plan.travel_heading(samples_out, ns_d, status=ok_d)
            if initial is not None:                      # the pre-trajectory of a path from the future (:801-840), in place
                st_out = torch.empty(P, dtype=torch.int32, device=dev)
                plan.splice_prediction(samples_out, ns_d, decision, k_d, age, pred[0], n_pred, status=ok_d, status_out=st_out)
                words = torch.cat([ns_d, st_out]).cpu().numpy()
                spliced, st_h = words[:P], words[P:]
                good = (st_h > 0) & (spliced <= cap)     # a prediction shorter than k, a spliced count above the capacity
                bad = np.flatnonzero((success != 0) & ~good)
                success[bad] = 0
                n_samples[:] = np.where(good & (success != 0), spliced, 0)
                if bad.size:
                    samples_out[torch.from_numpy(bad).to(dev)] = 0.0
                result.update(decision=decision_h, sample_offset=k_h)
        finally:
            plan.close()
    return result


def _rounds(ctx, pol, opt, dt, cap, d, ids, so, wp, stop, lim_d, state, elapsed, overtime, out):
    """the rounds of optimize() (:700-790) for the paths ids of one sampling_dt: so, wp, stop, lim_d, state describe the thinned
    batch; the answers go to the arrays of out at ids"""
    dev = wp.device
    success, n_samples, max_dev, n_wp, iters, samples_out = (out[key] for key in ("success", "n_samples", "max_dev", "n_wp", "iters",
                                                                                  "samples"))
    budget = float(pol.max_execution_time_s)
    opt = api.Options.from_buffer_copy(opt)
    opt.sampling_dt = dt
    for rnd in range(int(pol.max_deviation_iterations) + 1):
        # a path subdivided beyond the longest one a plan takes fails on its own (the reference has no such limit)
        fits = np.diff(so) <= MAX_SEGMENTS
        if not fits.all():
            keep = np.flatnonzero(fits)
            vtx = np.concatenate([np.arange(so[a] + a, so[a + 1] + a + 1) for a in keep]) if keep.size else np.zeros(0, dtype=np.int64)
            vtx = torch.from_numpy(vtx).to(dev)
            keep_d = torch.from_numpy(keep).to(dev)
            wp, stop, lim_d = wp[vtx], stop[vtx], lim_d[keep_d]
            state = None if state is None else (state[0][keep_d], state[1][keep_d])
            so = np.concatenate([[0], np.cumsum(np.diff(so)[keep])]).astype(np.int32)
            ids = ids[keep]
        A = ids.size
        if A == 0:
            break
        last_round = rnd == int(pol.max_deviation_iterations)
        # the solver of a round (:702-716, :754-768): the fallback sampler when it was asked for or when the request runs over
        # its time (it still succeeds), else findTrajectory under the time that is left (:899)
        use_fallback = bool(pol.fallback_sampling)
        if not use_fallback and budget > 0:
            spent = elapsed()
            opt.max_time_s = 2.0 * 0.95 * (0.0 if spent >= budget else budget - spent)
            use_fallback = overtime()
        n_s, n_v = int(so[-1]), int(so[-1]) + A
        plan = api.Plan(ctx, so)
        try:
            unwrapped = torch.empty_like(wp)
            baca = torch.empty(n_s, dtype=torch.float64, device=dev)
            ns = torch.zeros(A, dtype=torch.int32, device=dev)
            samples = torch.zeros((A, cap, api.N_DIM), dtype=torch.float64, device=dev)
            requested = lim_d.dim() == 3      # constraints=: [.][0] findTrajectory's limits, [.][1] findTrajectoryFallback's
            if use_fallback:                                                                 # findTrajectoryFallback, :1215-1395
                plan.unwrap_headings(wp.contiguous(), unwrapped)                             # :1233-1241, from the first waypoint
                if requested:
                    lim_fb = lim_d[:, 1].contiguous()
                else:
                    lim_fb = lim_d.clone()
                    lim_fb[:, 0:2] *= float(pol.fallback_speed_factor)
                    lim_fb[:, 3:5] *= float(pol.fallback_accel_factor)
                plan.estimate_times_baca(unwrapped, lim_fb, baca)
                plan.fallback_sample(wp.contiguous(), baca, dt, cap, ns, samples, stop_at=stop.contiguous(),
                                     stopping_time=pol.fallback_stopping_time)
                ok = ns <= cap
            else:
                lim_solve = lim_d[:, 0].contiguous() if requested else lim_d
                mask = torch.empty((n_v, 5), dtype=torch.uint8, device=dev)
                vals = torch.empty((n_v, 5, api.N_DIM), dtype=torch.float64, device=dev)
                has, rows = (None, None) if state is None else (state[0].to(torch.uint8).contiguous(), state[1].contiguous())
                plan.request_vertices(wp.contiguous(), unwrapped, mask, vals, stop_at=stop.contiguous(), has_state=has, state=rows,
                                      derivative_to_optimize=d)                             # :923-977, the unwrap from the state
                plan.estimate_times_baca(unwrapped, lim_solve, baca)                         # initial_total_time_baca, :1048-1056
                times = torch.zeros(n_s, dtype=torch.float64, device=dev)
                coeffs = torch.empty((n_s, api.N_DIM, api.N_COEFF), dtype=torch.float64, device=dev)
                status = torch.zeros(A, dtype=torch.int32, device=dev)
                cost = torch.zeros(A, dtype=torch.float64, device=dev)
                plan.solve(opt, mask, vals, times, coeffs, status, cost=cost, waypoints=unwrapped, limits=lim_solve, n_samples=ns,
                           samples=samples)
                verdict = torch.empty(A, dtype=torch.int32, device=dev)
                plan.length_gate(baca, ns, dt, max_factor=pol.max_trajectory_len_factor,
                                 min_factor=pol.min_trajectory_len_factor, status=status, verdict=verdict)   # :1138-1149, :1178-1199
                ok = (verdict == api.FIND_ACCEPTED) & (ns <= cap)
            worst =torch.zeros(A, dtype=torch.float64, device=dev)
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
        if not use_fallback and overtime():   # findTrajectory's own checks behind the solve and the sampler: "return {}" (:1085,
            ok_h, go_h = np.zeros(A, dtype=bool), np.zeros(A, dtype=bool)   # :1156, :1171): the readback came after the deadline
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
        keep_d = torch.from_numpy(keep).to(dev)
        wp, stop, lim_d = rows[vtx], stop_rows[vtx], lim_d[keep_d]
        state = None if state is None else (state[0][keep_d], state[1][keep_d])
        so = np.concatenate([[0], np.cumsum(np.diff(off)[keep] - 1)]).astype(np.int32)
        ids = ids[keep]
