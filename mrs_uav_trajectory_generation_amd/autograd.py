"""The segment-time estimate, the fixed-times solve, the segment maxima, the sampler, the evaluation at given times, the
deviation from the waypoint path and the waypoint passage as torch.autograd.Functions: gradients of a loss on the coefficients,
the cost, the derivative maxima, the samples, the states at chosen times, the deviations, the miss distances and the passing
times reach the waypoints (through the fixed values AND through the estimated times), the initial state, the segment times, the
limits and the query times.

Forward: Plan.solve with time_alloc_method = NONE, no sampling, no waypoints, no limits (the existing kernels, unchanged).
Backward: Plan.solve_vjp (mrs_tg_plan_solve_vjp, vjp_kernel), the exact chain rule of the linear QP at the returned solution
(DESIGN.md section 4c).  Differentiated: fixed_values and seg_times.  Not differentiated by solve itself: time allocation and
second derivatives; the feasibility scaling and the limits are segment_maxima and scale_times_to_limits below (DESIGN.md
section 4d), the sampling is sample / sample_states.  Both passes run on torch's current stream of the thread that runs them: the call binds
the plan's context to it (Context.use_torch_stream), and the context stays bound afterwards.

    >>> fv = fixed_values.clone(); fv[:, 0, :] = waypoints; coeffs, cost, status = solve(plan, fixed_mask, fv, seg_times)

segment_maxima (Plan.segment_maxima forward, Plan.segment_maxima_vjp backward: mrs_tg_plan_segment_maxima_vjp, DESIGN.md
section 4d) differentiates the per-segment maxima of |p^(k)| in the coefficients and the segment times; scale_times_to_limits
puts the product's feasibility step T <- T max(1, v, sqrt a, cbrt j) on top of it.  The intended chain
differentiates everything after the time allocation -- solve, maxima, scaling, re-solve:

    >>> coeffs, _, status = solve(plan, fixed_mask, fv, seg_times)
    >>> times = scale_times_to_limits(plan, coeffs, seg_times, limits, status)
    >>> coeffs, cost, status = solve(plan, fixed_mask, fv, times); samples, n = sample(plan, coeffs, times, dt, cap, status)

sample / sample_states (Plan.sample / Plan.sample_states forward, Plan.sample_states_vjp backward:
mrs_tg_plan_sample_states_vjp) put the losses people write on a trajectory -- clearance, tracking --
within reach: the gradient is that of the walk the forward took (sample count and segment membership held fixed).  From
waypoints to a loss on samples:

    >>> fv = fixed_values.clone().requires_grad_(); times = seg_times.clone().requires_grad_()
    >>> coeffs, _, status = solve(plan, fixed_mask, fv, times)
    >>> samples, n = sample(plan, coeffs, times, 0.2, 512, status)      # [n_paths][512][4], rows >= n are zero
    >>> valid = torch.arange(512, device=n.device)[None, :] < n[:, None]
    >>> loss = (torch.relu(1.0 - (samples[..., :3] - obstacle).norm(dim=-1)) * valid).sum()
    >>> loss.backward()                                                 # fv.grad, times.grad

evaluate (Plan.evaluate forward, Plan.evaluate_vjp backward: mrs_tg_plan_evaluate / mrs_tg_plan_evaluate_vjp, DESIGN.md section
7c) is the other access path: the state of every path at times the caller chooses, differentiable in the coefficients, the
segment times AND the query times, with nothing that appears or disappears as the total time moves.  The clearance between two
UAVs at common absolute time stamps -- two plans, trajectories of different durations, one time grid:

    >>> ca, _, sa = solve(plan_a, mask_a, fv_a, times_a); cb, _, sb = solve(plan_b, mask_b, fv_b, times_b)
    >>> grid = torch.arange(0.0, 12.0, 0.1, dtype=torch.float64, device="cuda").expand(plan_a.n_paths, -1)   # seconds from the start
    >>> pa, seg_a = evaluate(plan_a, ca, times_a, grid, n_orders=1, status=sa)   # [n_paths][120][1][4]; seg -1: behind the end
    >>> pb, seg_b = evaluate(plan_b, cb, times_b, grid, n_orders=1, status=sb)
    >>> both = (seg_a >= 0) & (seg_b >= 0)
    >>> loss = (torch.relu(2.0 - (pa[..., 0, :3] - pb[..., 0, :3]).norm(dim=-1)) * both).sum()
    >>> loss.backward()                                   # fv_a.grad, times_a.grad, fv_b.grad, times_b.grad

path_deviation (Plan.path_deviation forward, Plan.path_deviation_vjp backward: mrs_tg_plan_path_deviation /
mrs_tg_plan_path_deviation_vjp) is the figure the reference's own policy acts on: how far every sample
strays from the waypoint polyline, by validateTrajectorySpatial's scan with its waypoint cursor.  The cursor of every sample is
held fixed in the backward pass.  From waypoints to "stay within 5 cm of the path" -- the term the reference enforces by
subdividing segments -- through the solve and the sampler:

    >>> fv = fixed_values.clone().requires_grad_(); times = seg_times.clone().requires_grad_()
    >>> coeffs, _, status = solve(plan, fixed_mask, fv, times)
    >>> samples, n = sample(plan, coeffs, times, 0.2, 512, status)
    >>> deviation, cursor = path_deviation(plan, samples, n, fv[:, 0, :], first_segment=True, status=status)
    >>> corridor = torch.relu(deviation - 0.05).sum()             # rows behind a path's scan are zero: no mask needed
    >>> worst = deviation.amax(dim=1)                             # the reference's max_deviation per path (first_segment=True)
    >>> corridor.backward()                                       # fv.grad (through the samples AND the polyline), times.grad

estimate_times (Plan.estimate_times forward, Plan.estimate_times_vjp backward: mrs_tg_plan_estimate_times /
mrs_tg_plan_estimate_times_vjp) is where the times come from: the Euclidean estimate a solve with
estimate_times = 1 starts from, in the same bits, differentiable in the waypoints and the limits with every branch of the
forward held fixed.  With it the chain starts at the waypoints and the limits, and the corridor term sees a waypoint through its
two segment times as well -- estimate, solve, feasibility scaling, re-solve, sampler, deviation:

    >>> wp = waypoints.clone().requires_grad_(); lim = limits.clone().requires_grad_()
    >>> fv = fixed_values.clone(); fv[:, 0, :] = wp
    >>> times = estimate_times(plan, wp, lim)
    >>> coeffs, _, status = solve(plan, fixed_mask, fv, times)
    >>> times = scale_times_to_limits(plan, coeffs, times, lim, status)
    >>> coeffs, _, status = solve(plan, fixed_mask, fv, times)
    >>> samples, n = sample(plan, coeffs, times, 0.2, 512, status)
    >>> deviation, cursor = path_deviation(plan, samples, n, wp, first_segment=True, status=status)
    >>> torch.relu(deviation - 0.05).sum().backward()             # wp.grad (values, polyline AND times), lim.grad

preprocess_path and insert_midpoints (Plan.preprocess_path / Plan.insert_midpoints forward, Plan.path_edit_vjp backward:
mrs_tg_plan_path_edit_vjp) are the two stages that change the number of waypoints: they return the plan of
the edited batch with its waypoints, so the chain above carries on behind an unsafe segment and its gradient still arrives at
the requested waypoints -- a copy passes its row on, a mid-point gives half of its row to each end of its segment:

    >>> plan1, wp1, stop1, source = preprocess_path(plan, wp, min_waypoint_distance=0.05)
    >>> ...                                                       # estimate, solve, sample on plan1 / wp1
    >>> plan1.path_deviation(samples.detach(), n, wp1.detach(), segment_max=segment_max)   # [sum S] of plan1, preallocated
    >>> plan2, wp2, stop2, source, inserted = insert_midpoints(plan1, wp1, segment_max, 0.05)

travel_heading (Plan.travel_heading forward, Plan.travel_heading_vjp backward: mrs_tg_plan_travel_heading /
mrs_tg_plan_travel_heading_vjp) is the last stage before the answer leaves: with override_heading_atan2
the tracker receives the direction of travel as the heading, a row that barely moves keeping the heading of the row in front.
A loss on the heading the tracker actually gets -- here: look where a point of interest is -- reaches the waypoints through it:

    >>> samples, n = sample(plan, coeffs, times, 0.2, 512, status)
    >>> rows, source = travel_heading(plan, samples, n, status=status)        # a fresh tensor; source: the row whose step it was
    >>> valid = torch.arange(512, device=n.device)[None, :] < n[:, None] - 1  # the last row keeps its sampled yaw
    >>> bearing = torch.atan2(poi[1] - rows[..., 1], poi[0] - rows[..., 0])
    >>> ((1.0 - torch.cos(rows[..., 3] - bearing)) * valid).sum().backward()  # fv.grad, times.grad

request_vertices and request_limits (Plan.request_vertices / Plan.request_limits forward, Plan.request_vertices_vjp /
Plan.request_limits_vjp backward) are where a request becomes the solver's inputs: the headings unwrapped
from the state's heading with the constraint mask and values, and the limits from the constraints, the override and the state.
With them the chain starts at the RAW request and the state's velocity gets a gradient:

    >>> raw = waypoints.clone().requires_grad_(); st = state.clone().requires_grad_(); c = constraints.clone().requires_grad_()
    >>> lim = request_limits(plan, c, state=st)
    >>> wp, mask, fv = request_vertices(plan, raw, state=st)
    >>> times = estimate_times(plan, wp, lim)
    >>> coeffs, _, status = solve(plan, mask, fv, times); samples, n = sample(plan, coeffs, times, 0.2, 512, status)
    >>> ((samples[..., :3] - target) ** 2).sum().backward()            # raw.grad, st.grad (rows 1 .. 3), c.grad

mutual_clearance (Plan.mutual_clearance forward, Plan.mutual_clearance_vjp backward: mrs_tg_plan_mutual_clearance /
mrs_tg_plan_mutual_clearance_vjp) answers the first question a swarm asks of its trajectories: how close
do its UAVs come to each other, when, and who is the neighbour.  The paths of ONE plan are partitioned into groups; for every
row the stage gives the distance to the nearest other path of the row's group at the same step and that path's index -- one
launch, no [N][N][Q] temporary, a fixed order of every sum.  The neighbour is held fixed in the backward pass.  A swarm of four
paths in one plan, kept 2 m apart:

    >>> plan = api.Plan(ctx, seg_offsets)                               # four paths
    >>> fv = fixed_values.clone().requires_grad_(); times = seg_times.clone().requires_grad_()
    >>> coeffs, _, status = solve(plan, fixed_mask, fv, times)
    >>> samples, n = sample(plan, coeffs, times, 0.2, 512, status)
    >>> clearance, partner = mutual_clearance(plan, samples, n, [0, 4], status=status)   # one group; all start at step 0
    >>> torch.relu(2.0 - clearance).sum().backward()                    # +inf where nobody is near in time: no mask; fv.grad, times.grad
    >>> closest = clearance.amin(dim=1)                                 # per UAV; partner says to whom

obstacle_clearance (Plan.obstacle_clearance forward, Plan.obstacle_clearance_vjp backward: mrs_tg_plan_obstacle_clearance /
mrs_tg_plan_obstacle_clearance_vjp) is the clearance loss of the first example against a real map: a
point cloud or a list of spheres, hundreds to thousands of them, [n_obstacles][4] = (x, y, z, radius) with radius 0 for a point.
For every row the stage gives the signed distance to the nearest obstacle (negative inside a sphere) and that obstacle's index
-- one launch, no [N][Q][M] temporary, ties to the lowest index.  Paths may see different parts of the map (set_offsets,
path_set); the nearest obstacle is held fixed in the backward pass, and the map itself gets no gradient.  Keeping 1 m away
from everything, checked on a grid finer than the tracker's:

    >>> fv = fixed_values.clone().requires_grad_(); times = seg_times.clone().requires_grad_()
    >>> coeffs, _, status = solve(plan, fixed_mask, fv, times)
    >>> samples, n = sample(plan, coeffs, times, 0.05, 2048, status)    # (or evaluate(...) at times of the caller's choosing)
    >>> clearance, nearest = obstacle_clearance(plan, samples, n, obstacles, status=status)   # one set: the whole map
    >>> torch.relu(1.0 - clearance).sum().backward()                    # +inf behind a path's last row: no mask; fv.grad, times.grad
    >>> worst = clearance.amin(dim=1)                                   # per path; nearest says which obstacle

field_clearance (Plan.field_clearance forward, Plan.field_clearance_vjp backward: mrs_tg_plan_field_clearance /
mrs_tg_plan_field_clearance_vjp) is the same loss against a map given as a voxel grid of signed
distances (an ESDF), looked up by trilinear interpolation: eight voxel reads per row whatever the size of the map, where
obstacle_clearance pays for every obstacle on every iteration.  Where only a list of obstacles exists the grid is built once
(Plan.obstacle_clearance over the nodes of the grid).  The cell is held fixed in the backward pass, the
field itself gets no gradient, and the caller says what space outside the grid means (outside_value):

    >>> geometry = api.FieldGeometry(origin=(-20.0, -20.0, 0.0), spacing=(0.2, 0.2, 0.2), dims=(200, 200, 50))
    >>> clearance, cell, least, where = field_clearance(plan, samples, n, fields, geometry, status=status)   # fields [1][50][200][200]
    >>> torch.relu(1.0 - clearance).sum().backward()                    # or torch.relu(1.0 - least).sum(): the worst row of every path
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import api


class _FixedTimesSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, fixed_mask, fixed_values, seg_times, derivative, flags):
        fv = fixed_values.detach().contiguous()
        times = seg_times.detach().clone().contiguous()   # (seg_times_inout: the solve's own copy)
        dev = fv.device
        coeffs = torch.empty((plan.n_segments, api.N_DIM, api.N_COEFF), dtype=torch.float64, device=dev)
        status = torch.empty(plan.n_paths, dtype=torch.int32, device=dev)
        cost = torch.empty(plan.n_paths, dtype=torch.float64, device=dev)
        opt = api.default_options(derivative_to_optimize=int(derivative), time_alloc_method=api.TIME_ALLOC_NONE, estimate_times=0,
                                  sampling_dt=0.0, flags=int(flags))
        plan.ctx.use_torch_stream()
        plan.solve(opt, fixed_mask, fv, times, coeffs, status, cost)
        ctx.plan, ctx.derivative = plan, int(derivative)
        ctx.save_for_backward(fixed_mask, fv, times, coeffs, status)
        ctx.mark_non_differentiable(status)
        ctx.set_materialize_grads(False)
        return coeffs, cost, status

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_coeffs, grad_cost, _grad_status):
        fixed_mask, fv, times, coeffs, status = ctx.saved_tensors
        want_values, want_times = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gv = torch.zeros_like(fv) if want_values else None
        gt = torch.zeros_like(times) if want_times else None
        if (gv is None and gt is None) or (grad_coeffs is None and grad_cost is None):
            return None, None, gv, gt, None, None
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.solve_vjp(ctx.derivative, fixed_mask, fv, times, coeffs, status,
                       grad_coeffs=None if grad_coeffs is None else grad_coeffs.to(torch.float64).contiguous(),
                       grad_cost=None if grad_cost is None else grad_cost.to(torch.float64).contiguous(),
                       grad_fixed_values=gv, grad_seg_times=gt)
        return None, None, gv, gt, None, None


def solve(plan, fixed_mask, fixed_values, seg_times, derivative=4, flags=api.FLAG_GENERAL_PATTERNS):
    """(coeffs [sum S][4][10], cost [n_paths], status [n_paths]) of the fixed-times solve of `plan`'s batch, differentiable in
    fixed_values [sum V][5][4] and seg_times [sum S] (float64 device tensors; fixed_mask uint8 [sum V][5]).  A path with
    status <= 0 gets zero gradients."""
    return _FixedTimesSolve.apply(plan, fixed_mask, fixed_values, seg_times, derivative, flags)


class _SegmentMaxima(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, coeffs, seg_times):
        c = coeffs.detach().to(torch.float64).contiguous()
        t = seg_times.detach().to(torch.float64).contiguous()
        maxima = torch.empty((plan.n_segments, 3, 3), dtype=torch.float64, device=c.device)
        plan.ctx.use_torch_stream()
        plan.segment_maxima(c, t, maxima)
        ctx.plan = plan
        ctx.save_for_backward(c, t)
        ctx.set_materialize_grads(False)
        return maxima

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_maxima):
        c, t = ctx.saved_tensors
        want_c, want_t = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gc = torch.empty_like(c) if want_c else None
        gt = torch.empty_like(t) if want_t else None
        if grad_maxima is None:
            return None, None if gc is None else gc.zero_(), None if gt is None else gt.zero_()
        if gc is None and gt is None:
            return None, None, None
        plan = ctx.plan
        plan.ctx.use_torch_stream()
        plan.segment_maxima_vjp(c, t, grad_maxima.to(torch.float64).contiguous(), grad_coeffs=gc, grad_seg_times=gt)
        return None, gc, gt


def segment_maxima(plan, coeffs, seg_times):
    """maxima [sum S][3][3] = max over [0, T] of |p^(k)|, indexed [segment][k-1][group] (groups {x,y}, {z}, {heading}), of
    the trajectories (coeffs [sum S][4][10], seg_times [sum S]; float64 device tensors), differentiable in both.  The gradient
    is the envelope theorem's at the forward search's own maximiser (a tie gives that winner's one-sided gradient); a zero
    maximum and a segment with T <= 0 or non-finite inputs give zero gradients."""
    return _SegmentMaxima.apply(plan, coeffs, seg_times)


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, coeffs, seg_times, sampling_dt, sample_capacity, status, all_orders):
        c = coeffs.detach().to(torch.float64).contiguous()
        t = seg_times.detach().to(torch.float64).contiguous()
        cap = int(sample_capacity)
        n = torch.empty(plan.n_paths, dtype=torch.int32, device=c.device)
        # (the kernels write the rows a path has; the rows at or beyond its count stay zero)
        shape = (plan.n_paths, cap, api.STATE_ORDERS, api.N_DIM) if all_orders else (plan.n_paths, cap, api.N_DIM)
        out = torch.zeros(shape, dtype=torch.float64, device=c.device)
        plan.ctx.use_torch_stream()
        (plan.sample_states if all_orders else plan.sample)(c, t, float(sampling_dt), cap, n, out if cap > 0 else None)
        ctx.plan, ctx.dt, ctx.cap = plan, float(sampling_dt), cap
        ctx.status = None if status is None else status.detach().to(torch.int32).contiguous()
        ctx.save_for_backward(c, t)
        ctx.mark_non_differentiable(n)
        ctx.set_materialize_grads(False)
        return out, n

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_n):
        c, t = ctx.saved_tensors
        want_c, want_t = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if grad_out is None or not (want_c or want_t):
            return None, None, None, None, None, None, None
        gc = torch.empty_like(c) if want_c else None
        gt = torch.empty_like(t) if want_t else None
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.sample_states_vjp(c, t, ctx.dt, ctx.cap, grad_out.to(torch.float64).contiguous(), status=ctx.status,
                               grad_coeffs=gc, grad_seg_times=gt)
        return None, gc, gt, None, None, None, None


def sample_states(plan, coeffs, seg_times, sampling_dt, sample_capacity, status=None):
    """(states [n_paths][capacity][5][4], n_samples [n_paths] int32) of Plan.sample_states -- derivative orders 0..4 of
    (x, y, z, heading) every sampling_dt seconds -- differentiable in coeffs [sum S][4][10] and seg_times [sum S] (float64
    device tensors).  Rows at or beyond a path's n_samples are zero (n_samples = capacity + 1: more samples than fit, the first
    capacity are there).  The gradient is that of the walk the forward took: the sample count and the segment of every sample
    are held fixed, d(time in segment)/dT_i = -1 for the segments in front of the sample's own.  A path with status <= 0
    (status [n_paths], optional) gets zero gradients."""
    return _Sample.apply(plan, coeffs, seg_times, sampling_dt, sample_capacity, status, True)


def sample(plan, coeffs, seg_times, sampling_dt, sample_capacity, status=None):
    """(samples [n_paths][capacity][4], n_samples [n_paths] int32) of Plan.sample: positions and wrapped heading, order 0 of
    sample_states (same walk, same bits, a fifth of the stores); differentiable as sample_states is."""
    return _Sample.apply(plan, coeffs, seg_times, sampling_dt, sample_capacity, status, False)


class _Evaluate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, coeffs, seg_times, query_times, n_orders, status):
        c = coeffs.detach().to(torch.float64).contiguous()
        t = seg_times.detach().to(torch.float64).contiguous()
        q = query_times.detach().to(torch.float64).contiguous()
        if q.dim() != 2 or q.shape[0] != plan.n_paths:
            raise ValueError("query_times must be [n_paths][n_queries]")
        no = int(n_orders)
        states = torch.empty((plan.n_paths, q.shape[1], no, api.N_DIM), dtype=torch.float64, device=c.device)
        segment = torch.empty((plan.n_paths, q.shape[1]), dtype=torch.int32, device=c.device)
        plan.ctx.use_torch_stream()
        plan.evaluate(c, t, q, states, query_segment=segment)
        ctx.plan = plan
        ctx.status = None if status is None else status.detach().to(torch.int32).contiguous()
        ctx.save_for_backward(c, t, q)
        ctx.mark_non_differentiable(segment)
        ctx.set_materialize_grads(False)
        return states, segment

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_states, _grad_segment):
        c, t, q = ctx.saved_tensors
        want_c, want_t, want_q = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if grad_states is None or not (want_c or want_t or want_q):
            return None, None, None, None, None, None
        gc = torch.empty_like(c) if want_c else None
        gt = torch.empty_like(t) if want_t else None
        gq = torch.empty_like(q) if want_q else None
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.evaluate_vjp(c, t, q, grad_states.to(torch.float64).contiguous(), status=ctx.status, grad_coeffs=gc,
                          grad_seg_times=gt, grad_query_times=gq)
        return None, gc, gt, gq, None, None


def evaluate(plan, coeffs, seg_times, query_times, n_orders=5, status=None):
    """(states [n_paths][n_queries][n_orders][4], segment [n_paths][n_queries] int32) of Plan.evaluate: the derivative orders
    0 .. n_orders-1 (n_orders 1 or 5) of (x, y, z, heading) of every path at query_times [n_paths][n_queries], seconds from
    the path's start, in any order -- differentiable in coeffs [sum S][4][10], seg_times [sum S] and query_times (float64
    device tensors).  segment is the index within the path of the segment a query fell into, or -1 for a query that is
    negative, behind the path's end or NaN (the padding for a path with fewer queries): its state row is zero and it gets and
    gives no gradient.  The gradient holds the segment of every query fixed; d(time in segment)/dT_m = -1 for the segments in
    front of the query's own, d/dquery = 1.  A path with status <= 0 (status [n_paths], optional) gets zero gradients."""
    if int(n_orders) not in (1, api.STATE_ORDERS):
        raise ValueError("n_orders must be 1 or %d" % api.STATE_ORDERS)
    return _Evaluate.apply(plan, coeffs, seg_times, query_times, int(n_orders), status)


def _f64(t):
    return t.detach().to(torch.float64).contiguous()


def _i32(t):
    return t.detach().to(torch.int32).contiguous()


def _rows(plan, samples):
    """samples detached as a contiguous float64 tensor [n_paths][capacity][4], or ValueError"""
    s = _f64(samples)
    if s.dim() != 3 or s.shape[0] != plan.n_paths or s.shape[2] != api.N_DIM:
        raise ValueError("samples must be [n_paths][capacity][4]")
    return s


def _rows_and_counts(plan, samples, n_samples):
    """... and n_samples as a contiguous int32 tensor [n_paths]"""
    s, n = _rows(plan, samples), _i32(n_samples)
    if n.dim() != 1 or n.shape[0] != plan.n_paths:
        raise ValueError("n_samples must be [n_paths]")
    return s, n


class _PathDeviation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, samples, n_samples, waypoints, first_segment, status):
        w = waypoints.detach().to(torch.float64).contiguous()
        n = n_samples.detach().to(torch.int32).contiguous()
        s = _rows(plan, samples)
        if w.dim() != 2 or w.shape[0] != plan.n_segments + plan.n_paths or w.shape[1] != api.N_DIM:
            raise ValueError("waypoints must be [sum V][4]")
        st = None if status is None else status.detach().to(torch.int32).contiguous()
        deviation = torch.empty(s.shape[:2], dtype=torch.float64, device=s.device)
        cursor = torch.empty(s.shape[:2], dtype=torch.int32, device=s.device)
        plan.ctx.use_torch_stream()
        plan.path_deviation(s, n, w, first_segment=bool(first_segment), status=st, deviation=deviation, cursor=cursor)
        ctx.plan, ctx.status = plan, st
        ctx.save_for_backward(s, n, w)
        ctx.mark_non_differentiable(cursor)
        ctx.set_materialize_grads(False)
        return deviation, cursor

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_deviation, _grad_cursor):
        s, n, w = ctx.saved_tensors
        want_s, want_w = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if grad_deviation is None or not (want_s or want_w):
            return None, None, None, None, None, None
        gs = torch.empty_like(s) if want_s else None
        gw = torch.empty_like(w) if want_w else None
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.path_deviation_vjp(s, n, w, grad_deviation.to(torch.float64).contiguous(), status=ctx.status, grad_samples=gs,
                                grad_waypoints=gw)
        return None, gs, None, gw, None, None


def path_deviation(plan, samples, n_samples, waypoints, first_segment=True, status=None):
    """(deviation [n_paths][capacity], cursor [n_paths][capacity] int32) of Plan.path_deviation: the distance of every sample
    i = 0 .. n-2 of a path from the segment w_c -> w_{c+1} of its waypoint polyline that validateTrajectorySpatial's cursor c
    points at -- differentiable in samples [n_paths][capacity][4] and waypoints [sum V][4] (float64 device tensors; x, y, z
    are read, column 3 gets a zero gradient); n_samples [n_paths] int32 as the sampler returned it.  Rows from n - 1 on hold
    deviation 0 and cursor -1.  The deviation does not depend on first_segment; with first_segment=False the reference leaves
    the samples whose cursor is 0 out of its maximum (paths of more than one segment): mask with cursor > 0.  The gradient
    holds every cursor and the branch of every distance fixed; a sample on its segment (deviation 0) and a path with
    status <= 0 (status [n_paths], optional) get and give zero."""
    return _PathDeviation.apply(plan, samples, n_samples, waypoints, first_segment, status)


class _WaypointPassage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, samples, n_samples, waypoints, wp_offsets, status):
        w = waypoints.detach().to(torch.float64).contiguous()
        n = n_samples.detach().to(torch.int32).contiguous()
        s = _rows(plan, samples)
        if w.dim() != 2 or w.shape[1] != api.N_DIM:
            raise ValueError("waypoints must be [sum W][4]")
        off = None
        if wp_offsets is None:
            if w.shape[0] != plan.n_segments + plan.n_paths:
                raise ValueError("without wp_offsets the waypoints are the plan's vertices [sum V][4]")
        else:
            off = wp_offsets.detach().to(device=s.device, dtype=torch.int32).contiguous()
            if off.dim() != 1 or off.shape[0] != plan.n_paths + 1:
                raise ValueError("wp_offsets must be [n_paths + 1]")
        st = None if status is None else status.detach().to(torch.int32).contiguous()
        index = torch.empty(w.shape[0], dtype=torch.int32, device=s.device)
        count = torch.empty(plan.n_paths, dtype=torch.int32, device=s.device)
        miss = torch.empty(w.shape[0], dtype=torch.float64, device=s.device)
        fraction = torch.empty(w.shape[0], dtype=torch.float64, device=s.device)
        plan.ctx.use_torch_stream()
        plan.waypoint_passage(s, n, w, wp_offsets=off, status=st, index=index, count=count, miss=miss, fraction=fraction)
        ctx.plan, ctx.status, ctx.offsets = plan, st, off
        ctx.save_for_backward(s, n, w)
        ctx.mark_non_differentiable(index, count)
        ctx.set_materialize_grads(False)
        return index, count, miss, fraction

    @staticmethod
    @once_differentiable
    def backward(ctx, _grad_index, _grad_count, grad_miss, grad_fraction):
        s, n, w = ctx.saved_tensors
        want_s, want_w = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if (grad_miss is None and grad_fraction is None) or not (want_s or want_w):
            return None, None, None, None, None, None
        gs = torch.empty_like(s) if want_s else None
        gw = torch.empty_like(w) if want_w else None
        gm = None if grad_miss is None else grad_miss.to(torch.float64).contiguous()
        gf = None if grad_fraction is None else grad_fraction.to(torch.float64).contiguous()
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.waypoint_passage_vjp(s, n, w, grad_miss=gm, grad_fraction=gf, wp_offsets=ctx.offsets, status=ctx.status,
                                  grad_samples=gs, grad_waypoints=gw)
        return None, gs, None, gw, None, None


def waypoint_passage(plan, samples, n_samples, waypoints, wp_offsets=None, status=None):
    """(index [sum W] int32, count [n_paths] int32, miss [sum W], fraction [sum W]) of Plan.waypoint_passage: where the samples
    pass the waypoints by getWaypointInTrajectoryIdxs' scan -- waypoint k of a path is passed on the step index[k] -> index[k] + 1,
    at the distance miss[k], at the place fraction[k] in [0, 1] of that step, so at the time (index[k] + fraction[k]) *
    sampling_dt; index is -1 and the other two are 0 from the first waypoint not reached on, count is how many were.  miss and
    fraction are differentiable in samples [n_paths][capacity][4] and waypoints [sum W][4] (float64 device tensors; x, y, z are
    read, column 3 gets a zero gradient); index and count are not.  waypoints are the ones asked about, which need not be the
    plan's vertices: wp_offsets [n_paths + 1] (int32, a CSR over exactly the rows of waypoints) says which belong to which path;
    None means the plan's vertices [sum V][4].  n_samples [n_paths] int32 as the sampler returned it.  The gradient holds every
    index and the branch of every distance fixed; a waypoint on its step (miss 0) gives nothing through miss, a clamped fraction
    (0 or 1) nothing through fraction, and a path with status <= 0 (status [n_paths], optional) gets and gives zero.  "Be at
    waypoint k at time T" and "pass the requested waypoints closely", reached waypoints only:

        >>> index, count, miss, fraction = waypoint_passage(plan, samples, n, requested, wp_offsets=off, status=status)
        >>> reached = index >= 0
        >>> loss = ((((index + fraction) * dt - arrival) ** 2 + miss ** 2) * reached).sum()"""
    return _WaypointPassage.apply(plan, samples, n_samples, waypoints, wp_offsets, status)


class _EstimateTimes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, waypoints, limits):
        w = waypoints.detach().to(torch.float64).contiguous()
        lim = limits.detach().to(torch.float64).contiguous()
        if w.dim() != 2 or w.shape[0] != plan.n_segments + plan.n_paths or w.shape[1] != api.N_DIM:
            raise ValueError("waypoints must be [sum V][4]")
        if lim.dim() != 2 or lim.shape[0] != plan.n_paths or lim.shape[1] != 9:
            raise ValueError("limits must be [n_paths][9]")
        times = torch.empty(plan.n_segments, dtype=torch.float64, device=w.device)
        plan.ctx.use_torch_stream()
        plan.estimate_times(w, lim, times)
        ctx.plan = plan
        ctx.save_for_backward(w, lim)
        ctx.set_materialize_grads(False)
        return times

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_times):
        w, lim = ctx.saved_tensors
        want_w, want_l = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if grad_times is None or not (want_w or want_l):
            return None, None, None
        gw = torch.empty_like(w) if want_w else None
        gl = torch.empty_like(lim) if want_l else None
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.estimate_times_vjp(w, lim, grad_seg_times=grad_times.to(torch.float64).contiguous(), grad_waypoints=gw,
                                grad_limits=gl)
        return None, gw, gl


def estimate_times(plan, waypoints, limits):
    """seg_times [sum S] of Plan.estimate_times: the Euclidean segment-time estimate (the times a solve with
    estimate_times = 1 starts from, in the same bits) -- differentiable in waypoints [sum V][4] (x, y, z, unwrapped heading)
    and limits [n_paths][9] (float64 device tensors; entries 0, 1, 2 and 5 are read, the others get a zero gradient).  The
    gradient holds every branch of the forward fixed: the regime (horizontal / vertical), the 0.01 s floor (zero gradient),
    whether the heading term wins and its own two branches; Plan.estimate_times_vjp(term=...) reports the term per segment."""
    return _EstimateTimes.apply(plan, waypoints, limits)


class _EstimateTimesBaca(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, waypoints, limits):
        w = waypoints.detach().to(torch.float64).contiguous()
        lim = limits.detach().to(torch.float64).contiguous()
        if w.dim() != 2 or w.shape[0] != plan.n_segments + plan.n_paths or w.shape[1] != api.N_DIM:
            raise ValueError("waypoints must be [sum V][4]")
        if lim.dim() != 2 or lim.shape[0] != plan.n_paths or lim.shape[1] != 9:
            raise ValueError("limits must be [n_paths][9]")
        times = torch.empty(plan.n_segments, dtype=torch.float64, device=w.device)
        plan.ctx.use_torch_stream()
        plan.estimate_times_baca(w, lim, times)
        ctx.plan = plan
        ctx.save_for_backward(w, lim)
        ctx.set_materialize_grads(False)
        return times

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_times):
        w, lim = ctx.saved_tensors
        want_w, want_l = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if grad_times is None or not (want_w or want_l):
            return None, None, None
        gw = torch.empty_like(w) if want_w else None
        gl = torch.empty_like(lim) if want_l else None
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.estimate_times_baca_vjp(w, lim, grad_seg_times=grad_times.to(torch.float64).contiguous(), grad_waypoints=gw,
                                     grad_limits=gl)
        return None, gw, gl


def estimate_times_baca(plan, waypoints, limits):
    """seg_times [sum S] of Plan.estimate_times_baca: the Baca segment-time estimate (estimateSegmentTimesBaca, the reference's
    yardstick for the length of a trajectory) -- differentiable in waypoints [sum V][4] (x, y, z, unwrapped heading) and limits
    [n_paths][9] (float64 device tensors; entries 0 .. 7 are read, entry 8 gets a zero gradient).  The gradient holds every
    branch of the forward fixed: the inclination regime of v, a and j, the two caps, the clamped corners, the 0.01 s floor
    (zero gradient), whether the heading term wins and its own two branches; Plan.estimate_times_baca_vjp(flags=...) reports
    them per segment.  "Is this plan as long as the estimate allows" is a loss on its sum:

        >>> total = torch.zeros(plan.n_paths, dtype=torch.float64, device="cuda").index_add(0, path_of_segment,
        ...                                                                                  estimate_times_baca(plan, wp, lim))
        >>> torch.relu(n_samples * dt - 3.0 * total).sum().backward()

    The verdict itself (Plan.length_gate) is not differentiable and has no wrapper here."""
    return _EstimateTimesBaca.apply(plan, waypoints, limits)


_FLT_MAX = 3.4028234663852886e+38   # (double)FLT_MAX: a relaxed heading's limits (:1285-1288)


class _FallbackSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, waypoints, seg_times, sampling_dt, sample_capacity, stop_at, stopping_time):
        w = waypoints.detach().to(torch.float64).contiguous()
        t = seg_times.detach().to(torch.float64).contiguous()
        if w.dim() != 2 or w.shape[0] != plan.n_segments + plan.n_paths or w.shape[1] != api.N_DIM:
            raise ValueError("waypoints must be [sum V][4]")
        if t.dim() != 1 or t.shape[0] != plan.n_segments:
            raise ValueError("seg_times must be [sum S]")
        stop = None if stop_at is None else stop_at.detach().to(torch.uint8).contiguous()
        if stop is not None and (stop.dim() != 1 or stop.shape[0] != w.shape[0]):
            raise ValueError("stop_at must be [sum V]")
        cap = int(sample_capacity)
        n = torch.empty(plan.n_paths, dtype=torch.int32, device=w.device)
        # (the kernel writes the rows a path has; the rows at or beyond its count stay zero)
        out = torch.zeros((plan.n_paths, cap, api.N_DIM), dtype=torch.float64, device=w.device)
        plan.ctx.use_torch_stream()
        plan.fallback_sample(w, t, float(sampling_dt), cap, n, out, stop_at=stop, stopping_time=float(stopping_time))
        ctx.plan, ctx.dt, ctx.cap, ctx.stop, ctx.stopping_time = plan, float(sampling_dt), cap, stop, float(stopping_time)
        ctx.save_for_backward(t)
        ctx.mark_non_differentiable(n)
        ctx.set_materialize_grads(False)
        return out, n

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_n):
        (t,) = ctx.saved_tensors
        if grad_out is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None, None
        plan = ctx.plan
        gw = torch.empty((plan.n_segments + plan.n_paths, api.N_DIM), dtype=torch.float64, device=t.device)
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.fallback_sample_vjp(t, ctx.dt, ctx.cap, grad_out.to(torch.float64).contiguous(), gw, stop_at=ctx.stop,
                                 stopping_time=ctx.stopping_time)
        return None, gw, None, None, None, None, None


def fallback_sample(plan, waypoints, seg_times, sampling_dt, sample_capacity, stop_at=None, stopping_time=2.0):
    """(samples [n_paths][capacity][4], n_samples [n_paths] int32) of Plan.fallback_sample: the rows of findTrajectoryFallback
    -- constant-rate interpolation of the RAW waypoints [sum V][4] on seg_times [sum S] (the reference: the Baca estimate), a
    dwell of round(stopping_time / sampling_dt) repeated rows where stop_at [sum V] (uint8, optional) is set -- differentiable in
    waypoints (float64 device tensors).  Rows at or beyond a path's n_samples are zero (n_samples = capacity + 1: more rows than
    fit, the first capacity are there).  The counts are piecewise constant in seg_times and held fixed: seg_times gets no
    gradient.  All four columns carry the interpolation weights; the heading column is the almost-everywhere derivative, its
    wrap seams and the direction chosen at a heading difference of exactly pi held fixed.  The output is what path_deviation and
    waypoint_passage read."""
    return _FallbackSample.apply(plan, waypoints, seg_times, sampling_dt, sample_capacity, stop_at, stopping_time)


def fallback_trajectory(plan, waypoints, limits, sampling_dt, sample_capacity, stop_at=None, relax_heading=None,
                        speed_factor=1.0, accel_factor=1.0, stopping_time=2.0):
    """(samples, n_samples) of the reference's whole findTrajectoryFallback on the device: the headings of waypoints
    [sum V][4] unwrapped along every path (Plan.unwrap_headings), limits [n_paths][9] with entries 0, 1 times speed_factor and
    3, 4 times accel_factor (_fallback_sampling_speed_factor_, _accel_factor_) and entries 2, 5, 8 lifted to FLT_MAX where
    relax_heading [n_paths] (bool, optional) is set, the Baca estimate of that (Plan.estimate_times_baca, detached: the clock
    gets no gradient), then fallback_sample on the RAW waypoints -- differentiable in waypoints through the rows alone."""
    w = waypoints.detach().to(torch.float64).contiguous()
    lim = limits.detach().to(torch.float64).clone()
    # every shape is checked before the first launch: the unwrap and the clock below read and write [sum V] rows
    if w.dim() != 2 or w.shape[0] != plan.n_segments + plan.n_paths or w.shape[1] != api.N_DIM:
        raise ValueError("waypoints must be [sum V][4]")
    if lim.dim() != 2 or lim.shape[0] != plan.n_paths or lim.shape[1] != 9:
        raise ValueError("limits must be [n_paths][9]")
    if stop_at is not None and (stop_at.dim() != 1 or stop_at.shape[0] != w.shape[0]):
        raise ValueError("stop_at must be [sum V]")
    if relax_heading is not None:
        relax_heading = torch.as_tensor(relax_heading, device=lim.device).to(torch.bool)
        if relax_heading.dim() != 1 or relax_heading.shape[0] != plan.n_paths:
            raise ValueError("relax_heading must be [n_paths]")
    lim[:, 0:2] *= float(speed_factor)
    lim[:, 3:5] *= float(accel_factor)
    if relax_heading is not None:
        lim[:, [2, 5, 8]] = torch.where(relax_heading[:, None], torch.full_like(lim[:, [2, 5, 8]], _FLT_MAX), lim[:, [2, 5, 8]])
    unwrapped = torch.empty_like(w)
    times = torch.empty(plan.n_segments, dtype=torch.float64, device=w.device)
    plan.ctx.use_torch_stream()
    plan.unwrap_headings(w, unwrapped)
    plan.estimate_times_baca(unwrapped, lim.contiguous(), times)
    return fallback_sample(plan, waypoints, times, sampling_dt, sample_capacity, stop_at=stop_at, stopping_time=stopping_time)


class _TravelHeading(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, samples, n_samples, status, min_step):
        s, n = _rows_and_counts(plan, samples, n_samples)
        st = None if status is None else status.detach().to(torch.int32).contiguous()
        # (the kernel writes the rows a live path has; the rows behind them and the rows of a path with status <= 0 stay zero)
        out = torch.zeros_like(s)
        source = torch.full(s.shape[:2], -1, dtype=torch.int32, device=s.device)
        plan.ctx.use_torch_stream()
        plan.travel_heading(s, n, samples_out=out, status=st, min_step=float(min_step), source=source)
        ctx.plan, ctx.status, ctx.min_step = plan, st, float(min_step)
        ctx.save_for_backward(s, n)
        ctx.mark_non_differentiable(source)
        ctx.set_materialize_grads(False)
        return out, source

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_source):
        s, n = ctx.saved_tensors
        if grad_out is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        gs = torch.empty_like(s)
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.travel_heading_vjp(s, n, grad_out.to(torch.float64).contiguous(), gs, status=ctx.status, min_step=ctx.min_step)
        return None, gs, None, None, None


def travel_heading(plan, samples, n_samples, status=None, min_step=0.05):
    """(reference [n_paths][capacity][4], source [n_paths][capacity] int32) of Plan.travel_heading: the rows the tracker receives
    under override_heading_atan2 -- x, y, z of samples [n_paths][capacity][4], the heading of the rows 0 .. n-2 replaced by the
    direction of the step to the next row, a row that moves less than min_step keeping the heading of the row in front; row n-1
    keeps its own.  A fresh tensor, differentiable in samples (float64 device tensor; n_samples [n_paths] int32 as the sampler
    returned it); rows from n on and the rows of a path with status <= 0 (status [n_paths], optional) are zero and give zero.
    source is the row whose step gave a row's heading (-1 for row n-1 and behind).  The gradient holds the sources fixed: the
    heading of a run of slow rows flows into the two rows of its source's step, nothing into the headings the step replaces."""
    return _TravelHeading.apply(plan, samples, n_samples, status, min_step)


class _MutualClearance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, samples, n_samples, group_offsets, first_step, status, z_scale):
        s, n = _rows_and_counts(plan, samples, n_samples)
        fs = None if first_step is None else first_step.detach().to(torch.int32).contiguous()
        if fs is not None and (fs.dim() != 1 or fs.shape[0] != plan.n_paths):
            raise ValueError("first_step must be [n_paths]")
        st = None if status is None else status.detach().to(torch.int32).contiguous()
        g = plan._group_offsets_dev(group_offsets, s)
        # (a call without rows launches nothing: the neutral values are there beforehand)
        clearance = torch.full(s.shape[:2], float("inf"), dtype=torch.float64, device=s.device)
        partner = torch.full(s.shape[:2], -1, dtype=torch.int32, device=s.device)
        plan.ctx.use_torch_stream()
        plan.mutual_clearance(s, n, g, first_step=fs, status=st, z_scale=float(z_scale), clearance=clearance, partner=partner)
        ctx.plan, ctx.first_step, ctx.status, ctx.z_scale = plan, fs, st, float(z_scale)
        ctx.save_for_backward(s, n, g, partner)
        ctx.mark_non_differentiable(partner)
        ctx.set_materialize_grads(False)
        return clearance, partner

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_clearance, _grad_partner):
        s, n, g, partner = ctx.saved_tensors
        if grad_clearance is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None, None
        gs = torch.zeros_like(s)
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.mutual_clearance_vjp(s, n, g, partner, grad_clearance.to(torch.float64).contiguous(), gs, first_step=ctx.first_step,
                                  status=ctx.status, z_scale=ctx.z_scale)
        return None, gs, None, None, None, None, None


def mutual_clearance(plan, samples, n_samples, group_offsets, first_step=None, status=None, z_scale=1.0):
    """(clearance [n_paths][capacity], partner [n_paths][capacity] int32) of Plan.mutual_clearance: for every live row of samples
    [n_paths][capacity][4] the distance sqrt(dx^2 + dy^2 + (z_scale dz)^2) to the nearest OTHER path of the row's group at the
    same common step, and that path's index in the batch.  The groups (swarms) are contiguous runs of paths: group_offsets
    [n_groups + 1], a device int32 tensor or a host sequence (checked: starts at 0, does not decrease, ends at n_paths); row r
    of path p sits at step first_step[p] + r (first_step [n_paths] int32, None: all paths start together); n_samples [n_paths]
    int32 as the sampler returned it.  Differentiable in samples (float64 device tensor; x, y, z are read, column 3 gets a zero
    gradient).  Rows without a neighbour at their step, rows from n on and the rows of a path with status <= 0 (status
    [n_paths], optional) hold clearance +inf and partner -1 and get and give zero: relu(R - clearance) needs no mask.  The
    gradient holds every partner fixed; coincident rows (clearance 0) contribute zero.  A path counts only on the steps where
    it has rows -- to let a UAV hover at its last row, repeat that row up to the horizon and raise n_samples."""
    return _MutualClearance.apply(plan, samples, n_samples, group_offsets, first_step, status, z_scale)


class _ObstacleClearance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, samples, n_samples, obstacles, set_offsets, path_set, status, z_scale):
        s, n = _rows_and_counts(plan, samples, n_samples)
        ob = obstacles.detach().to(torch.float64).contiguous()
        if ob.dim() != 2 or ob.shape[1] != 4:
            raise ValueError("obstacles must be [n_obstacles][4]: x, y, z, radius")
        ps = None if path_set is None else path_set.detach().to(torch.int32).contiguous()
        if ps is not None and (ps.dim() != 1 or ps.shape[0] != plan.n_paths):
            raise ValueError("path_set must be [n_paths]")
        st = None if status is None else status.detach().to(torch.int32).contiguous()
        g = plan._set_offsets_dev([0, int(ob.shape[0])] if set_offsets is None else set_offsets, ob)
        # (a call without rows launches nothing: the neutral values are there beforehand)
        clearance = torch.full(s.shape[:2], float("inf"), dtype=torch.float64, device=s.device)
        nearest = torch.full(s.shape[:2], -1, dtype=torch.int32, device=s.device)
        plan.ctx.use_torch_stream()
        plan.obstacle_clearance(s, n, ob, g, path_set=ps, status=st, z_scale=float(z_scale), clearance=clearance, nearest=nearest)
        ctx.plan, ctx.path_set, ctx.status, ctx.z_scale = plan, ps, st, float(z_scale)
        ctx.save_for_backward(s, n, ob, g, nearest)
        ctx.mark_non_differentiable(nearest)
        ctx.set_materialize_grads(False)
        return clearance, nearest

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_clearance, _grad_nearest):
        s, n, ob, g, nearest = ctx.saved_tensors
        if grad_clearance is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None, None, None
        gs = torch.zeros_like(s)
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.obstacle_clearance_vjp(s, n, ob, g, nearest, grad_clearance.to(torch.float64).contiguous(), gs,
                                    path_set=ctx.path_set, status=ctx.status, z_scale=ctx.z_scale)
        return None, gs, None, None, None, None, None, None


def obstacle_clearance(plan, samples, n_samples, obstacles, set_offsets=None, path_set=None, status=None, z_scale=1.0):
    """(clearance [n_paths][capacity], nearest [n_paths][capacity] int32) of Plan.obstacle_clearance: for every live row of
    samples [n_paths][capacity][4] the signed distance sqrt(dx^2 + dy^2 + (z_scale dz)^2) - radius to the nearest obstacle of
    the path's set (negative inside a sphere), and that obstacle's index in the whole array.  obstacles [n_obstacles][4] =
    (x, y, z, radius), a radius of 0 a point of a cloud; the sets are contiguous runs of obstacles: set_offsets [n_sets + 1], a
    device int32 tensor or a host sequence (checked: starts at 0, does not decrease, ends at n_obstacles), None: one set that
    holds every obstacle; path_set [n_paths] int32 names every path's set (None: set 0; an entry outside [0, n_sets): no
    obstacle); n_samples [n_paths] int32 as the sampler returned it.  Differentiable in samples ONLY (float64 device tensor; x,
    y, z are read, column 3 gets a zero gradient): the obstacles are a static map, and asking for their gradient raises
    instead of returning None.  Rows of a path that sees no obstacle, rows from n on and the rows of a path with status <= 0
    (status [n_paths], optional) hold clearance +inf and nearest -1 and get a zero gradient: relu(R - clearance) needs no
    mask.  The gradient holds every nearest obstacle fixed; a row on an obstacle's centre contributes zero."""
    if isinstance(obstacles, torch.Tensor) and obstacles.requires_grad:
        raise ValueError("obstacle_clearance has no gradient with respect to the obstacles (a static map): pass "
                         "obstacles.detach()")
    return _ObstacleClearance.apply(plan, samples, n_samples, obstacles, set_offsets, path_set, status, z_scale)


class _FieldClearance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, samples, n_samples, fields, geometry, path_field, status, outside_value):
        s, n = _rows_and_counts(plan, samples, n_samples)
        fl = fields.detach().to(torch.float64).contiguous()
        if fl.dim() != 4:
            raise ValueError("fields must be [n_fields][nz][ny][nx]")
        pf = None if path_field is None else path_field.detach().to(torch.int32).contiguous()
        if pf is not None and (pf.dim() != 1 or pf.shape[0] != plan.n_paths):
            raise ValueError("path_field must be [n_paths]")
        st = None if status is None else status.detach().to(torch.int32).contiguous()
        # (a call without rows launches nothing: the neutral values are there beforehand)
        P = plan.n_paths
        clearance = torch.full(s.shape[:2], float("inf"), dtype=torch.float64, device=s.device)
        cell = torch.full(s.shape[:2], -1, dtype=torch.int32, device=s.device)
        least = torch.full((P,), float("inf"), dtype=torch.float64, device=s.device)
        argmin = torch.full((P, 2), -1, dtype=torch.int32, device=s.device)
        plan.ctx.use_torch_stream()
        plan.field_clearance(s, n, fl, geometry, path_field=pf, status=st, outside_value=float(outside_value),
                             clearance=clearance, cell=cell, min_clearance=least, argmin=argmin)
        ctx.plan, ctx.geometry, ctx.path_field, ctx.status = plan, geometry, pf, st
        ctx.save_for_backward(s, n, fl, cell, argmin)
        ctx.mark_non_differentiable(cell, argmin)
        ctx.set_materialize_grads(False)
        return clearance, cell, least, argmin

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_clearance, _grad_cell, grad_least, _grad_argmin):
        s, n, fl, cell, argmin = ctx.saved_tensors
        if (grad_clearance is None and grad_least is None) or not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None, None, None
        up = torch.zeros(s.shape[:2], dtype=torch.float64, device=s.device) if grad_clearance is None \
            else grad_clearance.to(torch.float64).contiguous().clone()
        if grad_least is not None and s.shape[1] > 0:
            # the minimum is the clearance of its argmin row: its upstream goes there (nowhere for a path without a minimum)
            row = argmin[:, 0].to(torch.int64)
            has = row >= 0
            up[has.nonzero(as_tuple=True)[0], row[has]] += grad_least.to(torch.float64)[has]
        gs = torch.zeros_like(s)
        plan = ctx.plan
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.field_clearance_vjp(s, n, fl, ctx.geometry, cell, up, gs, path_field=ctx.path_field, status=ctx.status)
        return None, gs, None, None, None, None, None, None


def field_clearance(plan, samples, n_samples, fields, geometry, path_field=None, status=None, outside_value=float("inf")):
    """(clearance [n_paths][capacity], cell [n_paths][capacity] int32, min_clearance [n_paths], argmin [n_paths][2] int32) of
    Plan.field_clearance: for every live row of samples [n_paths][capacity][4] the trilinear interpolant of the voxel grid of
    signed distances its path sees, the index of the cell's low corner in the whole fields array, per path the least
    clearance and {row, cell} of the first row that has it.  fields [n_fields][nz][ny][nx] float64 on the device, x fastest,
    node-centred, with geometry an api.FieldGeometry (origin, spacing, dims, n_fields; checked); path_field [n_paths] int32
    names every path's grid (None: grid 0; an entry outside [0, n_fields): none); n_samples [n_paths] int32 as the sampler
    returned it; outside_value is what a live row outside the grid gets (+inf: unknown space is free; a negative value: it is
    occupied), with cell -1.  Differentiable in samples ONLY (float64 device tensor; x, y, z are read, column 3 gets a zero
    gradient), through clearance and through min_clearance, whose gradient goes to its argmin row: the field is a static
    map, and asking for its gradient raises instead of returning None.  Rows outside the grid, rows of a path without a grid,
    rows from n on and the rows of a path with status <= 0 (status [n_paths], optional) have cell -1 and get a zero gradient;
    the last three hold clearance +inf, so relu(R - clearance) needs no mask.  The gradient holds every cell fixed: it is the
    gradient of the trilinear interpolant inside the cell the forward chose, which jumps across cell faces."""
    if isinstance(fields, torch.Tensor) and fields.requires_grad:
        raise ValueError("field_clearance has no gradient with respect to the field (a static map): pass fields.detach()")
    return _FieldClearance.apply(plan, samples, n_samples, fields, geometry, path_field, status, outside_value)


class _InitialCondition(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, tracker, uav_pose, pos, vel, acc, jerk, fixed):
        P = plan.n_paths
        tr, uav = _f64(tracker), _f64(uav_pose)
        pred = tuple(_f64(a) for a in (pos, vel, acc, jerk))
        if tr.shape != (P, 4, 4) or uav.shape != (P, 4):
            raise ValueError("tracker must be [n_paths][4][4] and uav_pose [n_paths][4]")
        if any(a.dim() != 3 or a.shape != pred[0].shape or a.shape[0] != P or a.shape[2] != api.N_DIM for a in pred):
            raise ValueError("the prediction's four arrays must be [n_paths][pred_capacity][4]")
        dev = tr.device
        decision = torch.empty(P, dtype=torch.int32, device=dev)
        k = torch.empty(P, dtype=torch.int32, device=dev)
        initial = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
        plan.ctx.use_torch_stream()
        plan.initial_condition(_i32(fixed["flags"]), tr, _f64(fixed["tracker_age"]), uav, fixed["takeoff_height"],
                               _f64(fixed["path_time_offset"]), _i32(fixed["vertex_offsets"]), pred, _i32(fixed["n_pred"]),
                               decision, k, initial)
        ctx.plan, ctx.pred_capacity = plan, pred[0].shape[1]
        ctx.save_for_backward(decision, k)
        ctx.mark_non_differentiable(decision, k)
        ctx.set_materialize_grads(False)
        return initial, decision, k

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_initial, *_):
        decision, k = ctx.saved_tensors
        if grad_initial is None or not any(ctx.needs_input_grad[1:7]):
            return (None,) * 8
        plan, P, dev = ctx.plan, ctx.plan.n_paths, decision.device
        gt = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
        gu = torch.empty((P, 4), dtype=torch.float64, device=dev)
        gp = tuple(torch.empty((P, ctx.pred_capacity, api.N_DIM), dtype=torch.float64, device=dev) for _ in range(4))
        plan.ctx.use_torch_stream()
        plan.initial_condition_vjp(decision, k, grad_initial.to(torch.float64).contiguous(), gt, gu, gp)
        return (None, gt, gu) + gp + (None,)


def initial_condition(plan, flags, tracker, tracker_age, uav_pose, takeoff_height, path_time_offset, vertex_offsets, prediction,
                      n_pred):
    """(initial [n_paths][4][4], decision [n_paths] int32, sample_offset [n_paths] int32) of Plan.initial_condition:
    prepareInitialCondition for every path -- row 0 of a block the waypoint to prepend, rows 1 .. 3 the derivatives, zeros where
    the decision has no api.IC_PREPEND.  Differentiable in tracker [n_paths][4][4], uav_pose [n_paths][4] and the four prediction
    arrays (a tuple position, velocity, acceleration, jerk, [n_paths][pred_capacity][4] each): every value is a copy, so the
    gradient of a block lands on the tracker command, on the UAV pose (row 0) or on row k of the prediction, whichever the
    decision took.  The decision and k are piecewise constant and held fixed.  Device tensors."""
    fixed = dict(flags=flags, tracker_age=tracker_age, takeoff_height=float(takeoff_height), path_time_offset=path_time_offset,
                 vertex_offsets=vertex_offsets, n_pred=n_pred)
    pos, vel, acc, jerk = prediction
    return _InitialCondition.apply(plan, tracker, uav_pose, pos, vel, acc, jerk, fixed)


class _PrependInitialCondition(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, waypoints, initial, vertex_offsets, decision, stop_at):
        w, ini = _f64(waypoints).reshape(-1, api.N_DIM), _f64(initial)
        vo, dec = _i32(vertex_offsets), _i32(decision)
        P, n_v, dev = plan.n_paths, w.shape[0], w.device
        if ini.shape != (P, 4, 4) or vo.shape != (P + 1,) or dec.shape != (P,):
            raise ValueError("initial must be [n_paths][4][4], vertex_offsets [n_paths + 1] and decision [n_paths]")
        stop = None if stop_at is None else stop_at.detach().to(torch.uint8).contiguous()
        offsets = torch.empty(P + 1, dtype=torch.int32, device=dev)
        out = torch.empty((n_v + P, api.N_DIM), dtype=torch.float64, device=dev)
        stop_out = torch.empty(n_v + P, dtype=torch.uint8, device=dev)
        source = torch.empty(n_v + P, dtype=torch.int32, device=dev)
        plan.ctx.use_torch_stream()
        plan.prepend_initial_condition(vo, w, dec, ini, offsets, out, stop_at=stop, stop_at_out=stop_out, source=source)
        total = int(offsets[-1].item())   # the one readback: the caller needs the offsets on the host for the next plan anyway
        out, stop_out, source = out[:total], stop_out[:total], source[:total]
        ctx.plan, ctx.n_v = plan, n_v
        ctx.save_for_backward(vo, dec, offsets)
        ctx.mark_non_differentiable(stop_out, source, offsets)
        ctx.set_materialize_grads(False)
        return out, stop_out, source, offsets

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, *_):
        vo, dec, offsets = ctx.saved_tensors
        if grad_out is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return (None,) * 6
        plan, P, dev = ctx.plan, ctx.plan.n_paths, vo.device
        gw = torch.empty((ctx.n_v, api.N_DIM), dtype=torch.float64, device=dev)
        row = torch.empty((P, api.N_DIM), dtype=torch.float64, device=dev)
        plan.ctx.use_torch_stream()
        plan.prepend_initial_condition_vjp(vo, dec, offsets, grad_out.to(torch.float64).contiguous(), gw, row)
        gi = torch.zeros((P, 4, 4), dtype=torch.float64, device=dev)
        gi[:, 0, :] = row
        return None, gw, gi, None, None, None


def prepend_initial_condition(plan, waypoints, initial, vertex_offsets, decision, stop_at=None):
    """(waypoints [sum V'][4], stop_at [sum V'] uint8, source [sum V'] int32, offsets [n_paths + 1] int32) of
    Plan.prepend_initial_condition: per path the first requested waypoint dropped where decision has api.IC_DROP_FIRST, row 0 of
    initial [n_paths][4][4] put in front where it has api.IC_PREPEND.  waypoints [n_vertices][4] are addressed by vertex_offsets
    [n_paths + 1] int32; a path may request no waypoint or one.  Differentiable in waypoints and in row 0 of initial (copies; a
    dropped vertex gets a zero row).  The edited batch is what a plan is created on (offsets minus arange, once every path has two
    vertices).  One readback (the offsets) per call."""
    return _PrependInitialCondition.apply(plan, waypoints, initial, vertex_offsets, decision, stop_at)


class _SplicePrediction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, samples, pred_position, n_samples, status, fixed):
        s, pp, n = _f64(samples), _f64(pred_position), _i32(n_samples)
        P = plan.n_paths
        if s.dim() != 3 or s.shape[0] != P or s.shape[2] != api.N_DIM or pp.dim() != 3 or pp.shape[0] != P or pp.shape[2] != api.N_DIM:
            raise ValueError("samples must be [n_paths][capacity][4] and the prediction's positions [n_paths][pred_capacity][4]")
        st = None if status is None else _i32(status)
        dec, k, age, n_pred = _i32(fixed["decision"]), _i32(fixed["sample_offset"]), _f64(fixed["prediction_age"]), _i32(fixed["n_pred"])
        # (the kernel writes the rows a live path has; the rows behind them and the rows of a path with status <= 0 stay zero)
        out = torch.zeros_like(s)
        n_out = torch.empty_like(n)
        st_out = torch.empty_like(n)
        plan.ctx.use_torch_stream()
        plan.splice_prediction(s, n, dec, k, age, pp, n_pred, samples_out=out, n_samples_out=n_out, status=st, status_out=st_out)
        ctx.plan, ctx.status, ctx.shapes = plan, st, (s.shape, pp.shape)
        ctx.save_for_backward(n, dec, k, age, n_pred)
        ctx.mark_non_differentiable(n_out, st_out)
        ctx.set_materialize_grads(False)
        return out, n_out, st_out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, *_):
        n, dec, k, age, n_pred = ctx.saved_tensors
        if grad_out is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return (None,) * 6
        plan = ctx.plan
        gs = torch.empty(ctx.shapes[0], dtype=torch.float64, device=n.device)
        gp = torch.empty(ctx.shapes[1], dtype=torch.float64, device=n.device)
        plan.ctx.use_torch_stream()
        plan.splice_prediction_vjp(n, dec, k, age, n_pred, grad_out.to(torch.float64).contiguous(), gs, gp, status=ctx.status)
        return None, gs, gp, None, None, None


def splice_prediction(plan, samples, n_samples, decision, sample_offset, prediction_age, pred_position, n_pred, status=None):
    """(samples [n_paths][capacity][4], n_samples [n_paths] int32, status [n_paths] int32) of Plan.splice_prediction, out of
    place: the first k = sample_offset rows of the prediction's positions in front of the samples of every live path from the
    future whose k exceeds the prediction's current index; every other live path's rows copied; rows behind a path's count and
    the rows of a path with status <= 0 are zero.  A count above the capacity means nothing was spliced; status -2 means the
    prediction has fewer than k rows.  Differentiable in samples and pred_position [n_paths][pred_capacity][4] (copies); the
    decision, k and the counts are held fixed."""
    fixed = dict(decision=decision, sample_offset=sample_offset, prediction_age=prediction_age, n_pred=n_pred)
    return _SplicePrediction.apply(plan, samples, pred_position, n_samples, status, fixed)


def _u8(t):
    return None if t is None else t.detach().to(torch.uint8).contiguous()


class _RequestVertices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, waypoints, state, has_state, stop_at, derivative):
        w = _f64(waypoints)
        P, n_v, dev = plan.n_paths, plan.n_segments + plan.n_paths, w.device
        if w.dim() != 2 or w.shape[0] != n_v or w.shape[1] != api.N_DIM:
            raise ValueError("waypoints must be [sum V][4]")
        st = None if state is None else _f64(state)
        if st is not None and st.shape != (P, 4, 4):
            raise ValueError("state must be [n_paths][4][4]")
        has = None
        if st is not None:
            has = torch.ones(P, dtype=torch.uint8, device=dev) if has_state is None else _u8(has_state)
            if has.shape != (P,):
                raise ValueError("has_state must be [n_paths]")
        unwrapped = torch.empty_like(w)
        mask = torch.empty((n_v, 5), dtype=torch.uint8, device=dev)
        vals = torch.empty((n_v, 5, api.N_DIM), dtype=torch.float64, device=dev)
        plan.ctx.use_torch_stream()
        plan.request_vertices(w, unwrapped, mask, vals, stop_at=_u8(stop_at), has_state=has, state=st,
                              derivative_to_optimize=int(derivative))
        ctx.plan, ctx.has = plan, has
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)
        return unwrapped, mask, vals

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_unwrapped, _grad_mask, grad_vals):
        want_w, want_s = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if (grad_unwrapped is None and grad_vals is None) or not (want_w or want_s):
            return (None,) * 6
        plan, P, n_v = ctx.plan, ctx.plan.n_paths, ctx.plan.n_segments + ctx.plan.n_paths
        dev = (grad_vals if grad_unwrapped is None else grad_unwrapped).device
        gw = torch.empty((n_v, api.N_DIM), dtype=torch.float64, device=dev) if want_w else None
        gs = torch.empty((P, 4, 4), dtype=torch.float64, device=dev) if want_s else None
        plan.ctx.use_torch_stream()
        plan.request_vertices_vjp(None if grad_unwrapped is None else grad_unwrapped.to(torch.float64).contiguous(),
                                  None if grad_vals is None else grad_vals.to(torch.float64).contiguous(), gw, gs, has_state=ctx.has)
        return None, gw, gs, None, None, None


def request_vertices(plan, waypoints, state=None, has_state=None, stop_at=None, derivative_to_optimize=4):
    """(unwrapped [sum V][4], mask [sum V][5] uint8, values [sum V][5][4]) of Plan.request_vertices: the vertices findTrajectory
    builds from the RAW waypoints [sum V][4] of a request -- the headings unwrapped along every path, from the heading of state
    [n_paths][4][4] (row 0 column 3; rows 1 .. 3 velocity, acceleration, jerk: the block initial_condition returns) where
    has_state [n_paths] says so (None: every path, if state is given), the state's rows fixed at the first vertex.
    Differentiable in waypoints and state, every branch held fixed: the unwrap adds a piecewise-constant multiple of 2 pi, so a
    waypoint collects the gradients of its unwrapped row and of its position values, the state's rows 1 .. 3 those of the first
    vertex's value rows, and the state's heading nothing.  With it the chain request -> vertices -> times -> solve -> samples ->
    loss starts at the raw request."""
    return _RequestVertices.apply(plan, waypoints, state, has_state, stop_at, derivative_to_optimize)


class _RequestLimits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, constraints, override, fixed):
        c = _f64(constraints)
        P, dev = plan.n_paths, c.device
        if c.shape != (P, 12):
            raise ValueError("constraints must be [n_paths][12]")
        o = None if override is None else _f64(override)
        if o is not None and o.shape != (P, 6):
            raise ValueError("override must be [n_paths][6]")
        flags = None if fixed["flags"] is None else _i32(fixed["flags"])
        st = None if fixed["state"] is None else _f64(fixed["state"])
        has = None
        if st is not None:
            has = torch.ones(P, dtype=torch.uint8, device=dev) if fixed["has_state"] is None else _u8(fixed["has_state"])
        limits = torch.empty((P, 9), dtype=torch.float64, device=dev)
        branch = torch.empty(P, dtype=torch.int32, device=dev)
        ctx.factors = dict(fallback=bool(fixed["fallback"]), speed_factor=float(fixed["speed_factor"]),
                           accel_factor=float(fixed["accel_factor"]))
        plan.ctx.use_torch_stream()
        plan.request_limits(c, limits, branch, override=o, flags=flags, has_state=has, state=st, **ctx.factors)
        ctx.plan = plan
        ctx.save_for_backward(branch)
        ctx.mark_non_differentiable(branch)
        ctx.set_materialize_grads(False)
        return limits, branch

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_limits, _grad_branch):
        want_c, want_o = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if grad_limits is None or not (want_c or want_o):
            return None, None, None, None
        (branch,) = ctx.saved_tensors
        P, dev = ctx.plan.n_paths, branch.device
        gc = torch.empty((P, 12), dtype=torch.float64, device=dev) if want_c else None
        go = torch.empty((P, 6), dtype=torch.float64, device=dev) if want_o else None
        ctx.plan.ctx.use_torch_stream()
        ctx.plan.request_limits_vjp(branch, grad_limits.to(torch.float64).contiguous(), gc, go, **ctx.factors)
        return None, gc, go, None


def request_limits(plan, constraints, override=None, flags=None, state=None, has_state=None, fallback=False, speed_factor=1.0,
                   accel_factor=1.0, return_branch=False):
    """limits [n_paths][9] of Plan.request_limits (with return_branch: (limits, branch [n_paths] int32, api.LIM_*)): what
    findTrajectory (fallback: findTrajectoryFallback) derives from constraints [n_paths][12], override [n_paths][6] with flags
    [n_paths] int32 (api.REQ_*) and the state.  Differentiable in constraints and override, the branch word held fixed: the
    entry that supplied a limit gets its gradient (times the fallback's factor on the four scaled entries) -- the override entry
    where the override was taken, else the smaller side of a vertical pair; a relaxed heading limit and the state get nothing."""
    fixed = dict(flags=flags, state=state, has_state=has_state, fallback=fallback, speed_factor=speed_factor,
                 accel_factor=accel_factor)
    limits, branch = _RequestLimits.apply(plan, constraints, override, fixed)
    return (limits, branch) if return_branch else limits


class _PathEdit(torch.autograd.Function):
    """both edit steps: thin (segment_max None) or subdivide; the outputs cut to the edited batch's size, which the forward reads
    back with the offsets"""

    @staticmethod
    def forward(ctx, plan, waypoints, stop_at, segment_max, args):
        w = waypoints.detach().to(torch.float64).contiguous()
        n_v = plan.n_segments + plan.n_paths
        if w.dim() != 2 or w.shape[0] != n_v or w.shape[1] != api.N_DIM:
            raise ValueError("waypoints must be [sum V][4]")
        stop = None if stop_at is None else stop_at.detach().to(torch.uint8).contiguous()
        if stop is not None and (stop.dim() != 1 or stop.shape[0] != n_v):
            raise ValueError("stop_at must be [sum V]")
        dev = w.device
        subdivide = segment_max is not None
        upper = n_v + (plan.n_segments if subdivide else 0)
        offsets = torch.empty(plan.n_paths + 1, dtype=torch.int32, device=dev)
        out = torch.empty((upper, api.N_DIM), dtype=torch.float64, device=dev)
        stop_out = torch.empty(upper, dtype=torch.uint8, device=dev)
        source = torch.empty(upper, dtype=torch.int32, device=dev)
        inserted = torch.empty(upper, dtype=torch.uint8, device=dev) if subdivide else None
        plan.ctx.use_torch_stream()
        if subdivide:
            m = segment_max.detach().to(torch.float64).contiguous()
            if m.dim() != 1 or m.shape[0] != plan.n_segments:
                raise ValueError("segment_max must be [sum S]")
            active = args.get("active")
            if active is not None:
                active = active.detach().to(torch.uint8).contiguous()
                if active.dim() != 1 or active.shape[0] != plan.n_paths:
                    raise ValueError("active must be [n_paths]")
            plan.insert_midpoints(w, m, args["max_deviation"], offsets, out, first_segment=args["first_segment"], stop_at=stop,
                                  active=active, stop_at_out=stop_out, source=source, inserted=inserted)
        else:
            plan.preprocess_path(w, offsets, out, min_waypoint_distance=args["min_waypoint_distance"], stop_at=stop,
                                 straightener_enabled=args["straightener_enabled"],
                                 straightener_max_deviation=args["straightener_max_deviation"],
                                 straightener_max_hdg_deviation=args["straightener_max_hdg_deviation"], stop_at_out=stop_out,
                                 source=source)
        total = int(offsets[-1].item())   # the one readback: the caller needs the offsets on the host for the next plan anyway
        out, stop_out, source = out[:total], stop_out[:total], source[:total]
        inserted = inserted[:total] if subdivide else torch.zeros(0, dtype=torch.uint8, device=dev)
        ctx.plan, ctx.subdivide = plan, subdivide
        ctx.save_for_backward(offsets, source, inserted)
        ctx.mark_non_differentiable(stop_out, source, inserted, offsets)
        ctx.set_materialize_grads(False)
        return out, stop_out, source, inserted, offsets

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, *_):
        offsets, source, inserted = ctx.saved_tensors
        if grad_out is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        plan = ctx.plan
        gw = torch.empty((plan.n_segments + plan.n_paths, api.N_DIM), dtype=torch.float64, device=source.device)
        plan.ctx.use_torch_stream()   # (the autograd engine runs this on its own thread, on the forward's stream)
        plan.path_edit_vjp(offsets, source, grad_out.to(torch.float64).contiguous(), gw,
                           inserted=inserted if ctx.subdivide else None)
        return None, gw, None, None, None


def _edited_plan(plan, offsets):
    off = offsets.cpu().numpy().astype("int64")
    return api.Plan(plan.ctx, off - np.arange(off.size))   # a path of V vertices has V - 1 segments


def preprocess_path(plan, waypoints, min_waypoint_distance=0.05, stop_at=None, straightener_enabled=False,
                    straightener_max_deviation=0.0, straightener_max_hdg_deviation=0.0):
    """(new plan, waypoints [sum V'][4], stop_at [sum V'] uint8, source [sum V'] int32) of Plan.preprocess_path: preprocessPath's
    thinning of waypoints [sum V][4] (raw headings; stop_at [sum V] uint8, optional) -- the packed batch the new plan is created
    on.  The kept rows are copies: differentiable in waypoints through Plan.path_edit_vjp, a dropped vertex gets a zero row; which
    vertices are kept is piecewise constant and held fixed.  source[k] is the input vertex row k copies.  One readback (the
    offsets) per call."""
    args = dict(min_waypoint_distance=float(min_waypoint_distance), straightener_enabled=bool(straightener_enabled),
                straightener_max_deviation=float(straightener_max_deviation),
                straightener_max_hdg_deviation=float(straightener_max_hdg_deviation))
    out, stop_out, source, _, offsets = _PathEdit.apply(plan, waypoints, stop_at, None, args)
    return _edited_plan(plan, offsets), out, stop_out, source


def insert_midpoints(plan, waypoints, segment_max, max_deviation, first_segment=True, stop_at=None, active=None):
    """(new plan, waypoints [sum V'][4], stop_at [sum V'] uint8, source [sum V'] int32, inserted [sum V'] uint8) of
    Plan.insert_midpoints: a mid-point into every segment whose segment_max [sum S] (path_deviation's fourth result) exceeds
    max_deviation, by the reference's rule, for the paths active [n_paths] (optional: all) marks.  Differentiable in waypoints
    through Plan.path_edit_vjp: a copy carries its gradient, a mid-point gives half of its to each end of its segment, all four
    columns alike (the heading column is the almost-everywhere derivative of radians::interp, its wrap held fixed); which
    segments are subdivided is held fixed, segment_max gets no gradient.  Raises when a subdivided path is longer than a plan
    takes (api.MrsTgError from mrs_tg_plan_create).  One readback (the offsets) per call."""
    args = dict(max_deviation=float(max_deviation), first_segment=bool(first_segment), active=active)
    out, stop_out, source, inserted, offsets = _PathEdit.apply(plan, waypoints, stop_at, segment_max, args)
    return _edited_plan(plan, offsets), out, stop_out, source, inserted


def _root(x, p):
    """x^(1/p) for x >= 0 with a finite gradient everywhere: 0 at x = 0 (where the root is never the active term of the
    scaling unless every term is 0, and the max(1, ...) then holds)"""
    pos = x > 0
    safe = torch.where(pos, x, torch.ones_like(x))
    r = torch.sqrt(safe) if p == 2 else torch.pow(safe, 1.0 / 3.0)
    return torch.where(pos, r, torch.zeros_like(x))


def scale_times_to_limits(plan, coeffs, seg_times, limits, status=None):
    """The product's one-sweep feasibility step (violation_scaling in mrs_tg_device.hpp) in torch on top
    of segment_maxima: T_i max(1, max_g v_g / v_lim_g, sqrt(max_g a_g / a_lim_g), cbrt(max_g j_g / j_lim_g)) per segment,
    limits [n_paths][9] indexed 3 (k-1) + group in the plan's (caller's) path order.  Segments of paths with status <= 0
    (status [n_paths], optional) keep their times; their maxima are set aside before the division, so that what the solve
    left in their coefficients (NaN included) reaches neither the scaling nor any gradient.  The maxima are combined with
    fmax, as violation_scaling combines them (a NaN term is ignored).  Differentiable in coeffs, seg_times and limits."""
    dev = seg_times.device
    so = torch.as_tensor(plan.seg_offsets, dtype=torch.int64, device=dev)
    counts = so[1:] - so[:-1]
    path_of_seg = torch.repeat_interleave(torch.arange(plan.n_paths, device=dev), counts, output_size=plan.n_segments)
    mx = segment_maxima(plan, coeffs, seg_times)
    keep = None
    if status is not None:
        keep = status.to(dev)[path_of_seg] > 0
        mx = torch.where(keep[:, None, None], mx, torch.zeros_like(mx))
    lim = limits.to(torch.float64).reshape(plan.n_paths, 3, 3)[path_of_seg]
    ratio = mx / lim
    viol = torch.fmax(torch.fmax(ratio[:, :, 0], ratio[:, :, 1]), ratio[:, :, 2])   # [sum S][3]: over the groups, per k
    one = torch.ones_like(viol[:, 0])
    s = torch.fmax(one, torch.fmax(torch.fmax(viol[:, 0], _root(viol[:, 1], 2)), _root(viol[:, 2], 3)))
    if keep is not None:
        s = torch.where(keep, s, one)
    return seg_times * s
