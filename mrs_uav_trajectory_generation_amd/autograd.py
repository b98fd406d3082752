"""The fixed-times solve as a torch.autograd.Function: gradients of a loss on the coefficients and the cost reach the fixed
values (waypoints, initial state) and the segment times.

Forward: Plan.solve with time_alloc_method = NONE, no sampling, no waypoints, no limits (the existing kernels, unchanged).
Backward: Plan.solve_vjp (mrs_tg_plan_solve_vjp, vjp_kernel), the exact chain rule of the linear QP at the returned solution
(DESIGN.md section 4c).  Differentiated: fixed_values and seg_times.  Not differentiated: time allocation, feasibility scaling,
limits, sampling, second derivatives.  Both passes run on torch's current stream of the thread that runs them: the call binds
the plan's context to it (Context.use_torch_stream), and the context stays bound afterwards.

    >>> fv = fixed_values.clone(); fv[:, 0, :] = waypoints; coeffs, cost, status = solve(plan, fixed_mask, fv, seg_times)
"""
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
