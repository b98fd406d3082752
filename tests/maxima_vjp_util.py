"""Shared helpers of the segment-maxima backward-pass tests (test_maxima_vjp_host.py, test_gpu_maxima_vjp.py): the fixtures,
the CPU harness of csrc/mrs_tg_maxima_vjp.hpp, and torch restatements of |p^(k)(t*)| and of the feasibility scaling."""
import functools

import numpy as np

from tests import host_harness as hh

load_cases = functools.partial(hh.load_cases, "maxima_vjp_cases.json")
load_composite_cases = functools.partial(hh.load_cases, "maxima_vjp_composite_cases.json")
build_harness = functools.partial(hh.build, "maxima_vjp_harness.cpp")   # (tmp_path, sanitize=False)
N, D = 10, 4
GROUPS = ((0, 1), (2,), (3,))
GRID = 32   # the forward search's grid cells (kGridCells, mrs_tg_maxima.hpp)


def cell_of(tau):
    """the grid cell [lo, hi] the forward's search gives a winner at tau: the polished cell for an interior point, the cell at
    an end point"""
    if tau <= 0.0:
        return 0.0, 1.0 / GRID
    if tau >= 1.0:
        return (GRID - 1) / GRID, 1.0
    i = min(int(tau * GRID), GRID - 1)
    return i / GRID, (i + 1) / GRID if i + 1 < GRID else 1.0


def run_harness(exe, problems, env=None):
    """problems: dicts with coeffs [4][10], T, seeds [9][4] (tau_seed, lo, hi, G).
    -> list of (grad_coeffs [4][10], grad_T, t* [9])"""
    lines = []
    for p in problems:
        vals = list(np.asarray(p["coeffs"], dtype=np.float64).reshape(-1)) + [float(p["T"])] + \
            list(np.asarray(p["seeds"], dtype=np.float64).reshape(-1))
        lines.append(hh.fmt(vals) + "\n")
    out = hh.run(exe, lines, len(problems), env=env)
    res = []
    for line in out:
        x = np.array([float(v) for v in line.split()])
        assert x.size == D * N + 1 + 9
        res.append((x[:D * N].reshape(D, N), x[D * N], x[D * N + 1:]))
    return res


def one_hot_problems(case, taus):
    """one problem per entry w of the case: upstream e_w, every entry seeded at taus[w] in its grid cell"""
    probs = []
    for w in range(9):
        seeds = []
        for v in range(9):
            lo, hi = cell_of(taus[v])
            seeds.append((taus[v], lo, hi, 1.0 if v == w else 0.0))
        probs.append(dict(coeffs=case["coeffs"], T=case["T"], seeds=seeds))
    return probs


def entry_error(gc, gT, ref):
    """|got - fixture| over the entry's 41 gradients, relative to the entry's largest component"""
    rc = np.array(ref["grad_coeffs"])
    scale = max(np.max(np.abs(rc)), abs(ref["grad_T"]), 1e-300)
    return max(np.max(np.abs(gc - rc)), abs(gT - ref["grad_T"])) / scale


# ------------------------------------------------------------------------------------------------------------------------
# torch restatements

def derivative_at(torch, coeffs, t, k):
    """p^(k)(t) [sum S][9][4] for coeffs [sum S][4][10] and t [sum S][9] (one abscissa per entry), by powers of t"""
    j = torch.arange(N, dtype=torch.float64, device=coeffs.device)
    fall = torch.ones(N, dtype=torch.float64, device=coeffs.device)
    for n in range(k):
        fall = fall * (j - n)
    e = (j - k).clamp(min=0)
    tp = torch.where(j >= k, t.unsqueeze(-1) ** e, torch.zeros((), dtype=torch.float64, device=coeffs.device))  # [S][9][10]
    return torch.einsum("sdj,swj->swd", coeffs * fall, tp)


def magnitudes_at(torch, coeffs, argmax, absolute=False):
    """|p^(k)(t*)| [sum S][3][3] of every entry at its own t* (argmax [sum S][3][3] in seconds); differentiable in coeffs and
    argmax.  absolute: the same with |c| and |t|, the magnitude sum that bounds the evaluation's rounding"""
    out = []
    t = argmax.reshape(-1, 9)
    if absolute:
        t = t.abs()
    for w in range(9):
        k, grp = w // 3 + 1, w % 3
        p = derivative_at(torch, coeffs, t, k)[:, w, :]
        dims = list(GROUPS[grp])
        m2 = (p[:, dims] ** 2).sum(dim=1)
        pos = m2 > 0   # (a zero magnitude gets a zero gradient, as the kernel gives it)
        out.append(torch.where(pos, torch.sqrt(torch.where(pos, m2, torch.ones_like(m2))), torch.zeros_like(m2)))
    return torch.stack(out, dim=1).reshape(-1, 3, 3)


def violation_scaling_np(maxima, limits):
    """numpy restatement of violation_scaling (mrs_tg_device.hpp) per segment: maxima [S][9], limits [S][9]"""
    viol = [np.maximum(np.maximum(maxima[:, 3 * k] / limits[:, 3 * k], maxima[:, 3 * k + 1] / limits[:, 3 * k + 1]),
                       maxima[:, 3 * k + 2] / limits[:, 3 * k + 2]) for k in range(3)]
    return np.maximum(1.0, np.maximum(np.maximum(viol[0], np.sqrt(viol[1])), np.cbrt(viol[2])))
