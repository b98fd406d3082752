"""The lean instantiation of the grouped two-sided solve, from its gfx950 assembly (no GPU needed; skipped without hipcc):
no scratch, within the register file of two wavefronts per SIMD, and a backward loop shorter than the general instantiation's --
the point of the instantiation.  Counts instruction classes with scripts/isa_count.py, as
profiles/duo_isa_counts.txt does."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mrs_uav_trajectory_generation_amd", "csrc", "mrs_tg_quad.hip")
LEAN, GENERAL = "solve_duo_group_kernel<true, true>", "solve_duo_group_kernel<true, false>"


def _have_hipcc():
    return os.path.exists("/opt/rocm/bin/hipcc") or shutil.which(os.environ.get("HIPCC", "hipcc")) is not None


def _parse(text):
    """kernel -> dict(vgprs, scratch, loops: label -> dict(depth1, all, fp64, valu, scalar, lds, vmem, wait))"""
    kernels, cur = {}, None
    for line in text.splitlines():
        if line.startswith("solve_"):
            cur = kernels.setdefault(line.strip(), dict(loops={}))
        m = re.match(r"\s+VGPRs (\d+) .*private_segment_fixed_size\) (\d+)", line)
        if m and cur is not None:
            cur["vgprs"], cur["scratch"] = int(m.group(1)), int(m.group(2))
        m = re.match(r"\s+loop (\S+)(?: in (\S+))?\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line)
        if m and cur is not None:
            n = [int(v) for v in m.groups()[2:]]
            cur["loops"][m.group(1)] = dict(zip(("all", "fp64", "valu", "scalar", "lds", "vmem", "wait"), n),
                                            depth1="Inner Loop Header: Depth=1" in line)
    return kernels


def _backward_loop(kernel):
    """The loop, among those the compiler marks as a source loop of depth 1, with FP64 arithmetic, LDS traffic AND vector-memory
    stores: the forward loops store nothing to memory, the general step's loops do not touch LDS."""
    cand = [c for c in kernel["loops"].values() if c["depth1"] and c["fp64"] > 0 and c["lds"] > 0 and c["vmem"] > 0]
    assert len(cand) == 1, kernel["loops"]
    return cand[0]


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed")
def test_lean_instantiation_has_no_scratch_fits_two_per_simd_and_a_shorter_backward_loop():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_count.py"), SRC, LEAN, GENERAL, "--min-loop", "100"],
                         check=True, capture_output=True, text=True, cwd=ROOT).stdout
    kernels = _parse(out)
    assert set(kernels) == {LEAN, GENERAL}, out
    lean, general = kernels[LEAN], kernels[GENERAL]
    print(out)
    assert lean["scratch"] == 0 and general["scratch"] == 0
    assert lean["vgprs"] <= 256
    b_lean, b_general = _backward_loop(lean), _backward_loop(general)
    print("backward loop: lean %s, general %s" % (b_lean, b_general))
    assert b_lean["fp64"] == b_general["fp64"], "the same arithmetic"
    assert b_lean["all"] < b_general["all"]
