"""Instruction mix of one kernel's loops, from the gfx950 assembly the build's flags give.  Runs without a GPU.

    python scripts/isa_count.py mrs_uav_trajectory_generation_amd/csrc/mrs_tg_quad.hip 'solve_duo_group_kernel<true, true>'
    python scripts/isa_count.py FILE.hip KERNEL [KERNEL ...] [--min-loop N] [-DX=1 ...]

KERNEL is matched against the demangled name without its argument list (`mrs_tg::` may be left out; defaulted template
arguments are spelled: the general grouped two-sided kernel is 'solve_duo_group_kernel<true, false>'); every match is printed.
For each: VGPRs, SGPRs, scratch (private_segment_fixed_size) and LDS as the kernel descriptor states them, the size of the
whole body, and one line per LOOP -- a label with a later branch back to it -- with its instructions split into FP64 arithmetic
(v_*_f64 except compares and moves), other VALU, scalar, LDS, vector memory (global / flat / buffer / scratch) and waits
(s_waitcnt, s_nop, s_sleep).  Loops shorter than --min-loop instructions (default 40) are left out; `in` names the enclosing
loop.  A wavefront of the two-sided solve issues one instruction after the other, so these counts times
the trip counts are its clocks."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ("fp64", "valu", "scalar", "lds", "vmem", "wait")


def kind_of(op):
    if op in ("s_waitcnt", "s_nop", "s_sleep") or op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        if "_f64" in op and not op.startswith(("v_cmp", "v_cmpx", "v_cndmask", "v_mov")):
            return "fp64"
        return "valu"
    return "scalar"


def assembly(src, defines):
    from mrs_uav_trajectory_generation_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call([b._hipcc()] + b.FLAGS + list(defines) + ["-S", "--cuda-device-only", src, "-o", out])
        with open(out) as f:
            return f.read().splitlines()


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, r))


def functions(lines):
    """mangled name -> (first line, last line) of its body, and -> its descriptor fields"""
    body, desc, cur, cur_desc = {}, {}, None, None
    for n, line in enumerate(lines):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L") and cur is None:
            cur = (m.group(1), n)
        m = re.match(r"^\s*\.size\s+(\w+),", line)
        if m and cur and m.group(1) == cur[0]:
            body[cur[0]] = (cur[1], n)
            cur = None
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\w+)", line)
        if m:
            cur_desc = desc.setdefault(m.group(1), {})
        elif re.match(r"^\s*\.end_amdhsa_kernel", line):
            cur_desc = None
        elif cur_desc is not None:
            m = re.match(r"^\s*\.amdhsa_(\w+)\s+(\S+)", line)
            if m:
                cur_desc[m.group(1)] = m.group(2)
    return body, desc


def instructions(lines, a, b):
    """[(line number, opcode or None, label or None, branch target or None)]"""
    out = []
    for n in range(a, b):
        s = lines[n].split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\w+):", s)
            if m:
                out.append((n, None, m.group(1), None))
            continue
        op = s.split()[0]
        if op.endswith(":"):
            continue
        m = re.search(r"(\.LBB\w+)\s*$", s) if op.startswith(("s_cbranch", "s_branch")) else None
        out.append((n, op, None, m.group(1) if m else None))
    return out


def mix(ins):
    c = dict.fromkeys(KINDS, 0)
    for _, op, _, _ in ins:
        if op:
            c[kind_of(op)] += 1
    return c


def report(lines, name, pretty, span, d, min_loop):
    ins = instructions(lines, *span)
    total = mix(ins)
    print("%s" % pretty)
    print("  VGPRs %s  SGPRs %s  accum_offset %s  scratch (private_segment_fixed_size) %s  static LDS %s" % (
        d.get("next_free_vgpr", "?"), d.get("next_free_sgpr", "?"), d.get("accum_offset", "-"),
        d.get("private_segment_fixed_size", "?"), d.get("group_segment_fixed_size", "?")))
    fmt = "  %-34s %6s %6s %6s %7s %5s %5s %5s"
    print(fmt % ("", "all", "fp64", "valu", "scalar", "lds", "vmem", "wait"))
    print(fmt % (("whole body",) + (sum(total.values()),) + tuple(total[k] for k in KINDS)))
    where = {lab: k for k, (_, _, lab, _) in enumerate(ins) if lab}
    loops = []
    for lab, k0 in where.items():
        back = [k for k, (_, op, _, tgt) in enumerate(ins) if tgt == lab and k > k0]
        if back:
            loops.append((k0, back[-1], lab))
    loops.sort()
    for k0, k1, lab in loops:
        c = mix(ins[k0:k1 + 1])
        n_all = sum(c.values())
        if n_all < min_loop:
            continue
        outer = [l for a, b, l in loops if a < k0 and b > k1]
        hint = ""
        for k in range(k0, min(k0 + 2, len(ins))):
            m = re.search(r";\s*=>(.*)$", lines[ins[k][0]])
            if m:
                hint = m.group(1).strip()
        tag = "loop %s%s" % (lab, " in " + outer[-1] if outer else "")
        print(fmt % ((tag,) + (n_all,) + tuple(c[k] for k in KINDS)) + ("   ; " + hint if hint else ""))
    print()


def main(argv):
    defines = [a for a in argv if a.startswith("-D")]
    min_loop = 40
    if "--min-loop" in argv:
        i = argv.index("--min-loop")
        min_loop = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    args = [a for a in argv if not a.startswith("-D")]
    if len(args) < 2:
        sys.exit(__doc__)
    src, wanted = args[0], args[1:]
    lines = assembly(src, defines)
    body, desc = functions(lines)
    pretty = demangle(list(desc))
    print("# %s, gfx950, flags: %s" % (os.path.relpath(os.path.abspath(src), ROOT), " ".join(defines) or "the build's"))
    hit = False
    for name in sorted(desc, key=lambda n: pretty[n]):
        short = re.sub(r"\(.*", "", pretty[name]).replace("void ", "").replace("mrs_tg::", "")
        if short in wanted and name in body:
            report(lines, name, short, body[name], desc[name], min_loop)
            hit = True
    if not hit:
        sys.exit("no kernel named %s in %s" % (wanted, src))


if __name__ == "__main__":
    main(sys.argv[1:])
