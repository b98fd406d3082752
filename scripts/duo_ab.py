"""A / B of library builds (and environment knobs) on the headline: alternating runs of bench.py on one box in one session, each a
fresh process, in the form of profiles/duo_store_through_ab.txt and profiles/duo_lean_ab.txt.

    python scripts/duo_ab.py [--runs 6] [--timeout 120] parent=PATH/libmrs_tg_parent.so new=PATH/libmrs_tg.so \\
        lean0=PATH/libmrs_tg.so,MRS_TG_DUO_LEAN=0 -- --gpus 1 --steps 20 --warmup 5

A variant is NAME=LIBRARY[,ENV=VALUE ...]; what follows `--` goes to bench.py.  Prints every run's median region and its nine
regions in microseconds, then each variant's range of run medians, the first variant's min-max spread (the noise a gain has to
be told from) and, for every other variant, whether each of its runs lies below every run of the first and whether the
difference of the medians is at least twice that spread.  Stops at the first run that fails."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    cut = argv.index("--") if "--" in argv else len(argv)
    mine, bench_args = argv[:cut], argv[cut + 1:] or ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs, timeout, variants = 6, 120, []
    k = 0
    while k < len(mine):
        if mine[k] == "--runs":
            runs, k = int(mine[k + 1]), k + 2
        elif mine[k] == "--timeout":
            timeout, k = int(mine[k + 1]), k + 2
        else:
            name, spec = mine[k].split("=", 1)
            lib, *envs = spec.split(",")
            variants.append((name, os.path.abspath(lib), dict(e.split("=", 1) for e in envs)))
            k += 1
    if len(variants) < 2:
        sys.exit(__doc__)
    steps = int(bench_args[bench_args.index("--steps") + 1]) if "--steps" in bench_args else 200
    print("== python bench.py %s   (%d runs each, alternating)" % (" ".join(bench_args), runs), flush=True)
    medians = {name: [] for name, _, _ in variants}
    width = max(len(name) for name in medians)
    for r in range(runs):
        for name, lib, envs in variants:
            env = dict(os.environ, MRS_TG_LIB_PATH=lib, **envs)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bench_args, env=env, cwd=ROOT, capture_output=True,
                               text=True, timeout=timeout)
            if p.returncode != 0:
                sys.exit("%s run %d: bench.py ended with %d\n%s" % (name, r + 1, p.returncode, p.stderr[-2000:]))
            line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            regions = [ms * steps * 1e3 for ms in line["ms_per_step_regions"]]
            med = line["ms_per_step_median"] * steps * 1e3
            medians[name].append(med)
            print("%-*s run %d  median %7.2f us   value %6.1f M/s   regions %s" % (width, name, r + 1, med, line["value"] / 1e6,
                                                                                 " ".join("%.1f" % u for u in regions)), flush=True)
    print("run medians: " + ", ".join("%s %.2f .. %.2f us" % (n, min(m), max(m)) for n, m in medians.items()))
    base_name = variants[0][0]
    base = medians[base_name]
    spread = max(base) - min(base)
    print("-- %s: median of the run medians %.2f us, min-max spread %.2f us" % (base_name, statistics.median(base), spread))
    for name, m in medians.items():
        if name == base_name:
            continue
        diff = statistics.median(base) - statistics.median(m)
        print("-- %s: median %.2f us, %.2f us below %s (%.1f x its spread); every run below every %s run: %s; at least twice the spread: %s"
              % (name, statistics.median(m), diff, base_name, diff / spread if spread > 0 else float("inf"), base_name,
                 "yes" if max(m) < min(base) else "NO", "yes" if diff >= 2 * spread else "NO"))


if __name__ == "__main__":
    main(sys.argv[1:])
