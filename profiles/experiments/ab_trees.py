#!/usr/bin/env python
"""A/B of two checkouts of this repository (each built: libheyoka_amd.so next to its package) on one GPU, the way
profiles/ab_v5_lane_sums.log was taken:

  ab_trees.py bench PARENT NEW OUT [--runs 5]   bench.py --gpus 1 --steps 20 --warmup 5, the two trees in alternation, parent
                                                first; mean, sample standard deviation, the bar of 10 parent standard deviations
  ab_trees.py trace PARENT NEW OUT              one rocprofv3 --kernel-trace --stats run per tree (4 timed launches)
  ab_trees.py pmc PARENT NEW OUT                rocprofv3 --pmc, two passes of their own per tree, no tracing domains: SQ_INSTS_VALU,
                                                SQ_INSTS_LDS, SQ_ACTIVE_INST_VALU, SQ_WAIT_ANY, SQ_WAVE_CYCLES of the last hy_taylor dispatch

Every child runs under a time limit of its own and the first one which fails ends the script: nothing more is started on the
GPU behind a fault. The text goes to OUT (appended) and to the terminal."""
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import summarize_rocprof  # noqa: E402

BENCH = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
PROFILED = ["--workload", "outer_ss", "--no-cpu-baseline", "--no-extra-workloads", "--steps", "4", "--warmup", "1"]
PASSES = (("SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_WAVE_CYCLES"), ("SQ_ACTIVE_INST_VALU", "SQ_WAIT_ANY", "SQ_WAVE_CYCLES"))


class Log:
    def __init__(self, path):
        self.f = open(path, "a")

    def __call__(self, text=""):
        print(text, flush=True)
        self.f.write(text + "\n")
        self.f.flush()


def child(cmd, tree, limit):
    """The command in the tree, under its time limit; its standard output. Anything but a clean exit ends the script."""
    env = {k: v for k, v in os.environ.items() if k not in ("HEYOKA_AMD_V5_OPTS", "PYTHONPATH")}
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=tree, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("ab_trees: %s in %s ended with status %d; stopping here.\n%s" % (" ".join(cmd), tree, r.returncode, r.stderr[-3000:]))
    return r.stdout


def bench_line(out):
    lines = [ln for ln in out.split("\n") if ln.startswith("{")]
    return lines[-1], json.loads(lines[-1])


def bench(trees, log, runs):
    log("# bench.py %s, parent and new in alternation (parent first), one session (the lines as printed, cut to 400 characters)" % " ".join(BENCH))
    vals = {"parent": [], "new": []}
    for _ in range(runs):
        for tag in ("parent", "new"):
            line, b = bench_line(child([sys.executable, "bench.py"] + BENCH, trees[tag], 400))
            vals[tag].append(float(b["value"]))
            log("%s %s" % (tag, line[:400]))
    log()
    mean = {t: statistics.mean(v) for t, v in vals.items()}
    sd = {t: statistics.stdev(v) for t, v in vals.items()}
    for t in ("parent", "new"):
        log("%-7s n = %d, mean = %.6e, sample standard deviation = %.3e (%.3f %%)" % (t + ":", len(vals[t]), mean[t], sd[t], 100.0 * sd[t] / mean[t]))
    d = mean["new"] - mean["parent"]
    log("new mean - parent mean = %.3e = %.1f parent standard deviations (asked: more than 10); ratio new / parent = %.4f"
        % (d, d / sd["parent"], mean["new"] / mean["parent"]))
    lo, hi = min(vals["new"]), max(vals["parent"])
    log("smallest new value %.6e %s largest parent value %.6e" % (lo, ">" if lo > hi else "<=", hi))
    log("bar met: %s" % ("yes" if d > 10.0 * sd["parent"] and lo > hi else "NO"))


def profiled(tree, args, limit=400):
    """bench.py under rocprofv3 in a scratch directory; the path of the rocpd database."""
    d = tempfile.mkdtemp(prefix="ab_trees_")
    child(["rocprofv3"] + args + ["-d", d, "-o", "p", "--", sys.executable, os.path.join(tree, "bench.py")] + PROFILED, tree, limit)
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if not dbs:
        sys.exit("ab_trees: rocprofv3 left no database in " + d)
    return d, dbs[0]


def trace(trees, log):
    log("# rocprofv3 --kernel-trace --stats of bench.py %s, one run each" % " ".join(PROFILED))
    avg = {}
    for tag in ("parent", "new"):
        d, db = profiled(trees[tag], ["--kernel-trace", "--stats"])
        txt, _ = summarize_rocprof.kernel_stats(db)
        for ln in txt.split("\n"):
            if ln.startswith("hy_taylor") or ln.startswith("kernel "):
                log("%s: %s" % (tag, ln))
            if "timed launches" in ln:
                avg[tag] = float(ln.split("avg_ns = ")[1])
        shutil.rmtree(d, ignore_errors=True)
    log("timed launches: kernel time new / parent = %.4f, i.e. rate x %.4f" % (avg["new"] / avg["parent"], avg["parent"] / avg["new"]))


def pmc(trees, log):
    log("# rocprofv3 --pmc (two passes of their own per tree, no tracing domains), last hy_taylor dispatch of bench.py %s" % " ".join(PROFILED))
    got = {}
    for tag in ("parent", "new"):
        got[tag] = {}
        for names in PASSES:
            d, db = profiled(trees[tag], ["--pmc"] + list(names))
            rows = summarize_rocprof.counters(db)
            last = max(r[0] for r in rows)
            for r in rows:
                if r[0] == last:
                    got[tag][r[1]] = float(r[2])
                    got[tag]["kernel_ms"] = r[10] / 1e6
            shutil.rmtree(d, ignore_errors=True)
        log("%s: kernel %.2f ms" % (tag, got[tag]["kernel_ms"]))
        for k in sorted(got[tag]):
            if k != "kernel_ms":
                log("  %-24s %16.0f  %.3f of SQ_WAVE_CYCLES" % (k, got[tag][k], got[tag][k] / got[tag]["SQ_WAVE_CYCLES"]))
    log()
    for k in sorted(got["new"]):
        if k != "kernel_ms":
            log("%-22s new / parent = %.4f" % (k, got["new"][k] / got["parent"][k]))


def main():
    if len(sys.argv) < 5 or sys.argv[1] not in ("bench", "trace", "pmc"):
        sys.exit(__doc__)
    trees = {"parent": os.path.abspath(sys.argv[2]), "new": os.path.abspath(sys.argv[3])}
    log = Log(sys.argv[4])
    if sys.argv[1] == "bench":
        bench(trees, log, int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 5)
    elif sys.argv[1] == "trace":
        trace(trees, log)
    else:
        pmc(trees, log)


if __name__ == "__main__":
    main()
