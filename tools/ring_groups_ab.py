"""Alternating A/B of the Target step for the ring producer's group launches (profiles/ring_groups.md).

Three builds take turns in one session: the parent commit's library (built from a checkout of the parent with
`make -C ndarray-interp_amd/csrc LIB=../libndinterp_hip_parent.so` and copied beside this tree's library), this tree's
library with full-width groups from the first chunk on (NDI_RING_GROUP=1) and with a narrow first launch (=2); one run
with the knob off (=0) follows.  Every run is one plain `python bench.py` process (default steps and warm-up).  Then, each
in a run of its own: rocprofv3 per-kernel stats and FETCH_SIZE of `bench.py --steps 5 --warmup 2` (the legs behind the
timed region switched off) for the parent and for the faster order, and `--dump-outputs` of both, compared byte for byte.
Writes ring_groups_ab.jsonl, ring_groups_kernel_stats_{before,after}.csv, ring_groups_pmc.txt and ring_groups_dump.txt
into --out.

    python tools/ring_groups_ab.py --out profiles [--parent-lib libndinterp_hip_parent.so] [--pairs 6]
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIM = ["--no-secondary", "--no-pmc", "--no-gather-leg", "--no-cpu-baseline", "--no-check", "--placement-probe", "0"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--parent-lib", default="libndinterp_hip_parent.so",
                    help="the parent commit's library, a file name beside the package's own library (NDI_LIB)")
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--budget-s", type=float, default=600.0, help="no further alternating round is started after this")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    builds = {"parent": {"NDI_LIB": args.parent_lib}, "groups_full": {"NDI_RING_GROUP": "1"},
              "groups_narrow_first": {"NDI_RING_GROUP": "2"}, "groups_off": {"NDI_RING_GROUP": "0"}}
    results = []
    t_start = time.time()

    def bench(build, flags, series):
        t0 = time.time()
        r = subprocess.run([sys.executable, "bench.py"] + flags, cwd=ROOT, env=dict(os.environ, **builds[build]),
                           capture_output=True, text=True, timeout=400)
        if r.returncode != 0:     # nothing more is started on the device after a failing run
            sys.exit(f"{build}: bench.py exited with {r.returncode}\n{r.stderr[-3000:]}")
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        rec = {"build": build, "flags": " ".join(flags) or "(plain)", "series": series, "ms_per_step": line["ms_per_step"],
               "ms_per_step_median": line["ms_per_step_median"], "wall_s": round(time.time() - t0, 1)}
        results.append(rec)
        with open(os.path.join(args.out, "ring_groups_ab.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    for i in range(args.pairs):
        if time.time() - t_start > args.budget_s:
            break
        for b in ("parent", "groups_full", "groups_narrow_first"):
            bench(b, [], f"alternating-{i}")
    bench("groups_off", [], "knob-off")

    def median(b):
        v = sorted(r["ms_per_step"] for r in results if r["build"] == b)
        return v[len(v) // 2]
    best = min(("groups_full", "groups_narrow_first"), key=median)
    print("faster order:", best, flush=True)

    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    short = ["--steps", "5", "--warmup", "2"] + TRIM

    def profiled(build, extra):
        d = tempfile.mkdtemp(prefix="ndi_ring_groups_")
        r = subprocess.run([prof] + extra + ["--output-format", "csv", "-d", d, "--", sys.executable,
                                             os.path.join(ROOT, "bench.py")] + short,
                           cwd=d, env=dict(os.environ, TMPDIR=d, **builds[build]), capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            sys.exit(f"{build}: rocprofv3 {' '.join(extra)} exited with {r.returncode}\n{r.stderr[-2000:]}")
        return d

    pmc = []
    for build, name in (("parent", "before"), (best, "after")):
        d = profiled(build, ["--kernel-trace", "--stats"])
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if files:
            shutil.copy(files[0], os.path.join(args.out, f"ring_groups_kernel_stats_{name}.csv"))
        shutil.rmtree(d, ignore_errors=True)
        d = profiled(build, ["--kernel-trace", "--pmc", "FETCH_SIZE"])     # counters in a run of their own
        vals = {}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if row["Counter_Name"] == "FETCH_SIZE" and "eval_bucketed" in row["Kernel_Name"]:
                    vals.setdefault(row["Kernel_Name"][:60], []).append(float(row["Counter_Value"]))
        shutil.rmtree(d, ignore_errors=True)
        for k, v in vals.items():
            pmc.append(f"{name} ({build}) {k}: launches={len(v)} FETCH_SIZE mean={sum(v) / len(v):.1f} KiB "
                       f"sum={sum(v):.1f} KiB (7 steps of 1e7 queries)")
    open(os.path.join(args.out, "ring_groups_pmc.txt"), "w").write("\n".join(pmc) + "\n")
    print("\n".join(pmc), flush=True)

    sums = {}
    for build in ("parent", best):
        d = tempfile.mkdtemp(prefix="ndi_ring_groups_dump_")
        r = subprocess.run([sys.executable, "bench.py", "--dump-outputs", d], cwd=ROOT, env=dict(os.environ, **builds[build]),
                           capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            sys.exit(f"{build}: bench.py --dump-outputs exited with {r.returncode}\n{r.stderr[-2000:]}")
        sums[build] = hashlib.sha256(open(os.path.join(d, "rows.npy"), "rb").read()).hexdigest()
        shutil.rmtree(d, ignore_errors=True)
    same = len(set(sums.values())) == 1
    open(os.path.join(args.out, "ring_groups_dump.txt"), "w").write(json.dumps({"sha256": sums, "identical": same}) + "\n")
    print("rows.npy identical:", same, flush=True)


if __name__ == "__main__":
    main()
