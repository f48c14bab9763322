#!/usr/bin/env python3
"""Measures the external road of -bamout ... -sort (urmapx_bam_sort_external, place_kernel in urmap_amd/csrc/bam_sort.hip) against the
in-core road on one GPU and prints one JSON object.  The reads are those of scripts/bam_sort_bench.py (same generator, same seed).

  in_core    `urmap -map reads.fq -bamout F -sort`: the parts of sort_s from the URMAPX_VERBOSE line, upload_s among them
  p2, p4     the same with -sortmem N, N being the smallest budget for which urmapx_bam_sort_plan_for answers 2 and 4 partitions:
             the same parts, and from the second verbose line the partitions, the staged chunks and stage_s -- the 1 + P passes over
             the input.  stage_s / (1 + P) is held against the in-core run's upload_s for the same bytes in the same session
  stages     --stage-sweep: p2 again with staged chunks of 4, 16 and 64 MiB (URMAPX_TEST_SORT_STAGE)

--rounds runs of each after a warm-up round, the variants taking turns; medians.

    python scripts/bam_sort_external_bench.py [--reads 10000000] [--genome-mbp 20] [--rounds 3] [--stage-sweep] [--out-dir DIR] [--out DIR]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bam_sort_bench import PARTS, run  # noqa: E402
from bgzf_bench import CLI, medium_of, write_fastq  # noqa: E402
from urmap_amd import api, synth  # noqa: E402


def run_external(fq, ufi, out, extra, env):
    """bam_sort_bench.run with the second verbose line read too"""
    r = subprocess.run([CLI, "-map", fq, "-ufi", ufi, "-bamout", out, "-sort"] + extra, capture_output=True, text=True, timeout=1800,
                       env=dict(os.environ, URMAPX_VERBOSE="1", **env))
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    m = re.search(r"bam_sort seconds: (.*?); records (\d+) bytes (\d+) passes (\d+) slices (\d+)", r.stderr)
    words = m.group(1).split()
    res = {"parts_s": {words[i]: float(words[i + 1]) for i in range(0, len(words), 2)}, "records": int(m.group(2)), "record_bytes": int(m.group(3))}
    m = re.search(r"bam_sort external: partitions (\d+) chunks (\d+) passes (\d+) stage ([0-9.]+)", r.stderr)
    if m:
        res.update(partitions=int(m.group(1)), chunks=int(m.group(2)), input_passes=int(m.group(3)), stage_s=float(m.group(4)))
    return res


def budget_for(n_bytes, n_records, partitions):
    """the smallest budget whose plan has at most `partitions` partitions (the count never rises with the budget)"""
    try:
        api.bam_sort_plan(n_bytes, n_records, 1)
        raise RuntimeError("a budget of one byte fits")
    except api.UrmapxError as e:
        lo = e.plan["device_bytes"]
    hi = api.bam_sort_plan(n_bytes, n_records, 1 << 62)["device_bytes"] - 1  # (one byte less than in core takes)
    if api.bam_sort_plan(n_bytes, n_records, lo)["partitions"] <= partitions:
        return lo
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if api.bam_sort_plan(n_bytes, n_records, mid)["partitions"] <= partitions:
            hi = mid
        else:
            lo = mid
    return hi


def summary(rs):
    kept = rs[1:]
    out = {"parts_s": {p: float(np.median([r["parts_s"][p] for r in kept])) for p in PARTS}}
    if "stage_s" in kept[-1]:
        passes = kept[-1]["input_passes"]
        stage = float(np.median([r["stage_s"] for r in kept]))
        out.update(partitions=kept[-1]["partitions"], chunks=kept[-1]["chunks"], input_passes=passes, stage_s=stage, stage_s_runs=[r["stage_s"] for r in kept],
                   stage_s_per_pass=stage / passes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-mbp", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stage-sweep", action="store_true")
    ap.add_argument("--out-dir", default=None, help="where the output files go")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    res = {"reads": args.reads, "rounds": args.rounds}
    with tempfile.TemporaryDirectory(dir=args.out_dir) as d:
        g = synth.make_genome(5, [int(args.genome_mbp * 1e6)], repeat_frac=0.05, n_families=8)
        fa, ufi, fq = os.path.join(d, "g.fa"), os.path.join(d, "g.ufi"), os.path.join(d, "r.fq")
        synth.write_fasta(fa, g)
        subprocess.run([CLI, "-make_ufi", fa, "-output", ufi, "-quiet"], check=True, capture_output=True, timeout=1800)
        write_fastq(fq, rng, g[0][1], args.reads, 150)
        res["medium"] = medium_of(d)
        first = run(CLI, fq, ufi, os.path.join(d, "s.bam"), ["-sort"])  # (the sizes the budgets are planned from; also warms the page cache)
        n_bytes, n_records = first["record_bytes"], first["records"]
        res.update(record_bytes=n_bytes, records=n_records)
        variants = {"in_core": ([], {})}
        for p in (2, 4):
            b = budget_for(n_bytes, n_records, p)
            variants["p%d" % p] = (["-sortmem", str(b)], {})
            res["p%d_budget" % p] = b
        if args.stage_sweep:
            for mib in (4, 16, 64):
                variants["p2_stage_%dMiB" % mib] = (variants["p2"][0], {"URMAPX_TEST_SORT_STAGE": str(mib << 20)})
        runs = {k: [] for k in variants}
        for k in range(args.rounds + 1):  # (the variants take turns; round 0 is the warm-up and is left out)
            for name, (extra, env) in variants.items():
                runs[name].append(run_external(fq, ufi, os.path.join(d, "s.bam"), extra, env))
            print(f"round {k} done", file=sys.stderr, flush=True)
        for name, rs in runs.items():
            res[name] = summary(rs)
        upload = res["in_core"]["parts_s"]["upload"]
        res["derived"] = {"in_core_upload_s": upload, "upload_bytes_per_s": n_bytes / upload,
                          **{name + "_stage_per_pass_over_upload": res[name]["stage_s_per_pass"] / upload for name in runs if "stage_s_per_pass" in res[name]}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bam_sort_external_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
