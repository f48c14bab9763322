#!/usr/bin/env python3
"""Measures -bamout ... -sort (urmap_amd/csrc/bam_sort.hip) on one GPU and prints one JSON object:

  unsorted   `urmap -map reads.fq -bamout F`, start of the process to its exit, --rounds runs after a warm-up run (--other-cli PATH: by
             another build's command line, the parent commit's)
  sorted     `urmap -map reads.fq -bamout F -sort` of this build, likewise; with it the command's own sort_s (last record mapped to last
             byte of F and F.bai written) and its parts as the library reports them under URMAPX_VERBOSE: the walk along the block_size
             chain, device allocations, records to the device, key and sort launches, gather launches, deflate, members back to the host, index, write
  derived    the sort launches' milliseconds per 1 M records; the gather's bytes per second (it reads and writes every byte once) against
             the rate of a device-to-device copy of 1 GiB measured in this process; what the sorted run costs over the unsorted one against
             the time the medium takes to write the file once more (a plain write of the file's bytes to --out-dir, timed here)

The reads are those of scripts/bgzf_bench.py (same generator, same seed).

    python scripts/bam_sort_bench.py [--reads 10000000] [--genome-mbp 20] [--rounds 3] [--out-dir DIR] [--other-cli PATH] [--out DIR]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bgzf_bench import CLI, medium_of, write_fastq  # noqa: E402
from urmap_amd import synth  # noqa: E402

PARTS = ("total", "scan", "alloc", "upload", "sort", "gather", "deflate", "copy", "index", "write")


def run(cli, fq, ufi, out, extra):
    t0 = time.time()
    r = subprocess.run([cli, "-map", fq, "-ufi", ufi, "-bamout", out] + extra, capture_output=True, text=True, timeout=1800,
                       env=dict(os.environ, URMAPX_VERBOSE="1"))
    wall = time.time() - t0
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    res = {"process_wall_s": wall, "file_bytes": os.path.getsize(out)}
    m = re.search(r"([0-9.]+)\s+Seconds in mapper", r.stderr)
    res["mapper_s"] = float(m.group(1)) if m else None
    m = re.search(r"bam_sort seconds: (.*?); records (\d+) bytes (\d+) passes (\d+) slices (\d+)", r.stderr)
    if m:
        words = m.group(1).split()
        res["parts_s"] = {words[i]: float(words[i + 1]) for i in range(0, len(words), 2)}
        res.update(records=int(m.group(2)), record_bytes=int(m.group(3)), passes=int(m.group(4)), slices=int(m.group(5)))
    return res


def copy_rate():
    """bytes per second of a device-to-device copy of 1 GiB (read once, written once), median of five after a warm-up"""
    import torch
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    times = []
    for k in range(6):
        torch.cuda.synchronize()
        t0 = time.time()
        b.copy_(a)
        torch.cuda.synchronize()
        times.append(time.time() - t0)
    return (1 << 30) / float(np.median(times[1:]))


def write_once(path, nbytes):
    """seconds the medium takes for a plain write of nbytes (what `the file once more` costs)"""
    buf = os.urandom(1 << 24)
    t0 = time.time()
    with open(path, "wb") as f:
        left = nbytes
        while left > 0:
            f.write(buf[:min(left, len(buf))])
            left -= len(buf)
    s = time.time() - t0
    os.remove(path)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-mbp", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out-dir", default=None, help="where the output files go (the medium that is measured)")
    ap.add_argument("--other-cli", default=None)
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
        res["unsorted_cli"] = args.other_cli or CLI
        runs = {"unsorted": [], "sorted": []}
        for k in range(args.rounds + 1):  # (the variants take turns; round 0 is the warm-up and is left out)
            runs["unsorted"].append(run(args.other_cli or CLI, fq, ufi, os.path.join(d, "u.bam"), []))
            runs["sorted"].append(run(CLI, fq, ufi, os.path.join(d, "s.bam"), ["-sort"]))
            print(f"round {k}: unsorted {runs['unsorted'][-1]['process_wall_s']:.2f} s, sorted {runs['sorted'][-1]['process_wall_s']:.2f} s", file=sys.stderr, flush=True)
        for name, rs in runs.items():
            kept = rs[1:]
            res[name] = {"process_wall_s_runs": [r["process_wall_s"] for r in kept], "median_process_wall_s": float(np.median([r["process_wall_s"] for r in kept])),
                         "median_mapper_s": float(np.median([r["mapper_s"] for r in kept])), "file_bytes": kept[-1]["file_bytes"]}
        kept = runs["sorted"][1:]
        parts = {p: float(np.median([r["parts_s"][p] for r in kept])) for p in PARTS}
        last = kept[-1]
        res["sorted"].update(parts_s=parts, records=last["records"], record_bytes=last["record_bytes"], passes=last["passes"], slices=last["slices"],
                             bai_bytes=os.path.getsize(os.path.join(d, "s.bam.bai")))
        rate = copy_rate()
        write_s = write_once(os.path.join(d, "w.bin"), res["sorted"]["file_bytes"])
        extra = res["sorted"]["median_process_wall_s"] - res["unsorted"]["median_process_wall_s"]
        res["derived"] = {"sort_ms_per_1M_records": 1e3 * parts["sort"] / (last["records"] / 1e6),
                          "gather_bytes_per_s": last["record_bytes"] / parts["gather"], "device_copy_bytes_per_s": rate,
                          "gather_over_copy": last["record_bytes"] / parts["gather"] / rate,
                          "sorted_minus_unsorted_s": extra, "write_file_once_s": write_s, "over_the_expectation_s": extra - write_s}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bam_sort_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
