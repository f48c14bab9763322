#!/usr/bin/env python3
"""Measures -bgzf (urmap_amd/csrc/bgzf_gpu.hip) on one GPU and prints one JSON object:

  kernel   the compress launches alone (HIP events around urmapx_bgzf_compress_device) over up to --kernel-mb of the SAM text the
           file-to-file run wrote: ms per GB of text and the ratio compressed / text; median of --steps runs after a warm-up
  file     `urmap -map reads.fq -samout F` file to file with and without -bgzf: reads/s as the command reports them (first read parsed
           to last byte written, index load excluded), the median of --rounds runs without the first (it also pages the FASTQ in), the medium F is on
           (--out-dir, default a temporary directory: state it with the number).  --other-cli PATH times the plain run of another
           build's command line on the same files (the parent commit's, for the flag-off comparison)

Reads: --reads of 150 bases drawn from a synthetic genome of --genome-mbp (urmap_amd.synth) with 1 % substitutions, a tenth random;
qualities in Illumina's four bins, so that the text is not as compressible as the golden fixtures' constant strings.

    python scripts/bgzf_bench.py [--reads 10000000] [--genome-mbp 20] [--steps 5] [--rounds 5] [--out-dir DIR] [--other-cli PATH] [--out DIR]
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
from urmap_amd import api, synth  # noqa: E402

CLI = os.path.join(ROOT, "urmap_amd", "urmap")
ACGT = np.frombuffer(b"ACGT", np.uint8)
QBINS = np.frombuffer(b"F:,#", np.uint8)


def write_fastq(path, rng, genome, n, L):
    with open(path, "wb") as f:
        for lo in range(0, n, 200000):
            k = min(200000, n - lo)
            starts = rng.integers(0, len(genome) - L, size=k)
            reads = genome[starts[:, None] + np.arange(L)[None, :]]
            sub = rng.random((k, L)) < 0.01
            reads[sub] = ACGT[rng.integers(0, 4, size=int(sub.sum()))]
            rnd = rng.random(k) < 0.1
            reads[rnd] = ACGT[rng.integers(0, 4, size=(int(rnd.sum()), L))]
            quals = QBINS[rng.choice(4, size=(k, L), p=[0.85, 0.10, 0.04, 0.01])]
            f.write(b"".join(b"@read%d\n%s\n+\n%s\n" % (lo + i, reads[i].tobytes(), quals[i].tobytes()) for i in range(k)))


def medium_of(path):
    try:
        with open("/proc/mounts") as f:
            best = ("", "unknown")
            for line in f:
                _, mnt, fstype = line.split()[:3]
                if os.path.abspath(path).startswith(mnt) and len(mnt) > len(best[0]):
                    best = (mnt, fstype)
        return best[1]
    except OSError:
        return "unknown"


def run_cli(cli, fq, ufi, out, extra):
    """one run -> reads/s as the command prints it, wall seconds of the process, bytes written"""
    t0 = time.time()
    r = subprocess.run([cli, "-map", fq, "-ufi", ufi, "-samout", out] + extra, capture_output=True, text=True, timeout=1800)
    wall = time.time() - t0
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    m = re.search(r"([0-9]+)\s+Reads/sec", r.stderr)
    return {"reads_per_s": float(m.group(1)) if m else None, "process_wall_s": wall, "file_bytes": os.path.getsize(out)}


def summarise(runs):
    """the first run (it also pages the FASTQ in) is left out of the median"""
    rates = [r["reads_per_s"] for r in runs]
    return {"reads_per_s_runs": rates, "median_reads_per_s": float(np.median(rates[1:] or rates)), "file_bytes": runs[-1]["file_bytes"],
            "process_wall_s_last": runs[-1]["process_wall_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-mbp", type=float, default=20.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5, help="file-to-file runs per variant; the first is left out of the median")
    ap.add_argument("--kernel-mb", type=int, default=512)
    ap.add_argument("--out-dir", default=None, help="where the SAM files go (the medium that is measured)")
    ap.add_argument("--other-cli", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    res = {}
    with tempfile.TemporaryDirectory(dir=args.out_dir) as d:
        g = synth.make_genome(5, [int(args.genome_mbp * 1e6)], repeat_frac=0.05, n_families=8)
        fa, ufi, fq = os.path.join(d, "g.fa"), os.path.join(d, "g.ufi"), os.path.join(d, "r.fq")
        synth.write_fasta(fa, g)
        subprocess.run([CLI, "-make_ufi", fa, "-output", ufi, "-quiet"], check=True, capture_output=True, timeout=1800)
        write_fastq(fq, rng, g[0][1], args.reads, 150)
        res["reads"] = args.reads
        res["fastq_bytes"] = os.path.getsize(fq)
        res["medium"] = medium_of(d)
        plain, z = os.path.join(d, "out.sam"), os.path.join(d, "out.sam.bgzf")
        # the variants take turns, round after round, so that a drift of the machine falls on all of them alike
        runs = {"plain": [], "bgzf": [], "other_cli_plain": []}
        for _ in range(args.rounds):
            runs["plain"].append(run_cli(CLI, fq, ufi, plain, []))
            runs["bgzf"].append(run_cli(CLI, fq, ufi, z, ["-bgzf"]))
            if args.other_cli:
                runs["other_cli_plain"].append(run_cli(args.other_cli, fq, ufi, os.path.join(d, "other.sam"), []))
        f = {k: summarise(v) for k, v in runs.items() if v}
        if args.other_cli:
            f["other_cli"] = args.other_cli
        f["rounds"] = args.rounds
        f["file_ratio"] = f["bgzf"]["file_bytes"] / f["plain"]["file_bytes"]
        res["file"] = f
        with open(plain, "rb") as fh:
            text = fh.read(args.kernel_mb << 20)
        os.remove(plain)
        ms = []
        for step in range(args.warmup + args.steps):
            blob, t = api.bgzf_compress_timed(text, device=0)
            if step >= args.warmup:
                ms.append(t)
        med = float(np.median(ms))
        res["kernel"] = {"text_bytes": len(text), "compressed_bytes": len(blob), "ratio": len(blob) / len(text), "ms": ms, "median_ms": med,
                         "ms_per_GB_text": med / (len(text) / 1e9), "GB_text_per_s": len(text) / 1e6 / med}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bgzf_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
