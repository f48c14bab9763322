#!/usr/bin/env python3
"""Measures -bamout (urmap_amd/csrc/bam_gpu.hip) on one GPU and prints one JSON object:

  file     `urmap -map reads.fq` file to file three ways -- `-samout F` (plain), `-samout F -bgzf`, `-bamout F` --: reads/s as the
           command reports them (first read parsed to last byte written, index load excluded), the median of --rounds runs without the
           first (it also pages the FASTQ in), the spread (max - min) / median of those runs, bytes written per read, the medium F is
           on (--out-dir, default a temporary directory: state it with the number).  --other-cli PATH times the plain and the -bgzf
           run of another build's command line on the same files in the same rounds (the parent commit's: what this build's two
           unchanged roads are held against)
  kernel   the format stage of one chunk of --kernel-reads records on its stream, by events (report ms_format: the length pass, the
           prefix sum and the write pass), as SAM text and as BAM records, per 1 M records; median of --steps chunks after a warm-up

The reads are those of scripts/bgzf_bench.py (same generator, same seed).

    python scripts/bam_bench.py [--reads 10000000] [--genome-mbp 20] [--steps 5] [--rounds 6] [--out-dir DIR] [--other-cli PATH] [--out DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bgzf_bench import CLI, medium_of, run_cli, write_fastq  # noqa: E402
from urmap_amd import api, synth  # noqa: E402


def run_bam(cli, fq, ufi, out):
    """run_cli with -bamout in -samout's place"""
    import re
    import time
    t0 = time.time()
    r = subprocess.run([cli, "-map", fq, "-ufi", ufi, "-bamout", out], capture_output=True, text=True, timeout=1800)
    wall = time.time() - t0
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    m = re.search(r"([0-9]+)\s+Reads/sec", r.stderr)
    return {"reads_per_s": float(m.group(1)) if m else None, "process_wall_s": wall, "file_bytes": os.path.getsize(out)}


def summarise(runs, reads):
    rates = [r["reads_per_s"] for r in runs]
    kept = rates[1:] or rates  # the first run also pages the FASTQ in
    med = float(np.median(kept))
    return {"reads_per_s_runs": rates, "median_reads_per_s": med, "spread": (max(kept) - min(kept)) / med if med else None,
            "file_bytes": runs[-1]["file_bytes"], "bytes_per_read": runs[-1]["file_bytes"] / reads}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-mbp", type=float, default=20.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=6, help="file-to-file runs per variant; the first is left out of the median")
    ap.add_argument("--kernel-reads", type=int, default=1 << 20)
    ap.add_argument("--out-dir", default=None, help="where the output files go (the medium that is measured)")
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
        out = lambda n: os.path.join(d, n)
        # the variants take turns, round after round, so that a drift of the machine falls on all of them alike
        runs = {"plain": [], "bgzf": [], "bam": [], "other_cli_plain": [], "other_cli_bgzf": []}
        for k in range(args.rounds):
            runs["plain"].append(run_cli(CLI, fq, ufi, out("out.sam"), []))
            runs["bgzf"].append(run_cli(CLI, fq, ufi, out("out.sam.bgzf"), ["-bgzf"]))
            runs["bam"].append(run_bam(CLI, fq, ufi, out("out.bam")))
            if args.other_cli:
                runs["other_cli_plain"].append(run_cli(args.other_cli, fq, ufi, out("other.sam"), []))
                runs["other_cli_bgzf"].append(run_cli(args.other_cli, fq, ufi, out("other.sam.bgzf"), ["-bgzf"]))
            print(f"round {k}: " + ", ".join(f"{n} {v[-1]['reads_per_s'] / 1e6:.2f} M/s" for n, v in runs.items() if v), file=sys.stderr, flush=True)
        f = {k: summarise(v, args.reads) for k, v in runs.items() if v}
        if args.other_cli:
            f["other_cli"] = args.other_cli
        f["rounds"] = args.rounds
        res["file"] = f
        for n in ("out.sam", "out.sam.bgzf", "out.bam", "other.sam", "other.sam.bgzf"):
            if os.path.exists(out(n)):
                os.remove(out(n))
        # the format stage alone: one chunk of the same reads, SAM text against BAM records
        with open(fq, "rb") as fh:
            chunk = fh.read(400 * args.kernel_reads)
        lines = chunk.split(b"\n")
        nrec = min(args.kernel_reads, (len(lines) - 1) // 4)
        chunk = b"\n".join(lines[:4 * nrec]) + b"\n"
        m = api.Mapper(api.Index.open(ufi).upload(0), device=0)
        kern = {"records": nrec}
        for name, on in (("sam", False), ("bam", True)):
            m.set_bam(on)
            ms, nbytes = [], 0
            for step in range(args.warmup + args.steps):
                (z, rep), = m.map_text_se_stream([chunk])
                assert rep["reason"] == api.TEXT_OK and rep["records"] == nrec, rep
                nbytes = rep["sam_text_bytes"]
                if step >= args.warmup:
                    ms.append(rep["ms_format"])
            kern[name] = {"ms_format": ms, "median_ms_per_1M_records": float(np.median(ms)) * 1e6 / nrec, "bytes_per_record": nbytes / nrec}
        m.set_bam(False)
        m.close()
        res["kernel"] = kern
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bam_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
