#!/usr/bin/env python3
"""Measures the k-mer bit-vector filter (urmap_amd/csrc/bitvec.hip) on one GPU and prints one JSON object:

  search   the search kernel alone (HIP events on the bit vector's stream) over N resident 150-base reads, at W = 14 (a 32 MiB table
           that stays in cache), 16 and 18 (tables in HBM); a fraction --hit-frac of the reads is drawn from the genome the table was
           built from, the rest are random bases (the found fraction is reported as measured)
  build    the include launch for a --build-gbp genome (urmap_amd.synth) at W = 16 and 18 (events; the upload of the sequence store
           is not in it) and the whole urmapx_bitvec_build call (wall clock)
  file     `urmap -search_bitvec` file to file (wall clock, process start to exit) at W = 16, and the reference binary's
           `-search_bitvec -threads 16` on the same files when oracle/_ref/urmap is present

    python scripts/bitvec_bench.py [--reads 4000000] [--steps 5] [--build-gbp 3.1] [--file-reads 2000000] [--out DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from urmap_amd import api, synth  # noqa: E402

CLI = os.path.join(ROOT, "urmap_amd", "urmap")
REF = os.path.join(ROOT, "oracle", "_ref", "urmap")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_reads(rng, genome, n, L, hit_frac):
    """n reads of L bases, a fraction hit_frac drawn from the genome (either orientation), the rest random"""
    reads = ACGT[rng.integers(0, 4, size=(n, L))]
    nh = int(n * hit_frac)
    g = genome
    starts = rng.integers(0, len(g) - L, size=nh)
    idx = starts[:, None] + np.arange(L)[None, :]
    reads[:nh] = g[idx]
    flip = rng.random(nh) < 0.5
    rc = synth.revcomp(reads[:nh][flip].reshape(-1)).reshape(-1, L)[::-1]
    reads[:nh][flip] = rc
    rng.shuffle(reads)
    return reads


def bench_search(args, rng, genome):
    import torch
    out = {}
    L = 150
    reads = make_reads(rng, genome, args.reads, L, args.hit_frac)
    offs = (np.arange(args.reads + 1, dtype=np.int64) * L)
    db = torch.from_numpy(reads.reshape(-1).copy()).cuda()
    do = torch.from_numpy(offs).cuda()
    dv = torch.zeros(args.reads, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for W in (14, 16, 18):
        bv, counts = api.BitVec.build(0, [genome.tobytes()], [], W)
        ms = []
        for step in range(args.warmup + args.steps):
            bv.search_device(db.data_ptr(), do.data_ptr(), args.reads, dv.data_ptr())
            bv.sync()
            if step >= args.warmup:
                ms.append(bv.last_ms()[2])
        v = dv.cpu().numpy()
        med = float(np.median(ms))
        out[f"W{W}"] = {"table_bytes": bv.nbytes, "words": counts[0], "reads": args.reads, "read_len": L, "ms": ms, "median_ms": med,
                        "M_reads_per_s": args.reads / med / 1e3, "found_frac": float((v != 0).mean()),
                        "forward_frac": float((v == 1).mean()), "reverse_frac": float((v == 2).mean())}
        bv.close()
    return out


def bench_build(args):
    n = max(1, int(round(args.build_gbp * 1e9 / 240e6)))
    lens = [int(args.build_gbp * 1e9 / n)] * n
    t0 = time.time()
    g = synth.make_genome(31, lens, repeat_frac=0.05, n_families=20)
    gen_s = time.time() - t0
    seqs = [s for _, s in g]
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    bases = np.concatenate(seqs)
    del g, seqs
    out = {"genome_bases": int(offs[-1]), "sequences": n, "synth_s": gen_s}
    for W in (16, 18):
        t0 = time.time()
        bv, counts = api.BitVec.build(0, (bases, offs), (), W)
        wall = time.time() - t0
        out[f"W{W}"] = {"include_kernel_ms": bv.last_ms()[0], "build_call_s": wall, "words": counts[0], "table_bytes": bv.nbytes}
        bv.close()
    return out


def bench_file(args, rng, genome, d):
    L = 150
    reads = make_reads(rng, genome, args.file_reads, L, args.hit_frac)
    fq = os.path.join(d, "r.fq")
    q = b"I" * L
    with open(fq, "wb") as f:
        for i in range(0, len(reads), 100000):
            f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i + k, r.tobytes(), q) for k, r in enumerate(reads[i:i + 100000])))
    fa, ex = os.path.join(d, "g.fa"), os.path.join(d, "e.fa")
    with open(fa, "wb") as f:
        f.write(b">g\n" + genome.tobytes() + b"\n")
    with open(ex, "wb") as f:
        f.write(b">e\n" + genome[:1000].tobytes() + b"\n")
    out = {"reads": args.file_reads, "read_len": L, "fastq_bytes": os.path.getsize(fq)}
    bv = os.path.join(d, "x.bv")
    subprocess.run([CLI, "-make_bitvec", fa, "-input2", ex, "-wordlength", "16", "-output", bv, "-quiet"], check=True, timeout=600)
    for rep in range(2):  # the first run also reads the FASTQ into the page cache
        t0 = time.time()
        r = subprocess.run([CLI, "-search_bitvec", fq, "-ref", bv, "-output", os.path.join(d, "h.fq")], capture_output=True, text=True,
                           timeout=600)
        wall = time.time() - t0
        if r.returncode:
            raise RuntimeError(r.stderr)
    out["urmap_s"] = wall
    out["urmap_M_reads_per_s"] = args.file_reads / wall / 1e6
    out["urmap_found"] = r.stderr.strip().splitlines()[-1]
    if os.path.exists(REF):
        rbv = os.path.join(d, "ref.bv")
        subprocess.run([REF, "-make_bitvec", fa, "-input2", ex, "-wordlength", "16", "-output", rbv], check=True, capture_output=True,
                       timeout=600)
        t0 = time.time()
        r = subprocess.run([REF, "-search_bitvec", fq, "-ref", rbv, "-output", os.path.join(d, "href.fq"), "-threads", "16"],
                           capture_output=True, text=True, timeout=1200)
        wall = time.time() - t0
        out["reference_threads16_s"] = wall
        out["reference_M_reads_per_s"] = args.file_reads / wall / 1e6
        out["reference_found"] = [l for l in r.stderr.splitlines() if "found" in l][-1:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--hit-frac", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-bp", type=int, default=200_000)
    ap.add_argument("--build-gbp", type=float, default=3.1)
    ap.add_argument("--file-reads", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")  # torch takes the device first
    rng = np.random.default_rng(2026)
    genome = synth.make_genome(5, [args.genome_bp], repeat_frac=0.0, n_families=0, n_run_frac=0.0)[0][1]
    res = {"device": torch.cuda.get_device_name(0), "search": bench_search(args, rng, genome)}
    with tempfile.TemporaryDirectory() as d:
        res["file"] = bench_file(args, rng, genome, d)
    if args.build_gbp > 0:
        res["build"] = bench_build(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bitvec_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
