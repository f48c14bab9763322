#!/usr/bin/env python3
"""Measures -stats (urmap_amd/csrc/stats.hip) on one GPU and prints one JSON object per read kind (single-end, paired):

  The reads (the generator, genome and mapping of scripts/markdup_bench.py) are mapped ONCE in this process to raw BAM records, as a lane
  hands them to -sort.  Then, on these same kept records and in this same process, the planned device sort with marking
  (urmapx_bam_sort_external, what -sort -markdup runs) is called --rounds times without the statistics and --rounds times with them
  (urmapx_bam_sort_with), taking turns (a drift of the machine falls on both alike), after one warm-up of each.  Without the
  statistics the call runs no line of their code.
      wall_s of both: median, min, max; added_wall_s: with minus without, median of the rounds' differences
      stats_parts_s: alloc, count, format of the statistics' result, each median, min, max; in core count_s is the one launch of
          stats_count_kernel over all records and the wait for it
      count_bytes_per_s: the record bytes over count_s (median)
      yardsticks of the same rounds: gather_s of the sort (gather_kernel: one pass that reads and writes the same record bytes, with its
          launches' waits) and, from --rounds sorts with the depth, the depth's count_s (depth_count_kernel on the same records)
      standalone: urmapx_bam_stats of the same records (they stream through its staging buffers): wall and parts
      host: urmapx_bam_stats_host of the same records (one thread), wall, --host-rounds times
  There is no target: what is reported is the added time against -sort -markdup alone, the kernel against the two yardsticks, and the
  device road against the host function.

    python scripts/stats_bench.py [--reads 4000000] [--genome-mbp 20] [--rounds 5] [--host-rounds 1] [--out DIR]

--out: a directory that receives stats_bench_se.json and stats_bench_pe.json.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bgzf_bench import CLI  # noqa: E402
from markdup_bench import kept_records, spread  # noqa: E402
from urmap_amd import api, synth  # noqa: E402

PARTS = ("alloc_s", "count_s", "format_s")


def measure(records, n_ref, names, lens, rounds, host_rounds):
    runs = {False: [], True: []}
    text = None
    for k in range(rounds + 1):  # (round 0 is the warm-up and is left out)
        for on in (False, True):
            t0 = time.time()
            out = api.bam_sort(records, n_ref, report=True, markdup=True, budget=0, stats=(names, lens) if on else None)
            rep = out[-1]
            rep["wall_s"] = time.time() - t0
            runs[on].append(rep)
            if on:
                text = out[2]
        print(f"round {k}: sort + markdup {runs[False][-1]['wall_s']:.3f} s, with stats {runs[True][-1]['wall_s']:.3f} s", file=sys.stderr, flush=True)
    plain, with_stats = runs[False][1:], runs[True][1:]
    n_bytes = plain[-1]["stream_bytes"]
    res = {"records": plain[-1]["records"], "record_bytes": n_bytes, "rounds": rounds, "external": plain[-1]["external"], "references": n_ref,
           "sort_markdup": {"wall_s": spread([r["wall_s"] for r in plain])},
           "sort_markdup_stats": {"wall_s": spread([r["wall_s"] for r in with_stats])},
           "added_wall_s": spread([b["wall_s"] - a["wall_s"] for a, b in zip(plain, with_stats)]),
           "stats_parts_s": {k: spread([r["stats_" + k] for r in with_stats]) for k in PARTS},
           "gather_s": spread([r["gather_s"] for r in with_stats]), "slices": with_stats[-1]["slices"],
           "text_bytes": len(text), "resident_bytes": api.bam_stats_resident_bytes(n_ref),
           "totals": {k: with_stats[-1]["stats_" + k] for k in ("reads", "mapped", "properly_paired", "duplicated", "insert_median")}}
    res["count_bytes_per_s"] = n_bytes / res["stats_parts_s"]["count_s"]["median"]
    res["gather_bytes_per_s"] = n_bytes / res["gather_s"]["median"]
    res["count_over_gather"] = res["stats_parts_s"]["count_s"]["median"] / res["gather_s"]["median"]
    depth = []
    for k in range(rounds + 1):
        depth.append(api.bam_sort(records, n_ref, report=True, markdup=True, budget=0, depth=(names, lens))[-1]["depth_count_s"])
    res["depth_count_s"] = spread(depth[1:])
    alone = []
    for k in range(rounds + 1):
        t0 = time.time()
        rep = api.bam_stats(records, n_ref, names, lens, report=True)[1]
        rep["wall_s"] = time.time() - t0
        alone.append(rep)
    res["standalone"] = {k: spread([r[k] for r in alone[1:]]) for k in PARTS + ("wall_s",)}
    res["standalone"]["stage_chunks"] = alone[-1]["stage_chunks"]
    host = []
    for k in range(host_rounds):
        t0 = time.time()
        got = api.bam_stats_host(records, n_ref, names, lens)
        host.append(time.time() - t0)
    res["host"] = {"wall_s": spread(host), "threads_granted": int(os.environ.get("OMP_NUM_THREADS", "0")) or None, "threads_used": 1}
    res["host_over_standalone"] = res["host"]["wall_s"]["median"] / res["standalone"]["wall_s"]["median"]
    res["standalone_equals_host"] = got == api.bam_stats(records, n_ref, names, lens)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000, help="single-end reads; the paired run takes half as many pairs")
    ap.add_argument("--genome-mbp", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5, "medians over at least five repetitions"
    with tempfile.TemporaryDirectory() as d:
        g = synth.make_genome(5, [int(args.genome_mbp * 1e6)], repeat_frac=0.05, n_families=8)
        fa, ufi = os.path.join(d, "g.fa"), os.path.join(d, "g.ufi")
        synth.write_fasta(fa, g)
        subprocess.run([CLI, "-make_ufi", fa, "-output", ufi, "-quiet"], check=True, capture_output=True, timeout=1800)
        idx = api.Index.open(ufi).upload(0)
        directory = idx.directory()
        names, lens = [x[0] for x in directory], [x[1] for x in directory]
        m = api.Mapper(idx, device=0)
        m.set_bam(True)
        for kind, n in (("se", args.reads), ("pe", args.reads // 2)):
            rng = np.random.default_rng(2026)
            records = kept_records(m, rng, g[0][1], n, 150, kind == "pe")
            res = {"kind": kind, "reads": n * (2 if kind == "pe" else 1), "genome_mbp": args.genome_mbp}
            res.update(measure(records, len(names), names, lens, args.rounds, args.host_rounds))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(args.out, exist_ok=True)
                with open(os.path.join(args.out, f"stats_bench_{kind}.json"), "w") as fh:
                    fh.write(line + "\n")
            del records
        m.set_bam(False)
        m.close()


if __name__ == "__main__":
    main()
