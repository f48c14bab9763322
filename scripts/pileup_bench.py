#!/usr/bin/env python3
"""Measures -vcfout (urmap_amd/csrc/pileup.hip) on one GPU and prints one JSON object per read kind (single-end, paired):

  The reads (the generator, genome and mapping of scripts/markdup_bench.py) are mapped ONCE in this process to raw BAM records, as a lane
  hands them to -sort.  Then, on these same kept records and in this same process, the planned device sort with marking
  (urmapx_bam_sort_external, what -sort -markdup runs) is called --rounds times without the pileup, --rounds times with it
  (urmapx_bam_sort_with; the bases are the index's resident sequence store, read in place) and --rounds times with the depth, the
  statistics and the pileup together, taking turns (a drift of the machine falls on all alike), after one warm-up of each.  Without
  the pileup the call runs no line of its code.
      wall_s of the first two: median, min, max; added_wall_s: with minus without, median of the rounds' differences
      pileup_parts_s: alloc, count, sites, format, copy of the pileup's result, each median, min, max; in core count_s is the one
          launch of pileup_count_kernel over all records and the wait for it
      increments: with min_baseq 0 and reads without N every covered base of every counted record is one atomic add, and their number
          is the depth's sum of bases (urmapx_bam_sort_with on the same records); --rounds more sorts with the pileup at min_baseq 0
          give increments_per_s and added_bytes_per_s (4 bytes an increment) against their count_s (median).  At the default floor
          of 13 fewer bases count; that count_s is the one in pileup_parts_s
      counter_bytes and sites_bytes_per_s: the counters' 16 bytes a column over sites_s (median)
      yardsticks of the same rounds (the third kind of call): the statistics' count_s (stats_count_kernel) and the depth's count_s
          (depth_count_kernel) beside the pileup's count_s, all three one launch over the same record bytes and the wait for it
      standalone: urmapx_bam_pileup of the same records (they stream through its staging buffers, the bases are uploaded): wall, parts
      host: urmapx_bam_pileup_host of the same records (one thread), wall, --host-rounds times
  There is no target: what is reported is the added time against -sort -markdup alone, the kernel against the two yardsticks and
  against the float-atomic rate of the hardware guide (the only yardstick there is; unmeasured for integer adds of one dword per 16
  bytes), and the device road against the host function.

    python scripts/pileup_bench.py [--reads 4000000] [--genome-mbp 20] [--rounds 5] [--host-rounds 1] [--out DIR]

--out: a directory that receives pileup_bench_se.json and pileup_bench_pe.json.
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

PARTS = ("alloc_s", "count_s", "sites_s", "format_s", "copy_s")
FLOAT_ATOMIC_BYTES_PER_S = 1.3e12  # the hardware guide's chip-wide rate of float atomic adds in contiguous 256-byte wave instructions


def measure(records, n_ref, names, lens, seqs, idx, rounds, host_rounds):
    kinds = ("plain", "pileup", "all")
    runs = {k: [] for k in kinds}
    text = None
    for k in range(rounds + 1):  # (round 0 is the warm-up and is left out)
        for kind in kinds:
            t0 = time.time()
            out = api.bam_sort(records, n_ref, report=True, markdup=True, budget=0, depth=(names, lens) if kind == "all" else None,
                               stats=(names, lens) if kind == "all" else None, pileup=(names, lens, idx, None) if kind != "plain" else None)
            rep = out[-1]
            rep["wall_s"] = time.time() - t0
            runs[kind].append(rep)
            if kind == "pileup":
                text = out[2]
        print(f"round {k}: sort + markdup {runs['plain'][-1]['wall_s']:.3f} s, with the pileup {runs['pileup'][-1]['wall_s']:.3f} s, with all three "
              f"{runs['all'][-1]['wall_s']:.3f} s", file=sys.stderr, flush=True)
    plain, with_pileup, with_all = (runs[k][1:] for k in kinds)
    n_bytes, columns = plain[-1]["stream_bytes"], int(sum(lens))
    res = {"records": plain[-1]["records"], "record_bytes": n_bytes, "rounds": rounds, "external": plain[-1]["external"], "references": n_ref, "columns": columns,
           "sort_markdup": {"wall_s": spread([r["wall_s"] for r in plain])},
           "sort_markdup_pileup": {"wall_s": spread([r["wall_s"] for r in with_pileup])},
           "added_wall_s": spread([b["wall_s"] - a["wall_s"] for a, b in zip(plain, with_pileup)]),
           "pileup_parts_s": {k: spread([r["pileup_" + k] for r in with_pileup]) for k in PARTS},
           "same_rounds_count_s": {"pileup": spread([r["pileup_count_s"] for r in with_all]), "stats": spread([r["stats_count_s"] for r in with_all]),
                                   "depth": spread([r["depth_count_s"] for r in with_all])},
           "gather_s": spread([r["gather_s"] for r in with_pileup]),
           "text_bytes": len(text), "resident_bytes": api.bam_pileup_resident_bytes(columns, n_ref, True), "counter_bytes": 16 * columns,
           "totals": {k: with_pileup[-1]["pileup_" + k] for k in ("records", "sites", "alt_alleles")}}
    res["pileup_over_stats"] = res["same_rounds_count_s"]["pileup"]["median"] / res["same_rounds_count_s"]["stats"]["median"]
    res["pileup_over_depth"] = res["same_rounds_count_s"]["pileup"]["median"] / res["same_rounds_count_s"]["depth"]["median"]
    res["sites_bytes_per_s"] = 16 * columns / res["pileup_parts_s"]["sites_s"]["median"]
    alone = []
    for k in range(rounds + 1):
        t0 = time.time()
        got, rep = api.bam_pileup(records, n_ref, names, lens, seqs, report=True)
        rep["wall_s"] = time.time() - t0
        alone.append(rep)
    res["standalone"] = {k: spread([r[k] for r in alone[1:]]) for k in PARTS + ("wall_s",)}
    res["standalone"]["stage_chunks"] = alone[-1]["stage_chunks"]
    res["standalone_sites"] = alone[-1]["sites"]
    host = []
    for k in range(host_rounds):
        t0 = time.time()
        want, hrep = api.bam_pileup_host(records, n_ref, names, lens, seqs, report=True)
        host.append(time.time() - t0)
    res["host"] = {"wall_s": spread(host), "count_s": hrep["count_s"], "sites_s": hrep["sites_s"], "format_s": hrep["format_s"],
                   "threads_granted": int(os.environ.get("OMP_NUM_THREADS", "0")) or None, "threads_used": 1}
    res["host_over_standalone"] = res["host"]["wall_s"]["median"] / res["standalone"]["wall_s"]["median"]
    res["standalone_equals_host"] = got == want
    # the increments: at min_baseq 0 (reads without N) they are the depth's sum of bases
    depth_bases = sum(r["bases"] for r in api.bam_sort(records, n_ref, markdup=True, budget=0, depth=(names, lens))[2][2])
    q0 = [api.bam_sort(records, n_ref, report=True, markdup=True, budget=0, pileup=(names, lens, idx, {"min_baseq": 0}))[-1]["pileup_count_s"]
          for k in range(rounds + 1)][1:]
    res["baseq0"] = {"count_s": spread(q0), "increments": int(depth_bases), "increments_per_s": depth_bases / float(np.median(q0)),
                     "added_bytes_per_s": 4 * depth_bases / float(np.median(q0))}
    res["float_atomic_yardstick_bytes_per_s"] = FLOAT_ATOMIC_BYTES_PER_S
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
        seqs = [np.asarray(s, dtype=np.uint8).tobytes() for _, s in g]
        assert [len(s) for s in seqs] == lens
        m = api.Mapper(idx, device=0)
        m.set_bam(True)
        for kind, n in (("se", args.reads), ("pe", args.reads // 2)):
            rng = np.random.default_rng(2026)
            records = kept_records(m, rng, g[0][1], n, 150, kind == "pe")
            res = {"kind": kind, "reads": n * (2 if kind == "pe" else 1), "genome_mbp": args.genome_mbp}
            res.update(measure(records, len(names), names, lens, seqs, idx, args.rounds, args.host_rounds))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(args.out, exist_ok=True)
                with open(os.path.join(args.out, f"pileup_bench_{kind}.json"), "w") as fh:
                    fh.write(line + "\n")
            del records
        m.set_bam(False)
        m.close()


if __name__ == "__main__":
    main()
