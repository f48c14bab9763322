#!/usr/bin/env python3
"""Measures -depth (urmap_amd/csrc/depth.hip) on one GPU and prints one JSON object per read kind (single-end, paired):

  The reads (the generator, genome and mapping of scripts/markdup_bench.py) are mapped ONCE in this process to raw BAM records, as a lane
  hands them to -sort.  Then, on these same kept records and in this same process, the planned device sort with marking
  (urmapx_bam_sort_external, what -sort -markdup runs) is called --rounds times without the depth and --rounds times with it
  (urmapx_bam_sort_with), taking turns (a drift of the machine falls on both alike), after one warm-up of each.  Without the depth the
  call runs no line of the depth's code.
      wall_s of both: median, min, max; added_wall_s: with minus without, median of the rounds' differences
      depth_parts_s: alloc, count, scan, runs, format, copy of the depth result, each median, min, max
      text_bytes, runs, text_slices, covered, bases
      standalone: urmapx_bam_depth of the same records (they stream through its staging buffers): wall and parts
      host: urmapx_bam_depth_host of the same records, wall, --host-rounds times
  There is no target: what is reported is the added time against -sort -markdup alone, and the device road against the host function.

    python scripts/depth_bench.py [--reads 4000000] [--genome-mbp 20] [--rounds 5] [--host-rounds 3] [--out DIR]

--out: a directory that receives depth_bench_se.json and depth_bench_pe.json.
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

PARTS = ("alloc_s", "count_s", "scan_s", "runs_s", "format_s", "copy_s")


def measure(records, n_ref, names, lens, rounds, host_rounds):
    runs = {False: [], True: []}
    depth = None
    for k in range(rounds + 1):  # (round 0 is the warm-up and is left out)
        for on in (False, True):
            t0 = time.time()
            out = api.bam_sort(records, n_ref, report=True, markdup=True, budget=0, depth=(names, lens) if on else None)
            rep = out[-1]
            rep["wall_s"] = time.time() - t0
            runs[on].append(rep)
            if on:
                depth = out[2]
        print(f"round {k}: sort + markdup {runs[False][-1]['wall_s']:.3f} s, with depth {runs[True][-1]['wall_s']:.3f} s", file=sys.stderr, flush=True)
    plain, with_depth = runs[False][1:], runs[True][1:]
    text, n_runs, summ = depth
    res = {"records": plain[-1]["records"], "record_bytes": plain[-1]["stream_bytes"], "rounds": rounds, "external": plain[-1]["external"],
           "columns": int(sum(lens)), "references": n_ref,
           "sort_markdup": {"wall_s": spread([r["wall_s"] for r in plain])},
           "sort_markdup_depth": {"wall_s": spread([r["wall_s"] for r in with_depth])},
           "added_wall_s": spread([b["wall_s"] - a["wall_s"] for a, b in zip(plain, with_depth)]),
           "depth_parts_s": {k: spread([r["depth_" + k] for r in with_depth]) for k in PARTS},
           "text_bytes": len(text), "runs": n_runs, "text_slices": with_depth[-1]["depth_text_slices"],
           "covered": sum(s["covered"] for s in summ), "bases": sum(s["bases"] for s in summ), "reads_counted": sum(s["reads"] for s in summ)}
    res["depth_parts_sum_s"] = sum(res["depth_parts_s"][k]["median"] for k in PARTS)
    alone = []
    for k in range(rounds + 1):
        t0 = time.time()
        rep = api.bam_depth(records, n_ref, names, lens, report=True)[3]
        rep["wall_s"] = time.time() - t0
        alone.append(rep)
    res["standalone"] = {k: spread([r[k] for r in alone[1:]]) for k in PARTS + ("wall_s",)}
    res["standalone"]["stage_chunks"] = alone[-1]["stage_chunks"]
    host = []
    for k in range(host_rounds):
        t0 = time.time()
        got = api.bam_depth_host(records, n_ref, names, lens)
        host.append(time.time() - t0)
    res["host"] = {"wall_s": spread(host), "threads_granted": int(os.environ.get("OMP_NUM_THREADS", "0")) or None}
    res["host_over_standalone"] = res["host"]["wall_s"]["median"] / res["standalone"]["wall_s"]["median"]
    res["standalone_equals_host"] = got == api.bam_depth(records, n_ref, names, lens)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000, help="single-end reads; the paired run takes half as many pairs")
    ap.add_argument("--genome-mbp", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=3)
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
                with open(os.path.join(args.out, f"depth_bench_{kind}.json"), "w") as fh:
                    fh.write(line + "\n")
            del records
        m.set_bam(False)
        m.close()


if __name__ == "__main__":
    main()
