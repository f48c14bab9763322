#!/usr/bin/env python3
"""Measures -markdup (urmap_amd/csrc/markdup.hip) on one GPU and prints one JSON object per read kind (single-end, paired):

  The reads (the generator and genome of scripts/bam_sort_bench.py; for pairs, two mates 300 +- 30 bases apart) are mapped ONCE in this
  process to raw BAM records, as a lane hands them to -sort.  Then, on these same kept records and in this same process, the device
  sort runs --rounds times without the option and --rounds times with it, taking turns (a drift of the machine falls on both alike),
  after one warm-up of each:
      sort_s, index_s, gather_s, deflate_s and the call's wall, without and with the option: median, min, max
      markdup_s: median, min, max; added_wall_s: the call's wall with the option minus without, median of the rounds' differences
      markdup_over_sort_index: markdup_s / (sort_s + index_s) of the plain call
      parts: two more calls under URMAPX_VERBOSE, which waits for the stream after each part: ends (ends, range, pack, first), pairs,
             fragments -- and the counters
  There is no target: what is reported is the added time against -sort alone.

    python scripts/markdup_bench.py [--reads 4000000] [--genome-mbp 20] [--rounds 5] [--out DIR]

--out: a directory that receives markdup_bench_se.json and markdup_bench_pe.json.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bgzf_bench import ACGT, CLI, QBINS  # noqa: E402
from urmap_amd import api, synth  # noqa: E402

CHUNK = 250000  # reads (pairs) handed to the text stage at a time
COMP = np.full(256, ord("N"), np.uint8)
COMP[list(b"ACGTN")] = list(b"TGCAN")
TIMES = ("sort_s", "index_s", "gather_s", "deflate_s", "upload_s", "scan_s")


def fastq_chunks(rng, genome, n, L, paired):
    """FASTQ text of n reads (pairs) in chunks: (mate 1 bytes, mate 2 bytes | None).  1 % substitutions; pairs face each other"""
    for lo in range(0, n, CHUNK):
        k = min(CHUNK, n - lo)
        ins = np.clip(rng.normal(300, 30, k).astype(np.int64), L, 600) if paired else np.full(k, L)
        starts = rng.integers(0, len(genome) - 600, size=k)
        mates = []
        for m in range(2 if paired else 1):
            at = starts if m == 0 else starts + ins - L
            reads = genome[at[:, None] + np.arange(L)[None, :]]
            sub = rng.random((k, L)) < 0.01
            reads[sub] = ACGT[rng.integers(0, 4, size=int(sub.sum()))]
            if m == 1:
                reads = COMP[reads[:, ::-1]]
            quals = QBINS[rng.choice(4, size=(k, L), p=[0.85, 0.10, 0.04, 0.01])]
            mates.append(b"".join(b"@read%d\n%s\n+\n%s\n" % (lo + i, reads[i].tobytes(), quals[i].tobytes()) for i in range(k)))
        yield mates[0], (mates[1] if paired else None)


def kept_records(m, rng, genome, n, L, paired):
    out = []
    for a, b in fastq_chunks(rng, genome, n, L, paired):
        raw, rep = m.map_text_pe(a, b) if paired else m.map_text_se(a)
        assert rep["reason"] == api.TEXT_OK, rep
        out.append(raw)
    return b"".join(out)


def stderr_of(fn):
    """what the library writes to file descriptor 2 while fn runs"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return f.read().decode("latin-1")


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [float(x) for x in v]}


def measure(records, n_ref, rounds):
    runs = {False: [], True: []}
    for k in range(rounds + 1):  # (round 0 is the warm-up and is left out)
        for md in (False, True):
            t0 = time.time()
            _, _, rep = api.bam_sort(records, n_ref, report=True, markdup=md)
            rep["wall_s"] = time.time() - t0
            runs[md].append(rep)
        print(f"round {k}: sort {runs[False][-1]['wall_s']:.3f} s, sort + markdup {runs[True][-1]['wall_s']:.3f} s "
              f"(markdup_s {runs[True][-1]['markdup_s']:.4f})", file=sys.stderr, flush=True)
    plain, marked = runs[False][1:], runs[True][1:]
    res = {"records": plain[-1]["records"], "record_bytes": plain[-1]["stream_bytes"], "sort_passes": plain[-1]["sort_passes"], "rounds": rounds,
           "sort": {k: spread([r[k] for r in plain]) for k in TIMES + ("wall_s",)},
           "sort_markdup": {k: spread([r[k] for r in marked]) for k in TIMES + ("wall_s", "markdup_s")},
           "added_wall_s": spread([b["wall_s"] - a["wall_s"] for a, b in zip(plain, marked)]),
           "counters": {k: marked[-1][k] for k in ("pairs_examined", "pairs_duplicate", "fragments_examined", "fragments_duplicate")}}
    base = res["sort"]["sort_s"]["median"] + res["sort"]["index_s"]["median"]
    res["markdup_over_sort_index"] = res["sort_markdup"]["markdup_s"]["median"] / base if base else None
    res["markdup_ms_per_1M_records"] = 1e3 * res["sort_markdup"]["markdup_s"]["median"] / (res["records"] / 1e6)
    os.environ["URMAPX_VERBOSE"] = "1"
    parts = []
    try:
        for _ in range(2):
            m = re.search(r"markdup parts: ends ([0-9.]+) pairs ([0-9.]+) fragments ([0-9.]+); records (\d+) pairs (\d+) eligible (\d+) end_bits (\d+)",
                          stderr_of(lambda: api.bam_sort(records, n_ref, markdup=True)))
            if m:
                parts.append(m.groups())
    finally:
        del os.environ["URMAPX_VERBOSE"]
    if parts:
        last = parts[-1]
        res["parts_s"] = {"ends": float(last[0]), "pairs": float(last[1]), "fragments": float(last[2])}
        res.update(eligible=int(last[5]), end_bits=int(last[6]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000, help="single-end reads; the paired run takes half as many pairs")
    ap.add_argument("--genome-mbp", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5, "medians over at least five repetitions"
    import subprocess
    with tempfile.TemporaryDirectory() as d:
        g = synth.make_genome(5, [int(args.genome_mbp * 1e6)], repeat_frac=0.05, n_families=8)
        fa, ufi = os.path.join(d, "g.fa"), os.path.join(d, "g.ufi")
        synth.write_fasta(fa, g)
        subprocess.run([CLI, "-make_ufi", fa, "-output", ufi, "-quiet"], check=True, capture_output=True, timeout=1800)
        idx = api.Index.open(ufi).upload(0)
        n_ref = len(idx.directory())
        m = api.Mapper(idx, device=0)
        m.set_bam(True)
        for kind, n in (("se", args.reads), ("pe", args.reads // 2)):
            rng = np.random.default_rng(2026)
            records = kept_records(m, rng, g[0][1], n, 150, kind == "pe")
            res = {"kind": kind, "reads": n * (2 if kind == "pe" else 1), "genome_mbp": args.genome_mbp}
            res.update(measure(records, n_ref, args.rounds))
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(args.out, exist_ok=True)
                with open(os.path.join(args.out, f"markdup_bench_{kind}.json"), "w") as fh:
                    fh.write(line + "\n")
            del records
        m.set_bam(False)
        m.close()


if __name__ == "__main__":
    main()
