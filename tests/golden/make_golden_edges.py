#!/usr/bin/env python3
"""Regenerates the edge fixtures in this directory (reads and pairs at the first and last bases of sequences and of the sequence
store, tests/edges_lib.py) with the UNMODIFIED reference binary (oracle/_ref/urmap, built by oracle/Makefile):

  edges.fa            five sequences of 1.5 .. 3 kbp of random ACGT (edges_lib.se_store)
  edges_se.fq.gz      edges_lib.golden_se: the 150-base flush reads of every edge and the sweep cases at which the outcome (unmapped /
                      ungapped / gapped) flips along the distance from the edge, with the case before each
  edges_se.sam.gz     reference `urmap -map edges_se.fq -ufi edges.ufi -samout ... -threads 1`, the @PG line dropped
  edges_rescue.fa     four sequences of 12.9 kbp around a 400-base repeat of 40 copies (edges_lib.rescue_store)
  edges_pe_1/2.fq.gz  edges_lib.golden_pe: rescue pairs at the first, a middle and the last copy of every sequence, minus anchors
                      around store position 1 024, 279-base mates, fragments at the sequences' edges
  edges_pe.sam.gz     reference `urmap -map2 edges_pe_1.fq -reverse edges_pe_2.fq -ufi edges_rescue.ufi -samout ... -threads 1`

Both indexes: reference `urmap -make_ufi X.fa -output X.ufi -slots 524309` (W = 24, MaxIx = 32); they are not kept, the tests build
them with the oracle (whose -make_ufi test_oracle_golden.py pins byte for byte).  Every case lies in the reference-defined subset:
nothing the reference does for it touches a byte behind the sequence store.  The selection needs an outcome per read; it is read off
the reference's own SAM of the whole 150-base sweep.

Run only where the reference binary has been built; the fixtures are data, the reference itself does not travel.
"""
import gzip
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edges_lib as el  # noqa: E402
import oracle_lib as ol  # noqa: E402
from urmap_amd import synth  # noqa: E402


def _gz(dst, data):
    with open(dst, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as z:
        z.write(data)


def main():
    if not ol.have_ref():
        sys.exit(f"{ol.REF_BIN} is not built (oracle/Makefile)")
    with tempfile.TemporaryDirectory() as d:
        st, rs = el.se_store(), el.rescue_store()
        for name, store in (("edges", st), ("edges_rescue", rs)):
            synth.write_fasta(os.path.join(HERE, name + ".fa"), store)
            synth.write_fasta(os.path.join(d, name + ".fa"), store)
            ol.run_ref(["-make_ufi", name + ".fa", "-output", name + ".ufi", "-slots", str(el.SLOTS)], cwd=d)

        def outcomes_of(reads):
            synth.write_fastq(os.path.join(d, "sweep.fq"), reads)
            ol.run_ref(["-map", "sweep.fq", "-ufi", "edges.ufi", "-samout", "sweep.sam", "-threads", "1"], cwd=d)
            return el.sam_outcomes(ol.sam_records(os.path.join(d, "sweep.sam")))

        reads, _ = el.golden_se(outcomes_of, st)
        synth.write_fastq(os.path.join(d, "edges_se.fq"), reads)
        ol.run_ref(["-map", "edges_se.fq", "-ufi", "edges.ufi", "-samout", "edges_se.sam", "-threads", "1"], cwd=d)
        _gz(os.path.join(HERE, "edges_se.fq.gz"), open(os.path.join(d, "edges_se.fq"), "rb").read())
        _gz(os.path.join(HERE, "edges_se.sam.gz"), b"\n".join(ol.sam_records(os.path.join(d, "edges_se.sam"))) + b"\n")
        pairs, _ = el.golden_pe(rs)
        pairs = el.strip_mate_suffix(pairs)
        synth.write_fastq(os.path.join(d, "edges_pe_1.fq"), pairs[0::2])
        synth.write_fastq(os.path.join(d, "edges_pe_2.fq"), pairs[1::2])
        ol.run_ref(["-map2", "edges_pe_1.fq", "-reverse", "edges_pe_2.fq", "-ufi", "edges_rescue.ufi", "-samout", "edges_pe.sam", "-threads", "1"], cwd=d)
        for suf in ("_1.fq", "_2.fq"):
            _gz(os.path.join(HERE, "edges_pe" + suf + ".gz"), open(os.path.join(d, "edges_pe" + suf), "rb").read())
        _gz(os.path.join(HERE, "edges_pe.sam.gz"), b"\n".join(ol.sam_records(os.path.join(d, "edges_pe.sam"))) + b"\n")
        print(f"{len(reads)} reads, {len(pairs) // 2} pairs")
        for n in sorted(os.listdir(HERE)):
            if n.startswith("edges"):
                print(n, os.path.getsize(os.path.join(HERE, n)))


if __name__ == "__main__":
    main()
