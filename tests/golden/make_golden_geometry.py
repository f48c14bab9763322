#!/usr/bin/env python3
"""Regenerates the pair-geometry fixtures in this directory (pairs placed at the template-length limit, in every orientation, on
neighbouring sequences and beside copies of a locus, tests/geometry_lib.py) with the UNMODIFIED reference binary (oracle/_ref/urmap,
built by oracle/Makefile):

  geometry.fa             nine sequences of random ACGT (geometry_lib.store)
  geometry_1/2.fq.gz      geometry_lib.cases: every pair of the list
  geometry.sam.gz         reference `urmap -map2 geometry_1.fq -reverse geometry_2.fq -ufi geometry.ufi -samout ... -tabbedout ...
                          -threads 1`, the @PG line dropped
  geometry.tab.gz         the -tabbedout file of the same run (SetSAM2 has cleared overhanging top hits before the line is written)
  geometry_nosam.tab.gz   reference `urmap -map2 ... -tabbedout ... -threads 1` without -samout

The index: reference `urmap -make_ufi geometry.fa -output geometry.ufi -slots 524309` (W = 24, MaxIx = 32); it is not kept, the tests
build it with the oracle.  The digests of the three outputs also go into ref_runs.json (key geometry_golden), so that a checkout with
the reference binary built runs it afresh against the same record.

Run only where the reference binary has been built; the fixtures are data, the reference itself does not travel.
"""
import gzip
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edges_lib as el  # noqa: E402
import geometry_lib as gl  # noqa: E402
import oracle_lib as ol  # noqa: E402
from urmap_amd import synth  # noqa: E402


def _gz(dst, data):
    with open(dst, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as z:
        z.write(data)


def run_reference(d, fa, f1, f2):
    """the three outputs of the reference binary for the pairs in f1 / f2 on the store in fa (paths inside d) -> {name: bytes}"""
    ol.run_ref(["-make_ufi", fa, "-output", "geometry.ufi", "-slots", str(el.SLOTS)], cwd=d)
    ol.run_ref(["-map2", f1, "-reverse", f2, "-ufi", "geometry.ufi", "-samout", "ref.sam", "-tabbedout", "ref.tab", "-threads", "1"], cwd=d)
    ol.run_ref(["-map2", f1, "-reverse", f2, "-ufi", "geometry.ufi", "-tabbedout", "ref_nosam.tab", "-threads", "1"], cwd=d)
    return {"sam": b"\n".join(ol.sam_records(os.path.join(d, "ref.sam"))) + b"\n", "tab": open(os.path.join(d, "ref.tab"), "rb").read(),
            "nosam_tab": open(os.path.join(d, "ref_nosam.tab"), "rb").read()}


def main():
    if not ol.have_ref():
        sys.exit(f"{ol.REF_BIN} is not built (oracle/Makefile)")
    with tempfile.TemporaryDirectory() as d:
        st, reads, tags = gl.cases()
        synth.write_fasta(os.path.join(HERE, "geometry.fa"), st)
        synth.write_fasta(os.path.join(d, "geometry.fa"), st)
        pairs = el.strip_mate_suffix(reads)
        synth.write_fastq(os.path.join(d, "geometry_1.fq"), pairs[0::2])
        synth.write_fastq(os.path.join(d, "geometry_2.fq"), pairs[1::2])
        out = run_reference(d, "geometry.fa", "geometry_1.fq", "geometry_2.fq")
        for suf in ("_1.fq", "_2.fq"):
            _gz(os.path.join(HERE, "geometry" + suf + ".gz"), open(os.path.join(d, "geometry" + suf), "rb").read())
        _gz(os.path.join(HERE, "geometry.sam.gz"), out["sam"])
        _gz(os.path.join(HERE, "geometry.tab.gz"), out["tab"])
        _gz(os.path.join(HERE, "geometry_nosam.tab.gz"), out["nosam_tab"])
        os.environ["URMAP_RECORD_REF_RUNS"] = "1"
        ol.reference_outputs("geometry_golden", lambda: dict(out, pairs=len(tags)))
        print(f"{len(tags)} pairs")
        for n in sorted(os.listdir(HERE)):
            if n.startswith("geometry"):
                print(n, os.path.getsize(os.path.join(HERE, n)))


if __name__ == "__main__":
    main()
