#!/usr/bin/env python3
"""Regenerates the golden fixtures in this directory with the UNMODIFIED reference binary
(oracle/_ref/urmap, built by oracle/Makefile from /root/reference/src).  Inputs are seeded synthetic data;
outputs are what the reference itself wrote:

  g.fa            40 kbp, 3 sequences, repeats, N runs, soft-masked stretches
  g.ufi.gz        reference `urmap -make_ufi g.fa -output g.ufi` (default W=24, MaxIx=32, table prime)
  se150.fq/.sam   400 reads, 150 bp, 1 % sub, 0.2 % indel, N / lower-case / IUPAC edge cases
  se250.fq/.sam   200 reads, 250 bp, 4 % sub, 1 % indel
  se_short.fq/.sam 100 reads of 24..60 bp
  reference `urmap -map X.fq -ufi g.ufi -samout X.sam -threads 1`; the @PG line is dropped.
  pe150_1/2.fq, pe100_noisy_1/2.fq + .sam + .tab   300 pairs each, reference `urmap -map2 A_1.fq -reverse A_2.fq ...
                                                   -samout A.sam -tabbedout A.tab`
  se_alpha.fq/.sam, pe_alpha_1/2.fq + .sam + .tab, each .gz   560 reads / 300 pairs of 150 bp in the letter classes of tests/alphabet_lib.py (N at
                  the ends and in runs, lower case, IUPAC, U / u, letters without a complement, reads that keep the store's N), the
                  classes of the two mates drawn independently; python make_golden.py alpha regenerates only these
  edges.fa, edges_rescue.fa, edges_se.fq/.sam, edges_pe_1/2.fq + .sam, the read files .gz   reads and pairs at the first and last bases of sequences
                  and of the sequence store (tests/edges_lib.py): written by make_golden_edges.py, not by this script
  geometry.fa, geometry_1/2.fq + .sam + .tab + _nosam.tab, all but the FASTA .gz   pairs at the template-length limit, in every orientation, on
                  neighbouring sequences and beside copies of a locus (tests/geometry_lib.py): written by make_golden_geometry.py
  r.fa, r.ufi.gz, pe120_rep_*               repeat-rich second genome: pairs with a second-best pair (see make_repeat_set)

  ufi_opts.json   sha256 / slot count / labels of the reference's .ufi for -make_ufi option sets (-load_factor, -veryfast,
                  -notrunclabels); python make_golden.py ufiopts regenerates only this file

  hitstats.json   the count lines of the reference's end-of-run report (State1::HitStats, state1.cpp:593-632) for the
                  sets above, incl. -minq 3 runs (python make_golden.py hitstats regenerates only this file)

  ref_runs.json   sha256 of the .ufi / SAM files the reference wrote in the tests that run it on seeded inputs of their own
                  (*_equals_reference_binary), keyed by test case; the tests compare against it when the binary is not built.
                  Written by those tests: URMAP_RECORD_REF_RUNS=1 pytest tests -k equals_reference_binary

Run only where /root/reference exists; the fixtures are data, the reference itself does not travel.
"""
import gzip
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol  # noqa: E402
from urmap_amd import synth  # noqa: E402


def edge(reads, seed):
    rng = np.random.default_rng(seed)
    out = list(reads)
    for k in range(0, len(out), 13):
        lab, s, q = out[k]
        s = s.copy(); s[int(rng.integers(0, len(s)))] = ord("N"); out[k] = (lab, s, q)
    for k in range(4, len(out), 41):
        lab, s, q = out[k]; out[k] = (lab, s | 0x20, q)
    for k in range(7, len(out), 53):
        lab, s, q = out[k]
        s = s.copy(); s[int(rng.integers(0, len(s)))] = ord("R"); out[k] = (lab + " extra words/1", s, q)
    return out


def make_repeat_set(tmp):
    """A second, repeat-rich genome (near-identical family copies) so that FindPairs sees several pairs per read pair:
    the -tabbedout lines then carry a second pair and the TL/Score info string (outputtab2.cpp:6-27,98-102).
    r.fa, r.ufi.gz, pe120_rep_1/2.fq, pe120_rep.sam (with -samout), pe120_rep.tab, pe120_rep_nosam.tab (without)."""
    g = synth.make_genome(77, [30000, 30000], repeat_frac=0.6, n_families=4, max_div=0.03, label_prefix="rep")
    synth.write_fasta(os.path.join(HERE, "r.fa"), g)
    shutil.copy(os.path.join(HERE, "r.fa"), os.path.join(tmp, "r.fa"))
    ol.run_ref(["-make_ufi", "r.fa", "-output", "r.ufi", "-slots", "100003"], cwd=tmp)
    with open(os.path.join(tmp, "r.ufi"), "rb") as f, gzip.GzipFile(os.path.join(HERE, "r.ufi.gz"), "wb", mtime=0) as z:
        z.write(f.read())
    r1, r2 = synth.make_pairs(5, g, 400, read_len=120, sub1=0.02, sub2=0.04)
    name = "pe120_rep"
    synth.write_fastq(os.path.join(HERE, name + "_1.fq"), r1)
    synth.write_fastq(os.path.join(HERE, name + "_2.fq"), r2)
    for suf in ("_1.fq", "_2.fq"):
        shutil.copy(os.path.join(HERE, name + suf), os.path.join(tmp, name + suf))
    ol.run_ref(["-map2", name + "_1.fq", "-reverse", name + "_2.fq", "-ufi", "r.ufi", "-samout", name + ".sam",
                "-tabbedout", name + ".tab", "-threads", "1"], cwd=tmp)
    with open(os.path.join(HERE, name + ".sam"), "wb") as f:
        f.write(b"\n".join(ol.sam_records(os.path.join(tmp, name + ".sam"))) + b"\n")
    shutil.copy(os.path.join(tmp, name + ".tab"), os.path.join(HERE, name + ".tab"))
    ol.run_ref(["-map2", name + "_1.fq", "-reverse", name + "_2.fq", "-ufi", "r.ufi", "-tabbedout", name + "_nosam.tab",
                "-threads", "1"], cwd=tmp)
    shutil.copy(os.path.join(tmp, name + "_nosam.tab"), os.path.join(HERE, name + "_nosam.tab"))


def _gz(src, dst, data=None):
    """fixture kept gzip-compressed (mtime 0: the same bytes every time); the tests unpack it"""
    if data is None:
        with open(src, "rb") as f:
            data = f.read()
    with open(dst, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as z:
        z.write(data)


def make_alpha(tmp):
    """se_alpha / pe_alpha: the letter classes of tests/alphabet_lib.py against the existing g.ufi, `-threads 1`; every file .gz"""
    import alphabet_lib as al
    with gzip.open(os.path.join(HERE, "g.ufi.gz"), "rb") as z, open(os.path.join(tmp, "g.ufi"), "wb") as f:
        f.write(z.read())
    store = al.Store(ol.Index.load(os.path.join(tmp, "g.ufi")), os.path.join(HERE, "g.fa"))
    reads, _ = al.make_reads(31, store, 560, read_len=150)
    synth.write_fastq(os.path.join(tmp, "se_alpha.fq"), reads)
    _gz(os.path.join(tmp, "se_alpha.fq"), os.path.join(HERE, "se_alpha.fq.gz"))
    ol.run_ref(["-map", "se_alpha.fq", "-ufi", "g.ufi", "-samout", "se_alpha.sam", "-threads", "1"], cwd=tmp)
    _gz(None, os.path.join(HERE, "se_alpha.sam.gz"), b"\n".join(ol.sam_records(os.path.join(tmp, "se_alpha.sam"))) + b"\n")
    r1, r2, _, _ = al.make_pairs(32, store, 300, read_len=150)
    name = "pe_alpha"
    synth.write_fastq(os.path.join(tmp, name + "_1.fq"), r1)
    synth.write_fastq(os.path.join(tmp, name + "_2.fq"), r2)
    for suf in ("_1.fq", "_2.fq"):
        _gz(os.path.join(tmp, name + suf), os.path.join(HERE, name + suf + ".gz"))
    ol.run_ref(["-map2", name + "_1.fq", "-reverse", name + "_2.fq", "-ufi", "g.ufi", "-samout", name + ".sam",
                "-tabbedout", name + ".tab", "-threads", "1"], cwd=tmp)
    _gz(None, os.path.join(HERE, name + ".sam.gz"), b"\n".join(ol.sam_records(os.path.join(tmp, name + ".sam"))) + b"\n")
    _gz(os.path.join(tmp, name + ".tab"), os.path.join(HERE, name + ".tab.gz"))


HITSTATS_CASES = [  # (key, mode, read set, index, extra options)
    ("se150", "map", "se150", "g", []), ("se250", "map", "se250", "g", []), ("se_short", "map", "se_short", "g", []),
    ("se150_minq3", "map", "se150", "g", ["-minq", "3"]),
    ("pe150", "map2", "pe150", "g", []), ("pe100_noisy", "map2", "pe100_noisy", "g", []),
    ("pe100_noisy_minq3", "map2", "pe100_noisy", "g", ["-minq", "3"]),
    ("pe120_rep_minq25", "map2", "pe120_rep", "r", ["-minq", "25"]),
]


def hitstats_lines(stderr_text):
    """The four count lines of the report; the timing lines are not comparable."""
    keep = ("  Reads (", "  Mapped Q>=", "  Mapped Q< ", "  Unmapped (", "WARNING: Option -minq")
    return [ln for ln in stderr_text.replace("\r", "\n").split("\n") if any(k in ln for k in keep)]


def make_hitstats(tmp):
    import json
    for g in ("g", "r"):
        with gzip.open(os.path.join(HERE, g + ".ufi.gz"), "rb") as z, open(os.path.join(tmp, g + ".ufi"), "wb") as f:
            f.write(z.read())
    out = {}
    for key, mode, name, g, extra in HITSTATS_CASES:
        if mode == "map":
            shutil.copy(os.path.join(HERE, name + ".fq"), os.path.join(tmp, name + ".fq"))
            args = ["-map", name + ".fq"]
        else:
            for suf in ("_1.fq", "_2.fq"):
                shutil.copy(os.path.join(HERE, name + suf), os.path.join(tmp, name + suf))
            args = ["-map2", name + "_1.fq", "-reverse", name + "_2.fq"]
        r = ol.run_ref(args + ["-ufi", g + ".ufi", "-samout", "hs.sam", "-threads", "1"] + extra, cwd=tmp)
        out[key] = hitstats_lines(r.stderr.decode())
    with open(os.path.join(HERE, "hitstats.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


UFI_OPT_CASES = [  # (key, FASTA, options): -make_ufi options beyond -slots (ufindexio.cpp:117-150)
    ("load_factor_0.3", "g.fa", ["-load_factor", "0.3"]),
    ("load_factor_0.9_veryfast", "g.fa", ["-load_factor", "0.9", "-veryfast"]),
    ("notrunclabels", "g.fa", ["-notrunclabels", "-slots", "100003"]),
    ("trunclabels_default", "g.fa", ["-slots", "100003"]),
]


def make_ufi_opts(tmp):
    """ufi_opts.json: for each option set, the sha256 of the .ufi the reference wrote, its slot count and its labels."""
    import hashlib
    import json
    out = {}
    shutil.copy(os.path.join(HERE, "g.fa"), os.path.join(tmp, "g.fa"))
    for key, fa, opts in UFI_OPT_CASES:
        ol.run_ref(["-make_ufi", fa, "-output", "o.ufi"] + opts, cwd=tmp)
        p = os.path.join(tmp, "o.ufi")
        w, maxix, sds, slots = ol.ufi_header(p)
        idx = ol.Index.load(p)
        out[key] = {"options": opts, "sha256": hashlib.sha256(open(p, "rb").read()).hexdigest(), "slots": int(slots), "max_ix": int(maxix),
                    "labels": [d[0] for d in idx.directory()]}
    with open(os.path.join(HERE, "ufi_opts.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    assert ol.have_ref(), "build oracle/_ref/urmap first (make -C oracle ref)"
    tmp = os.path.join(HERE, "_tmp")
    os.makedirs(tmp, exist_ok=True)
    g = synth.make_genome(424242, [22000, 13000, 5000], repeat_frac=0.35, n_families=6, n_run_frac=0.02)
    synth.write_fasta(os.path.join(HERE, "g.fa"), g, lowercase_frac=0.05, seed=3)
    shutil.copy(os.path.join(HERE, "g.fa"), os.path.join(tmp, "g.fa"))
    ol.run_ref(["-make_ufi", "g.fa", "-output", "g.ufi"], cwd=tmp)
    with open(os.path.join(tmp, "g.ufi"), "rb") as f, gzip.GzipFile(os.path.join(HERE, "g.ufi.gz"), "wb", mtime=0) as z:
        z.write(f.read())
    sets = {
        "se150": edge(synth.make_reads(11, g, 400, read_len=150, sub=0.01, ins=0.001, dele=0.001, random_frac=0.03), 1),
        "se250": edge(synth.make_reads(12, g, 200, read_len=250, sub=0.04, ins=0.005, dele=0.005, random_frac=0.03), 2),
    }
    short = []
    for i, L in enumerate(range(24, 61)):
        short += synth.make_reads(100 + i, g, 3, read_len=L, sub=0.01, ins=0, dele=0, label_prefix=f"s{L}_")
    sets["se_short"] = short[:100]
    for name, reads in sets.items():
        fq = os.path.join(HERE, name + ".fq")
        synth.write_fastq(fq, reads)
        shutil.copy(fq, os.path.join(tmp, name + ".fq"))
        ol.run_ref(["-map", name + ".fq", "-ufi", "g.ufi", "-samout", name + ".sam", "-threads", "1"], cwd=tmp)
        with open(os.path.join(HERE, name + ".sam"), "wb") as f:
            f.write(b"\n".join(ol.sam_records(os.path.join(tmp, name + ".sam"))) + b"\n")
    # paired-end: urmap -map2 R1 -reverse R2 (map2.cpp:39-90)
    pe_sets = {
        "pe150": synth.make_pairs(21, g, 300, read_len=150, sub1=0.01, sub2=0.02, ins=0.001, dele=0.001),
        "pe100_noisy": synth.make_pairs(22, g, 300, read_len=100, sub1=0.04, sub2=0.08, ins=0.01, dele=0.01),
    }
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for name, (r1, r2) in pe_sets.items():
        for k in range(5, len(r1), 37):  # one mate replaced by random sequence: rescue scan / unpaired output
            lab, s, q = r2[k]
            r2[k] = (lab, acgt[rng.integers(0, 4, size=len(s))], q)
        for k in range(9, len(r1), 97):
            lab, s, q = r1[k]
            s = s.copy(); s[int(rng.integers(0, len(s)))] = ord("N"); r1[k] = (lab, s, q)
        synth.write_fastq(os.path.join(HERE, name + "_1.fq"), r1)
        synth.write_fastq(os.path.join(HERE, name + "_2.fq"), r2)
        for suf in ("_1.fq", "_2.fq"):
            shutil.copy(os.path.join(HERE, name + suf), os.path.join(tmp, name + suf))
        ol.run_ref(["-map2", name + "_1.fq", "-reverse", name + "_2.fq", "-ufi", "g.ufi", "-samout", name + ".sam",
                    "-tabbedout", name + ".tab", "-threads", "1"], cwd=tmp)
        with open(os.path.join(HERE, name + ".sam"), "wb") as f:
            f.write(b"\n".join(ol.sam_records(os.path.join(tmp, name + ".sam"))) + b"\n")
        shutil.copy(os.path.join(tmp, name + ".tab"), os.path.join(HERE, name + ".tab"))
    make_alpha(tmp)
    make_repeat_set(tmp)
    make_hitstats(tmp)
    make_ufi_opts(tmp)
    shutil.rmtree(tmp)
    print("golden fixtures written to", HERE)


if __name__ == "__main__":
    if sys.argv[1:] == ["hitstats"]:
        _tmp = os.path.join(HERE, "_tmp")
        os.makedirs(_tmp, exist_ok=True)
        make_hitstats(_tmp)
        shutil.rmtree(_tmp)
    elif sys.argv[1:] == ["alpha"]:
        _tmp = os.path.join(HERE, "_tmp")
        os.makedirs(_tmp, exist_ok=True)
        make_alpha(_tmp)
        shutil.rmtree(_tmp)
    elif sys.argv[1:] == ["ufiopts"]:
        _tmp = os.path.join(HERE, "_tmp")
        os.makedirs(_tmp, exist_ok=True)
        make_ufi_opts(_tmp)
        shutil.rmtree(_tmp)
    else:
        main()
