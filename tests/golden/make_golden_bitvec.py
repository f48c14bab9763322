#!/usr/bin/env python3
"""Regenerates the k-mer bit-vector fixtures in this directory (-make_bitvec, -search_bitvec, -search_bitvec2) with the UNMODIFIED
reference binary (oracle/_ref/urmap, built by oracle/Makefile).  Inputs are seeded synthetic data:

  bv_ref.fa        3 sequences, 6 kbp: N runs, soft-masked (lower-case) stretches, 'u' / 'U', IUPAC letters, one sequence shorter
                   than 2W-1 at W = 16 (none shorter than W-1: the reference's loop bound wraps there)
  bv_excl.fa       2 sequences: stretches copied from bv_ref.fa (so the exclusion pass clears words) and random bases
  bv_r1.fq         reads drawn from bv_ref.fa in both orientations, reads of 2W-2, 2W-1 and 2W bases for W = 8, 12, 16, reads whose
                   only genomic bases are their last ones, random reads, labels with blanks
  bv_r2.fq         the mates: as many records as bv_r1.fq
  bitvec_runs.json per W in (8, 12, 16): sha256 of the reference's .bv and its included / excluded counts; per W in (8, 12): sha256
                   and found counts of `-search_bitvec bv_r1.fq` and `-search_bitvec2 bv_r1.fq -reverse bv_r2.fq`, with and without
                   -trunclabels, all at -threads 1

Run only where the reference binary has been built; the fixtures are data, the reference itself does not travel.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "urmap")
MAKE_W = (8, 12, 16)
SEARCH_W = (8, 12)


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def rc_chars(s):
    comp = dict(zip("ACGTUNRYSWKMBDHVacgtnryswkmbdhv", "TGCAANYRSWMKVHDBtgcanyrswmkvhdb"))
    return "".join(comp.get(c, "?") for c in reversed(s))


def make_inputs(d):
    rng = np.random.default_rng(20261015)
    rand = lambda n: "".join(rng.choice(list("ACGT"), n))
    g1 = list(rand(4000))
    for a in (500, 1800, 3100):  # N runs
        g1[a:a + 30] = "N" * 30
    for a in (900, 2600):  # soft-masked stretches
        g1[a:a + 200] = [c.lower() for c in g1[a:a + 200]]
    for a in range(100, 4000, 97):  # 'U' (a letter on both strands) and 'u' (no complement letter)
        g1[a] = "U" if (a // 97) % 2 else "u"
    for a, c in zip(range(1300, 1400, 9), "RYSWKMBDHVX"):
        g1[a] = c
    g1 = "".join(g1)
    g2 = rand(2000)
    g3 = rand(25)  # shorter than 2W-1 at W = 16
    with open(os.path.join(d, "bv_ref.fa"), "w") as f:
        f.write(">chr1 first sequence\n" + "\n".join(g1[i:i + 70] for i in range(0, len(g1), 70)) + "\n")
        f.write(">chr2\n" + g2 + "\n>tiny\n" + g3 + "\n")
    with open(os.path.join(d, "bv_excl.fa"), "w") as f:
        f.write(">x1\n" + g1[2000:2300] + rand(100) + "\n>x2 copy\n" + g2[100:400].lower() + "\n")
    reads = []

    def add(label, s):
        reads.append((label, s))

    for i in range(60):  # from the genome, both orientations, mixed lengths
        L = int(rng.choice([20, 40, 75, 150]))
        src = g1 if i % 2 else g2
        a = int(rng.integers(0, len(src) - L))
        s = src[a:a + L]
        s = "".join(c if c.isalpha() and c.upper() in "ACGTUN" else "N" for c in s)
        add(f"g{i} pos={a} len={L}", s if i % 3 else rc_chars(s).replace("?", "N"))
    for W in MAKE_W:  # 2W-2, 2W-1, 2W bases from chr2
        for L in (2 * W - 2, 2 * W - 1, 2 * W):
            a = int(rng.integers(0, len(g2) - L))
            add(f"edge W={W} L={L}", g2[a:a + L])
            add(f"edgerc W={W} L={L}", rc_chars(g2[a:a + L]))
    for W in MAKE_W:  # only the last (first) 20 bases genomic
        a = int(rng.integers(0, len(g2) - 20))
        add(f"tail W={W}", rand(30) + g2[a:a + 20])
        add(f"head W={W}", g2[a:a + 20] + rand(30))
    for i in range(20):
        add(f"rand{i}\tblank", rand(int(rng.integers(12, 120))))  # none shorter than W-1 at the searched W
    add("lower", g2[500:580].lower())
    add("withu", g2[600:650].replace("T", "u"))
    add("withU", g2[700:750].replace("T", "U"))
    qual = lambda n: "".join(chr(33 + int(x)) for x in rng.integers(2, 41, n))
    with open(os.path.join(d, "bv_r1.fq"), "w") as f:
        for lab, s in reads:
            f.write(f"@{lab}\n{s}\n+\n{qual(len(s))}\n")
    with open(os.path.join(d, "bv_r2.fq"), "w") as f:  # mate 2: random for most, genomic for some
        for i, (lab, _) in enumerate(reads):
            L = int(rng.integers(30, 100))
            s = rand(L) if i % 4 else rc_chars(g1[1000 + i:1000 + i + L]).replace("?", "N")
            f.write(f"@{lab.split()[0]}/2 mate\n{s}\n+\n{qual(L)}\n")


def run(args):
    r = subprocess.run([REF] + args + ["-threads", "1"], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr)
    return r.stderr


def main():
    if not os.path.exists(REF):
        sys.exit(f"{REF} is not built (oracle/Makefile)")
    make_inputs(HERE)
    fa, ex, r1, r2 = (os.path.join(HERE, n) for n in ("bv_ref.fa", "bv_excl.fa", "bv_r1.fq", "bv_r2.fq"))
    out = {"make": {}, "search": {}, "search2": {}}
    with tempfile.TemporaryDirectory() as d:
        for W in MAKE_W:
            bv = os.path.join(d, f"w{W}.bv")
            msg = run(["-make_bitvec", fa, "-input2", ex, "-wordlength", str(W), "-output", bv])
            inc = int(re.search(r"(\d+) words included", msg).group(1))
            exc = int(re.search(r"(\d+) words excluded", msg).group(1))
            out["make"][str(W)] = {"sha256": sha(bv), "bytes": os.path.getsize(bv), "included": inc, "excluded": exc}
            if W not in SEARCH_W:
                continue
            for trunc in (False, True):
                key = f"{W}{'_trunc' if trunc else ''}"
                t = ["-trunclabels"] if trunc else []
                h = os.path.join(d, "h.fq")
                msg = run(["-search_bitvec", r1, "-ref", bv, "-output", h] + t)
                m = re.search(r"(\d+) / (\d+) found", msg)
                out["search"][key] = {"sha256": sha(h), "found": int(m.group(1)), "reads": int(m.group(2))}
                h1, h2 = os.path.join(d, "h1.fq"), os.path.join(d, "h2.fq")
                msg = run(["-search_bitvec2", r1, "-reverse", r2, "-ref", bv, "-output1", h1, "-output2", h2] + t)
                m = re.search(r"(\d+) / (\d+) found", msg)
                out["search2"][key] = {"sha256_1": sha(h1), "sha256_2": sha(h2), "found": int(m.group(1)), "pairs": int(m.group(2))}
    with open(os.path.join(HERE, "bitvec_runs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
