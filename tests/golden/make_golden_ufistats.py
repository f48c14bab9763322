#!/usr/bin/env python3
"""Regenerates ufi_stats.json, the index-statistics fixtures (-ufi_stats, -ufi_counts, -ufi_info), with the UNMODIFIED reference binary
(oracle/_ref/urmap, built by oracle/Makefile).  Tables:

  g, r          the golden g.ufi.gz / r.ufi.gz
  veryfast      -make_ufi g.fa -veryfast
  lf09          -make_ufi g.fa -load_factor 0.9      (long links)
  s40009        -make_ufi g.fa -slots 40009          (long links, rows cut at MaxIx, words that are not indexed)
  sat           -make_ufi sat.fa: g.fa plus a sequence of 600 A, GATTACA x 30 and CA x 400 (slots whose count saturates at 255)

Per table: the build options (None: a golden file), the .ufi's sha256, the report lines of `-ufi_stats X -log F` verbatim (the histogram
rows, then the block from the blank line before "Word length" through the blank line after "Total"; the log's own header and
progress lines are not kept), the lines `-ufi_info X` prints, and sha256 and bincount of the `-ufi_counts X -output F` file.

Run only where the reference binary has been built; the fixtures are data, the reference itself does not travel.
"""
import gzip
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "urmap")

TABLES = [  # (name, FASTA or golden .ufi.gz, -make_ufi options or None)
    ("g", "g.ufi.gz", None),
    ("r", "r.ufi.gz", None),
    ("veryfast", "g.fa", ["-veryfast"]),
    ("lf09", "g.fa", ["-load_factor", "0.9"]),
    ("s40009", "g.fa", ["-slots", "40009"]),
    ("sat", "sat.fa", []),
]

SAT_EXTRA = "A" * 600 + "GATTACA" * 30 + "CA" * 400


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def write_sat_fasta(path):
    """g.fa plus the saturation sequence (deterministic: no seed)"""
    with open(path, "w") as f:
        f.write(open(os.path.join(HERE, "g.fa")).read())
        f.write(">sat\n" + "\n".join(SAT_EXTRA[i:i + 80] for i in range(0, len(SAT_EXTRA), 80)) + "\n")


def report_lines(log_text):
    """the histogram rows and the summary block of a -ufi_stats log, verbatim"""
    lines = log_text.split("\n")
    hist = [l for l in lines if re.match(r"^\[\s*\d+\]  ", l)]
    i = next(k for k, l in enumerate(lines) if l.endswith("  Word length"))
    j = next(k for k, l in enumerate(lines) if l.endswith("  Total"))
    assert lines[i - 1] == "" and lines[j + 1] == ""
    return hist + lines[i - 1:j + 2]


def run(args, cwd):
    return subprocess.run([REF] + args, cwd=cwd, check=True, capture_output=True, text=True)


def main():
    if not os.path.exists(REF):
        sys.exit(f"{REF} not built (make -C oracle ref)")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(os.path.join(HERE, "g.fa"), d)
        write_sat_fasta(os.path.join(d, "sat.fa"))
        for name, src, opts in TABLES:
            ufi = os.path.join(d, name + ".ufi")
            if opts is None:
                with gzip.open(os.path.join(HERE, src), "rb") as z, open(ufi, "wb") as f:
                    f.write(z.read())
            else:
                run(["-make_ufi", src, "-output", ufi] + opts, d)
            log = os.path.join(d, name + ".log")
            run(["-ufi_stats", ufi, "-log", log], d)
            counts = os.path.join(d, name + ".counts")
            run(["-ufi_counts", ufi, "-output", counts], d)
            info = run(["-ufi_info", ufi, "-log", os.path.join(d, name + ".info.log")], d)
            info_lines = [l for l in open(os.path.join(d, name + ".info.log")).read().split("\n")
                          if l.startswith((" Word length", "       MaxIx", "     SeqData", "       Slots"))]
            assert len(info_lines) == 4, info.stderr
            c = np.fromfile(counts, dtype=np.uint8)
            bc = np.bincount(c, minlength=256)
            out[name] = {
                "source": src,
                "options": opts,
                "sha256": sha(ufi),
                "report": report_lines(open(log).read()),
                "info": info_lines,
                "counts_sha256": sha(counts),
                "counts_bincount": {str(k): int(v) for k, v in enumerate(bc) if v},
            }
    with open(os.path.join(HERE, "ufi_stats.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
