"""The yardstick of the pileup (-vcfout): a model in numpy and struct written from the "Pileup" text of include/urmapx.h and sharing
nothing with the product, and a parser of the VCF text that checks its syntax on the way.

    model(records, names, lens, seqs, opts, command)   the text the rule asks for
    counts(records, lens, opts)                        the four counters of every column, (columns, 4), and the records that counted
    parse(text)                                        {"command", "contigs", "sites"}; raises AssertionError on any line out of form
    DEFAULTS                                           min_mapq 0, min_baseq 13, min_alt 3, min_pct 10

The records are built with stats_lib.rec, which sets every field the rule reads.
"""
import struct

import numpy as np

from stats_lib import split

DEFAULTS = {"min_mapq": 0, "min_baseq": 13, "min_alt": 3, "min_pct": 10}
LETTERS = "ACGT"
CODE_TO_BASE = np.full(16, -1, dtype=np.int64)
CODE_TO_BASE[[1, 2, 4, 8]] = [0, 1, 2, 3]
HEADER_TAIL = ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Bases counted on the column">',
               '##INFO=<ID=AD,Number=R,Type=Integer,Description="Bases counted per allele, the reference\'s first">',
               "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]


def rule(opts):
    full = dict(DEFAULTS)
    full.update(opts or {})
    return full


def counts(records, lens, opts=None, flags=None):
    """rules 1 and 2 -> (the counters, one row of A C G T per column of all references end to end; the records that counted).
    flags: the flag of every record where it shall not be the record's own"""
    R = rule(opts)
    first = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
    cnt = np.zeros((int(first[-1]), 4), dtype=np.int64)
    counted = 0
    for k, r in enumerate(split(bytes(records))):
        size, ref, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<IiiBBHHHI", r, 0)
        if flags is not None:
            flag = flags[k]
        if ref < 0 or ref >= len(lens) or pos < 0 or flag & 0x704 or mapq < R["min_mapq"]:
            continue
        counted += 1
        at = 36 + l_name
        if at + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > len(r):
            continue
        ops = struct.unpack_from("<%dI" % n_cigar, r, at)
        at += 4 * n_cigar
        packed = np.frombuffer(r, dtype=np.uint8, count=(l_seq + 1) // 2, offset=at)
        codes = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq]
        qual = np.frombuffer(r, dtype=np.uint8, count=l_seq, offset=at + (l_seq + 1) // 2)
        passes = np.ones(l_seq, dtype=bool) if l_seq and qual[0] == 0xFF else qual >= R["min_baseq"]
        base = CODE_TO_BASE[codes]
        x, q = pos, 0
        for w in ops:
            op, length = w & 15, w >> 4
            if op in (0, 7, 8):
                m = max(0, min(length, lens[ref] - x, l_seq - q))
                if m:
                    b, ok = base[q:q + m], passes[q:q + m] & (base[q:q + m] >= 0)
                    np.add.at(cnt, (first[ref] + x + np.nonzero(ok)[0], b[ok]), 1)
                x += length
                q += length
            elif op in (1, 4):
                q += length
            elif op in (2, 3):
                x += length
    return cnt, counted


def text_of(cnt, names, lens, seqs, opts=None, command=b""):
    """rules 3 and 4 on the counters"""
    R = rule(opts)
    names = [n.decode("latin-1") if isinstance(n, bytes) else n for n in names]
    lines = ["##fileformat=VCFv4.2", "##source=urmap", "##urmapCommand=" + (command.decode("latin-1") if isinstance(command, bytes) else command)]
    lines += ["##contig=<ID=%s,length=%d>" % (n, l) for n, l in zip(names, lens)] + HEADER_TAIL
    at = 0
    for name, l_ref, seq in zip(names, lens, seqs):
        c = cnt[at:at + l_ref]
        at += l_ref
        if not l_ref:
            continue
        letters = np.frombuffer(bytes(seq).upper(), dtype=np.uint8)
        assert len(letters) == l_ref
        ref = np.full(l_ref, -1, dtype=np.int64)
        for b, ch in enumerate(LETTERS):
            ref[letters == ord(ch)] = b
        dp = c.sum(axis=1)
        alt = (c >= R["min_alt"]) & (c * 100 >= R["min_pct"] * dp[:, None]) & (np.arange(4)[None, :] != ref[:, None]) & (ref >= 0)[:, None]
        for x in np.nonzero(alt.any(axis=1))[0]:
            alleles = sorted(np.nonzero(alt[x])[0], key=lambda b: (-int(c[x, b]), b))
            lines.append("%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AD=%s" % (name, x + 1, LETTERS[ref[x]], ",".join(LETTERS[b] for b in alleles), dp[x],
                                                                  ",".join(str(int(c[x, b])) for b in [ref[x]] + alleles)))
    return ("\n".join(lines) + "\n").encode("latin-1")


def model(records, names, lens, seqs, opts=None, command=b"", flags=None):
    return text_of(counts(records, lens, opts, flags)[0], names, lens, seqs, opts, command)


def parse(text):
    """the VCF text -> {"command": str, "contigs": [(name, length)], "sites": [(chrom, pos (1-based), ref, [alt], dp, [ad])]}; every
    line is checked against rule 4's form"""
    assert text.endswith(b"\n")
    lines = text.decode("latin-1").split("\n")[:-1]
    assert lines[:2] == ["##fileformat=VCFv4.2", "##source=urmap"] and lines[2].startswith("##urmapCommand=")
    out = {"command": lines[2][len("##urmapCommand="):], "contigs": [], "sites": []}
    k = 3
    while lines[k].startswith("##contig=<ID="):
        body = lines[k][len("##contig=<ID="):]
        assert body.endswith(">") and ",length=" in body
        name, length = body[:-1].rsplit(",length=", 1)
        out["contigs"].append((name, int(length)))
        k += 1
    assert lines[k:k + 3] == HEADER_TAIL
    order = {n: i for i, (n, _) in enumerate(out["contigs"])}
    last = (-1, 0)
    for line in lines[k + 3:]:
        f = line.split("\t")
        assert len(f) == 8 and f[2] == f[5] == f[6] == "." and f[3] in LETTERS and len(f[3]) == 1, line
        alts = f[4].split(",")
        assert 1 <= len(alts) <= 3 and all(a in LETTERS and len(a) == 1 and a != f[3] for a in alts) and len(set(alts)) == len(alts), line
        info = dict(kv.split("=") for kv in f[7].split(";"))
        assert list(info) == ["DP", "AD"], line
        ad = [int(v) for v in info["AD"].split(",")]
        pos, dp = int(f[1]), int(info["DP"])
        assert str(pos) == f[1] and len(ad) == 1 + len(alts) and sum(ad) <= dp and 1 <= pos <= out["contigs"][order[f[0]]][1], line
        assert all(ad[i] > ad[i + 1] or (ad[i] == ad[i + 1] and LETTERS.index(alts[i - 1]) < LETTERS.index(alts[i])) for i in range(1, len(alts))), line
        assert (order[f[0]], pos) > last, line
        last = (order[f[0]], pos)
        out["sites"].append((f[0], pos, f[3], alts, dp, ad))
    return out
