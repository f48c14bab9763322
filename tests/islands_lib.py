"""The "islands" fixture: genome-scale coordinates at the cost of a small genome (tests/test_bam_scale_cpu.py,
tests/test_gpu_bam_scale.py).  Reference `big` is 2^26 + 40 000 bases of N with islands of random ACGT around the first boundary of every
bin level of the BAI scheme -- 2^14, 2^17, 2^20, 2^23, 2^26 -- and at both ends; reference `small` puts a second refID and a sequence-store
offset above 2^26 into play.  Three islands more lie around the last boundary of the 2^14, 2^17 and 2^20 grids below 2^26, where a read
across the boundary lands in the LAST bin of the level above (585 + 511, 73 + 63, 9 + 7): at the first boundaries every bin of the
upper levels is the level's first, and a wrong shift in "first bin + (beg >> shift)" would not show.  Reads are drawn across every
boundary, so records, bins, linear windows, reference fetches and depth columns all see the coordinates of a human chromosome while the
index builds in seconds.  Nothing here is golden data: everything is a pure function of the seed.

    genome(seed)          [("big", uint8 array), ("small", uint8 array)]
    single_reads(g, seed) [Read]: where each was drawn from, and its FASTQ record
    pairs(g, seed)        [(Read, Read)]: FR pairs with the mates on either side of a boundary
    build(directory)      the FASTA, the .ufi, the FASTQ files, the oracle's index: what a module-scoped fixture holds
"""
import os
from collections import namedtuple

import numpy as np

EDGES = [1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26]
LAST_EDGES = [(1 << 26) - (1 << 20), (1 << 26) - (1 << 17), (1 << 26) - (1 << 14)]  # the last boundary below 2^26 that is no multiple of the next grid
BIG = (1 << 26) + 40000
SMALL = 30000
ISLAND = 2000          # bases around every boundary
END_ISLAND = 1500      # bases at either end of big
SLOTS = 100003
READ = 150
UNMAPPED = 0xFFFFFFFF

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b

# ref: 0 big, 1 small, None drawn from nowhere; pos: zero-based leftmost reference base; span: reference bases the alignment covers
Read = namedtuple("Read", "label seq qual ref pos plus span mutated")


def genome(seed=17):
    rng = np.random.default_rng(seed)
    big = np.full(BIG, ord("N"), dtype=np.uint8)
    big[:END_ISLAND] = ACGT[rng.integers(0, 4, END_ISLAND)]
    big[BIG - END_ISLAND:] = ACGT[rng.integers(0, 4, END_ISLAND)]
    for e in EDGES:  # in ascending order: an island overwrites what it overlaps of the ones before
        big[e - ISLAND // 2:e + ISLAND // 2] = ACGT[rng.integers(0, 4, ISLAND)]
    for e in LAST_EDGES:
        big[e - ISLAND // 2:e + ISLAND // 2] = ACGT[rng.integers(0, 4, ISLAND)]
    return [("big", big), ("small", ACGT[rng.integers(0, 4, SMALL)])]


def write_fasta(path, g, width=80):
    with open(path, "wb") as f:
        for name, seq in g:
            f.write(b">" + name.encode() + b"\n")
            whole = len(seq) // width * width
            rows = np.empty((whole // width, width + 1), dtype=np.uint8)
            rows[:, :width] = seq[:whole].reshape(-1, width)
            rows[:, width] = 10
            f.write(rows.tobytes())
            if whole < len(seq):
                f.write(seq[whole:].tobytes() + b"\n")


def _other(rng, c):
    return ACGT[(int(np.searchsorted(ACGT, c)) + 1 + int(rng.integers(0, 3))) % 4]


def draw(rng, g, ref, pos, plus, kind, label, qual=ord("I")):
    """a read of READ bases drawn from g[ref] at pos.  kind 0: as it stands; 1: two substitutions; 2: substitutions and an insertion of
    1-3 bases; 3: substitutions and a deletion of 1-3 bases.  Every change lies between columns 30 and 120, so the alignment begins at
    pos and covers `span` bases whatever the aligner makes of the change itself"""
    seq = g[ref][1]
    k = int(rng.integers(1, 4)) if kind >= 2 else 0
    span = READ - k if kind == 2 else READ + k
    assert 0 <= pos and pos + span <= len(seq), (label, pos, span)
    frag = seq[pos:pos + span].copy()
    assert ord("N") not in frag, (label, pos)
    if kind:
        for col in rng.choice(np.arange(30, 50), 2, replace=False):
            frag[col] = _other(rng, frag[col])
    if kind == 2:
        at = int(rng.integers(60, 80))
        ins = ACGT[rng.integers(0, 4, k)]
        ins[0] = _other(rng, frag[at])  # (the inserted run neither begins nor ends like its neighbours: its place is not ambiguous)
        ins[-1] = _other(rng, frag[at]) if k > 1 else ins[0]
        frag = np.concatenate([frag[:at], ins, frag[at:]])
    elif kind == 3:
        at = int(rng.integers(90, 110))
        frag = np.concatenate([frag[:at], frag[at + k:]])
    assert len(frag) == READ
    if not plus:
        frag = COMP[frag[::-1]]
    return Read(label, frag, np.full(READ, qual, np.uint8), ref, pos, plus, span, kind != 0)


def random_read(rng, label):
    return Read(label, ACGT[rng.integers(0, 4, READ)], np.full(READ, ord("I"), np.uint8), None, None, True, 0, True)


def single_reads(g, seed=23):
    """a few hundred single-end reads: starts swept across every boundary, reads that end exactly at it and begin exactly at it, the first
    and the last base of big, a few on small, exact duplicates, reads from nowhere"""
    rng = np.random.default_rng(seed)
    out = []

    def add(ref, pos, plus, kind, tag):
        out.append(draw(rng, g, ref, pos, plus, kind, f"s{len(out)}_{tag}_{pos}", qual=ord("I") - 7 * (len(out) % 3)))

    for e in EDGES:
        for n, start in enumerate(range(e - 160, e + 21, 7)):
            add(0, start, n % 2 == 0, n % 4, f"sweep{e}")
        for plus in (True, False):
            add(0, e - READ, plus, 0, f"ends{e}")      # the last base is e - 1: the bin stays on the child level
            add(0, e, plus, 0, f"begins{e}")
        add(0, e - READ + 1, True, 0, f"crosses{e}")   # one base beyond
    for e in LAST_EDGES:
        for n, start in enumerate((e - 160, e - READ, e - 75, e - 3, e)):
            add(0, start, n % 2 == 0, (0, 0, 3, 2, 1)[n], f"lastedge{e}")
    for plus in (True, False):
        add(0, 0, plus, 0, "first")
        add(0, BIG - READ, plus, 0, "last")
    for n, start in enumerate((0, 777, 16384 - 75, 20000, SMALL - READ)):
        add(1, start, n % 2 == 0, n % 4 if start else 0, "small")
    for r in [out[3], out[4], out[30], out[31], out[60], out[-1], out[-1]]:  # exact duplicates under other names
        out.append(r._replace(label=f"s{len(out)}_dup_of_{r.label}", qual=np.full(READ, ord("5"), np.uint8)))
    for n in range(6):
        out.insert(17 + 29 * n, random_read(rng, f"nowhere{n}"))
    return out


def pairs(g, seed=29):
    """FR pairs whose mates lie on either side of a boundary (TLEN crosses it, next_pos beyond it), a mate across it, pairs on small,
    exact duplicates of some pairs, pairs from nowhere"""
    rng = np.random.default_rng(seed)
    out = []

    def add(ref, left, right, kinds, tag, swap=False):
        a = draw(rng, g, ref, left, True, kinds[0], f"p{len(out)}_{tag}_{left}/1")
        b = draw(rng, g, ref, right, False, kinds[1], f"p{len(out)}_{tag}_{left}/2")
        if swap:  # the reverse mate comes first
            a, b = b._replace(label=a.label), a._replace(label=b.label)
        out.append((a, b))

    for e in EDGES:
        add(0, e - 200, e + 60, (0, 0), f"astride{e}")
        add(0, e - 163, e + 11, (1, 3), f"astride{e}", swap=True)
        add(0, e - 100, e + 150, (0, 2), f"across{e}")       # the forward mate spans the boundary
        add(0, e - 330, e - 149, (2, 0), f"reaches{e}")      # the reverse mate ends one base beyond it
    for e in LAST_EDGES:
        add(0, e - 200, e + 60, (0, 1), f"lastedge{e}")
        add(0, e - 100, e + 150, (1, 0), f"lastedge{e}", swap=True)
    add(1, 100, 420, (0, 1), "small")
    add(1, 16384 - 200, 16384 + 30, (0, 0), "small", swap=True)
    for a, b in [out[0], out[2], out[17], out[17], out[-1]]:
        n = len(out)
        out.append((a._replace(label=f"p{n}_dup/1", qual=np.full(READ, ord("5"), np.uint8)), b._replace(label=f"p{n}_dup/2")))
    for n in range(2):
        out.insert(5 + 11 * n, (random_read(rng, f"nowherepair{n}/1"), random_read(rng, f"nowherepair{n}/2")))
    return out


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for r in reads:
            f.write(b"@" + r.label.encode() + b"\n" + r.seq.tobytes() + b"\n+\n" + r.qual.tobytes() + b"\n")


def build(directory):
    """everything the tests share, made once: -> dict(dir, fasta, ufi, oracle, genome, text, refs, se, pe, fq_se, fq_1, fq_2)"""
    import oracle_lib as ol
    d = str(directory)
    g = genome()
    out = {"dir": d, "genome": g, "fasta": os.path.join(d, "islands.fa"), "ufi": os.path.join(d, "islands.ufi"),
           "refs": [(name, len(seq)) for name, seq in g], "se": single_reads(g), "pe": pairs(g)}
    write_fasta(out["fasta"], g)
    out["oracle"] = ol.Index.build(out["fasta"], SLOTS)
    out["oracle"].save(out["ufi"])
    out["text"] = {name: seq.tobytes().decode("ascii") for name, seq in g}  # the FASTA's sequences, as tags_lib.calmd reads them
    for key, reads in (("fq_se", out["se"]), ("fq_1", [a for a, _ in out["pe"]]), ("fq_2", [b for _, b in out["pe"]])):
        out[key] = os.path.join(d, key + ".fq")
        write_fastq(out[key], reads)
    return out


def level_of(bin_):
    """0 for bin 0 .. 5 for the 16 kb bins"""
    return sum(bin_ >= first for first in (1, 9, 73, 585, 4681))
