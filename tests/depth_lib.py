"""The depth rule of include/urmapx.h "Depth" as a model of its own, for tests/test_depth_cpu.py and tests/test_gpu_depth.py: a loop over
the records that adds one to a plain numpy array per covered column, then np.diff / np.flatnonzero for the runs.  It shares no code with
depth_host.cpp or depth.hip (no difference array, no scan), so agreement with either says something.  Also the inputs both test files
use."""
import struct

import numpy as np

import bam_lib as bl
import bam_sort_lib as sl
import markdup_lib as ml

R = ml.rec
EXCLUDED = 0x4 | 0x100 | 0x200 | 0x400  # samtools depth's default mask


def with_mapq(rec, mapq):
    """the record with another MAPQ byte"""
    return rec[:13] + bytes([mapq]) + rec[14:]


def model(records, names, lens, min_mapq=0):
    """records: bytes, the chain of BAM records -> (bedGraph text, number of lines, [dict of reads, covered, bases, mapq_sum])"""
    n_ref = len(lens)
    depth = [np.zeros(int(l), dtype=np.int32) for l in lens]  # (four bytes a column: a chromosome's worth stays within a second or two)
    summary = [dict(reads=0, covered=0, bases=0, mapq_sum=0) for _ in lens]
    for _, r in sl.split_records(bytes(records)):
        ref_id, pos, l_name, mapq, _bin, n_cigar, flag = struct.unpack_from("<iiBBHHH", r, 4)
        if not 0 <= ref_id < n_ref or pos < 0 or flag & EXCLUDED or mapq < min_mapq:
            continue
        summary[ref_id]["reads"] += 1
        summary[ref_id]["mapq_sum"] += mapq
        c = pos
        for k in range(n_cigar):
            w, = struct.unpack_from("<I", r, 36 + l_name + 4 * k)
            op, length = bl.CIGAR_LETTERS[w & 15], w >> 4
            if op in "M=X":
                depth[ref_id][c:c + length] += 1  # (numpy cuts the slice off at the array's end)
            if op in "MDN=X":
                c += length
    lines = []
    for r, d in enumerate(depth):
        summary[r]["covered"] = int(np.count_nonzero(d))
        summary[r]["bases"] = int(d.sum(dtype=np.int64))
        if not len(d):
            continue
        begs = np.concatenate(([0], np.flatnonzero(np.diff(d)) + 1))
        ends = np.append(begs[1:], len(d))
        name = names[r].encode("latin-1") if isinstance(names[r], str) else names[r]
        lines += [b"%s\t%d\t%d\t%d\n" % (name, b, e, d[b]) for b, e in zip(begs.tolist(), ends.tolist())]
    return b"".join(lines), len(lines), summary


def parse(text):
    """the lines of a bedGraph text -> [(name, beg, end, depth)]"""
    return [(n, int(b), int(e), int(d)) for n, b, e, d in (l.split(b"\t") for l in text.split(b"\n") if l)]


def check_tiling(text, names, lens):
    """the lines of every reference with columns tile it exactly, in index order, and neighbouring runs differ in depth"""
    rows = parse(text)
    at = 0
    for name, l in zip(names, lens):
        name = name.encode("latin-1") if isinstance(name, str) else name
        if not l:
            continue
        x = 0
        while x < l:
            n, b, e, d = rows[at]
            assert (n, b) == (name, x) and b < e <= l, rows[at]
            assert x == 0 or d != rows[at - 1][3], rows[at]
            x = e
            at += 1
    assert at == len(rows)


def span(ref_id, pos, length, mapq=0, flag=0, name=b"a"):
    """a 38-byte record and one M op behind it: the smallest record that covers something"""
    return with_mapq(R(ref_id, pos, flag, "%dM" % length, b"", name[:1]), mapq)


def cigar_cases():
    """(records, names, lens) of the CPU cases of the rule: every op, the edges of a reference, the flags, names and digit counts"""
    names = ["c", "zero", "one", "n" * 200, "last"]
    lens = [400, 0, 1, 300, 50]
    recs = [
        R(0, 10, 0, "5M2I3D4N6S7H8P9=10X", b""),             # every op
        R(0, 0, 0, "4D6M", b""),                             # pos 0; starts with D
        R(0, 20, 0, "5S3I", b""),                            # only S and I: covers nothing, counts as a read
        R(0, 30, 0, "", b""),                                # no CIGAR
        R(0, 390, 0, "30M", b""),                            # hangs past l_ref
        R(0, 395, 0, "5M", b""),                             # ends exactly at l_ref ...
        R(2, 0, 0, "1M", b""),                               # ... beside the one column of reference 2
        R(2, 0, 0, "8M", b""),                               # over the end of a reference of length 1
        R(2, 1, 0, "3M", b""),                               # wholly beyond it
        R(3, 0, 0, "300M", b""), R(3, 299, 0, "1M", b""),   # a whole reference; its last column
        R(4, 0, 0, "20M", b""),                              # starts at 0 of the last reference
        R(-1, -1, 4, "", b""),                               # no reference
    ]
    for flag in (0x4, 0x100, 0x200, 0x400, 0x800, 0x10, 0x1 | 0x40):
        recs.append(R(4, 30, flag, "10M", b""))
    for q in (0, 17, 18, 60, 255):
        recs.append(with_mapq(R(4, 45, 0, "3M", b""), q))
    return b"".join(recs), names, lens


def digits_case(depth):
    """`depth` identical records over one 20-column span of a 30-column reference"""
    return span(0, 5, 20) * depth, ["d"], [30]
