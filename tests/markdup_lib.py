"""The yardstick of -markdup: rules 1-7 of "Duplicate marking" (include/urmapx.h) in plain Python over the records of
bam_sort_lib.split_records, sharing nothing with the product.

    model(records)                 [bytes] in input order -> ([is the record flagged 0x400 on output], counters)
    end5(rec)                      the end (refID, u5, rev) of one record
    score(rec)                     the sum of its QUAL bytes q with 15 <= q != 0xFF
    rec(...)                       one hand-made record with any CIGAR, flag, qualities and aux bytes
    flags_of(stream)               the flag of every record of a stream
    check(...)                     a marked stream against the plain sort of the same records and the model
"""
import struct

import bam_lib as bl
import bam_sort_lib as sl

DUP = 0x400
INELIGIBLE = 0x4 | 0x100 | 0x800
MAX_SCORE = (1 << 31) - 1


def core(r):
    ref_id, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", r, 4)
    return ref_id, pos, l_name, n_cig, flag, l_seq


def cigar(r):
    _, _, l_name, n_cig, _, _ = core(r)
    ws = struct.unpack_from(f"<{n_cig}I", r, 36 + l_name)
    return [(w >> 4, bl.CIGAR_LETTERS[w & 15]) for w in ws]


def end5(r):
    ref_id, pos, _, _, flag, _ = core(r)
    ops = cigar(r)
    on_ref = [k for k, (_, op) in enumerate(ops) if op in bl.REF_CONSUMING]
    span = sum(ops[k][0] for k in on_ref) or 1
    clip = lambda part: sum(n for n, op in part if op in "SH")
    if flag & 0x10:
        return ref_id & 0xFFFFFFFF, pos + span - 1 + clip(ops[on_ref[-1] + 1:] if on_ref else ops), 1
    return ref_id & 0xFFFFFFFF, pos - clip(ops[:on_ref[0]] if on_ref else ops), 0


def score(r):
    _, _, l_name, n_cig, _, l_seq = core(r)
    at = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
    q = r[at:at + l_seq]
    assert len(q) == l_seq
    return min(MAX_SCORE, sum(b for b in q if 15 <= b != 0xFF))


def name(r):
    return r[36:36 + r[12]]


def model(records):
    n = len(records)
    flag = [core(r)[4] for r in records]
    ok = [not f & INELIGIBLE for f in flag]
    end = [end5(r) if ok[i] else None for i, r in enumerate(records)]
    sc = [score(r) if ok[i] else 0 for i, r in enumerate(records)]
    dup = [bool(f & DUP) for f in flag]       # (ineligible records keep theirs)
    for i in range(n):
        if ok[i]:
            dup[i] = False
    # rule 3: pairs, from the front
    mate = [None] * n   # 1: first of a pair, 2: second
    pairs = []
    i = 0
    while i < n:
        if (i + 1 < n and ok[i] and ok[i + 1] and mate[i] is None and flag[i] & 0xC1 == 0x41 and flag[i + 1] & 0x81 == 0x81
                and name(records[i]) == name(records[i + 1])):
            mate[i], mate[i + 1] = 1, 2
            pairs.append(i)
            i += 2
        else:
            i += 1
    # rule 5
    groups = {}
    for i in pairs:
        groups.setdefault((min(end[i], end[i + 1]), max(end[i], end[i + 1])), []).append(i)
    pair_dups = 0
    for members in groups.values():
        best = max(members, key=lambda i: (sc[i] + sc[i + 1], -i))
        for i in members:
            if i != best:
                dup[i] = dup[i + 1] = True
                pair_dups += 1
    # rule 6
    groups = {}
    for i in range(n):
        if ok[i]:
            groups.setdefault(end[i], []).append(i)
    frags = frag_dups = 0
    for members in groups.values():
        lone = [i for i in members if mate[i] is None]
        frags += len(lone)
        if not lone:
            continue
        best = None if len(lone) < len(members) else max(lone, key=lambda i: (sc[i], -i))
        for i in lone:
            if i != best:
                dup[i] = True
                frag_dups += 1
    return dup, {"pairs_examined": len(pairs), "pairs_duplicate": pair_dups, "fragments_examined": frags, "fragments_duplicate": frag_dups}


def rec(ref_id, pos, flag=0, cig="", qual=b"", qname=b"r", aux=b"", l_seq=None):
    """one record: cig as text ('5S20M', '' for none), qual as bytes (raw values), the bases all 'A'"""
    ops = bl.parse_cigar(cig) if cig else []
    nm = qname + b"\0"
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, len(nm), 0, bl.record_bin(pos, ops) if ref_id >= 0 else 4680, len(ops), flag,
                       len(qual) if l_seq is None else l_seq, -1, -1, 0)  # (l_seq: a length field that lies, for the refusals)
    body += nm + b"".join(struct.pack("<I", k << 4 | bl.CIGAR_LETTERS.index(op)) for k, op in ops) + b"\x11" * ((len(qual) + 1) // 2) + bytes(qual) + aux
    return struct.pack("<I", len(body)) + body


def flags_of(stream):
    return [core(r)[4] for _, r in sl.split_records(stream)]


def mask_dup(stream):
    """the stream with bit 0x400 of every record cleared"""
    out = bytearray(stream)
    for off, _ in sl.split_records(stream):
        out[off + 19] &= 0xFB
    return bytes(out)


def check(records, marked_stream, plain_stream, rep=None):
    """records: the unsorted input; marked_stream: the inflated result with the option; plain_stream: without.  Only 0x400 bits
    differ, they are the model's, and so are the counters of rep"""
    assert mask_dup(marked_stream) == mask_dup(plain_stream), "more than bit 0x400 differs from the plain sort"
    recs = [r for _, r in sl.split_records(records)]
    want, counters = model(recs)
    # the sort is stable and 0x400 is no part of the key: record k of the sorted stream is record order[k] of the input
    order = sorted(range(len(recs)), key=lambda i: sl.sort_key(recs[i]))
    got = [bool(f & DUP) for f in flags_of(marked_stream)]
    assert len(got) == len(recs)
    assert got == [want[i] for i in order], [(k, order[k]) for k in range(len(got)) if got[k] != want[order[k]]][:10]
    if rep is not None:
        for k, v in counters.items():
            assert rep[k] == v, (k, rep[k], v)
    return want, counters
