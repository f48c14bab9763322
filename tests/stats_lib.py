"""The yardstick of the alignment statistics (-stats): a model in numpy and struct written from the "Stats" text of include/urmapx.h
and sharing nothing with the product, a builder of BAM records that sets every field the rule reads, and a parser of the text.

    rec(...)                            one BAM alignment record
    model(records, names, lens, cmd)    the text the rule asks for
    parse(text)                         the text as a dict of tables
    quotient(num, den, d)               rule 7
"""
import struct

import numpy as np

CYCLES, QUALS, IS_MAX, RL_MAX, ID_MAX = 1024, 94, 8000, 65535, 256
OPS = "MIDNSHP=X"
SN_NAMES = ["records", "secondary", "supplementary", "reads", "reads paired", "first fragments", "last fragments", "reads mapped", "reads unmapped",
            "reads properly paired", "reads mapped and paired", "singletons", "mate on another reference", "reads reverse strand", "reads duplicated",
            "reads QC failed", "reads MQ0", "reads without qualities", "total length", "bases mapped", "bases mapped (cigar)", "bases soft clipped",
            "bases inserted", "bases deleted", "insertions", "deletions", "bases duplicated", "reads with NM", "mismatches", "error rate",
            "average length", "maximum length", "average quality", "pairs with insert size", "inward pairs", "outward pairs", "other pairs",
            "insert size average", "insert size median"]


def parse_cigar(text):
    """"3M2I" -> [(3, 0), (2, 1)]"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), OPS.index(ch)))
            n = ""
    return out


def rec(flag=0, ref=-1, pos=None, mapq=0, next_ref=-1, next_pos=-1, tlen=0, cigar=(), seq=(), qual=None, aux=b"", name=b"r", l_seq=None):
    """One record.  cigar: text or [(length, op code 0..15)]; seq: the 4-bit codes of the bases; qual: bytes (default: 30 each); aux: the
    raw bytes behind QUAL; l_seq: the value of the field where it shall differ from len(seq)."""
    if isinstance(cigar, str):
        cigar = parse_cigar(cigar)
    seq = list(seq)
    if pos is None:
        pos = 0 if ref >= 0 else -1
    if qual is None:
        qual = bytes([30]) * len(seq)
    assert len(qual) == len(seq)
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= c << 4 if i % 2 == 0 else c
    name = name + b"\0"
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name), mapq, 4680, len(cigar), flag, len(seq) if l_seq is None else l_seq, next_ref, next_pos, tlen)
    body += name + b"".join(struct.pack("<I", (l << 4) | op) for l, op in cigar) + bytes(packed) + bytes(qual) + bytes(aux)
    return struct.pack("<I", len(body)) + body


def split(records):
    out, at = [], 0
    while at < len(records):
        size, = struct.unpack_from("<I", records, at)
        out.append(records[at:at + 4 + size])
        at += 4 + size
    assert at == len(records)
    return out


def quotient(num, den, d):
    """rule 7 -> text"""
    v = (10 ** d * num + den // 2) // den if den else 0
    return "%d.%0*d" % (v // 10 ** d, d, v % 10 ** d)


WIDTH = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
INT_FORMAT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}


def find_nm(aux):
    """rule 5 -> the NM value or None"""
    at = 0
    while len(aux) - at >= 3:
        tag, t = aux[at:at + 2], aux[at + 2:at + 3]
        at += 3
        left = len(aux) - at
        if t in WIDTH:
            size = WIDTH[t]
        elif t in (b"Z", b"H"):
            z = aux.find(b"\0", at)
            if z < 0:
                return None
            size = z - at + 1
        elif t == b"B":
            if left < 5 or aux[at:at + 1] == b"A" or aux[at:at + 1] not in WIDTH:
                return None
            size = 5 + struct.unpack_from("<I", aux, at + 1)[0] * WIDTH[aux[at:at + 1]]
        else:
            return None
        if size > left:
            return None
        if tag == b"NM" and t in INT_FORMAT:
            return max(0, struct.unpack_from(INT_FORMAT[t], aux, at)[0])
        at += size
    return None


CLASS_OF = np.full(16, 5, dtype=np.int64)
CLASS_OF[[1, 2, 4, 8, 15]] = [0, 1, 2, 3, 4]
SWAP = np.array([3, 2, 1, 0, 4, 5])


class Tables:
    def __init__(self, n_ref):
        self.sn = dict.fromkeys(SN_NAMES, 0)
        self.nm_bases = self.qual_sum = self.qual_bases = 0
        self.rl = np.zeros((RL_MAX + 1, 2), dtype=object)
        self.mq = [0] * 256
        self.isz = np.zeros((IS_MAX + 1, 3), dtype=np.int64)
        self.q = np.zeros((2, CYCLES + 1, QUALS), dtype=np.int64)
        self.bc = np.zeros((CYCLES + 1, 6), dtype=np.int64)
        self.gc = [0] * 101
        self.ind = np.zeros((ID_MAX + 1, 2), dtype=np.int64)
        self.rf = np.zeros((n_ref + 1, 3), dtype=np.int64)


def count(records, n_ref, T=None):
    """rules 1 .. 6 over the records -> Tables"""
    T = T or Tables(n_ref)
    sn = T.sn
    for r in split(records):
        ref, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, next_ref, _next_pos, tlen = struct.unpack_from("<iiBBHHHIiii", r, 4)
        sn["records"] += 1
        sn["secondary"] += bool(flag & 0x100)
        sn["supplementary"] += bool(flag & 0x800)
        if flag & 0x900:
            continue
        at_cigar = 36 + l_name
        at_seq = at_cigar + 4 * n_cigar
        at_qual = at_seq + (l_seq + 1) // 2
        if at_qual + l_seq > len(r):  # rule 2
            l_seq, n_cigar, aux = 0, 0, b""
            at_seq = at_qual = at_cigar
        else:
            aux = r[at_qual + l_seq:]
        paired, mapped, rev, last, dup = bool(flag & 1), not flag & 4, bool(flag & 0x10), bool(flag & 0x80), bool(flag & 0x400)
        sn["reads"] += 1
        sn["reads paired"] += paired
        sn["last fragments" if last else "first fragments"] += 1
        sn["reads mapped" if mapped else "reads unmapped"] += 1
        sn["reads properly paired"] += paired and mapped and bool(flag & 2)
        mapped_paired = paired and mapped and not flag & 8
        sn["reads mapped and paired"] += mapped_paired
        sn["singletons"] += paired and mapped and bool(flag & 8)
        sn["mate on another reference"] += mapped_paired and next_ref != ref
        sn["reads reverse strand"] += mapped and rev
        sn["reads duplicated"] += dup
        sn["bases duplicated"] += l_seq if dup else 0
        sn["reads QC failed"] += bool(flag & 0x200)
        sn["reads MQ0"] += mapped and mapq == 0
        sn["total length"] += l_seq
        sn["maximum length"] = max(sn["maximum length"], l_seq)
        T.rl[min(l_seq, RL_MAX), int(last)] += 1
        T.rf[ref if ref >= 0 else n_ref, 0 if mapped else 1] += 1
        T.rf[ref if ref >= 0 else n_ref, 2] += dup
        if mapped:
            sn["bases mapped"] += l_seq
            T.mq[mapq] += 1
            ops = np.frombuffer(r, dtype="<u4", count=n_cigar, offset=at_cigar).astype(np.int64)
            op, length = ops & 15, ops >> 4
            aligned = int(length[np.isin(op, [0, 1, 7, 8])].sum())
            sn["bases mapped (cigar)"] += aligned
            sn["bases soft clipped"] += int(length[op == 4].sum())
            for code, bases, events, col in ((1, "bases inserted", "insertions", 0), (2, "bases deleted", "deletions", 1)):
                mine = length[op == code]
                sn[bases] += int(mine.sum())
                mine = mine[mine >= 1]
                sn[events] += len(mine)
                np.add.at(T.ind[:, col], np.minimum(mine, ID_MAX), 1)
            nm = find_nm(aux)
            if nm is not None:
                sn["reads with NM"] += 1
                sn["mismatches"] += nm
                T.nm_bases += aligned
            if mapped_paired and next_ref == ref and tlen > 0:
                mate_rev = bool(flag & 0x20)
                kind = 0 if not rev and mate_rev else 1 if rev and not mate_rev else 2
                T.isz[min(tlen, IS_MAX), kind] += 1
        if l_seq == 0:
            continue
        packed = np.frombuffer(r, dtype=np.uint8, count=(l_seq + 1) // 2, offset=at_seq)
        codes = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq].astype(np.int64)
        qual = np.frombuffer(r, dtype=np.uint8, count=l_seq, offset=at_qual).astype(np.int64)
        cycle = np.arange(l_seq)
        if rev:
            cycle = l_seq - 1 - cycle
        row = np.minimum(cycle, CYCLES)
        cls = CLASS_OF[codes]
        if rev:
            cls = SWAP[cls]
        np.add.at(T.bc, (row, cls), 1)
        T.gc[100 * int(((codes == 2) | (codes == 4)).sum()) // l_seq] += 1
        if qual[0] == 0xFF:
            sn["reads without qualities"] += 1
        else:
            q = np.minimum(qual, QUALS - 1)
            np.add.at(T.q[int(last)], (row, q), 1)
            T.qual_sum += int(q.sum())
            T.qual_bases += l_seq
    return T


def text_of(T, names, lens, command=b""):
    """rules 6 .. 8"""
    sn = dict(T.sn)
    totals = T.isz.sum(axis=1)
    pairs = int(totals.sum())
    sn["error rate"] = quotient(sn["mismatches"], T.nm_bases, 6)
    sn["average length"] = quotient(sn["total length"], sn["reads"], 2)
    sn["average quality"] = quotient(T.qual_sum, T.qual_bases, 2)
    sn["pairs with insert size"] = pairs
    sn["inward pairs"], sn["outward pairs"], sn["other pairs"] = (int(x) for x in T.isz.sum(axis=0))
    sn["insert size average"] = quotient(int((totals * np.arange(IS_MAX + 1)).sum()), pairs, 2)
    sn["insert size median"] = int(np.searchsorted(np.cumsum(totals), (pairs + 1) // 2)) if pairs else 0
    lines = ["# urmapx stats 1", "# command: " + (command.decode("latin-1") if isinstance(command, bytes) else command or "")]
    lines += ["SN\t%s\t%s" % (k, sn[k]) for k in SN_NAMES]
    lines += ["RL\t%d\t%d\t%d" % (l, a, b) for l, (a, b) in enumerate(T.rl) if a or b]
    lines += ["MQ\t%d\t%d" % (q, c) for q, c in enumerate(T.mq) if c]
    lines += ["IS\t%d\t%d\t%d\t%d\t%d" % (s, totals[s], *T.isz[s]) for s in range(IS_MAX + 1) if totals[s]]

    def per_cycle(tag, table):
        used = np.nonzero(table[:CYCLES].any(axis=1))[0]
        rows = ["%s\t%d\t%s" % (tag, c + 1, "\t".join(map(str, table[c]))) for c in range(used[-1] + 1 if len(used) else 0)]
        if table[CYCLES].any():
            rows.append("%s\t>%d\t%s" % (tag, CYCLES, "\t".join(map(str, table[CYCLES]))))
        return rows

    lines += per_cycle("FFQ", T.q[0]) + per_cycle("LFQ", T.q[1]) + per_cycle("BC", T.bc)
    lines += ["GC\t%d\t%d" % (g, c) for g, c in enumerate(T.gc) if c]
    lines += ["ID\t%d\t%d\t%d" % (l, a, b) for l, (a, b) in enumerate(T.ind) if a or b]
    names = [n.decode("latin-1") if isinstance(n, bytes) else n for n in names]
    lines += ["RF\t%s\t%d\t%d\t%d\t%d" % (n, l, *T.rf[k]) for k, (n, l) in enumerate(zip(names, lens))]
    lines.append("RF\t*\t0\t%d\t%d\t%d" % tuple(T.rf[len(lens)]))
    return ("\n".join(lines) + "\n").encode("latin-1")


def model(records, names, lens, command=b""):
    return text_of(count(records, len(lens)), names, lens, command)


def parse(text):
    """{"#": [the comment lines], "SN": {name: value text}, "RL": {length: (first, last)}, ..., "RF": [(name, length, mapped, unmapped,
    duplicated)]}; the keys of the per-cycle tables are the printed cycles (">1024" for the shared row)"""
    out = {"#": [], "SN": {}, "RL": {}, "MQ": {}, "IS": {}, "FFQ": {}, "LFQ": {}, "BC": {}, "GC": {}, "ID": {}, "RF": []}
    order = []
    for line in text.decode("latin-1").split("\n")[:-1]:
        if line.startswith("#"):
            out["#"].append(line)
            continue
        f = line.split("\t")
        if not order or order[-1] != f[0]:
            order.append(f[0])
        if f[0] == "SN":
            out["SN"][f[1]] = f[2]
        elif f[0] == "RF":
            out["RF"].append((f[1],) + tuple(int(x) for x in f[2:]))
        else:
            key = f[1] if f[1].startswith(">") else int(f[1])
            vals = tuple(int(x) for x in f[2:])
            out[f[0]][key] = vals[0] if len(vals) == 1 else vals
    assert order == [s for s in ("SN", "RL", "MQ", "IS", "FFQ", "LFQ", "BC", "GC", "ID", "RF") if s in order], order
    assert list(out["SN"]) == SN_NAMES
    return out
