"""The yardstick of the sorted BAM output (-bamout ... -sort): a reader of .bai files and of BGZF virtual offsets in pure Python,
written from the SAM/BAM specification (SAMv1 sections 4.1, 5.2 and 5.3) and sharing nothing with the product.  Beside bam_lib.py,
which reads and writes the records themselves.

    split_records(stream)               the records of an uncompressed record stream, each with its offset
    fields(record)                      refID, pos, end on the reference, the bin the index files it under, flag
    oracle_order(records)               the order the sort must give: Python's stable sort on (refID, pos) read as unsigned
    parse_bai(data)                     a .bai file -> Bai (bins with their chunks, pseudo-bins, linear indexes, n_no_coor)
    reg2bins(beg, end)                  the bins that may hold records overlapping [beg, end)
    BgzfFile(blob)                      a BGZF file read by virtual offset, member by member
    query(bai, f, ref, beg, end)        what a reader does with an index; brute(...) is the answer over all records
    check_sorted_bam(...)               every property the tests ask of a sorted stream and its index
"""
import bisect
import struct
import zlib

import numpy as np

import bam_lib as bl

MEMBER = 65280
PSEUDO_BIN = 37450
WINDOW = 1 << 14
INDEX_END = 1 << 29   # the scheme of section 5.3 covers [0, 2^29) of a reference
MAX_BIN = 37448       # its last bin: 4681 + 2^15 - 1
MAX_WINDOWS = INDEX_END // WINDOW
LEVELS = [(0, 0), (1, 8), (9, 72), (73, 584), (585, 4680), (4681, MAX_BIN)]  # first and last bin of each of the six levels


def split_records(stream):
    """[(offset, record bytes)] along the block_size chain"""
    out, at = [], 0
    while at < len(stream):
        size, = struct.unpack_from("<I", stream, at)
        assert size >= 32 and at + 4 + size <= len(stream), (at, size)
        out.append((at, stream[at:at + 4 + size]))
        at += 4 + size
    assert at == len(stream)
    return out


def fields(rec):
    """(refID, pos, end, bin, flag) of one record; end = pos + the reference bases of the CIGAR, at least one.  bin is where the index
    files the record: that of [pos, min(end, 2^29)); None for a record without a reference or with pos >= 2^29, which gets no chunk
    and no window"""
    ref_id, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    span = 0
    for k in range(n_cig):
        w, = struct.unpack_from("<I", rec, 36 + l_name + 4 * k)
        if bl.CIGAR_LETTERS[w & 15] in bl.REF_CONSUMING:
            span += w >> 4
    end = pos + (span if span else 1)
    return ref_id, pos, end, bl.reg2bin(pos, min(end, INDEX_END)) if ref_id >= 0 and pos < INDEX_END else None, flag


def sort_key(rec):
    ref_id, pos = struct.unpack_from("<ii", rec, 4)
    return ref_id & 0xFFFFFFFF, pos & 0xFFFFFFFF


def oracle_order(records):
    """records (bytes each) in the order of the issue: refID as unsigned, then pos, ties in input order (sorted() is stable)"""
    return sorted(records, key=sort_key)


# ---- .bai ----
class Bai:
    def __init__(self):
        self.refs = []       # per reference: {"bins": [(bin, [(beg, end)])] in file order, "pseudo": (beg, end, mapped, unmapped) | None, "linear": [..]}
        self.n_no_coor = None


def parse_bai(data):
    assert data[:4] == b"BAI\1", data[:4]
    n_ref, = struct.unpack_from("<I", data, 4)
    at = 8
    b = Bai()
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<I", data, at)
        at += 4
        bins, pseudo = [], None
        for _ in range(n_bin):
            bin_, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if bin_ == PSEUDO_BIN:
                assert n_chunk == 2 and pseudo is None
                pseudo = (chunks[0][0], chunks[0][1], chunks[1][0], chunks[1][1])
            else:
                assert n_chunk >= 1 and bin_ <= MAX_BIN, (bin_, n_chunk)
                bins.append((bin_, chunks))
        n_intv, = struct.unpack_from("<I", data, at)
        assert n_intv <= MAX_WINDOWS, n_intv
        at += 4
        linear = list(struct.unpack_from(f"<{n_intv}Q", data, at))
        at += 8 * n_intv
        b.refs.append({"bins": bins, "pseudo": pseudo, "linear": linear})
    b.n_no_coor, = struct.unpack_from("<Q", data, at)
    at += 8
    assert at == len(data), (at, len(data))
    return b


def reg2bins(beg, end):
    """section 5.3: the bins that overlap the zero-based half-open region [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


# ---- BGZF by virtual offset ----
class BgzfFile:
    """a BGZF file as a reader sees it: members found by their file offset, inflated one at a time"""

    def __init__(self, blob):
        self.blob = blob
        self.cache = {}

    def member(self, coffset):
        """(inflated bytes, file offset of the next member)"""
        if coffset not in self.cache:
            h = self.blob[coffset:coffset + 18]
            assert h[:4] == b"\x1f\x8b\x08\x04" and h[12:14] == b"BC", (coffset, h)
            size = struct.unpack_from("<H", h, 16)[0] + 1
            data = zlib.decompress(self.blob[coffset + 18:coffset + size - 8], -15)
            crc, isize = struct.unpack_from("<II", self.blob, coffset + size - 8)
            assert zlib.crc32(data) == crc and len(data) == isize
            self.cache[coffset] = (data, coffset + size)
        return self.cache[coffset]

    def members(self, start=0):
        """[(file offset, inflated size)] of every member from `start` on"""
        out, at = [], start
        while at < len(self.blob):
            data, nxt = self.member(at)
            out.append((at, len(data)))
            at = nxt
        return out

    def read_records(self, vbeg, vend):
        """the records that START in [vbeg, vend), as a reader takes them: seek to vbeg, read record after record across members until
        the place reached is vend or beyond"""
        coff, within = vbeg >> 16, vbeg & 0xFFFF
        out = []

        def take(n):
            nonlocal coff, within
            got = b""
            while len(got) < n:
                data, nxt = self.member(coff)
                if within >= len(data):
                    assert data or n == 0, "read past the end-of-file member"
                    coff, within = nxt, 0
                    continue
                piece = data[within:within + n - len(got)]
                got += piece
                within += len(piece)
            return got

        while True:
            data, nxt = self.member(coff)
            if within >= len(data) and data:  # at a member's end: the place is the next member's start
                coff, within = nxt, 0
                continue
            if (coff << 16 | within) >= vend or not data:
                return out
            head = take(4)
            out.append(head + take(struct.unpack("<I", head)[0]))


def stream_place(v, table):
    """a virtual offset back into a place of the record stream; table: {file offset of a member: stream offset of its first byte}"""
    return table[v >> 16] + (v & 0xFFFF)


def member_places(f, in_front):
    """{file offset: stream offset} of the record members of a file whose records begin at file offset in_front; the end-of-file
    member (or the end of a bare member series) is in it, so a place at the very end is defined"""
    table, u = {}, 0
    for coff, size in f.members(in_front):
        table[coff] = u
        u += size
    table[len(f.blob)] = u
    return table


def overlaps(ref_id, pos, end, ref, beg, stop):
    return ref_id == ref and pos < stop and end > beg


def query(bai, f, ref, beg, end):
    """the records of reference `ref` that overlap [beg, end), found the way section 5.1.1 and 5.3 describe: the bins of the region, their
    chunks, without those that end at or before the linear index's value for the region's first window; seek, read, keep what overlaps"""
    r = bai.refs[ref]
    lin = r["linear"]
    w = beg >> 14
    floor = lin[w] if w < len(lin) else (lin[-1] if lin else 0)
    want = set(reg2bins(beg, end))
    chunks = sorted(c for b, cs in r["bins"] if b in want for c in cs if c[1] > floor)
    out = []
    for cb, ce in chunks:
        for rec in f.read_records(cb, ce):
            fr, fp, fe, _, _ = fields(rec)
            if overlaps(fr, fp, fe, ref, beg, end):
                out.append(rec)
    return out


def brute(records, ref, beg, end):
    return [rec for rec in records if overlaps(*fields(rec)[:3], ref, beg, end)]


# ---- everything a sorted stream and its index must satisfy ----
def check_stream(members_blob, unsorted):
    """members_blob: the BGZF members of the sorted stream alone.  The stream is the oracle's order of the unsorted records, cut every
    65 280 bytes.  -> (stream, [(offset, record)])"""
    f = BgzfFile(members_blob)
    sizes = [s for _, s in f.members()]
    assert all(s == MEMBER for s in sizes[:-1]) and (not sizes or 0 < sizes[-1] <= MEMBER), sizes[-3:]
    stream = b"".join(f.member(c)[0] for c, _ in f.members())
    want = oracle_order([r for _, r in split_records(unsorted)])
    got = split_records(stream)
    assert len(got) == len(want)
    assert [r for _, r in got] == want, "order differs from the stable Python sort"
    assert sorted(r for _, r in got) == sorted(r for _, r in split_records(unsorted)), "the multiset of records changed"
    return stream, got


def index_in_places(bai, table):
    """the index with every virtual offset turned back into a place of the stream: what two sorts of the same records must agree on"""
    refs = []
    for r in bai.refs:
        p = r["pseudo"]
        refs.append({"bins": [(b, [(stream_place(x, table), stream_place(y, table)) for x, y in cs]) for b, cs in r["bins"]],
                     "pseudo": None if p is None else (stream_place(p[0], table), stream_place(p[1], table), p[2], p[3]),
                     "linear": [stream_place(v, table) for v in r["linear"]]})
    return refs, bai.n_no_coor


def check_index(bai, recs, table, n_ref):
    """recs: [(stream offset, record)] of the sorted stream; table: member_places of the file the index belongs to.  A record with
    pos >= 2^29 counts in its reference's pseudo-bin and nowhere else; one that ends beyond 2^29 has its windows up to 32 767"""
    assert len(bai.refs) == n_ref
    refs, n_no_coor = index_in_places(bai, table)
    by_ref = [[] for _ in range(n_ref)]
    none = 0
    for off, rec in recs:
        ref_id, pos, end, bin_, flag = fields(rec)
        if ref_id < 0:
            none += 1
        else:
            by_ref[ref_id].append((off, off + len(rec), pos, end, bin_, flag))
    assert n_no_coor == none
    for r, mine in zip(refs, by_ref):
        bins = r["bins"]
        assert [b for b, _ in bins] == sorted(set(b for b, _ in bins)), "bins out of order or repeated"
        chunks_of = dict(bins)
        for b, cs in bins:  # chunks of a bin: in order, not overlapping, not empty
            for (x, y), nxt in zip(cs, cs[1:] + [None]):
                assert x < y and (nxt is None or y <= nxt[0]), (b, cs)
        for off, stop, pos, end, bin_, flag in mine:  # every record lies inside a chunk of its bin
            assert bin_ is None or any(x <= off and stop <= y for x, y in chunks_of.get(bin_, [])), (off, bin_)
        assert set(chunks_of) == set(m[4] for m in mine if m[4] is not None)
        every = sorted((x, y, b) for b, cs in bins for x, y in cs)  # no record lies inside a chunk of another bin, or of any without one
        assert all(a[1] <= c[0] for a, c in zip(every, every[1:])), "chunks of different bins overlap"
        begins = [x for x, _, _ in every]
        for off, stop, pos, end, bin_, flag in mine:
            at = bisect.bisect_right(begins, off) - 1
            holder = every[at][2] if at >= 0 and stop <= every[at][1] else None
            assert holder == bin_, (off, bin_, holder)
        starts = set(m[0] for m in mine) | set(m[1] for m in mine)
        assert all(x in starts and y in starts for cs in chunks_of.values() for x, y in cs), "a chunk does not begin and end at a record"
        if not mine:
            assert r["pseudo"] is None and not bins and not r["linear"]
            continue
        unm = sum(1 for m in mine if m[5] & 4)
        assert r["pseudo"] == (mine[0][0], mine[-1][1], len(mine) - unm, unm), r["pseudo"]
        lin = r["linear"]
        mine = [(off, stop, pos, min(end, INDEX_END), bin_, flag) for off, stop, pos, end, bin_, flag in mine if bin_ is not None]
        if not mine:
            assert not lin
            continue
        assert len(lin) == ((max(m[3] for m in mine) - 1) >> 14) + 1, "the linear index does not end behind the last non-empty window"
        assert all(a <= b for a, b in zip(lin, lin[1:])), "linear index not monotone"
        none = 1 << 63  # (no place of a stream is that large)
        smallest = np.full(len(lin), none, dtype=np.uint64)  # per window: the smallest place of a record that overlaps it
        for off, stop, pos, end, bin_, flag in mine:
            a, b = pos >> 14, ((end - 1) >> 14) + 1
            smallest[a:b] = np.minimum(smallest[a:b], np.uint64(off))
        want = smallest.tolist()
        assert want[-1] != none
        for w in range(len(want) - 2, -1, -1):  # an empty window: the next non-empty one's value
            if want[w] == none:
                want[w] = want[w + 1]
        assert lin == want, [(w, v, x) for w, (v, x) in enumerate(zip(lin, want)) if v != x][:5]


def check_queries(bai, f, records, regions):
    for ref, beg, end in regions:
        assert query(bai, f, ref, beg, end) == brute(records, ref, beg, end), (ref, beg, end)


def edge_regions(ref_lengths, rng, n_random=200):
    """seeded random regions, position 0, a reference's last base, across the first boundary of every level: 2^14, 2^17, 2^20, 2^23, 2^26"""
    out = []
    for _ in range(n_random):
        ref = int(rng.integers(0, len(ref_lengths)))
        L = ref_lengths[ref]
        beg = int(rng.integers(0, L))
        out.append((ref, beg, min(L, beg + int(rng.integers(1, 1 + max(1, L // 4))))))
    for ref, L in enumerate(ref_lengths):
        out += [(ref, 0, 1), (ref, 0, min(L, 100)), (ref, L - 1, L)]
        for edge in (1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26):
            if L > edge:
                out += [(ref, edge - 1, edge + 1), (ref, edge - 10, min(L, edge + 300)), (ref, edge, edge + 1), (ref, edge - 1, edge)]
    return out


def compose_file(header_members, sorted_members):
    """a BAM file as -sort lays it out: header block in members of its own, the sorted stream, the end-of-file member"""
    from urmap_amd import api
    return header_members + sorted_members + api.BGZF_EOF
