"""A small BAM reader and writer in pure Python, written from the SAM/BAM specification (SAMv1 section 4.2 and 5.3) and sharing
nothing with the product: the yardstick of tests/test_bam_cpu.py and tests/test_gpu_bam.py.

    read_bam(data)                    uncompressed BAM bytes -> (header text, [(name, length)], [SAM line])
    sam_to_bam_records(sam, refs)     SAM text -> the bytes of its alignment records (header lines are skipped)
    bam_header(text, refs)            the bytes in front of the first record
    inflate(blob)                     a BGZF file -> the bytes inside

Optional fields are neither read nor written: the product writes none, and read_bam refuses a record that has any."""
import gzip
import struct

SEQ_LETTERS = "=ACMGRSVTWYHKDBN"   # section 4.2: the 4-bit code of a base is its index here
CIGAR_LETTERS = "MIDNSHP=X"        # op codes 0..8
REF_CONSUMING = "MDN=X"            # ops that advance the reference (section 1.4, CIGAR)


def reg2bin(beg, end):
    """section 5.3, the C code of the specification word for word: bin of the zero-based half-open region [beg, end)"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def nibble(letter):
    """4-bit code of one SEQ letter: case-insensitive, anything outside the table is N (what htslib's seq_nt16_table does)"""
    k = SEQ_LETTERS.find(letter.upper())
    return k if k >= 0 else 15


def parse_cigar(text):
    """'3M2I' -> [(3, 'M'), (2, 'I')]; '*' -> []"""
    if text == "*":
        return []
    ops, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            assert num and ch in CIGAR_LETTERS, text
            ops.append((int(num), ch))
            num = ""
    assert not num, text
    return ops


def record_bin(pos, ops):
    """the bin field of a record at zero-based pos (-1: unplaced) with these CIGAR ops"""
    span = sum(n for n, op in ops if op in REF_CONSUMING)
    return reg2bin(pos, pos + (span if span else 1)) & 0xFFFF  # (the field is 16 bits; the bins cover positions below 2^29)


def sam_line_to_bam(line, ref_index):
    """one SAM line (str, eleven fields, no optional ones) -> its BAM record, block_size included"""
    f = line.rstrip("\n").split("\t")
    assert len(f) == 11, f"{len(f)} fields: {line[:80]!r}"
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f
    ref_id = -1 if rname == "*" else ref_index[rname]
    next_id = -1 if rnext == "*" else ref_id if rnext == "=" else ref_index[rnext]
    pos0, pnext0 = int(pos) - 1, int(pnext) - 1
    ops = parse_cigar(cigar)
    name = qname.encode("latin-1") + b"\0"
    assert len(name) <= 255, "QNAME does not fit l_read_name"
    l_seq = 0 if seq == "*" else len(seq)
    packed = bytearray((l_seq + 1) // 2)
    for i in range(l_seq):
        packed[i >> 1] |= nibble(seq[i]) << (0 if i & 1 else 4)
    if qual == "*":
        q = b"\xff" * l_seq
    else:
        assert len(qual) == l_seq
        q = bytes(ord(c) - 33 for c in qual)
    body = struct.pack("<iiBBHHHIiii", ref_id, pos0, len(name), int(mapq), record_bin(pos0, ops), len(ops), int(flag), l_seq,
                       next_id, pnext0, int(tlen))
    body += name + b"".join(struct.pack("<I", n << 4 | CIGAR_LETTERS.index(op)) for n, op in ops) + bytes(packed) + q
    return struct.pack("<I", len(body)) + body


def _ref_list(refs):
    return [(r, 0) if isinstance(r, str) else (r[0], int(r[1])) for r in refs]


def sam_to_bam_records(sam_text, refs):
    """SAM text (bytes or str; '@' lines are skipped) -> the expected bytes of its alignment records.  refs: the reference
    names in header order, or (name, length) pairs"""
    if isinstance(sam_text, bytes):
        sam_text = sam_text.decode("latin-1")
    index = {}
    for i, (name, _) in enumerate(_ref_list(refs)):
        index.setdefault(name, i)
    return b"".join(sam_line_to_bam(l, index) for l in sam_text.split("\n") if l and not l.startswith("@"))


def bam_header(text, refs):
    """magic, l_text, text, n_ref and the reference list"""
    if isinstance(text, str):
        text = text.encode("latin-1")
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for name, length in _ref_list(refs):
        n = name.encode("latin-1") + b"\0"
        out += struct.pack("<I", len(n)) + n + struct.pack("<I", length)
    return out


def refs_of_header(text):
    """[(SN, LN)] of the @SQ lines of a SAM header"""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    refs = []
    for l in text.split("\n"):
        if l.startswith("@SQ"):
            tags = dict(t.split(":", 1) for t in l.split("\t")[1:])
            refs.append((tags["SN"], int(tags["LN"])))
    return refs


def read_bam(data):
    """uncompressed BAM bytes -> (header text as bytes, [(name, length)], [SAM line as str]).  Checks as it goes: the magic, every
    length against the bytes that are there, NUL termination of names, block_size against the fields inside, bin == reg2bin,
    indexes inside the reference list, no bytes left over."""
    assert data[:4] == b"BAM\1", data[:4]
    l_text, = struct.unpack_from("<I", data, 4)
    at = 8
    text = data[at:at + l_text]
    assert len(text) == l_text
    at += l_text
    n_ref, = struct.unpack_from("<I", data, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", data, at)
        name = data[at + 4:at + 4 + l_name]
        assert l_name >= 1 and len(name) == l_name and name[-1] == 0 and 0 not in name[:-1], name
        l_ref, = struct.unpack_from("<I", data, at + 4 + l_name)
        refs.append((name[:-1].decode("latin-1"), l_ref))
        at += 8 + l_name
    return text, refs, read_bam_records(data[at:], refs)


def read_bam_records(data, refs):
    """the records alone (what a chunk of the text stage holds) -> [SAM line as str]"""
    lines, at = [], 0

    def ref_name(i):
        assert -1 <= i < len(refs), i
        return "*" if i < 0 else refs[i][0]

    while at < len(data):
        assert at + 36 <= len(data), "truncated record"
        block_size, ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq, next_id, next_pos, tlen = struct.unpack_from("<IiiBBHHHIiii", data, at)
        assert block_size == 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq, (at, block_size, l_name, n_cig, l_seq)
        assert at + 4 + block_size <= len(data), "block_size runs past the end"
        p = at + 36
        name = data[p:p + l_name]
        assert l_name >= 1 and name[-1] == 0 and 0 not in name[:-1], name
        p += l_name
        ops = []
        for k in range(n_cig):
            w, = struct.unpack_from("<I", data, p + 4 * k)
            assert w & 15 < len(CIGAR_LETTERS)
            ops.append((w >> 4, CIGAR_LETTERS[w & 15]))
        p += 4 * n_cig
        assert pos >= -1 and next_pos >= -1
        assert bin_ == record_bin(pos, ops), (at, bin_, pos, ops)
        packed = data[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join(SEQ_LETTERS[packed[i >> 1] >> (0 if i & 1 else 4) & 15] for i in range(l_seq))
        if l_seq & 1:
            assert packed[-1] & 15 == 0, "the unused low nibble is not zero"
        q = data[p:p + l_seq]
        p += l_seq
        assert p == at + 4 + block_size
        if l_seq and q == b"\xff" * l_seq:
            qual = "*"
        else:
            assert all(b <= 93 for b in q), "quality above '~'"
            qual = "".join(chr(b + 33) for b in q) if l_seq else "*"
        rnext = "*" if next_id < 0 else "=" if next_id == ref_id else ref_name(next_id)
        lines.append("\t".join([name[:-1].decode("latin-1"), str(flag), ref_name(ref_id), str(pos + 1), str(mapq),
                                "".join(f"{n}{op}" for n, op in ops) or "*", rnext, str(next_pos + 1), str(tlen), seq or "*", qual]))
        at = p
    assert at == len(data)
    return lines


def normalise_sam_line(line):
    """a SAM line as it comes back out of BAM: SEQ upper-cased, letters outside the 4-bit table as N"""
    if isinstance(line, bytes):
        line = line.decode("latin-1")
    f = line.rstrip("\n").split("\t")
    if f[9] != "*":
        f[9] = "".join(SEQ_LETTERS[nibble(c)] for c in f[9])
    return "\t".join(f)


def sam_records(sam_text):
    """the record lines of SAM text, normalised"""
    if isinstance(sam_text, bytes):
        sam_text = sam_text.decode("latin-1")
    return [normalise_sam_line(l) for l in sam_text.split("\n") if l and not l.startswith("@")]


def sam_header(sam_text):
    if isinstance(sam_text, bytes):
        sam_text = sam_text.decode("latin-1")
    return "".join(l + "\n" for l in sam_text.split("\n") if l.startswith("@"))


def inflate(blob):
    """a BGZF file (a series of gzip members) -> the bytes inside"""
    return gzip.decompress(blob) if blob else b""
