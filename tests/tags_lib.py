"""The yardstick of the optional fields NM, MD, AS and RG (tests/test_tags_cpu.py, tests/test_gpu_tags.py): plain Python written from
the SAM specification (section 1.5, SAMtags, section 4.2.4) and the rules of include/urmapx.h "Optional fields", sharing nothing with
the product.

    read_fasta(path)                      {name: sequence as it stands in the file, case kept}
    calmd(ref, pos, cigar, seq)           (NM, MD) of a record at 1-based pos of the sequence ref
    rebuild_reference(seq, cigar, md)     the reference span a record's SEQ + CIGAR + MD describe (the inverse check)
    split_fields(line)                    a SAM line -> (the eleven mandatory fields joined, {tag: (type, value)}, [tag order])
    read_bam_records_aux(data, refs)      BAM records with aux fields -> [(SAM line by bam_lib, [(tag, type, value)])]
    check_sam_record(line, fasta, ...)    every rule for one tagged SAM line
"""
import re
import struct

import bam_lib as bl

MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*$")
FIELD_ORDER = ["NM", "MD", "AS", "RG"]


def read_fasta(path):
    seqs, name = {}, None
    for line in open(path, "r"):
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        elif name is not None:
            seqs[name].append(line)
    return {k: "".join(v) for k, v in seqs.items()}


def letters_match(a, b):
    """samtools calmd's test: equal 4-bit codes, and that code is not 15 (N, or anything outside the table)"""
    x, y = bl.nibble(a), bl.nibble(b)
    return x == y and x != 15


def calmd(ref, pos, cigar, seq):
    """ref: the whole sequence (str); pos: 1-based POS; cigar: text or [(n, op)] with ops M I D; seq: SEQ as printed -> (NM, MD)"""
    ops = bl.parse_cigar(cigar) if isinstance(cigar, str) else cigar
    t, q, nm, run, md = pos - 1, 0, 0, 0, []
    for n, op in ops:
        if op == "M":
            for _ in range(n):
                if letters_match(seq[q], ref[t]):
                    run += 1
                else:
                    md.append(f"{run}{ref[t].upper()}")
                    run = 0
                    nm += 1
                q += 1
                t += 1
        elif op == "I":
            q += n
            nm += n
        elif op == "D":
            md.append(f"{run}^{ref[t:t + n].upper()}")
            run = 0
            t += n
            nm += n
        else:
            raise AssertionError(op)
    assert q == len(seq), (q, len(seq))
    md.append(str(run))
    return nm, "".join(md)


def rebuild_reference(seq, cigar, md):
    """The reference span that SEQ + CIGAR + MD describe, with '=' where MD only says "the read's letter" -- resolved from SEQ -- so the
    result can be compared with the FASTA letter by letter (through the 4-bit codes, where MD says "match")."""
    assert MD_RE.match(md), md
    ops = bl.parse_cigar(cigar) if isinstance(cigar, str) else cigar
    # MD as a stream over reference columns: ('=',) a match, ('X', letter) a mismatch, ('D', letter) a deleted base
    stream = []
    for num, letters in re.findall(r"([0-9]+)|(\^[A-Z]+|[A-Z])", md):
        if num:
            stream += [("=",)] * int(num)
        elif letters.startswith("^"):
            stream += [("D", c) for c in letters[1:]]
        else:
            stream.append(("X", letters))
    out, q, k = [], 0, 0
    for n, op in ops:
        if op == "M":
            for _ in range(n):
                s = stream[k]
                assert s[0] in "=X", (md, k, s)
                out.append((s[0], seq[q] if s[0] == "=" else s[1]))
                q += 1
                k += 1
        elif op == "I":
            q += n
        elif op == "D":
            for _ in range(n):
                assert stream[k][0] == "D", (md, k, stream[k])
                out.append(("D", stream[k][1]))
                k += 1
    assert k == len(stream) and q == len(seq), (md, k, len(stream), q, len(seq))
    return out


def check_against_fasta(ref, pos, seq, cigar, md):
    """the inverse check: the rebuilt span against the FASTA"""
    span = rebuild_reference(seq, cigar, md)
    for i, (kind, letter) in enumerate(span):
        have = ref[pos - 1 + i]
        if kind == "=":
            assert letters_match(letter, have), (i, letter, have)
        else:
            assert letter == have.upper(), (i, kind, letter, have)  # a mismatch or a deleted base: MD names the FASTA's letter


def split_fields(line):
    if isinstance(line, bytes):
        line = line.decode("latin-1")
    f = line.rstrip("\n").split("\t")
    tags, order = {}, []
    for x in f[11:]:
        tag, typ, val = x.split(":", 2)
        assert tag not in tags, line
        tags[tag] = (typ, val)
        order.append(tag)
    return "\t".join(f[:11]), tags, order


def check_sam_record(line, fasta, want_tags, rg_id, score=None):
    """One tagged SAM line against the rules.  want_tags: subset of {"NM","MD","AS"} asked for.  -> the line with its fields cut off"""
    base, tags, order = split_fields(line)
    f = base.split("\t")
    mapped = f[2] != "*"
    expect = [t for t in FIELD_ORDER if (t in want_tags and mapped) or (t == "RG" and rg_id is not None)]
    assert order == expect, (order, expect, line[:100])
    if rg_id is not None:
        assert tags["RG"] == ("Z", rg_id)
    if mapped and ({"NM", "MD"} & set(want_tags)):
        nm, md = calmd(fasta[f[2]], int(f[3]), f[5], f[9])
        if "NM" in want_tags:
            assert tags["NM"] == ("i", str(nm)), (tags["NM"], nm, line[:100])
        if "MD" in want_tags:
            assert tags["MD"] == ("Z", md), (tags["MD"], md, line[:100])
            assert MD_RE.match(md)
            check_against_fasta(fasta[f[2]], int(f[3]), f[9], f[5], tags["MD"][1])
    if mapped and "AS" in want_tags:
        assert tags["AS"][0] == "i"
        if score is not None:
            assert int(tags["AS"][1]) == int(score), (tags["AS"], score)
    return base


INT_TYPES = {"c": ("<b", 1), "C": ("<B", 1), "s": ("<h", 2), "S": ("<H", 2), "i": ("<i", 4), "I": ("<I", 4)}


def smallest_int_type(v):
    """what htslib picks for an integer aux value"""
    if v >= 0:
        return "C" if v <= 0xFF else "S" if v <= 0xFFFF else "I"
    return "c" if v >= -128 else "s" if v >= -32768 else "i"


def parse_aux(data):
    """aux bytes -> [(tag, type, value)]; only the types this project writes (integers and Z)"""
    out, at = [], 0
    while at < len(data):
        assert at + 3 <= len(data), "truncated aux field"
        tag, typ = data[at:at + 2].decode("latin-1"), chr(data[at + 2])
        at += 3
        if typ in INT_TYPES:
            fmt, n = INT_TYPES[typ]
            assert at + n <= len(data)
            out.append((tag, typ, struct.unpack_from(fmt, data, at)[0]))
            at += n
        elif typ == "Z":
            end = data.index(b"\0", at)
            out.append((tag, typ, data[at:end].decode("latin-1")))
            at = end + 1
        else:
            raise AssertionError(f"aux type {typ!r}")
    return out


def read_bam_records_aux(data, refs):
    """BAM records that may carry aux fields -> [(SAM line as bam_lib reads the record without them, [(tag, type, value)])].
    block_size must cover exactly the record and its aux fields."""
    out, at = [], 0
    while at < len(data):
        assert at + 36 <= len(data), "truncated record"
        block_size, _, _, l_name, _, _, n_cig, _, l_seq = struct.unpack_from("<IiiBBHHHI", data, at)
        core = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        assert block_size >= core and at + 4 + block_size <= len(data), (at, block_size, core)
        rec = struct.pack("<I", core) + data[at + 4:at + 4 + core]
        lines = bl.read_bam_records(rec, refs)
        out.append((lines[0], parse_aux(data[at + 4 + core:at + 4 + block_size])))
        at += 4 + block_size
    assert at == len(data)
    return out


def aux_of_sam_fields(tags, order):
    """the aux fields a tagged SAM line's optional fields become in BAM"""
    out = []
    for t in order:
        typ, val = tags[t]
        if typ == "i":
            out.append((t, smallest_int_type(int(val)), int(val)))
        else:
            out.append((t, "Z", val))
    return out


# ---- hand-made alignments: the smallest shapes at which a 64-column walk can go wrong (shared by the CPU and the GPU tests) ----
COMP = str.maketrans("ACGTRYNacgtryn", "TGCAYRNtgcayrn")
OTHER = str.maketrans("ACGT", "CATG")  # a letter that differs from the given one


def revcomp(s):
    return s.translate(COMP)[::-1]


def hand_store(n=90000, seed=7):
    """a sequence store of plain letters with a few marked places: 'N' at 1000..1199, 'R' at 2000..2009, lower case at 3000..3199"""
    import random
    rng = random.Random(seed)
    s = [rng.choice("ACGT") for _ in range(n)]
    s[1000:1200] = "N" * 200
    s[2000:2010] = "R" * 10
    s[3000:3200] = [c.lower() for c in s[3000:3200]]
    return "".join(s)


def hand_case(store, name, coord, runs, edits=None, plus=True, lower=()):
    """runs: [(n, op)] in CIGAR letters as the PATH has them (before the dangling-M polish).  The printed SEQ copies the reference in M
    runs except at `edits` {alignment column of the read: letter}, and is 'T's in I runs; `lower`: read columns printed in lower case.
    -> dict(name, coord, plus, read = the bytes as they lie in the FASTQ file, path = product path ops)"""
    edits = edits or {}
    seq, t = [], coord
    for n, op in runs:
        if op == "M":
            seq += list(store[t:t + n])
            t += n
        elif op == "I":
            seq += ["T"] * n
        else:
            t += n
    for col, letter in edits.items():
        seq[col] = letter
    for col in lower:
        seq[col] = seq[col].lower()
    printed = "".join(seq)
    ops = []
    for n, op in runs:
        code = {"M": 0, "I": 1, "D": 2}[op]  # path D (query only) prints as CIGAR I and the other way round
        while n > 0:
            k = min(n, 14000)
            ops.append((k << 2) | code)
            n -= k
    return {"name": name, "coord": coord, "plus": plus, "read": printed if plus else revcomp(printed), "ops": ops, "printed": printed}


def hand_cases(store):
    c = []
    for n in (1, 63, 64, 65, 127, 128, 129):
        c.append(hand_case(store, f"cols{n}", 5000, [(n, "M")]))
        c.append(hand_case(store, f"cols{n}_mm_ends", 5000, [(n, "M")],
                           {0: store[5000].translate(OTHER), n - 1: store[5000 + n - 1].translate(OTHER)}))
    mm = lambda cols, base=6000: {k: store[base + k].upper().translate(OTHER) for k in cols}
    c.append(hand_case(store, "mm_0_63_64_last", 6000, [(200, "M")], mm([0, 63, 64, 199])))
    c.append(hand_case(store, "run_across_step_and_I", 6000, [(10, "M"), (7, "I"), (150, "M")], mm([3])))  # 6 + 150 matches print as one number
    c.append(hand_case(store, "D_then_mismatch", 6000, [(40, "M"), (2, "D"), (60, "M")], {40: store[6042].translate(OTHER)}))
    c.append(hand_case(store, "starts_with_D", 6000, [(1, "M"), (6, "D"), (100, "M")]))   # polished: 6D101M, MD starts 0^
    c.append(hand_case(store, "starts_with_I", 6000, [(2, "M"), (6, "I"), (100, "M")]))   # polished: 6I102M
    c.append(hand_case(store, "ends_with_D", 6000, [(100, "M"), (6, "D"), (2, "M")]))
    c.append(hand_case(store, "N_against_N", 1050, [(70, "M")]))
    c.append(hand_case(store, "R_against_R", 1990, [(40, "M")]))
    c.append(hand_case(store, "A_against_R", 1990, [(40, "M")], {12: "A"}))
    c.append(hand_case(store, "lower_case_read", 6000, [(70, "M")], lower=range(5, 70, 3)))
    letters = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"  # every letter a FASTQ line may hold, against plain bases and against R
    c.append(hand_case(store, "every_letter", 6000, [(104, "M")], {k: letters[k % 52] for k in range(104)}))
    c.append(hand_case(store, "every_letter_at_R", 1996, [(60, "M")], {k: letters[k % 52] for k in range(60)}))
    c.append(hand_case(store, "lower_case_store", 2990, [(130, "M")], mm([20, 64], 2990)))
    c.append(hand_case(store, "minus", 6000, [(30, "M"), (3, "I"), (50, "M"), (4, "D"), (47, "M")], mm([0, 29, 70]), plus=False))
    c.append(hand_case(store, "minus_cols65", 6100, [(65, "M")], mm([64], 6100), plus=False))
    runs = []
    for k in range(60):  # 120 runs: more than the 96 a fast kernel's path holds
        runs += [(9, "M"), (1, "I" if k % 2 else "D")]
    c.append(hand_case(store, "many_runs", 7000, runs + [(9, "M")]))
    for n in (255, 256, 65535, 65536, 70000):  # NM in every width of the BAM integer types; 70 000 all-mismatch columns
        edits = {k: store[10000 + k].translate(OTHER) for k in range(n)}
        c.append(hand_case(store, f"nm{n}", 10000, [(n, "M")], edits))
    return c


def hand_batch(cases):
    """-> (bases uint8, offs uint64, results as the product's dtype fields dict list, ops uint16) in numpy, for the api calls"""
    import numpy as np
    from urmap_amd import api
    bases = np.frombuffer("".join(x["read"] for x in cases).encode(), dtype=np.uint8)
    offs = np.zeros(len(cases) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x["read"]) for x in cases])
    res = np.zeros(len(cases), dtype=api.RESULT_DTYPE)
    ops = []
    for i, x in enumerate(cases):
        res["dbpos"][i] = x["coord"]; res["coord"][i] = x["coord"]; res["seq_index"][i] = 0
        res["plus"][i] = 1 if x["plus"] else 0; res["mapq"][i] = 30; res["score"][i] = (-3 * i) if i % 2 else 37 * i
        whole = len(x["ops"]) == 1 and (x["ops"][0] & 3) == 0
        if not whole:  # (a path of one M run is what a result without a path says)
            res["path_off"][i] = len(ops); res["path_nops"][i] = len(x["ops"])
            ops += x["ops"]
    return bases, offs, res, np.array(ops, dtype=np.uint16)


def read_bam_aux(data):
    """uncompressed BAM bytes whose records may carry aux fields -> (header text, [(name, length)], read_bam_records_aux of the rest)"""
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<I", data, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<I", data, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", data, at)
        at += 8 + l_name
    text, refs, none = bl.read_bam(data[:at])
    assert none == []
    return text, refs, read_bam_records_aux(data[at:], refs), data[at:]
