"""BAM output, host side: the yardstick's own self-check (tests/bam_lib.py against values taken from the specification), then the
host encoders urmapx_bam_se / _pe / _header against it -- fed with the oracle's hits they must give the bytes bam_lib makes of the
reference-written SAM goldens --, the edge records, and urmapx_map_files with bam set under the sanitizer builds."""
import gzip
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import oracle_lib as ol
from test_abi_cpu import oracle_results_as_product
from test_bgzf_cpu import EOF_MEMBER, walk_bgzf
from urmap_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SAN_DIR = os.path.join(ROOT, "urmap_amd", "csrc", "build_san")


def gold(name):
    p = os.path.join(GOLD, name)
    if os.path.exists(p):
        return open(p, "rb").read()
    with gzip.open(p + ".gz", "rb") as z:  # the alpha fixtures are kept .gz
        return z.read()


@pytest.fixture(scope="module")
def ufis(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_ufi")
    out = {}
    for name in ("g", "r"):
        out[name] = os.path.join(d, name + ".ufi")
        with gzip.open(os.path.join(GOLD, name + ".ufi.gz"), "rb") as z, open(out[name], "wb") as f:
            f.write(z.read())
    return out


def fastq_arrays(name, tmp_path):
    p = os.path.join(GOLD, name)
    if not os.path.exists(p):
        p = os.path.join(tmp_path, name)
        open(p, "wb").write(gold(name))
    return api.read_fastq_arrays(p)


# ---- the yardstick ----
def test_bam_lib_against_the_specification():
    # section 5.3: bin 4681 is the first 16 kb bin, 4680 what reg2bin gives an unplaced read (-1, 0)
    assert bl.reg2bin(0, 1) == 4681
    assert bl.reg2bin(-1, 0) == 4680
    assert bl.reg2bin(0, 1 << 14) == 4681 and bl.reg2bin((1 << 14) - 1, 1 << 14) == 4681
    # a region across a 16 kb boundary lands in the parent (128 kb) bin, 585 + (beg >> 17)
    assert bl.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585
    assert bl.reg2bin(5 * (1 << 17) + (1 << 14) - 10, 5 * (1 << 17) + (1 << 14) + 10) == 585 + 5
    assert bl.reg2bin(0, 1 << 29) == 0
    # one record assembled by hand from the field table of section 4.2:
    #   r1  0  chr1  100  40  4M  *  0  0  ACGT  IIII
    by_hand = bytes.fromhex(
        "2d000000"              # block_size 45 = 32 + 3 + 4 + 2 + 4
        "00000000" "63000000"   # refID 0, pos 99
        "03" "28" "4912"        # l_read_name 3, mapq 40, bin 4681
        "0100" "0000"           # n_cigar_op 1, flag 0
        "04000000"              # l_seq
        "ffffffff" "ffffffff"   # next_refID, next_pos
        "00000000"              # tlen
        "723100"                # r1\0
        "40000000"              # 4M
        "1248"                  # A=1 C=2 | G=4 T=8
        "28282828")             # 'I' - 33
    line = "r1\t0\tchr1\t100\t40\t4M\t*\t0\t0\tACGT\tIIII"
    assert bl.sam_to_bam_records(line + "\n", ["chr1"]) == by_hand
    assert bl.read_bam_records(by_hand, [("chr1", 1000)]) == [line]
    # unplaced, odd length, lower case and a letter outside the table, no qualities
    rec = bl.sam_to_bam_records("q\t4\t*\t0\t0\t*\t*\t0\t0\tacn?u\t*\n", [])
    assert rec[4:12] == b"\xff" * 8 and struct.unpack_from("<H", rec, 14)[0] == 4680
    assert rec[-8:] == bytes([0x12, 0xFF, 0xF0]) + b"\xff" * 5
    assert bl.read_bam_records(rec, []) == ["q\t4\t*\t0\t0\t*\t*\t0\t0\tACNNN\t*"]
    # header block
    hdr = bl.bam_header("@SQ\tSN:c\tLN:7\n", [("c", 7)])
    assert hdr == b"BAM\1" + struct.pack("<I", 14) + b"@SQ\tSN:c\tLN:7\n" + struct.pack("<II", 1, 2) + b"c\0" + struct.pack("<I", 7)
    assert bl.read_bam(hdr + by_hand.replace(b"chr1", b"c")) [:2] == (b"@SQ\tSN:c\tLN:7\n", [("c", 7)])
    # the reader refuses what is wrong
    for bad in (by_hand[:-1], by_hand[:14] + b"\x00\x00" + by_hand[16:], by_hand[:38] + b"x" + by_hand[39:]):
        with pytest.raises(AssertionError):
            bl.read_bam_records(bad, [("chr1", 1000)])


# ---- the host encoders against the reference's goldens ----
def refs_of(idx):
    return [(name, length) for name, length, _ in idx.directory()]


@pytest.mark.parametrize("name", ["se150", "se250", "se_short", "se_alpha"])
def test_bam_se_equals_the_golden_sam_in_bam(ufis, tmp_path, name):
    labels, bases, offs, quals = fastq_arrays(name + ".fq", tmp_path)
    ores, opaths, _ = ol.Index.load(ufis["g"]).map_se(bases, offs)
    res, ops = oracle_results_as_product(ores, opaths)
    idx = api.Index.open(ufis["g"])
    got = idx.bam_se(res, ops, labels, bases, offs, quals)
    want_sam = gold(name + ".sam")
    assert got == bl.sam_to_bam_records(want_sam, refs_of(idx))
    assert bl.read_bam_records(got, refs_of(idx)) == bl.sam_records(want_sam)


@pytest.mark.parametrize("name,ufi", [("pe150", "g"), ("pe100_noisy", "g"), ("pe120_rep", "r"), ("pe_alpha", "g")])
def test_bam_pe_equals_the_golden_sam_in_bam(ufis, tmp_path, name, ufi):
    labels, bases, offs, quals = api.interleave_pairs(fastq_arrays(name + "_1.fq", tmp_path), fastq_arrays(name + "_2.fq", tmp_path))
    ores, opaths, _ = ol.Index.load(ufis[ufi]).map_pe(bases, offs)
    res, ops = oracle_results_as_product(ores, opaths)
    idx = api.Index.open(ufis[ufi])
    got = idx.bam_pe(res, ops, labels, bases, offs, quals)
    want_sam = gold(name + ".sam")
    assert got == bl.sam_to_bam_records(want_sam, refs_of(idx))
    assert bl.read_bam_records(got, refs_of(idx)) == bl.sam_records(want_sam)


@pytest.mark.parametrize("ufi", ["g", "r"])
def test_bam_header_block(ufis, ufi):
    idx = api.Index.open(ufis[ufi])
    cl = "urmap -map x.fq -ufi i.ufi -bamout o.bam "
    block = idx.bam_header(cl)
    text, refs, records = bl.read_bam(block)
    assert records == [] and refs == refs_of(idx) and len(refs) >= 1
    assert text == idx.sam_header_sq() + b"@PG\tID:urmap\tPN:urmap\tVN:1.0.mi355x\tCL:" + cl.encode() + b"\n"
    assert bl.refs_of_header(text) == refs
    assert block == bl.bam_header(text, refs)


# ---- hand-made records ----
def dummy_index(length=400, name="c"):
    seq = np.frombuffer(b"ACGT" * 100, dtype=np.uint8)  # (the encoders read the directory, not the sequence bytes)
    blob = np.zeros(5 * 101 + 8, dtype=np.uint8)
    return api.Index.wrap_host(24, 32, 101, blob, seq, [length], [0], [name])


def one_record(idx, path, L, coord=0, plus=1, mapped=True, label="r", bases=None, quals=None, both=False):
    """a read of L bases with this path through bam_se and sam_se -> (BAM record bytes, SAM line)"""
    res = np.zeros(1, dtype=api.RESULT_DTYPE)
    ops = np.zeros(0, dtype=np.uint16)
    if mapped:
        res["dbpos"] = coord; res["seq_index"] = 0; res["coord"] = coord; res["plus"] = plus; res["mapq"] = 37
        _, ops = oracle_results_as_product(np.array([(0, 0, 0, 0, 0, 0, 0, 0, 1, 6, len(path), 0)], dtype=ol.RESULT_DTYPE), [path])
        res["path_nops"] = len(ops)
    else:
        res["dbpos"] = 0xFFFFFFFF; res["seq_index"] = 0xFFFFFFFF
    b = np.full(L, 65, np.uint8) if bases is None else np.frombuffer(bases, dtype=np.uint8)
    q = np.full(L, 73, np.uint8) if quals is None else np.frombuffer(quals, dtype=np.uint8)
    offs = np.array([0, L], np.uint64)
    return idx.bam_se(res, ops, [label], b, offs, q), idx.sam_se(res, ops, [label], b, offs, q).decode("latin-1").rstrip("\n")


def cigar_of(rec):
    return bl.read_bam_records(rec, [("c", 1 << 30)])[0].split("\t")[5]


def test_cigar_dangling_m_rules_in_bam():
    """the hand-made paths of test_abi_cpu.test_cigar_dangling_m_rules: the ops of the BAM record are the ops the text prints"""
    idx = dummy_index()
    for path, L, want in (("M" * 1 + "D" * 6 + "M" * 100, 107, "6I101M"), ("M" * 100 + "I" * 6 + "M" * 2, 102, "102M6D"),
                          ("M" * 3 + "D" * 6 + "M" * 100, 109, "3M6I100M"), ("M" * 2 + "D" * 4 + "M" * 100, 106, "2M4I100M"),
                          ("M" * 1 + "D" * 6 + "M" * 100 + "I" * 6 + "M" * 1, 108, "6I101M6D1M"), ("", 150, "150M")):
        rec, line = one_record(idx, path, L)
        assert line.split("\t")[5] == want
        assert cigar_of(rec) == want
        assert rec == bl.sam_to_bam_records(line + "\n", ["c"])


def test_edge_records():
    idx = dummy_index()
    refs = [("c", 400)]
    # unmapped
    rec, line = one_record(idx, "", 5, mapped=False, bases=b"ACGTN", quals=b"!#5I~")
    assert rec == bl.sam_to_bam_records(line + "\n", refs)
    assert bl.read_bam_records(rec, refs) == ["r\t4\t*\t0\t0\t*\t*\t0\t0\tACGTN\t!#5I~"]
    # odd and even l_seq, both strands (packing meets reversal), l_seq 1
    for L in (1, 2, 7, 8, 63, 64, 65):
        for plus in (1, 0):
            bases = (b"ACGTTGCAAC" * 7)[:L]
            quals = bytes(33 + (3 * i) % 60 for i in range(L))
            rec, line = one_record(idx, "", L, plus=plus, bases=bases, quals=quals)
            assert rec == bl.sam_to_bam_records(line + "\n", refs), (L, plus)
            assert bl.read_bam_records(rec, refs) == [line]
            assert len(rec) == 36 + 2 + 4 + (L + 1) // 2 + L
    # QNAME: 254 bytes pass (l_read_name 255), 255 are an error that names the read; "/1" and what follows a blank do not count
    for label in ("n" * 254, "n" * 254 + "/1", "n" * 254 + " comment"):
        rec, line = one_record(idx, "", 4, label=label)
        assert rec[12] == 255 and rec == bl.sam_to_bam_records(line + "\n", refs)
    with pytest.raises(api.UrmapxError) as e:
        one_record(idx, "", 4, label="n" * 255)
    assert "254" in str(e.value) and "nnnn" in str(e.value)


@pytest.mark.parametrize("level", [14, 17, 20, 23, 26])
def test_span_across_a_bin_boundary(level):
    """a record whose reference span crosses a boundary of the bins of this level lands in the bin above; one base short of the
    boundary it stays below"""
    idx = dummy_index(1 << 28)
    edge = 3 << level if level < 26 else 1 << 26
    refs = [("c", 1)]
    for coord, L in ((edge - 10, 20), (edge - 20, 20), (edge, 20)):
        rec, line = one_record(idx, "M" * 8 + "I" * 5 + "M" * (L - 8), L, coord=coord)  # a deletion: the span is L + 5
        assert rec == bl.sam_to_bam_records(line + "\n", refs), (coord, L)
        bin_ = struct.unpack_from("<H", rec, 14)[0]
        assert bin_ == bl.reg2bin(coord, coord + L + 5)
    crossing = struct.unpack_from("<H", one_record(idx, "", 20, coord=edge - 10)[0], 14)[0]
    below = struct.unpack_from("<H", one_record(idx, "", 20, coord=edge - 20)[0], 14)[0]
    assert crossing != below and crossing == bl.reg2bin(edge - 10, edge + 10) and below == bl.reg2bin(edge - 20, edge)
    first_of_level = {14: 4681, 17: 585, 20: 73, 23: 9, 26: 1}
    assert below >= first_of_level[level] and crossing < first_of_level[level]


# ---- urmapx_map_files with bam set, host side under the sanitizer builds ----
@pytest.fixture(scope="module")
def san():
    if not shutil.which("g++"):
        pytest.skip("no g++ for the sanitizer builds")
    r = subprocess.run(["make", "-s", "-j3", "-C", os.path.join(ROOT, "urmap_amd", "csrc"), "san"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    return {k: os.path.join(SAN_DIR, "urmap_san_" + k) for k in ("asan", "tsan")}


@pytest.mark.parametrize("build,extra", [("asan", []), ("asan", ["-shards", "2"]), ("asan", ["-batch", "64", "-streams", "3"]),
                                         ("asan", ["-2"]), ("tsan", ["-batch", "64", "-streams", "3"])])
def test_pipeline_bam_under_sanitizers(tmp_path, san, build, extra):
    """header block, lane chunks (the device stand-in runs the host encoders), end-of-file member, shards: every file is a complete
    BAM whose records are the plain run's SAM records"""
    paired = "-2" in extra
    fq = os.path.join(GOLD, "pe150_1.fq" if paired else "se150.fq")
    extra = ["-2", os.path.join(GOLD, "pe150_2.fq")] if paired else extra
    env = dict(os.environ, URX_STUB_MAP="1", ASAN_OPTIONS="exitcode=99:detect_leaks=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1",
               TSAN_OPTIONS="exitcode=99")
    plain, bam = str(tmp_path / "p.sam"), str(tmp_path / "o.bam")
    extra = extra + ["-biglen", "500000000"]  # (the stand-in index's largest sequence, inside the 2^29 bases the BAM bins cover)
    for out, flag in ((plain, []), (bam, ["-bam"])):
        r = subprocess.run([san[build], "map", fq, "-o", out] + extra + flag, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    shards = 2 if "-shards" in extra else 0
    names = [f".{s}" for s in range(shards)] if shards else [""]
    text = b"".join(open(plain + s, "rb").read() for s in names)
    got = []
    for s in names:
        blob = open(bam + s, "rb").read()
        assert blob.endswith(EOF_MEMBER)
        walk_bgzf(blob)
        htext, refs, lines = bl.read_bam(bl.inflate(blob))
        assert bl.refs_of_header(htext) == refs and bl.sam_header(text).startswith(bl.sam_header(htext).split("@PG")[0])
        got += lines
    assert got == bl.sam_records(text) and len(got) >= 400
    # bam and bgzf together are refused
    r = subprocess.run([san[build], "map", fq, "-o", bam, "-bam", "-bgzf"] + extra, env=env, capture_output=True, text=True)
    assert "rc=-5" in r.stdout and "always BGZF" in r.stdout, r.stdout + r.stderr
