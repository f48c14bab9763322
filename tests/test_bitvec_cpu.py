"""CPU: the k-mer bit-vector filter (-make_bitvec, -search_bitvec, -search_bitvec2) restated in numpy and checked against the
reference's outputs (tests/golden/bitvec_runs.json, written by tests/golden/make_golden_bitvec.py), against live reference runs
where oracle/_ref/urmap is built, and the command line's usage errors that stop before a device is opened."""
import hashlib
import json
import os
import re
import subprocess
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "urmap")
CLI = os.path.join(ROOT, "urmap_amd", "urmap")
RUNS = json.load(open(os.path.join(GOLD, "bitvec_runs.json")))

# g_CharToLetterNucleo (ACGTU / acgtu -> 0..3, else invalid) and g_CharToCompChar (IUPAC, case kept, 'u' and non-letters -> '?')
LETTER = np.full(256, 4, np.uint8)
for _c, _v in zip(b"ACGTUacgtu", (0, 1, 2, 3, 3, 0, 1, 2, 3, 3)):
    LETTER[_c] = _v
COMP = np.full(256, ord("?"), np.uint8)
for _a, _b in zip(b"ACGTUNRYSWKMBDHVX", b"TGCAANYRSWMKVHDBX"):
    COMP[_a] = _b
    if _a != ord("U"):
        COMP[_a | 0x20] = _b | 0x20


def as_u8(s):
    return np.frombuffer(bytes(s), dtype=np.uint8) if not isinstance(s, np.ndarray) else s.astype(np.uint8)


def revcomp(s):
    return COMP[as_u8(s)[::-1]]


def strand_words(s, W):
    """the words the reference's loop examines on one strand (valid ones only): starts 0 .. L-2W+1; none below 2W-1 bases"""
    s = as_u8(s)
    n = len(s) - 2 * W + 2
    if n <= 0:
        return np.zeros(0, np.uint64)
    lt = LETTER[s[:n + W - 1]].astype(np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(lt, W)
    ok = (win < 4).all(axis=1)
    shifts = (2 * np.arange(W - 1, -1, -1)).astype(np.uint64)
    words = ((win & np.uint64(3)) << shifts).sum(axis=1, dtype=np.uint64)
    return words[ok]


def seq_words(s, W):
    """(strand 0 words, strand 1 words): strand 1 = the sequence reverse-complemented by characters"""
    return strand_words(s, W), strand_words(revcomp(s), W)


def build_bits(seqs, excl, W):
    """Scan (makebitvec.cpp) over both strands of seqs, then of excl with clearing -> (.bv payload bytes, included, excluded)"""
    bits = np.zeros(4 ** W, dtype=bool)
    for s in seqs:
        for w in seq_words(s, W):
            bits[w] = True
    inc = int(bits.sum())
    for s in excl:
        for w in seq_words(s, W):
            bits[w] = False
    return np.packbits(bits, bitorder="little"), inc, inc - int(bits.sum())


def verdict(read, bits, W):
    """SearchBitVec1: 1 forward, 2 reverse, 0 not found"""
    lookup = lambda ws: bool(len(ws)) and bool(((bits[(ws >> np.uint64(3)).astype(np.int64)] >> (ws & np.uint64(7)).astype(np.uint8)) & 1).any())
    f, r = seq_words(read, W)
    return 1 if lookup(f) else 2 if lookup(r) else 0


def read_fasta(path):
    """SeqDB::FromFasta: records of letters (case kept), gaps / digits / blanks dropped, empty records skipped"""
    seqs, cur = [], None
    for line in open(path, "rb").read().split(b"\n"):
        line = line.rstrip(b"\r")
        if line.startswith(b">"):
            if cur:
                seqs.append(bytes(cur))
            cur = bytearray()
        elif cur is not None:
            cur += bytes(c for c in line if chr(c).isalpha())
    if cur:
        seqs.append(bytes(cur))
    return seqs


def read_fastq(path):
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def record(label, seq, qual, v, trunc):
    if trunc:
        m = re.search(rb"\s", label)
        label = label[:m.start()] if m else label
    if v != 1:  # RevCompInPlace was applied and not undone
        seq, qual = bytes(revcomp(seq)), qual[::-1]
    return b"@" + label + b"\n" + seq + b"\n+\n" + qual + b"\n" if seq else b""


def filter_se(reads, bits, W, trunc):
    out, found = [], 0
    for lab, s, q in reads:
        v = verdict(s, bits, W)
        if v:
            out.append(record(lab, s, q, v, trunc))
            found += 1
    return b"".join(out), found


def filter_pe(reads1, reads2, bits, W, trunc):
    o1, o2, found = [], [], 0
    for (l1, s1, q1), (l2, s2, q2) in zip(reads1, reads2):
        v1, v2 = verdict(s1, bits, W), verdict(s2, bits, W)
        if v1 or v2:
            o1.append(record(l1, s1, q1, v1, trunc))
            o2.append(record(l2, s2, q2, v2, trunc))
            found += 1
    return b"".join(o1), b"".join(o2), found


def sha(b):
    return hashlib.sha256(b).hexdigest()


def bv_file(bits, W):
    return struct.pack("<II", 0x42563130, W) + bits.tobytes()


@pytest.fixture(scope="module")
def fixtures():
    return {"ref": read_fasta(os.path.join(GOLD, "bv_ref.fa")), "excl": read_fasta(os.path.join(GOLD, "bv_excl.fa")),
            "r1": read_fastq(os.path.join(GOLD, "bv_r1.fq")), "r2": read_fastq(os.path.join(GOLD, "bv_r2.fq"))}


def test_restatement_of_the_loop_bound_and_strands():
    W = 12
    g = b"ACGTTGCAAGCTTGACCGTAGGCTAGCTAGGATCCA" * 3
    bits, inc, exc = build_bits([g], [], W)
    assert exc == 0 and inc > 0
    assert verdict(g[:23], bits, W) == 1 and verdict(g[:22], bits, W) == 0  # 2W-1 bases examine one word, 2W-2 none
    rnd = b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"
    assert verdict(rnd + g[:20], bits, W) == 2  # the genomic bases only at the end: found through the reverse complement
    assert verdict(g[:5], bits, W) == 0
    # 'u' has no complement letter, 'U' does
    assert len(seq_words(b"ACGu" * 8, 4)[1]) < len(seq_words(b"ACGU" * 8, 4)[1])
    assert (seq_words(b"ACGU" * 8, 4)[0] == seq_words(b"ACGT" * 8, 4)[0]).all()


@pytest.mark.parametrize("W", [8, 12, 16])
def test_restated_build_equals_reference_bv(fixtures, W):
    bits, inc, exc = build_bits(fixtures["ref"], fixtures["excl"], W)
    want = RUNS["make"][str(W)]
    data = bv_file(bits, W)
    assert len(data) == want["bytes"]
    assert (inc, exc) == (want["included"], want["excluded"])
    assert sha(data) == want["sha256"]


@pytest.mark.parametrize("trunc", [False, True])
@pytest.mark.parametrize("W", [8, 12])
def test_restated_search_equals_reference_outputs(fixtures, W, trunc):
    bits, _, _ = build_bits(fixtures["ref"], fixtures["excl"], W)
    key = f"{W}{'_trunc' if trunc else ''}"
    out, found = filter_se(fixtures["r1"], bits, W, trunc)
    assert (found, len(fixtures["r1"])) == (RUNS["search"][key]["found"], RUNS["search"][key]["reads"])
    assert sha(out) == RUNS["search"][key]["sha256"]
    o1, o2, found = filter_pe(fixtures["r1"], fixtures["r2"], bits, W, trunc)
    assert found == RUNS["search2"][key]["found"]
    assert (sha(o1), sha(o2)) == (RUNS["search2"][key]["sha256_1"], RUNS["search2"][key]["sha256_2"])


def _run_ref(args, cwd):
    r = subprocess.run([REF] + args + ["-threads", "1"], capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r.stderr


@pytest.mark.skipif(not os.path.exists(REF), reason="reference binary not built here")
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_equals_live_reference_on_random_cases(tmp_path, seed):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTACGTACGTacgtNUuRY", np.uint8)
    W = int(rng.integers(3, 11))
    seqs = [bytes(rng.choice(alpha, int(rng.integers(W - 1 if i else 100, 400)))) for i in range(5)]  # none shorter than W-1
    excl = [seqs[0][10:90], bytes(rng.choice(alpha, 60))]
    reads = []
    for i in range(150):
        s = seqs[int(rng.integers(0, 5))]
        L = int(rng.integers(W - 1, 80))
        a = int(rng.integers(0, max(1, len(s) - L)))
        r = s[a:a + L] if i % 3 else bytes(rng.choice(alpha, L))
        r = bytes(revcomp(r)).replace(b"?", b"N") if i % 2 else r
        reads.append((f"r{i} x".encode(), r, bytes(rng.integers(35, 75, len(r)).astype(np.uint8))))
    fa, ex, fq = (str(tmp_path / n) for n in ("g.fa", "e.fa", "r.fq"))
    open(fa, "wb").write(b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    open(ex, "wb").write(b"".join(b">e%d\n%s\n" % (i, s) for i, s in enumerate(excl)))
    open(fq, "wb").write(b"".join(b"@%s\n%s\n+\n%s\n" % r for r in reads))
    msg = _run_ref(["-make_bitvec", fa, "-input2", ex, "-wordlength", str(W), "-output", "x.bv"], str(tmp_path))
    bits, inc, exc = build_bits(seqs, excl, W)
    assert open(tmp_path / "x.bv", "rb").read() == bv_file(bits, W)
    assert f"{inc} words included" in msg and f"{exc} words excluded" in msg
    _run_ref(["-search_bitvec", fq, "-ref", "x.bv", "-output", "h.fq"], str(tmp_path))
    assert open(tmp_path / "h.fq", "rb").read() == filter_se(reads, bits, W, False)[0]


def test_bv_header_layout():
    bits, _, _ = build_bits([b"ACGTACGTTTGG"], [], 4)
    f = bv_file(bits, 4)
    magic, W = struct.unpack_from("<II", f)
    assert f[:4] == b"01VB" and magic == 0x42563130 and W == 4 and len(f) == 8 + 4 ** 4 // 8
    # bit n = byte[n >> 3] & (1 << (n & 7)) = bit n & 31 of little-endian uint32 word n >> 5
    n = int(strand_words(b"ACGTACGTTTGG", 4)[0])
    assert n == 0b00011011
    assert f[8 + (n >> 3)] & (1 << (n & 7))
    assert np.frombuffer(f[8:], "<u4")[n >> 5] & (1 << (n & 31))


@pytest.mark.parametrize("args, msg", [
    (["-make_bitvec", "{fa}", "-wordlength", "12", "-output", "{d}/x.bv"], "Missing input file name"),
    (["-make_bitvec", "{fa}", "-input2", "{ex}", "-wordlength", "21", "-output", "{d}/x.bv"], "-wordlength 21"),
    (["-make_bitvec", "{fa}", "-input2", "{ex}", "-wordlength", "1", "-output", "{d}/x.bv"], "-wordlength 1"),
    (["-search_bitvec", "{fq}", "-ref", "{fa}", "-output", "{d}/h.fq"], "Invalid .bv file"),
    (["-search_bitvec", "{fq}", "-ref", "{d}/w30.bv", "-output", "{d}/h.fq"], "-wordlength 30"),
    (["-search_bitvec2", "{fq}", "-ref", "{fa}", "-output1", "{d}/a", "-output2", "{d}/b"], "-reverse required"),
])
def test_cli_usage_errors_before_any_device(tmp_path, args, msg):
    if not os.path.exists(CLI):
        pytest.fail("urmap not built")
    open(tmp_path / "w30.bv", "wb").write(struct.pack("<II", 0x42563130, 30))
    sub = {"fa": os.path.join(GOLD, "bv_ref.fa"), "ex": os.path.join(GOLD, "bv_excl.fa"), "fq": os.path.join(GOLD, "bv_r1.fq"),
           "d": str(tmp_path)}
    r = subprocess.run([CLI] + [a.format(**sub) for a in args], capture_output=True, text=True)
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "x.bv")


def test_bitvec_kernels_have_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import kernel_meta
    table = kernel_meta.kernel_table(os.path.join(ROOT, "urmap_amd", "liburmapx.so"))
    bv = {k: r for k, r in table.items() if k.startswith("bv_")}
    assert sorted(bv) == ["bv_build_kernel<false>", "bv_build_kernel<true>", "bv_popcount_kernel", "bv_search_kernel"]
    for k, r in bv.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
