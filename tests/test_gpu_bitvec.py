"""GPU: the k-mer bit-vector filter on the device (urmap_amd/csrc/bitvec.hip) against the reference's outputs on the fixtures
(tests/golden/bitvec_runs.json) and against the numpy restatement of tests/test_bitvec_cpu.py."""
import gzip
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from test_bitvec_cpu import GOLD, build_bits, filter_pe, filter_se, read_fasta, revcomp, seq_words, verdict
from urmap_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "urmap_amd", "urmap")
RUNS = json.load(open(os.path.join(GOLD, "bitvec_runs.json")))
FA, EX, R1, R2 = (os.path.join(GOLD, n) for n in ("bv_ref.fa", "bv_excl.fa", "bv_r1.fq", "bv_r2.fq"))


def sha_file(p):
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


def arrays(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8) if reads else np.zeros(0, np.uint8)
    return bases, offs


def cli(args, timeout=300):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)
    return r


@pytest.mark.parametrize("W", [8, 12, 16])
def test_device_build_equals_reference_bv(tmp_path, W):
    bv = str(tmp_path / "x.bv")
    r = cli(["-make_bitvec", FA, "-input2", EX, "-wordlength", str(W), "-output", bv])
    assert r.returncode == 0, r.stderr
    want = RUNS["make"][str(W)]
    assert os.path.getsize(bv) == want["bytes"] and sha_file(bv) == want["sha256"]
    assert f"{want['included']} words included" in r.stderr and f"{want['excluded']} words excluded" in r.stderr
    assert api.make_bitvec(0, FA, EX, W, str(tmp_path / "y.bv")) == (want["included"], want["excluded"])
    assert sha_file(str(tmp_path / "y.bv")) == want["sha256"]


def test_build_of_sequences_shorter_than_w_minus_1_adds_nothing():
    W = 12
    g = read_fasta(FA)
    b1, c1 = api.BitVec.build(0, g, [], W)
    b2, c2 = api.BitVec.build(0, [b"ACG", b""] + g + [b"ACGTACGTAC"], [b"T"], W)
    assert c1 == c2 and c1[1] == 0
    assert (b1.download() == b2.download()).all()
    assert (b1.download() == build_bits(g, [], W)[0]).all()


def random_reads(rng, genome, n, lens):
    alpha = np.frombuffer(b"ACGTACGTACGTacgtNUuRY", np.uint8)
    out = []
    for i in range(n):
        L = int(rng.choice(lens))
        s = genome[int(rng.integers(0, len(genome)))]
        if i % 3 == 0 or len(s) <= L:
            r = bytes(rng.choice(alpha, L))
        else:
            a = int(rng.integers(0, len(s) - L))
            r = s[a:a + L]
            if i % 2:
                r = bytes(revcomp(r)).replace(b"?", b"N")
        out.append(r)
    return out


@pytest.mark.parametrize("W", [8, 12, 16])
def test_verdicts_equal_restatement_on_random_reads(W):
    rng = np.random.default_rng(W)
    g, ex = read_fasta(FA), read_fasta(EX)
    bits, _, _ = build_bits(g, ex, W)
    bv, _ = api.BitVec.build(0, g, ex, W)
    reads = random_reads(rng, g, 3000, [0, 1, W - 2, W - 1, 2 * W - 2, 2 * W - 1, 2 * W, 63, 64, 65, 100, 150, 151, 250])
    got = bv.search(*arrays(reads))
    want = np.array([verdict(r, bits, W) for r in reads], np.uint8)
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    assert set(np.unique(want)) >= {0, 1, 2}


def test_verdicts_on_an_asymmetric_hand_made_table():
    W = 10
    rng = np.random.default_rng(7)
    bits = np.zeros(4 ** W // 8, np.uint8)
    target = b"ACGTTGCAAGCTAGGCTTAC"
    w0 = int(seq_words(target[:2 * W - 1], W)[0][0])  # the first strand-0 word of target, alone in the table
    bits[w0 >> 3] |= 1 << (w0 & 7)
    bv = api.BitVec.wrap_host(W, bits, 0)
    assert bv.popcount() == 1 and (bv.download() == bits).all()
    fwd = target[:2 * W - 1]
    rev = bytes(revcomp(fwd))
    long5k = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000))
    long30k = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 30000))
    reads = [fwd, rev, fwd[:-1], rev[1:], b"", b"A", fwd[:W - 2], long5k + fwd, long30k + rev, rev + long30k, fwd + long5k,
             b"N" * 3000 + rev + b"N" * 3000]
    reads += [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(L))) for L in rng.integers(0, 400, 500)]
    got = bv.search(*arrays(reads))
    want = np.array([verdict(r, bits, W) for r in reads], np.uint8)
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    assert list(got[:12]) == [1, 2, 0, 0, 0, 0, 0, 1, 2, 2, 1, 2]


def test_search_device_matches_host_arrays():
    import torch
    W = 12
    g = read_fasta(FA)
    bv, _ = api.BitVec.build(0, g, [], W)
    reads = random_reads(np.random.default_rng(3), g, 2000, [150])
    bases, offs = arrays(reads)
    db = torch.from_numpy(bases.copy()).cuda()
    do = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    dv = torch.full((len(reads),), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bv.search_device(db.data_ptr(), do.data_ptr(), len(reads), dv.data_ptr())
    bv.sync()
    assert (dv.cpu().numpy() == bv.search(bases, offs)).all()
    assert bv.last_ms()[2] > 0


def _gz(src, dst):
    with open(src, "rb") as f, gzip.open(dst, "wb") as g:
        shutil.copyfileobj(f, g)
    return dst


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("trunc", [False, True])
@pytest.mark.parametrize("W", [8, 12])
def test_cli_search_outputs_equal_reference(tmp_path, W, trunc, gz):
    bv = str(tmp_path / "x.bv")
    assert cli(["-make_bitvec", FA, "-input2", EX, "-wordlength", str(W), "-output", bv]).returncode == 0
    r1 = _gz(R1, str(tmp_path / "r1.fq.gz")) if gz else R1
    r2 = _gz(R2, str(tmp_path / "r2.fq.gz")) if gz else R2
    t = ["-trunclabels"] if trunc else []
    key = f"{W}{'_trunc' if trunc else ''}"
    h = str(tmp_path / "h.fq")
    r = cli(["-search_bitvec", r1, "-ref", bv, "-output", h, "-threads", "4"] + t)
    assert r.returncode == 0, r.stderr
    want = RUNS["search"][key]
    assert sha_file(h) == want["sha256"]
    assert f"{want['found']} / {want['reads']} found" in r.stderr
    h1, h2 = str(tmp_path / "h1.fq"), str(tmp_path / "h2.fq")
    r = cli(["-search_bitvec2", r1, "-reverse", r2, "-ref", bv, "-output1", h1, "-output2", h2] + t)
    assert r.returncode == 0, r.stderr
    want = RUNS["search2"][key]
    assert (sha_file(h1), sha_file(h2)) == (want["sha256_1"], want["sha256_2"])
    assert f"{want['found']} / {want['pairs']} found" in r.stderr


def test_file_search_equals_restatement_across_batches(tmp_path):
    """more reads than one batch of the file-to-file call, so that the two batches in flight alternate"""
    W = 12
    g, ex = read_fasta(FA), read_fasta(EX)
    bits, _, _ = build_bits(g, ex, W)
    rng = np.random.default_rng(11)
    reads = random_reads(rng, g, 270000, [12, 30, 100, 150])
    recs1 = [(b"q%d x" % i, r, bytes([65 + (i % 20)]) * len(r)) for i, r in enumerate(reads)]
    recs2 = [(b"m%d" % i, r, b"I" * len(r)) for i, r in enumerate(reads[::-1])]
    p1, p2 = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(p1, "wb").write(b"".join(b"@%s\n%s\n+\n%s\n" % x for x in recs1))
    open(p2, "wb").write(b"".join(b"@%s\n%s\n+\n%s\n" % x for x in recs2))
    bv, _ = api.BitVec.build(0, g, ex, W)
    h, h1, h2 = (str(tmp_path / n) for n in ("h.fq", "h1.fq", "h2.fq"))
    v = np.array([verdict(r, bits, W) for r in reads], np.uint8)
    assert (bv.search(*arrays(reads)) == v).all()
    want, nfound = filter_se(recs1, bits, W, True)
    assert bv.search_files(p1, h, trunc_labels=True) == (nfound, len(reads))
    assert open(h, "rb").read() == want
    w1, w2, nfound = filter_pe(recs1, recs2, bits, W, False)
    assert bv.search_files(p1, h1, p2, h2) == (nfound, len(reads))
    assert open(h1, "rb").read() == w1 and open(h2, "rb").read() == w2


def test_unequal_mate_counts_are_an_error(tmp_path):
    bv = str(tmp_path / "x.bv")
    assert cli(["-make_bitvec", FA, "-input2", EX, "-wordlength", "12", "-output", bv]).returncode == 0
    short = str(tmp_path / "r2.fq")
    open(short, "wb").write(b"\n".join(open(R2, "rb").read().split(b"\n")[:8]) + b"\n")  # two records
    r = cli(["-search_bitvec2", R1, "-reverse", short, "-ref", bv, "-output1", str(tmp_path / "a"), "-output2", str(tmp_path / "b")])
    assert r.returncode == 1 and "different numbers of records" in r.stderr
    B = api.BitVec.open(bv, 0)
    with pytest.raises(api.UrmapxError) as e:
        B.search_files(R1, str(tmp_path / "a"), short, str(tmp_path / "b"))
    assert e.value.code == api.E_FORMAT


def test_open_rejects_bad_files(tmp_path):
    p = tmp_path / "bad.bv"
    p.write_bytes(struct.pack("<II", 0x42563131, 8) + bytes(8192))
    with pytest.raises(api.UrmapxError) as e:
        api.BitVec.open(str(p), 0)
    assert e.value.code == api.E_FORMAT
    p.write_bytes(struct.pack("<II", 0x42563130, 8) + bytes(100))  # shorter than 4^8/8
    with pytest.raises(api.UrmapxError) as e:
        api.BitVec.open(str(p), 0)
    assert e.value.code == api.E_FORMAT
    p.write_bytes(struct.pack("<II", 0x42563130, 21))
    with pytest.raises(api.UrmapxError) as e:
        api.BitVec.open(str(p), 0)
    assert e.value.code == api.E_UNSUPPORTED
    with pytest.raises(api.UrmapxError) as e:
        api.BitVec.build(0, [b"ACGT"], [], 21)
    assert e.value.code == api.E_UNSUPPORTED


def test_w18_build_save_open_search_round_trip(tmp_path):
    """an 8 GiB table: built, written, streamed back into HBM and searched; checked against word sets (no dense restatement)"""
    W = 18
    if shutil.disk_usage(str(tmp_path)).free < (24 << 30):
        pytest.fail("needs 24 GiB of free disk space for the 8 GiB table file")
    g, ex = read_fasta(FA), read_fasta(EX)
    words = set()
    for s in g:
        for ws in seq_words(s, W):
            words.update(int(w) for w in ws)
    inc = len(words)
    for s in ex:
        for ws in seq_words(s, W):
            words.difference_update(int(w) for w in ws)
    bv, counts = api.BitVec.build(0, g, ex, W)
    assert counts == (inc, inc - len(words))
    p = str(tmp_path / "w18.bv")
    bv.save(p)
    assert os.path.getsize(p) == 8 + 4 ** W // 8
    bv.close()
    bv2 = api.BitVec.open(p, 0)
    os.remove(p)
    assert bv2.word_length == W and bv2.popcount() == len(words)
    reads = random_reads(np.random.default_rng(18), g, 4000, [W - 2, 2 * W - 2, 2 * W - 1, 2 * W, 150, 300])

    def v(r):
        f, rr = seq_words(r, W)
        return 1 if any(int(w) in words for w in f) else 2 if any(int(w) in words for w in rr) else 0

    want = np.array([v(r) for r in reads], np.uint8)
    assert (bv2.search(*arrays(reads)) == want).all()
    assert set(np.unique(want)) >= {0, 1, 2}
