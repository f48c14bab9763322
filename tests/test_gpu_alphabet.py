"""GPU: letters other than upper-case ACGT, in single reads and in BOTH mates of a pair, on every road through the kernels.

The search kernels set a read up in one of three ways (dev_common.h: acgt_pick / comp_char + seq_code / q_other), the pair kernel
per mate; tests/alphabet_lib.py makes reads and mates in tagged letter classes (N at the ends and in runs, lower case, IUPAC, U / u,
letters without a complement, reads that keep the store's own N and -- on an index whose store kept the FASTA's case -- its lower
case).  Everything is compared bit for bit with the oracle, which test_oracle_golden.py pins to the reference binary on the same
classes; no read or pair is left out of a comparison.  Before the device runs, each case asserts on the oracle's results alone that
it is not vacuous (alphabet_lib.check_classes / check_pair_kinds): >= 20 mapped reads or mates per class that can map, >= 20
unmapped all-lower-case reads, >= 90 % of the case-kept reads on lower-cased stretches exact at their own position (the oracle
reaches 100 %: 57 of 57 single reads, 33 of 33 mates on the 300 kbp genome), all nine (plain, four-plane, other)^2 mate combinations
>= 10 times, >= 30 proper pairs with a non-plain mate 2.
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

import alphabet_lib as al
import oracle_lib as ol
import test_gpu_parity as tp
import test_gpu_slow as ts
from conftest import reads_to_arrays
from test_gpu_parity import dense_case, gpu, rescue_case  # noqa: F401  (fixtures; small_case comes from conftest.py)
from urmap_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "urmap_amd", "urmap")


@pytest.fixture(scope="module")
def store(small_case):
    return al.Store(small_case["oracle_index"], small_case["fasta"])


@pytest.fixture(scope="module")
def soft_case(small_case, workdir):
    """small_case's index with the FASTA's case put back into the sequence store: lower case has to match lower case"""
    oi = al.soft_masked_index(small_case["oracle_index"], small_case["fasta"])
    ufi = os.path.join(workdir, "soft.ufi")
    oi.save(ufi)
    return {"oracle_index": oi, "ufi": ufi, "store": al.Store(oi, small_case["fasta"])}


def se_case(oi, st, seed, read_len, n, method=6, min_exact=al.MIN_PER_CLASS, **kw):
    """reads in the letter classes + the oracle's results, with the conditions on them asserted"""
    reads, tags = al.make_reads(seed, st, n, read_len=read_len, **kw)
    bases, offs = reads_to_arrays(reads)
    ores, opaths, _ = oi.map_se(bases, offs, method=method, threads=4)
    cc = al.check_classes(tags, ores, np.diff(offs.astype(np.int64)), min_exact=min_exact)
    print(f"single-end {read_len}: (reads, mapped) per class {cc}")
    return bases, offs, ores, opaths, tags


def pe_case(oi, st, tmp_path, seed, rl, n, veryfast=False, **kw):
    """pairs in the letter classes as FASTQ files + the oracle's SAM, with the conditions on it asserted"""
    r1, r2, t1, t2 = al.make_pairs(seed, st, n, read_len=rl, **kw)
    f1, f2, osam = (os.path.join(tmp_path, x) for x in ("r1.fq", "r2.fq", "o.sam"))
    synth.write_fastq(f1, r1)
    synth.write_fastq(f2, r2)
    oi.map_file_pe(f1, f2, osam, threads=4, veryfast=veryfast)
    want = open(osam, "rb").read()
    combos, proper = al.check_pair_kinds(t1, t2, want)
    bases, offs = reads_to_arrays([x for ab in zip(r1, r2) for x in ab])
    ores, _, _ = oi.map_pe(bases, offs, threads=4, veryfast=veryfast)
    cc = al.check_classes([x for ab in zip(t1, t2) for x in ab], ores, np.diff(offs.astype(np.int64)), classes=kw.get("classes", al.CLASSES))
    for k in ("four", "other"):  # each non-plain kind in mate 2 alone
        assert sum(1 for a, b in zip(t1, t2) if a["kind"] == "plain" and b["kind"] == k) >= 10
    print(f"pairs {rl}: per (kind, kind) {combos}; proper with a non-plain mate 2 {proper}; (mates, mapped) per class {cc}")
    return f1, f2, want


def same_sam(got, want):
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        raise AssertionError(f"{len(bad)} differing records of {len(w)}, first: {g[bad[0]][:220]!r} vs {w[bad[0]][:220]!r}")


# ---------------------------------------------------------------------------------------------------------------------------
# single-end
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_len,no_k2", [(150, False), (150, True), (152, False), (250, False), (400, False)])  # 150: the two-chunk instance (and without it), 152: three chunks
def test_se_letter_classes_match_oracle(small_case, store, gpu, monkeypatch, read_len, no_k2):
    if no_k2:
        monkeypatch.setenv("URMAPX_NO_K2", "1")
    bases, offs, ores, opaths, _ = se_case(small_case["oracle_index"], store, 7000 + read_len, read_len, 2800, sub=0.01, indel=0.001)
    gres, gops = gpu["mapper"].map_se(bases, offs)
    tp.compare_results(gres, gops, ores, opaths)


def test_se_letter_classes_method7_on_a_maxix3_index(small_case, tmp_path):
    oi = ol.Index.build(small_case["fasta"], 524309, max_ix=3)
    ufi = os.path.join(tmp_path, "vf.ufi")
    oi.save(ufi)
    bases, offs, ores, opaths, _ = se_case(oi, al.Store(oi, small_case["fasta"]), 7007, 150, 2800, method=7, sub=0.02, indel=0.002)
    m = api.Mapper(api.Index.open(ufi).upload(0), device=0, method=7)
    gres, gops = m.map_se(bases, offs)
    tp.compare_results(gres, gops, ores, opaths)


def test_se_letter_classes_with_phase3_parked(small_case, store, monkeypatch):
    monkeypatch.setenv("URMAPX_PARK_PHASE3", "1")  # read at upload (the row layout stays) and at every call
    m = api.Mapper(api.Index.open(small_case["ufi"]).upload(0), device=0)
    bases, offs, ores, opaths, _ = se_case(small_case["oracle_index"], store, 7003, 150, 2800, sub=0.01, indel=0.004)
    gres, gops = m.map_se(bases, offs)
    tp.compare_results(gres, gops, ores, opaths)
    _, st = m.phase3()
    assert st[1] > 50 and st[0] >= st[1], st  # reads did park at phase 3


def test_se_letter_classes_on_a_store_that_kept_case(soft_case):
    """lower case against lower case, N against N: a four-plane compare that never lets a == a match would fail here"""
    c = soft_case
    bases, offs, ores, opaths, tags = se_case(c["oracle_index"], c["store"], 7011, 150, 2800, sub=0.01, indel=0.001)
    assert sum(1 for t in tags if t["cls"] == "case_kept" and t["lower"] and t["kind"] == "four") >= 40
    m = api.Mapper(api.Index.open(c["ufi"]).upload(0), device=0)
    gres, gops = m.map_se(bases, offs)
    tp.compare_results(gres, gops, ores, opaths)


def test_long_reads_in_letter_classes_go_through_the_general_kernel(small_case, store, monkeypatch):
    """1 100 .. 2 000 bases: beyond the fast kernels (1 024).  With the general kernel switched off every one of them stays flagged
    (status != 0): it is the general kernel that maps them."""
    # the penalty cap is absolute (state1.cpp:152-179): a long read maps only if it is nearly exact
    bases, offs, ores, opaths, _ = se_case(small_case["oracle_index"], store, 7013, (1100, 2000), 560, min_exact=10, sub=0.002, indel=0.0002)  # 40 case_kept reads
    idx = api.Index.open(small_case["ufi"]).upload(0)
    m = api.Mapper(idx, device=0)
    monkeypatch.setenv("URMAPX_TEST_NO_GENERAL", "1")
    flagged, _ = m.map_se(bases, offs, allow_unsupported=True)
    assert (flagged["status"] != 0).all()
    monkeypatch.delenv("URMAPX_TEST_NO_GENERAL")
    g, gops = m.map_se(bases, offs)
    ts._compare(g, gops, ores, opaths)


# ---------------------------------------------------------------------------------------------------------------------------
# pairs: the classes of the two mates drawn independently
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rl,n,env,veryfast", [(150, 1500, {}, False), (250, 1000, {}, False),
                                               (150, 1500, {"URMAPX_TEST_HSP_LDS_CAP": "64"}, False),  # the later tiers
                                               (150, 1000, {"URMAPX_TEST_PE_GENERAL": "1"}, False),  # every pair again in the general pair kernel
                                               (150, 1500, {}, True), (150, 1000, {"URMAPX_TEST_PE_GENERAL": "1"}, True)])
def test_pe_letter_classes_match_oracle(small_case, store, tmp_path, monkeypatch, rl, n, env, veryfast):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f1, f2, want = pe_case(small_case["oracle_index"], store, tmp_path, 8000 + rl + len(env) + 2 * veryfast, rl, n, veryfast=veryfast)
    same_sam(tp._map_pe_sam(small_case["ufi"], f1, f2, veryfast=veryfast), want)


def test_pe_letter_classes_on_the_dense_index(dense_case, tmp_path):
    oi = dense_case["oracle_index"]
    f1, f2, want = pe_case(oi, al.Store(oi), tmp_path, 8101, 150, 1500, classes=tuple(c for c in al.CLASSES if c != "case_kept"))
    same_sam(tp._map_pe_sam(dense_case["ufi"], f1, f2), want)


def test_pe_letter_classes_on_a_store_that_kept_case(soft_case, tmp_path):
    f1, f2, want = pe_case(soft_case["oracle_index"], soft_case["store"], tmp_path, 8103, 150, 1500)
    same_sam(tp._map_pe_sam(soft_case["ufi"], f1, f2), want)


RESCUE_CLASSES = ("n_mid", "n_first", "n_last", "lower_stretch", "iupac_upper", "iupac_lower", "U_for_T", "u_for_t", "no_complement")


@pytest.mark.parametrize("which", ["rescued", "anchor"])
@pytest.mark.parametrize("general", [False, True])
def test_pe_rescue_scan_with_a_non_plain_mate(rescue_case, monkeypatch, which, general):
    """rescue_case (the mate in the 60-copy repeat can only be placed by State2::ScanPair) with the letter classes in the mate that
    is rescued, and in the mate that anchors the scan: the oracle's counters say the scan still produces hits, every mate's result
    equals the oracle's"""
    if general:
        monkeypatch.setenv("URMAPX_TEST_PE_GENERAL", "1")
    c = rescue_case
    rng = np.random.default_rng(5)
    reads = list(c["reads"])
    changed = []
    for j in range(len(reads) // 2):
        rep = 2 * j + 1 if j % 2 == 0 else 2 * j  # the fixture's repeat mate: mate 2 of the even pairs, mate 1 of the odd ones
        k = rep if which == "rescued" else rep ^ 1
        lab, s, q = reads[k]
        cls = RESCUE_CLASSES[j % len(RESCUE_CLASSES)]
        s = al.apply_class(rng, s, cls)
        if cls == "lower_stretch":  # one short stretch: the mate still has to be placed
            s = reads[k][1].copy()
            s[40:52] |= 0x20
        reads[k] = (lab, s, q)
        changed.append(k)
    bases, offs = reads_to_arrays(reads)
    ores, opaths, cnt = c["oracle_index"].map_pe(bases, offs)
    assert cnt["n_scan"] >= 50 and cnt["n_scan_hits"] >= 30, cnt
    assert (ores["dbpos"][changed] != 0xFFFFFFFF).sum() >= 40, (ores["dbpos"][changed] != 0xFFFFFFFF).sum()
    assert {al.kind_of(reads[k][1]) for k in changed} == {"four", "other"}
    m = api.Mapper(api.Index.open(c["ufi"]).upload(0), device=0)
    g, gops = m.map_pe(bases, offs)
    ts._compare_pe(g, gops, ores, opaths)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's own bytes (tests/golden/se_alpha, pe_alpha), through the library and through the command line
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def gold_ufi(tmp_path):
    p = os.path.join(tmp_path, "g.ufi")
    with gzip.open(os.path.join(GOLD, "g.ufi.gz"), "rb") as z, open(p, "wb") as f:
        f.write(z.read())
    return p


def _alpha(name, tmp_path=None):
    """an alpha fixture (kept .gz): its bytes, or -- with tmp_path -- the path of an unpacked copy"""
    with gzip.open(os.path.join(GOLD, name + ".gz"), "rb") as z:
        data = z.read()
    if tmp_path is None:
        return data
    p = os.path.join(tmp_path, name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _records(data, drop=b"@PG"):
    return [l for l in data.split(b"\n") if l and not l.startswith(drop)]


def test_device_sam_of_the_alpha_goldens_is_the_references(gold_ufi, tmp_path):
    idx = api.Index.open(gold_ufi).upload(0)
    m = api.Mapper(idx, device=0)
    sam, rep = m.map_text_se(_alpha("se_alpha.fq"))
    assert rep["reason"] == api.TEXT_OK and rep["records"] == 560, rep
    assert _records(sam) == _records(_alpha("se_alpha.sam"), b"@")
    same_sam(tp._map_pe_sam(gold_ufi, _alpha("pe_alpha_1.fq", tmp_path), _alpha("pe_alpha_2.fq", tmp_path)), _alpha("pe_alpha.sam"))


@pytest.mark.parametrize("way", ["device_text", "host_text", "gz"])
def test_cli_on_the_alpha_goldens(gold_ufi, tmp_path, way):
    """`urmap -map` and `urmap -map2 ... -tabbedout` on the device text path, with URMAPX_HOST_TEXT=1 and from .gz input: the
    reference's files (reverse-strand SEQ with '?', case kept, U -> A included)"""
    env = dict(os.environ)
    if way == "host_text":
        env["URMAPX_HOST_TEXT"] = "1"
    src = {name: os.path.join(GOLD, name + ".gz") if way == "gz" else _alpha(name, tmp_path)  # the fixtures are kept .gz
           for name in ("se_alpha.fq", "pe_alpha_1.fq", "pe_alpha_2.fq")}
    sam, tab = os.path.join(tmp_path, "o.sam"), os.path.join(tmp_path, "o.tab")
    r = subprocess.run([EXE, "-map", src["se_alpha.fq"], "-ufi", gold_ufi, "-samout", sam, "-batch", "128"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert _records(open(sam, "rb").read()) == _records(_alpha("se_alpha.sam"))
    r = subprocess.run([EXE, "-map2", src["pe_alpha_1.fq"], "-reverse", src["pe_alpha_2.fq"], "-ufi", gold_ufi, "-samout", sam,
                        "-tabbedout", tab, "-batch", "128"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(tab, "rb").read() == _alpha("pe_alpha.tab")
    assert _records(open(sam, "rb").read()) == _records(_alpha("pe_alpha.sam"))


# ---------------------------------------------------------------------------------------------------------------------------
# seed + probe: every letter at every offset of a 64-base chunk
# ---------------------------------------------------------------------------------------------------------------------------
def test_seed_probe_with_every_letter_at_every_chunk_offset(small_case, gpu):
    """52 letters x 64 offsets, read lengths 24 .. 200: slots, tallies and positions of both strands against slots_vec and the blob"""
    oi = small_case["oracle_index"]
    g0 = small_case["genome"][0][1]
    rng = np.random.default_rng(52)
    reads = []
    for li, letter in enumerate(al.ALL_LETTERS):
        for o in range(64):
            k = li * 64 + o
            L = 24 + (7 * k) % 177
            if L <= o:
                L = max(24, o + 1 + k % 30)
            lo = int(rng.integers(0, len(g0) - 256))
            s = g0[lo:lo + L].copy()
            s[o::64] = letter
            reads.append((f"l{k}", s, np.full(L, ord("I"), np.uint8)))
    assert {len(r[1]) for r in reads} >= {24, 200}
    bases, offs = reads_to_arrays(reads)
    slots, tallies, positions = gpu["mapper"].seed_probe(bases, offs)
    blob = oi.blob()
    W = oi.word_length
    none = np.iinfo(np.uint64).max
    for r, (_, seq, _) in enumerate(reads):
        L = len(seq)
        rc = np.zeros(L, np.uint8)
        ol.lib().uo_revcomp(np.ascontiguousarray(seq).ctypes.data, L, rc.ctypes.data)
        for strand, s in ((0, seq), (1, rc)):
            want = oi.slots_vec(s)
            base = 2 * int(offs[r]) + strand * L
            assert (slots[base: base + L - W + 1] == want).all(), f"read {r} strand {strand}: slots differ"
            valid = want != none
            sv = want[valid].astype(np.int64)
            wt = np.zeros(len(want), np.uint8)
            wt[valid] = blob[5 * sv]
            wp = (blob[5 * sv + 1].astype(np.uint32) | (blob[5 * sv + 2].astype(np.uint32) << 8)
                  | (blob[5 * sv + 3].astype(np.uint32) << 16) | (blob[5 * sv + 4].astype(np.uint32) << 24))
            assert (tallies[base: base + len(want)] == wt).all(), f"read {r} strand {strand}: tallies differ"
            assert (positions[base: base + len(want)][valid] == wp).all(), f"read {r} strand {strand}: positions differ"


# ---------------------------------------------------------------------------------------------------------------------------
# the Viterbi entry point on the bytes a flank window really holds
# ---------------------------------------------------------------------------------------------------------------------------
def viterbi_problems(soft_oi):
    """A from the letter classes, B from the bytes of a sequence store: lower case, N runs, the '-' pad between two sequences and the
    zero bytes behind the store.  Shapes as in test_gpu_parity.test_viterbi_matches_oracle: flanks with a 24-base margin, Left / Right
    variants, long flanks over many row blocks, the rescue's whole-read DP against a 1 024 + 2 QL window."""
    rng = np.random.default_rng(77)
    sd = np.concatenate([soft_oi.seqdata(), np.zeros(600, np.uint8)])  # the store and what lies behind it
    d = soft_oi.directory()
    pads = [off + ln for _, ln, off in d[:-1]]  # first '-' of each pad
    end = d[-1][2] + d[-1][1]
    low = np.nonzero((sd & 0x20) != 0)[0]
    nn = np.nonzero(sd == ord("N"))[0]
    pairs, flags = [], []
    k = 0
    for anchor in ("any", "lower", "n", "pad", "tail"):
        for cls in al.CLASSES:
            for la in (9, 40, 77, 140, 260):
                lb = la + 24 + (k % 2)
                if anchor == "any":
                    lo = int(rng.integers(0, end - lb))
                elif anchor == "lower":
                    lo = int(low[int(rng.integers(0, len(low)))]) - int(rng.integers(0, lb))
                elif anchor == "n":
                    lo = int(nn[int(rng.integers(0, len(nn)))]) - int(rng.integers(0, lb))
                elif anchor == "pad":
                    lo = pads[k % len(pads)] - int(rng.integers(1, lb))
                else:
                    lo = end - int(rng.integers(1, lb))
                lo = max(0, lo)
                b = sd[lo:lo + lb]
                st = 0 if k % 2 else min(24, lb - la)
                a = b[st:st + la].copy()
                if cls != "case_kept":
                    a = np.where(a == 0, ord("A"), np.where(a == ord("-"), ord("C"), a & 0xDF)).astype(np.uint8)
                    nm = int(rng.integers(0, max(1, la // 8)))
                    a[rng.integers(0, la, size=nm)] = synth.ACGT[rng.integers(0, 4, size=nm)]
                    if la > 8 and k % 3 == 0:
                        x = int(rng.integers(1, la - 3))
                        a = np.delete(a, slice(x, x + int(rng.integers(1, 3))))
                    elif la > 8 and k % 3 == 1:
                        x = int(rng.integers(1, la - 1))
                        a = np.insert(a, x, synth.ACGT[rng.integers(0, 4, size=int(rng.integers(1, 3)))])
                    a = al.apply_class(rng, a, cls) if len(a) > 2 else a
                else:
                    a = np.where((a == 0) | (a == ord("-")), ord("N"), a).astype(np.uint8)
                pairs.append((a.tobytes(), b.tobytes()))
                flags.append((1 if k % 2 == 0 else 2) if k % 5 else 3 * (k % 2))
                k += 1
    for la, lb in ((150, 1324), (250, 1524)):  # the rescue's window around an N run and over the pad
        for lo in (int(nn[len(nn) // 2]) - 700, pads[0] - 900, end - 1000):
            b = sd[max(0, lo):max(0, lo) + lb]
            st = int(rng.integers(0, lb - la))
            a = al.apply_class(rng, np.where(al._PLAIN[b[st:st + la] & 0xDF], b[st:st + la] & 0xDF, ord("G")).astype(np.uint8),
                               al.CLASSES[1 + len(pairs) % 12])
            for fl in (0, 3):
                pairs.append((a.tobytes(), b.tobytes()))
                flags.append(fl)
    return pairs, flags


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("method", [6, 7])
def test_viterbi_on_store_bytes_and_letter_classes(small_case, soft_case, monkeypatch, method, pair):
    """method 6's constants and -veryfast's (mismatch -4, gaps -6 / -2, band radius 8), one problem and two per wavefront.  The entry
    point takes its band radius from the context's parameters, which the method sets: pair -veryfast's radius 4 (set per call inside
    urmapx_map_pe_device) cannot be asked for here and is left to the end-to-end -veryfast pair cases above."""
    import itertools
    if pair:
        monkeypatch.setenv("URMAPX_VITERBI_PAIR", "1")
    else:
        monkeypatch.delenv("URMAPX_VITERBI_PAIR", raising=False)
    pairs, flags = viterbi_problems(soft_case["oracle_index"])
    joined = b"".join(b for _, b in pairs)
    assert all(x in joined for x in (b"-", b"N", b"a", b"\0")) and len(pairs) > 300
    m = api.Mapper(api.Index.open(small_case["ufi"]).upload(0), device=0, method=method)
    scores, status, paths = m.viterbi_batch(pairs, flags)
    for k, ((a, b), fl) in enumerate(zip(pairs, flags)):
        s, p = ol.viterbi(a, b, bool(fl & 1), bool(fl & 2), method=method)
        assert float(scores[k]) == s, f"case {k}: score gpu {scores[k]} oracle {s}"
        if sum(1 for _ in itertools.groupby(p)) > 96:  # more runs than URMAPX_MAX_PATH_OPS: flagged, never cut silently
            assert status[k] == 0x04, f"case {k}: status {status[k]}"
            continue
        assert status[k] == 0, f"case {k}: status {status[k]}"
        assert paths[k] == p, f"case {k}: path gpu {paths[k]} oracle {p}"
