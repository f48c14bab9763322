"""GPU tests of -markdup: the marking on the device (markdup.hip) against the host function and against the model of
tests/markdup_lib.py -- record counts at the edges of a wavefront, of a workgroup's tile and of a whole grid, the shapes groups take,
the width of the packed ends, the shapes records take, the slices --, and `urmap ... -bamout out.bam -sort -markdup` through its roads."""
import os
import re

import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
import markdup_lib as ml
from test_bam_sort_cpu import check_sorted_file
from test_gpu_bam_sort import MAX_BLOCKS, TILE, TINY, _run, golden  # noqa: F401  (golden is a fixture)
from test_markdup_cpu import Q, R, counters, pair, places, with_copies

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STATS = ("pairs_examined", "pairs_duplicate", "fragments_examined", "fragments_duplicate")


def both(records, n_ref):
    """the marked device sort and the marked host sort of the same records: the same inflated stream, counters and index in places
    -> (the stream, the device's report)"""
    from urmap_amd import api
    dm, dbai, drep = api.bam_sort(records, n_ref, device=0, report=True, markdup=True)
    hm, hbai, hrep = api.bam_sort_host(records, n_ref, report=True, markdup=True)
    stream = bl.inflate(dm)
    assert stream == bl.inflate(hm), "the device's stream differs from the host's"
    for k in ("stream_bytes", "records", "no_coor") + STATS:
        assert drep[k] == hrep[k], (k, drep[k], hrep[k])
    assert places(dm, dbai) == places(hm, hbai), "the device's index differs from the host's"
    return stream, drep


def full(recs, n_ref=3):
    """device = host = model; only bit 0x400 differs from the device sort without the option -> (is record i of the input flagged, report)"""
    from urmap_amd import api
    raw = b"".join(recs) if isinstance(recs, list) else recs
    stream, rep = both(raw, n_ref)
    want, _ = ml.check(raw, stream, bl.inflate(api.bam_sort(raw, n_ref)[0]), rep)
    return want, rep


# ---- grid edges: tiny records, few ends ----
def tiny_mixed(n, seed):
    """38-byte records (the name "a", no CIGAR, no bases: every score is 0, so ties decide alone) with ends from 3 x 8 x 2 values, flags
    that make pairs of neighbours (all names are equal), lone mates, ineligible records and incoming 0x400 bits; record i carries i in tlen"""
    rng = np.random.default_rng(seed)
    a = np.zeros(n, TINY)
    a["block_size"], a["l_name"], a["name"] = 34, 2, b"a"
    a["ref"] = rng.integers(0, 3, n)
    a["pos"] = rng.integers(0, 8, n) * 1000
    a["bin"] = 4681
    a["flag"] = rng.choice([0, 16, 0x41, 0x81, 0x51, 0x91, 0x4, 0x400, 0x410, 0x904, 0xC1], n)
    a["next_ref"], a["next_pos"], a["tlen"] = -1, -1, np.arange(n)
    return a.tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, TILE + 1])
def test_device_equals_host_and_model_at_the_edges_of_the_grid(n):
    dup, rep = full(tiny_mixed(n, n))
    if n >= 257:
        p, pd, f, fd = counters(rep)
        assert p > 0 and f > n // 4 and fd > f // 2


def test_device_equals_host_beyond_one_tile_a_workgroup():
    """MAX_BLOCKS * TILE + 1 records: every workgroup of a sort pass walks more than one tile.  Device against host here; the model
    (too slow for this many) on the first 5 000 of them as an input of their own"""
    n = MAX_BLOCKS * TILE + 1
    records = tiny_mixed(n, 7)
    stream, rep = both(records, 3)
    p, pd, f, fd = counters(rep)
    assert p > n // 40 and pd > p // 2 and fd > f // 2  # (48 ends: nearly everything is a duplicate)
    flags = np.frombuffer(stream, TINY)["flag"]
    assert ((flags & 0x400) != 0).sum() >= 2 * pd + fd
    full(records[:5000 * 38])


# ---- group shapes ----
def test_one_group_of_all_records():
    rng = np.random.default_rng(2)
    recs = [R(0, 500, 0, "20M", bytes(rng.integers(10, 41, 20, dtype=np.uint8)), b"r%d" % i) for i in range(1000)]
    dup, rep = full(recs)
    assert sum(dup) == 999 and counters(rep) == (0, 0, 1000, 999)


def test_all_groups_of_size_one():
    recs = [R(i % 3, 10 * i, 16 * (i % 2), "20M", Q(30), b"r%d" % i) for i in range(1000)]
    dup, rep = full(recs)
    assert not any(dup) and counters(rep) == (0, 0, 1000, 0)


def test_all_scores_equal():
    recs = [R(0, 100 * (i % 7), 0, "20M", Q(30), b"r%d" % i) for i in range(1000)]
    dup, rep = full(recs)
    assert [i for i, d in enumerate(dup) if not d] == list(range(7)) and counters(rep) == (0, 0, 1000, 993)


@pytest.mark.parametrize("what", ["pairs", "fragments", "mix"])
def test_pairs_fragments_and_fragments_at_pair_ends(what):
    rng = np.random.default_rng(4)
    recs = []
    for i in range(500):
        q = lambda: bytes(rng.integers(10, 41, 20, dtype=np.uint8))  # noqa: E731
        a, b = (0, 100 * int(rng.integers(0, 6)), 0), (0, 5000 + 100 * int(rng.integers(0, 6)), 1)
        if what == "pairs" or (what == "mix" and i % 2):
            recs += pair(b"p%d" % i, *((a, b) if i % 3 else (b, a)), qa=q(), qb=q())
        else:
            recs += [R(*a[:2], 0, "20M", q(), b"f%d" % i), R(*b[:2], 16, "20M", q(), b"g%d" % i)]
    dup, rep = full(recs)
    p, pd, f, fd = counters(rep)
    if what == "pairs":
        assert (p, f) == (500, 0) and pd >= 500 - 36
    elif what == "fragments":
        assert (p, f) == (0, 1000) and fd == 1000 - 12
    else:
        assert (p, f) == (250, 500) and fd == 500  # (every end holds a member of a pair)


# ---- the width of the packed end ----
def test_ends_beyond_32_bits_and_pair_keys_beyond_64():
    top = (1 << 31) - 200
    recs = (pair(b"a", (5, 1000, 0), (200, top, 1)) + pair(b"b", (5, 1000, 0), (201, top, 1)) +    # agree in the low end, differ in the high end's reference
            pair(b"c", (5, 1000, 0), (200, top, 1), qa=Q(20)) +                                     # a duplicate of a
            pair(b"d", (256, top, 1), (5, 1000, 0), qa=Q(20)) + pair(b"e", (5, 1000, 0), (256, top, 1)) +
            [R(0, 0, 0, "5S15M", Q(30), b"f"), R(0, 3, 0, "8S12M", Q(20), b"g"),                    # u5 = -5
             R(256, top, 16, "100M99S", Q(30, 199), b"h"), R(256, top + 99, 16, "100M", Q(40, 100), b"i")])  # reverse ends beyond the largest pos
    assert ml.end5(recs[-1])[1] == top + 198 == ml.end5(recs[-2])[1] and ml.end5(recs[-3])[1] == -5
    dup, rep = full(recs, 257)
    assert dup == [False, False, False, False, True, True, True, True, False, False, False, True, False, True]
    assert counters(rep) == (5, 2, 4, 2)


# ---- record shapes ----
def test_record_shapes():
    """QUAL at every address residue and across 64-byte steps, l_seq around a wavefront's width, names of 1 and 254 bytes, 1 and 300
    CIGAR ops, aux fields behind QUAL (which are not qualities)"""
    rng = np.random.default_rng(9)
    long_cigar = "1M1I" * 149 + "1M1S"  # 300 ops, 150 reference bases; forward end at pos, reverse end at pos + 150
    assert len(bl.parse_cigar(long_cigar)) == 300
    recs = []
    for l_seq in (0, 1, 63, 64, 65, 300):
        for name in (b"n", b"nn", b"nnn", b"nnnn", b"N" * 254):
            for cig in ("150M", long_cigar):
                for copy in range(2):
                    q = rng.integers(0, 61, l_seq, dtype=np.uint8)
                    q[rng.integers(0, 4, l_seq) == 0] = 0xFF
                    recs.append(R(1, 700, 16 * (len(recs) % 2), cig, bytes(q), name, aux=b"NMC\x07XZZ" + b"\xfe" * int(rng.integers(0, 9)) + b"\0"))
    raw = b"".join(recs)
    offs = [o for o, _ in sl.split_records(raw)]
    qual_at = [o + 36 + ml.core(r)[2] + 4 * ml.core(r)[3] + (ml.core(r)[5] + 1) // 2 for o, r in sl.split_records(raw)]
    assert set(o % 4 for o in offs) == {0, 1, 2, 3} and set(q % 4 for q in qual_at) == {0, 1, 2, 3}
    dup, rep = full(recs)
    assert counters(rep) == (0, 0, len(recs), len(recs) - 3)  # (forward at 700; reverse at 849 and, with the trailing clip, at 850)
    assert len(set(ml.score(r) for r in recs)) > 60


# ---- slices ----
def test_flagged_records_cross_slice_cuts(monkeypatch):
    rng = np.random.default_rng(3)
    recs = [R(0, 1000 * int(rng.integers(0, 300)), 0, "%dM" % (40 + i % 7), bytes(rng.integers(20, 41, 40 + i % 7, dtype=np.uint8)), b"r%d" % i) for i in range(4000)]
    raw = b"".join(recs)
    whole, rep = both(raw, 1)
    assert rep["slices"] == 1 and len(raw) > 5 * sl.MEMBER
    monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
    sliced, rep1 = both(raw, 1)
    assert rep1["slices"] == -(-len(raw) // sl.MEMBER) > 1 and sliced == whole
    ml.check(raw, sliced, ml.mask_dup(whole), rep1)
    cuts = [k * sl.MEMBER for k in range(1, rep1["slices"])]
    flagged = [(o, r) for o, r in sl.split_records(whole) if ml.core(r)[4] & ml.DUP]
    assert any(o < c < o + len(r) for c in cuts for o, r in flagged), "no flagged record straddles a slice's end"


# ---- the golden inputs through the command line ----
RG_ARG = "@RG\\tID:grp.1\\tSM:s1"
VARIANTS = {"plain": [], "streams": ["-streams", "3", "-batch", "64"], "host": ["-host"], "tags": ["-tags", "NM,MD,AS", "-rg", RG_ARG]}


def split_file(blob):
    """a BAM file -> (offset of its first record member, the inflated record stream), aux fields or not"""
    data = bl.inflate(blob)
    l_text, = np.frombuffer(data, "<u4", 1, 4)
    at = 8 + int(l_text)
    n_ref, = np.frombuffer(data, "<u4", 1, at)
    at += 4
    for _ in range(int(n_ref)):
        l_name, = np.frombuffer(data, "<u4", 1, at)
        at += 8 + int(l_name)
    f = sl.BgzfFile(blob)
    return f.member(0)[1], data[at:], int(n_ref)


@pytest.fixture(scope="module")
def inputs(golden):  # noqa: F811
    d = golden["dir"]
    se = os.path.join(d, "md_se.fq")
    open(se, "wb").write(with_copies(open(os.path.join(GOLD, "se150.fq"), "rb").read()))
    pe = [os.path.join(d, "md_pe_%d.fq" % k) for k in (1, 2)]
    for k, path in zip((1, 2), pe):
        open(path, "wb").write(with_copies(open(os.path.join(GOLD, "pe120_rep_%d.fq" % k), "rb").read()))
    return {"se": ["-map", se, "-ufi", golden["g"]], "pe": ["-map2", pe[0], "-reverse", pe[1], "-ufi", golden["r"]]}


@pytest.fixture(scope="module")
def marked_plain(golden, inputs):  # noqa: F811
    """kind -> the inflated records of `-sort -markdup` with no further option (made once)"""
    made = {}

    def get(kind):
        if kind not in made:
            path = os.path.join(golden["dir"], f"md_{kind}_reference.bam")
            _run(inputs[kind] + ["-quiet", "-bamout", path, "-sort", "-markdup"])
            made[kind] = split_file(open(path, "rb").read())[1]
        return made[kind]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", ["se", "pe"])
def test_cli(golden, inputs, marked_plain, kind, variant):  # noqa: F811
    from urmap_amd import api
    args, extra = inputs[kind], VARIANTS[variant]
    paths = {k: os.path.join(golden["dir"], f"md_{kind}_{variant}_{k}.bam") for k in ("unsorted", "sorted", "marked")}
    _run(args + ["-quiet", "-bamout", paths["unsorted"]] + extra)
    _run(args + ["-quiet", "-bamout", paths["sorted"], "-sort"] + extra)
    r = _run(args + ["-bamout", paths["marked"], "-sort", "-markdup"] + extra)
    blob = {k: open(p, "rb").read() for k, p in paths.items()}
    if variant != "tags":  # (the yardstick's reader of whole files takes no optional fields)
        check_sorted_file(blob["sorted"], open(paths["sorted"] + ".bai", "rb").read(), blob["unsorted"])
    _, unsorted, n_ref = split_file(blob["unsorted"])
    _, plain, _ = split_file(blob["sorted"])
    in_front, marked, _ = split_file(blob["marked"])
    # the marked file: the plain one's records but for bit 0x400, the cuts of a sorted file, an index that holds, the model's flags
    want, cnt = ml.check(unsorted, marked, plain)
    f = sl.BgzfFile(blob["marked"])
    assert blob["marked"].endswith(api.BGZF_EOF)
    sizes = [s for _, s in f.members(in_front)][:-1]
    assert all(s == sl.MEMBER for s in sizes[:-1]) and 0 < sizes[-1] <= sl.MEMBER and sum(sizes) == len(marked)
    sl.check_index(sl.parse_bai(open(paths["marked"] + ".bai", "rb").read()), sl.split_records(marked), sl.member_places(f, in_front), n_ref)
    m = re.search(rb"Seconds to mark duplicates: (\d+) of (\d+) pairs, (\d+) of (\d+) fragments", r.stderr)
    assert m, r.stderr
    assert tuple(int(x) for x in m.groups()) == (cnt["pairs_duplicate"], cnt["pairs_examined"], cnt["fragments_duplicate"], cnt["fragments_examined"])
    assert sum(want) >= 40
    assert (cnt["pairs_examined"] > 100) == (kind == "pe")
    # the inflated records do not depend on the road
    if variant in ("streams", "host"):
        assert marked == marked_plain(kind), variant


def test_cli_refusals(golden, inputs):  # noqa: F811
    out, sam = os.path.join(golden["dir"], "md_no.bam"), os.path.join(golden["dir"], "md_no.sam")
    for args, word in ((["-bamout", out, "-markdup"], b"-sort"), (["-samout", sam, "-sort", "-markdup"], b"-bamout"), (["-samout", sam, "-markdup"], b"-sort")):
        r = _run(["-map", os.path.join(GOLD, "se150.fq"), "-ufi", os.path.join(golden["dir"], "no_such.ufi"), "-quiet"] + args, ok=False)
        # (the index does not exist: the refusal comes before it is opened)
        assert r.returncode != 0 and word in r.stderr and b"no_such" not in r.stderr and len(r.stderr.strip().split(b"\n")) == 2, r.stderr
        assert r.stdout == b"" and not os.path.exists(out) and not os.path.exists(out + ".bai") and not os.path.exists(sam)
