"""Duplicate marking, host side: urmapx_bam_sort_markdup_host against the model of tests/markdup_lib.py (rules 1-7 of "Duplicate
marking" in include/urmapx.h) -- hand-made records, one property a test, then seeded random records with large groups --, its refusals,
and urmapx_map_files with markdup set through the stand-alone sanitizer program (the device stand-in marks with the host function)."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
import markdup_lib as ml
from test_bam_sort_cpu import SAN_ENV, check_sorted_file, san, tiny  # noqa: F401  (san is a fixture)
from urmap_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

Q = lambda q, n=20: bytes([q]) * n  # noqa: E731
R = ml.rec


def places(members, bai, in_front=0):
    f = sl.BgzfFile(b"\0" * in_front + members + api.BGZF_EOF)
    return sl.index_in_places(sl.parse_bai(bai), sl.member_places(f, in_front))


def host(recs, n_ref=3):
    """the marked host sort of these records, checked against the plain host sort and the model -> (is record i of the INPUT flagged on
    output, the report)"""
    raw = b"".join(recs)
    members, bai, rep = api.bam_sort_host(raw, n_ref, report=True, markdup=True)
    plain, plain_bai = api.bam_sort_host(raw, n_ref)
    want, _ = ml.check(raw, bl.inflate(members), bl.inflate(plain), rep)
    # the index: the same in places of the stream (its bytes hold compressed offsets, which follow the flags' bytes once a second member
    # exists); with one member the bytes themselves
    assert places(members, bai) == places(plain, plain_bai)
    if len(raw) < sl.MEMBER:
        assert bai == plain_bai
    return want, rep


def counters(rep):
    return rep["pairs_examined"], rep["pairs_duplicate"], rep["fragments_examined"], rep["fragments_duplicate"]


# ---- ends ----
def test_forward_strand_leading_clips_move_the_end():
    recs = [R(0, 100, 0, "20M", Q(30)), R(0, 105, 0, "5S15M", Q(40)), R(0, 110, 0, "3H7S10M", Q(35)), R(0, 105, 0, "15M5S", Q(50))]
    assert [ml.end5(r)[1] for r in recs] == [100, 100, 100, 105]
    dup, rep = host(recs)
    assert dup == [True, False, True, False] and counters(rep) == (0, 0, 4, 2)


def test_reverse_strand_trailing_clips_move_the_end():
    recs = [R(0, 100, 16, "20M", Q(30)), R(0, 100, 16, "15M5S", Q(40)), R(0, 100, 16, "10M4S6H", Q(35)), R(0, 100, 16, "5S20M", Q(50)),
            R(0, 119, 0, "20M", Q(60))]  # (leading clips do not move a reverse end; a forward read at 119 is another end)
    assert [ml.end5(r)[1:] for r in recs] == [(119, 1), (119, 1), (119, 1), (119, 1), (119, 0)]
    dup, rep = host(recs)
    assert dup == [True, True, True, False, False] and counters(rep) == (0, 0, 5, 3)


def test_an_end_in_front_of_the_reference():
    recs = [R(0, 0, 0, "5S15M", Q(30)), R(0, 2, 0, "7S13M", Q(40)), R(0, 0, 0, "20M", Q(20))]
    assert [ml.end5(r)[1] for r in recs] == [-5, -5, 0]
    dup, _ = host(recs)
    assert dup == [True, False, False]


def test_a_trailing_clip_moves_a_reverse_read_into_another_group():
    recs = [R(0, 100, 16, "30M", Q(30, 30)), R(0, 100, 16, "20M", Q(30)), R(0, 100, 16, "20M10S", Q(20, 30))]
    dup, _ = host(recs)
    assert dup == [False, False, True]


def test_reference_consuming_ops():
    recs = [R(1, 100, 16, "10M2D10M", Q(30)), R(1, 100, 16, "5=5X2I12N", Q(31, 12)), R(1, 100, 16, "22M", Q(29, 22)),
            R(1, 100, 16, "10M2I10M", Q(50)),                      # (an insertion spans nothing: the end is 119)
            R(1, 100, 0, "2I18M", Q(30)), R(1, 100, 0, "20M", Q(20))]  # (nor is it a clip)
    assert [ml.end5(r)[1] for r in recs] == [121, 121, 121, 119, 100, 100]
    dup, _ = host(recs)
    assert dup == [True, True, False, False, False, True]


def test_a_record_without_a_reference_consuming_op():
    recs = [R(0, 100, 0, "", Q(30)), R(0, 105, 0, "5S", Q(20, 5)), R(0, 100, 16, "", Q(30)), R(0, 95, 16, "5S", Q(20, 5)), R(0, 100, 16, "1M", Q(10, 1))]
    assert [ml.end5(r)[1:] for r in recs] == [(100, 0), (100, 0), (100, 1), (100, 1), (100, 1)]
    dup, _ = host(recs)
    assert dup == [False, True, False, True, True]


# ---- scores ----
def test_the_score_counts_qualities_from_15_on_and_not_0xff():
    recs = [R(0, 7, 0, "20M", Q(14, 100)), R(0, 7, 0, "20M", Q(15, 2)), R(0, 7, 0, "20M", Q(0xFF, 10))]
    assert [ml.score(r) for r in recs] == [0, 30, 0]
    assert host(recs)[0] == [True, False, True]
    assert host([recs[0], recs[2]])[0] == [False, True] and host([recs[2], recs[0]])[0] == [False, True]


def test_a_tie_goes_to_the_first_in_the_input():
    recs = [R(0, 7, 0, "20M", Q(30), b"a"), R(0, 7, 0, "20M", Q(30), b"b"), R(0, 7, 0, "20M", Q(20, 30), b"c")]
    assert host(recs)[0] == [False, True, True]


def test_no_bases():
    recs = [R(0, 7, 0, "20M", b""), R(0, 7, 0, "20M", Q(15, 1)), R(0, 9, 0, "20M", b""), R(0, 9, 0, "20M", b"")]
    assert host(recs)[0] == [True, False, False, True]


# ---- pairs ----
def pair(name, a, b, qa=Q(30), qb=Q(30), fa=0, fb=0):
    """a, b: (ref, pos, reverse)"""
    return [R(a[0], a[1], 0x41 | fa | (16 if a[2] else 0), "20M", qa, name), R(b[0], b[1], 0x81 | fb | (16 if b[2] else 0), "20M", qb, name)]


def test_fr_and_rf_share_a_key():
    recs = pair(b"p", (0, 100, 0), (0, 200, 1)) + pair(b"q", (0, 200, 1), (0, 100, 0), qa=Q(40))
    dup, rep = host(recs)
    assert dup == [True, True, False, False] and counters(rep) == (2, 1, 0, 0)


def test_pairs_that_share_one_end_only():
    recs = pair(b"p", (0, 100, 0), (0, 200, 1)) + pair(b"q", (0, 100, 0), (0, 201, 1)) + pair(b"s", (0, 99, 0), (0, 200, 1))
    dup, rep = host(recs)
    assert not any(dup) and counters(rep) == (3, 0, 0, 0)


def test_mates_split_by_another_record_are_fragments():
    a, b = pair(b"p", (0, 100, 0), (0, 200, 1))
    dup, rep = host([a, R(0, 300, 0, "20M", Q(30), b"x"), b])
    assert not any(dup) and counters(rep) == (0, 0, 3, 0)


def test_names_that_differ_in_the_last_byte():
    a, _ = pair(b"ab1", (0, 100, 0), (0, 200, 1))
    _, b = pair(b"ab2", (0, 100, 0), (0, 200, 1))
    _, c = pair(b"ab", (0, 100, 0), (0, 200, 1))  # (and a name that is a prefix of the other)
    for second in (b, c):
        assert counters(host([a, second])[1]) == (0, 0, 2, 0)


def test_a_record_belongs_to_one_pair():
    a, b = pair(b"p", (0, 100, 0), (0, 200, 1))
    # 0x40 0x80 0x80: (0, 1) is the pair, the third record a fragment at a pair member's end
    dup, rep = host([a, b, b])
    assert dup == [False, False, True] and counters(rep) == (1, 0, 1, 1)
    # 0x40 0x40 0x80: (1, 2) is the pair
    dup, rep = host([a, a, b])
    assert dup == [True, False, False] and counters(rep) == (1, 0, 1, 1)
    # a record with both bits is no first mate
    both_bits = R(0, 100, 0xC1, "20M", Q(30), b"p")
    assert counters(host([both_bits, b])[1]) == (0, 0, 2, 0)
    assert counters(host([a, both_bits])[1]) == (1, 0, 0, 0)


def test_a_pair_with_an_unmapped_mate_is_a_fragment():
    a, b = pair(b"p", (0, 100, 0), (0, 100, 0), fa=0x8, fb=0x4)
    lone = R(0, 100, 0, "20M", Q(20), b"x")
    dup, rep = host([a, b, lone])
    assert dup == [False, False, True] and counters(rep) == (0, 0, 2, 1)


def test_a_fragment_at_a_pair_members_end_is_flagged_whatever_its_score():
    recs = pair(b"p", (0, 100, 0), (0, 200, 1), qa=Q(15, 1), qb=Q(15, 1)) + [R(0, 100, 0, "20M", Q(60, 200), b"x"), R(0, 200, 16, "20M", Q(60, 200), b"y"),
                                                                                R(0, 100, 16, "20M", Q(20), b"z")]  # (the other strand: another end)
    dup, rep = host(recs)
    assert dup == [False, False, True, True, False] and counters(rep) == (1, 0, 3, 2)


# ---- flags ----
def test_ineligible_records_keep_their_bytes():
    odd = [R(0, 100, 0x4 | 0x400, "20M", Q(60)), R(0, 100, 0x100 | 0x400, "20M", Q(60)), R(0, 100, 0x800 | 0x400, "20M", Q(60)), R(0, 100, 0x100, "20M", Q(60)),
           R(-1, -1, 0x4, "", Q(60))]
    recs = odd[:2] + [R(0, 100, 0, "20M", Q(30), b"k")] + odd[2:] + [R(0, 100, 0, "20M", Q(20), b"d")]
    raw = b"".join(recs)
    members, _, rep = api.bam_sort_host(raw, 3, report=True, markdup=True)
    out = [r for _, r in sl.split_records(bl.inflate(members))]
    assert all(r in out for r in odd) and counters(rep) == (0, 0, 2, 1)
    dup, _ = host(recs)
    assert dup == [True, True, False, True, False, False, True]


def test_an_incoming_flag_on_an_eligible_record_is_overwritten():
    recs = [R(0, 100, 0x400, "20M", Q(40), b"k"), R(0, 100, 0, "20M", Q(30), b"d"), R(0, 500, 0x400, "20M", Q(30), b"s")]
    assert host(recs)[0] == [False, True, False]


# ---- seeded random: large groups ----
def random_records(seed, n, n_ref=3, positions=40):
    rng = np.random.default_rng(seed)
    spots = rng.integers(0, 5000, positions)
    clips = ["", "3S", "2H3S", "7S"]
    out = []
    serial = 0

    def one(flag, name, crowded=False):
        """crowded: few ends, so that whole pairs meet"""
        rev = int(rng.integers(0, 2))
        a, b = (int(x) for x in rng.integers(0, 4, 2) * (rng.integers(0, 4, 2) == 0 if crowded else 1))
        lead, trail = clips[a], "".join(reversed([clips[b][k:k + 2] for k in (0, 2)]))
        m = int(rng.integers(18, 23))
        cig = lead + f"{m}M" + trail
        qn = m + sum(k for k, op in bl.parse_cigar(cig) if op == "S")
        q = bytes(rng.integers(10, 41, qn, dtype=np.uint8)) if rng.integers(0, 8) else Q(30, qn)
        return R(int(rng.integers(0, 2 if crowded else n_ref)), int(spots[int(rng.integers(0, 5 if crowded else positions))]), flag | (16 if rev else 0), cig, q, name)

    while len(out) < n:
        serial += 1
        kind = int(rng.integers(0, 10))
        name = b"n%d" % serial
        if kind < 4 and len(out) + 2 <= n:
            out += [one(0x41, name, True), one(0x81, name, True)]
        elif kind == 4:
            out.append(one(int(rng.choice([0x4, 0x100, 0x800, 0x404, 0x900])), name))
        elif kind == 5:
            out.append(one(int(rng.choice([0x41, 0x81, 0x400, 0xC1])), name))  # lone mates, an incoming flag
        else:
            out.append(one(0, name))
    return out


def test_seeded_random_records_with_large_groups():
    recs = random_records(1, 3000)
    dup, rep = host(recs)
    p, pd, f, fd = counters(rep)
    assert p > 400 and pd > 20 and f > 1000 and fd > 300 and len(b"".join(recs)) > 2 * sl.MEMBER
    # known record starts change nothing
    raw = b"".join(recs)
    offs = [o for o, _ in sl.split_records(raw)]
    assert api.bam_sort_host(raw, 3, markdup=True, starts=offs[::97]) == api.bam_sort_host(raw, 3, markdup=True)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_few_records(n):
    recs = [R(0, 100, 0, "20M", Q(30 - i), b"a") for i in range(n)]
    dup, rep = host(recs, 2)
    assert dup == [False, True][:n] and counters(rep) == (0, 0, n, max(0, n - 1)) and rep["records"] == n


def test_refusals_of_the_records():
    good = tiny(0, 5) + tiny(1, 7)
    for bad in (good[:-1], good + b"\x10\0\0\0" + b"\0" * 16, tiny(2, 5), tiny(-2, 5), tiny(0, -2), tiny(1, -1),
                good[:16] + struct.pack("<H", 60000) + good[18:],
                R(0, 5, 0, "20M", Q(30), l_seq=21),         # SEQ and QUAL do not lie inside the record
                R(0, 5, 0, "20M", b"", l_seq=0xFFFFFFFF)):
        with pytest.raises(api.UrmapxError) as e:
            api.bam_sort_host(bad, 2, markdup=True)
        assert e.value.code == -2, bad[:40]  # URMAPX_E_FORMAT
    api.bam_sort_host(R(0, 5, 0x4, "20M", Q(30), l_seq=21), 2, markdup=True)  # (an ineligible record's bases are not read)


def test_markdup_without_bam_sort_is_refused(tmp_path):
    ufi = str(tmp_path / "g.ufi")
    with gzip.open(os.path.join(GOLD, "g.ufi.gz"), "rb") as z, open(ufi, "wb") as f:
        f.write(z.read())
    idx = api.Index.open(ufi)
    out = str(tmp_path / "o.bam")
    with pytest.raises(api.UrmapxError) as e:
        api.map_files(idx, os.path.join(GOLD, "se150.fq"), samout=out, bam=True, markdup=True)
    assert e.value.code == -5 and "bam_sort" in str(e.value) and not os.path.exists(out)  # URMAPX_E_ARG


def test_structs_in_step_with_the_header():
    """the options as urmapx_map_files reads them: the fields up to read_group where they were, markdup appended; the report's counters
    and markdup_s at its end"""
    import ctypes as C
    full, old = api.MapOptionsMarkdup, api.MapOptions
    assert full._fields_[:-1] == old._fields_ and full._fields_[-1][0] == "markdup"
    assert all(getattr(full, n).offset == getattr(old, n).offset for n, _ in old._fields_)
    assert full.markdup.offset == C.sizeof(old) == 72 and C.sizeof(full) == 80
    assert [n for n, _ in api.MapReport._fields_][-6:] == ["sort_s", "pairs_examined", "pairs_duplicate", "fragments_examined", "fragments_duplicate", "markdup_s"]
    assert C.sizeof(api.MarkdupStats) == 40
    header = open(os.path.join(ROOT, "include", "urmapx.h")).read()
    opts = header[header.index("typedef struct urmapx_map_options"):header.index("} urmapx_map_options;")]
    assert opts.rindex("int markdup;") > opts.rindex("const char *read_group;")
    # the estimator: 24 bytes a record more than the sort alone
    L = api.lib()
    for fn in (L.urmapx_bam_sort_device_bytes, L.urmapx_bam_sort_markdup_device_bytes):
        fn.restype, fn.argtypes = C.c_uint64, [C.c_size_t, C.c_uint64]
    a, b = L.urmapx_bam_sort_device_bytes(10 ** 9, 4 * 10 ** 6), L.urmapx_bam_sort_markdup_device_bytes(10 ** 9, 4 * 10 ** 6)
    assert 24 * 4 * 10 ** 6 <= b - a <= 24 * 4 * 10 ** 6 + (1 << 20)


# ---- urmapx_map_files with markdup set: the stand-alone sanitizer program ----
def with_copies(fq_bytes, n_low=40, n_high=10, per=4):
    """the reads and behind them a copy of the first n_low with new names and every quality lowered by 10, and of the next n_high with
    raised qualities (the copy wins)"""
    lines = fq_bytes.split(b"\n")
    out = []
    for k in range(n_low + n_high):
        name, seq, plus, qual = lines[per * k:per * k + 4]
        shift = -10 if k < n_low else 5
        word = name.split()[0]
        out += [word[:1] + b"copy%d_" % k + word[1:] + name[len(word):], seq, plus, bytes(min(126, max(35, c + shift)) for c in qual)]
    return b"\n".join(lines[:-1] + out) + b"\n"


@pytest.mark.parametrize("extra", [[], ["-batch", "64", "-streams", "3"]])
def test_pipeline_markdup_under_asan(tmp_path, san, extra):  # noqa: F811
    fq = str(tmp_path / "in.fq")
    with open(fq, "wb") as f:
        f.write(with_copies(open(os.path.join(GOLD, "se150.fq"), "rb").read()))
    env = dict(os.environ, **SAN_ENV)
    paths = {k: str(tmp_path / (k + ".bam")) for k in ("plain", "sorted", "marked")}
    for k, flag in (("plain", ["-bam"]), ("sorted", ["-bam", "-sort"]), ("marked", ["-bam", "-sort", "-markdup"])):
        r = subprocess.run([san["asan"], "map", fq, "-o", paths[k], "-biglen", "500000000"] + extra + flag, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    blob = {k: open(p, "rb").read() for k, p in paths.items()}
    inflated, _, _, recs, _ = check_sorted_file(blob["sorted"], open(paths["sorted"] + ".bai", "rb").read(), blob["plain"], option=None)
    marked = bl.inflate(blob["marked"])
    head = len(inflated) - sum(len(x) for _, x in recs)
    assert marked[:head] == inflated[:head]
    text, refs, _ = bl.read_bam(bl.inflate(blob["plain"]))
    unsorted = bl.inflate(blob["plain"])[len(bl.bam_header(text, refs)):]
    want, cnt = ml.check(unsorted, marked[head:], inflated[head:])
    assert f"markdup pairs={cnt['pairs_examined']} pair_dups={cnt['pairs_duplicate']} fragments={cnt['fragments_examined']} fragment_dups={cnt['fragments_duplicate']}\n" in r.stdout
    # every mapped read among the 50 copied ones shares its end with its copy: a group of k records has k - 1 flagged
    mapped = sum(1 for f in ml.flags_of(unsorted)[:50] if not f & 4)
    assert mapped >= 10 and sum(want) >= mapped
    r = subprocess.run([san["asan"], "map", fq, "-o", paths["marked"] + "2", "-bam", "-markdup"], env=env, capture_output=True, text=True)
    assert "rc=-5" in r.stdout and "bam_sort" in r.stdout and not os.path.exists(paths["marked"] + "2")
