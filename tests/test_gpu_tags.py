"""GPU tests of the optional fields NM, MD, AS, RG (tags_gpu.hip): the stage-level entry point on hand-made shapes (device = host
function = the yardstick of tests/tags_lib.py), the text stage on the goldens (SAM text and raw BAM records equal the host formatters'
byte for byte, every record checked against the FASTA), each field alone, long reads and long paths, and `urmap -tags ... -rg ...`
through every output road."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_lib as bl
import bam_sort_lib as sl
import tags_lib as tl
from test_bgzf_cpu import EOF_MEMBER, walk_bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "urmap_amd", "urmap")
RG_LINE, RG_ID = "@RG\tID:grp.1\tSM:s1", "grp.1"
RG_ARG = "@RG\\tID:grp.1\\tSM:s1"
ALL = {"NM", "MD", "AS"}


def gold(name):
    p = os.path.join(GOLD, name)
    if os.path.exists(p):
        return open(p, "rb").read()
    with gzip.open(p + ".gz", "rb") as z:
        return z.read()


def recs_of(text):
    return [l for l in text.decode("latin-1").split("\n") if l and not l.startswith("@")]


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    import edges_lib as el
    import oracle_lib as ol
    from urmap_amd import api
    d = tmp_path_factory.mktemp("tags")
    out = {"dir": str(d)}
    for name, fa in (("g", "g.fa"), ("geometry", "geometry.fa")):
        ufi = os.path.join(d, name + ".ufi")
        if name == "g":
            with gzip.open(os.path.join(GOLD, "g.ufi.gz"), "rb") as z, open(ufi, "wb") as f:
                f.write(z.read())
        else:
            ol.Index.build(os.path.join(GOLD, fa), el.SLOTS).save(ufi)
        idx = api.Index.open(ufi).upload(0)
        out[name] = {"ufi": ufi, "index": idx, "mapper": api.Mapper(idx, device=0), "refs": [(n, l) for n, l, _ in idx.directory()],
                     "fasta": tl.read_fasta(os.path.join(GOLD, fa))}
    out["ufi"] = out["g"]["ufi"]
    yield out
    for name in ("g", "geometry"):
        out[name]["mapper"].close()


# ---- the stage-level entry point ----
@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    import oracle_lib as ol
    from urmap_amd import api
    d = tmp_path_factory.mktemp("hand")
    store = tl.hand_store()
    fa = os.path.join(d, "hand.fa")
    open(fa, "w").write(">c\n" + "\n".join(store[i:i + 80] for i in range(0, len(store), 80)) + "\n")
    ufi = os.path.join(d, "hand.ufi")
    ol.Index.build(fa, 196613).save(ufi)
    idx = api.Index.open(ufi).upload(0)
    assert idx.directory() == [("c", len(store), idx.directory()[0][2])]
    m = api.Mapper(idx, device=0)
    yield {"store": store, "idx": idx, "m": m, "off": idx.directory()[0][2]}
    m.close()


def check_batch(hand, cases):
    from urmap_amd import api
    bases, offs, res, ops = tl.hand_batch(cases)
    res["dbpos"] += hand["off"]
    nm, tagged, md = hand["m"].tags_batch(bases, offs, res, ops)
    labels = [c["name"] for c in cases]
    quals = np.full(len(bases), 73, np.uint8)
    host = recs_of(hand["idx"].records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL))
    assert tagged.tolist() == [1] * len(cases)
    for i, (c, line) in enumerate(zip(cases, host)):
        f = line.split("\t")
        want = tl.calmd(hand["store"], int(f[3]), f[5], f[9])
        _, tags, _ = tl.split_fields(line)
        assert (int(tags["NM"][1]), tags["MD"][1]) == want, c["name"]   # host function = yardstick
        assert (int(nm[i]), md[i]) == want, c["name"]                   # device = yardstick
    return nm, md


def test_stage_entry_on_hand_made_shapes(hand):
    from urmap_amd import api
    cases = tl.hand_cases(hand["store"])
    nm, md = check_batch(hand, cases)
    by = {c["name"]: (int(n), t) for c, n, t in zip(cases, nm, md)}
    assert by["cols64"] == (0, "64") and by["cols65"] == (0, "65") and by["nm70000"][0] == 70000 and by["N_against_N"][0] == 70
    assert by["starts_with_D"][1].startswith("0^") and by["run_across_step_and_I"][1].endswith("156")
    # the mask: NM alone gives no MD text, MD alone no NM
    bases, offs, res, ops = tl.hand_batch(cases[:12])
    res["dbpos"] += hand["off"]
    n1, _, m1 = hand["m"].tags_batch(bases, offs, res, ops, tags=api.TAG_NM)
    n2, _, m2 = hand["m"].tags_batch(bases, offs, res, ops, tags=api.TAG_MD)
    assert n1.tolist() == nm[:12].tolist() and m1 == [""] * 12 and n2.tolist() == [0] * 12 and m2 == md[:12]
    # an unmapped record between mapped ones gets nothing
    res["dbpos"][3] = 0xFFFFFFFF
    n3, t3, m3 = hand["m"].tags_batch(bases, offs, res, ops)
    assert t3.tolist() == [1, 1, 1, 0] + [1] * 8 and m3[3] == "" and n3[3] == 0 and m3[4] == md[4]
    # an alignment that leaves its sequence is refused, not walked
    res["dbpos"][3] = hand["off"]
    res["coord"][2] = len(hand["store"]) - 3  # (63 columns from three bases before the end)
    with pytest.raises(api.UrmapxError):
        hand["m"].tags_batch(bases, offs, res, ops)


def test_stage_entry_alternating_lengths(hand):
    """1-column and 2 000-column alignments in turn: a wavefront's loop bounds change from record to record"""
    store = hand["store"]
    cases = []
    for k in range(150):
        if k % 2 == 0:
            cases.append(tl.hand_case(store, f"one{k}", 20000 + k, [(1, "M")], {0: store[20000 + k].translate(tl.OTHER)} if k % 4 == 0 else None))
        else:
            edits = {c: store[30000 + k + c].translate(tl.OTHER) for c in range(k % 7, 2000, 61 + k % 5)}
            cases.append(tl.hand_case(store, f"long{k}", 30000 + k, [(900, "M"), (3, "D"), (500, "M"), (2, "I"), (598, "M")], edits, plus=k % 3 != 0))
    check_batch(hand, cases)


# ---- the text stage ----
def tagged_text(m, fq, tags, rg, bam=False):
    from urmap_amd import api
    m.set_tags(tags, rg)
    m.set_bam(bam)
    try:
        out, rep = m.map_text_se(fq[0]) if len(fq) == 1 else m.map_text_pe(*fq)
    finally:
        m.set_bam(False)
        m.set_tags(0, None)
    assert rep["reason"] == api.TEXT_OK and rep["sam_bytes"] == len(out) == rep["sam_text_bytes"], rep
    return out


def host_arrays(c, d, names):
    from urmap_amd import api
    sets = []
    for i, name in enumerate(names):
        p = os.path.join(d, f"h{i}.fq")
        open(p, "wb").write(gold(name))
        sets.append(api.read_fastq_arrays(p))
    if len(sets) == 1:
        labels, bases, offs, quals = sets[0]
        res, ops = c["mapper"].map_se(bases, offs)
    else:
        labels, bases, offs, quals = api.interleave_pairs(*sets)
        res, ops = c["mapper"].map_pe(bases, offs)
    return res, ops, labels, bases, offs, quals


GOLD_RUNS = [(("se150.fq",), "g"), (("se250.fq",), "g"), (("se_alpha.fq",), "g"), (("pe150_1.fq", "pe150_2.fq"), "g"),
             (("pe100_noisy_1.fq", "pe100_noisy_2.fq"), "g"), (("geometry_1.fq", "geometry_2.fq"), "geometry")]


@pytest.mark.parametrize("names,ufi", GOLD_RUNS)
def test_text_stage_equals_the_host_formatters(golden, tmp_path, names, ufi):
    from urmap_amd import api
    c = golden[ufi]
    m = c["mapper"]
    fq = [gold(n) for n in names]
    paired = len(names) == 2
    arrays = host_arrays(c, str(tmp_path), names)
    sam = tagged_text(m, fq, api.TAG_ALL, RG_ID)
    assert sam == c["index"].records_tags(*arrays, tags=api.TAG_ALL, rg_id=RG_ID, paired=paired)
    plain = recs_of(m.map_text_se(fq[0])[0] if not paired else m.map_text_pe(*fq)[0])
    for line, pl, r in zip(recs_of(sam), plain, arrays[0]):
        assert tl.check_sam_record(line, c["fasta"], ALL, RG_ID, score=r["score"]) == pl
    bam = tagged_text(m, fq, api.TAG_ALL, RG_ID, bam=True)
    assert bam == c["index"].records_tags(*arrays, tags=api.TAG_ALL, rg_id=RG_ID, bam=True, paired=paired)
    for (bline, aux), line in zip(tl.read_bam_records_aux(bam, c["refs"]), recs_of(sam)):
        base, tags, order = tl.split_fields(line)
        assert bline == bl.normalise_sam_line(base) and aux == tl.aux_of_sam_fields(tags, order)
    # BGZF members of both inflate to the plain bytes
    m.set_bgzf(True)
    try:
        for want, as_bam in ((sam, False), (bam, True)):
            m.set_tags(api.TAG_ALL, RG_ID)
            m.set_bam(as_bam)
            z, rep = m.map_text_se(fq[0]) if not paired else m.map_text_pe(*fq)
            assert rep["reason"] == api.TEXT_OK and rep["sam_text_bytes"] == len(want)
            assert b"".join(x[0] for x in walk_bgzf(z, eof=False)) == want
    finally:
        m.set_bgzf(False); m.set_bam(False); m.set_tags(0, None)
    # 64-record chunks: records at every position of a wavefront's 64, the same bytes
    lines = [f.split(b"\n")[:-1] for f in fq]
    per = 64 if not paired else 32
    got = b""
    for a in range(0, len(lines[0]) // 4, per):
        got += tagged_text(m, [b"\n".join(l[4 * a:4 * (a + per)]) + b"\n" for l in lines], api.TAG_ALL, RG_ID)
    assert got == sam
    # switched off again: today's bytes
    assert recs_of(m.map_text_se(fq[0])[0] if not paired else m.map_text_pe(*fq)[0]) == plain


@pytest.mark.parametrize("tags,rg", [(1, None), (2, None), (4, None), (0, RG_ID), (3, None), (6, RG_ID)])
def test_each_field_alone(golden, tmp_path, tags, rg):
    c = golden["g"]
    arrays = host_arrays(c, str(tmp_path), ("se150.fq",))
    want = {n for n, b in (("NM", 1), ("MD", 2), ("AS", 4)) if tags & b}
    for bam in (False, True):
        got = tagged_text(c["mapper"], [gold("se150.fq")], tags, rg, bam=bam)
        assert got == c["index"].records_tags(*arrays, tags=tags, rg_id=rg, bam=bam)
        if not bam:
            for line, r in zip(recs_of(got), arrays[0]):
                tl.check_sam_record(line, c["fasta"], want, rg, score=r["score"])


def test_set_tags_rules(golden):
    from urmap_amd import api
    m = golden["g"]["mapper"]
    with pytest.raises(api.UrmapxError):
        m.set_tags(8, None)
    with pytest.raises(api.UrmapxError):
        m.set_tags(1, "")
    se = gold("se150.fq")
    z, rep = m.map_text_se(se, sam_cap=16)
    assert z is None and rep["reason"] == api.TEXT_SAM_CAP
    with pytest.raises(api.UrmapxError):  # a chunk waits to be fetched
        m.set_tags(1, None)
    z, rep = m.fetch_text_sam(rep["sam_bytes"])
    assert recs_of(z) == recs_of(gold("se150.sam"))
    m.set_tags(0, None)


def test_long_reads_and_long_paths(small_case, tmp_path):
    """a single-end read of more than 1 024 bases with indels (the general kernel's road) and reads whose paths have more than 96
    runs, made as tests/test_gpu_bam.py makes them: the fields equal the yardstick's and the host formatters' bytes"""
    from test_gpu_pe_general import _gappy, _relaxed
    from urmap_amd import api, synth
    rng = np.random.default_rng(96)
    g0 = small_case["genome"][0][1]
    idx = api.Index.open(small_case["ufi"]).upload(0)
    m = api.Mapper(idx, device=0, params=_relaxed(api.params_for_method(6)))
    reads = []
    for k, QL in enumerate((1000, 600, 2000, 1500)):
        lo = int(rng.integers(1000, len(g0) - 6000))
        s = _gappy(rng, g0[lo:lo + 2 * QL], QL // 3, QL // 6)[:QL]
        if k & 1:
            s = synth.revcomp(s)
        reads.append((f"long{k}", s, np.full(len(s), ord("I") - k, np.uint8)))
    plain = synth.make_reads(7, small_case["genome"], 70, read_len=150, sub=0.02, ins=0.002, dele=0.002)
    reads = plain[:40] + reads[:2] + plain[40:] + reads[2:]
    fq = os.path.join(tmp_path, "long.fq")
    synth.write_fastq(fq, reads)
    fasta = tl.read_fasta(small_case["fasta"])
    labels, bases, offs, quals = api.read_fastq_arrays(fq)
    try:
        res, ops = m.map_se(bases, offs)
        sam = tagged_text(m, [open(fq, "rb").read()], api.TAG_ALL, RG_ID)
        bam = tagged_text(m, [open(fq, "rb").read()], api.TAG_ALL, RG_ID, bam=True)
    finally:
        m.close()
    assert sam == idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID)
    assert bam == idx.records_tags(res, ops, labels, bases, offs, quals, tags=api.TAG_ALL, rg_id=RG_ID, bam=True)
    n_ops, long_gapped = [], 0
    for line, r in zip(recs_of(sam), res):
        tl.check_sam_record(line, fasta, ALL, RG_ID, score=r["score"])
        f = line.split("\t")
        if f[2] != "*":
            n_ops.append(len(bl.parse_cigar(f[5])))
            long_gapped += len(f[9]) > 1024 and n_ops[-1] > 1
    assert max(n_ops) > 96 and long_gapped >= 1, sorted(n_ops)[-6:]


# ---- command line ----
def _run(args, ok=True, **kw):
    r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _se(golden):
    return ["-map", os.path.join(GOLD, "se150.fq"), "-ufi", golden["ufi"], "-quiet"]


def _pe(golden):
    return ["-map2", os.path.join(GOLD, "pe150_1.fq"), "-reverse", os.path.join(GOLD, "pe150_2.fq"), "-ufi", golden["ufi"], "-quiet"]


TAGS = ["-tags", "AS,NM,MD", "-rg", RG_ARG]
no_pg = lambda text: b"\n".join(l for l in text.split(b"\n") if not l.startswith(b"@PG"))


@pytest.fixture(scope="module")
def tagged_se(golden):
    """`urmap -map ... -samout` with the flags, next to a run without them"""
    plain, out = os.path.join(golden["dir"], "plain.sam"), os.path.join(golden["dir"], "tagged.sam")
    _run(_se(golden) + ["-samout", plain])
    _run(_se(golden) + ["-samout", out] + TAGS)
    assert no_pg(open(plain, "rb").read()) == no_pg(gold("se150.sam"))  # nothing changes without the flags
    return open(out, "rb").read()


def check_tagged_sam(text, golden_sam, fasta):
    lines = text.decode("latin-1").split("\n")
    hdr = [l for l in lines if l.startswith("@")]
    ghdr = [l for l in golden_sam.decode("latin-1").split("\n") if l.startswith("@")]
    assert [l for l in hdr if l[:3] not in ("@PG", "@RG")] == [l for l in ghdr if not l.startswith("@PG")]
    assert hdr[-2] == RG_LINE and hdr[-1].startswith("@PG") and "-tags AS,NM,MD" in hdr[-1] and "-rg" in hdr[-1]
    for line, want in zip(recs_of(text), recs_of(golden_sam)):
        assert tl.check_sam_record(line, fasta, ALL, RG_ID) == want
    assert len(recs_of(text)) == len(recs_of(golden_sam))


def test_cli_map_and_map2(golden, tagged_se):
    check_tagged_sam(tagged_se, gold("se150.sam"), golden["g"]["fasta"])
    out = os.path.join(golden["dir"], "tagged_pe.sam")
    _run(_pe(golden) + ["-samout", out] + TAGS)
    check_tagged_sam(open(out, "rb").read(), gold("pe150.sam"), golden["g"]["fasta"])
    out2 = os.path.join(golden["dir"], "tagged_pe_vf.sam")
    _run(_pe(golden) + ["-samout", out2, "-veryfast"] + TAGS)
    for line in recs_of(open(out2, "rb").read()):
        tl.check_sam_record(line, golden["g"]["fasta"], ALL, RG_ID)


def test_cli_roads_give_the_same_bytes(golden, tagged_se):
    want = no_pg(tagged_se)
    for extra, env in ((["-streams", "1"], {}), (["-streams", "3", "-batch", "64"], {}), (["-gpus", "1", "-streams", "2", "-batch", "128"], {}), (["-host"], {}),
                       (["-threads", "3"], {"URMAPX_HOST_TEXT": "1"}), (["-bgzf"], {})):
        out = os.path.join(golden["dir"], "road.sam")
        _run(_se(golden) + ["-samout", out] + TAGS + extra, env={**os.environ, **env})
        blob = open(out, "rb").read()
        assert no_pg(bl.inflate(blob) if "-bgzf" in extra else blob) == want, extra
    out = os.path.join(golden["dir"], "sh.sam")
    _run(_se(golden) + ["-samout", out, "-samshards", "2", "-batch", "64"] + TAGS)
    assert no_pg(open(out + ".0", "rb").read() + open(out + ".1", "rb").read()) == want
    # a '\r' in the input: that chunk takes the host road, with the index in device memory only (the span call's device road)
    fq = os.path.join(golden["dir"], "cr.fq")
    lines = gold("se150.fq").split(b"\n")[:-1]
    lines[4 * 100 + 1] += b"\r"
    open(fq, "wb").write(b"\n".join(lines) + b"\n")
    _run(["-map", fq, "-ufi", golden["ufi"], "-quiet", "-samout", out, "-batch", "64"] + TAGS)
    assert no_pg(open(out, "rb").read()) == want


def test_cli_bamout_and_sort(golden, tagged_se):
    from urmap_amd import api
    out, srt = os.path.join(golden["dir"], "t.bam"), os.path.join(golden["dir"], "s.bam")
    _run(_se(golden) + ["-bamout", out] + TAGS)
    blob = open(out, "rb").read()
    assert blob.endswith(EOF_MEMBER)
    walk_bgzf(blob)
    text, refs, recs, stream = tl.read_bam_aux(bl.inflate(blob))
    assert [l[:3] for l in text.decode().split("\n") if l] == ["@SQ"] * len(refs) + ["@RG", "@PG"]
    for (bline, aux), line in zip(recs, recs_of(tagged_se)):
        base, tags, order = tl.split_fields(line)
        assert bline == bl.normalise_sam_line(base) and aux == tl.aux_of_sam_fields(tags, order)
    assert len(recs) == len(recs_of(tagged_se))
    for extra in (["-host"], ["-batch", "64", "-streams", "1"]):
        other = os.path.join(golden["dir"], "o.bam")
        _run(_se(golden) + ["-bamout", other] + TAGS + extra)
        assert tl.read_bam_aux(bl.inflate(open(other, "rb").read()))[3] == stream, extra
    # -sort: the header, the order and the index hold with the fields on the records
    _run(_se(golden) + ["-bamout", srt, "-sort"] + TAGS)
    sblob = open(srt, "rb").read()
    stext, srefs, srecs, sstream = tl.read_bam_aux(bl.inflate(sblob))
    assert [l[:3] for l in stext.decode().split("\n") if l] == ["@HD"] + ["@SQ"] * len(refs) + ["@RG", "@PG"] and srefs == refs
    f = sl.BgzfFile(sblob)
    first = f.members()[0]
    in_front = f.member(first[0])[1]
    members = sblob[in_front:len(sblob) - len(api.BGZF_EOF)]
    got_stream, chain = sl.check_stream(members, stream)
    assert got_stream == sstream and sorted(a for _, a in srecs) == sorted(a for _, a in recs)
    b = sl.parse_bai(open(srt + ".bai", "rb").read())
    sl.check_index(b, chain, sl.member_places(f, in_front), len(refs))
    sl.check_queries(b, f, [r for _, r in chain], sl.edge_regions([L for _, L in refs], np.random.default_rng(3), 40))
    assert all(aux and aux[-1] == ("RG", "Z", RG_ID) for _, aux in srecs)
