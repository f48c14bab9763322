"""GPU tests of -bamout: the device record encoder (bam_gpu.hip) through the text stage -- raw records against the yardstick of
tests/bam_lib.py applied to the same mapper's SAM text, and against the host encoder's bytes --, its edge shapes (partial wavefronts,
CIGARs longer than a lane's LDS slice, odd and even lengths on both strands), the device-road variants, and `urmap ... -bamout`
through every output road.  The BGZF layer goes through the walker of tests/test_bgzf_cpu.py."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_lib as bl
from test_bgzf_cpu import EOF_MEMBER, walk_bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "urmap_amd", "urmap")


def gold(name):
    p = os.path.join(GOLD, name)
    if os.path.exists(p):
        return open(p, "rb").read()
    with gzip.open(p + ".gz", "rb") as z:  # the alpha fixtures are kept .gz
        return z.read()


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    from urmap_amd import api
    d = tmp_path_factory.mktemp("bam")
    out = {"dir": str(d)}
    for name in ("g", "r"):
        ufi = os.path.join(d, name + ".ufi")
        with gzip.open(os.path.join(GOLD, name + ".ufi.gz"), "rb") as z, open(ufi, "wb") as f:
            f.write(z.read())
        idx = api.Index.open(ufi).upload(0)
        out[name] = {"ufi": ufi, "index": idx, "mapper": api.Mapper(idx, device=0), "refs": [(n, l) for n, l, _ in idx.directory()]}
    out["ufi"] = out["g"]["ufi"]
    yield out
    for name in ("g", "r"):
        out[name]["mapper"].close()


def text_then_bam(m, fq1, fq2=None):
    """the same chunk through the mapper's text stage as SAM text and as raw BAM records"""
    from urmap_amd import api
    call = (lambda: m.map_text_se(fq1)) if fq2 is None else (lambda: m.map_text_pe(fq1, fq2))
    sam, rep = call()
    assert rep["reason"] == api.TEXT_OK, rep
    m.set_bam(True)
    try:
        bam, brep = call()
    finally:
        m.set_bam(False)
    assert brep["reason"] == api.TEXT_OK and brep["records"] == rep["records"], brep
    assert brep["sam_bytes"] == len(bam) == brep["sam_text_bytes"]
    for k in ("mapped_q", "mapped_lowq", "unmapped", "unsupported"):
        assert brep[k] == rep[k], k
    return sam, bam


def host_bam(c, tmp_path, names):
    """the host encoder on the device's own results for these FASTQ files (one: single-end, two: mates)"""
    from urmap_amd import api
    sets = []
    for i, name in enumerate(names):
        p = os.path.join(tmp_path, f"h{i}.fq")
        open(p, "wb").write(gold(name))
        sets.append(api.read_fastq_arrays(p))
    if len(sets) == 1:
        labels, bases, offs, quals = sets[0]
        res, ops = c["mapper"].map_se(bases, offs)
        return c["index"].bam_se(res, ops, labels, bases, offs, quals)
    labels, bases, offs, quals = api.interleave_pairs(*sets)
    res, ops = c["mapper"].map_pe(bases, offs)
    return c["index"].bam_pe(res, ops, labels, bases, offs, quals)


# ---- raw records ----
@pytest.mark.parametrize("names,ufi", [(("se150.fq",), "g"), (("se250.fq",), "g"), (("se_short.fq",), "g"), (("se_alpha.fq",), "g"),
                                       (("pe150_1.fq", "pe150_2.fq"), "g"), (("pe120_rep_1.fq", "pe120_rep_2.fq"), "r"),
                                       (("pe_alpha_1.fq", "pe_alpha_2.fq"), "g")])
def test_raw_records(golden, tmp_path, names, ufi):
    c = golden[ufi]
    sam, bam = text_then_bam(c["mapper"], *[gold(n) for n in names])
    assert bam == bl.sam_to_bam_records(sam, c["refs"])
    assert bl.read_bam_records(bam, c["refs"]) == bl.sam_records(sam)
    assert bam == host_bam(c, str(tmp_path), names)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_chunks(golden, n):
    """the wavefront's partial last group of 64 records, and one record more than a group"""
    c = golden["g"]
    lines = gold("se150.fq").split(b"\n")
    sam, bam = text_then_bam(c["mapper"], b"\n".join(lines[:4 * n]) + b"\n")
    assert len(bl.sam_records(sam)) == n
    assert bam == bl.sam_to_bam_records(sam, c["refs"])
    if n >= 64:  # pairs: the mates of a pair fall into different groups at 65 records
        l1, l2 = gold("pe150_1.fq").split(b"\n"), gold("pe150_2.fq").split(b"\n")
        k = (n + 1) // 2
        sam, bam = text_then_bam(c["mapper"], b"\n".join(l1[:4 * k]) + b"\n", b"\n".join(l2[:4 * k]) + b"\n")
        assert bam == bl.sam_to_bam_records(sam, c["refs"])


def test_long_cigars_leave_the_lds_slice(small_case, tmp_path):
    """reads made as in test_gpu_pe_general.test_paths_of_more_than_96_runs (relaxed penalties, a one-base gap every three bases):
    CIGARs of more than 15 ops are written straight into the record by their lane, next to records that go through LDS"""
    from test_gpu_pe_general import _gappy, _relaxed
    from urmap_amd import api, synth
    rng = np.random.default_rng(96)
    g0 = small_case["genome"][0][1]
    idx = api.Index.open(small_case["ufi"]).upload(0)
    m = api.Mapper(idx, device=0, params=_relaxed(api.params_for_method(6)))
    reads = []
    for k, QL in enumerate((1000, 600, 270, 1000, 2000)):
        lo = int(rng.integers(1000, len(g0) - 6000))
        s = _gappy(rng, g0[lo:lo + 2 * QL], QL // 3, QL // 6)[:QL]
        if k & 1:
            s = synth.revcomp(s)
        reads.append((f"long{k}", s, np.full(len(s), ord("I") - k, np.uint8)))
    plain = synth.make_reads(7, small_case["genome"], 70, read_len=150, sub=0.02, ins=0.002, dele=0.002)
    reads = plain[:40] + reads[:3] + plain[40:] + reads[3:]  # long ones inside a group of 64 and in the partial group
    fq = os.path.join(tmp_path, "long.fq")
    synth.write_fastq(fq, reads)
    refs = [(n, l) for n, l, _ in idx.directory()]
    try:
        sam, bam = text_then_bam(m, open(fq, "rb").read())
    finally:
        m.close()
    n_ops = [len(bl.parse_cigar(l.split("\t")[5])) for l in bl.sam_records(sam)]
    assert sum(n > 15 for n in n_ops) >= 4 and max(n_ops) > 96 and sum(0 < n <= 15 for n in n_ops) >= 40, sorted(n_ops)[-8:]
    assert bam == bl.sam_to_bam_records(sam, refs)
    assert bl.read_bam_records(bam, refs) == bl.sam_records(sam)


def test_both_strands_odd_and_even_lengths(golden, tmp_path):
    """nibble packing meets reversal: reads of 149, 150, 151 and 152 bases from both strands in one chunk"""
    from urmap_amd import synth
    c = golden["g"]
    g = [(n, np.frombuffer(s.encode(), np.uint8)) for n, s in _fasta(os.path.join(GOLD, "g.fa"))]
    reads = []
    for k, L in enumerate((149, 150, 151, 152) * 20):
        r = synth.make_reads(100 + k, g, 1, read_len=L, sub=0.01, ins=0.0, dele=0.0)[0]
        s = synth.revcomp(r[1]) if (k // 4) & 1 else r[1]
        reads.append((f"s{k}", s, np.frombuffer(bytes(33 + (7 * i + k) % 41 for i in range(len(s))), np.uint8)))
    fq = os.path.join(tmp_path, "strands.fq")
    synth.write_fastq(fq, reads)
    sam, bam = text_then_bam(c["mapper"], open(fq, "rb").read())
    recs = bl.sam_records(sam)
    # (the single-end flag carries no strand bit, as in the reference: a minus-strand hit shows in SEQ, printed reverse-complemented)
    seen = set()
    for (_, s, _), l in zip(reads, recs):
        f = l.split("\t")
        if f[2] != "*":
            fwd, rev = s.tobytes().decode().upper(), synth.revcomp(s).tobytes().decode().upper()  # (sam_records folds the case)
            assert f[9] in (fwd, rev)
            seen.add((f[9] != fwd, len(s) & 1))
    assert seen == {(False, 0), (False, 1), (True, 0), (True, 1)}, seen
    assert bam == bl.sam_to_bam_records(sam, c["refs"])
    assert bl.read_bam_records(bam, c["refs"]) == recs


def _fasta(path):
    name, seq = None, []
    for l in open(path).read().split("\n"):
        if l.startswith(">"):
            if name is not None:
                yield name, "".join(seq)
            name, seq = l[1:].split()[0], []
        elif l:
            seq.append(l)
    if name is not None:
        yield name, "".join(seq)


# ---- device-road variants ----
def test_device_road_variants(golden):
    from urmap_amd import api
    c = golden["g"]
    m = c["mapper"]
    se = gold("se150.fq")
    plain, raw = text_then_bam(m, se)
    lines = se.split(b"\n")[:-1]
    chunks = [b"\n".join(lines[a:b]) + b"\n" for a, b in ((0, 4 * 120), (4 * 120, len(lines)))]
    raw_chunks = [text_then_bam(m, ch)[1] for ch in chunks]
    assert b"".join(raw_chunks) == raw
    m.set_bam(True)
    try:
        # the SAM_CAP refusal names the size, the fetch gives the records
        z, rep = m.map_text_se(se, sam_cap=len(raw) // 2)
        assert z is None and rep["reason"] == api.TEXT_SAM_CAP and rep["sam_bytes"] == len(raw)
        z, rep = m.fetch_text_sam(rep["sam_bytes"])
        assert z == raw
        # the deferred road, two chunks in flight
        res = m.map_text_se_stream(chunks)
        for (z, rep), want in zip(res, raw_chunks):
            assert rep["reason"] == api.TEXT_OK and rep["sam_bytes"] == len(z) == rep["sam_text_bytes"] and z == want
        # BGZF members of the records
        m.set_bgzf(True)
        try:
            z, rep = m.map_text_se(se)
            assert rep["reason"] == api.TEXT_OK and rep["sam_bytes"] == len(z) and rep["sam_text_bytes"] == len(raw) and len(z) < len(raw)
            assert b"".join(x[0] for x in walk_bgzf(z, eof=False)) == raw
            res = m.map_text_se_stream(chunks)
            for (z, rep), want in zip(res, raw_chunks):
                assert rep["reason"] == api.TEXT_OK and b"".join(x[0] for x in walk_bgzf(z, eof=False)) == want
        finally:
            m.set_bgzf(False)
    finally:
        m.set_bam(False)
    assert m.map_text_se(se)[0] == plain  # switched back off: today's text bytes


# ---- command line ----
def _run(args, ok=True, **kw):
    r = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _se(golden, fq=None):
    return ["-map", fq or os.path.join(GOLD, "se150.fq"), "-ufi", golden["ufi"], "-quiet"]


def _pe(golden):
    return ["-map2", os.path.join(GOLD, "pe150_1.fq"), "-reverse", os.path.join(GOLD, "pe150_2.fq"), "-ufi", golden["ufi"], "-quiet"]


def check_bam_file(blob, plain_text, option="-bamout"):
    """a complete BAM file whose records are the plain run's: BGZF members and the end-of-file member, the header text the plain
    header up to the @PG line (which names the option), references = the @SQ lines, records = the SAM records (normalised)"""
    assert blob.endswith(EOF_MEMBER)
    walk_bgzf(blob)
    text, refs, lines = bl.read_bam(bl.inflate(blob))
    text = text.decode("latin-1")
    want_hdr = bl.sam_header(plain_text)
    assert [l for l in text.split("\n") if not l.startswith("@PG")] == [l for l in want_hdr.split("\n") if not l.startswith("@PG")]
    pg = [l for l in text.split("\n") if l.startswith("@PG")]
    assert len(pg) == 1 and option in pg[0]
    assert refs == bl.refs_of_header(want_hdr) and refs
    return lines


def twice(args, out):
    """the run twice: the same file bytes"""
    _run(args)
    blob = open(out, "rb").read()
    _run(args)
    assert open(out, "rb").read() == blob
    return blob


@pytest.fixture(scope="module")
def plain_se(golden):
    out = os.path.join(golden["dir"], "plain_se.sam")
    _run(_se(golden) + ["-samout", out])
    text = open(out, "rb").read()
    assert bl.sam_records(text) == bl.sam_records(gold("se150.sam"))
    return text


def test_cli_map(golden, plain_se):
    out = os.path.join(golden["dir"], "se.bam")
    blob = twice(_se(golden) + ["-bamout", out], out)
    assert check_bam_file(blob, plain_se) == bl.sam_records(plain_se)
    assert len(blob) < len(plain_se) // 2
    r = _run(_se(golden)[:-1] + ["-bamout", out])
    assert b"Bytes of BAM records" in r.stderr


def test_cli_map2_with_tabbedout(golden):
    plain, out, tab = (os.path.join(golden["dir"], n) for n in ("plain_pe.sam", "pe.bam", "pe.tab"))
    _run(_pe(golden) + ["-samout", plain])
    blob = twice(_pe(golden) + ["-bamout", out, "-tabbedout", tab], out)
    want = open(plain, "rb").read()
    assert bl.sam_records(want) == bl.sam_records(gold("pe150.sam"))
    assert check_bam_file(blob, want) == bl.sam_records(want)
    assert open(tab, "rb").read() == gold("pe150.tab")  # -tabbedout stays plain text


def test_cli_shards_are_complete_bam_files(golden, plain_se):
    out = os.path.join(golden["dir"], "sh.bam")
    args = _se(golden) + ["-bamout", out, "-samshards", "2", "-batch", "64"]
    _run(args)
    blobs = [open(f"{out}.{s}", "rb").read() for s in range(2)]
    parts = [check_bam_file(b, plain_se) for b in blobs]
    assert all(parts) and parts[0] + parts[1] == bl.sam_records(plain_se)
    _run(args)
    assert [open(f"{out}.{s}", "rb").read() for s in range(2)] == blobs
    # more shards than records: a shard without records is the header block and the end-of-file member
    fq = os.path.join(golden["dir"], "one.fq")
    open(fq, "wb").write(b"\n".join(gold("se150.fq").split(b"\n")[:4]) + b"\n")
    _run(_se(golden, fq) + ["-bamout", out, "-samshards", "2"])
    parts = [check_bam_file(open(f"{out}.{s}", "rb").read(), plain_se) for s in range(2)]
    assert parts[0] + parts[1] == bl.sam_records(plain_se)[:1] and [] in parts


def test_cli_stdout_pipe(golden, plain_se):
    cmd = f"'{EXE}' -map '{os.path.join(GOLD, 'se150.fq')}' -ufi '{golden['ufi']}' -bamout /dev/stdout -quiet | cat"
    outs = []
    for _ in range(2):
        r = subprocess.run(cmd, shell=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    assert check_bam_file(outs[0], plain_se) == bl.sam_records(plain_se)


def test_cli_host_text_road(golden, plain_se):
    out = os.path.join(golden["dir"], "host.bam")
    env = dict(os.environ, URMAPX_HOST_TEXT="1", OMP_NUM_THREADS="4")
    _run(_se(golden) + ["-bamout", out, "-threads", "4"], env=env)
    blob = open(out, "rb").read()
    _run(_se(golden) + ["-bamout", out, "-threads", "4"], env=env)
    assert open(out, "rb").read() == blob
    assert check_bam_file(blob, plain_se) == bl.sam_records(plain_se)
    out2 = os.path.join(golden["dir"], "hostflag.bam")
    _run(_se(golden) + ["-bamout", out2, "-host"])
    assert check_bam_file(open(out2, "rb").read(), plain_se) == bl.sam_records(plain_se)


def test_cli_carriage_return_takes_the_host_fallback(golden):
    fq = os.path.join(golden["dir"], "cr.fq")
    lines = gold("se150.fq").split(b"\n")[:-1]
    lines[4 * 100 + 1] += b"\r"
    open(fq, "wb").write(b"\n".join(lines) + b"\n")
    plain, out = os.path.join(golden["dir"], "cr.sam"), os.path.join(golden["dir"], "cr.bam")
    _run(_se(golden, fq) + ["-samout", plain, "-batch", "64"])
    blob = twice(_se(golden, fq) + ["-bamout", out, "-batch", "64", "-threads", "4"], out)
    want = open(plain, "rb").read()
    assert bl.sam_records(want) == bl.sam_records(gold("se150.sam"))
    assert check_bam_file(blob, want) == bl.sam_records(want)


def test_cli_gz_input(golden, plain_se):
    fq = os.path.join(golden["dir"], "in.fq.gz")
    with gzip.open(fq, "wb") as f:
        f.write(gold("se150.fq"))
    out = os.path.join(golden["dir"], "gz.bam")
    blob = twice(_se(golden, fq) + ["-bamout", out], out)
    assert check_bam_file(blob, plain_se) == bl.sam_records(plain_se)


def test_cli_refusals(golden):
    out = os.path.join(golden["dir"], "no.bam")
    for extra, word in ((["-samout", os.path.join(golden["dir"], "no.sam")], b"-samout"), (["-bgzf"], b"-bgzf")):
        if os.path.exists(out):
            os.remove(out)
        r = _run(_se(golden) + ["-bamout", out] + extra, ok=False)
        assert r.returncode != 0 and word in r.stderr and b"-bamout" in r.stderr, r.stderr
        assert not os.path.exists(out)
    # a QNAME of 255 bytes does not fit l_read_name: the run stops and names the read; 254 bytes pass
    lines = gold("se150.fq").split(b"\n")[:4 * 70]
    for n, ok in ((254, True), (255, False)):
        fq = os.path.join(golden["dir"], f"name{n}.fq")
        ls = list(lines)
        ls[4 * 66] = b"@" + b"q" * n + b" tail"
        open(fq, "wb").write(b"\n".join(ls) + b"\n")
        for env in ({}, {"URMAPX_HOST_TEXT": "1"}):
            r = _run(_se(golden, fq) + ["-bamout", out], ok=False, env={**os.environ, **env})
            if ok:
                assert r.returncode == 0, r.stderr
                recs = bl.read_bam(bl.inflate(open(out, "rb").read()))[2]
                assert len(recs) == 70 and recs[66].split("\t")[0] == "q" * 254
            else:
                assert r.returncode != 0 and b"254" in r.stderr and b"qqqqqqqq" in r.stderr, r.stderr


def test_cli_samout_named_bam_is_still_text(golden, plain_se):
    out = os.path.join(golden["dir"], "x.bam")
    _run(_se(golden) + ["-samout", out])
    text = open(out, "rb").read()
    assert [l for l in text.split(b"\n") if not l.startswith(b"@PG")] == [l for l in plain_se.split(b"\n") if not l.startswith(b"@PG")]
