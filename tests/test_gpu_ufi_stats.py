"""-ufi_stats, -ufi_counts and Index.stats() / slot_counts() on the device (ufi_stats.hip) against the reference's fixture
(tests/golden/ufi_stats.json) and the numpy restatement (tests/ufistats_lib.py): the report byte for byte, every counter and both
histograms, the count files, the minus counts, another word length, and a damaged table."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ufistats_lib as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URMAP = os.path.join(ROOT, "urmap_amd", "urmap")
FIX = json.load(open(os.path.join(U.GOLD, "ufi_stats.json")))
NUMBERS = ("word_length", "max_ix", "seqdata_size", "slots", "indexed", "not_indexed", "wildcard", "indexed2", "free", "collision",
           "single_both", "single_plus", "end", "mine", "other", "trunc", "trunc2", "long_mine", "long_other", "total", "count_hist",
           "trunc_hist")


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def make(fasta, out, opts):
    subprocess.run([URMAP, "-make_ufi", fasta, "-output", out] + opts, check=True, capture_output=True, timeout=300)
    return out


def table(name, d):
    v = FIX[name]
    p = U.gunzip(v["source"], d) if v["options"] is None else make(os.path.join(U.GOLD, v["source"]), os.path.join(d, name + ".ufi"), v["options"])
    assert sha(p) == v["sha256"]
    return p


def run(args, env=None, ok=True):
    r = subprocess.run([URMAP] + args, capture_output=True, text=True, timeout=300, env=env)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("name", sorted(FIX))
def test_stats_equal_the_reference(name, tmp_path):
    from urmap_amd import api

    p = table(name, str(tmp_path))
    log = str(tmp_path / "s.log")
    run(["-ufi_stats", p, "-log", log, "-quiet"])
    assert U.log_report(open(log).read()) == FIX[name]["report"]
    counts = str(tmp_path / "c.bin")
    run(["-ufi_counts", p, "-output", counts])
    assert sha(counts) == FIX[name]["counts_sha256"]

    u = U.Ufi(p)
    want = U.stats(u)
    plus, minus = U.slot_counts(u)
    idx = api.Index.open(p).upload(0)
    try:
        st = idx.stats()
        assert {k: st[k] for k in NUMBERS} == want
        assert st["bad_rows"] == 0 and st["first_bad_slot"] == 2 ** 64 - 1
        assert U.report(st) == FIX[name]["report"]
        assert np.array_equal(idx.slot_counts(), plus)
        assert np.array_equal(idx.slot_counts(minus=True), minus)
        _, rep = idx.validate()  # (a table whose rows MaxIx cuts leaves chain links unreached: validate's own check fails there)
        assert st["indexed2"] == rep["positions"]
    finally:
        idx.close()


def test_stats_through_host_arrays_and_stderr(tmp_path):
    """URMAPX_HOST_INDEX=1 opens through host arrays; without -quiet the report also goes to stderr"""
    p = table("s40009", str(tmp_path))
    log = str(tmp_path / "s.log")
    r = run(["-ufi_stats", p, "-log", log], env=dict(os.environ, URMAPX_HOST_INDEX="1"))
    assert U.log_report(open(log).read()) == FIX["s40009"]["report"]
    assert "\n".join(FIX["s40009"]["report"][:-1]) in r.stderr


@pytest.mark.parametrize("w,opts", [(16, ["-wordlength", "16"]), (32, ["-wordlength", "32", "-slots", "80021", "-maxix", "4"])])
def test_other_word_lengths(w, opts, tmp_path):
    from urmap_amd import api

    for fa in ("g.fa", "sat.fa"):
        p = make(os.path.join(U.GOLD, fa), str(tmp_path / "w.ufi"), opts)
        u = U.Ufi(p)
        assert u.W == w
        plus, minus = U.slot_counts(u)
        idx = api.Index.open(p).upload(0)
        try:
            st = idx.stats()
            assert {k: st[k] for k in NUMBERS} == U.stats(u)
            assert np.array_equal(idx.slot_counts(), plus)
            assert np.array_equal(idx.slot_counts(minus=True), minus)
        finally:
            idx.close()


def test_damaged_row_is_a_format_error(tmp_path):
    """a row position moved past the sequence store: E_FORMAT naming the row's head slot, a non-zero exit; the device never reads there"""
    from urmap_amd import api

    p = table("g", str(tmp_path))
    u = U.Ufi(p)
    b = bytearray(open(p, "rb").read())
    blob_off = len(b) - 4 - u.sds - 4 - 5 * u.slots
    heads = [s for s in np.flatnonzero((u.tally >= 128) & (u.tally < 253)) if 0 < (u.tally[s] & 127) < 125]
    head = int(heads[len(heads) // 2])
    second = (head + int(u.tally[head] & 127)) % u.slots
    b[blob_off + 5 * second + 1: blob_off + 5 * second + 5] = (u.sds + 1000).to_bytes(4, "little")
    bad = str(tmp_path / "bad.ufi")
    open(bad, "wb").write(bytes(b))
    idx = api.Index.open(bad).upload(0)
    try:
        with pytest.raises(api.UrmapxError) as e:
            idx.stats()
        assert e.value.code == api.E_FORMAT
    finally:
        idx.close()
    r = run(["-ufi_stats", bad, "-quiet"], ok=False)
    assert r.returncode != 0
    assert "damaged row at slot 0x%x" % head in r.stderr
