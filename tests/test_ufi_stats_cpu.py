"""The index statistics (-ufi_stats, -ufi_counts, -ufi_info) written down in numpy (tests/ufistats_lib.py) against what the reference
printed for the fixture tables (tests/golden/ufi_stats.json, written by tests/golden/make_golden_ufistats.py).  This pins the semantics
without a device: the last byte of the sequence store is never looked at, the minus strand has no 'u', GetRow's MaxIx cap comes before
a long link is resolved, Collision compares raw bytes, the report's widths, blanks and size strings.  The tables other than the two
golden ones are built by the product's -make_ufi on the host, and must be the reference's bytes."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ufistats_lib as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URMAP = os.path.join(ROOT, "urmap_amd", "urmap")
FIX = json.load(open(os.path.join(U.GOLD, "ufi_stats.json")))


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def table(name, d):
    """the fixture table `name` as a .ufi file in d: a golden file, or the product's -make_ufi (on the host) with the fixture's options"""
    v = FIX[name]
    if v["options"] is None:
        return U.gunzip(v["source"], d)
    p = os.path.join(d, name + ".ufi")
    subprocess.run([URMAP, "-make_ufi", os.path.join(U.GOLD, v["source"]), "-output", p, "-host"] + v["options"], check=True,
                   capture_output=True)
    return p


def test_fixture_covers_the_regimes():
    assert set(FIX) == {"g", "r", "veryfast", "lf09", "s40009", "sat"}
    s = FIX["s40009"]["report"]
    assert any(l.endswith(" NotIndexed") and int(l.split()[0]) > 0 for l in s)
    assert any(l.endswith(" LongMine") and int(l.split()[0]) > 0 for l in s)
    assert any(l.endswith(" Trunc2") and int(l.split()[0]) > 0 for l in s)
    assert FIX["sat"]["counts_bincount"]["255"] == 3
    assert open(os.path.join(U.GOLD, "sat.fa")).read() == open(os.path.join(U.GOLD, "g.fa")).read() + ">sat\n" + "\n".join(
        U.SAT_EXTRA[i:i + 80] for i in range(0, len(U.SAT_EXTRA), 80)) + "\n"


@pytest.mark.parametrize("name", sorted(FIX))
def test_restatement_equals_reference(name, tmp_path):
    p = table(name, str(tmp_path))
    assert sha(p) == FIX[name]["sha256"]
    u = U.Ufi(p)
    st = U.stats(u)
    assert U.report(st) == FIX[name]["report"]
    assert U.info_lines(u) == FIX[name]["info"]
    plus, minus = U.slot_counts(u)
    assert hashlib.sha256(plus.tobytes()).hexdigest() == FIX[name]["counts_sha256"]
    assert {str(k): int(v) for k, v in enumerate(np.bincount(plus, minlength=256)) if v} == FIX[name]["counts_bincount"]
    # the report's own identities
    assert sum(st["count_hist"]) == st["slots"] == st["free"] + st["mine"] + st["other"]
    assert st["indexed"] + st["not_indexed"] + st["wildcard"] == st["seqdata_size"] - 1
    assert sum(i * c for i, c in enumerate(st["count_hist"])) == st["total"]


@pytest.mark.parametrize("name", ["g", "s40009"])
def test_ufi_info_cli_equals_reference(name, tmp_path):
    """-ufi_info reads the header only: no device is needed"""
    p = table(name, str(tmp_path))
    log = str(tmp_path / "info.log")
    r = subprocess.run([URMAP, "-ufi_info", p, "-log", log], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr.splitlines() == FIX[name]["info"]
    assert [l for l in open(log).read().split("\n") if l in FIX[name]["info"]] == FIX[name]["info"]


def test_ufi_info_api_and_bad_magic(tmp_path):
    from urmap_amd import api

    p = table("g", str(tmp_path))
    assert api.ufi_info(p) == {"word_length": 24, "max_ix": 32, "seqdata_size": 40064, "slots": 71347}
    bad = tmp_path / "bad.ufi"
    bad.write_bytes(b"\0" * 64)
    with pytest.raises(api.UrmapxError) as e:
        api.ufi_info(str(bad))
    assert e.value.code == api.E_FORMAT
    r = subprocess.run([URMAP, "-ufi_info", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad magic" in r.stderr
    r = subprocess.run([URMAP, "-ufi_counts", p], capture_output=True, text=True)
    assert r.returncode != 0 and "Missing output file name" in r.stderr
