"""CPU tests of the device sort's plan (urmapx_bam_sort_plan_for; host arithmetic in bam_sort_host.cpp): which road a budget of device
bytes gets -- in core, or the records streamed through the device in partitions of whole slices --, that the plan stays within its
budget and is the largest that does, that it never needs more partitions for more memory, and what it says where nothing fits."""
import ctypes as C

import pytest

from test_sanitizers_cpu import run as san_run, san  # noqa: F401  (san is a fixture: it builds the programs)
from urmap_amd import api

MEMBER = 65280
DEFAULT_SLICE = 2048  # members in a slice (bam_sort.h)
E_NOMEM = -3


def in_core(n_bytes, n, markdup):
    L = api.lib()
    fn = L.urmapx_bam_sort_markdup_device_bytes if markdup else L.urmapx_bam_sort_device_bytes
    fn.restype, fn.argtypes = C.c_uint64, [C.c_size_t, C.c_uint64]
    return int(fn(n_bytes, n))


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in ("URMAPX_TEST_SORT_SLICE", "URMAPX_TEST_SORT_PARTITION", "URMAPX_TEST_SORT_STAGE"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("markdup", [False, True])
@pytest.mark.parametrize("n_bytes,n", [(2_764_241_530, 10_000_000), (10_000_000, 40_000)])
def test_the_road_turns_at_the_in_core_need(n_bytes, n, markdup):
    need = in_core(n_bytes, n, markdup)
    p = api.bam_sort_plan(n_bytes, n, need, markdup)
    assert p["external"] == 0 and p["device_bytes"] == need and p["partitions"] == 0
    q = api.bam_sort_plan(n_bytes, n, need - 1, markdup)
    assert q["external"] == 1 and q["partitions"] >= 1 and q["device_bytes"] <= need - 1


@pytest.mark.parametrize("markdup", [False, True])
def test_a_whole_genome_beside_a_resident_index(markdup):
    n_bytes, n, budget = 200 * 10**9, 700 * 10**6, 150 * 10**9
    slice_bytes = DEFAULT_SLICE * MEMBER
    p = api.bam_sort_plan(n_bytes, n, budget, markdup)
    assert p["external"] == 1
    assert p["partition_bytes"] > 0 and p["partition_bytes"] % slice_bytes == 0
    assert p["partitions"] == -(-n_bytes // p["partition_bytes"])
    assert p["device_bytes"] <= budget
    assert p["stage_bytes"] > 0 and p["stage_bytes"] <= n_bytes // 16
    # the per-record arrays are in the sum: 48 bytes a record, 25 more under marking
    assert p["device_bytes"] >= (73 if markdup else 48) * n + p["partition_bytes"] + 2 * p["stage_bytes"]
    # one slice more would not have fitted: with a slice's worth more budget the plan takes exactly that slice
    q = api.bam_sort_plan(n_bytes, n, p["device_bytes"] + slice_bytes, markdup)
    assert q["partition_bytes"] == p["partition_bytes"] + slice_bytes and q["device_bytes"] == p["device_bytes"] + slice_bytes
    assert q["partitions"] == -(-n_bytes // q["partition_bytes"]) <= p["partitions"]
    assert budget - p["device_bytes"] < slice_bytes
    r = api.bam_sort_plan(n_bytes, n, p["device_bytes"] + slice_bytes - 1, markdup)
    assert r["partition_bytes"] == p["partition_bytes"]


@pytest.mark.parametrize("markdup", [False, True])
def test_more_memory_never_means_more_partitions(markdup):
    n_bytes, n = 200 * 10**9, 700 * 10**6
    least = minimum(n_bytes, n, markdup)
    before, budget, seen = None, least, set()
    while budget < 2 * in_core(n_bytes, n, markdup):
        p = api.bam_sort_plan(n_bytes, n, budget, markdup)
        assert p["device_bytes"] <= budget
        if before is not None:
            assert p["partitions"] <= before, budget
        before = p["partitions"]
        seen.add(before)
        budget += budget // 50 + 12345
    assert before == 0 and len(seen) > 10  # (the sweep ends in core and has passed through many partition counts)


def minimum(n_bytes, n, markdup):
    with pytest.raises(api.UrmapxError) as e:
        api.bam_sort_plan(n_bytes, n, 1, markdup)
    assert e.value.code == E_NOMEM
    return e.value.plan["device_bytes"]


@pytest.mark.parametrize("markdup", [False, True])
@pytest.mark.parametrize("n_bytes,n", [(200 * 10**9, 700 * 10**6), (3_000_000, 20_000)])
def test_a_budget_that_fits_nothing_names_the_minimum(n_bytes, n, markdup):
    least = minimum(n_bytes, n, markdup)
    assert least > 48 * n
    p = api.bam_sort_plan(n_bytes, n, least, markdup)
    slice_bytes = DEFAULT_SLICE * MEMBER
    assert p["external"] == 1 and p["partition_bytes"] == slice_bytes and p["device_bytes"] == least
    with pytest.raises(api.UrmapxError) as e:
        api.bam_sort_plan(n_bytes, n, least - 1, markdup)
    assert e.value.code == E_NOMEM and e.value.plan["device_bytes"] == least


def test_the_slice_knob_changes_the_slice_the_plan_counts_in(monkeypatch):
    n_bytes, n = 3_000_000, 20_000
    wide = api.bam_sort_plan(n_bytes, n, in_core(n_bytes, n, False) - 1)
    monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
    budget = in_core(n_bytes, n, False) - 4 * 65536
    p = api.bam_sort_plan(n_bytes, n, budget)
    assert p["external"] == 1 and p["partition_bytes"] % MEMBER == 0 and p["partition_bytes"] % (DEFAULT_SLICE * MEMBER) != 0
    assert p["partitions"] == -(-n_bytes // p["partition_bytes"]) >= 2 and p["device_bytes"] <= budget
    assert wide["partition_bytes"] == DEFAULT_SLICE * MEMBER and wide["partitions"] == 1
    q = api.bam_sort_plan(n_bytes, n, p["device_bytes"] + MEMBER)
    assert q["partition_bytes"] == p["partition_bytes"] + MEMBER


def test_the_partition_and_stage_knobs(monkeypatch):
    n_bytes, n = 3_000_000, 20_000
    monkeypatch.setenv("URMAPX_TEST_SORT_SLICE", "1")
    monkeypatch.setenv("URMAPX_TEST_SORT_PARTITION", "3")
    monkeypatch.setenv("URMAPX_TEST_SORT_STAGE", "4096")
    p = api.bam_sort_plan(n_bytes, n, 1 << 40)  # (a budget everything fits: the knob forces the road all the same)
    assert p["external"] == 1 and p["partition_bytes"] == 3 * MEMBER and p["partitions"] == -(-n_bytes // (3 * MEMBER)) and p["stage_bytes"] == 4096


@pytest.mark.parametrize("shape", [(200 * 10**9, 700 * 10**6, 1), (3_000_000, 20_000, 0), (0, 0, 0)])
def test_the_plan_under_the_sanitizers(san, shape):  # noqa: F811
    """the stand-alone sanitizer program (make san) sweeps the budgets: every plan within its budget, the partition count never rising;
    the pipeline's planned call and its refusal through the stand-in device"""
    rc, out = san_run(san["asan"], ["plan"] + list(shape))
    assert rc == 0 and "rc=0 partitions=0" in out, out


def test_sort_mem_through_the_pipeline_under_the_sanitizers(san, tmp_path):  # noqa: F811
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"ACGT" * 10, b"I" * 40) for i in range(300)))
    out = tmp_path / "o.bam"
    for mem, want in (("64G", 0), ("1", 1)):
        rc, text = san_run(san["asan"], ["map", fq, "-o", out, "-bam", "-sort", "-sortmem", mem])
        assert rc == want, text
        if want:
            assert "at least" in text and "sort_mem" in text and not out.exists() and not (tmp_path / "o.bam.bai").exists()
        else:
            assert out.exists() and (tmp_path / "o.bam.bai").exists()
    rc, text = san_run(san["asan"], ["map", fq, "-o", out, "-bam", "-sortmem", "1G"])
    assert rc == 1 and "sort_mem needs bam_sort" in text


IN_CORE, MARKING, PLANNED, DEPTH = "urmapx_bam_sort", "urmapx_bam_sort_markdup", "urmapx_bam_sort_external", "urmapx_bam_sort_with"
G = 1 << 30
# options, the device-sort calls the stand-in refuses, the calls it then sees (entry, budget; None: an in-core entry), does the run end well
LADDER = [
    ([], 0, [(IN_CORE, None)], True),
    ([], 1, [(IN_CORE, None)] * 2, True),
    ([], 2, [(IN_CORE, None)] * 2 + [(PLANNED, 0)], True),
    (["-markdup"], 0, [(MARKING, None)], True),
    (["-markdup"], 2, [(MARKING, None)] * 2 + [(PLANNED, 0)], True),
    (["-sortmem", "1G"], 1, [(PLANNED, G)] * 2, True),
    (["-sortmem", "1G"], 2, [(PLANNED, G)] * 2, False),
    (["-depth"], 0, [(DEPTH, 0)], True),
    (["-depth"], 1, [(DEPTH, 0)] * 2, True),
]


def test_the_order_in_which_the_device_sorts_are_tried(san, tmp_path):  # noqa: F811
    """the ladder of Run::write_sorted's sort (pipeline.cpp) through the stand-in device, which finds the device full K times
    (URX_STUB_SORT_NOMEM) and says which entry was called with what budget: in core twice, then planned from what is free; a planned
    sort (sort_mem, depth_out) twice and nothing else; then the refusal, which leaves no file.  Whatever the rung, the files are those
    of the run that was never refused."""
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"ACGT"[i % 4:] + b"ACGT" * 9, b"I" * (40 - i % 4)) for i in range(300)))
    want = {}
    for n, (extra, k, calls, ok) in enumerate(LADDER):
        out, bed = tmp_path / f"{n}.bam", tmp_path / f"{n}.bedgraph"
        args = ["map", fq, "-o", out, "-biglen", "300000", "-bam", "-sort"] + [a for e in extra for a in ([e, bed] if e == "-depth" else [e])]
        rc, text = san_run(san["asan"], args, env={"URX_STUB_MAP": "1", "URX_STUB_SORT_NOMEM": str(k)})
        seen = [l.split() for l in text.splitlines() if l.startswith("stub sort: ")]
        assert [(w[2], int(w[4]) if len(w) > 3 else None) for w in seen] == calls, text
        bai = tmp_path / f"{n}.bam.bai"
        if not ok:
            assert rc == 1 and "rc=-3" in text and "bam_sort: out of device memory: the plan takes " in text, text
            assert not out.exists() and not bai.exists()
            continue
        assert rc == 0, text
        files = (out.read_bytes(), bai.read_bytes(), bed.read_bytes() if "-depth" in extra else None)
        assert len(files[0]) > 1000 and len(files[1]) > 8
        # (marking changes the records' flags; the budget and the depth change nothing of the BAM file)
        assert files == want.setdefault(("-markdup" in extra, "-depth" in extra), files), (extra, k)
    assert want[False, False][:2] == want[False, True][:2] and want[False, True][2]
    assert want[False, False] != want[True, False]


def test_an_empty_input_plans_no_partition():
    p = api.bam_sort_plan(0, 0, 1 << 40)
    assert p["external"] == 0 and p["partitions"] == 0
