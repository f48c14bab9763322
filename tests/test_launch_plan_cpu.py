"""The decisions of the single-end launcher (urmap_amd/csrc/launch_plan.h), on the CPU: which search_se_kernel instance runs for which index,
read class and knob, and what URMAPX_DP_BOUNDS is parsed to.

tests/tools/launch_plan_main.cpp is compiled with g++ under ASan + UBSan and run as a child process; it prints the plan for every
combination of inputs.  The rows spelled out below were written by hand from the if / else ladder the plan replaced.

The layout of the work buffer's head (kernels.h: DpHead -- counters at bytes 0 / 16 / 32, work counters at 64 / 128 / 192, 256 bytes) is held
by a static_assert next to the struct: kernels.h needs the HIP headers, so it is the library's build that checks it, not this file."""
import itertools
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
SO = os.path.join(ROOT, "urmap_amd", "liburmapx.so")
CLASSES = (2, 3, 4, 5, 8, 16)
LENS = (150, 151, 152, 192)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "launch_plan_main.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def plan(prog):
    """{(nch, rowinfo, slot16, stats, phase6, park3, len, no_k2): ([the first pass's kernels], phase 6 as launches, the second pass's kernel)}"""
    out = subprocess.run([prog], capture_output=True, text=True, check=True).stdout
    table = {}
    for ln in out.strip().split("\n"):
        key, kernels, p6, second = [f.strip() for f in ln.split("|")]
        k = dict(kv.split("=") for kv in key.split())
        table[tuple(int(k[f]) for f in ("nch", "rowinfo", "slot16", "stats", "phase6", "park3", "len", "no_k2"))] = (
            kernels.split(" + "), p6 == "phase6=1", second.replace("second: ", ""))
    assert len(table) == len(CLASSES) * 2 ** 6 * len(LENS)  # every combination, once
    return table


def first(plan, nch, rowinfo, slot16, stats=0, phase6=1, park3=0, length=150, no_k2=0):
    return plan[(nch, rowinfo, slot16, stats, phase6, park3, length, no_k2)]


def test_the_rows_of_the_resource_table_are_reached_from_the_inputs_their_comments_name(plan):
    # 150-base reads on a default index (row layout dropped once slot16 is built; with both it is the same): two chunks of k-mer starts
    for rowinfo in (0, 1):
        assert first(plan, 3, rowinfo, 1) == (["search_se_kernel<3, false, false, 2, 0, 2>"], True, "search_se_kernel<3, true, false, 0, 0, 3>")
    # 151 bases at W = 24 are 128 k-mer starts, 152 are 129: the boundary of the two-chunk instance; URMAPX_NO_K2 takes it away
    assert first(plan, 3, 0, 1, length=151)[0] == ["search_se_kernel<3, false, false, 2, 0, 2>"]
    assert first(plan, 3, 0, 1, length=152)[0] == ["search_se_kernel<3, false, false, 2, 0, 3>"]
    assert first(plan, 3, 0, 1, length=192)[0] == ["search_se_kernel<3, false, false, 2, 0, 3>"]
    assert first(plan, 3, 0, 1, length=150, no_k2=1)[0] == ["search_se_kernel<3, false, false, 2, 0, 3>"]
    assert first(plan, 4, 0, 1)[0] == ["search_se_kernel<4, false, false, 2, 0, 4>"]  # 250-base reads
    assert first(plan, 2, 0, 1)[0] == ["search_se_kernel<2, false, false, 2, 0, 2>"]  # reads of up to 128 bases
    assert first(plan, 3, 1, 0)[0] == ["search_se_kernel<3, false, false, 1, 0, 3>"]  # an index without slot16 (row layout only)
    # URMAPX_PARK_PHASE3=1 (the index then keeps its row layout beside slot16): the two search launches around phase 3's DP launch
    for slot16 in (0, 1):
        assert first(plan, 3, 1, slot16, park3=1) == (
            ["search_se_kernel<3, false, false, 1, 1, 3>", "dp_kernel<3>", "search_se_kernel<3, false, false, 1, 2, 3>"], True, "search_se_kernel<3, true, false, 0, 0, 3>")


def test_the_other_arms_of_the_ladder(plan):
    # neither layout: hop by hop, every class; phase 6 inline (URMAPX_INLINE_PHASE6) changes no instance
    for nch in CLASSES:
        for phase6 in (0, 1):
            assert first(plan, nch, 0, 0, phase6=phase6) == ([f"search_se_kernel<{nch}, false, false, 0, 0, {nch}>"], bool(phase6), f"search_se_kernel<{nch}, true, false, 0, 0, {nch}>")
        assert first(plan, nch, 1, 0)[0] == [f"search_se_kernel<{nch}, false, false, 1, 0, {nch}>"]
        assert first(plan, nch, 1, 1)[0][0].startswith(f"search_se_kernel<{nch}, false, false, 2, 0, ")
    # diagnostics: the 150 / 250 bp classes have instances of their own with phase 6 inline, whatever the index holds; the other
    # classes run the row-layout or hop-by-hop instance with the counters (never slot16), phase 6 as launches
    for rowinfo, slot16, park3 in itertools.product((0, 1), repeat=3):
        assert first(plan, 3, rowinfo, slot16, stats=1, park3=park3) == (["search_se_kernel<3, false, true, 0, 0, 3>"], False, "search_se_kernel<3, true, false, 0, 0, 3>")
        assert first(plan, 4, rowinfo, slot16, stats=1, park3=park3)[:2] == (["search_se_kernel<4, false, true, 0, 0, 4>"], False)
        for nch in (2, 5, 8, 16):
            assert first(plan, nch, rowinfo, slot16, stats=1, park3=park3)[:2] == ([f"search_se_kernel<{nch}, false, false, {rowinfo}, 0, {nch}>"], True)
    # phase 3 parked needs phase 6's launches (its reads go on to them)
    assert first(plan, 3, 1, 1, phase6=0, park3=1)[0] == ["search_se_kernel<3, false, false, 2, 0, 2>"]
    # the classes beyond 320 bases keep phase 3 inline
    assert first(plan, 8, 1, 1, park3=1)[0] == ["search_se_kernel<8, false, false, 2, 0, 8>"]
    assert first(plan, 16, 1, 0, park3=1)[0] == ["search_se_kernel<16, false, false, 1, 0, 16>"]


def test_restrictions_hold_over_every_combination(plan):
    for (nch, rowinfo, slot16, stats, phase6, park3, length, no_k2), (kernels, p6, second) in plan.items():
        a = [int(x) if x.isdigit() else x for x in re.match(r"search_se_kernel<(.*)>$", kernels[0]).group(1).split(", ")]
        if a[4] != 0:  # parked phase 3
            assert rowinfo and nch <= 5 and not stats and phase6 and park3 and len(kernels) == 3
        else:
            assert len(kernels) == 1
        if a[2] == "true":  # diagnostic
            assert nch in (3, 4) and stats and not p6
        if a[5] != a[0]:  # fewer chunks of k-mer starts than byte chunks: the one instance <3, ..., 2, 0, 2>
            assert a == [3, "false", "false", 2, 0, 2] and length <= 151 and not no_k2
        assert a[0] == nch and a[1] == "false" and p6 == bool(phase6 and a[2] == "false")


def test_every_instance_the_plan_names_is_in_the_library(plan):
    import kernel_meta
    if not os.path.exists(SO):
        pytest.fail(f"{SO} is missing: run __graft_entry__.build() first")
    table = kernel_meta.kernel_table(SO)
    names = {k for kernels, _, second in plan.values() for k in kernels + [second]}
    assert len(names) == 6 + 6 + 6 + 1 + 2 + 6 + 3 * 4  # hops, rows, slot16, its two-chunk instance, diagnostic, second pass, phase 3 parked: three launches in four classes
    assert not sorted(names - set(table))


@pytest.mark.parametrize("text,want", [
    ("0,2,8,32", "4 0 2 8 32 4294967295"),
    ("0,5", "2 0 5 4294967295 4294967295 4294967295"),
    # the default stays when the first bound is not 0, when the bounds do not rise and when there is no number at all
    # what follows a number that is no comma-separated number ends the list; so does the fourth number (DP_ROUNDS)
    ("1,2", None), ("0,2,2", None), ("", None), ("x", None),
    ("0,x", "1 0 4294967295 4294967295 4294967295 4294967295"), ("0,1,2,3,4", "4 0 1 2 3 4294967295"),
])
def test_dp_bounds_parser(prog, text, want):
    got = subprocess.run([prog, "bounds", text], capture_output=True, text=True, check=True).stdout.strip()
    assert got == (want or "3 0 2 16 4294967295 4294967295")
