"""Register / spill / scratch / LDS figures of every gfx950 kernel inside the shipped liburmapx.so (test infrastructure).

The library's .hip_fatbin section holds one clang offload bundle per translation unit; each bundle's gfx950 entry is an ELF
code object whose NT_AMDGPU_METADATA note lists, per kernel, what the compiler allocated.  Nothing is compiled here: the
numbers are those of the binary that runs."""
import hashlib
import os
import re
import struct
import subprocess
import tempfile

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
OBJCOPY = "/opt/rocm/lib/llvm/bin/llvm-objcopy"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = {"vgpr": ".vgpr_count", "agpr": ".agpr_count", "sgpr": ".sgpr_count", "vgpr_spill": ".vgpr_spill_count", "sgpr_spill": ".sgpr_spill_count",
          "scratch": ".private_segment_fixed_size", "lds": ".group_segment_fixed_size", "max_threads": ".max_flat_workgroup_size"}


def code_objects(so_path):
    """bytes of every gfx950 code object bundled in the shared library"""
    raw = open(so_path, "rb").read()
    out, i = [], 0
    while True:
        i = raw.find(MAGIC, i)
        if i < 0:
            break
        n = struct.unpack_from("<Q", raw, i + 24)[0]
        p = i + 32
        if 0 < n < 16:
            for _ in range(n):
                off, size, ts = struct.unpack_from("<QQQ", raw, p)
                p += 24
                triple = raw[p:p + ts]
                p += ts
                if b"gfx950" in triple and size:
                    out.append(raw[i + off:i + off + size])
        i += len(MAGIC)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


def waves_per_simd(vgpr, agpr=0):
    """gfx950: 512 VGPRs per SIMD lane (unified with AGPRs), allocated in blocks of 8, at most 8 waves per SIMD"""
    tot = max(1, -(-(vgpr + agpr) // 8) * 8)
    return max(1, min(8, 512 // tot))


def _rows(elf_path):
    """{mangled kernel name: resource row} of one code object on disk"""
    table = {}
    txt = subprocess.run([READELF, "--notes", elf_path], capture_output=True, text=True, check=True).stdout
    for blk in re.split(r"\n  - \.agpr_count:", "\n" + txt)[1:]:
        blk = "    .agpr_count:" + blk
        m = re.search(r"\.name:\s+(\S+)", blk)
        if not m:
            continue
        row = {}
        for k, f_ in FIELDS.items():
            mm = re.search(re.escape(f_) + r":\s+(\d+)", blk)
            row[k] = int(mm.group(1)) if mm else 0
        row["waves_per_simd"] = waves_per_simd(row["vgpr"], row["agpr"])
        table[m.group(1)] = row
    return table


def _nice(table):
    """the same table keyed by the demangled kernel name without its argument list"""
    names = list(table)
    out = {}
    for mangled, nice in zip(names, demangle(names)):
        # "void urx::search_se_kernel<3, false, false, true>(urx::DevIndex, ...)" -> "search_se_kernel<3, false, false, true>"
        nice = re.sub(r"^void\s+", "", nice).replace("(anonymous namespace)::", "")  # (before the cut at the argument list's parenthesis)
        depth, cut = 0, len(nice)
        for j, ch in enumerate(nice):
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = j
                break
        nice = nice[:cut].replace("urx::", "").replace("(anonymous namespace)::", "")
        out[nice] = table[mangled]
    return out


def kernel_table(so_path):
    """{demangled kernel name without its argument list: {vgpr, agpr, sgpr, vgpr_spill, sgpr_spill, scratch, lds, max_threads, waves_per_simd}}"""
    table = {}
    for co in code_objects(so_path):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(co)
            f.flush()
            table.update(_rows(f.name))
    return _nice(table)


def code_digests(so_path):
    """One entry per code object (= translation unit with kernels), ordered by its kernel names: {kernels: the sorted names, text / rodata: sha256 of
    the section's bytes, rows: {name: resource row}}.  Two builds run the same device code iff these agree: the whole code object does not compare
    (its symbol table carries an id derived from the source text), the instructions and constants do."""
    out = []
    for co in code_objects(so_path):
        with tempfile.TemporaryDirectory() as d:
            elf = os.path.join(d, "co.elf")
            with open(elf, "wb") as f:
                f.write(co)
            rows = _nice(_rows(elf))
            if not rows:
                continue
            sha = {}
            for sec in (".text", ".rodata"):
                binp = os.path.join(d, "sec.bin")
                subprocess.run([OBJCOPY, "-O", "binary", "--only-section=" + sec, elf, binp], check=True)
                with open(binp, "rb") as f:
                    sha[sec] = hashlib.sha256(f.read()).hexdigest()
            out.append({"kernels": sorted(rows), "text": sha[".text"], "rodata": sha[".rodata"], "rows": rows})
    return sorted(out, key=lambda e: e["kernels"])


def _blank_pc_literals(lines):
    """the listing with the 32-bit literals of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 blanked: a pc-relative address (a call to
    a function that was not inlined, a constant's address), which moves with the order the compiler emitted the functions in"""
    out, after_getpc = [], 0
    for ln in lines:
        op = ln.split(None, 1)[0] if ln.strip() else ""
        if after_getpc and op == ("s_add_u32", "s_addc_u32")[2 - after_getpc]:
            ln = ln.rsplit(",", 1)[0] + ", <pcrel>"
            after_getpc -= 1
        else:
            after_getpc = 2 if op == "s_getpc_b64" else 0
        out.append(ln)
    return out


def function_digests(so_path):
    """sorted [(mangled name, sha256 of its disassembly with the pc-relative literals blanked)] over the FUNC symbols of every code object (a
    helper two translation units compile appears twice).  Unlike the sections' digests these do not depend on the order of the functions
    inside a code object."""
    out = []
    for co in code_objects(so_path):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(co)
            f.flush()
            syms = subprocess.run([READELF, "--symbols", "--wide", f.name], capture_output=True, text=True, check=True).stdout
            funcs = {ln.split()[7] for ln in syms.split("\n") if len(ln.split()) >= 8 and ln.split()[3] == "FUNC"}
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", f.name], capture_output=True, text=True, check=True).stdout
        body = {}
        cur = None
        for ln in txt.split("\n"):
            m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", ln)
            if m:
                if m.group(1) in funcs:
                    cur = body.setdefault(m.group(1), [])
                continue
            if cur is not None and ln.strip():
                cur.append(re.sub(r"\s+", " ", ln.split("//")[0].strip()))  # (behind "//": the address and the encoding, whatever the switches say)
        assert set(body) == funcs, sorted(funcs ^ set(body))
        for lines in body.values():
            while lines and lines[-1] == "...":  # zero bytes up to the next function's alignment: they depend on what follows
                lines.pop()
        out += [(name, hashlib.sha256("\n".join(_blank_pc_literals(lines)).encode()).hexdigest()) for name, lines in body.items()]
    return sorted(out)


def _print_rows(t, pat=""):
    print(f"{'kernel':64s} {'vgpr':>5s} {'sgpr':>5s} {'vspill':>6s} {'sspill':>6s} {'scratch':>7s} {'lds':>6s} {'waves':>5s}")
    for k in sorted(t):
        if pat in k:
            r = t[k]
            print(f"{k:64s} {r['vgpr']:5d} {r['sgpr']:5d} {r['vgpr_spill']:6d} {r['sgpr_spill']:6d} {r['scratch']:7d} {r['lds']:6d} {r['waves_per_simd']:5d}")


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = [a for a in sys.argv[1:] if a not in ("--digests", "--functions")]
    so = args[0] if len(args) > 0 else os.path.join(here, "urmap_amd", "liburmapx.so")
    if "--functions" in sys.argv[1:]:  # kernel_meta.py --functions [library]: name and digest of every device function, sorted
        for name, d in function_digests(so):
            print(name, d)
    elif "--digests" in sys.argv[1:]:  # kernel_meta.py --digests [library]: what has to agree between two builds of the same device code
        for n, e in enumerate(code_digests(so)):
            print(f"code object {n}: {len(e['kernels'])} kernels\n  .text   sha256 {e['text']}\n  .rodata sha256 {e['rodata']}")
            _print_rows(e["rows"])
            print()
    else:
        _print_rows(kernel_table(so), args[1] if len(args) > 1 else "")
