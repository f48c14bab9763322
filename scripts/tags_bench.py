#!/usr/bin/env python3
"""Measures -tags / -rg (urmap_amd/csrc/tags_gpu.hip) on one GPU and prints one JSON object:

  file     `urmap -map reads.fq` file to file through urmapx_map_files, SAM and BAM, without the options and with
           `-tags NM,MD,AS -rg @RG\\tID:bench\\tSM:s`: per run the report's seconds (first read parsed to last byte written), the summed
           dev_format_s of the lanes and sam_text_bytes; per variant the median and the spread (max - min) of --rounds runs, the
           first left out (it also pages the FASTQ in).  --parent ROOT runs the plain variants of ANOTHER build's library (the parent
           commit's tree, built beside this one) on the same files in the same rounds: the run without the options is held against it,
           with the parent's own spread as the margin.  Every run is a process of its own (one library per process).
  kernel   one chunk of --kernel-reads records through the text stage, by events: ms_format without and with the options, and the two
           tag passes alone (urmapx_text_tag_ms), SAM and BAM, per 1 M records; median of --steps chunks after a warm-up

The reads are those of scripts/bgzf_bench.py (same generator, same seed).

    python scripts/tags_bench.py [--reads 10000000] [--genome-mbp 20] [--rounds 4] [--steps 5] [--parent ROOT] [--out-dir DIR] [--out DIR]

--out-dir: where the genome, the reads and the output files of the runs go (the medium that is measured; default: a temporary directory).
--out: a directory that receives the JSON line as tags_bench.json.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RG = "@RG\tID:bench\tSM:s"


def worker(root, fq, ufi, out, bam, tagged):
    """one file-to-file run with the library of the tree at `root`, in this process -> the report's numbers as JSON"""
    sys.path.insert(0, root)
    from urmap_amd import api
    idx = api.Index.open_device(ufi, 0) if hasattr(api.Index, "open_device") else api.Index.open(ufi)
    kw = dict(samout=out, bam=bool(bam), cmdline="tags_bench ")
    if tagged:
        kw.update(tags=api.TAG_ALL, read_group=RG)
    rep = api.map_files(idx, fq, **kw)
    keep = ("reads", "seconds", "dev_format_s", "dev_map_s", "dev_d2h_s", "sam_text_bytes", "sam_file_bytes", "text_on_device", "lanes")
    print(json.dumps({k: rep[k] for k in keep}))


def run_worker(root, fq, ufi, out, bam, tagged):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root, fq, ufi, out, str(int(bam)), str(int(tagged))],
                       capture_output=True, text=True, timeout=1800)
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().split("\n")[-1])


def summarise(runs):
    import numpy as np
    kept = runs[1:] or runs
    out = {"runs": runs}
    for k in ("seconds", "dev_format_s"):
        v = [r[k] for r in kept]
        out[k] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    out["sam_text_bytes"] = runs[-1]["sam_text_bytes"]
    out["reads_per_s_median"] = runs[-1]["reads"] / out["seconds"]["median"]
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5], int(sys.argv[6]), int(sys.argv[7]))
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from bgzf_bench import CLI, medium_of, write_fastq
    from urmap_amd import api, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-mbp", type=float, default=20.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=4, help="file-to-file runs per variant; the first is left out of the median")
    ap.add_argument("--kernel-reads", type=int, default=1 << 20)
    ap.add_argument("--parent", default=None, help="root of the parent commit's tree, built")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(2026)
    res = {}
    with tempfile.TemporaryDirectory(dir=args.out_dir) as d:
        g = synth.make_genome(5, [int(args.genome_mbp * 1e6)], repeat_frac=0.05, n_families=8)
        fa, ufi, fq = os.path.join(d, "g.fa"), os.path.join(d, "g.ufi"), os.path.join(d, "r.fq")
        synth.write_fasta(fa, g)
        subprocess.run([CLI, "-make_ufi", fa, "-output", ufi, "-quiet"], check=True, capture_output=True, timeout=1800)
        write_fastq(fq, rng, g[0][1], args.reads, 150)
        res.update(reads=args.reads, fastq_bytes=os.path.getsize(fq), medium=medium_of(d))
        out = os.path.join(d, "out")
        variants = [("sam", ROOT, 0, 0), ("sam_tagged", ROOT, 0, 1), ("bam", ROOT, 1, 0), ("bam_tagged", ROOT, 1, 1)]
        if args.parent:
            variants += [("parent_sam", args.parent, 0, 0), ("parent_bam", args.parent, 1, 0)]
        runs = {v[0]: [] for v in variants}
        for k in range(args.rounds):  # the variants take turns, round after round: a drift of the machine falls on all of them alike
            for name, root, bam, tagged in variants:
                runs[name].append(run_worker(root, fq, ufi, out, bam, tagged))
            print(f"round {k}: " + ", ".join(f"{n} {v[-1]['seconds']:.3f} s" for n, v in runs.items()), file=sys.stderr, flush=True)
        res["file"] = {n: summarise(v) for n, v in runs.items()}
        res["file"]["rounds"] = args.rounds
        if os.path.exists(out):
            os.remove(out)
        # the format stage of one chunk, by events
        with open(fq, "rb") as fh:
            chunk = fh.read(400 * args.kernel_reads)
        lines = chunk.split(b"\n")
        nrec = min(args.kernel_reads, (len(lines) - 1) // 4)
        chunk = b"\n".join(lines[:4 * nrec]) + b"\n"
        m = api.Mapper(api.Index.open(ufi).upload(0), device=0)
        kern = {"records": nrec}
        for name, bam, tagged in (("sam", False, False), ("sam_tagged", False, True), ("bam", True, False), ("bam_tagged", True, True)):
            m.set_bam(bam)
            m.set_tags(api.TAG_ALL if tagged else 0, "bench" if tagged else None)
            ms, t0, t1, nbytes = [], [], [], 0
            for step in range(args.warmup + args.steps):
                (z, rep), = m.map_text_se_stream([chunk])
                assert rep["reason"] == api.TEXT_OK and rep["records"] == nrec, rep
                nbytes = rep["sam_text_bytes"]
                if step >= args.warmup:
                    ms.append(rep["ms_format"])
                    a, b = m.tag_ms()
                    t0.append(a); t1.append(b)
            per = 1e6 / nrec
            kern[name] = {"ms_format": ms, "ms_format_per_1M": float(np.median(ms)) * per, "tag_len_ms_per_1M": float(np.median(t0)) * per,
                          "tag_write_ms_per_1M": float(np.median(t1)) * per, "bytes_per_record": nbytes / nrec}
        m.set_bam(False)
        m.set_tags(0, None)
        m.close()
        res["kernel"] = kern
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "tags_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
