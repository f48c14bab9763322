"""The single-end search kernels' slot entries on the slot16 layout: one 12-byte LDS-DMA per k-mer brings the three dwords of an entry
(position, tally | row length << 8, second position or row index) into LDS as entry e = dwords 3 * e .. 3 * e + 2 (kernels.hip:
SearchWave::probe_gather, probe_get, walk_heads).  What can go wrong is in the lanes and chunks at the edges -- a chunk of 64 k-mer
starts with one valid lane, lanes without a k-mer in the middle of a chunk, the last chunk of every instance class -- and in the second
and third dword, which only chains with rows use.  Every batch is compared with the oracle read by read (test_gpu_parity's
compare_results: hit, scores, MAPQ, hit count, exit phase, path)."""
import os

import numpy as np
import pytest

from test_gpu_parity import compare_results, dense_case, gpu, mutate_edge_reads  # noqa: F401 (gpu, dense_case: fixtures)

pytestmark = pytest.mark.gpu


def _one_read(seed, genome, L):
    from urmap_amd import synth
    for k in range(50):  # (make_reads drops a read that its deletions left short)
        r = synth.make_reads(seed + 7919 * k, genome, 1, read_len=int(L), sub=0.02, ins=0.002, dele=0.002)
        if r:
            return r[0]
    raise AssertionError(f"no read of {L} bases")


def edge_batch(genome, w, hi, seed, n=600):
    """Reads for the instance class of `hi` bases at word length w: every length from w to hi; exactly w bases (one k-mer: 63 lanes of
    its chunk gather the zero entry); 63, 64, 65, 127, 128 and 129 k-mer starts (a chunk with one valid lane, either side of it), twice
    each; reads with an N, an IUPAC letter or a lower-case stretch in the middle of a chunk (lanes without a k-mer between lanes with
    one) as drawn and reverse-complemented; filled up to n reads with reads of hi bases; then test_gpu_parity's sprinkled letters."""
    from urmap_amd import synth
    lens = list(range(w, hi + 1)) + [w, w]
    for starts in (63, 64, 65, 127, 128, 129):
        if starts + w - 1 <= hi:
            lens += [starts + w - 1] * 2
    lens += [hi] * max(0, n - 12 - len(lens))
    reads = [_one_read(seed + 31 * i, genome, L) for i, L in enumerate(lens)]
    reads = mutate_edge_reads(reads, seed)
    rng = np.random.default_rng(seed)
    for j, letter in enumerate((ord("N"), ord("R"), None)):
        for L in (hi, min(hi, 100 + w)):
            lab, s, q = _one_read(seed + 100003 + 17 * j + L, genome, L)
            s = s.copy()
            p = int(rng.integers(w, L - w + 1)) if L > 2 * w else L // 2
            if letter is None:
                s[p:p + 5] |= 0x20  # lower case: the k-mers stay, the letters go through the case fold
            else:
                s[p] = letter
            reads.append((lab + "_e", s, q))
            reads.append((lab + "_erc", np.ascontiguousarray(synth.revcomp(s)), q))
    return reads


def _mapped_by_oracle(oi, reads):
    from conftest import reads_to_arrays
    bases, offs = reads_to_arrays(reads)
    ores, opaths, _ = oi.map_se(bases, offs, threads=4)
    return bases, offs, ores, opaths


@pytest.fixture(scope="module")
def batch150(small_case):
    """the 150-base batch on the small index and what the oracle makes of it (tests A and C)"""
    return _mapped_by_oracle(small_case["oracle_index"], edge_batch(small_case["genome"], 24, 150, 150))


@pytest.mark.parametrize("hi", [128, 150, 192, 250, 320, 512, 1000])
def test_every_instance_class_reads_its_entries(small_case, gpu, batch150, hi):
    """Test A: one batch per instance class at W = 24 (longest read 128: two chunks; 150: two chunks of k-mer starts in a three-chunk
    read; 192: three; 250: four; 320: five; 512: eight; 1 000: sixteen)."""
    if hi == 150:
        bases, offs, ores, opaths = batch150
    else:
        bases, offs, ores, opaths = _mapped_by_oracle(small_case["oracle_index"], edge_batch(small_case["genome"], 24, hi, hi))
    lens = np.diff(offs.astype(np.int64))
    assert lens.max() == hi and lens.min() == 24 and len(np.unique(lens)) == hi - 24 + 1
    assert (ores["dbpos"] != 0xFFFFFFFF).mean() > 0.5
    gres, gops = gpu["mapper"].map_se(bases, offs)
    compare_results(gres, gops, ores, opaths)


@pytest.mark.parametrize("w", [24, 16, 30])
def test_dense_index_rows_use_all_three_dwords(dense_case, workdir, tmp_path, w):
    """Test B: the 150-base batch on the dense index (load 0.95: rows of three and more, long links): chain heads there carry a row
    length above 2 in the second dword's second byte and a row index in the third.  W = 16: 135 k-mer starts, the three-chunk instance;
    W = 24 and 30: the two-chunk one."""
    import oracle_lib as ol
    from urmap_amd import api
    if w == 24:
        oi, idx, m = dense_case["oracle_index"], None, dense_case["mapper"]
    else:
        oi = ol.Index.build(os.path.join(workdir, "dense.fa"), 578_041, word_length=w)
        ufi = os.path.join(tmp_path, f"dense_w{w}.ufi")
        oi.save(ufi)
        idx = api.Index.open(ufi).upload(0)
        m = api.Mapper(idx, device=0, method=6)
    assert (dense_case["index"] if idx is None else idx).chain_row_bytes() > 0  # the slot16 table and the rows are resident
    bases, offs, ores, opaths = _mapped_by_oracle(oi, edge_batch(dense_case["genome"], w, 150, 1000 + w))
    assert int(ores["hit_count"].max()) > 1  # reads with more than one candidate: chains were followed
    gres, gops = m.map_se(bases, offs)
    compare_results(gres, gops, ores, opaths)
    if idx is not None:
        m.close()
        idx.close()


def test_two_and_three_chunk_instances_agree_with_the_oracle(gpu, batch150, monkeypatch):
    """Test C: the 150-base batch twice on one Mapper, by the two-chunk instance and (URMAPX_NO_K2) by the three-chunk one."""
    bases, offs, ores, opaths = batch150
    m = gpu["mapper"]
    gres, gops = m.map_se(bases, offs)
    compare_results(gres, gops, ores, opaths)
    monkeypatch.setenv("URMAPX_NO_K2", "1")
    gres3, gops3 = m.map_se(bases, offs)
    compare_results(gres3, gops3, ores, opaths)
