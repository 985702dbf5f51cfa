"""Reads at contig ends, on short contigs and in indices of thousands of contigs, on the device against the oracle.

  * the cases of test_emu_geometry.py (1,000 and 1,100 contigs: K8's contig tables in LDS and in the slab) under every flag set, index from arrays and
    from the device builder, ALT off and on;
  * a reference shaped like an analysis set: hg38's 24 primary contigs scaled to 30 Mb plus 3,000 short contigs (20 bp to 30 kb, some overlapping
    their neighbour, some ALT copies of primary sequence), 100 barcodes of 100-400 pairs of which about a tenth lie at junctions and ends — every
    result field, through FASTQ ingest; the same index saved and loaded back (.ann / .amb / .alt with thousands of entries); the BAM record text
    of the HIP result against oracle/bam_oracle.py on the oracle's; the BAM header's @SQ lines."""
import os
import sys

import numpy as np
import pytest

import helpers
from lariat_amd import capi, synth, workload
from test_emu_geometry import FLAGS, INDEX_ALT, run_geometry

pytestmark = pytest.mark.gpu
THREADS = min(os.cpu_count() or 8, 16)
COLS = ("name", "rgid", "qual1", "qual2", "trim_bases", "trim_quals", "bc", "rawbc", "bcqual", "si", "siqual")


@pytest.fixture(scope="module")
def lib():
    L = capi.load_library()
    assert L.device_count() >= 1
    return L


@pytest.mark.parametrize("n_contigs", [1000, 1100])
def test_geometry(lib, oracle, n_contigs):
    cov = run_geometry(lib, oracle, n_contigs, [(f, how, a) for f in FLAGS for how, a in INDEX_ALT], threads=THREADS)
    print("%d contigs: %s" % (n_contigs, cov[True]))


def analysis_set(seed=29, total=30000000, n_short=3000):
    """(names, contigs, alt, number of primary contigs): hg38-like primaries, then fragmented_genome's short contigs; an ALT contig longer than 200 bp is a
    copy of primary sequence at 1-3 % divergence (an alternate haplotype), so that reads on it have primary candidates too"""
    rng = np.random.default_rng(seed)
    prim = workload.hg38_like_contigs(total)
    names = [c[0] for c in prim[:-1]]
    contigs = [rng.choice(4, size=c[1], p=[0.295, 0.205, 0.205, 0.295]).astype(np.uint8) for c in prim[:-1]]
    fnames, fcontigs, alt = helpers.fragmented_genome(seed + 1, n_short + 1, long_lens=(prim[-1][1],), short_max=30000, alt_frac=0.05)
    names += [prim[-1][0]] + ["%s_%s" % ("alt" if a else "un", n) for n, a in zip(fnames[1:], alt[1:])]
    contigs += fcontigs
    for k in np.nonzero(alt)[0]:
        c = fcontigs[k]
        if len(c) > 200:
            src = contigs[int(rng.integers(0, len(prim) - 1))]
            at = int(rng.integers(0, len(src) - len(c)))
            seg = src[at:at + len(c)].copy()
            m = rng.random(len(c)) < rng.uniform(0.01, 0.03)
            seg[m] = (seg[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
            c[:] = seg
    return names, contigs, np.concatenate([np.zeros(len(prim) - 1, dtype=np.uint8), alt]), len(prim)


def analysis_reads(contigs, names, n_prim, seed=31, n_barcodes=100):
    """per barcode 100-400 pairs: nine tenths linked-read molecules on the primaries (synth.make_reads), one tenth geometry pairs on the whole reference"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(100, 401, size=n_barcodes)
    n_geo = np.maximum(1, sizes // 10)
    mol = synth.make_reads(contigs[:n_prim], names[:n_prim], n_barcodes=n_barcodes, pairs_per_barcode=int(sizes.max()), seed=seed + 1, junk_frac=0.01)
    geo = helpers.geometry_reads(contigs, list(n_geo), seed=seed + 2, kinds=("junction", "overhang", "inside_short", "split_mates", "ends", "rescue_edge"))
    reads, rnames = [], []
    for b in range(n_barcodes):
        p0 = int(mol.bc_pair_off[b])
        g0 = int(geo.bc_pair_off[b])
        for p in list(range(p0, p0 + int(sizes[b] - n_geo[b]))):
            reads += [mol.read(2 * p), mol.read(2 * p + 1)]; rnames.append(mol.names[p])
        for p in range(g0, g0 + int(n_geo[b])):
            reads += [geo.read(2 * p), geo.read(2 * p + 1)]; rnames.append(geo.names[p])
    rs = synth.ReadSet()
    lens = np.array([len(x) for x in reads], dtype=np.int64)
    rs.seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rs.seq = np.concatenate(reads)
    rs.bc_pair_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rs.names = rnames
    rs.name_seed = synth._name_seeds(rnames)
    rs.barcodes = mol.barcodes
    return rs


def test_analysis_set_shaped_reference(lib, oracle, tmp_path):
    sys.path.insert(0, os.path.join(helpers.ROOT, "oracle"))
    import bam_oracle
    import bam_reader
    names, contigs, alt, n_prim = analysis_set()
    lens = [len(c) for c in contigs]
    offs = np.concatenate([[0], np.cumsum(lens)])
    assert len(contigs) > 3000 and int(alt.sum()) > 50
    pac, l_pac, _, _ = lib.reference_pack(contigs)
    idx = lib.index_build_device(pac, l_pac, [(names[i], lens[i], int(offs[i])) for i in range(len(names))])
    oidx = oracle.index_from_arrays(idx.export(), pac)
    idx.set_alt(alt); oidx.set_alt(alt)
    prefix = str(tmp_path / "aset.fa")
    idx.save(prefix)
    assert open(prefix + ".ann").read().count("\n") >= 2 * len(contigs)
    li = lib.index_load(prefix)
    assert li.contigs() == idx.contigs() and li.alt() == list(alt)
    rs = analysis_reads(contigs, names, n_prim)
    path = str(tmp_path / "reads.fastq")
    open(path, "w").write(synth.to_fastq9(rs, trim_prefix=7))
    outdir = tmp_path / "bam"
    outdir.mkdir()
    w = lib.bam_writer(str(outdir), names, lens)
    ctx, lctx = idx.context(rs.n_pairs), li.context(rs.n_pairs)
    n_pairs, want_text = 0, []
    cov = None
    for b in lib.ingest(path, trim=7):
        ores = oidx.align_barcodes(b, threads=THREADS)
        res = ctx.align_barcodes(b)
        helpers.assert_same_result(res, ores, inference=True)
        helpers.assert_same_result(lctx.align_barcodes(b), ores, inference=True)
        got = lib.records_text(res, b, names)
        assert got == bam_oracle.records_text(ores, {c: b.column(c) for c in COLS}, b.seq, b.seq_off, b.bc_pair_off, b.set_complete, names)
        want_text += got.splitlines()
        w.append(res, b)
        c = helpers.geometry_coverage(lens, oidx.stage_dump(b), ores, b)
        cov = c if cov is None else {k: cov[k] + v if k != "max_filtered" else max(cov[k], v) for k, v in c.items()}
        n_pairs += b.n_pairs
    w.close()
    assert n_pairs == rs.n_pairs
    text, refs, lines = bam_reader.read_bam(str(outdir / "bc_sorted_bam.bam"))
    assert refs == list(zip(names, lens)) and text.count("@SQ") == len(contigs)
    assert [ln for ln, _ in lines] == want_text
    print("analysis set, %d contigs, %d pairs: %s" % (len(contigs), n_pairs, cov))
    helpers.assert_geometry_coverage(cov, bridging_seeds=50, regions_on_contig_end=20, cand_pos0=2, cand_aend_at_contig_end=2, soft_clips_at_contig_end=5,
                                     cand_on_contig_shorter_than_read=5, n_rescue=20,
                                     barcodes_under_256=0)   # (every barcode here has 100 pairs or more)
