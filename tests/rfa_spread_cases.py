"""The inputs of test_emu_rfa_spread.py and test_gpu_rfa_spread.py.  In the small instance of K8's barcode program (k_rfa.h: k_rfa<1>) a barcode of at most 32
molecules gives every sink of fastScore G = 64 / (M rounded up to a power of two, at least 2) lanes, which read G * 4 of the source's active alignments a step
(dev_fast_score_spread), and the molecule status shares a molecule's alignments among lanes in the same way.  The cases cover every group width, the one-lane form
beyond 32 molecules, and sources of one alignment, of a partial step and of more than one step.  rfa_small_cases.check() holds each batch to the oracle, byte for
byte to the same batch in the regular instance (LH_F_RFA_SLAB) and to a second run.

What a batch covers is asserted from the oracle's result, not from the generator's arguments: scrapMolecules and the 50 kb rule decide how many molecules come out.
helpers.small_genome() (600 kb in three contigs) yields at most about six molecules a barcode — two alignments 50 kb apart on a contig share a molecule —, so the
classes from nine molecules on come from a genome of 56 contigs of 12 kb (synth.make_genome), where a molecule has a contig to itself."""
import numpy as np

import helpers
import rfa_small_cases as rc
import tail_pass_cases as tp
from lariat_amd import synth

U = 4   # alignments a sub-lane reads per step (k_rfa.h)
CLASSES = [(1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32)]   # molecules per barcode: one class per group width G = 32, 32, 16, 8, 4, 2


def group_width(m):
    p = 2
    while p < m:
        p *= 2
    return 64 // p


def many_contig_genome():
    names = ["c%02d" % i for i in range(56)]
    return names, synth.make_genome([12000] * 56, seed=4, n_dup=40, dup_len=2500, dup_identity=0.99)   # (duplications: reads with an alignment in another molecule, the moves fastScore weighs)


def spread_shapes(ores, bc_pair_off):
    """per barcode: reads, candidates, molecules, and the molecules' active-alignment counts (the sources of the probability sums), from the oracle's result"""
    out = []
    for b, (nr, nc, m) in enumerate(rc.shape_of(ores, bc_pair_off)):
        r0, r1 = 2 * int(bc_pair_off[b]), 2 * int(bc_pair_off[b + 1])
        c0, c1 = int(ores.cand_off[r0]), int(ores.cand_off[r1])
        mid, act = ores.molecule_id[c0:c1], ores.active[c0:c1]
        counts = np.bincount(mid[(mid >= 0) & (act != 0)], minlength=m) if m else np.zeros(0, dtype=np.int64)
        out.append((nr, nc, m, [int(x) for x in counts]))
    return out


# (molecules asked of the generator, pairs a barcode, barcodes, seed): what comes out is asserted by covered() below
SMALL_GENOME = [(1, 6, 1, 11), (2, 12, 1, 11), (5, 8, 6, 3), (12, 16, 6, 3), (8, 100, 2, 3)]
MANY_CONTIGS = [(12, 40, 1, 3), (30, 100, 1, 3), (70, 100, 1, 3)]


def split_pairs(contigs, first, n_pairs):
    """a barcode whose pairs have their reads on two different contigs: molecules of ONE active alignment (the model is rfa_small_cases.chimeric_case)"""
    reads = []
    for p in range(n_pairs):
        reads += [contigs[first + 2 * p][100:250].copy(), tp._rc(contigs[first + 2 * p + 1][300:450])]
    return tp._read_set(reads, ["split:%d" % p for p in range(n_pairs)], [0, n_pairs])


def _reads(names, contigs, specs, extra, seed_one):
    sets = [synth.make_reads(contigs, names, n_barcodes=nb, pairs_per_barcode=pairs, seed=seed, mol_min=k, mol_max=k, junk_frac=0.0) for k, pairs, nb, seed in specs] + extra
    sets.append(synth.make_reads(contigs, names, n_barcodes=1, pairs_per_barcode=6, seed=seed_one + 1, mol_min=2, mol_max=2, junk_frac=0.0))   # a barcode without inference
    sets.append(synth.make_reads(contigs, names, n_barcodes=1, pairs_per_barcode=1, seed=seed_one, junk_frac=0.0))   # a barcode of one pair
    rs = rc.join_read_sets(sets)
    do_rfa = np.ones(len(rs.bc_pair_off) - 1, dtype=np.uint8)
    do_rfa[-2] = 0
    return rs, do_rfa


def case(which):
    names, contigs = helpers.small_genome() if which == "small_genome" else many_contig_genome()
    if which == "small_genome":
        rs, do_rfa = _reads(names, contigs, SMALL_GENOME, [], 77)
    else:
        rs, do_rfa = _reads(names, contigs, MANY_CONTIGS, [split_pairs(contigs, 40, 3)], 77)
    return names, contigs, rs, do_rfa


def covered(shapes, do_rfa, caps=rc.DEFAULT_CAPS):
    """the molecule classes and the source lengths the barcodes with inference inside the small caps cover"""
    small = [s for s, d in zip(shapes, do_rfa) if d and s[0] <= caps["nr"] and s[1] <= caps["nc"] and 0 < s[2] <= caps["m"]]
    classes = {c for c in CLASSES if any(c[0] <= s[2] <= c[1] for s in small)}
    spread = [s for s in small if s[2] <= 32]
    return dict(classes=classes, old_form=any(s[2] > 32 for s in small),
                one=any(1 in s[3] for s in spread if s[2] > 1),
                partial=any(n % (group_width(s[2]) * U) for s in spread if s[2] > 1 for n in s[3] if n > 0),
                two_steps=any(n > group_width(s[2]) * U for s in spread if s[2] > 1 for n in s[3]))


def check_case(lib, oracle, which, caps=rc.DEFAULT_CAPS):
    names, contigs, rs, do_rfa = case(which)
    assert rs.bc_pair_off[-1] - rs.bc_pair_off[-2] == 1 and int(np.diff(rs.bc_pair_off).max()) <= 100
    ores, _, cls = rc.check(lib, oracle, names, contigs, rs, caps, do_rfa=do_rfa)
    return covered(spread_shapes(ores, rs.bc_pair_off), do_rfa, caps), cls


def assert_cover(cov):
    """both cases together: every group width, the one-lane form, the three source lengths"""
    assert cov["classes"] == set(CLASSES), sorted(set(CLASSES) - cov["classes"])
    assert cov["old_form"], "no barcode of more than 32 molecules within the small caps"
    assert cov["one"] and cov["partial"] and cov["two_steps"], cov


def merge(a, b):
    return {k: (a[k] | b[k]) for k in a}
