"""Six-frame translated sketches (libhypergen_tx.so, include/hypergen_tx.h) on the GPU, all comparisons `==` against tests/tx_ref.py:
every t1ha2 tail-word boundary of k at the lengths where the window of 3k bases, the kernel's tile, the plan's work item or the
sequence end decide; the classification of all 256 byte values, non-bases and stops at every place of a window on both strands;
both strands and all three phases; the threshold at a hash and one above it; hit densities that overflow the LDS stage and
sets beyond the one-workgroup sort -- two k-mers per start, more than a plan for one would hold; the proteins of planted ORFs as
a subset; nucleotide, protein and translated calls with one ksize on one ctx over the same buffers; the command line end to end;
what is rejected."""
import gzip
import shutil
import subprocess

import numpy as np
import pytest
import torch

import aa_ref
import containment_ref as cr
import tx_census
import tx_ref

pytestmark = pytest.mark.gpu

KS = (1, 7, 8, 9, 16, 17, 24, 25, 31, 32)  # both ends of every kernel instantiation's range: the tail word is 1 byte / a whole word
BASES = np.frombuffer(b"ACGT", np.uint8)
MAX = 2**64 - 1
HV_D = 1024
STOPS = (b"TAA", b"TAG", b"TGA")
# codons that are no stop on either strand: a sequence of them is open in frame 0 and in the frame of the other strand on the same grid
OPEN = [c for c in ("".join((a, b, d)).encode() for a in "TCAG" for b in "TCAG" for d in "TCAG")
        if c not in STOPS and tx_ref.revcomp(c) not in STOPS]
# the first codon of every residue, for back-translation
CODON_OF = {}
for _i, _r in enumerate(tx_ref.CODONS):
    CODON_OF.setdefault(ord(_r), ("TCAG"[_i >> 4] + "TCAG"[(_i >> 2) & 3] + "TCAG"[_i & 3]).encode())


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_tx()
    hypergen_amd.lib_aa()
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    with hg.Context(0) as c:
        yield c


def dna(rng, n, lower=0.0):
    s = rng.choice(BASES, n)
    if lower:
        s = np.where(rng.random(n) < lower, s | 0x20, s).astype(np.uint8)
    return s


def open_dna(rng, codons):
    return np.frombuffer(b"".join(OPEN[i] for i in rng.integers(0, len(OPEN), codons)), np.uint8).copy()


def arr(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def back_translate(protein):
    return b"".join(CODON_OF[r] for r in bytes(protein))


def ref_rows(orc, sets, hv_d=HV_D, layout=1):
    hv = np.stack([orc.encode_hv(u, hv_d, layout) for u in sets]) if sets else np.zeros((0, hv_d), np.int16)
    return hv, np.array([orc.hv_norm2(r) for r in hv], np.int32), np.array([u.size for u in sets], np.uint32)


def same(got, want):
    return got.size == want.size and bool((got == want).all())


# ---- k and lengths -----------------------------------------------------------------------------------------------------------

def edge_lengths(hg, k):
    T, I, w = hg.tx_tile_starts(), hg.tx_item_starts(k), 3 * k
    return sorted({0, w - 1, w, w + 1, w + 2,
                   T - 1, T, T + 1, T + w - 2, T + w - 1, T + w,          # tile size +- 1 as a length and as a number of starts
                   I - 1, I, I + 1, I + w - 2, I + w - 1, I + w,          # item size +- 1 and + 3k - 1
                   2 * I + 1, 2 * I + w})                                   # two items + 1


@pytest.mark.parametrize("k", KS)
def test_every_tail_boundary_at_every_edge_length(hg, ctx, orc, k):
    rng = np.random.default_rng(100 + k)
    lens = edge_lengths(hg, k)
    T, I = hg.tx_tile_starts(), hg.tx_item_starts(k)
    base = dna(rng, lens[-1], lower=0.2)
    for at in rng.integers(0, base.size, 12):  # a dozen non-bases
        base[at] = ord("N")
    base[T - 1:T + 2] = arr(b"TAA")  # a stop codon across a tile edge ...
    base[I - 2:I + 1] = arr(b"tga")  # ... and one across the item edge
    scaled = 40
    sets = tx_ref.prefix_sets(base, k, lens, scaled)
    assert (sets[-1].size > 100 or k == 1) and same(sets[-1], tx_ref.hash_sample(base, k, scaled))  # (k = 1 has twenty k-mers in all)
    want_hv, want_n2, want_nh = ref_rows(orc, sets)
    p = hg.default_params(ksize=k, scaled=scaled, hv_d=HV_D)
    hv, n2, nh = ctx.tx_sketch_batch([base[:L] for L in lens], p)
    assert ctx.last_kernel("kmer") == hg.tx_kernel_name(k) and ctx.last_kernel("kmer") in [r.name for r in tx_census.ROWS if k in r.ksizes]
    assert nh.tolist() == want_nh.tolist(), (k, lens)
    assert (n2 == want_n2).all() and (hv == want_hv).all()
    for L in lens[:-2]:  # the hash lists themselves at the lengths around 3k, T and I
        got, want = ctx.tx_hash_sample(base[:L], k, scaled), sets[lens.index(L)]
        assert same(got, want), (k, L)


# ---- classification ----------------------------------------------------------------------------------------------------------

def test_all_256_byte_values_non_bases_and_stops_at_every_window_position(hg, ctx):
    k = 9
    w = 3 * k
    rng = np.random.default_rng(7)
    T = hg.tx_tile_starts()
    N, DASH = arr(b"N"), arr(b"-")
    parts = []
    for v in range(256):  # every byte value between two runs of bases
        parts += [open_dna(rng, k + 2), dna(rng, v % 3), np.array([v], np.uint8)]
    for j in range(w):  # a non-base at each position of a window: 3k - 1 bases on either side, no window is whole
        parts += [open_dna(rng, k)[:w - 1], N, open_dna(rng, k)[:w - 1], DASH]
    for stop in STOPS:  # each stop at each codon of an otherwise open window, on each strand, at each phase
        for strand in (0, 1):
            for j in range(k):
                run = open_dna(rng, k)
                run[3 * j:3 * j + 3] = arr(stop if strand == 0 else tx_ref.revcomp(stop))
                parts += [run, N, dna(rng, j % 3)]
    seq = np.concatenate(parts + [open_dna(rng, T + 40)])
    # a non-base as first and last start of a tile, and as first and last byte of what a tile stages (T + 96 bytes)
    for at in (T - 1, T, 2 * T - 1, 2 * T, T + 95, T + 96, 2 * T + 95, 3 * T - 1, 3 * T):
        seq[at] = ord("R")
    assert seq.size > 3 * T + w
    want = tx_ref.hash_sample(seq, k, threshold=MAX)  # every window is kept: a window hashed that should not be shows
    got = ctx.tx_hash_sample(seq, k, threshold=MAX, cap=want.size + 64)
    assert same(got, want)
    assert want.size > 8192 and "bucket_sort_kernel" in ctx.last_kernel("sort")
    # the stop runs alone: the open frame yields nothing, whatever the other frames do
    for stop in STOPS:
        for strand in (0, 1):
            for j in range(k):
                run = open_dna(np.random.default_rng(j), k)
                clean = tx_ref.frame_windows(run, k)
                assert len(clean[0]) == 1 and len(clean[3]) == 1
                run[3 * j:3 * j + 3] = arr(stop if strand == 0 else tx_ref.revcomp(stop))
                want = tx_ref.hash_sample(run, k, threshold=MAX)
                assert want.size == 1  # the other strand's window
                assert same(ctx.tx_hash_sample(run, k, threshold=MAX), want), (stop, strand, j)
    # three case variants of one sequence yield one set of hashes
    run = open_dna(np.random.default_rng(8), 40)
    one = tx_ref.hash_sample(run, k, threshold=MAX)
    assert one.size >= 2 * (40 - k + 1)
    for s in (run, run | 0x20, np.where(np.arange(run.size) % 2 == 0, run | 0x20, run).astype(np.uint8)):
        assert same(ctx.tx_hash_sample(s, k, threshold=MAX), one)
    for k2 in (1, 32):  # every byte value alone
        allb = np.concatenate([np.arange(256, dtype=np.uint8), dna(rng, 95), np.arange(256, dtype=np.uint8)[::-1]])
        want = tx_ref.hash_sample(allb, k2, threshold=MAX)
        assert same(ctx.tx_hash_sample(allb, k2, threshold=MAX), want)
        assert want.size <= 20 if k2 == 1 else True


# ---- both strands, all phases ------------------------------------------------------------------------------------------------

def test_a_sequence_and_its_reverse_complement_give_one_result(hg, ctx):
    rng = np.random.default_rng(21)
    for k, n in ((9, 9000), (25, 9001), (32, 4102)):
        s = dna(rng, n, lower=0.3)
        s[rng.integers(0, n, 9)] = ord("N")
        want = tx_ref.hash_sample(s, k, scaled=3)
        rc = arr(tx_ref.revcomp(s))
        assert same(want, tx_ref.hash_sample(rc, k, scaled=3))
        assert same(ctx.tx_hash_sample(s, k, scaled=3), want) and same(ctx.tx_hash_sample(rc, k, scaled=3), want)


# 8 codons, open in frame 0; every other frame of either strand meets a stop in them: TAA in frame 1 of CTAACT, TAG in frame 2 of
# GCTAGC; on the other strand TAG opposite CTA, TAA opposite the TTA of ATTACC (phase 1) and of GGTTAC (phase 2)
UNIT = b"CTAACTGCTAGCATTACCGGTTAC"


@pytest.mark.parametrize("pad", (1, 2))
@pytest.mark.parametrize("lead", (0, 1, 2))
def test_only_open_frame_on_the_reverse_strand(hg, ctx, pad, lead):
    k = 9  # a stop every k - 1 = 8 codons in the five other frames
    orf = UNIT * 60
    s = b"N" * lead + tx_ref.revcomp(orf) + b"N" * pad  # the reverse complement of s reads pad non-bases, then the ORF: frame 3 + pad
    fw = tx_ref.frame_windows(s, k)
    assert [len(f) for f in fw] == [len(orf) // 3 - k + 1 if f == 3 + pad else 0 for f in range(6)]
    want = aa_ref.hash_sample(tx_ref.translate(orf), k, threshold=MAX)
    assert want.size == 8 and same(want, tx_ref.hash_sample(s, k, threshold=MAX))  # (the unit repeats: 8 distinct windows)
    assert same(ctx.tx_hash_sample(s, k, threshold=MAX), want)
    # ... and with the repeats told apart: the last codon of every unit drawn from four (what that opens elsewhere, the reference says)
    rng = np.random.default_rng(10 * pad + lead)
    o = bytearray(orf)
    for u in range(0, 60):
        o[24 * u + 21:24 * u + 24] = [b"TAC", b"TAT", b"CAC", b"AAC"][rng.integers(0, 4)]
    s = b"N" * lead + tx_ref.revcomp(bytes(o)) + b"N" * pad
    want = tx_ref.hash_sample(s, k, threshold=MAX)
    assert same(ctx.tx_hash_sample(s, k, threshold=MAX), want)


# ---- threshold ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (9, 25))
def test_threshold_is_exact(hg, ctx, k):
    s = open_dna(np.random.default_rng(300 + k), 1500)
    s = np.where(np.random.default_rng(k).random(s.size) < 0.3, s | 0x20, s).astype(np.uint8)
    u = tx_ref.hash_sample(s, k, threshold=MAX)
    assert u.size >= 2 * (1500 - k + 1)
    assert same(ctx.tx_hash_sample(s, k, threshold=MAX), u)  # 2^64 - 1 keeps every window
    assert ctx.tx_hash_sample(s, k, threshold=0).size == 0
    for h in (int(u[0]), int(u[u.size // 2]), int(u[-1]), int(u[7]) | 0xFFFFFFFF, int(u[9]) & ~0xFFFFFFFF):
        for t in (h, h + 1):  # threshold = h drops the k-mer with hash h, h + 1 keeps it
            want = u[u < np.uint64(t)]
            assert same(ctx.tx_hash_sample(s, k, threshold=t, cap=u.size + 8), want), (k, hex(t))


# ---- density -------------------------------------------------------------------------------------------------------------------

def test_two_hashes_sixty_thousand_times_each(hg, ctx, orc):
    k, n = 9, 60_000
    want = np.array(sorted({orc.t1ha2_atonce(b"K" * k, 123), orc.t1ha2_atonce(b"F" * k, 123)}), np.uint64)  # AAA forward, TTT on the other strand
    seq = np.full(n, ord("a"), np.uint8)
    assert same(want, tx_ref.hash_sample(seq[:300], k, threshold=MAX))
    regrows = ctx.tx_plan_regrows()
    # scaled = 1: both windows of every start are hits, a hundred times the LDS stage
    hv, n2, nh = ctx.tx_sketch_batch([seq], hg.default_params(ksize=k, scaled=1, hv_d=HV_D))
    want_hv, want_n2, _ = ref_rows(orc, [want])
    assert nh.tolist() == [2] and (n2 == want_n2).all() and (hv == want_hv).all()
    assert same(ctx.tx_hash_sample(seq, k, threshold=MAX), want)
    assert ctx.tx_plan_regrows() == regrows  # 2 (n - 3k + 1) hits: the plan had room for all of them at the first attempt
    lo, hi = int(want[0]), int(want[1])
    assert ctx.tx_hash_sample(seq, k, threshold=hi).tolist() == [lo] and ctx.tx_hash_sample(seq, k, threshold=lo).size == 0


def test_more_distinct_hashes_than_starts_and_than_one_workgroup_sorts(hg, ctx, orc):
    k = 9
    s = np.random.default_rng(11).choice(np.frombuffer(b"ACac", np.uint8), 6000)  # no T: no stop; no A on the other strand: none there
    u = tx_ref.hash_sample(s, k, threshold=MAX)
    starts = s.size - 3 * k + 1
    assert u.size > 8192 and u.size > starts  # more than a plan for one k-mer per start has room for
    regrows = ctx.tx_plan_regrows()
    hv, n2, nh = ctx.tx_sketch_batch([s], hg.default_params(ksize=k, scaled=1, hv_d=HV_D))
    assert ctx.tx_plan_regrows() == regrows  # no hit region overflowed
    assert "bucket_sort_kernel" in ctx.last_kernel("sort")
    want_hv, want_n2, _ = ref_rows(orc, [u])
    assert nh.tolist() == [u.size] and (n2 == want_n2).all() and (hv == want_hv).all()
    got = ctx.tx_hash_sample(s, k, threshold=MAX, cap=16)  # too small a buffer first: HG_ERR_CAPACITY reports the count
    assert same(got, u)


# ---- the proteins of a genome are a subset ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """random DNA of 6 000 bases with three ORFs of 120 residues planted: forward at phase 0, forward at phase 2, reverse strand"""
    rng = np.random.default_rng(55)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    proteins = [rng.choice(letters, 120).tobytes() for _ in range(3)]
    g = dna(rng, 6000, lower=0.1)
    for at, coding in ((900, back_translate(proteins[0])), (2402, back_translate(proteins[1])),
                       (4000, tx_ref.revcomp(back_translate(proteins[2])))):
        g[at:at + 360] = arr(coding)
    return g, proteins


def test_planted_proteins_are_a_subset(hg, ctx, planted):
    g, proteins = planted
    k, scaled, seed = 7, 3, 99
    genome = ctx.tx_hash_sample(g, k, scaled, seed)
    assert same(genome, tx_ref.hash_sample(g, k, scaled, seed))
    for p in proteins:
        want = aa_ref.hash_sample(p, k, scaled, seed)
        got = ctx.aa_hash_sample(p, k, scaled, seed)
        assert want.size > 20 and same(got, want)
        assert np.isin(want, genome).all()
    assert not np.isin(aa_ref.hash_sample(proteins[0][::-1], k, scaled, seed), genome).all()  # (a protein that is not there)


# ---- nucleotides, amino acids and translation with one ksize on one ctx, the same buffers --------------------------------------

def test_dna_step_protein_translated_and_dna_again_on_one_ctx(hg, orc):
    k, scaled, n = 9, 50, 3
    dev = torch.device("cuda:0")
    genomes = [orc.synth_genome(g, 30_000)[:30_000] for g in (0, 1, 2)]
    for g in genomes:
        g[::997] = ord("N")
    stride = 30_064
    flat = np.full(n * stride + 64, ord("A"), np.uint8)  # (bases between the genomes: a read past an end would be hashed)
    offs, lens = [i * stride for i in range(n)], [30_000] * n
    for o, g in zip(offs, genomes):
        flat[o:o + g.size] = g
    d_seq = torch.from_numpy(flat).to(dev)
    sets = {"aa": [aa_ref.hash_sample(g, k, scaled) for g in genomes], "tx": [tx_ref.hash_sample(g, k, scaled) for g in genomes]}
    assert all(a.size and t.size and not same(a, t) for a, t in zip(sets["aa"], sets["tx"]))

    def outs():
        return (torch.full((n, HV_D), -1, dtype=torch.int16, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev),
                torch.full((n,), -1, dtype=torch.int32, device=dev))

    def check(o, rows):
        want_hv, want_n2, want_nh = rows
        assert (o[2].cpu().numpy().view(np.uint32) == want_nh).all()
        assert (o[1].cpu().numpy() == want_n2).all() and (o[0].cpu().numpy() == want_hv).all()

    for layout in (hg.LAYOUT_AVX2, hg.LAYOUT_SCALAR):
        p = hg.default_params(ksize=k, scaled=scaled, hv_d=HV_D, hv_layout=layout)
        dna_rows = [orc.sketch_genome(g, ksize=k, scaled=scaled, hv_d=HV_D, layout=layout) for g in genomes]
        dna_rows = (np.stack([r[0] for r in dna_rows]), np.array([r[1] for r in dna_rows], np.int32), np.array([r[2] for r in dna_rows], np.uint32))
        with hg.Context(0) as c:
            o_dna, o_aa, o_tx, o_dna2, o_tx2 = outs(), outs(), outs(), outs(), outs()
            ptrs = lambda o: [t.data_ptr() for t in o]
            c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, *ptrs(o_dna))
            assert c.sketch_step_counts()[0] == 1, "the nucleotide step was not deferred"
            c.aa_sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, *ptrs(o_aa))
            assert c.last_kernel("kmer") == hg.aa_kernel_name(k)
            c.tx_sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, *ptrs(o_tx))
            assert c.last_kernel("kmer") == hg.tx_kernel_name(k) == "tx_kmer_sample_kernel<2>"
            c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, *ptrs(o_dna2))
            c.sync()
            assert c.last_kernel("kmer").startswith("kmer_sample_shared<9")
            c.tx_sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, *ptrs(o_tx2))  # translated behind nucleotides, protein behind translated
            c.aa_sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, *ptrs(o_aa))
            c.sync()
            assert c.sketch_step_counts()[0] == 2  # the two nucleotide calls; the companions never take the deferred step
            # host-fed, same ctx
            hv, n2, nh = c.tx_sketch_batch(genomes, p)
            hv_a, n2_a, nh_a = c.aa_sketch_batch(genomes, p)
        check(o_dna, dna_rows), check(o_dna2, dna_rows)
        tx_rows, aa_rows = ref_rows(orc, sets["tx"], HV_D, layout), ref_rows(orc, sets["aa"], HV_D, layout)
        check(o_tx, tx_rows), check(o_tx2, tx_rows), check(o_aa, aa_rows)
        assert (nh == tx_rows[2]).all() and (n2 == tx_rows[1]).all() and (hv == tx_rows[0]).all()
        assert (nh_a == aa_rows[2]).all() and (n2_a == aa_rows[1]).all() and (hv_a == aa_rows[0]).all()


def test_dense_protein_then_translated_plans_are_told_apart(hg, orc):
    """The plan-cache trap where it shows: one ctx, one buffer, one ksize, scaled = 1.  The protein plan has a slot per start,
    the translated call fills two: taken for each other, the translated call would overflow its regions and regrow them."""
    k = 9
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(12)
    seqs = [rng.choice(np.frombuffer(b"ACac", np.uint8), n) for n in (6000, 5000, 6000)]  # open in every frame; A and C are residues too
    offs, lens = [0, 6080, 11136], [s.size for s in seqs]
    flat = np.zeros(17_300, np.uint8)
    for o, s in zip(offs, seqs):
        flat[o:o + s.size] = s
    d_seq = torch.from_numpy(flat).to(dev)
    tx_sets = [tx_ref.hash_sample(s, k, threshold=MAX) for s in seqs]
    aa_sets = [aa_ref.hash_sample(s, k, threshold=MAX) for s in seqs]
    assert all(t.size > n - 3 * k + 1 for t, n in zip(tx_sets, lens))  # more hits than the protein plan's regions hold
    assert hg.tx_plan_describe(lens, k, 1, offs)["min_cap"] >= 2 * (5000 - 26)
    p = hg.default_params(ksize=k, scaled=1, hv_d=HV_D)
    n = len(seqs)
    with hg.Context(0) as c:
        for name, sets in (("aa", aa_sets), ("tx", tx_sets), ("aa", aa_sets), ("tx", tx_sets)):
            o = (torch.full((n, HV_D), -1, dtype=torch.int16, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev),
                 torch.full((n,), -1, dtype=torch.int32, device=dev))
            getattr(c, name + "_sketch_batch_dev")(d_seq.data_ptr(), offs, lens, p, *(t.data_ptr() for t in o))
            c.sync()
            want_hv, want_n2, want_nh = ref_rows(orc, sets)
            assert (o[2].cpu().numpy().view(np.uint32) == want_nh).all(), name
            assert (o[1].cpu().numpy() == want_n2).all() and (o[0].cpu().numpy() == want_hv).all(), name
            assert c.tx_plan_regrows() == 0, name


# ---- the shape the command line runs at: Mbp genomes, thousands of workgroups ------------------------------------------------------

def test_a_batch_of_mbp_genomes_on_the_device(hg, ctx, orc):
    k, scaled, L, copies = 9, 1500, 1_000_000, 32
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(99)
    two = [dna(rng, L), dna(rng, L - 1)]
    sets = [tx_ref.hash_sample(g, k, scaled) for g in two]
    assert all(550 < s.size < 1200 for s in sets)  # 2 (L - 26) (61 / 64)^9 / 1500 = 865 expected
    n = 2 * copies
    stride = (L + 32 + 63) // 64 * 64
    flat = torch.zeros(n * stride + 64, dtype=torch.uint8, device=dev)
    view = flat[: n * stride].view(n, stride)
    for i, g in enumerate(two):
        view[i::2, : g.size] = torch.from_numpy(g).to(dev)
    torch.cuda.synchronize()
    assert hg.tx_plan_describe([L] * n, k, scaled)["items"] > 2000  # several workgroups per CU at once
    d_hv = torch.full((n, HV_D), -1, dtype=torch.int16, device=dev)
    d_n2 = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_nh = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p = hg.default_params(ksize=k, scaled=scaled, hv_d=HV_D)
    ctx.tx_sketch_batch_dev(flat.data_ptr(), [i * stride for i in range(n)], [two[i % 2].size for i in range(n)], p,
                            d_hv.data_ptr(), d_n2.data_ptr(), d_nh.data_ptr())
    ctx.sync()
    want_hv, want_n2, want_nh = ref_rows(orc, sets)
    assert (d_nh.cpu().numpy().view(np.uint32) == np.tile(want_nh, copies)).all()
    assert (d_n2.cpu().numpy() == np.tile(want_n2, copies)).all() and (d_hv.cpu().numpy() == np.tile(want_hv, (copies, 1))).all()
    assert same(ctx.tx_hash_sample(two[0], k, scaled), sets[0])


# ---- command line ----------------------------------------------------------------------------------------------------------------

def fasta_text(records, width=70, tag=b"contig"):
    out = []
    for i, r in enumerate(records):
        out.append(b">%s_%d some description" % (tag, i))
        out += [bytes(r[j:j + width]) for j in range(0, len(r), width)]
    return b"\n".join(out) + b"\n"


def test_cli_sketch_translate_then_dist_and_containment(hg, orc, planted, tmp_path):
    g, proteins = planted
    rng = np.random.default_rng(78)
    a = [g[:3000], g[3000:]]  # two records, cut between the ORFs: the reader puts one N between them
    b = [x.copy() for x in a]
    for r in b:  # the same genome, one base in 50 substituted
        at = rng.random(r.size) < 0.02
        r[at] = rng.choice(BASES, int(at.sum()))
    c = [dna(rng, 3000), dna(rng, 2000), dna(rng, 10)]  # unrelated
    d = tmp_path / "fna"
    d.mkdir()
    texts = {"a.fna": fasta_text(a), "b.fna": fasta_text(b), "c.fna": fasta_text(c)}
    (d / "a.fna").write_bytes(texts["a.fna"])
    (d / "b.fna").write_bytes(gzip.compress(texts["b.fna"]))  # gzip content
    (d / "c.fna").write_bytes(texts["c.fna"])
    (d / "ignored.faa").write_bytes(b">x\nMKVLAAGIWRTYPLDE\n")
    out, tsv = str(tmp_path / "t.sketch"), str(tmp_path / "t.tsv")
    r = subprocess.run([hg.CLI_PATH, "sketch", "--translate", "-p", str(d), "-o", out, "-s", "5", "-t", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Sketching 3 files took" in r.stdout
    recs = hg.read_sketch_file(out)
    names = [str(d / f) for f in ("a.fna", "b.fna", "c.fna")]
    assert [x["file_str"] for x in recs] == names
    merged = [orc.read_merge_seq(texts[f]) for f in ("a.fna", "b.fna", "c.fna")]  # one N per record start
    assert merged[0].size == g.size + 2 and bytes(merged[0][:1]) == b"N"
    sets = [tx_ref.hash_sample(m, 9, 5) for m in merged]  # -k defaults to 9
    assert np.intersect1d(sets[0], sets[1]).size > 0 and np.intersect1d(sets[0], sets[2]).size == 0
    hvs, n2s, _ = ref_rows(orc, sets, 4096)
    for x, hv, n2 in zip(recs, hvs, n2s):
        assert (x["ksize"], x["canonical"], x["scaled"], x["seed"], x["hv_d"]) == (9, 0, 5, 123, 4096)
        assert x["hv_norm_2"] == n2 and (hg.hv_unpack(x["hv"].view(np.uint8), 4096, x["hv_quant_bits"]) == hv).all()
    out2 = str(tmp_path / "t2.sketch")  # (dist on ONE file writes each pair i < j once: a copy as the query gives all nine)
    shutil.copy(out, out2)
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", out, "-q", out2, "-o", tsv, "-a", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {(x, y): v for x, y, v in (l.split("\t") for l in open(tsv).read().splitlines())}
    assert len(got) == 9
    for i in range(3):
        for j in range(3):
            assert got[(names[i], names[j])] == "%.3f" % aa_ref.aai(hvs[i], hvs[j], 9), (i, j)
        assert got[(names[i], names[i])] == "100.000"  # a file with itself
    # (c shares no 9-mer with a or b; what its lines print is the estimate's noise at |set| ~ 1 500 and D = 4 096, far below a : b)
    assert max(float(got[(names[0], names[2])]), float(got[(names[1], names[2])])) + 10.0 < float(got[(names[0], names[1])]) < 100.0
    # the planted proteins, sketched as proteins, are contained in the translated sketch of their genome and not in c's
    f = tmp_path / "faa"
    f.mkdir()
    (f / "p.faa").write_bytes(fasta_text(proteins, 60, b"protein"))
    pout, ctsv = str(tmp_path / "p.sketch"), str(tmp_path / "c.tsv")
    r = subprocess.run([hg.CLI_PATH, "sketch", "--alphabet", "protein", "-p", str(f), "-o", pout, "-s", "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pset = aa_ref.hash_sample(aa_ref.parse_fasta(fasta_text(proteins, 60, b"protein")), 9, 5)
    assert pset.size > 40 and np.isin(pset, sets[0]).all() and not np.isin(pset, sets[2]).any()
    phv, pn2, _ = ref_rows(orc, [pset], 4096)
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", out, "-q", pout, "-o", ctsv, "-a", "0", "--ani_metric", "containment"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {(x, y): v for x, y, v in (l.split("\t") for l in open(ctsv).read().splitlines())}
    want = cr.ani_ref(orc, cr.exact_dots(hvs, phv), n2s[:, None], pn2[None, :], 9, cr.CONTAINMENT)  # x = dot / |query|: the proteins
    pname = str(f / "p.faa")
    assert got == {(names[i], pname): "%.3f" % float(want[i, 0]) for i in range(3)}
    assert float(got[(names[0], pname)]) > 95.0 and float(got[(names[2], pname)]) + 10.0 < float(got[(names[0], pname)])


# ---- rejected inputs -------------------------------------------------------------------------------------------------------------

def test_rejected_before_anything_is_launched(hg):
    s = dna(np.random.default_rng(1), 1500)
    with hg.Context(0) as c:
        for kw, status in (({"ksize": 33}, hg.ERR_UNSUPPORTED), ({"min_count": 2}, hg.ERR_UNSUPPORTED), ({"norm_mode": 1}, hg.ERR_INVALID),
                           ({"ksize": 0}, hg.ERR_INVALID), ({"scaled": 0}, hg.ERR_INVALID)):
            p = hg.default_params(**dict({"ksize": 9, "hv_d": HV_D}, **kw))
            with pytest.raises(hg.HgError) as e:
                c.tx_sketch_batch([s], p)
            assert e.value.status == status, kw
            dev = torch.device("cuda:0")
            buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
            with pytest.raises(hg.HgError) as e:
                c.tx_sketch_batch_dev(buf.data_ptr(), [0], [1500], p, buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
            assert e.value.status == status, kw
        with pytest.raises(hg.HgError) as e:
            c.tx_hash_sample(s, 33)
        assert e.value.status == hg.ERR_UNSUPPORTED
        with pytest.raises(hg.HgError) as e:
            c.tx_hash_sample(s, 0)
        assert e.value.status == hg.ERR_INVALID
        assert c.tx_hash_sample(s[:26], 9, threshold=MAX).size == 0  # shorter than 3k: nothing, and nothing launched
        assert c.last_kernel("kmer") == "" and c.sketch_step_counts() == (0, 0, 0)
        p = hg.default_params(ksize=9, min_count=1, canonical=1, hv_d=HV_D)  # min_count = 1 is every sampled k-mer; canonical is ignored
        assert c.tx_sketch_batch([s], p)[2][0] == tx_ref.hash_sample(s, 9).size
