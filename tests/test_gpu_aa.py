"""Amino-acid k-mer sketches (libhypergen_aa.so, include/hypergen_aa.h) on the GPU, all comparisons `==` against tests/aa_ref.py:
every t1ha2 tail-word boundary of k at the lengths where the kernel's tile, the plan's work item or the sequence end decide;
the classification of all 256 byte values; the threshold at a hash and one above it; hit densities that overflow the LDS
stage and the hit region and sets beyond the one-workgroup sort; a batch through both entry points and both layouts; a
deferred nucleotide step followed by an amino-acid call on one ctx; the command line end to end; what is rejected."""
import gzip
import shutil
import subprocess

import numpy as np
import pytest
import torch

import aa_census
import aa_ref

pytestmark = pytest.mark.gpu

KS = (1, 7, 8, 9, 16, 17, 24, 25, 31, 32)  # both ends of every kernel instantiation's range: the tail word is 1 byte / a whole word
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
MAX = 2**64 - 1
HV_D = 1024


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_aa()
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    with hg.Context(0) as c:
        yield c


def residues(rng, n, lower=0.0):
    s = rng.choice(LETTERS, n)
    if lower:
        s = np.where(rng.random(n) < lower, s | 0x20, s).astype(np.uint8)
    return s


def ref_rows(orc, sets, hv_d=HV_D, layout=1):
    hv = np.stack([orc.encode_hv(u, hv_d, layout) for u in sets]) if sets else np.zeros((0, hv_d), np.int16)
    return hv, np.array([orc.hv_norm2(r) for r in hv], np.int32), np.array([u.size for u in sets], np.uint32)


# ---- k and lengths -----------------------------------------------------------------------------------------------------------

def edge_lengths(hg, k):
    T, I = hg.aa_tile_starts(), hg.aa_item_starts(k)
    return sorted({0, k - 1, k, k + 1,
                   T - 1, T, T + 1, T + k - 2, T + k - 1, T + k,          # tile size +- 1 as a length and as a number of starts
                   I - 1, I, I + 1, I + k - 2, I + k - 1, I + k,          # item size +- 1 and + k - 1
                   2 * I + 1, 2 * I + k})                                   # two items + 1


@pytest.mark.parametrize("k", KS)
def test_every_tail_boundary_at_every_edge_length(hg, ctx, orc, k):
    rng = np.random.default_rng(100 + k)
    lens = edge_lengths(hg, k)
    base = residues(rng, lens[-1], lower=0.2)
    for at in rng.integers(0, base.size, 12):  # a few non-residues, some of them next to a tile or item edge
        base[at] = ord("X")
    base[hg.aa_item_starts(k) - 1] = ord("*")
    scaled = 40
    wh = aa_ref.window_hashes(base, k)
    starts = np.array([s for s, _ in wh], np.int64)
    hashes = np.array([h for _, h in wh], np.uint64)
    keep = hashes < np.uint64(MAX // scaled)
    sets = [np.unique(hashes[keep & (starts <= L - k)]) for L in lens]  # a prefix's windows are the base's that end inside it
    want_hv, want_n2, want_nh = ref_rows(orc, sets)
    p = hg.default_params(ksize=k, scaled=scaled, hv_d=HV_D)
    hv, n2, nh = ctx.aa_sketch_batch([base[:L] for L in lens], p)
    assert ctx.last_kernel("kmer") == hg.aa_kernel_name(k) and ctx.last_kernel("kmer") in [r.name for r in aa_census.ROWS if k in r.ksizes]
    assert nh.tolist() == want_nh.tolist(), (k, lens)
    assert (n2 == want_n2).all() and (hv == want_hv).all()
    T, I = hg.aa_tile_starts(), hg.aa_item_starts(k)
    for L in (k - 1, k, k + 1, T + k, I + k, 2 * I + k):  # the hash lists themselves: around k, a tile / an item / two items + 1 start
        got, want = ctx.aa_hash_sample(base[:L], k, scaled), sets[lens.index(L)]
        assert got.size == want.size and (got == want).all(), (k, L)


# ---- byte classification -----------------------------------------------------------------------------------------------------

def test_all_256_byte_values_case_stop_and_window_positions(hg, ctx):
    k = 9
    rng = np.random.default_rng(7)
    T = hg.aa_tile_starts()
    parts = []
    for v in range(256):  # every byte value between two runs of residues
        parts += [residues(rng, 2 * k + v % 3), np.array([v], np.uint8)]
    for case in (0.0, 1.0, 0.5):  # upper, lower, mixed: the same k-mers three times
        run = residues(np.random.default_rng(8), 40)
        parts += [np.where(rng.random(40) < case, run | 0x20, run).astype(np.uint8), np.frombuffer(b"*", np.uint8)]
    parts += [np.frombuffer(b"NNNNNNNNNNNNANNNNNNNNN*", np.uint8)]  # N is a residue here
    for j in range(k):  # a non-residue at each position of a window: k - 1 residues on either side, no window is whole
        parts += [residues(rng, k - 1), np.frombuffer(b"X", np.uint8), residues(rng, k - 1), np.frombuffer(b"-", np.uint8)]
    seq = np.concatenate(parts + [residues(rng, 3 * T)])
    # a non-residue as first and last start of a tile, and as first and last byte of what a tile stages (T + 64 bytes)
    for at in (T - 1, T, 2 * T - 1, 2 * T, T + 63, T + 64, 2 * T + 63, 3 * T - 1, 3 * T):
        seq[at] = ord("B")
    seq[0] = ord("*")
    want = aa_ref.hash_sample(seq, k, threshold=MAX)  # every window is kept: a window hashed that should not be shows
    got = ctx.aa_hash_sample(seq, k, threshold=MAX, cap=want.size + 64)
    assert got.size == want.size and (got == want).all()
    assert want.size > 8192 and "bucket_sort_kernel" in ctx.last_kernel("sort")
    # the three case variants yield one set of hashes
    run = residues(np.random.default_rng(8), 40)
    one = aa_ref.hash_sample(run, k, threshold=MAX)
    for s in (run, run | 0x20, np.where(np.arange(40) % 2 == 0, run | 0x20, run).astype(np.uint8)):
        got = ctx.aa_hash_sample(s, k, threshold=MAX)
        assert got.size == 40 - k + 1 == one.size and (got == one).all()
    for k2 in (1, 32):  # every byte value alone: k = 1 keeps the twenty letters' hashes, k = 32 windows need 32 of them in a row
        allb = np.concatenate([np.arange(256, dtype=np.uint8), residues(rng, 31), np.arange(256, dtype=np.uint8)[::-1]])
        want = aa_ref.hash_sample(allb, k2, threshold=MAX)
        got = ctx.aa_hash_sample(allb, k2, threshold=MAX)
        assert (want.size == 20 if k2 == 1 else want.size == 0) and got.size == want.size and (got == want).all()


# ---- threshold ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (9, 25))
def test_threshold_is_exact(hg, ctx, k):
    s = residues(np.random.default_rng(300 + k), 5000, lower=0.3)
    u = aa_ref.hash_sample(s, k, threshold=MAX)
    assert u.size == 5000 - k + 1
    got = ctx.aa_hash_sample(s, k, threshold=MAX)  # 2^64 - 1 keeps every window
    assert got.size == u.size and (got == u).all()
    assert ctx.aa_hash_sample(s, k, threshold=0).size == 0
    for h in (int(u[0]), int(u[u.size // 2]), int(u[-1]), int(u[7]) | 0xFFFFFFFF, int(u[9]) & ~0xFFFFFFFF):
        for t in (h, h + 1):  # threshold = h drops the k-mer with hash h, h + 1 keeps it
            want = u[u < np.uint64(t)]
            got = ctx.aa_hash_sample(s, k, threshold=t, cap=u.size + 8)
            assert got.size == want.size and (got == want).all(), (k, hex(t))


# ---- adversarial density -----------------------------------------------------------------------------------------------------

def test_one_hash_forty_thousand_times(hg, ctx, orc):
    k, n = 9, 40_000
    by_letter = {c: orc.t1ha2_atonce(bytes([c]) * k, 123) for c in LETTERS.tolist()}
    c = min(by_letter, key=by_letter.get)
    h = by_letter[c]
    seq = np.full(n, c | 0x20, np.uint8)  # lower case
    # scaled = 1: every window is a hit, thousands of times the LDS stage
    p = hg.default_params(ksize=k, scaled=1, hv_d=HV_D)
    hv, n2, nh = ctx.aa_sketch_batch([seq], p)
    want_hv, want_n2, want_nh = ref_rows(orc, [np.array([h], np.uint64)])
    assert nh.tolist() == [1] and (n2 == want_n2).all() and (hv == want_hv).all()
    got = ctx.aa_hash_sample(seq, k, scaled=1)
    assert got.tolist() == [h]
    # the largest scaled that still keeps the hash: the plan expects n / scaled hits and gets n -- the hit region overflows and is regrown
    scaled = MAX // (h + 1)
    while not h < MAX // scaled:
        scaled -= 1
    assert scaled >= 4 and (n - k + 1) // scaled * 2 + 1024 < n - k + 1, "the letter's hash leaves no room for an overflow"
    p = hg.default_params(ksize=k, scaled=scaled, hv_d=HV_D)
    other = residues(np.random.default_rng(5), 3000)
    hv, n2, nh = ctx.aa_sketch_batch([other, seq, other[::-1].copy()], p)
    sets = [aa_ref.hash_sample(other, k, scaled), np.array([h], np.uint64), aa_ref.hash_sample(other[::-1].copy(), k, scaled)]
    want_hv, want_n2, want_nh = ref_rows(orc, sets)
    assert nh.tolist() == want_nh.tolist() and (n2 == want_n2).all() and (hv == want_hv).all()
    assert ctx.aa_hash_sample(seq, k, threshold=h + 1).tolist() == [h] and ctx.aa_hash_sample(seq, k, threshold=h).size == 0


def test_more_distinct_hashes_than_one_workgroup_sorts(hg, ctx, orc):
    k = 9
    s = residues(np.random.default_rng(11), 12_000)
    u = aa_ref.hash_sample(s, k, scaled=1)
    assert u.size > 8192
    hv, n2, nh = ctx.aa_sketch_batch([s], hg.default_params(ksize=k, scaled=1, hv_d=HV_D))
    assert "bucket_sort_kernel" in ctx.last_kernel("sort")
    want_hv, want_n2, want_nh = ref_rows(orc, [u])
    assert nh.tolist() == [u.size] and (n2 == want_n2).all() and (hv == want_hv).all()
    got = ctx.aa_hash_sample(s, k, scaled=1, cap=16)  # too small a buffer first: HG_ERR_CAPACITY reports the count
    assert got.size == u.size and (got == u).all()


# ---- batch ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch(orc):
    """300 proteomes of 0..3 000 residues and one of 200 000, records separated by '*', some lower case; k = 9, scaled = 100"""
    rng = np.random.default_rng(2024)
    k, scaled = 9, 100
    seqs = []
    for n in list(rng.integers(0, 3001, 300)) + [200_000]:
        s = residues(rng, int(n), lower=0.1)
        if n:
            s[rng.integers(0, n, max(1, int(n) // 300))] = ord("*")
        seqs.append(s)
    seqs[3], seqs[4], seqs[5] = seqs[3][:0], seqs[4][:k - 1], seqs[5][:k]
    sets = [aa_ref.hash_sample(s, k, scaled) for s in seqs]
    rows = {layout: ref_rows(orc, sets, HV_D, layout) for layout in (0, 1)}
    return k, scaled, seqs, rows


def test_batch_on_the_device_both_layouts(hg, ctx, batch):
    k, scaled, seqs, rows = batch
    dev = torch.device("cuda:0")
    offs, total = [], 0
    for s in seqs:
        offs.append(total)
        total += (s.size + 32 + 3) & ~3
    flat = np.full(total + 64, ord("A"), np.uint8)  # (residues between the proteomes: a read past an end would be hashed)
    for o, s in zip(offs, seqs):
        flat[o:o + s.size] = s
    d_seq = torch.from_numpy(flat).to(dev)
    n = len(seqs)
    for layout in (hg.LAYOUT_AVX2, hg.LAYOUT_SCALAR):
        d_hv = torch.full((n, HV_D), -1, dtype=torch.int16, device=dev)
        d_n2 = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_nh = torch.full((n,), -1, dtype=torch.int32, device=dev)
        p = hg.default_params(ksize=k, scaled=scaled, hv_d=HV_D, hv_layout=layout, canonical=1)  # (canonical is ignored)
        ctx.aa_sketch_batch_dev(d_seq.data_ptr(), offs, [s.size for s in seqs], p, d_hv.data_ptr(), d_n2.data_ptr(), d_nh.data_ptr())
        ctx.sync()
        assert ctx.last_kernel("kmer") == hg.aa_kernel_name(k) == "aa_kmer_sample_kernel<2>"
        want_hv, want_n2, want_nh = rows[layout]
        assert (d_nh.cpu().numpy().view(np.uint32) == want_nh).all()
        assert (d_n2.cpu().numpy() == want_n2).all() and (d_hv.cpu().numpy() == want_hv).all()
    assert ctx.sketch_step_counts()[0] == 0  # never the deferred step


def test_batch_from_the_host(hg, ctx, batch):
    k, scaled, seqs, rows = batch
    hv, n2, nh = ctx.aa_sketch_batch(seqs, hg.default_params(ksize=k, scaled=scaled, hv_d=HV_D))
    want_hv, want_n2, want_nh = rows[hg.LAYOUT_AVX2]
    assert (nh == want_nh).all() and (n2 == want_n2).all() and (hv == want_hv).all()
    assert ctx.last_kernel("kmer") == hg.aa_kernel_name(k)
    hv0, n20, nh0 = ctx.aa_sketch_batch([], hg.default_params(ksize=k))
    assert hv0.shape == (0, 4096) and nh0.size == 0


# ---- a deferred nucleotide step, then amino acids, on one ctx ------------------------------------------------------------------

def test_dna_step_then_amino_acids_on_one_ctx(hg, orc, batch):
    k, scaled, seqs, rows = batch
    dev = torch.device("cuda:0")
    genomes = [orc.synth_genome(g, 60_000)[:60_000] for g in (0, 1, 2)]
    dna = np.zeros(3 * 60_064 + 64, np.uint8)
    for i, g in enumerate(genomes):
        dna[i * 60_064:i * 60_064 + 60_000] = g
    prot = seqs[:40]
    offs, total = [], 0
    for s in prot:
        offs.append(total)
        total += (s.size + 32 + 3) & ~3
    flat = np.zeros(total + 64, np.uint8)
    for o, s in zip(offs, prot):
        flat[o:o + s.size] = s
    d_dna, d_prot = torch.from_numpy(dna).to(dev), torch.from_numpy(flat).to(dev)
    outs = [(torch.zeros((m, HV_D), dtype=torch.int16, device=dev), torch.zeros(m, dtype=torch.int32, device=dev),
             torch.zeros(m, dtype=torch.int32, device=dev)) for m in (3, len(prot))]
    with hg.Context(0) as c:
        pd = hg.default_params(scaled=200, hv_d=HV_D)
        c.sketch_batch_dev(d_dna.data_ptr(), [0, 60_064, 120_128], [60_000] * 3, pd, *(t.data_ptr() for t in outs[0]))
        assert c.sketch_step_counts()[0] == 1, "the nucleotide step was not deferred"
        pa = hg.default_params(ksize=k, scaled=scaled, hv_d=HV_D)
        c.aa_sketch_batch_dev(d_prot.data_ptr(), offs, [s.size for s in prot], pa, *(t.data_ptr() for t in outs[1]))
        assert c.last_kernel("kmer") == hg.aa_kernel_name(k)
        c.sync()
        # ... and a nucleotide call behind it runs the nucleotide kernel again
        c.sketch_batch_dev(d_dna.data_ptr(), [0, 60_064, 120_128], [60_000] * 3, pd, *(t.data_ptr() for t in outs[0]))
        c.sync()
        assert c.last_kernel("kmer").startswith("kmer_sample_shared<21")
    for i, g in enumerate(genomes):
        w_hv, w_n2, w_nh = orc.sketch_genome(g, scaled=200, hv_d=HV_D)
        assert int(outs[0][2][i]) == w_nh and int(outs[0][1][i]) == w_n2 and (outs[0][0][i].cpu().numpy() == w_hv).all()
    want_hv, want_n2, want_nh = rows[hg.LAYOUT_AVX2]
    m = len(prot)
    assert (outs[1][2].cpu().numpy().view(np.uint32) == want_nh[:m]).all()
    assert (outs[1][1].cpu().numpy() == want_n2[:m]).all() and (outs[1][0].cpu().numpy() == want_hv[:m]).all()


# ---- command line ----------------------------------------------------------------------------------------------------------------

def fasta_text(records, width=60):
    out = []
    for i, r in enumerate(records):
        out.append(b">protein_%d some description" % i)
        out += [bytes(r[j:j + width]) for j in range(0, len(r), width)]
    return b"\n".join(out) + b"\n"


def test_cli_sketch_protein_then_dist(hg, orc, tmp_path):
    rng = np.random.default_rng(77)
    a = [residues(rng, int(n)) for n in rng.integers(150, 600, 12)]
    b = [r.copy() for r in a]
    for r in b:  # the same proteins, one residue in 25 substituted
        at = rng.random(r.size) < 0.04
        r[at] = rng.choice(LETTERS, int(at.sum()))
    c = [residues(rng, int(n)) for n in rng.integers(150, 600, 12)]  # unrelated: no 9-mer in common
    d = tmp_path / "faa"
    d.mkdir()
    (d / "a.faa").write_bytes(fasta_text(a))
    (d / "b.faa").write_bytes(gzip.compress(fasta_text(b).lower()))  # gzip content, lower case
    (d / "c.faa").write_bytes(fasta_text(c).replace(b"\n", b"\r\n"))
    (d / "ignored.fna").write_bytes(b">x\nACGTACGTACGTACGTACGTACGTACGT\n")
    out, tsv = str(tmp_path / "p.sketch"), str(tmp_path / "p.tsv")
    r = subprocess.run([hg.CLI_PATH, "sketch", "--alphabet", "protein", "-p", str(d), "-o", out, "-s", "5", "-t", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Sketching 3 files took" in r.stdout
    recs = hg.read_sketch_file(out)
    names = [str(d / f) for f in ("a.faa", "b.faa", "c.faa")]
    assert [x["file_str"] for x in recs] == names
    sets = [aa_ref.hash_sample(aa_ref.parse_fasta(fasta_text(p)), 9, 5) for p in (a, b, c)]  # -k defaults to 9
    assert np.intersect1d(sets[0], sets[1]).size > 0 and np.intersect1d(sets[0], sets[2]).size == 0
    hvs, n2s, _ = ref_rows(orc, sets, 4096)
    for x, hv, n2 in zip(recs, hvs, n2s):
        assert (x["ksize"], x["canonical"], x["scaled"], x["seed"], x["hv_d"]) == (9, 0, 5, 123, 4096)
        assert x["hv_norm_2"] == n2 and (hg.hv_unpack(x["hv"].view(np.uint8), 4096, x["hv_quant_bits"]) == hv).all()
    out2 = str(tmp_path / "p2.sketch")  # (dist on ONE file writes each pair i < j once: a copy as the query gives all nine)
    shutil.copy(out, out2)
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", out, "-q", out2, "-o", tsv, "-a", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {(x, y): v for x, y, v in (l.split("\t") for l in open(tsv).read().splitlines())}
    assert len(got) == 9
    for i in range(3):
        for j in range(3):
            assert got[(names[i], names[j])] == "%.3f" % aa_ref.aai(hvs[i], hvs[j], 9), (i, j)
        assert got[(names[i], names[i])] == "100.000"  # a file with itself
    assert got[(names[0], names[2])] == got[(names[1], names[2])] == "0.000"  # no shared 9-mer
    assert 90.0 < float(got[(names[0], names[1])]) < 100.0


# ---- rejected inputs -------------------------------------------------------------------------------------------------------------

def test_rejected_before_anything_is_launched(hg):
    s = residues(np.random.default_rng(1), 500)
    with hg.Context(0) as c:
        for kw, status in (({"ksize": 33}, hg.ERR_UNSUPPORTED), ({"min_count": 2}, hg.ERR_UNSUPPORTED), ({"norm_mode": 1}, hg.ERR_INVALID),
                           ({"ksize": 0}, hg.ERR_INVALID), ({"scaled": 0}, hg.ERR_INVALID)):
            p = hg.default_params(**dict({"ksize": 9, "hv_d": HV_D}, **kw))
            with pytest.raises(hg.HgError) as e:
                c.aa_sketch_batch([s], p)
            assert e.value.status == status, kw
            dev = torch.device("cuda:0")
            buf = torch.zeros(2048, dtype=torch.uint8, device=dev)
            with pytest.raises(hg.HgError) as e:
                c.aa_sketch_batch_dev(buf.data_ptr(), [0], [500], p, buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
            assert e.value.status == status, kw
        with pytest.raises(hg.HgError) as e:
            c.aa_hash_sample(s, 33)
        assert e.value.status == hg.ERR_UNSUPPORTED
        assert c.last_kernel("kmer") == "" and c.sketch_step_counts() == (0, 0, 0)
        p = hg.default_params(ksize=9, min_count=1, hv_d=HV_D)  # min_count = 1 is every sampled k-mer, as 0 is
        assert c.aa_sketch_batch([s], p)[2][0] == aa_ref.hash_sample(s, 9).size
