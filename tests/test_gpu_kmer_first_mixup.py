"""kmer_sample_shared, k = 17..32: the first t1ha2 mixup runs a text that relies on bounded operands (hg_kmer_asm.h,
HG_KS_MUL128_BOUNDED: staged bytes are ACGT, and the wave-uniform operand -- the seed for k <= 24, K for k >= 25 -- is
small); for k <= 24 a seed of 2^28 or more takes the general text instead.  Everything here is exact equality with the CPU
oracle.  With threshold = 2^64 - 1 every k-mer's hash is kept, so whole hash sets are compared.

Inputs are two tiles of one work item (7 000 bases): random ACGT, all T (the largest operands on the forward strand), all A
(the largest on the reverse strand: its reverse complement is all T), and a sequence with lower-case letters, Ns and a U
(the tile is "dirty": the second copy of the k-mer loop).  Seeds lie on both sides of 2^28, and some make s + w0 wrap 64 bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
N_BASES = 7000
ALL = 2**64 - 1
SEEDS = (0, 123, 2**28 - 1, 2**28, 2**32 + 5, 2**63 + 11, 2**64 - 1)
KS = (17, 21, 24, 25, 28, 32)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def ctxs(hg):
    """one ctx per input form of hg_kmer_hash_sample: <K, CANON, false> and <K, CANON, true>"""
    out = {}
    for form in ("ascii", "packed"):
        c = hg.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.set_debug("hostfed", form)
        out[form] = c
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(1117)
    rnd = rng.choice(ACGT, N_BASES).astype(np.uint8)
    mixed = rng.choice(ACGT, N_BASES).astype(np.uint8)
    mixed[100:160] |= 0x20                      # a lower-case run: still bases
    mixed[3040:3060] |= 0x20                    # ... across the tile boundary
    for at in (7, 500, 501, 3050, 6990):
        mixed[at] = ord("N")
    mixed[1234] = ord("U")
    mixed[4321] = ord("u")
    return {"random": rnd, "all_T": np.full(N_BASES, ord("T"), np.uint8), "all_A": np.full(N_BASES, ord("A"), np.uint8),
            "mixed": mixed}


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", KS)
def test_whole_hash_set(ctxs, orc, inputs, k, canonical):
    for name, s in inputs.items():
        for norm in ((0, 1) if name == "mixed" else (0,)):  # u/U: a non-base, or a T under HG_NORM_U2T
            for seed in SEEDS:
                want = orc.kmer_hash_sample(s, k, 1, seed, canonical, norm, threshold=ALL)
                assert want.size > 0
                for form, c in ctxs.items():
                    got = c.kmer_hash_sample(s, k, 1, seed, canonical, norm, threshold=ALL, cap=N_BASES + 64)
                    assert c.last_kernel("kmer") == "kmer_sample_shared<%d, %s, %s>" % (
                        k, "true" if canonical else "false", "true" if form == "packed" else "false")
                    assert got.size == want.size and (got == want).all(), (name, norm, hex(seed), form, got.size, want.size)


def upload(seqs, align=16):
    offs, total = [], 0
    for s in seqs:
        offs.append(total)
        total += (len(s) + align - 1) // align * align
    host = np.zeros(total + 64, np.uint8)
    for o, s in zip(offs, seqs):
        host[o:o + len(s)] = s
    return torch.from_numpy(host).cuda(), np.array(offs, np.uint64), np.array([len(s) for s in seqs], np.uint64)


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", KS)
def test_resident_entry_points(hg, ctxs, orc, inputs, k, canonical):
    """sketch_batch_dev and sketch_batch_dev_packed on three genomes, default `scaled`, every seed"""
    ctx = ctxs["ascii"]
    seqs = [inputs["random"], inputs["all_T"], inputs["mixed"]]
    n = len(seqs)
    d_seq, offs, lens = upload(seqs)
    sizes = [hg.lib().hg_pack2_size(len(s)) for s in seqs]
    boffs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    d_blobs = torch.zeros(int(sum(sizes)) + 64, dtype=torch.uint8, device="cuda")
    ctx.pack2_batch_dev(d_seq.data_ptr(), offs, lens, d_blobs.data_ptr(), boffs)
    for seed in SEEDS:
        p = hg.default_params(ksize=k, canonical=int(canonical), seed=seed)
        want = [orc.sketch_genome(s, k, p.scaled, seed, canonical, hv_d=p.hv_d) for s in seqs]
        for form in ("ascii", "packed"):
            hv = torch.zeros((n, p.hv_d), dtype=torch.int16, device="cuda")
            n2 = torch.zeros(n, dtype=torch.int32, device="cuda")
            nh = torch.zeros(n, dtype=torch.int32, device="cuda")
            if form == "ascii":
                ctx.sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
            else:
                ctx.sketch_batch_dev_packed(d_blobs.data_ptr(), boffs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
            ctx.sync()
            assert ctx.last_kernel("kmer").endswith("true>") == (form == "packed")
            hv, n2, nh = hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy()
            for i, (w_hv, w_n2, w_nh) in enumerate(want):
                assert nh[i] == w_nh and n2[i] == w_n2 and np.array_equal(hv[i], w_hv), (form, hex(seed), i)
