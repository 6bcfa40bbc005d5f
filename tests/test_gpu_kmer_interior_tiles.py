"""kmer_sample_shared stages a tile through one of two front ends: an INTERIOR tile (tile_start + NB_T + WIN <= n_bps: every
byte any lane fetches holds bases of the genome) loads from a scalar base plus a lane constant and knows no genome end; an
edge tile does the arithmetic per lane.  Everything here is exact equality with the CPU oracle, at the lengths where the
choice between the two flips, where a wave or a tile ends with the genome, and with non-bases inside interior tiles (the
packed form must raise the tile's "dirty" flag from the blob's bitmap alone).

Geometry (GeoS in hg_kmer_shared.h): 256 lanes x 12 starts are staged (NB_T = 3 072 bases); k <= 21 has a 32-base code
window and tiles of 254 x 12 = 3 048 starts, k = 22..32 a 48-base window and tiles of 253 x 12 = 3 036 starts (a tile then
starts at bit 0 or bit 4 of a bitmap byte, alternating); a work item is 9 tiles."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
NB_T, M = 3072, 12
SCALED = 3
HV_D = 256


def geo(k):
    """(TILE, WIN, hashing lanes)"""
    return (3048, 32, 254) if k <= 21 else (3036, 48, 253)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def ctxs(hg):
    """one ctx per input form of hg_kmer_hash_sample ("packed": the sequence is 2-bit packed on the host and crosses the link
    as a blob, whatever its size; "ascii": never)"""
    out = {}
    for form in ("ascii", "packed"):
        c = hg.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.set_debug("hostfed", form)
        out[form] = c
    yield out
    for c in out.values():
        c.close()


def clean(rng, n):
    return rng.choice(ACGT, n).astype(np.uint8)


def check_hash_sets(ctxs, orc, seqs, k, canonical, norm=0, what=""):
    for i, s in enumerate(seqs):
        want = orc.kmer_hash_sample(s, k, SCALED, 123, canonical, norm)
        for form, c in ctxs.items():
            got = c.kmer_hash_sample(s, k, SCALED, 123, canonical, norm, cap=s.size + 64)
            if s.size >= k:
                assert c.last_kernel("kmer").endswith("true>") == (form == "packed"), (form, c.last_kernel("kmer"))
            assert got.size == want.size and (got == want).all(), (what, form, k, canonical, i, s.size, got.size, want.size)


def upload(seqs, align=16):
    offs, total = [], 0
    for s in seqs:
        offs.append(total)
        total += (len(s) + align - 1) // align * align
    host = np.zeros(total + 64, np.uint8)
    for o, s in zip(offs, seqs):
        host[o:o + len(s)] = s
    return torch.from_numpy(host).cuda(), np.array(offs, np.uint64), np.array([len(s) for s in seqs], np.uint64)


def check_device_paths(hg, ctx, orc, seqs, k, canonical, norm=0, what=""):
    """pack2_batch_dev + sketch_batch_dev_packed == sketch_batch_dev on the ASCII bytes == orc.sketch_genome"""
    n = len(seqs)
    p = hg.default_params(ksize=k, scaled=SCALED, canonical=int(canonical), hv_d=HV_D)
    p.norm_mode = norm
    d_seq, offs, lens = upload(seqs)
    sizes = [hg.lib().hg_pack2_size(len(s)) for s in seqs]
    boffs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    d_blobs = torch.zeros(int(sum(sizes)) + 64, dtype=torch.uint8, device="cuda")
    ctx.pack2_batch_dev(d_seq.data_ptr(), offs, lens, d_blobs.data_ptr(), boffs, norm)
    out = {}
    for form in ("ascii", "packed"):
        hv = torch.zeros((n, HV_D), dtype=torch.int16, device="cuda")
        n2 = torch.zeros(n, dtype=torch.int32, device="cuda")
        nh = torch.zeros(n, dtype=torch.int32, device="cuda")
        if form == "ascii":
            ctx.sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
        else:
            ctx.sketch_batch_dev_packed(d_blobs.data_ptr(), boffs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
        ctx.sync()
        assert ctx.last_kernel("kmer").endswith("true>") == (form == "packed")
        out[form] = (hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy())
    for i, s in enumerate(seqs):
        w_hv, w_n2, w_nh = orc.sketch_genome(s, k, SCALED, 123, canonical, norm, hv_d=HV_D)
        for form, (hv, n2, nh) in out.items():
            assert nh[i] == w_nh and n2[i] == w_n2 and np.array_equal(hv[i], w_hv), (what, form, k, canonical, i, s.size)


# ---- the interior boundary: n_bps = t TILE + NB_T + WIN + d makes tile t the last interior one (d >= 0) or an edge tile ----------

def boundary_lengths(k):
    tile, win, _ = geo(k)
    ts = (0, 1, 8, 9) if k <= 21 else (0, 1, 2, 8, 9)  # t = 8 / 9: last tile of a work item / first of the next; 48-base
    return [t * tile + NB_T + win + d for t in ts for d in (-1, 0, 1)]  # windows: t = 1 starts at bit 4, t = 2 at bit 0


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", [4, 17, 21, 22, 32])
def test_interior_boundary(hg, ctxs, orc, k, canonical):
    rng = np.random.default_rng(100 * k + canonical)
    seqs = [clean(rng, n) for n in boundary_lengths(k)]
    check_hash_sets(ctxs, orc, seqs, k, canonical, what="boundary")
    check_device_paths(hg, ctxs["ascii"], orc, seqs, k, canonical, what="boundary")


# ---- a genome that ends with a wave (64 lanes x 12 starts) or with a tile -------------------------------------------------------

@pytest.mark.parametrize("k,canonical", [(21, True), (32, True), (17, False), (24, False)])
def test_genome_ends_at_a_wave_or_tile_boundary(hg, ctxs, orc, k, canonical):
    tile = geo(k)[0]
    lens = [768 * w + k - 1 + d for w in (1, 4, 5) for d in (-1, 0, 1)] + [tile + k - 1, tile + k]  # n_starts = TILE, TILE + 1
    rng = np.random.default_rng(7 * k)
    seqs = [clean(rng, n) for n in lens]
    check_hash_sets(ctxs, orc, seqs, k, canonical, what="wave/tile end")
    check_device_paths(hg, ctxs["ascii"], orc, seqs, k, canonical, what="wave/tile end")


# ---- non-bases inside an interior tile (and the same in the edge tile), one feature per genome and all together ---------------

def nonbase_genomes(rng, k, with_u):
    """3-tile genomes: tiles 0 and 1 interior, tile 2 an edge tile; the features sit in tile 1 or in tile 2"""
    tile, win, lanes = geo(k)
    n = 2 * tile + 2000
    assert tile + NB_T + win <= n < 2 * tile + NB_T + win
    base = clean(rng, n)
    out = []
    for t0 in (tile, 2 * tile):
        last = M * (lanes - 1) if t0 == tile else M * ((n - k - t0) // M)  # the tile's last lane with a k-mer start
        feats = [
            [(t0 + 5, b"N")],                       # the first lane's window only
            [(t0 + last + 7, b"N")],                # the last hashing lane's window
            [(t0 + M * 50 + M - 1, b"NN")],         # across the units of lanes 50 and 51
            [(t0 + M * 120 + 3, bytes(base[t0 + M * 120 + 3:t0 + M * 120 + 43] | 0x20))],  # a lower-case run: still bases
        ]
        if with_u:
            feats.append([(t0 + M * 150 + 3, b"U"), (t0 + M * 155, b"u")])
        feats.append([f for fs in feats for f in fs])
        for fs in feats:
            s = base.copy()
            for at, b in fs:
                s[at:at + len(b)] = np.frombuffer(b, np.uint8)
            out.append(s)
    return out


@pytest.mark.parametrize("k,canonical", [(21, True), (32, True), (17, False), (22, True)])
def test_interior_non_bases(hg, ctxs, orc, k, canonical):
    rng = np.random.default_rng(300 + k)
    seqs = nonbase_genomes(rng, k, False)
    check_hash_sets(ctxs, orc, seqs, k, canonical, what="non-bases")
    check_device_paths(hg, ctxs["ascii"], orc, seqs, k, canonical, what="non-bases")


@pytest.mark.parametrize("norm", [0, 1], ids=["acgt", "u2t"])
@pytest.mark.parametrize("k", [21, 32])
def test_interior_u_under_both_norm_modes(hg, ctxs, orc, k, norm):
    """u/U is a T under HG_NORM_U2T (ASCII form: rewritten in the kernel; packed form: by the packer) and a non-base otherwise"""
    rng = np.random.default_rng(400 + k)
    seqs = nonbase_genomes(rng, k, True)
    check_hash_sets(ctxs, orc, seqs, k, True, norm, what="U")
    check_device_paths(hg, ctxs["ascii"], orc, seqs, k, True, norm, what="U")


# ---- one batch with grouped small genomes (edge path only), a genome of exactly one interior tile, and a large one ------------

@pytest.mark.parametrize("k", [21, 32])
def test_mixed_batch(hg, ctxs, orc, k):
    tile, win, _ = geo(k)
    rng = np.random.default_rng(500 + k)
    seqs = [clean(rng, n) for n in (2000, NB_T + win, 60_000, 2000, 1999, NB_T + win - 1, 2 * tile + 5)]
    seqs[2][30_000] = ord("N")  # an interior tile of the large genome with a non-base
    check_device_paths(hg, ctxs["ascii"], orc, seqs, k, True, what="mixed")
