"""FracMinHash sampling at the exact threshold and under adversarial hit density, in every k-mer kernel.

A. hg_kmer_hash_sample takes the threshold itself: thresholds ON, one above and one below hashes of the sequence's own set
   (the smallest, the largest, the two around the dense_sampling switch at (2^64 - 1) // 850, hashes whose low dword is near 0
   or near 2^32), the same hash's high dword with the low dword all zero / all one / carried into the high dword, and fixed
   thresholds from 0 to 2^64 - 1.  Every template family and both code windows (k = 1 .. 255), both strand modes, both input
   forms, a few seeds whose SGPR halves are 0 or all ones.  `h <= threshold`, a compare of the high dwords only or a threshold
   with swapped halves fails here; random hashes almost never come near the threshold.
B. Genomes made of DISTINCT sampled k-mers (tests/sampling_craft.py), packed as densely as their spacing allows: several times a
   work item's LDS list, more than the genome's hit region, at scaled = 1 500 / 851 / 850 / 849 (the stage has 256 entries at
   all four; the quarter-full flushes between tiles start at 849), through hg_kmer_hash_sample, hg_sketch_batch,
   hg_sketch_batch_dev (the crafted genomes come out through the re-run) and the streaming entry points.  A hit lost, stored
   twice or filed under a neighbouring genome changes a set of distinct hashes and fails the comparison with the oracle.
"""
import numpy as np
import pytest
import torch

from sampling_craft import B_KS, B_SCALED, DENSE_EDGE, MAX, dense_batch, offsets_for, thr, window_hashes

pytestmark = pytest.mark.gpu

A_KS = (1, 2, 5, 8, 9, 16, 17, 21, 22, 24, 25, 31, 32, 33, 40, 48, 63, 64, 65, 100, 128, 200, 255)
A_LENS = (20_000, 27_500, 31_000, 45_000, 60_000)  # (by k mod 5) all cross tiles, all but the first also a k <= 32 work item (27 432 / 27 324 starts)
FIXED = (0, 1, DENSE_EDGE, DENSE_EDGE + 1, 2**63 - 1, 2**63, MAX - 1, MAX)
LO = 0xFFFFFFFF
ACGT = np.frombuffer(b"ACGT", np.uint8)
PENDING = 0xFFFFFFFF
HV_D = 1024


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module", params=["ascii", "packed"])
def ctx(hg, request):
    """both input forms: "packed" makes the library 2-bit pack each ASCII batch on the device and run the packed-input kernels"""
    c = hg.Context(0)
    c.set_debug("kmer_input", "packed" if request.param == "packed" else "")
    c.form = request.param
    yield c
    c.close()


# ---- A: the threshold compare itself ---------------------------------------------------------------------------------------

def a_sequence(orc, k, canonical, seed):
    """20 - 60 kb of random ACGT with a few Ns, with k-mers planted whose hash has a low dword below 2^16 or above 2^32 - 2^16"""
    rng = np.random.default_rng(9500 + 2 * k + int(canonical) + (seed % 1000003))
    s = rng.choice(ACGT, A_LENS[k % len(A_LENS)] + 7 * k)
    src = rng.choice(ACGT, 300_000)
    pos, h = window_hashes(orc, src, k, canonical, seed)
    low = h & np.uint64(LO)
    for sel in (low < 2**16, low >= 2**32 - 2**16):
        for p in pos[sel][:2]:
            at = int(rng.integers(0, s.size - k))
            s[at:at + k] = src[p:p + k]
    for at in rng.integers(0, s.size, 5):
        s[at] = ord("N")
    return s


def a_thresholds(u):
    """thresholds around hashes of the sorted set u, and the fixed ones"""
    piv = [u[0], u[-1], u[u.size // 2]]
    piv += list(u[u <= np.uint64(DENSE_EDGE)][-1:]) + list(u[u > np.uint64(DENSE_EDGE)][:1])
    low = u & np.uint64(LO)
    piv += list(u[low < 2**16][:2]) + list(u[low >= 2**32 - 2**16][:2])
    out = set(FIXED)
    for h in (int(x) for x in piv):
        out.update((h, h + 1, h - 1, h & ~LO, h | LO))
        if h >> 32 != LO:
            out.add((h | LO) + 1)
    return sorted(t for t in out if 0 <= t <= MAX)


def check_thresholds(ctx, orc, k, canonical, seed):
    s = a_sequence(orc, k, canonical, seed)
    u = np.unique(window_hashes(orc, s, k, canonical, seed)[1])
    ts = a_thresholds(u)
    for t in ts:
        want = u[:int(np.searchsorted(u, np.uint64(t), "left"))]
        got = ctx.kmer_hash_sample(s, k, seed=seed, canonical=canonical, threshold=t, cap=u.size + 64)
        assert got.size == want.size and (got == want).all(), (k, canonical, seed, hex(t), got.size, want.size)
    return u, ts


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", A_KS)
def test_exact_threshold(ctx, orc, k, canonical):
    u, ts = check_thresholds(ctx, orc, k, canonical, 123)
    if k >= 9:  # the set really has hashes on both sides of the dense_sampling switch and near both dword edges
        assert u[0] <= np.uint64(DENSE_EDGE) < u[-1]
        assert ((u & np.uint64(LO)) < 2**16).any() and ((u & np.uint64(LO)) >= 2**32 - 2**16).any()


@pytest.mark.parametrize("seed", [0, 2**32 - 1, 0xFFFFFFFF00000000, MAX], ids=["zero", "lo_ones", "hi_ones", "ones"])
def test_exact_threshold_seed_halves(ctx, orc, seed):
    for k, canonical in ((9, True), (16, False), (21, True), (28, False), (32, True), (40, True), (100, False)):
        check_thresholds(ctx, orc, k, canonical, seed)


# ---- B: distinct-hit density ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dense(orc):
    """(genomes, roles, chosen, window-hash sets, oracle sketches by scaled) per (k, canonical, clean)"""
    cache = {}

    def get(k, canonical, clean):
        key = (k, canonical, clean)
        if key not in cache:
            genomes, roles, chosen = dense_batch(orc, k, canonical, clean)
            sets = [np.unique(window_hashes(orc, g, k, canonical)[1]) for g in genomes]
            cache[key] = (genomes, roles, chosen, sets, {})
        return cache[key]

    def sketches(k, canonical, clean, scaled):
        genomes, _, _, _, sk = get(k, canonical, clean)
        if scaled not in sk:
            sk[scaled] = [orc.sketch_genome(g, ksize=k, scaled=scaled, canonical=canonical, hv_d=HV_D) for g in genomes]
        return sk[scaled]

    get.sketches = sketches
    return get


def params(hg, k, canonical, scaled):
    return hg.default_params(ksize=k, scaled=scaled, canonical=int(canonical), hv_d=HV_D)


def check_sketches(want, hv, n2, nh, what):
    for i, (w_hv, w_n2, w_nh) in enumerate(want):
        assert nh[i] == w_nh and n2[i] == w_n2 and (hv[i] == w_hv).all(), (what, i, int(nh[i]), w_nh)


B_CELLS = [(k, c, cl) for k in B_KS for c in (True, False) for cl in (False, True)]
B_IDS = ["k%d-%s-%s" % (k, "canon" if c else "fwd", "clean" if cl else "dirty") for k, c, cl in B_CELLS]


@pytest.mark.parametrize("k,canonical,clean", B_CELLS, ids=B_IDS)
def test_dense_hash_sets(ctx, orc, dense, k, canonical, clean):
    genomes, roles, chosen, sets, _ = dense(k, canonical, clean)
    for scaled in B_SCALED:
        t = np.uint64(thr(scaled))
        for g, role, ch, u in zip(genomes, roles, chosen, sets):
            if ch is None:
                continue
            want = u[u < t]
            got = ctx.kmer_hash_sample(g, k, scaled=scaled, canonical=canonical, cap=u.size + 64)
            assert got.size == want.size and (got == want).all(), (role, scaled, got.size, want.size)
            assert np.isin(ch, got).all(), (role, scaled)


@pytest.mark.parametrize("k,canonical,clean", B_CELLS, ids=B_IDS)
def test_dense_sketch_batch(ctx, hg, dense, k, canonical, clean):
    genomes = dense(k, canonical, clean)[0]
    for scaled in B_SCALED:
        hv, n2, nh = ctx.sketch_batch(genomes, params(hg, k, canonical, scaled))
        check_sketches(dense.sketches(k, canonical, clean, scaled), hv, n2, nh, ("host-fed", scaled))


@pytest.mark.parametrize("k,canonical,clean", B_CELLS, ids=B_IDS)
def test_dense_sketch_batch_dev_rerun(ctx, hg, dense, k, canonical, clean):
    """the crafted genomes overflow their hit regions: pending after the step, redone by the sync; the others final at once"""
    genomes, roles, _, _, _ = dense(k, canonical, clean)
    lens = np.array([g.size for g in genomes], np.uint64)
    offs = offsets_for(lens)
    host = np.zeros(int(offs[-1] + lens[-1]) + 64, np.uint8)
    for o, g in zip(offs, genomes):
        host[int(o):int(o) + g.size] = g
    d_seq = torch.from_numpy(host).cuda()
    big = [r in ("head", "across", "tail") for r in roles]
    dev = torch.device("cuda:0")
    c = hg.Context(0)  # (a fresh ctx: a plan cached from an earlier call of the same geometry keeps the re-run's larger regions)
    try:
        c.set_debug("kmer_input", "packed" if ctx.form == "packed" else "")
        for scaled in B_SCALED:
            want = dense.sketches(k, canonical, clean, scaled)
            hv = torch.full((len(genomes), HV_D), 7, dtype=torch.int16, device=dev)
            n2 = torch.full((len(genomes),), 7, dtype=torch.int32, device=dev)
            nh = torch.full((len(genomes),), 7, dtype=torch.int32, device=dev)
            c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, params(hg, k, canonical, scaled), hv.data_ptr(), n2.data_ptr(),
                               nh.data_ptr())
            torch.cuda.synchronize()  # (the stream only: not the library's completion point)
            nh0, hv0 = nh.cpu().numpy().view(np.uint32), hv.cpu().numpy()
            for i, (w_hv, _, w_nh) in enumerate(want):
                if big[i]:
                    assert nh0[i] == PENDING and (hv0[i] == 7).all(), (roles[i], scaled, int(nh0[i]))
                else:
                    assert nh0[i] == w_nh and (hv0[i] == w_hv).all(), (roles[i], i, scaled)
            before = c.sketch_step_counts()
            c.sync()
            after = c.sketch_step_counts()
            assert after[2] - before[2] == 1, (scaled, before, after)
            check_sketches(want, hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy().view(np.uint32), ("dev", scaled))
    finally:
        c.close()


@pytest.mark.parametrize("form", ["ascii", "packed"])
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", B_KS)
def test_dense_genome_in_a_stream(hg, orc, dense, k, canonical, form):
    genomes, roles, _, _, _ = dense(k, canonical, False)
    files = [i for i, r in enumerate(roles) if r in ("plain", "across")]  # one dense genome among ordinary files
    for scaled in (1500, 849):
        want = dense.sketches(k, canonical, False, scaled)
        st = hg.SketchStream([0], params(hg, k, canonical, scaled))
        try:
            for i in files:
                if form == "packed":
                    st.push_packed(hg.pack2(genomes[i]), genomes[i].size, i)
                else:
                    st.push(genomes[i], i)
            st.finish()
            seen = {}
            while True:
                r = st.pop()
                if r is None:
                    break
                seen[r[0]] = r[1:]
        finally:
            st.close()
        assert sorted(seen) == files
        for i in files:
            hv, n2, nh = seen[i]
            assert nh == want[i][2] and n2 == want[i][1] and (hv == want[i][0]).all(), (roles[i], i, scaled)
