"""Host-side checks of the crafted genomes of test_gpu_sampling_edges.py (tests/sampling_craft.py): with the oracle and the batch
plan of hg_sketch_plan_describe only, no GPU.  The device tests rely on these properties; a change of the tile or work-item
geometry that took them away would turn those tests into tests of nothing:
  * the work-item size the crafted layouts assume is the plan's;
  * every work item that a dense stretch fills holds more distinct sampled k-mers than the LDS hit list has entries -- three
    times as many for kmer_sample_shared (k <= 28), more for kmer_sample_long at k = 33 and 40;
  * every large crafted genome samples more distinct hashes than its hit region has slots, at every scaled of the tests;
  * the small dense genome shares one workgroup with ordinary neighbours on both sides, and fills none of its limits.
"""
import numpy as np
import pytest

from sampling_craft import (B_KS, B_SCALED, STAGE, SPARSE, dense_batch, dense_count, item_starts, offsets_for, thr,
                            window_hashes)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.mark.parametrize("k", sorted(set(B_KS) | {1, 16, 22, 32, 255}))
def test_work_item_size_is_the_plans(hg, k):
    item = item_starts(k)
    for n_starts, items in ((item, 1), (item + 1, 2), (3 * item, 3)):
        d, _ = hg.sketch_plan_describe(offsets_for([n_starts + k - 1]), [n_starts + k - 1], k, SPARSE)
        assert d["items"] == items, (k, n_starts, d)
    if k <= 32:
        assert d["item_tiles"] == 9 and item % 9 == 0


B_CELLS = [(k, c, cl) for k in B_KS for c in (True, False) for cl in (False, True)]


@pytest.mark.parametrize("k,canonical,clean", B_CELLS,
                         ids=["k%d-%s-%s" % (k, "canon" if c else "fwd", "clean" if cl else "dirty") for k, c, cl in B_CELLS])
def test_dense_genomes_overload_stage_and_hit_region(hg, orc, k, canonical, clean):
    genomes, roles, chosen = dense_batch(orc, k, canonical, clean)
    t = np.uint64(thr(SPARSE))  # the sparsest threshold of the tests: the counts below hold at every other one
    item = item_starts(k)
    for g, role, ch in zip(genomes, roles, chosen):
        if role not in ("head", "across", "tail"):
            continue
        assert ch.size == dense_count(k) and np.unique(ch).size == ch.size
        pos, h = window_hashes(orc, g, k, canonical)
        keep = h < t
        assert np.isin(ch, h[keep]).all(), role  # every chosen k-mer is sampled where it was placed
        distinct = np.unique(h[keep]).size
        # distinct sampled hashes per work item of the genome
        per_item = np.array([np.unique(h[keep & (pos // item == i)]).size for i in range(int(pos[-1]) // item + 1)])
        full = per_item[per_item > STAGE]
        if k <= 28:
            assert full.size >= 1 and full.max() > 3 * STAGE, (role, per_item)
        elif k <= 40:
            assert full.size >= 1, (role, per_item)
        if role == "across" and k <= 40:  # the stretch overloads the work items on both sides of a boundary
            assert full.size >= 2, per_item
        for scaled in B_SCALED:
            d, _ = hg.sketch_plan_describe(offsets_for([g.size]), [g.size], k, scaled)
            assert distinct > d["max_cap"], (role, scaled, distinct, d)


@pytest.mark.parametrize("k", [k for k in B_KS if k <= 32])
@pytest.mark.parametrize("clean", [False, True], ids=["dirty", "clean"])
def test_small_dense_genome_shares_a_workgroup(hg, orc, k, clean):
    genomes, roles, chosen = dense_batch(orc, k, True, clean)
    lens = [g.size for g in genomes]
    j = roles.index("small")
    assert 1_500 <= lens[j] <= 3_000
    assert roles[j - 1] == roles[j + 1] == "plain" and max(lens[j - 1], lens[j + 1]) < 3_000
    item = item_starts(k)
    items = [-(-max(0, n - k + 1) // item) for n in lens]
    first = int(np.sum(items[:j]))  # the small genomes have one work item each
    for scaled in B_SCALED:
        d, gf = hg.sketch_plan_describe(offsets_for(lens), lens, k, scaled)
        assert d["items"] == sum(items)
        grp = int(np.searchsorted(gf, first, "right")) - 1
        assert gf[grp] <= first - 1 and first + 1 < gf[grp + 1], (scaled, first, gf)
        # nothing overflows: the genome's distinct sampled hashes fit the LDS list and its hit region
        _, h = window_hashes(orc, genomes[j], k, True)
        n = np.unique(h[h < np.uint64(thr(scaled))]).size
        d1, _ = hg.sketch_plan_describe(offsets_for([lens[j]]), [lens[j]], k, scaled)
        assert chosen[j].size <= n < min(STAGE, d1["max_cap"]), (n, d1)
