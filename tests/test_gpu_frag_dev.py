"""hg_frag_ani_dev and hg_frag_ani (libhypergen_frag.so) on clustered random hypervectors: 600 reference windows of 200 hashes,
500 query fragments of 100 hashes that share 0 to 100 of them with one window, D = 4096.  Under each of the three ANI metrics
the records equal tests/frag_ref.py applied to the matrix hg_dist_full_dev writes for the same inputs, for every block_rows --
1 and 7 cut every genome, 64 some, R none -- and are therefore identical across them."""
import numpy as np
import pytest
import torch

import frag_ref

pytestmark = pytest.mark.gpu

HV_D, KSIZE, TH = 4096, 21, 90.0
REF_GENOMES = [70, 1, 33, 200, 0, 64, 232]  # windows per reference genome: 600
QRY_GENOMES = [100, 1, 255, 144]            # fragments per query genome: 500
BLOCK = 10                                  # hashes per shared block: a fragment shares 0..10 blocks with its window
SHARES = [0, 1, 2, 5, 10]                   # (at k = 21 a containment of 12.2 % reads as 90: one block is below, two are above)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_frag()
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    with hg.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def sketches():
    """(ref hv, ref norm2, qry hv, qry norm2) on the device and the offsets.  A hash adds a +-1 vector; 10 of them are
    normal(0, 10) rounded per dimension, which is all the ANI arithmetic sees of them."""
    R, Q = sum(REF_GENOMES), sum(QRY_GENOMES)
    rng = np.random.default_rng(4096)

    def hashes(n, shape):
        return np.rint(np.sqrt(n) * rng.standard_normal(shape, np.float32)).astype(np.int32)

    blocks = hashes(BLOCK, (R, 10, HV_D))                       # the 100 hashes of a window a fragment may share, in blocks
    ref = blocks.sum(axis=1) + hashes(100, (R, HV_D))           # ... and 100 it never does
    of = rng.integers(0, R, Q)                                  # the window a fragment comes from
    share = rng.choice(SHARES, Q)
    qry = np.stack([blocks[of[q], : share[q]].sum(axis=0) for q in range(Q)])
    qry += np.stack([hashes(100 - BLOCK * share[q], HV_D) if share[q] < 10 else np.zeros(HV_D, np.int32) for q in range(Q)])
    dev = "cuda:0"
    out = []
    for hv in (ref, qry):
        out += [torch.from_numpy(hv.astype(np.int16)).to(dev), torch.from_numpy((hv.astype(np.int64) ** 2).sum(axis=1).astype(np.int32)).to(dev)]
    rf = np.concatenate(([0], np.cumsum(REF_GENOMES))).astype(np.uint32)
    qf = np.concatenate(([0], np.cumsum(QRY_GENOMES))).astype(np.uint32)
    torch.cuda.synchronize()
    return out, rf, qf


def reduce_dev(hg, ctx, sketches, block_rows, want_best=True):
    (rh, rn, qh, qn), rf, qf = sketches
    R, Q, n_ref, n_qry = rh.shape[0], qh.shape[0], len(rf) - 1, len(qf) - 1
    d_pair = torch.full((n_ref * n_qry * 16,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_best = torch.full((n_ref * Q * 8,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = ctx.frag_ani_dev(rh.data_ptr(), rn.data_ptr(), R, qh.data_ptr(), qn.data_ptr(), Q, HV_D, KSIZE, rf, qf, TH, d_pair.data_ptr(),
                          d_best.data_ptr() if want_best else None, block_rows=block_rows)
    assert st == hg.OK
    return (d_pair.cpu().numpy().view(hg.FRAG_PAIR_DTYPE).reshape(n_ref, n_qry),
            d_best.cpu().numpy().view(hg.FRAG_BEST_DTYPE).reshape(n_ref, Q) if want_best else None)


@pytest.mark.parametrize("metric", ["ANI_CONTAINMENT", "ANI_MASH", "ANI_MAX_CONTAINMENT"])
def test_equals_the_reference_on_the_dist_matrix_for_every_block_size(hg, ctx, sketches, metric):
    (rh, rn, qh, qn), rf, qf = sketches
    R, Q = rh.shape[0], qh.shape[0]
    ctx.set_ani_metric(getattr(hg, metric))
    try:
        full = torch.empty(R * Q, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.dist_full_dev(rh.data_ptr(), rn.data_ptr(), R, qh.data_ptr(), qn.data_ptr(), Q, HV_D, KSIZE, full.data_ptr())
        ctx.sync()
        want_pair, want_best = frag_ref.reduce(full.cpu().numpy().reshape(R, Q), rf, qf, TH)
        results = [reduce_dev(hg, ctx, sketches, b) for b in (0, 1, 7, 64, R)]
        for pair, best in results:
            assert (best == want_best).all() and (pair == want_pair).all()
        assert all(r[0].tobytes() == results[0][0].tobytes() and r[1].tobytes() == results[0][1].tobytes() for r in results)
        pair, _ = reduce_dev(hg, ctx, sketches, 7, want_best=False)
        assert (pair == want_pair).all()
        if metric == "ANI_CONTAINMENT":  # the inputs do what they were made for: matched and unmatched fragments in numbers
            matched = int(want_pair["matched"].sum())
            assert Q // 4 < matched < Q and (want_pair["matched"][4] == 0).all() and (want_pair["total"] == np.diff(qf)).all()
            # the host form stages the same arrays: the same records
            pair, best = ctx.frag_ani(rh.cpu().numpy(), rn.cpu().numpy(), qh.cpu().numpy(), qn.cpu().numpy(), rf, qf, TH, ksize=KSIZE)
            assert (pair == want_pair).all() and (best == want_best).all()
    finally:
        ctx.set_ani_metric(hg.ANI_MASH)
