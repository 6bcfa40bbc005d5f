"""hg_frag_ani_matrix_dev (libhypergen_frag.so, include/hypergen_frag.h) on crafted matrices, every record `==` tests/frag_ref.py,
the table of bests included.  The matrices are about 300 x 970: the reference genomes have 1, 2 and the row chunk and the wave
size - 1, + 0, + 1 rows, and one has none; the query genomes have 1, 2 and the wave size, the column tile and the fold's
workgroup - 1, + 0, + 1 columns; Q is no multiple of 4, so three rows in four start off a 16-byte boundary.  Values: NaN, -1,
100.0004, 100.5, equal maxima in two rows of a genome and in two genomes, one exactly at m_th and one a thousandth below."""
import numpy as np
import pytest
import torch

import frag_census
import frag_ref

pytestmark = pytest.mark.gpu

FILL = 0xEE
TH = 50.0  # the threshold of the crafted values: 50.0 is m_th exactly, 49.999 one thousandth below


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
def shape(hg):
    g = hg.frag_geometry()
    rows = [1, 2, g["row_chunk"] - 1, g["row_chunk"], g["row_chunk"] + 1, g["wave"] - 1, g["wave"], g["wave"] + 1, 0, 9]
    cols = sorted({1, 2, 3} | {s + d for s in (g["wave"], g["col_tile"], g["fold_threads"]) for d in (-1, 0, 1)})
    ref_first = np.concatenate(([0], np.cumsum(rows))).astype(np.uint32)
    qry_first = np.concatenate(([0], np.cumsum(cols))).astype(np.uint32)
    assert int(qry_first[-1]) % 4 != 0 and 250 <= int(ref_first[-1]) <= 350
    return ref_first, qry_first


@pytest.fixture(scope="module")
def matrices(shape):
    """name -> (matrix, reference results per threshold), computed once"""
    ref_first, qry_first = shape
    R, Q = int(ref_first[-1]), int(qry_first[-1])
    rng = np.random.default_rng(20260)
    crafted = (rng.random((R, Q)) * 40.0).astype(np.float32)
    g = [(int(ref_first[k]), int(ref_first[k + 1])) for k in range(ref_first.size - 1)]
    crafted[g[2][0]:g[2][1], 0] = np.nan          # a genome that sees only NaN: m 0, its first row
    crafted[g[2][0]:g[2][1], 1] = -1.0            # ... only negative values
    crafted[g[2][0] + 2, 2] = 100.0004            # above 100: 100 000
    crafted[g[2][0] + 3, 3], crafted[g[2][0] + 1, 3] = 100.5, 100.0  # ... ties with 100.0 in an earlier row
    crafted[g[3][0] + 6, 4] = crafted[g[3][0] + 16, 4] = 77.777      # equal maxima in two rows of one genome
    crafted[g[0][0], 5] = crafted[g[1][0], 5] = 88.5                 # ... and in two genomes
    crafted[g[4][0] + 20, 6] = 50.0                                  # exactly m_th
    crafted[g[4][0] + 21, 7] = 49.999                                # one thousandth below
    crafted[g[7][1] - 1, Q - 1] = 99.0                               # the last row of a genome, the last column of the matrix
    crafted[R - 1, Q - 2] = 98.0
    ties = (rng.integers(0, 6, (R, Q)) * 20).astype(np.float32)     # six levels: every column ties in every genome
    ties[rng.random((R, Q)) < 0.05] = np.nan
    out = {}
    for name, a in (("crafted", crafted), ("ties", ties)):
        out[name] = (a, {th: frag_ref.reduce(a, ref_first, qry_first, th) for th in (0.0, TH, 100.0)})
    pair, best = out["crafted"][1][TH]
    assert best["m"][4, 6] == 50000 and best["m"][4, 7] == 49999 and best["row"][2, 3] == g[2][0] + 1 and best["row"][3, 4] == g[3][0] + 6
    assert best["m"][2, 0] == 0 and best["row"][2, 0] == g[2][0] and (best["row"][8] == frag_ref.NONE).all()
    return out


def run(hg, ctx, ani, ref_first, qry_first, th, want_best=True, shift=0):
    """the call on a copy of the matrix that starts `shift` floats behind an aligned address; outputs with sentinels behind"""
    R, Q = ani.shape
    n_ref, n_qry = max(len(ref_first) - 1, 0), max(len(qry_first) - 1, 0)
    d_ani = torch.zeros(R * Q + shift + 4, dtype=torch.float32, device="cuda:0")
    d_ani[shift:shift + R * Q] = torch.from_numpy(ani.reshape(-1)).to("cuda:0")
    d_pair = torch.full((n_ref * n_qry * 16 + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    d_best = torch.full((n_ref * Q * 8 + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st = ctx.frag_ani_matrix_dev(d_ani.data_ptr() + 4 * shift, R, Q, ref_first, qry_first, th, d_pair.data_ptr(),
                                 d_best.data_ptr() if want_best else None)
    assert st == hg.OK
    pair, best = d_pair.cpu().numpy(), d_best.cpu().numpy()
    assert (pair[n_ref * n_qry * 16:] == FILL).all() and (best[n_ref * Q * 8 if want_best else 0:] == FILL).all()
    return (pair[: n_ref * n_qry * 16].view(hg.FRAG_PAIR_DTYPE).reshape(n_ref, n_qry),
            best[: n_ref * Q * 8].view(hg.FRAG_BEST_DTYPE).reshape(n_ref, Q) if want_best else None)


@pytest.mark.parametrize("name", ["crafted", "ties"])
@pytest.mark.parametrize("th", [0.0, TH, 100.0])
def test_equals_the_reference(hg, ctx, shape, matrices, name, th):
    ani, want = matrices[name]
    before = hg.frag_launch_counts()
    pair, best = run(hg, ctx, ani, *shape, th)
    assert (best == want[th][1]).all() and (pair == want[th][0]).all()
    if th == 0.0:
        assert (pair["matched"] == pair["total"]).all()  # every fragment matches, in the genome without rows too
    after = hg.frag_launch_counts()
    assert [r.name for r in frag_census.ROWS] == list(after) and all(after[k] > before[k] for k in after)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_matrix_off_a_16_byte_boundary_and_without_the_bests(hg, ctx, shape, matrices, shift):
    ani, want = matrices["crafted"]
    pair, best = run(hg, ctx, ani, *shape, TH, shift=shift)
    assert (best == want[TH][1]).all() and (pair == want[TH][0]).all()
    pair, _ = run(hg, ctx, ani, *shape, TH, want_best=False, shift=shift)
    assert (pair == want[TH][0]).all()


def test_single_query_genome_and_single_reference_genome(hg, ctx, shape, matrices):
    ani, _ = matrices["ties"]
    R, Q = ani.shape
    for rf, qf in ((shape[0], [0, Q]), ([0, R], shape[1]), ([0, R], [0, Q]), ([0, 0, R, R], [0, 0, Q])):
        want = frag_ref.reduce(ani, rf, qf, 40.0)
        pair, best = run(hg, ctx, ani, rf, qf, 40.0)
        assert (pair == want[0]).all() and (best == want[1]).all()


def test_more_genomes_and_rows_than_one_launch_takes(hg, ctx):
    """45 000 reference genomes of one row (every fifth has none, the last has 40 000) and 10 columns: the genomes go through
    two fold launches, the rows of the second group through two slabs of the matrix, and the second of each starts at an offset"""
    n_ref, Q, T = 45_000, 10, 40_000
    rows = np.ones(n_ref, np.int64)
    rows[::5] = 0
    rows[-1] = T
    ref_first = np.concatenate(([0], np.cumsum(rows))).astype(np.uint32)
    R = int(ref_first[-1])
    assert n_ref > 32768 and T > 32768
    rng = np.random.default_rng(7)
    ani = (rng.integers(0, 1000, (R, Q)) / 10.0).astype(np.float32)
    # (frag_ref.bests loops over the genomes: here every genome is its own row, or none)
    m = frag_ref.milli(ani)
    best = np.zeros((n_ref, Q), frag_ref.BEST_DTYPE)
    best["row"] = frag_ref.NONE
    one = rows == 1
    best["m"][one], best["row"][one] = m[ref_first[:-1][one]], ref_first[:-1][one][:, None]
    tail = m[R - T:]
    best["m"][-1], best["row"][-1] = tail.max(axis=0), R - T + tail.argmax(axis=0)
    want = frag_ref.fold(best, [0, 3, Q], 60.0, R=R)
    pair, got = run(hg, ctx, ani, ref_first, [0, 3, Q], 60.0)
    assert (got == best).all() and (pair == want).all()
    pair, _ = run(hg, ctx, ani, ref_first, [0, 3, Q], 60.0, want_best=False)
    assert (pair == want).all()


def test_empty_comparisons_and_refusals(hg, ctx, shape, matrices):
    ani, _ = matrices["crafted"]
    R, Q = ani.shape
    ref_first, qry_first = shape
    # no rows: every record empty, every best {0, NONE}, whatever the threshold
    pair, best = run(hg, ctx, ani[:0], [0] * len(ref_first), qry_first, 0.0)
    want = frag_ref.reduce(ani[:0], [0] * len(ref_first), qry_first, 0.0)
    assert (pair == want[0]).all() and (best == want[1]).all()
    assert (pair["matched"] == 0).all() and (pair["total"] == np.diff(qry_first)).all() and (best["row"] == hg.FRAG_NONE).all()
    # no columns, no query genome, no reference genome
    pair, _ = run(hg, ctx, ani[:, :0], ref_first, [0, 0, 0], 0.0)
    assert pair.shape == (len(ref_first) - 1, 2) and not pair.view(np.uint8).any()
    assert run(hg, ctx, ani[:, :0], ref_first, [], 50.0)[0].size == 0
    assert run(hg, ctx, ani[:0], [], qry_first, 50.0)[0].size == 0
    d = torch.zeros(R * Q, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(16 * 1024, dtype=torch.uint8, device="cuda:0")
    bad_ref = ref_first.copy()
    bad_ref[3], bad_ref[4] = bad_ref[4], bad_ref[3]
    for rf, qf in ((bad_ref, qry_first), (ref_first[:-1], qry_first), (ref_first, qry_first[1:]), (ref_first, list(qry_first[:-1]) + [Q + 1]), ([], qry_first)):
        assert ctx.frag_ani_matrix_dev(d.data_ptr(), R, Q, rf, qf, 50.0, out.data_ptr(), allow=(hg.ERR_INVALID,)) == hg.ERR_INVALID
    assert ctx.frag_ani_matrix_dev(d.data_ptr(), 1 << 31, 1, [0, 1 << 31], [0, 1], 50.0, out.data_ptr(), allow=(hg.ERR_UNSUPPORTED,)) == hg.ERR_UNSUPPORTED
