"""hg_hist_add_matrix_dev (libhypergen_hist.so, include/hypergen_hist.h) on crafted matrices, every count `==` tests/hist_ref.py.
The matrix is 300 x 970: two row tiles and four column tiles of hist_count_kernel, Q no multiple of 4 -- three rows in four
start off a 16-byte boundary and the last lane of a row owns two columns.  Values: random ones in 0..40, NaN, -1, -0.0, +inf,
100.0004, 100.5, for every width a bin edge and the value one thousandth below it, at width 1 the values around the first two
slice boundaries of the LDS table, the last row and the last column.  Widths: one per path of the kernel -- 13 slices (1), two
slices (7), one table without copies (13), two copies (33), four (100 and up).  The three selections with the diagonal through
the block's interior, a pitch, a matrix off a 16-byte boundary, two and four calls into one table, a block wholly below the
diagonal, the worst contention (one repeated value; all NaN), a block at the top of the index range, the argument faults."""
import numpy as np
import pytest
import torch

import hist_census
import hist_ref

pytestmark = pytest.mark.gpu

FILL = 0xEE
R, Q = 300, 970
ROW0, COL0 = 1000, 800  # the diagonal i == j enters the block at column 200 and leaves it at column 499: through tile corners' neighbourhood
WIDTHS = [1, 7, 13, 33, 100, 1000, 33_333, 100_000]
EDGES = {1: (12_345,), 7: (35_000,), 13: (65_000,), 33: (66_000,), 100: (95_000,), 1000: (96_000,), 33_333: (33_333, 66_666, 99_999), 100_000: (100_000,)}
POISON = 77.777  # what lies between the rows of a pitched matrix: counted, it would show


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_hist()
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    with hg.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def crafted(hg):
    geo = hg.hist_geometry()
    S = geo["lds_bins"]
    assert R > geo["tile_rows"] and Q > 3 * geo["tile_cols"] and Q % 4 != 0
    rng = np.random.default_rng(20261)
    a = (rng.random((R, Q)) * 40.0).astype(np.float32)
    a[rng.random((R, Q)) < 0.3] = 0.0  # the skew of unrelated pairs
    special = [np.nan, -1.0, -0.0, np.inf, 100.0004, 100.5, 0.0004]
    milli = [S - 1, S, S + 1, 2 * S - 1, 2 * S]
    for w in WIDTHS:
        for e in EDGES[w]:
            assert e % w == 0
            milli += [e, e - 1]
    values = special + [m / 1000.0 for m in milli]
    # every value above the diagonal, below it and on it (the diagonal of the block at ROW0, COL0 is column r + 200), and in the corners
    for k, v in enumerate(values):
        a[3 + k, 700 + k] = v
        a[250 - k, 10 + k] = v
        a[20 + k, 220 + k] = v
        a[257 + k % 40, 457 + k % 40] = v  # the diagonal behind the tile corner (256, 456)
    a[R - 1, Q - 1], a[R - 1, 0], a[0, Q - 1], a[0, 0] = 99.0, 98.0, 97.0, 96.0
    a[R - 1, Q - 2], a[R - 2, Q - 1] = 100.5, np.nan
    assert (hist_ref.milli(np.array(values[len(special):], np.float32)) == np.array(milli)).all()  # float32 carries every crafted m
    return a


def upload(ani, pitch_extra=0, shift=0):
    """(tensor, pointer, pitch) of a copy of the matrix that starts `shift` floats behind an aligned address, POISON between the rows"""
    rows, cols = ani.shape
    pitch = cols + pitch_extra
    host = np.full(rows * pitch + shift + 4, POISON, np.float32)
    for r in range(rows):
        host[shift + r * pitch: shift + r * pitch + cols] = ani[r]
    d = torch.from_numpy(host).to("cuda:0")
    return d, d.data_ptr() + 4 * shift, pitch


def new_counts(w):
    """zeroed counts with sentinel bytes behind them"""
    n = hist_ref.bins(w)
    d = torch.full((n * 8 + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    d[: n * 8] = 0
    return d


def read_counts(ctx, d, w):
    ctx.sync()
    n = hist_ref.bins(w)
    h = d.cpu().numpy()
    assert (h[n * 8:] == FILL).all()
    return h[: n * 8].view(np.uint64).copy()


def run(hg, ctx, ani, w, pairs, row0=0, col0=0, pitch_extra=0, shift=0):
    d_ani, ptr, pitch = upload(ani, pitch_extra, shift)
    d_counts = new_counts(w)
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    assert ctx.hist_add_matrix_dev(ptr, ani.shape[0], ani.shape[1], pitch, row0, col0, pairs, w, d_counts.data_ptr()) == hg.OK
    return read_counts(ctx, d_counts, w)


def same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "bins %s: %s != %s" % (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("pairs", [hist_ref.ALL, hist_ref.UPPER, hist_ref.OFFDIAG])
@pytest.mark.parametrize("w", WIDTHS)
def test_equals_the_reference(hg, ctx, crafted, w, pairs):
    before = hg.hist_launch_counts()
    want = hist_ref.counts(crafted, w, pairs, ROW0, COL0)
    got = run(hg, ctx, crafted, w, pairs, ROW0, COL0)
    same(got, want)
    n_sel = int(hist_ref.selected(R, Q, ROW0, COL0, pairs).sum())
    assert int(got.sum()) == n_sel and (pairs == hist_ref.ALL or 0 < R * Q - n_sel)
    after = hg.hist_launch_counts()
    assert [r.name for r in hist_census.ROWS] == list(after) and all(after[k] > before[k] for k in after)  # every kernel of the census ran


@pytest.mark.parametrize("w", [1, 100])
@pytest.mark.parametrize("pitch_extra,shift", [(5, 0), (0, 1), (0, 2), (5, 3), (0, 3)])
def test_pitch_and_a_matrix_off_a_16_byte_boundary(hg, ctx, crafted, w, pitch_extra, shift):
    for pairs in (hist_ref.ALL, hist_ref.UPPER):
        same(run(hg, ctx, crafted, w, pairs, ROW0, COL0, pitch_extra, shift), hist_ref.counts(crafted, w, pairs, ROW0, COL0))


@pytest.mark.parametrize("pairs", [hist_ref.ALL, hist_ref.UPPER, hist_ref.OFFDIAG])
def test_calls_into_one_table_add_up(hg, ctx, crafted, pairs):
    w = 7
    want = hist_ref.counts(crafted, w, pairs, ROW0, COL0)
    d_ani, ptr, pitch = upload(crafted)
    for r_cut, c_cut in ((130, Q), (257, 513), (1, Q - 1)):
        d_counts = new_counts(w)
        torch.cuda.synchronize()
        for r0, r1 in ((0, r_cut), (r_cut, R)):
            for c0, c1 in ((0, c_cut), (c_cut, Q)):
                # a part of the matrix is the matrix with a pitch, at its own global indices
                st = ctx.hist_add_matrix_dev(ptr + 4 * (r0 * pitch + c0), r1 - r0, c1 - c0, pitch, ROW0 + r0, COL0 + c0, pairs, w, d_counts.data_ptr())
                assert st == hg.OK
        same(read_counts(ctx, d_counts, w), want)
    # ... and the same block twice is every count twice
    d_counts = new_counts(w)
    torch.cuda.synchronize()
    for _ in range(2):
        ctx.hist_add_matrix_dev(ptr, R, Q, pitch, ROW0, COL0, pairs, w, d_counts.data_ptr())
    same(read_counts(ctx, d_counts, w), 2 * want)


def test_a_block_outside_the_selection_launches_nothing(hg, ctx, crafted):
    d_ani, ptr, pitch = upload(crafted)
    for row0, col0, rows, cols in ((5000, 0, R, Q), (Q - 1, 0, R, Q), (0, 0, R, 1), (7, 7, 1, 1)):
        for pairs in (hist_ref.UPPER, hist_ref.OFFDIAG):
            if pairs == hist_ref.OFFDIAG and (rows, cols) != (1, 1):
                continue
            d_counts = new_counts(100)
            torch.cuda.synchronize()
            before = hg.hist_launch_counts()
            assert ctx.hist_add_matrix_dev(ptr, rows, cols, pitch, row0, col0, pairs, 100, d_counts.data_ptr()) == hg.OK
            assert hg.hist_launch_counts() == before
            assert not read_counts(ctx, d_counts, 100).any()
            assert not hist_ref.selected(rows, cols, row0, col0, pairs).any()
    # one row further up the first pair appears: (Q - 2, Q - 1)
    got = run(hg, ctx, crafted, 100, hist_ref.UPPER, Q - 2, 0)
    same(got, hist_ref.counts(crafted, 100, hist_ref.UPPER, Q - 2, 0))
    assert int(got.sum()) == 1


@pytest.mark.parametrize("w", [1, 7, 33, 100, 100_000])
def test_worst_contention(hg, ctx, w):
    """one repeated non-zero value: every LDS atomic of a wave hits one address; all NaN: the register path of bin 0"""
    rows, cols = 256, 1024
    for value, m in ((97.5, 97_500), (np.nan, 0)):
        a = np.full((rows, cols), value, np.float32)
        got = run(hg, ctx, a, w, hist_ref.ALL)
        want = np.zeros(hist_ref.bins(w), np.uint64)
        want[m // w] = rows * cols
        same(got, want)
    got = run(hg, ctx, a, w, hist_ref.UPPER, 100, 0)  # (all NaN under the mask: bin 0 counts the selected pairs only)
    assert int(got[0]) == int(hist_ref.selected(rows, cols, 100, 0, hist_ref.UPPER).sum()) and not got[1:].any()


def test_a_block_at_the_top_of_the_index_range(hg, ctx, crafted):
    top = 1 << 31
    for pairs in (hist_ref.UPPER, hist_ref.OFFDIAG):
        got = run(hg, ctx, crafted, 100, pairs, top - R, top - Q)  # its last row and its last column are 2^31 - 1; the diagonal crosses it
        same(got, hist_ref.counts(crafted, 100, pairs, top - R, top - Q))
        assert 0 < int(got.sum()) < R * Q
    d_ani, ptr, pitch = upload(crafted)
    d_counts = new_counts(100)
    torch.cuda.synchronize()
    before = hg.hist_launch_counts()
    for row0, col0 in ((top - R + 1, 0), (0, top - Q + 1), (top + 5, 0)):
        st = ctx.hist_add_matrix_dev(ptr, R, Q, pitch, row0, col0, hist_ref.ALL, 100, d_counts.data_ptr(), allow=(hg.ERR_UNSUPPORTED,))
        assert st == hg.ERR_UNSUPPORTED
    assert hg.hist_launch_counts() == before and not read_counts(ctx, d_counts, 100).any()


def test_empty_blocks_and_refusals(hg, ctx, crafted):
    d_ani, ptr, pitch = upload(crafted)
    d_counts = new_counts(100)
    torch.cuda.synchronize()
    before = hg.hist_launch_counts()
    for rows, cols in ((0, Q), (R, 0), (0, 0)):
        assert ctx.hist_add_matrix_dev(ptr, rows, cols, pitch, 0, 0, hist_ref.ALL, 100, d_counts.data_ptr()) == hg.OK
    assert ctx.hist_add_matrix_dev(0, 0, Q, Q, 0, 0, hist_ref.ALL, 100, d_counts.data_ptr()) == hg.OK  # (no block: no pointer needed)
    bad = [dict(pairs=3), dict(pairs=0xFFFFFFFF), dict(w=0), dict(w=100_001), dict(counts=0), dict(counts=d_counts.data_ptr() + 4),
           dict(ani=0), dict(ani=ptr + 2), dict(pitch=Q - 1)]
    for kw in bad:
        st = ctx.hist_add_matrix_dev(kw.get("ani", ptr), R, Q, kw.get("pitch", pitch), 0, 0, kw.get("pairs", hist_ref.ALL), kw.get("w", 100),
                                     kw.get("counts", d_counts.data_ptr()), allow=(hg.ERR_INVALID,))
        assert st == hg.ERR_INVALID, kw
    assert hg.hist_launch_counts() == before and not read_counts(ctx, d_counts, 100).any()
