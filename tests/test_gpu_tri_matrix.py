"""hg_tri_format_dev (libhypergen_tri.so, include/hypergen_tri.h) on crafted float blocks, every byte `==` tests/tri_ref.py.
Values: a 317 x 317 block that holds every m in 0..100 000 as float32(m / 1000); NaN, +-inf, -0.0, -1, 100.0001, 101; the
float32 neighbours of 0.0005, 0.0015, 9.9995 and 99.9995 (ties to even, the carry into the next digit).  Shapes around the
kernel's tile (T columns, Tr rows): 1..5, T - 1, T, T + 1 and 2 T + 3 columns, 1, Tr - 1, Tr and Tr + 1 rows, a pitch, a
matrix one, two and three floats off a 16-byte boundary.  HG_TRI_LOWER with the diagonal above, inside and below a tile, a block
that starts at row 0, odd and even row0 (row starts on and off a 16-byte boundary), a text that itself starts off by 8.  The
text lies between two guards of 64 bytes that must come back intact.  The argument faults return their statuses."""
import numpy as np
import pytest
import torch

import tri_census
import tri_ref

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
POISON = 77.777  # what lies between the rows of a pitched matrix and beyond a LOWER row's fields: formatted, it would show
N_ALL = 317      # 317 * 317 = 100 489 >= 100 001 values


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_tri()
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    with hg.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def geo(hg):
    g = hg.tri_geometry()
    return g["tile_cols"], g["tile_rows"]


def special_values():
    f32 = np.float32
    out = [np.nan, np.inf, -np.inf, -0.0, -1.0, 100.0001, 101.0, 0.0, 100.0]
    for x in (0.0005, 0.0015, 9.9995, 99.9995):
        v = f32(x)
        out += [np.nextafter(v, f32(-1000)), v, np.nextafter(v, f32(1000))]
    out += [0.0625, 0.1875, 96.0625, 96.1875]  # exact ties: odd sixteenths times 1000 end in .5
    return np.array(out, np.float32)


def upload(ani, pitch_extra=0, shift=0):
    """(tensor, pointer, pitch) of a copy of the block that starts `shift` floats behind an aligned address, POISON between the rows"""
    rows, cols = ani.shape
    pitch = cols + pitch_extra
    host = np.full(rows * pitch + shift + 4, POISON, np.float32)
    for r in range(rows):
        host[shift + r * pitch: shift + r * pitch + cols] = ani[r]
    d = torch.from_numpy(host).to("cuda:0")
    return d, d.data_ptr() + 4 * shift, pitch


def run(hg, ctx, ani, layout, row0=0, pitch_extra=0, shift=0, text_shift=0, want_status=None):
    """the block's text between its guards; text_shift 8 puts the text off a 16-byte boundary"""
    rows, cols = ani.shape
    size = tri_ref.text_bytes(layout, row0, rows, cols)
    d_ani, ptr, pitch = upload(ani, pitch_extra, shift)
    d_text = torch.full((GUARD + text_shift + size + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    assert d_text.data_ptr() % 16 == 0
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    st = ctx.tri_format_dev(ptr, rows, cols, pitch, row0, layout, d_text.data_ptr() + GUARD + text_shift, allow=(want_status,) if want_status else ())
    ctx.sync()
    h = d_text.cpu().numpy()
    assert (h[: GUARD + text_shift] == FILL).all() and (h[GUARD + text_shift + size:] == FILL).all(), "a guard was written"
    return st, h[GUARD + text_shift: GUARD + text_shift + size].tobytes()


def same(got, want):
    assert len(got) == len(want)
    if got != want:
        g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        at = int(np.flatnonzero(g != w)[0]) // 8 * 8
        raise AssertionError("%d bytes differ, first in field %d: %r != %r" % ((g != w).sum(), at // 8, got[at: at + 8], want[at: at + 8]))


def lower_block(rng, row0, rows):
    """a LOWER block of global rows [row0, row0 + rows): row0 + rows - 1 columns, POISON at and above the diagonal"""
    cols = max(row0 + rows - 1, 1)
    a = (rng.random((rows, cols)) * 100.0).astype(np.float32)
    for r in range(rows):
        a[r, row0 + r:] = POISON
    return a


def test_every_printed_value(hg, ctx):
    before = hg.tri_launch_counts()
    v = np.zeros(N_ALL * N_ALL, np.float32)
    v[:100_001] = (np.arange(100_001) / 1000.0).astype(np.float32)
    sp = special_values()
    v[100_001: 100_001 + sp.size] = sp
    assert (tri_ref.milli(v[:100_001]) == np.arange(100_001)).all()  # float32 carries every m
    a = v.reshape(N_ALL, N_ALL)
    st, got = run(hg, ctx, a, tri_ref.FULL)
    assert st == hg.OK
    same(got, tri_ref.block_text(a, tri_ref.FULL))
    assert got[:8] == b"  0.000\t" and got[8 * 95_123: 8 * 95_123 + 8] in (b" 95.123\t", b" 95.123\n") and b"100.000" in got
    # the same values below the diagonal of a LOWER block: rows 317..633 carry at least 317 fields each
    low = np.full((N_ALL, 2 * N_ALL - 1), POISON, np.float32)
    low[:, :N_ALL] = a
    for r in range(N_ALL):
        low[r, N_ALL: N_ALL + r] = sp[np.arange(r) % sp.size]
    st, got = run(hg, ctx, low, tri_ref.LOWER, row0=N_ALL)
    assert st == hg.OK
    same(got, tri_ref.block_text(low, tri_ref.LOWER, N_ALL))
    after = hg.tri_launch_counts()
    assert [r.name for r in tri_census.ROWS] == list(after) and all(after[k] > before[k] for k in after)  # every kernel of the census ran


def test_special_values_and_ties(hg, ctx):
    sp = special_values()
    assert tri_ref.milli(sp[:7]).tolist() == [0, 100_000, 0, 0, 0, 100_000, 100_000]
    # 0.0005 and 0.0015 are no float32, their neighbours straddle the tie; the carry: 9.9995 -> 9.999 | 10.000
    m = tri_ref.milli(sp[9:21]).reshape(4, 3)
    assert m[0].tolist()[0] == 0 and m[0].tolist()[2] == 1 and m[1].tolist()[0] == 1 and m[1].tolist()[2] == 2
    assert set(m[2].tolist()) == {9_999, 10_000} and set(m[3].tolist()) == {99_999, 100_000}
    assert tri_ref.milli(sp[21:]).tolist() == [62, 188, 96_062, 96_188]  # ties go to the even neighbour
    for cols in (1, 2, 3, 4, 5, 7):
        a = np.resize(sp, (3, cols)).astype(np.float32)
        for layout in (tri_ref.FULL,):
            st, got = run(hg, ctx, a, layout)
            same(got, tri_ref.block_text(a, layout))
    a = np.resize(sp, (2, sp.size)).astype(np.float32)
    st, got = run(hg, ctx, a, tri_ref.FULL)
    same(got, tri_ref.block_text(a, tri_ref.FULL))
    assert got.startswith(b"  0.000\t100.000\t  0.000\t  0.000\t  0.000\t100.000\t100.000\t  0.000\t100.000\t")


@pytest.mark.parametrize("rows_at", ["1", "Tr-1", "Tr", "Tr+1"])
@pytest.mark.parametrize("cols_at", ["1", "2", "3", "4", "5", "T-1", "T", "T+1", "2T+3"])
def test_full_shapes(hg, ctx, geo, rows_at, cols_at):
    T, Tr = geo
    rows, cols = eval(rows_at, {"Tr": Tr}), eval(cols_at.replace("2T", "2*T"), {"T": T})
    rng = np.random.default_rng(rows * 1000 + cols)
    a = (rng.random((rows, cols)) * 100.0).astype(np.float32)
    a[-1, -1], a[0, 0] = 100.0, 0.0
    want = tri_ref.block_text(a, tri_ref.FULL)
    for pitch_extra, shift, text_shift in ((5, 0, 0), (5, 1, 0), (5, 2, 8), (5, 3, 0), (0, 0, 8)):
        st, got = run(hg, ctx, a, tri_ref.FULL, row0=7, pitch_extra=pitch_extra, shift=shift, text_shift=text_shift)
        assert st == hg.OK
        same(got, want)
    assert want.count(b"\n") == rows and len(want) == 8 * rows * cols


@pytest.mark.parametrize("rows_at", ["1", "Tr-1", "Tr", "Tr+1"])
@pytest.mark.parametrize("row0_at", ["0", "1", "2", "T-1", "T", "T+1", "2T+2", "2T+3"])
def test_lower_shapes(hg, ctx, geo, rows_at, row0_at):
    """row0 0: the first row has no field; T - 1, T, T + 1: the diagonal leaves a tile, ends it, enters the next; odd and even
    row0: the rows' texts start on and off a 16-byte boundary in turn; 2 T + 2 and 2 T + 3: two tiles that test nothing in front"""
    T, Tr = geo
    rows, row0 = eval(rows_at, {"Tr": Tr}), eval(row0_at.replace("2T", "2*T"), {"T": T})
    rng = np.random.default_rng(rows * 1000 + row0)
    a = lower_block(rng, row0, rows)
    want = tri_ref.block_text(a, tri_ref.LOWER, row0)
    assert len(want) == tri_ref.text_bytes(tri_ref.LOWER, row0, rows, a.shape[1])
    for pitch_extra, shift, text_shift in ((5, 0, 0), (5, 1, 8), (0, 2, 0), (5, 3, 8)):
        st, got = run(hg, ctx, a, tri_ref.LOWER, row0=row0, pitch_extra=pitch_extra, shift=shift, text_shift=text_shift)
        assert st == hg.OK
        same(got, want)
    if rows > 1 or row0:
        # more columns than the block needs are not read: the same text
        wide = np.full((rows, a.shape[1] + T + 1), POISON, np.float32)
        wide[:, : a.shape[1]] = a
        st, got = run(hg, ctx, wide, tri_ref.LOWER, row0=row0)
        same(got, want)


def test_a_block_of_several_row_tiles_across_the_diagonal(hg, ctx, geo):
    T, Tr = geo
    rows, row0 = 3 * Tr + 5, T - Tr - 2  # the diagonal crosses the tile boundary at column T inside the block
    a = lower_block(np.random.default_rng(5), row0, rows)
    st, got = run(hg, ctx, a, tri_ref.LOWER, row0=row0, pitch_extra=5, shift=1)
    same(got, tri_ref.block_text(a, tri_ref.LOWER, row0))
    a = (np.random.default_rng(6).random((rows, 2 * T + 3)) * 100.0).astype(np.float32)
    st, got = run(hg, ctx, a, tri_ref.FULL, row0=row0, pitch_extra=5, shift=3, text_shift=8)
    same(got, tri_ref.block_text(a, tri_ref.FULL))


def test_empty_blocks_and_refusals(hg, ctx, geo):
    T, Tr = geo
    R, Q = 5, 9
    a = np.zeros((R, Q), np.float32)
    d_ani, ptr, pitch = upload(a)
    d_text = torch.full((1024,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    before = hg.tri_launch_counts()
    text = d_text.data_ptr() + 64
    for layout in (tri_ref.LOWER, tri_ref.FULL):
        for rows, cols in ((0, Q), (R, 0), (0, 0)):
            assert ctx.tri_format_dev(ptr, rows, cols, pitch, 0, layout, text) == hg.OK
        assert ctx.tri_format_dev(0, 0, Q, Q, 0, layout, text) == hg.OK  # (no block: no pointer needed)
    assert ctx.tri_format_dev(ptr, 1, Q, pitch, 0, tri_ref.LOWER, text) == hg.OK  # row 0 alone: no field
    bad = [dict(layout=2), dict(layout=0xFFFFFFFF), dict(text=0), dict(text=text + 4), dict(ani=0), dict(ani=ptr + 2), dict(pitch=Q - 1),
           dict(row0=Q - R + 2, layout=tri_ref.LOWER)]  # (LOWER: the last row, Q + 1, needs Q + 1 columns)
    for kw in bad:
        st = ctx.tri_format_dev(kw.get("ani", ptr), R, Q, kw.get("pitch", pitch), kw.get("row0", 0), kw.get("layout", tri_ref.FULL),
                                kw.get("text", text), allow=(hg.ERR_INVALID,))
        assert st == hg.ERR_INVALID, kw
    assert ctx.tri_format_dev(ptr, R, Q, pitch, Q - R + 1, tri_ref.LOWER, text) == hg.OK  # ... and Q columns do for row Q
    top = 1 << 31
    for rows, cols, row0 in ((R, Q, top - R + 1), (R, top + 1, 0), (top + 1, Q, 0), (R, Q, top + 5)):
        st = ctx.tri_format_dev(ptr, rows, cols, max(pitch, cols), row0, tri_ref.FULL, text, allow=(hg.ERR_UNSUPPORTED,))
        assert st == hg.ERR_UNSUPPORTED, (rows, cols, row0)
    ctx.sync()
    after = hg.tri_launch_counts()
    assert sum(after.values()) == sum(before.values()) + 1  # only the one good LOWER block launched
    h = d_text.cpu().numpy()
    size = tri_ref.text_bytes(tri_ref.LOWER, Q - R + 1, R, Q)
    assert (h[:64] == FILL).all() and (h[64 + size:] == FILL).all()
    same(h[64: 64 + size].tobytes(), tri_ref.block_text(a, tri_ref.LOWER, Q - R + 1))
