"""Every kernel that works on packed bits (tests/bits_census.py), run by the input its census row names and then at the shapes
where a bit position, a word boundary or an alignment decides.  Every comparison is integer or byte equality with the CPU
oracle (binarize, hamming_matrix, unpack_hv, unpack_hv_naive, synth_genome) or with the host's hg.pack2; no tolerance appears.

Every output buffer is a Guard: pre-filled with a sentinel byte, with sentinel slack behind it (and in front where the pointer
is shifted), and reading it back asserts that the slack is untouched.  Error-path calls pass only arguments the entry points
refuse before any launch (hg_hamming_full_dev: words % 4; hamming_block_once: ref_off + R > 2^32 - 1; hg_hv_unpack_batch_dev:
widths, layouts and lengths are checked on the host).
"""
import numpy as np
import pytest
import torch

import bits_census as bc
from payload_models import bp8x_model, naive_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5
U32 = 2**32 - 1


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def mctx(hg):
    c = hg.Context(0)
    # (the ctx's own stream does not wait for torch's: the sentinel fills and uploads below must be in front of the kernels)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture
def ctx(mctx):
    """the module's ctx, back on the default paths after each test"""
    yield mctx
    for key in ("dist_path", "dist_tile", "ham_path"):
        mctx.set_debug(key, "")


class Guard:
    """`nbytes` of device memory for a kernel's output between `front` and `slack` bytes that no kernel may touch, all of it
    pre-filled with SENT.  (torch's allocations are 512-byte aligned: `front` is the alignment of ptr.)"""

    def __init__(self, nbytes, front=0, slack=256):
        self.front, self.n = front, int(nbytes)
        self.buf = torch.full((front + self.n + slack,), SENT, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 512 == 0
        self.ptr = self.buf.data_ptr() + front

    def host(self, dtype=np.uint8):
        h = self.buf.cpu().numpy()
        assert (h[:self.front] == SENT).all(), "bytes in front of the output were written"
        assert (h[self.front + self.n:] == SENT).all(), "bytes behind the output were written"
        return h[self.front:self.front + self.n].copy().view(dtype)


def up(a):
    """a host array's bytes on the device"""
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


# ---- Hamming: inputs and the check of a hit list --------------------------------------------------------------------------
def bit_rows(R, Q, hv_d, seed):
    """random bit rows with zero pad bits (as binarize leaves them); planted: a duplicate ((R - 1, 0) at distance 0) and rows
    at distance 1 ((0, 0) when R > 1; (R / 2, Q - 1) when Q > 1, differing in the LAST valid bit)"""
    rng = np.random.default_rng(seed)
    words = (hv_d + 31) // 32
    r = rng.integers(0, 1 << 32, (R, words), dtype=np.uint64).astype(np.uint32)
    q = rng.integers(0, 1 << 32, (Q, words), dtype=np.uint64).astype(np.uint32)
    if hv_d % 32:
        r[:, -1] &= np.uint32((1 << (hv_d % 32)) - 1)
        q[:, -1] &= np.uint32((1 << (hv_d % 32)) - 1)
    q[0] = r[R - 1]
    if R > 1:
        r[0] = q[0]
        r[0, 0] ^= np.uint32(1)
    if Q > 1:
        q[Q - 1] = r[R // 2]
        q[Q - 1, (hv_d - 1) // 32] ^= np.uint32(1 << ((hv_d - 1) % 32))
    return r, q


def check_hits(hg, g, n, st, want, md, cap, ro=0, qo=0, what=None):
    """the records of a search in Guard g (room for more than cap records): exactly the oracle's pairs with their distances,
    shifted by the offsets; beyond cap: HG_ERR_CAPACITY, n = all of them, cap distinct members written, the rest untouched"""
    R, Q = want.shape
    rec = g.host(np.uint32).reshape(-1, 3)
    i, j = np.nonzero(want <= md)
    assert n == i.size, (what, n, i.size)
    assert st == (hg.OK if n <= cap else hg.ERR_CAPACITY), (what, st)
    m = min(n, cap)
    assert rec.shape[0] > m and (rec[m:] == np.uint32(SENT * 0x01010101)).all(), ("records behind the last one were written", what)
    got = rec[:m].astype(np.int64)
    a, b = got[:, 0] - ro, got[:, 1] - qo
    assert ((a >= 0) & (a < R) & (b >= 0) & (b < Q)).all(), what
    key = a * Q + b
    assert np.unique(key).size == m, ("duplicate hits", what)
    assert (want[a, b] <= md).all() and (got[:, 2] == want[a, b]).all(), what
    if n <= cap:
        assert np.array_equal(np.sort(key), i.astype(np.int64) * Q + j), what


def search(hg, ctx, d_ref, R, d_qry, Q, hv_d, md, want, cap=None, ro=0, qo=0, what=None):
    cap = R * Q if cap is None else cap
    g = Guard(12 * (cap + 8))
    n, st = ctx.hamming_search_block_dev(d_ref.data_ptr(), R, ro, d_qry.data_ptr(), Q, qo, hv_d, md, g.ptr, cap)
    check_hits(hg, g, n, st, want, md, cap, ro, qo, what)
    return n


def popc_name(Q):
    return "hamming_kernel<%d>" % (1 if Q <= 16 else 2 if Q <= 32 else 8)


# ---- 1. every row at one small input ------------------------------------------------------------------------------------
ACGT = np.frombuffer(b"ACGT", np.uint8)


def small_genome(seed, L=3000):
    rng = np.random.default_rng(seed)
    s = rng.choice(ACGT, L)
    s[100:140] = ord("N")
    s[2000:2003] = ord("n")
    s[500:520] |= 0x20
    return s


def run_stream_row(hg, orc, forms):
    """a sketch stream fed the given forms: the HVs of hg_sketch_batch's definition (the oracle's).

    unpack2_kernel runs only for a chunk that holds ASCII and packed genomes TOGETHER, and the uploader closes a chunk as soon
    as it finds its queue empty -- two small genomes pushed one after the other may each get a chunk of their own.  So the
    mixed row first pushes a 16 MiB genome (all 'N': nothing to sketch), which fills a chunk alone (a burst's first chunk
    closes at 8 MiB) and whose copy keeps the uploader busy while the small genomes, alternating between the two forms, queue
    up behind it.  Any chunk with two of them holds both forms; the stream's chunk count says that there was one."""
    p = hg.default_params(scaled=20, hv_d=512)
    mixed = set(forms) == {"ascii", "packed"}
    kinds = ["ascii"] + ["ascii", "packed"] * 4 if mixed else list(forms)
    genomes = [small_genome(70 + i) for i in range(len(kinds))]
    if mixed:
        genomes[0] = np.full(16 << 20, ord("N"), np.uint8)
    items = []
    for form, s in zip(kinds, genomes):  # (packed before the first push: nothing but the pushes between two pushes)
        blob = s if form == "ascii" else hg.pack2(s) if form == "packed" else hg.pack2s(s)
        assert blob is not None
        items.append(blob)
    with hg.SketchStream((0,), p) as st:
        for i, (form, s, blob) in enumerate(zip(kinds, genomes, items)):
            if form == "ascii":
                st.push(blob, i)
            elif form == "packed":
                st.push_packed(blob, s.size, i)
            else:
                st.push_packed_sparse(blob, s.size, i)
        st.finish()
        out = {}
        while True:
            r = st.pop()
            if r is None:
                break
            out[r[0]] = r[1:]
        chunks = int(st.stats()["chunks"])
    assert sorted(out) == list(range(len(kinds)))
    if mixed:
        assert 2 <= chunks < len(kinds), "no chunk held an ASCII and a packed genome: unpack2_kernel did not run (%d chunks)" % chunks
    for i, s in enumerate(genomes):
        w_hv, w_n2, w_nh = orc.sketch_genome(s, 21, 20, 123, True, hv_d=512)
        assert (w_nh > 50 or s.size > 3000) and out[i][2] == w_nh and out[i][1] == w_n2 and np.array_equal(out[i][0], w_hv), (kinds, i)


@pytest.mark.parametrize("row", bc.ROWS, ids=[r.name for r in bc.ROWS])
def test_census_row(hg, ctx, orc, row):
    assert row.unreachable is None
    for key, val in row.debug.items():
        ctx.set_debug(key, val)
    if row.entry == "hamming":
        popc = row in bc.HAMMING_ROWS  # the popcount tiles report their own name, the expansions feed the GEMM that is named
        R, Q, hv_d = 129, row.inputs["Q"], 128
        rb, qb = bit_rows(R, Q, hv_d, 5)
        want = orc.hamming_matrix(rb, qb)
        d_r, d_q = up(rb), up(qb)
        for md in (0, hv_d // 2 - 4):
            search(hg, ctx, d_r, R, d_q, Q, hv_d, md, want, what=(row.name, md))
            assert ctx.last_hamming_path() == {"popc": 0, "mfma": 1, "fp4": 2}[row.debug["ham_path"]]
            if popc:
                assert ctx.last_kernel("dist") == row.name
            else:
                assert ctx.last_kernel("dist").startswith("dist_mfma_kernel<")
        if popc:  # the popcount tiles also serve the full matrix
            g = Guard(4 * R * Q)
            ctx.hamming_full_dev(d_r.data_ptr(), R, d_q.data_ptr(), Q, hv_d, g.ptr)
            ctx.sync()
            assert ctx.last_kernel("dist") == row.name and np.array_equal(g.host(np.uint32).reshape(R, Q), want)
    elif row.entry == "binarize":
        run_binarize(ctx, orc, 5, 100, 1)
    elif row.entry == "unpack":
        # one call whose largest payload sizes the LDS stage at its maximum: q = 8 fits it, q = 9 does not
        cases = [(q, lay, (q + lay) % 4) for q in (8, 9) for lay in (hg.PAYLOAD_BITPACKER8X, hg.PAYLOAD_NAIVE)]
        assert len(cases) == len(row.inputs)
        run_unpack(hg, ctx, orc, 32768, cases, seed=1)
    elif row.entry == "pack2":
        run_pack2(hg, ctx, [high_bit_seq(np.random.default_rng(3), 33)], hg.NORM_U2T)
    elif row.entry == "unpack2":
        run_unpack2(hg, ctx, high_bit_seq(np.random.default_rng(4), 33), hg.NORM_U2T)
    elif row.entry == "stream":
        run_stream_row(hg, orc, row.inputs)
    elif row.entry == "synth":
        run_synth(ctx, orc, 12345, 3, 33, 1000, 64)
    else:
        raise AssertionError(row)


# ---- 2. the popcount kernel: tile, K-slice and staging edges ----------------------------------------------------------
# the tile is 128 references x 16 JN queries, a K slice 32 words, rows are read in 16-byte pieces: words = 4, 28, 32, 36, 68
POPC_HVD = (128, 896, 1024, 1152, 2176)
POPC_Q = {1: (1, 16), 2: (17, 32), 8: (33, 128, 129)}
POPC_R = (1, 127, 128, 129, 257)
POPC_CASES = [(POPC_R[(i + k) % 5], POPC_Q[jn][i % len(POPC_Q[jn])], d, jn)
              for k, jn in enumerate((1, 2, 8)) for i, d in enumerate(POPC_HVD)]


def test_popcount_cases_cover_the_cross():
    assert {c[0] for c in POPC_CASES} == set(POPC_R) and {c[1] for c in POPC_CASES} == {1, 16, 17, 32, 33, 128, 129}
    assert {(c[2], c[3]) for c in POPC_CASES} == {(d, jn) for d in POPC_HVD for jn in (1, 2, 8)}
    assert {(d + 31) // 32 for d in POPC_HVD} == {4, 28, 32, 36, 68}


@pytest.mark.parametrize("R,Q,hv_d,jn", POPC_CASES)
def test_popcount_kernel(hg, ctx, orc, R, Q, hv_d, jn):
    rb, qb = bit_rows(R, Q, hv_d, 1000 * R + Q)
    want = orc.hamming_matrix(rb, qb)
    assert (want == 0).any() and ((want == 1).any() or R * Q == 1)
    d_r, d_q = up(rb), up(qb)
    g = Guard(4 * R * Q)
    ctx.hamming_full_dev(d_r.data_ptr(), R, d_q.data_ptr(), Q, hv_d, g.ptr)
    ctx.sync()
    assert ctx.last_kernel("dist") == "hamming_kernel<%d>" % jn
    assert np.array_equal(g.host(np.uint32).reshape(R, Q), want)
    ctx.set_debug("ham_path", "popc")
    for md in (0, 1, hv_d - 1, hv_d, U32):
        n = search(hg, ctx, d_r, R, d_q, Q, hv_d, md, want, what=(R, Q, hv_d, md))
        assert ctx.last_hamming_path() == 0 and ctx.last_kernel("dist") == "hamming_kernel<%d>" % jn
        assert n == R * Q if md >= hv_d else n >= 1


@pytest.mark.parametrize("Q", [16, 32, 129])
def test_popcount_every_pair_hits_fills_and_flushes_the_stage(hg, ctx, orc, Q):
    """each wave stages up to 512 records and flushes above 448: with every pair a hit and all 128 rows of a tile present, the
    JN = 1 stage fills to exactly 512 and the wider tiles flush several times"""
    R, hv_d = 257, 128
    rb, qb = bit_rows(R, Q, hv_d, 31 + Q)
    want = orc.hamming_matrix(rb, qb)
    d_r, d_q = up(rb), up(qb)
    ctx.set_debug("ham_path", "popc")
    for md in (hv_d, hv_d + 1, U32):
        assert search(hg, ctx, d_r, R, d_q, Q, hv_d, md, want, what=(Q, md)) == R * Q
        assert ctx.last_kernel("dist") == popc_name(Q)


def test_hamming_full_refuses_rows_that_are_no_16_byte_pieces(hg, ctx):
    """hv_d = 96: three words per row.  ham_launch refuses before the launch; nothing is written"""
    rb, qb = bit_rows(5, 5, 96, 2)
    d_r, d_q = up(rb), up(qb)
    g = Guard(4 * 25)
    with pytest.raises(hg.HgError) as e:
        ctx.hamming_full_dev(d_r.data_ptr(), 5, d_q.data_ptr(), 5, 96, g.ptr)
    assert e.value.status == hg.ERR_UNSUPPORTED
    ctx.sync()
    assert (g.host() == SENT).all()


# ---- 3. offsets and capacity on all three routes ----------------------------------------------------------------------
ROUTES = [("popc", ""), ("mfma", "big"), ("mfma", "wide"), ("fp4", "big"), ("fp4", "wide")]
_OFFSET_SET = {}


def offset_set(orc):
    if not _OFFSET_SET:
        R, Q, hv_d = 300, 270, 256
        rb, qb = bit_rows(R, Q, hv_d, 41)
        want = orc.hamming_matrix(rb, qb)
        _OFFSET_SET.update(R=R, Q=Q, hv_d=hv_d, rb=rb, qb=qb, want=want, md=int(np.percentile(want, 2)))
    return _OFFSET_SET


@pytest.mark.parametrize("path,tile", ROUTES, ids=["-".join(r).rstrip("-") for r in ROUTES])
def test_hamming_offsets_and_capacity(hg, ctx, orc, path, tile):
    s = offset_set(orc)
    R, Q, hv_d, want, md = s["R"], s["Q"], s["hv_d"], s["want"], s["md"]
    found = int((want <= md).sum())
    assert 500 < found < R * Q // 10
    d_r, d_q = up(s["rb"]), up(s["qb"])
    ctx.set_debug("ham_path", path)
    ctx.set_debug("dist_tile", tile)
    code = {"popc": 0, "mfma": 1, "fp4": 2}[path]
    for ro, qo in ((0, 0), (5, 0), (0, 7), (U32 - R, U32 - Q)):  # the last: the largest offsets the entry point accepts
        assert search(hg, ctx, d_r, R, d_q, Q, hv_d, md, want, ro=ro, qo=qo, what=(path, tile, ro, qo)) == found
        assert ctx.last_hamming_path() == code
    # global indices must fit 32 bits: refused on the host, nothing written
    for ro, qo in ((U32 - R + 1, 0), (0, U32 - Q + 1)):
        g = Guard(12 * 64)
        with pytest.raises(hg.HgError) as e:
            ctx.hamming_search_block_dev(d_r.data_ptr(), R, ro, d_q.data_ptr(), Q, qo, hv_d, md, g.ptr, 64)
        assert e.value.status == hg.ERR_UNSUPPORTED
        assert (g.host() == SENT).all()
    # count only: no output buffer at all
    n, st = ctx.hamming_search_block_dev(d_r.data_ptr(), R, 5, d_q.data_ptr(), Q, 7, hv_d, md, 0, 0)
    assert (n, st) == (found, hg.ERR_CAPACITY)
    n, st = ctx.hamming_search_block_dev(d_r.data_ptr(), R, 5, d_q.data_ptr(), Q, 7, hv_d, 0, 0, 0)
    assert n == int((want == 0).sum()) and n >= 1 and st == hg.ERR_CAPACITY
    # one record too few: all hits counted, cap distinct ones written, the record behind them untouched
    for ro, qo in ((0, 0), (5, 7)):
        assert search(hg, ctx, d_r, R, d_q, Q, hv_d, md, want, cap=found - 1, ro=ro, qo=qo, what=(path, tile, "cap")) == found
    assert search(hg, ctx, d_r, R, d_q, Q, hv_d, md, want, cap=found, what=(path, tile, "cap = found")) == found


# ---- 4. the route choice of a search, no hook set, at its borders -----------------------------------------------------
def test_hamming_route_border_32_queries(hg, ctx, orc):
    """up to 32 queries: the popcount kernel's narrow tiles; 33: still popcount at this size, on the square tile"""
    R, hv_d = 300, 256
    for Q, name in ((32, "hamming_kernel<2>"), (33, "hamming_kernel<8>")):
        rb, qb = bit_rows(R, Q, hv_d, Q)
        want = orc.hamming_matrix(rb, qb)
        for md in (1, int(np.percentile(want, 5))):
            search(hg, ctx, up(rb), R, up(qb), Q, hv_d, md, want, what=(Q, md))
            assert ctx.last_hamming_path() == 0 and ctx.last_kernel("dist") == name


def test_hamming_route_border_2_pow_24_pairs(hg, ctx, orc):
    """R * Q = 2^24 - 64: popcount; 2^24: the matrix pipe (FP4); 2^24 pairs with 32 queries: the narrow popcount tiles all the
    same.  A few planted pairs (in the first and the last reference rows) at a small max_dist"""
    hv_d, md = 128, 6
    for Q, R_hi in ((64, 1 << 18), (32, 1 << 19)):
        rng = np.random.default_rng(Q)
        rb = rng.integers(0, 1 << 32, (R_hi, 4), dtype=np.uint64).astype(np.uint32)
        qb = rng.integers(0, 1 << 32, (Q, 4), dtype=np.uint64).astype(np.uint32)
        for k, row in enumerate((0, 1, 127, 128, R_hi // 2 + 3, R_hi - 130, R_hi - 2, R_hi - 1)):
            qb[5 * k % Q + k // 7] = rb[row]
            qb[5 * k % Q + k // 7, k % 4] ^= np.uint32((1 << (k % 7)) - 1)  # distance k % 7
        want_hi = orc.hamming_matrix(rb, qb)
        d_r, d_q = up(rb), up(qb)
        for R in ((R_hi - 1, R_hi) if Q == 64 else (R_hi,)):
            want = want_hi[:R]
            found = int((want <= md).sum())
            assert 6 <= found <= 64
            assert search(hg, ctx, d_r, R, d_q, Q, hv_d, md, want, cap=1024, what=(R, Q)) == found
            if Q == 32:
                assert ctx.last_hamming_path() == 0 and ctx.last_kernel("dist") == "hamming_kernel<2>"
            elif R * Q < 1 << 24:
                assert R * Q == (1 << 24) - 64 and ctx.last_hamming_path() == 0 and ctx.last_kernel("dist") == "hamming_kernel<8>"
            else:
                assert R * Q == 1 << 24 and ctx.last_hamming_path() == 2


def test_hamming_route_three_words_take_fp4(hg, ctx, orc):
    """hv_d = 96: rows of three words are no 16-byte pieces, the search runs on e2m1 operands"""
    R, Q, hv_d = 140, 50, 96
    rb, qb = bit_rows(R, Q, hv_d, 96)
    want = orc.hamming_matrix(rb, qb)
    for md in (0, 1, int(np.percentile(want, 10)), hv_d - 1, hv_d):
        search(hg, ctx, up(rb), R, up(qb), Q, hv_d, md, want, what=md)
        assert ctx.last_hamming_path() == 2


def test_hamming_route_more_than_65536_dims_take_popcount(hg, ctx, orc):
    """hv_d = 65664 (2052 words): beyond the matrix pipe's operand rows, popcount even when the hook asks for FP4"""
    R = Q = 40
    hv_d = 65664
    rb, qb = bit_rows(R, Q, hv_d, 65)
    want = orc.hamming_matrix(rb, qb)
    for path in ("", "fp4"):
        ctx.set_debug("ham_path", path)
        for md in (1, int(np.median(want))):
            search(hg, ctx, up(rb), R, up(qb), Q, hv_d, md, want, what=(path, md))
            assert ctx.last_hamming_path() == 0 and ctx.last_kernel("dist") == "hamming_kernel<8>"


# ---- 5. binarize --------------------------------------------------------------------------------------------------------
SPECIAL = np.array([-32768, -1, 0, 1, 32767], np.int16)


def run_binarize(ctx, orc, n, hv_d, seed, corners=False):
    """corners: nothing but the sign test's corners, dim d of row g holds SPECIAL[(d + g) % 5] -- with five rows every corner
    at every dimension, so at every bit position, the last bit of a word and of the row included.  Otherwise random values
    with a corner, in turn, at every third (3 and 5 are coprime to 32: in a longer input they reach every bit position too)"""
    rng = np.random.default_rng(seed)
    if corners:
        hv = SPECIAL[(np.arange(hv_d)[None, :] + np.arange(n)[:, None]) % 5]
    else:
        hv = rng.integers(-32768, 32768, (n, hv_d)).astype(np.int16)
        flat = hv.reshape(-1)
        flat[::3] = SPECIAL[np.arange(flat[::3].size) % 5]
    words = (hv_d + 31) // 32
    g = Guard(4 * n * words)
    ctx.hv_binarize_dev(up(hv).data_ptr(), n, hv_d, g.ptr)
    ctx.sync()
    got = g.host(np.uint32).reshape(n, words)
    want = orc.binarize(hv)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (hv_d, "first differing row", int(bad[0]))
    if hv_d % 32:
        assert (got[:, -1] >> np.uint32(hv_d % 32) == 0).all(), "tail bits of the last word"
    return hv, got


@pytest.mark.parametrize("hv_d", [1, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257])
def test_binarize_word_edges(ctx, orc, hv_d):
    run_binarize(ctx, orc, 5, hv_d, hv_d)
    run_binarize(ctx, orc, 5, hv_d, hv_d, corners=True)


def test_binarize_more_rows_than_a_grid_dimension(ctx, orc):
    """65 537 rows: two full launches of 65 535 rows are not enough"""
    run_binarize(ctx, orc, 65537, 32, 7)


def test_binarize_100_dims_into_the_fp4_search(hg, ctx, orc):
    """the pad bits binarize leaves (zero on both sides) count nothing in the search that reads whole words"""
    R, Q, hv_d = 140, 50, 100
    hv, bits = run_binarize(ctx, orc, R + Q, hv_d, 100)
    hv[R + 3] = hv[7]
    hv[R + 4] = hv[8]
    hv[R + 4, 99] = ~hv[R + 4, 99]  # the last dimension's sign: distance 1
    g = Guard(4 * (R + Q) * 4)
    ctx.hv_binarize_dev(up(hv).data_ptr(), R + Q, hv_d, g.ptr)
    ctx.sync()
    bits = g.host(np.uint32).reshape(R + Q, 4)
    assert np.array_equal(bits, orc.binarize(hv))
    want = orc.hamming_matrix(bits[:R], bits[R:])
    assert want[7, 3] == 0 and want[8, 4] == 1 and want.max() <= hv_d
    ctx.set_debug("ham_path", "fp4")
    for md in (0, 1, int(np.median(want)), hv_d - 1, hv_d):
        search(hg, ctx, up(bits[:R]), R, up(bits[R:]), Q, hv_d, md, want, what=md)
        assert ctx.last_hamming_path() == 2


# ---- 6. the payload decoder -----------------------------------------------------------------------------------------------
def payload_bytes(hg, hv_d, q, lay):
    """the lengths hg_hv_unpack_batch_dev validates"""
    L = hg.lib()
    return int(L.hg_hv_packed_bytes_naive(hv_d, q)) if lay == hg.PAYLOAD_NAIVE else int(L.hg_hv_packed_bytes(hv_d, q)) // 2 * 2


def build_image(payloads, aligns):
    """payloads back to back in one image, payload i at an offset = aligns[i] (mod 4), a junk pattern between them, in front
    (where the alignment asks for it) and behind the last one"""
    parts, offs, pos = [], [], 0
    for p, a in zip(payloads, aligns):
        pad = 1 + (a - pos - 1) % 4 if pos else a
        parts.append((np.arange(pad, dtype=np.uint8) * 37 + 0xEE).astype(np.uint8))
        pos += pad
        assert pos % 4 == a
        offs.append(pos)
        parts.append(p)
        pos += p.size
    parts.append(np.full(8, 0xEE, np.uint8))
    return np.concatenate(parts), offs


def oracle_unpack(hg, orc, payload, hv_d, q, lay):
    if lay == hg.PAYLOAD_NAIVE:
        return orc.unpack_hv_naive(payload.copy().view(np.int16), hv_d, q)
    return orc.unpack_hv(np.concatenate([payload, np.zeros(1, np.uint8)]), hv_d, q)


def run_unpack(hg, ctx, orc, hv_d, cases, seed, front=0, payloads=None, want=None):
    """cases: (q, layout, alignment) per row; random payload bytes unless given; returns (payloads, want)"""
    rng = np.random.default_rng(seed)
    if payloads is None:
        payloads = [rng.integers(0, 256, payload_bytes(hg, hv_d, q, lay)).astype(np.uint8) for q, lay, _ in cases]
        want = [oracle_unpack(hg, orc, p, hv_d, q, lay) for p, (q, lay, _) in zip(payloads, cases)]
    img, offs = build_image(payloads, [a for _, _, a in cases])
    d_img = up(img)
    n = len(cases)
    g = Guard(2 * n * hv_d, front=front)
    ctx.hv_unpack_batch_dev(d_img.data_ptr(), img.size, offs, [c[0] for c in cases], [c[1] for c in cases], hv_d, g.ptr)
    ctx.sync()
    got = g.host(np.int16).reshape(n, hv_d)
    for i, (q, lay, a) in enumerate(cases):
        bad = np.nonzero(got[i] != want[i])[0]
        assert bad.size == 0, ("hv_d, q, layout, alignment", hv_d, q, lay, a, "first differing dim", int(bad[0]),
                               int(got[i][bad[0]]), int(want[i][bad[0]]))
    return payloads, want


def all_cases(hg, aligns):
    return [(q, lay, a if a is not None else (q + 2 * lay) % 4) for q in range(1, 17)
            for lay in (hg.PAYLOAD_BITPACKER8X, hg.PAYLOAD_NAIVE) for a in aligns]


# 8 and 248: no whole BitPacker8x block; 100 and 4100: hv_d % 8 != 0, the direct decoder; 256 / 264 / 1000: one block, one and a
# tail, three and a tail; every width 1..16 in both layouts at every alignment
@pytest.mark.parametrize("hv_d", [8, 100, 248, 256, 264, 1000, 4100])
def test_unpack_every_width_layout_and_alignment(hg, ctx, orc, hv_d):
    run_unpack(hg, ctx, orc, hv_d, all_cases(hg, (0, 1, 2, 3)), seed=hv_d)


def test_unpack_32768_dims_staged_and_direct_in_one_call(hg, ctx, orc):
    """the stage holds 32 KiB: q <= 8 decode from LDS, q >= 9 directly from the image, in one launch (every alignment occurs)"""
    cases = all_cases(hg, (None,))
    assert {c[2] for c in cases} == {0, 1, 2, 3}
    run_unpack(hg, ctx, orc, 32768, cases, seed=32768)


def test_unpack_into_rows_that_are_not_16_byte_aligned(hg, ctx, orc):
    """the same hv_d = 4096 batch into an aligned matrix (staged) and into one shifted by two bytes: every row is misaligned,
    the direct decoder runs, the integers are the same and the bytes in front of the matrix stay"""
    cases = all_cases(hg, (None,))
    payloads, want = run_unpack(hg, ctx, orc, 4096, cases, seed=4096)
    run_unpack(hg, ctx, orc, 4096, cases, seed=4096, front=16 + 2, payloads=payloads, want=want)


@pytest.mark.parametrize("hv_d", [100, 264])
def test_unpack_against_the_python_integer_models(hg, ctx, orc, hv_d):
    """payloads written by the bit-by-bit Python models of both layouts (payload_models.py) from known values: the decoder
    returns those values -- with the layouts' own corners: dimensions behind the last whole BitPacker8x block are -2^(q-1);
    the naive layout returns -2^(q-1) as +2^(q-1) and, at q = 16, every value but -32768 one lower"""
    rng = np.random.default_rng(hv_d)
    cases, payloads, want = [], [], []
    for q in (1, 5, 9, 16):
        lim = 1 << (q - 1)
        # (q = 16: values below zero only -- the sum with the i16 offset is then non-negative and does not spill into the
        # neighbouring field, so the block decodes to the values it was packed from)
        hv = rng.integers(-lim, 0 if q == 16 else lim, hv_d).astype(np.int16)
        hv[:2] = [-lim, -1 if q == 16 else lim - 1]
        off = -32768 if q == 16 else lim
        whole = hv_d // 256 * 256
        body = b"".join(bp8x_model([(((int(x) + off + 32768) % 65536) - 32768) & 0xFFFFFFFF for x in hv[b:b + 256]], q)
                        for b in range(0, whole, 256))
        p = np.zeros(payload_bytes(hg, hv_d, q, hg.PAYLOAD_BITPACKER8X), np.uint8)
        p[:len(body)] = np.frombuffer(body, np.uint8)
        w = hv.copy()
        w[whole:] = -32768 if q == 16 else -lim
        cases.append((q, hg.PAYLOAD_BITPACKER8X, q % 4)), payloads.append(p), want.append(w)
        hv = rng.integers(-lim, lim, hv_d).astype(np.int16)
        hv[:3] = [-lim, lim - 1, -1]
        p = naive_model(hv, q).view(np.uint8)
        assert p.size == payload_bytes(hg, hv_d, q, hg.PAYLOAD_NAIVE)
        if q < 16:
            w = hv.astype(np.int32)
            w[w == -lim] = lim
            w = w.astype(np.int16)
        else:
            w = np.where(hv == -32768, hv, (hv.astype(np.int32) - 1).astype(np.int16))
        cases.append((q, hg.PAYLOAD_NAIVE, (q + 1) % 4)), payloads.append(p), want.append(w)
    for p, w, (q, lay, _) in zip(payloads, want, cases):  # the oracle agrees with the models
        assert np.array_equal(oracle_unpack(hg, orc, p, hv_d, q, lay), w), (q, lay)
    run_unpack(hg, ctx, orc, hv_d, cases, seed=0, payloads=payloads, want=want)


def test_unpack_refuses_bad_widths_layouts_and_lengths(hg, ctx):
    """checked on the host before the launch: q = 0 / 17, a third layout, a payload whose validated length ends one byte
    behind the image; nothing is written"""
    hv_d = 256
    img = up(np.zeros(32 * 16 + 2, np.uint8))
    g = Guard(2 * hv_d)
    for q, lay, off, size in ((0, 0, 0, 514), (17, 0, 0, 514), (9, 2, 0, 514), (16, 0, 1, 512), (16, 1, 0, 513), (9, 0, 515, 514)):
        with pytest.raises(hg.HgError) as e:
            ctx.hv_unpack_batch_dev(img.data_ptr(), size, [off], [q], [lay], hv_d, g.ptr)
        assert e.value.status == hg.ERR_INVALID, (q, lay, off, size)
    ctx.sync()
    assert (g.host() == SENT).all()


# ---- 7. 2-bit blobs: bytes with bit 7 set -------------------------------------------------------------------------------------
def high_bit_seq(rng, L):
    """bases, u / U and N with and without bit 7 (0xD5 / 0xF5 differ from 'U' / 'u' in that bit only), and bytes 0x80..0xFF"""
    base = np.frombuffer(b"ACGTacgtUuN", np.uint8)
    s = rng.choice(np.concatenate([base, base | 0x80]), L)
    hi = rng.random(L) < 0.3
    s[hi] = rng.integers(0x80, 0x100, int(hi.sum())).astype(np.uint8)
    s[:4] = [ord("U"), 0xD5, ord("u"), 0xF5]
    s[-2:] = [0xF5, ord("U")]
    return s


def run_pack2(hg, ctx, seqs, norm):
    offs, total = [], 0
    for s in seqs:
        offs.append(total)
        total += (len(s) + 3) // 4 * 4
    host = np.full(total + 64, 0xFF, np.uint8)  # (what lies behind a sequence is not a base either way)
    for o, s in zip(offs, seqs):
        host[o:o + len(s)] = s
    sizes = [int(hg.lib().hg_pack2_size(len(s))) for s in seqs]
    boffs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    g = Guard(sum(sizes))
    ctx.pack2_batch_dev(up(host).data_ptr(), np.array(offs, np.uint64), np.array([len(s) for s in seqs], np.uint64), g.ptr, boffs, norm)
    ctx.sync()
    got = g.host()
    for s, o, z in zip(seqs, boffs, sizes):
        assert np.array_equal(got[int(o):int(o) + z], hg.pack2(s, norm)), (len(s), norm)


def run_unpack2(hg, ctx, s, norm):
    L = s.size
    ok = np.isin(s, np.frombuffer(b"ACGTacgtUu" if norm == hg.NORM_U2T else b"ACGTacgt", np.uint8))
    up_ = s & 0xDF
    want = np.where(ok, np.where(up_ == ord("U"), ord("T"), up_), ord("N")).astype(np.uint8)
    g = Guard((L + 15) // 16 * 16)
    ctx.unpack2_dev(up(hg.pack2(s, norm)).data_ptr(), L, g.ptr)
    ctx.sync()
    assert np.array_equal(g.host()[:L], want), (L, norm)


@pytest.mark.parametrize("norm", [0, 1])
def test_pack2_and_unpack2_of_bytes_with_bit_7_set(hg, ctx, norm):
    rng = np.random.default_rng(80 + norm)
    seqs = [high_bit_seq(rng, L) for L in (31, 32, 33)] + [rng.integers(0x80, 0x100, L).astype(np.uint8) for L in (31, 32, 33)]
    run_pack2(hg, ctx, seqs, norm)
    for s in seqs:
        run_unpack2(hg, ctx, s, norm)


# ---- 8. the synthetic genomes, byte for byte ---------------------------------------------------------------------------------
def run_synth(ctx, orc, first, n, L, ppm, gap):
    stride = L + 1 + gap
    g = Guard(n * stride)
    ctx.synth_genomes_dev(first, n, L, stride, g.ptr, cluster_size=100, sub_ppm_per_member=ppm)
    ctx.sync()
    got = g.host().reshape(n, stride)
    for i in range(n):
        want = orc.synth_genome(first + i, L, 100, ppm)
        assert want.size == L + 1 and np.array_equal(got[i, :L + 1], want), (first + i, L, ppm)
    assert (got[:, L + 1:] == SENT).all(), "the gap between two genomes was written"


@pytest.mark.parametrize("ppm", [0, 1000, 1_000_000])
def test_synth_equals_the_oracle_byte_for_byte(ctx, orc, ppm):
    """first = 0: member 0 of a cluster has no substitutions; 99 / 100: a cluster's last member and the next cluster's root;
    L around one thread's 32 bases and one workgroup's 8 192; a stride larger than L + 1"""
    for first in (0, 99, 100, 12345):
        for L in (0, 1, 31, 32, 33, 8191, 8193):
            run_synth(ctx, orc, first, 3, L, ppm, gap=13 if L % 2 else 64)
    if ppm:  # (the cases are not vacuous: members differ from their root, member 0 is the root)
        a, b = orc.synth_genome(100, 8193, 100, ppm), orc.synth_genome(101, 8193, 100, ppm)
        assert (a != b).any() and np.array_equal(a, orc.synth_genome(100, 8193, 100, 0))


# ---- 9. the byte-operand workspaces, shared by dist and the Hamming search ------------------------------------------------
def test_dist_i8_and_hamming_fp4_interleaved_on_one_context(hg, ctx, orc):
    """hg_run_hamming_mfma expands into the workspaces the dist i8 path keeps its operand copies in and forgets that path's
    marks: a dist call repeated on the same buffers after a search must prepare its operands again (and equal its first
    result and the oracle), and so must the search after it"""
    rng = np.random.default_rng(79)
    D, R = 4096, 700
    base = rng.binomial(2000, 0.5, (5, D))
    cnt = base[rng.integers(0, 5, R)] + rng.binomial(3333 - 1999, 0.5, (R, D))  # sketch-like: hv = 2 * count - n, shared parts
    hv = (2 * cnt - 3333).astype(np.int16)
    rn = np.array([orc.hv_norm2(x) for x in hv], np.int32)
    ani = orc.ani_matrix(hv, rn, hv, rn, 21)
    sel = np.triu(ani >= np.float32(70.0), 1)
    wi, wj = np.nonzero(sel)
    assert wi.size > 100
    d_hv, d_rn = up(hv), up(rn)
    hR, hQ, hd = 300, 270, 1024
    rb, qb = bit_rows(hR, hQ, hd, 9)
    hwant = orc.hamming_matrix(rb, qb)
    hmd = int(np.percentile(hwant, 3))
    d_rb, d_qb = up(rb), up(qb)

    def dist():
        cap = wi.size + 16
        g = Guard(12 * cap)
        ctx.set_debug("dist_path", "i8")
        n, st = ctx.dist_dev(d_hv.data_ptr(), d_rn.data_ptr(), R, d_hv.data_ptr(), d_rn.data_ptr(), R, D, 21, True, 70.0, g.ptr, cap)
        ctx.set_debug("dist_path", "")
        assert st == hg.OK and ctx.last_dist_path() == 1
        raw = g.host()
        assert n == wi.size and (raw[12 * n:] == SENT).all()
        h = raw[:12 * n].view(hg.ANI_HIT_DTYPE)
        order = np.argsort(h["ref_idx"].astype(np.int64) * R + h["qry_idx"])
        h = h[order]
        assert np.array_equal(h["ref_idx"], wi) and np.array_equal(h["qry_idx"], wj)
        assert np.array_equal(h["ani"].view(np.uint32), ani[wi, wj].view(np.uint32))
        return h

    def ham():
        ctx.set_debug("ham_path", "fp4")
        cap = hR * hQ
        g = Guard(12 * (cap + 8))
        n, st = ctx.hamming_search_dev(d_rb.data_ptr(), hR, d_qb.data_ptr(), hQ, hd, hmd, g.ptr, cap)
        ctx.set_debug("ham_path", "")
        assert ctx.last_hamming_path() == 2
        check_hits(hg, g, n, st, hwant, hmd, cap)
        rec = g.host(np.uint32).reshape(-1, 3)[:n]
        return rec[np.lexsort((rec[:, 1], rec[:, 0]))]

    d1, h1, d2, h2 = dist(), ham(), dist(), ham()
    assert np.array_equal(d1, d2) and np.array_equal(h1, h2) and h1.shape[0] > 100
