"""One multi-FASTA text split into its records on the GPU (libhypergen_rec.so, include/hypergen_rec.h): hg_rec_count_dev and
hg_rec_split_dev against tests/rec_ref.py on the texts of tests/rec_cases.py, all comparisons `==`.  Every split compares the
record table and the WHOLE output buffer -- sequences, 'N' pads, and a sentinel behind seq_bytes and behind the capacities --
and every text lies on the device with '>' and LF bytes behind its last byte, which must be ignored.  Then the invariant
against hg_read_merge_seq, the capacities, the per-record sketches against hg_sketch_batch, and the census."""
import gzip

import numpy as np
import pytest
import torch

import rec_cases
import rec_census
import rec_ref

pytestmark = pytest.mark.gpu

FILL = 0xEE
HV_D = 1024
BASES = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_rec()
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    with hg.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def cases(hg):
    """name -> (text, the reference's (table, buffer) or None for sequence data before the first header), computed once"""
    out = {}
    for name, text in rec_cases.cases(hg.rec_block_bytes()):
        out[name] = (text, reference(text))
    return out


def reference(text):
    try:
        return rec_ref.layout(rec_ref.split(text))
    except rec_ref.SequenceBeforeHeader:
        return None


def upload(text, behind=b"\n>"):
    """the text on the device, readable up to n rounded up to 16 and a little further; `behind` repeats from byte n on"""
    n = len(text)
    size = (n + 15) // 16 * 16 + 16
    host = np.frombuffer((behind * (size // len(behind) + 1))[:size], np.uint8).copy()
    host[:n] = np.frombuffer(text, np.uint8)
    t = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    return t


def split_on_device(hg, ctx, text, seq_cap=None, rec_cap=None, behind=b"\n>"):
    """hg_rec_count_dev, then hg_rec_split_dev into buffers with 64 sentinel bytes / 2 sentinel entries behind the capacities
    (default: exactly what the count asks for): (status, n_recs, seq_bytes, table incl. sentinels, buffer incl. sentinels)"""
    d_text = upload(text, behind)
    st, n_recs, seq_bytes = ctx.rec_count_dev(d_text.data_ptr(), len(text))
    if st != hg.OK:
        assert (n_recs, seq_bytes) == (0, 0)
    seq_cap = seq_bytes + 32 if seq_cap is None else seq_cap
    rec_cap = n_recs if rec_cap is None else rec_cap
    d_seq = torch.full((seq_cap + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    d_recs = torch.full(((rec_cap + 2) * 32,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st2, n_recs2, seq_bytes2 = ctx.rec_split_dev(d_text.data_ptr(), len(text), d_seq.data_ptr(), seq_cap, d_recs.data_ptr(), rec_cap)
    ctx.sync()
    if st != hg.OK:
        assert st2 == st  # the error comes from both calls
    else:
        assert (n_recs2, seq_bytes2) == (n_recs, seq_bytes)  # (also with HG_ERR_CAPACITY: the needed sizes)
    return st2, n_recs2, seq_bytes2, d_recs.cpu().numpy().view(hg.REC_DTYPE), d_seq.cpu().numpy()


def check(hg, ctx, text, want, name=""):
    st, n_recs, seq_bytes, recs, seq = split_on_device(hg, ctx, text)
    if want is None:
        assert st == hg.ERR_IO, name
        assert (recs.view(np.uint8) == FILL).all() and (seq == FILL).all(), name
        return
    table, buf = want
    assert (st, n_recs, seq_bytes) == (hg.OK, table.size, buf.size), name
    assert (recs[:n_recs] == table).all(), name
    assert (recs[n_recs:].view(np.uint8) == FILL).all(), name
    assert (seq[:seq_bytes] == buf).all(), name
    assert (seq[seq_bytes:] == FILL).all(), name  # bytes from seq_bytes on are not written


def check_named(hg, ctx, cases, prefixes):
    names = [n for n in cases if n.startswith(prefixes)]
    assert names
    for name in names:
        check(hg, ctx, *cases[name], name)
    return names


# ---- 1 .. 8: the cases ---------------------------------------------------------------------------------------------------------

def test_anchor(hg, ctx, cases):
    text, want = cases["anchor"]
    assert want[0]["seq_len"].tolist() == [18, 6, 9] and want[1].tobytes() == b"ACGTACGTACGGTTAACCNNTTTTACNNGATTACAGANNN"
    check(hg, ctx, text, want, "anchor")


def test_motif_slid_over_a_block_boundary(hg, ctx, cases):
    B = hg.rec_block_bytes()
    names = check_named(hg, ctx, cases, ("motif_", "gt_inside_line_at", "gt_behind_lf_at"))
    assert len(names) == len(rec_cases.MOTIF) + 1 + 2
    last_first = {(cases[n][0][B - 1:B], cases[n][0][B:B + 1]) for n in names}
    assert {(b"\r", b"\n"), (b"\n", b">"), (b"A", b">"), (b">", b"i")} <= last_first
    # the '>' at the start of a block is a sequence byte in one text and a header in the other
    assert cases["gt_inside_line_at_block_start"][1][0].size == 3 and cases["gt_behind_lf_at_block_start"][1][0].size == 2


def test_long_lines(hg, ctx, cases):
    B = hg.rec_block_bytes()
    check_named(hg, ctx, cases, ("header_", "sequence_3B"))
    assert cases["header_2p5B_blank"][1][0]["id_len"].tolist() == [1, 2 * B, 1]
    assert cases["header_2p5B_no_blank"][1][0]["hdr_len"].tolist() == [5 * B // 2 + 1, 2]
    assert cases["header_2p5B_unterminated"][1][0]["id_len"].tolist() == [1, 5 * B // 2]
    assert cases["sequence_3B_plus_1_unterminated"][1][0]["seq_len"].tolist() == [3 * B + 1]


def test_dense_tiny_records(hg, ctx, cases):
    B = hg.rec_block_bytes()
    check_named(hg, ctx, cases, ("dense_",))
    assert cases["dense_a"][1][0].size > 256 * 3 and cases["dense_empty"][1][0].size == B  # more headers per block than lanes
    assert not cases["dense_empty"][1][0]["id_len"].any() and cases["dense_empty"][1][1].size == 0


def test_record_lengths_0_to_9(hg, ctx, cases):
    check_named(hg, ctx, cases, ("lengths_",))
    assert cases["lengths_0_to_9"][1][0]["seq_off"].tolist() == [0, 0, 4, 8, 12, 16, 24, 32, 40, 48]


def test_ends_of_text(hg, ctx, cases):
    B = hg.rec_block_bytes()
    names = check_named(hg, ctx, cases, ("no_final_lf", "final_", "cr_inside", "empty", "lfs_only", "one_header_byte", "n_"))
    assert {len(cases[n][0]) for n in names} >= {0, 1, 7, B - 1, B, B + 1}
    for name in ("empty", "lfs_only"):
        assert split_on_device(hg, ctx, cases[name][0])[:3] == (hg.OK, 0, 0)


def test_bytes_behind_n_are_ignored(hg, ctx, cases):
    B = hg.rec_block_bytes()
    base = rec_cases.filler(B - 20) + b"\n>r\nAC\n>s t\nACGTACGTACGTACGTACGTACGTACG"
    for cut in range(16):  # every residue of n modulo 16, in the second block
        text = base[:len(base) - cut]
        want = reference(text)
        for behind in (b"\n>x\nACGT\n", b">", b"\n", b"\r\n>", b"A"):
            st, n_recs, seq_bytes, recs, seq = split_on_device(hg, ctx, text, behind=behind)
            assert (st, n_recs, seq_bytes) == (hg.OK, want[0].size, want[1].size), (cut, behind)
            assert (recs[:n_recs] == want[0]).all() and (seq[:seq_bytes] == want[1]).all() and (seq[seq_bytes:] == FILL).all(), (cut, behind)


def test_in_front_of_the_first_header(hg, ctx, cases):
    errors = ("sequence_before_header", "fastq", "blank_before_header", "cr_content_before_header", "only_sequence",
              "sequence_a_block_before_header", "gt_inside_first_line")
    fine = ("empty_lines_before_header", "empty_lines_a_block_before_header")
    for name in errors:
        assert cases[name][1] is None, name
        check(hg, ctx, *cases[name], name)
    for name in fine:
        assert cases[name][1] is not None and cases[name][1][0].size == 1, name
        check(hg, ctx, *cases[name], name)


def test_more_blocks_than_one_scan_tile(hg, ctx):
    """a text of more than 1024 blocks: the prefix of a block then comes from the tiles in front of its own"""
    B = hg.rec_block_bytes()
    rng = np.random.default_rng(5)
    parts = []
    for r in range(90):
        seq = rng.choice(BASES, int(rng.integers(1000, 100_000))).tobytes()
        parts.append(b">contig_%d length=%d\n" % (r, len(seq)) + b"\n".join(seq[j:j + 80] for j in range(0, len(seq), 80)) + b"\n")
    text = b"".join(parts)
    assert 1024 * B < len(text) < 3 * 1024 * B
    check(hg, ctx, text, reference(text), "two tiles")


# ---- 9: capacities -------------------------------------------------------------------------------------------------------------

def test_capacity_one_too_small(hg, ctx, cases):
    text, (table, buf) = cases["lengths_0_to_9"]
    for seq_cap, rec_cap in ((buf.size + 31, table.size), (buf.size + 32, table.size - 1), (buf.size + 31, table.size - 1)):
        st, n_recs, seq_bytes, recs, seq = split_on_device(hg, ctx, text, seq_cap=seq_cap, rec_cap=rec_cap)
        assert (st, n_recs, seq_bytes) == (hg.ERR_CAPACITY, table.size, buf.size)
        # nothing is written beyond the capacities
        assert (seq[seq_cap:] == FILL).all() and (recs[rec_cap:].view(np.uint8) == FILL).all()
    st, n_recs, seq_bytes, recs, seq = split_on_device(hg, ctx, text, seq_cap=buf.size + 32, rec_cap=table.size)
    assert st == hg.OK and (seq[:buf.size] == buf).all() and (seq[buf.size:] == FILL).all() and (recs[:n_recs] == table).all()


def test_host_form_and_its_capacities(hg, ctx, cases):
    for name in ("anchor", "dense_mixed", "final_header_with_cr", "motif_12"):
        text, (table, buf) = cases[name]
        st, n_recs, seq_bytes, recs, seq = ctx.rec_split(text, fill=FILL)
        assert (st, n_recs, seq_bytes) == (hg.OK, table.size, buf.size), name
        assert (recs == table).all() and (seq[:buf.size] == buf).all() and (seq[buf.size:] == FILL).all(), name
    text, (table, buf) = cases["anchor"]
    st, n_recs, seq_bytes, recs, seq = ctx.rec_split(text, seq_cap=buf.size + 31, rec_cap=table.size, fill=FILL)
    assert (st, n_recs, seq_bytes) == (hg.ERR_CAPACITY, table.size, buf.size) and (seq == FILL).all()
    assert ctx.rec_split(cases["fastq"][0])[0] == hg.ERR_IO
    assert "sequence data before the first header" in hg.lib().hg_last_error(ctx._h).decode()
    assert ctx.rec_split(b"")[:3] == (hg.OK, 0, 0)


# ---- 10: fuzz ------------------------------------------------------------------------------------------------------------------

def test_seeded_fuzz(hg, ctx):
    texts = rec_cases.fuzz_texts(hg.rec_block_bytes())
    assert len(texts) == 200
    errors = 0
    for i, text in enumerate(texts):
        want = reference(text)
        errors += want is None
        check(hg, ctx, text, want, "fuzz %d" % i)
    assert 10 < errors < 100


# ---- 11: the invariant ---------------------------------------------------------------------------------------------------------

def test_records_joined_with_n_are_what_read_merge_seq_returns(hg, ctx, cases, tmp_path):
    checked = 0
    for name, (text, want) in cases.items():
        if want is None or not name.startswith(("anchor", "motif_1", "dense_mixed", "final_", "cr_inside", "lengths_", "no_final")):
            continue
        st, n_recs, seq_bytes, recs, seq = split_on_device(hg, ctx, text)
        path = tmp_path / "t.fna"
        path.write_bytes(text)
        joined = b"".join(b"N" + seq[int(r["seq_off"]):int(r["seq_off"] + r["seq_len"])].tobytes() for r in recs[:n_recs])
        assert joined == hg.read_merge_seq(str(path)).tobytes(), name
        checked += 1
    assert checked >= 15
    # ... and a gzip file, through the library's reader
    text = cases["anchor"][0] * 50
    path = tmp_path / "t.fna.gz"
    path.write_bytes(gzip.compress(text))
    assert hg.rec_read_text(str(path)) == text
    plain = tmp_path / "p.fna"
    plain.write_bytes(text)
    assert hg.rec_read_text(str(plain)) == text
    st, n_recs, seq_bytes, recs, seq = split_on_device(hg, ctx, hg.rec_read_text(str(path)))
    joined = b"".join(b"N" + seq[int(r["seq_off"]):int(r["seq_off"] + r["seq_len"])].tobytes() for r in recs[:n_recs])
    assert n_recs == 150 and joined == hg.read_merge_seq(str(path)).tobytes()
    with pytest.raises(hg.HgError):
        hg.rec_read_text(str(tmp_path / "missing.fna"))


# ---- 12: end to end ------------------------------------------------------------------------------------------------------------

def wrapped(records, width=60, eol=b"\n"):
    out = []
    for i, r in enumerate(records):
        out.append(b">rec%d description %d" % (i, i))
        out += [bytes(r[j:j + width]) for j in range(0, len(r), width)]
    return eol.join(out) + eol


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(12)
    g = [rng.choice(BASES, n) for n in (3000, 20, 5000, 0, 21, 1500)]  # one shorter than k, one empty, one of exactly k
    g[2][2500:3500] = g[2][500:1500]  # a repeat: k-mers that occur twice
    g[0][100] = ord("N")
    g[5][::7] |= 0x20
    return [x.tobytes() for x in g]


@pytest.mark.parametrize("canonical,min_count,eol", [(1, 1, b"\n"), (0, 1, b"\r\n"), (1, 2, b"\n")])
def test_per_record_sketches_equal_the_batch_sketch_of_the_sequences(hg, ctx, genomes, canonical, min_count, eol):
    text = wrapped(genomes, eol=eol)
    seqs = [r.seq for r in rec_ref.split(text)]
    assert seqs == genomes
    p = hg.default_params(ksize=21, scaled=50, canonical=canonical, hv_d=HV_D, min_count=min_count)
    want_hv, want_n2, want_nh = ctx.sketch_batch(seqs, p)
    assert want_nh[1] == 0 and want_nh[3] == 0 and (want_nh[0] > 20 or min_count == 2)
    if min_count == 2:
        assert 0 < want_nh[2] < 40 and want_nh[0] == 0  # only the repeat survives the filter
    d_text = upload(text)
    recs, which, hv, n2, nh = ctx.rec_sketch_text_dev(d_text.data_ptr(), len(text), p)
    assert (recs == rec_ref.layout(rec_ref.split(text))[0]).all()
    assert which.tolist() == list(range(6))
    assert nh.tolist() == want_nh.tolist() and (n2 == want_n2).all() and (hv == want_hv).all()
    # --min_length: decided from the table, the rows of the others are the same rows
    recs, which, hv, n2, nh = ctx.rec_sketch_text_dev(d_text.data_ptr(), len(text), p, min_length=21)
    assert recs.size == 6 and which.tolist() == [0, 2, 4, 5]
    assert nh.tolist() == want_nh[which].tolist() and (n2 == want_n2[which]).all() and (hv == want_hv[which]).all()


def test_per_record_sketches_of_texts_without_records(hg, ctx):
    p = hg.default_params(ksize=21, scaled=50, hv_d=HV_D)
    for text in (b"", b"\n\n"):
        d_text = upload(text)
        recs, which, hv, n2, nh = ctx.rec_sketch_text_dev(d_text.data_ptr(), len(text), p)
        assert recs.size == 0 and which.size == 0 and hv.shape == (0, HV_D)
    d_text = upload(b"ACGT\n>a\nAC\n")
    with pytest.raises(hg.HgError) as e:
        ctx.rec_sketch_text_dev(d_text.data_ptr(), 11, p)
    assert e.value.status == hg.ERR_IO


# ---- 13: the census ------------------------------------------------------------------------------------------------------------

def test_every_kernel_of_the_census_is_launched_by_a_split(hg, ctx, cases):
    assert [r.name for r in rec_census.ROWS] == hg.rec_kernel_names()
    before = hg.rec_launch_counts()
    d_text = upload(cases["anchor"][0])
    assert ctx.rec_count_dev(d_text.data_ptr(), len(cases["anchor"][0]))[0] == hg.OK
    counted = hg.rec_launch_counts()
    for row in rec_census.ROWS:
        assert counted[row.name] - before[row.name] == (1 if "hg_rec_count_dev" in row.entries else 0), row.name
    check(hg, ctx, *cases["anchor"], "anchor")  # (a count and a split)
    after = hg.rec_launch_counts()
    for row in rec_census.ROWS:
        assert after[row.name] - counted[row.name] == (2 if "hg_rec_count_dev" in row.entries else 1), row.name
