"""`hyper-gen sketch --fragment` and `hyper-gen dist --fragments` end to end.  Seeded genomes: A of 120 kbp; B = A with 3 %
substitutions and its middle 40 % replaced by random sequence; C and D unrelated.  The reference side (A, D) is cut into windows
of 4 000 every 2 000, the query side (B, C) into fragments of 2 000; k = 21 and -s 20, about 100 hashes per fragment.  The TSV
and the --fragment_hits file equal, byte for byte, what tests/frag_ref.py makes of the CPU oracle's sketches of the same windows
under the containment formula of tests/containment_ref.py.

The seed (SEED = 2026) is chosen so that the oracle alone, on the CPU, satisfies the conditions on the input -- every B
fragment wholly inside the replaced region is unmatched against A, every B fragment wholly inside the kept region and at
least one window length from its edges is matched against A, C matches nothing, nothing matches D: the first test checks
that without a device."""
import os
import subprocess

import numpy as np
import pytest

import containment_ref as cr
import frag_ref

SEED = 2026
LEN, W_REF, S_REF, W_QRY = 120_000, 4000, 2000, 2000
KSIZE, SCALED, HV_D = 21, 20, 4096
FRAG_TH, ANI_TH = 90.0, 85.0
REPLACED = (36_000, 84_000)  # of B, in bases of the genome: the middle 40 %
BASES = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_frag()
    return hypergen_amd


def genomes(seed=SEED):
    rng = np.random.default_rng(seed)
    a = rng.choice(BASES, LEN)
    b = a.copy()
    sub = rng.random(LEN) < 0.03
    b[sub] = BASES[(np.searchsorted(BASES, b[sub]) + rng.integers(1, 4, int(sub.sum()))) % 4]  # always another base
    b[REPLACED[0]:REPLACED[1]] = rng.choice(BASES, REPLACED[1] - REPLACED[0])
    return {"a": a, "b": b, "c": rng.choice(BASES, LEN), "d": rng.choice(BASES, LEN)}


def fasta(name, seq, width=80):
    s = seq.tobytes()
    return b"\n".join([b">" + name.encode()] + [s[j:j + width] for j in range(0, len(s), width)]) + b"\n"


def oracle_side(orc, paths, texts, window, step):
    """(record names, hv, norm2) of one side as `sketch --fragment` must write it: the windows of every file's merged sequence"""
    names, hv, n2 = [], [], []
    for path, text in zip(paths, texts):
        seq = orc.read_needletail(text)
        for start, n in frag_ref.plan(seq.size, window, step):
            h, norm2, _ = orc.sketch_genome(seq[start:start + n], ksize=KSIZE, scaled=SCALED, norm=orc.NORM_U2T, hv_d=HV_D)
            names.append("%s:%d-%d" % (path, start + 1, start + n)), hv.append(h), n2.append(norm2)
    return names, np.stack(hv), np.array(n2, np.int32)


def oracle_expect(orc, ref, qry, frag_th=FRAG_TH, ani_th=ANI_TH):
    """(tsv, hits file, pair records, best records, reference genomes, query genomes) from two oracle_side() results"""
    (rn, rh, r2), (qn, qh, q2) = ref, qry
    ani = cr.ani_ref(orc, cr.exact_dots(rh, qh), r2[:, None], q2[None, :], KSIZE, cr.CONTAINMENT)
    rf, rg = frag_ref.genomes(rn)
    qf, qg = frag_ref.genomes(qn)
    pair, best = frag_ref.reduce(ani, rf, qf, frag_th)
    return frag_ref.tsv(pair, rg, qg, ani_th), frag_ref.hits(best, rn, qn, frag_th), pair, best, rg, qg


@pytest.fixture(scope="module")
def sides(orc, tmp_path_factory):
    """the two directories and the oracle's records for them, computed once"""
    root = tmp_path_factory.mktemp("fragments")
    g = genomes()
    out = {}
    for side, members in (("ref", "ad"), ("qry", "bc")):
        d = root / side
        d.mkdir()
        paths, texts = [], []
        for m in members:
            texts.append(fasta("genome_" + m, g[m]))
            paths.append(str(d / (m + ".fna")))
            (d / (m + ".fna")).write_bytes(texts[-1])
        out[side] = (d, oracle_side(orc, paths, texts, *((W_REF, S_REF) if side == "ref" else (W_QRY, W_QRY))))
    return root, out


def test_the_oracle_alone_satisfies_the_conditions_on_the_input(orc, sides):
    _, out = sides
    tsv, hits, pair, best, rg, qg = oracle_expect(orc, out["ref"][1], out["qry"][1])
    assert [os.path.basename(x) for x in rg] == ["a.fna", "d.fna"] and [os.path.basename(x) for x in qg] == ["b.fna", "c.fna"]
    n_frag = len(frag_ref.plan(LEN + 1, W_QRY, W_QRY))  # (the merged sequence starts with the record's 'N')
    assert pair["total"].tolist() == [[n_frag, n_frag]] * 2 and n_frag == 60
    m_th = frag_ref.threshold(FRAG_TH)
    b_vs_a = best["m"][0, :n_frag] >= m_th
    lo, hi = REPLACED[0] + 1, REPLACED[1] + 1  # the replaced region in the merged sequence
    starts = np.arange(n_frag) * W_QRY
    inside = (starts >= lo) & (starts + W_QRY <= hi)
    kept = (starts + W_QRY <= lo - W_REF) | (starts >= hi + W_REF)
    assert inside.sum() == 23 and kept.sum() >= 30
    assert not b_vs_a[inside].any() and b_vs_a[kept].all()
    assert (best["m"][:, n_frag:] < m_th).all() and (best["m"][1] < m_th).all()  # C matches nothing, nothing matches D
    assert pair["matched"].tolist() == [[int(b_vs_a.sum()), 0], [0, 0]] and 30 <= int(b_vs_a.sum()) <= n_frag - 23
    assert tsv.count("\n") == 1 and tsv.split("\t")[2].startswith("9") and hits.count("\n") == int(b_vs_a.sum())
    # the noise floor of the issue, as this input shows it: the best unrelated window stays well below the threshold
    print("largest unrelated best: %.3f, lowest matched best: %.3f" % (max(best["m"][1].max(), best["m"][0, n_frag:].max()) / 1000,
                                                                     best["m"][0, :n_frag][b_vs_a].min() / 1000))


def cli(hg, *args):
    r = subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def sketched(hg, sides):
    root, out = sides
    log_r = cli(hg, "sketch", "-p", str(out["ref"][0]), "-o", str(root / "ref.sketch"), "-s", str(SCALED), "-t", "2", "--fragment", str(W_REF),
                "--fragment_step", str(S_REF))
    log_q = cli(hg, "sketch", "-p", str(out["qry"][0]), "-o", str(root / "qry.sketch"), "-s", str(SCALED), "-t", "2", "--fragment=%d" % W_QRY)
    return root, log_r, log_q


@pytest.mark.gpu
def test_sketch_fragment_writes_the_oracles_windows(hg, sides, sketched):
    root, log_r, log_q = sketched
    _, out = sides
    assert "Sketching 120 windows of 2 files took" in log_r and "Sketching 120 windows of 2 files took" in log_q
    for side in ("ref", "qry"):
        names, hv, n2 = out[side][1]
        recs = hg.read_sketch_file(str(root / (side + ".sketch")))
        assert [r["file_str"] for r in recs] == names
        assert [r["hv_norm_2"] for r in recs] == n2.tolist()
        assert all((r["ksize"], r["scaled"], r["hv_d"], r["canonical"]) == (KSIZE, SCALED, HV_D, True) for r in recs)
        for r, h in zip(recs, hv):
            assert (hg.hv_unpack(r["hv"].view(np.uint8), HV_D, r["hv_quant_bits"]) == h).all()


@pytest.mark.gpu
def test_dist_fragments_equals_the_reference_byte_for_byte(hg, orc, sides, sketched, tmp_path):
    root, _, _ = sketched
    _, out = sides
    want_tsv, want_hits, pair, _, _, _ = oracle_expect(orc, out["ref"][1], out["qry"][1])
    log = cli(hg, "dist", "--fragments", "-r", str(root / "ref.sketch"), "-q", str(root / "qry.sketch"), "-o", str(tmp_path / "f.tsv"),
              "--fragment_hits", str(tmp_path / "hits.tsv"))
    assert (tmp_path / "f.tsv").read_text() == want_tsv and (tmp_path / "hits.tsv").read_text() == want_hits
    assert "Output 1 of 4 genome pairs" in log and "Output %d fragment hits" % int(pair["matched"].sum()) in log
    # -a 0, a threshold in the noise and --min_fragments: every pair of genomes appears, then only the one with enough fragments
    want0 = oracle_expect(orc, out["ref"][1], out["qry"][1], frag_th=70.0, ani_th=0.0)
    assert want0[0].count("\n") == 4
    cli(hg, "dist", "--fragments", "-r", str(root / "ref.sketch"), "-q", str(root / "qry.sketch"), "-o", str(tmp_path / "f0.tsv"),
        "--fragment_hits=" + str(tmp_path / "hits0.tsv"), "--fragment_ani", "70", "-a", "0")
    assert (tmp_path / "f0.tsv").read_text() == want0[0] and (tmp_path / "hits0.tsv").read_text() == want0[1]
    n = int(pair["matched"][0, 0])
    for more, lines in ((n, 1), (n + 1, 0)):
        cli(hg, "dist", "--fragments", "-r", str(root / "ref.sketch"), "-q", str(root / "qry.sketch"), "-o", str(tmp_path / "f1.tsv"),
            "--min_fragments", str(more))
        assert (tmp_path / "f1.tsv").read_text() == frag_ref.tsv(pair, want0[4], want0[5], ANI_TH, min_fragments=more)
        assert (tmp_path / "f1.tsv").read_text().count("\n") == lines


@pytest.mark.gpu
def test_one_file_against_itself_writes_every_ordered_pair(hg, orc, sides, sketched, tmp_path):
    root, _, _ = sketched
    _, out = sides
    want_tsv, want_hits, pair, _, _, _ = oracle_expect(orc, out["qry"][1], out["qry"][1])
    cli(hg, "dist", "--fragments", "-r", str(root / "qry.sketch"), "-q", str(root / "qry.sketch"), "-o", str(tmp_path / "s.tsv"),
        "--fragment_hits", str(tmp_path / "s_hits.tsv"))
    assert (tmp_path / "s.tsv").read_text() == want_tsv and (tmp_path / "s_hits.tsv").read_text() == want_hits
    lines = want_tsv.splitlines()
    assert len(lines) == 2 and all(x.split("\t")[0] == x.split("\t")[1] and x.split("\t")[2:] == ["100.000", "60", "60"] for x in lines)


@pytest.mark.gpu
def test_a_genome_that_reappears_is_fatal(hg, sides, sketched, tmp_path):
    root, _, _ = sketched
    recs = hg.read_sketch_file(str(root / "qry.sketch"))
    hg.write_sketch_file(str(tmp_path / "bad.sketch"), recs[:3] + recs[60:62] + recs[3:5])
    r = subprocess.run([hg.CLI_PATH, "dist", "--fragments", "-r", str(root / "ref.sketch"), "-q", str(tmp_path / "bad.sketch"), "-o",
                        str(tmp_path / "x.tsv")], capture_output=True, text=True)
    assert r.returncode == 2 and "reappears at record '%s'" % recs[3]["file_str"] in r.stderr and not (tmp_path / "x.tsv").exists()
