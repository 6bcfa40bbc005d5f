"""bench.py quotes profile counters only from summaries that belong to the tree and the kernel that ran (CPU test of the
stamp logic: no GPU, no torch)."""
import json

import numpy as np
import os
import sys
import types

from conftest import ROOT


def test_profiled_requires_matching_stamp_and_kernel(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "hg", types.SimpleNamespace(source_stamp=lambda: "aaaa000011112222"))
    good = {"_stamp": {"source_sha": "aaaa000011112222", "kernels": ["kmer_sample_shared<21, true>"], "head": "c0ffee" * 6},
            "kmer_sample_shared<21, true>": {"hbm_bytes_per_launch": 5.0e9}}
    json.dump(good, open(prof / "r07_pmc.json", "w"))
    d, src = bench.profiled("_pmc.json", "kmer_sample_shared<21, true>")
    assert d is not None and "r07_pmc.json" in src and "c0ffeec0ffee" in src
    # another kernel ran than the one that was profiled
    d, src = bench.profiled("_pmc.json", "kmer_sample_shared<25, true>")
    assert d is None and "does not hold the kernel" in src
    # a newer summary taken on other sources shadows the good one: null, with the reason
    stale = dict(good, _stamp=dict(good["_stamp"], source_sha="ffff000011112222"))
    json.dump(stale, open(prof / "r08_pmc.json", "w"))
    d, src = bench.profiled("_pmc.json", "kmer_sample_shared<21, true>")
    assert d is None and "other sources" in src
    # no stamp at all (the pre-round-3 files)
    json.dump({"kmer_sample_grouped<21>": {}}, open(prof / "r09_pmc.json", "w"))
    assert bench.profiled("_pmc.json", "kmer_sample_grouped<21>")[0] is None
    assert bench.profiled("_nothing.json", "x")[0] is None


def test_full_is_an_option_and_off_by_default(monkeypatch):
    """a plain `bench.py --gpus 1 --steps K --warmup W` is the headline alone; the other legs are asked for with --full"""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and (a.gpus, a.steps, a.warmup, a.dump_outputs) == (1, 3, 2, None)
    monkeypatch.setattr(sys, "argv", sys.argv + ["--full"])
    assert bench.parse().full is True


def test_committed_profiles_carry_stamps():
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r03_*.json")))
    assert files
    for f in files:
        if f.endswith(("_bench_line.json",)):
            continue
        d = json.load(open(f))
        sha = (d.get("_stamp") or {}).get("source_sha") or d.get("source_sha")
        assert sha and len(sha) == 16, f


def test_draftify_makes_what_it_says():
    """bench.draftify (the `realistic.draft_assemblies` input): 200 contigs, ~30 % soft-masked in 1 kbp runs, 0.05 % IUPAC codes,
    one tandem repeat of a 171-base unit -- checked on the CPU on three small genomes (the generator runs on whatever device
    the buffer lives on)"""
    import torch
    import bench
    n, L = 3, 300_000
    stride = (L + 1 + 15) // 16 * 16
    g = torch.Generator().manual_seed(1)
    seq = torch.tensor(list(b"ACGT"), dtype=torch.uint8)[torch.randint(0, 4, (n * stride + 64,), generator=g)]
    seq.view(-1)[0: n * stride: stride] = ord("N")
    clean = seq.clone()
    bench.draftify(seq, n, stride, L, repeat_len=50_000)
    a = seq[: n * stride].view(n, stride).numpy()
    c = clean[: n * stride].view(n, stride).numpy()
    assert (a[:, 0] == ord("N")).all() and np.array_equal(a[:, L + 1:], c[:, L + 1:])  # nothing outside the bodies moved
    body = a[:, 1: 1 + L]
    for row in body:
        assert 150 <= (row == ord("N")).sum() <= 199            # the record starts (a few coincide / are overwritten)
        low = np.isin(row, np.frombuffer(b"acgt", np.uint8)).mean()
        assert 0.2 < low < 0.4                                    # soft-masked share
        iupac = np.isin(row, np.frombuffer(b"RYKMSWBDHVn", np.uint8)).sum()
        assert 0.0003 * L < iupac <= 0.0005 * L + 1
        up = row & 0xDF
        # the tandem repeat: somewhere a 50 kbp stretch in which base i equals base i + 171 (but for the sprinkled codes)
        same = (up[:-171] == up[171:]).astype(np.int32)
        cs = np.concatenate([[0], np.cumsum(same)])
        run = cs[40_000:] - cs[:-40_000]  # matches in every window of 40 000 positions
        assert run.max() > 0.995 * 40_000


def test_dump_outputs_exact_bounded_and_seeded(tmp_path, monkeypatch):
    """bench.dump_outputs (--dump-outputs): the headline's arrays as float32 / float64 with their values unchanged; more genomes
    than fit 64 MB: the same seeded sample on every call, named in hv_rows.npy, and never more than 64 MB in all"""
    import torch
    import bench
    monkeypatch.setattr(bench, "np", np)
    monkeypatch.setattr(bench, "torch", torch)
    g = torch.Generator().manual_seed(2)
    for n, world in ((300, 1), (5000, 1), (3000, 2)):
        hv = torch.randint(-2**15, 2**15, (n, 4096), dtype=torch.int16, generator=g)
        n2 = torch.randint(0, 2**31 - 1, (n,), dtype=torch.int32, generator=g)
        nh = torch.randint(0, 2**31 - 1, (n,), dtype=torch.int32, generator=g)
        picks = []
        for rep in range(2):
            d = tmp_path / ("n%d_w%d_%d" % (n, world, rep))
            info = bench.dump_outputs(str(d), hv, n2, nh, world - 1, world)
            out = d / ("rank%d" % (world - 1)) if world > 1 else d
            got = {f.name: np.load(f) for f in out.iterdir()}
            assert (got["hv.npy"].dtype, got["hv_norm_2.npy"].dtype, got["nhash.npy"].dtype) == (np.float32, np.float64, np.float64)
            rows = got["hv_rows.npy"].astype(np.int64) if "hv_rows.npy" in got else np.arange(n)
            assert info["genomes"] == rows.size and info["of"] == n and (rows.size == n) == ("hv_rows.npy" not in got)
            assert np.array_equal(got["hv.npy"], hv.numpy()[rows]) and np.array_equal(got["hv_norm_2.npy"], n2.numpy()[rows])
            assert np.array_equal(got["nhash.npy"], nh.numpy()[rows])
            assert sum(f.stat().st_size for f in out.iterdir()) * world <= 64 << 20
            picks.append(rows)
        assert np.array_equal(picks[0], picks[1])
