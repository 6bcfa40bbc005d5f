"""The amino-acid sketch step (hg_aa_sketch_batch_dev, libhypergen_aa.so) against the tuned nucleotide kernel on the same bytes.

`--n` synthetic proteomes of `--len` residues (uniform over the 20 letters, a '*' every 400 bytes: protein boundaries) are made
on the device with torch and stay there.  The yardstick is hg_sketch_batch_dev on random ACGT of the same byte count, the same
k and scaled, canonical = 0, "sketch_path" = "sync": the same bytes, the same hash length and the same synchronous path,
through kmer_sample_shared.  Both legs run in one process, alternating, `--rounds` times; per round and leg `--steps` warm
steps give the wall ms (call + hg_ctx_sync) and, in a second pass with timing on, the device ms of the k-mer, sort and encode
classes (hg_ctx_timings).  Reported: medians over the rounds, the ratios, bytes per second of the k-mer kernels, and -- for
scale -- the rate at which tests/aa_ref.py's reference walks a proteome on one CPU core (Python windows around the oracle's C
t1ha2).  No figure is a pass condition.  Prints one JSON line and stores it (--out, default profiles/aa_sketch_bench.json).

    python tools/aa_sketch_bench.py [--n 1000 --len 1500000 --k 9 --scaled 1500 --rounds 3 --steps 5 --warmup 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=1_500_000)
    ap.add_argument("--k", type=int, default=9)
    ap.add_argument("--scaled", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-residues", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aa_sketch_bench.json"))
    return ap.parse_args()


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    a = parse()
    import numpy as np
    import torch
    import hypergen_amd as hg
    hg.lib_aa()
    dev = torch.device("cuda:0")
    stride = (a.len + 32 + 63) // 64 * 64
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def make(letters, stop):
        lut = torch.tensor(list(letters), dtype=torch.uint8, device=dev)
        buf = torch.zeros(a.n * stride + 64, dtype=torch.uint8, device=dev)
        view = buf[: a.n * stride].view(a.n, stride)
        for lo in range(0, a.n, 50):  # (in slices: the index tensor of the whole batch would take 12 GB)
            hi = min(a.n, lo + 50)
            idx = torch.randint(0, len(letters), (hi - lo, a.len), device=dev, generator=gen)
            view[lo:hi, : a.len] = lut[idx]
        if stop:
            view[:, 0: a.len: 400] = stop
        return buf

    prot, dna = make(b"ACDEFGHIKLMNPQRSTVWY", ord("*")), make(b"ACGT", 0)
    offs = np.arange(a.n, dtype=np.uint64) * stride
    lens = np.full(a.n, a.len, np.uint64)
    hv = torch.empty((a.n, 4096), dtype=torch.int16, device=dev)
    n2 = torch.empty(a.n, dtype=torch.int32, device=dev)
    nh = torch.empty(a.n, dtype=torch.int32, device=dev)
    p_aa = hg.default_params(ksize=a.k, scaled=a.scaled, canonical=0)
    p_dna = hg.default_params(ksize=a.k, scaled=a.scaled, canonical=0)
    runs = {"aa": [], "dna": []}
    names = {}
    with hg.Context(0) as c_aa, hg.Context(0) as c_dna:
        c_dna.set_debug("sketch_path", "sync")

        def step_aa():
            c_aa.aa_sketch_batch_dev(prot.data_ptr(), offs, lens, p_aa, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
            c_aa.sync()

        def step_dna():
            c_dna.sketch_batch_dev(dna.data_ptr(), offs, lens, p_dna, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
            c_dna.sync()

        for _ in range(a.rounds):
            for leg, ctx, step in (("aa", c_aa, step_aa), ("dna", c_dna, step_dna)):
                for _ in range(a.warmup):
                    step()
                wall = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    step()
                    wall.append((time.perf_counter() - t0) * 1e3)
                ctx.enable_timing(True)
                step()
                ctx.timings()
                for _ in range(a.steps):
                    step()
                t = ctx.timings()
                ctx.enable_timing(False)
                names[leg] = ctx.last_kernel("kmer")
                runs[leg].append({"wall_ms": round(median(wall), 3), "wall_ms_min": round(min(wall), 3),
                                  "kmer_ms": round(t["kmer"][0] / a.steps, 4), "sort_ms": round(t["sort"][0] / a.steps, 4),
                                  "encode_ms": round(t["encode"][0] / a.steps, 4),
                                  "nhash_mean": float(nh.cpu().numpy().view(np.uint32).mean())})
        counts = {"aa": c_aa.sketch_step_counts(), "dna": c_dna.sketch_step_counts()}
    total = float(a.n) * a.len
    med = {leg: {key: median([r[key] for r in runs[leg]]) for key in ("wall_ms", "kmer_ms", "sort_ms", "encode_ms")} for leg in runs}
    # the reference on one CPU core
    import aa_ref
    rng = np.random.default_rng(1)
    s = rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8), a.cpu_residues)
    t0 = time.perf_counter()
    aa_ref.hash_sample(s, a.k, a.scaled)
    cpu_s = time.perf_counter() - t0
    out = {"what": "hg_aa_sketch_batch_dev against hg_sketch_batch_dev (canonical = 0, sketch_path = sync) on the same bytes, one process, alternating",
           "version": hg.lib().hg_version().decode(), "source_stamp": hg.source_stamp(), "device": torch.cuda.get_device_name(0),
           "n": a.n, "residues_each": a.len, "ksize": a.k, "scaled": a.scaled, "rounds": a.rounds, "steps": a.steps,
           "resident_gb": round(total / 1e9, 3), "kernels": names, "step_counts": counts, "runs": runs, "median": med,
           "kmer_gb_per_s": {leg: round(total / 1e6 / med[leg]["kmer_ms"], 1) for leg in med},
           "ratio_aa_over_dna": {key: round(med["aa"][key] / med["dna"][key], 4) for key in ("wall_ms", "kmer_ms")},
           "cpu_reference": {"residues": a.cpu_residues, "seconds": round(cpu_s, 4), "mb_per_s_one_core": round(a.cpu_residues / 1e6 / cpu_s, 3)}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
