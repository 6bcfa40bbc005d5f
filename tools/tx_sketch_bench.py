"""The translated sketch step (hg_tx_sketch_batch_dev, libhypergen_tx.so) against the two kernels it stands between.

`--n` synthetic genomes of `--len` bases (uniform ACGT) are made on the device with torch and stay there.  Three legs:
  tx   hg_tx_sketch_batch_dev on the genomes: two amino-acid k-mers per nucleotide start, translated in the kernel;
  aa   hg_aa_sketch_batch_dev on the six frame strings of the same genomes, translated beforehand with torch (6 n proteomes of
       len / 3 residues, stops as '*'): the same k-mers and the same hashes by construction, without the translation and with
       one k-mer per input byte instead of two -- twice the bytes;
  dna  hg_sketch_batch_dev on the same nucleotides, the same k and scaled, canonical = 0, "sketch_path" = "sync": the tuned
       nucleotide kernel (kmer_sample_shared) on the bytes tx reads, one k-mer per byte.
All legs run in one process, alternating, `--rounds` times; per round and leg `--steps` warm steps give the wall ms (call +
hg_ctx_sync) and, in a second pass with timing on, the device ms of the k-mer, sort and encode classes (hg_ctx_timings).
Reported: medians over the rounds, the ratios, input bytes and k-mers per second of the k-mer kernels, and `legs_compared`:
whether tx and aa sampled the same k-mers (set sizes of every genome, hash lists where they differ and of the first --check).  No figure is a pass
condition.  Prints one JSON line and stores it (--out, default profiles/tx_sketch_bench.json).

    python tools/tx_sketch_bench.py [--n 400 --len 1500000 --k 9 --scaled 1500 --rounds 3 --steps 5 --warmup 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODONS = b"FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"  # NCBI table 1, bases ordered T C A G


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--len", type=int, default=1_500_000)
    ap.add_argument("--k", type=int, default=9)
    ap.add_argument("--scaled", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=4, help="genomes whose hash lists are compared between the legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx_sketch_bench.json"))
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
    hg.lib_tx()
    dev = torch.device("cuda:0")
    stride = (a.len + 32 + 63) // 64 * 64
    flen = a.len // 3
    fstride = (flen + 32 + 63) // 64 * 64
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    letters = torch.tensor(list(b"TCAG"), dtype=torch.uint8, device=dev)
    table = torch.tensor(list(CODONS), dtype=torch.uint8, device=dev)
    dna = torch.zeros(a.n * stride + 64, dtype=torch.uint8, device=dev)
    frames = torch.zeros(6 * a.n * fstride + 64, dtype=torch.uint8, device=dev)
    dview = dna[: a.n * stride].view(a.n, stride)
    fview = frames[: 6 * a.n * fstride].view(a.n, 6, fstride)
    flens = np.zeros((a.n, 6), np.uint64)
    for lo in range(0, a.n, 20):  # (in slices: the index tensors of the whole batch would take tens of GB)
        hi = min(a.n, lo + 20)
        rank = torch.randint(0, 4, (hi - lo, a.len), device=dev, generator=gen)  # rank in T C A G
        dview[lo:hi, : a.len] = letters[rank]
        for strand, r in enumerate((rank, (rank ^ 2).flip(1))):  # the complement of a rank is rank ^ 2
            for f in range(3):
                m = (a.len - f) // 3
                idx = 16 * r[:, f:f + 3 * m:3] + 4 * r[:, f + 1:f + 3 * m:3] + r[:, f + 2:f + 3 * m:3]
                fview[lo:hi, 3 * strand + f, :m] = table[idx]
                flens[lo:hi, 3 * strand + f] = m
        del rank, idx
    torch.cuda.synchronize()  # the library's streams are not torch's: the genomes must be complete before a ctx reads them
    offs = np.arange(a.n, dtype=np.uint64) * stride
    lens = np.full(a.n, a.len, np.uint64)
    foffs = np.arange(6 * a.n, dtype=np.uint64) * fstride
    flens = flens.reshape(-1)
    hv = torch.empty((6 * a.n, 4096), dtype=torch.int16, device=dev)
    n2 = torch.empty(6 * a.n, dtype=torch.int32, device=dev)
    nh = torch.empty(6 * a.n, dtype=torch.int32, device=dev)
    p = hg.default_params(ksize=a.k, scaled=a.scaled, canonical=0)
    runs = {"tx": [], "aa": [], "dna": []}
    names = {}
    nhash = {}
    with hg.Context(0) as c_tx, hg.Context(0) as c_aa, hg.Context(0) as c_dna:
        c_dna.set_debug("sketch_path", "sync")

        def step_tx():
            c_tx.tx_sketch_batch_dev(dna.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
            c_tx.sync()

        def step_aa():
            c_aa.aa_sketch_batch_dev(frames.data_ptr(), foffs, flens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
            c_aa.sync()

        def step_dna():
            c_dna.sketch_batch_dev(dna.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
            c_dna.sync()

        for _ in range(a.rounds):
            for leg, ctx, step, rows in (("tx", c_tx, step_tx, a.n), ("aa", c_aa, step_aa, 6 * a.n), ("dna", c_dna, step_dna, a.n)):
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
                nhash[leg] = nh[:rows].cpu().numpy().view(np.uint32).astype(np.int64)
                runs[leg].append({"wall_ms": round(median(wall), 3), "wall_ms_min": round(min(wall), 3),
                                  "kmer_ms": round(t["kmer"][0] / a.steps, 4), "sort_ms": round(t["sort"][0] / a.steps, 4),
                                  "encode_ms": round(t["encode"][0] / a.steps, 4),
                                  "nhash_sum": int(nh[:rows].cpu().numpy().view(np.uint32).astype(np.int64).sum())})
        # the two legs against each other.  Every genome: the six frame sets' sizes must add up to the translated set's size but
        # for k-mers that two frames share.  The first --check genomes and every genome where the sizes do not add up (64 at
        # most): the hash lists themselves -- the union of the six frame lists must BE the translated list, and the k-mers the
        # frames share must account for the difference -- and the frame strings against the library's host translation.
        per_genome = nhash["aa"].reshape(a.n, 6).sum(1) - nhash["tx"]
        lists_equal, shared, frames_equal = True, [], True
        listed = sorted(set(range(min(a.check, a.n))) | set(np.nonzero(per_genome)[0][:64].tolist()))
        for g in listed:
            seq = dview[g, : a.len].cpu().numpy()
            got = c_tx.tx_hash_sample(seq, a.k, a.scaled)
            fl = []
            for f in range(6):
                fr = fview[g, f, : int(flens[6 * g + f])].cpu().numpy()
                frames_equal = frames_equal and fr.tobytes() == hg.tx_translate_frame(seq, f)
                fl.append(c_aa.aa_hash_sample(fr, a.k, a.scaled))
            union = np.unique(np.concatenate(fl))
            lists_equal = lists_equal and union.size == got.size and bool((union == got).all()) and got.size == int(nhash["tx"][g])
            shared.append(int(sum(x.size for x in fl) - union.size))
            lists_equal = lists_equal and shared[-1] == int(per_genome[g])
        check = {"genomes_listed": len(listed), "every_difference_listed": int((per_genome != 0).sum()) <= 64, "translated_list_equals_union_of_frame_lists": lists_equal,
                 "frame_strings_equal_host_translation": frames_equal, "kmers_shared_between_frames_listed": shared,
                 "frames_nhash_minus_tx_nhash": {"sum": int(per_genome.sum()), "min": int(per_genome.min()), "max": int(per_genome.max()),
                                                 "genomes_nonzero": int((per_genome != 0).sum())}}
        counts = {"tx": c_tx.sketch_step_counts(), "aa": c_aa.sketch_step_counts(), "dna": c_dna.sketch_step_counts()}
    med = {leg: {key: median([r[key] for r in runs[leg]]) for key in ("wall_ms", "kmer_ms", "sort_ms", "encode_ms")} for leg in runs}
    in_bytes = {"tx": float(a.n) * a.len, "aa": float(flens.sum()), "dna": float(a.n) * a.len}
    kmers = {"tx": 2.0 * a.n * (a.len - 3 * a.k + 1), "aa": float((flens - a.k + 1).sum()), "dna": float(a.n) * (a.len - a.k + 1)}  # windows looked at
    out = {"what": "hg_tx_sketch_batch_dev against hg_aa_sketch_batch_dev on the six frame strings and hg_sketch_batch_dev (canonical = 0, "
                   "sketch_path = sync) on the same nucleotides, one process, alternating",
           "version": hg.lib().hg_version().decode(), "source_stamp": hg.source_stamp(), "device": torch.cuda.get_device_name(0),
           "n": a.n, "bases_each": a.len, "ksize": a.k, "scaled": a.scaled, "rounds": a.rounds, "steps": a.steps,
           "resident_gb": round((in_bytes["tx"] + in_bytes["aa"]) / 1e9, 3), "kernels": names, "step_counts": counts, "legs_compared": check, "runs": runs,
           "median": med,
           "kmer_input_gb_per_s": {leg: round(in_bytes[leg] / 1e6 / med[leg]["kmer_ms"], 1) for leg in med},
           "kmer_gwindows_per_s": {leg: round(kmers[leg] / 1e6 / med[leg]["kmer_ms"], 1) for leg in med},
           "ratio_tx_over_aa": {key: round(med["tx"][key] / med["aa"][key], 4) for key in ("wall_ms", "kmer_ms")},
           "ratio_tx_over_dna": {key: round(med["tx"][key] / med["dna"][key], 4) for key in ("wall_ms", "kmer_ms")}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
