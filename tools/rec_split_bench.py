"""The record splitter (hg_rec_split_dev, libhypergen_rec.so) on one large multi-FASTA text, against two yardsticks that are not
the code under test: a device-to-device copy of the same number of bytes (the floor of reading n and writing about n) and
hg_rec_split_host on one host thread over the same text (what a per-file host reader would do).

Three synthetic texts of about `--mb` MB each, made on the host and resident (device and host) before anything is timed:
records of 50 kbp in lines of 80 columns, the same records unwrapped, and records of 2 kbp in lines of 80.  All legs run in
one process, alternating, `--rounds` times; a leg's time is the wall time of call plus synchronisation, `--steps` warm steps
per round, and the figures are medians over the rounds.  A second process under `rocprofv3 --kernel-trace --stats` runs the
split alone on the first text and gives the per-kernel times (null when the profiler is not there).  `--cli` adds the wall time
of `hyper-gen sketch --individual` on the first text written to a file.  No figure is a pass condition.  Prints one JSON line
and stores it (--out, default profiles/rec_split_bench.json).

    python tools/rec_split_bench.py [--mb 1024 --rounds 3 --steps 3 --cli]
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) the split alone, for the profiler")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_split_bench.json"))
    return ap.parse_args()


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def make_text(np, total, rec_len, width, seed):
    """records of rec_len bases in lines of `width` columns (0: one line) under fixed-width headers, about `total` bytes"""
    rng = np.random.default_rng(seed)
    width = width or rec_len
    lines = -(-rec_len // width)
    header = b">contig_00000000 length=%d synthetic\n" % rec_len
    rec_bytes = len(header) + lines * (width + 1)
    n = max(1, total // rec_bytes)
    text = np.empty((n, rec_bytes), np.uint8)
    text[:, :len(header)] = np.frombuffer(header, np.uint8)
    idx = np.arange(n)
    for d in range(8):  # the record number, eight digits
        text[:, 15 - d] = 48 + (idx // 10 ** d) % 10
    body = text[:, len(header):].reshape(n, lines, width + 1)
    lut = np.frombuffer(b"ACGT", np.uint8)
    for lo in range(0, n, 256):
        body[lo:lo + 256, :, :width] = lut[rng.integers(0, 4, (min(256, n - lo), lines, width), dtype=np.uint8)]
    body[:, :, width] = 10
    return text.reshape(-1), n


def kernel_times(a):
    """per-kernel device time of one split of the first text, from a run of its own under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rec", "--", sys.executable, os.path.abspath(__file__), "--child",
               "--mb", str(a.mb), "--steps", str(a.steps)]
        try:
            subprocess.run(cmd, check=True, capture_output=True, timeout=600)
        except Exception as e:  # no profiler, or it failed: not measured
            return None, repr(e)[:200]
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                m = re.search(r"\brec_\w+_kernel\b", row.get("Name", ""))
                if m:
                    rows[m.group(0)] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
        return rows or None, (None if rows else "no rec_* rows in the profiler's kernel statistics")


def main():
    a = parse()
    import numpy as np
    import torch
    import hypergen_amd as hg
    hg.lib_rec()
    dev = torch.device("cuda:0")
    total = a.mb << 20
    shapes = [("50kbp_80col", 50_000, 80)] if a.child else [("50kbp_80col", 50_000, 80), ("50kbp_unwrapped", 50_000, 0), ("2kbp_80col", 2_000, 80)]
    out = {"tool": "rec_split_bench", "mb": a.mb, "rounds": a.rounds, "steps": a.steps, "block_bytes": hg.rec_block_bytes(), "shapes": {}}
    with hg.Context(0) as ctx:
        for name, rec_len, width in shapes:
            text, n_records = make_text(np, total, rec_len, width, 1)
            n = int(text.size)
            d_text = torch.zeros((n + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
            d_text[:n] = torch.from_numpy(text).to(dev)
            torch.cuda.synchronize()
            st, n_recs, seq_bytes = ctx.rec_count_dev(d_text.data_ptr(), n)
            assert st == hg.OK and n_recs == n_records and seq_bytes == n_records * rec_len
            d_seq = torch.empty(seq_bytes + 32, dtype=torch.uint8, device=dev)
            d_recs = torch.empty(n_recs * 32, dtype=torch.uint8, device=dev)
            d_copy = torch.empty(n, dtype=torch.uint8, device=dev)
            h_seq = np.empty(seq_bytes + 32, np.uint8)
            h_recs = np.empty(n_recs, hg.REC_DTYPE)
            torch.cuda.synchronize()

            def split():
                assert ctx.rec_split_dev(d_text.data_ptr(), n, d_seq.data_ptr(), seq_bytes + 32, d_recs.data_ptr(), n_recs)[0] == hg.OK
                ctx.sync()

            def copy():
                d_copy.copy_(d_text[:n])
                torch.cuda.synchronize()

            def host():
                import ctypes as C
                r, b = C.c_size_t(0), C.c_size_t(0)
                assert hg.lib_rec().hg_rec_split_host(text.ctypes.data, n, h_seq.ctypes.data, h_seq.size, h_recs.ctypes.data, n_recs,
                                                      C.byref(r), C.byref(b)) == hg.OK

            def timed(fn, steps):
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                return (time.perf_counter() - t0) / steps * 1e3

            split(), copy()  # warm
            if a.child:
                for _ in range(a.steps):
                    split()
                return
            legs = {"split": [], "copy": [], "host": []}
            for _ in range(a.rounds):
                legs["split"].append(timed(split, a.steps))
                legs["copy"].append(timed(copy, a.steps))
                legs["host"].append(timed(host, 1))
            ms = {k: median(v) for k, v in legs.items()}
            # the device result is the host's
            assert (d_recs.cpu().numpy().view(hg.REC_DTYPE) == h_recs).all() and (d_seq[:seq_bytes].cpu().numpy() == h_seq[:seq_bytes]).all()
            out["shapes"][name] = {"text_bytes": n, "records": n_recs, "seq_bytes": seq_bytes,
                                   "split_ms": round(ms["split"], 3), "copy_d2d_ms": round(ms["copy"], 3), "host_1thread_ms": round(ms["host"], 1),
                                   "split_GBps": round(n / ms["split"] / 1e6, 1), "copy_GBps": round(n / ms["copy"] / 1e6, 1),
                                   "host_GBps": round(n / ms["host"] / 1e6, 2), "split_over_copy": round(ms["split"] / ms["copy"], 2),
                                   "host_over_split": round(ms["host"] / ms["split"], 1), "all_rounds_ms": legs}
            if a.cli and name == "50kbp_80col":
                with tempfile.TemporaryDirectory() as d:
                    text.tofile(os.path.join(d, "all.fna"))
                    t0 = time.perf_counter()
                    r = subprocess.run([hg.CLI_PATH, "sketch", "--individual", "-p", d, "-o", os.path.join(d, "o.sketch")], capture_output=True, text=True)
                    out["cli_individual_s"] = round(time.perf_counter() - t0, 2) if r.returncode == 0 else None
            del d_text, d_seq, d_recs, d_copy, text
    out["kernels_us"], out["kernels_note"] = kernel_times(a)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
