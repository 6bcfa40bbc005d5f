#!/usr/bin/env python3
"""bench.py -- HyperGen sketch + ANI hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]      the headline alone
    python bench.py --gpus N --steps K --warmup W --full                    ... and every other leg
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run does what the headline needs and nothing else: it generates and packs the genomes, settles and warms up,
times the K steps, writes the step's outputs if asked to and prints the line (the headline, its kernel times and the
roofline figures that follow from them).  --full adds every other leg after the headline's timed steps -- the
ASCII-resident form, the realistic inputs, the 10k-genome job, the host-fed and per-call legs, dist, the Hamming search,
the CLI end to end, the CPU baselines and the parity gates against the CPU oracle (20 s on one GPU, where the plain
run spends 2.5 s beside its steps); the options that size or skip one of those legs mean something only beside it.

One "step" = one pass of the sketch hot path (k-mer hash + FracMinHash sample -> set ->
HV encode -> norm; what src/sketch.rs:35-48 does per file) over one batch of synthetic genomes
that are already resident in HBM.  Workload at every N: BASELINE.json configs[1] per GPU
(1 000 synthetic 5 Mbp genomes, k=21 scaled=1500 D=4096) -- genomes shard embarrassingly, no
data-path collective, weak scaling.  The secondary metric (M ANI-pairs/s, configs[3]:
10 000 x 10 000 HVs, ani_th=85) is reported in the "dist" object of a --full run's line; its only
exchange step is the RCCL all-gather of the reference HV matrix.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# numpy / torch / hypergen_amd are imported by main() AFTER the self-launch decision: the parent of an N > 1 run
# must not load the HIP runtime (its children are fresh processes, never a re-exec of one that touched the GPU)
np = torch = hg = None

L_GENOME = 5_000_000
HV_D = 4096
KSIZE = 21
SCALED = 1500
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense f16/bf16 MFMA peak


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--genomes", type=int, default=1000, help="genomes per GPU and step")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run every other leg too (ascii_resident, realistic, sketch_10k, host_fed, per_call, dist, "
                         "hamming, cli, the CPU baselines and the parity gates); without it the options of those legs are not used")
    ap.add_argument("--dist-n", type=int, default=10000, help="R = Q of the ANI matrix (0 = skip)")
    ap.add_argument("--hamming-refs", type=int, default=50000, help="refs of the bit-packed D=16384 search (0 = skip)")
    ap.add_argument("--hamming-queries", type=int, default=10000, help="queries of the bit-packed search")
    ap.add_argument("--genomes-10k", type=int, default=10000,
                    help="TOTAL genomes of the configs[2] leg, sharded over the ranks (0 = skip)")
    ap.add_argument("--hostfed-genomes", type=int, default=256, help="genomes of the host-fed (PCIe) leg (0 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-realistic", action="store_true", help="skip the draft-assembly and many-small-genomes legs")
    ap.add_argument("--cli-sketch-files", type=int, default=8192, help="files of the cli leg's `hyper-gen sketch` run (64 distinct 5 Mbp genomes + links; 0 = skip)")
    ap.add_argument("--no-dist-variants", action="store_true", help="skip dist.two_sets / dist.symmetric (profiling runs: their "
                                                                     "launches would enter the dist kernel's per-launch averages)")
    ap.add_argument("--small-genomes", type=int, default=100000, help="genomes of the many-small-genomes leg (50 kbp each)")
    ap.add_argument("--no-cli", action="store_true", help="skip the `cli` object (tools/cli_dist_bench.py as a child process: end-to-end "
                                                           "hyper-gen dist / search at --dist-n sketches and hyper-gen sketch over --cli-sketch-files FASTA files; N = 1 only, ~12 s)")
    ap.add_argument("--cli", action="store_true", help=argparse.SUPPRESS)  # (the leg is on by default since round 5)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to test the "
                                                      "multi-rank logic on a box with fewer GPUs than ranks)")
    ap.add_argument("--share-gpu", action="store_true", help="testing aid: every rank uses device 0")
    ap.add_argument("--collectives", action="store_true",
                    help="initialise the process group and run the all-gather / broadcast steps even with ONE rank "
                         "(a one-GPU box then executes the RCCL code path of the N > 1 run)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--dist-chunks", type=int, default=2,
                    help="row chunks per rank of the dist leg's operand exchange (chunk c + 1 travels under the GEMM of chunk c)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the headline's timed steps, write what its last step computed (hv, hv_norm_2, nhash) as "
                         "DIR/<name>.npy (see dump_outputs)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    return a


_CTX = []  # the bench's hg.Context once it exists: barrier_sync completes its queued sketch step (hg_ctx_sync) first


def dev_sync():
    for c in _CTX:
        c.sync()  # reads the check word of the last queued sketch step (re-running it if it asks), waits for the ctx's stream
    torch.cuda.synchronize()


def barrier_sync(world):
    dev_sync()
    if world > 1 or torch.distributed.is_initialized():
        torch.distributed.barrier()
    torch.cuda.synchronize()


def max_over_ranks(x, world, dev):
    if world == 1 and not torch.distributed.is_initialized():
        return x
    if torch.distributed.get_backend() != "nccl":
        dev = torch.device("cpu")
    t = torch.tensor([x], dtype=torch.float64, device=dev)
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    return float(t.item())


def clustered_hvs(rows, first_row, dev, n=3333, shared_frac=0.5, cluster=100, salt=0):
    """Synthetic i16 HVs with the statistics of real sketches: hv = 2*count - n where count is
    Binomial(n, 1/2); members of a cluster share the counts of shared_frac*n hashes, so
    within-cluster ANI is ~96-97 % and cross-cluster ANI ~0 (about 1 % of pairs pass ani_th=85).
    salt != 0: OTHER members of the same clusters (same shared counts, fresh private ones) -- a second,
    distinct set with the hit structure of the first (the two-set legs)."""
    import torch  # (tests import this helper without going through main())
    ns = int(n * shared_frac)
    ids = torch.arange(first_row, first_row + rows, device=dev)
    cl = ids // cluster
    out = torch.empty((rows, HV_D), dtype=torch.int16, device=dev)
    half = torch.tensor(0.5, device=dev)
    for c in torch.unique(cl).tolist():
        g = torch.Generator(device=dev)
        g.manual_seed(0x48470000 + int(c))
        # normal approximation of Binomial(ns, 1/2), rounded: cheap, deterministic per cluster
        shared = torch.round(ns / 2 + (ns ** 0.5) / 2 * torch.randn(HV_D, generator=g, device=dev))
        m = cl == c
        k = int(m.sum())
        g2 = torch.Generator(device=dev)
        g2.manual_seed(0x48480000 + int(c) * 7919 + first_row + 104729 * salt)
        fresh = torch.round((n - ns) / 2 + ((n - ns) ** 0.5) / 2 * torch.randn((k, HV_D), generator=g2, device=dev))
        out[m] = (2 * (shared[None, :] + fresh) - n).to(torch.int16)
    del half
    return out


def draftify(seq, n, stride, L, seed=0x5EED, repeat_len=50_000):
    """Rewrites the n clean single-contig synthetic genomes in `seq` (genome g at g*stride: 'N' + L bases, the
    read_merge_seq layout of src/fastx_reader.rs:6-29) IN PLACE into what a draft assembly looks like to the sketch path:
      * 200 contigs: 199 further record starts, i.e. an 'N' at 199 random positions (one per FASTA header);
      * ~30 % soft-masked: whole 1 kbp blocks lower-cased (RepeatMasker-style runs);
      * 0.05 % IUPAC ambiguity codes (RYKMSWBDHV and n) at random positions;
      * one 50 kbp tandem repeat of a 171-base unit at a random place.
    Deterministic (torch generator on the buffer's device); the same bytes go to the CPU oracle for the gate."""
    import torch
    dev = seq.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    view = seq[: n * stride].view(n, stride)
    iupac = torch.tensor(list(b"RYKMSWBDHVn"), dtype=torch.uint8, device=dev)
    CH = 50  # genomes per pass (bounds the scratch)
    for g0 in range(0, n, CH):
        m = min(CH, n - g0)
        body = view[g0: g0 + m, 1: 1 + L]
        rows = torch.arange(m, device=dev)[:, None]
        # tandem repeat first (the masks below then apply to it like to everything else)
        start = torch.randint(0, L - repeat_len, (m,), generator=g, device=dev)
        unit = torch.gather(body, 1, start[:, None] + torch.arange(171, device=dev)[None, :])
        idx = start[:, None] + torch.arange(repeat_len, device=dev)[None, :]
        body[rows, idx] = unit[:, torch.arange(repeat_len, device=dev) % 171]
        nblk = (L + 999) // 1000
        soft = torch.rand((m, nblk), generator=g, device=dev) < 0.30
        soft = soft.repeat_interleave(1000, dim=1)[:, :L]
        body |= soft.to(torch.uint8) * 0x20
        del soft
        k = int(L * 0.0005)
        pos = torch.randint(0, L, (m, k), generator=g, device=dev)
        body[rows, pos] = iupac[torch.randint(0, iupac.numel(), (m, k), generator=g, device=dev)]
        brk = torch.randint(0, L, (m, 199), generator=g, device=dev)
        body[rows, brk] = ord("N")


def newest_profile(suffix):
    """Path of the newest committed profiles/rNN<suffix> (the counters cannot be collected inside this process:
    rocprofv3 --pmc passes of this very command produce them, tools/profile_gpu.sh)."""
    import glob
    c = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]" + suffix)))
    return c[-1] if c else None


def profiled(suffix, kernel):
    """(summary, path) of the newest committed profiles/rNN<suffix> -- but only if it was taken on THESE sources
    (`_stamp.source_sha` == hypergen_amd.source_stamp(), written by tools/summarize_prof.py on the GPU box) and names the
    kernel the library says it has just launched (hg_ctx_last_kernel).  Otherwise (None, reason): a kernel change
    without a re-profile must report null, not the previous kernel's counters."""
    path = newest_profile(suffix)
    if not path:
        return None, "no profiles/rNN%s" % suffix
    try:
        d = json.load(open(path))
    except Exception as e:
        return None, "%s unreadable: %s" % (os.path.relpath(path, ROOT), e)
    st = d.get("_stamp") or {}
    rel = os.path.relpath(path, ROOT)
    if st.get("source_sha") != hg.source_stamp():
        return None, "%s was taken on other sources (%s, this tree %s)" % (rel, st.get("source_sha"), hg.source_stamp())
    if kernel not in (st.get("kernels") or []) and d.get("kernel") != kernel:
        return None, "%s does not hold the kernel that ran (%s)" % (rel, kernel)
    return d, "%s (commit %s, kernel %s)" % (rel, (st.get("head") or "?")[:12], kernel)


SETTLE = {"sketch": 25, "dist": 300, "hamming": 30}  # untimed repetitions in front of a leg's warmup steps


def settle(fn, n):
    """Untimed clock settle in front of a leg's W warmup steps: the GPU's DVFS takes a few tens of milliseconds of load
    to reach the clock it then holds (three back-to-back 1 000-genome sketches on an idle MI355X: 12.9 / 11.3 /
    10.8 ms), so with a small K the timed steps would otherwise measure the ramp.  The leg's own step is repeated a
    FIXED number of times (about 0.2 s of work; the same count on every rank -- the steps of the dist and search legs
    contain collectives); the counts are reported as `settle_steps` in the line."""
    for _ in range(n):
        fn()
    dev_sync()


def valu_issue(n_genomes, kernel):
    """Secondary, informative roofline of the k-mer kernel: its VALU instruction rate against the issue rate the
    same instruction mix reaches in tools/gpu_microbench.hip.  Instruction count and kernel cycles: the newest
    committed PMC passes of this command (SQ_INSTS_VALU, GRBM_GUI_ACTIVE), quoted only when they belong to this tree
    and this kernel (profiled()); the slow-class / plain split of the mix: the committed ISA histogram of the kernel
    (profiles/rNN_kmer_isa.json, tools/kmer_isa.py)."""
    d, src = profiled("_pmc.json", kernel)
    if d is None:
        return {"frac": None, "source": src}
    try:
        k = d[kernel]
        insts, cycles = k["SQ_INSTS_VALU"], k["GRBM_GUI_ACTIVE"] / 8.0
        ipath = newest_profile("_kmer_packed_isa.json" if kernel.endswith(", true>") else "_kmer_isa.json")
        isa = json.load(open(ipath))
        if isa.get("kernel") != kernel or isa.get("source_sha") != hg.source_stamp():
            raise KeyError("ISA histogram of another kernel / tree")
        slow_frac = isa["per_kmer"]["slow_class"] / isa["per_kmer"]["valu"]
    except Exception as e:
        return {"frac": None, "source": "%s; %r" % (src, e)}
    rate = insts / (1024 * cycles)  # wave-instructions per SIMD per cycle, as profiled
    per_kmer = insts * 64.0 / (n_genomes * (L_GENOME + 1 - KSIZE + 1)) if n_genomes == 1000 else None
    # issue cost of the mix: slow class 3.9 cycles, plain 2.3 cycles per wave-instruction (profiles/r01_instruction_rates.txt)
    bound = 1.0 / (slow_frac * 3.9 + (1.0 - slow_frac) * 2.3)
    return {"valu_instr_per_simd_cycle": rate, "mix_issue_bound": bound, "frac": rate / bound,
            "valu_instr_per_kmer": per_kmer, "slow_class_fraction": slow_frac,
            "source": "%s (rocprofv3 --pmc of this command), %s (static ISA histogram), "
                      "profiles/r01_instruction_rates.txt (issue costs)" % (src, os.path.relpath(ipath, ROOT))}


def effective_cores():
    """Host cores this process may really use: min(cpu_count, affinity mask, cgroup CPU quota),
    capped at 255 like the reference's `-t` (u8, src/utils.rs:54-56)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]  # cgroup v2
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except Exception:
            pass
    return max(1, min(n, 255))


def cpu_baseline_sketch(seconds, log):
    """Oracle (CPU port of src/sketch.rs:35-56: per-genome task parallelism, ASCII canonical k-mers,
    t1ha2, set, AVX2-layout encode, norm) on a bounded sample of the same workload, all host cores."""
    from oracle import oracle as orc
    orc.lib()
    cores = effective_cores()
    n = min(max(2 * cores, 16), 512)                # bounded host memory: n x 5 MB
    genomes = orc.synth_genomes_mt(0, n, L_GENOME, cores)
    t0 = time.perf_counter()
    orc.sketch_batch_mt(genomes[:cores], cores)  # calibration pass (also warms the threads)
    t1 = time.perf_counter() - t0
    reps = max(1, min(20, int(seconds / max(t1 * n / cores, 1e-3))))
    t0 = time.perf_counter()
    for _ in range(reps):
        orc.sketch_batch_mt(genomes, cores)
    dt = time.perf_counter() - t0
    log("cpu baseline: %d genomes x %d passes on %d threads in %.1f s" % (n, reps, cores, dt))
    return {"value": n * reps / dt, "unit": "genomes/sec", "cores": cores, "kind": "port",
            "sample": "%d of the step's synthetic 5 Mbp genomes x %d passes, oracle/libhg_oracle.so "
                      "orc_sketch_batch_mt (CPU restatement of src/sketch.rs:35-56, OpenMP over genomes), "
                      "%d threads, %.1f s" % (n, reps, cores, dt)}


def cpu_baseline_dist(hv, n2, seconds, log):
    from oracle import oracle as orc
    cores = effective_cores()
    orc.set_threads(cores)
    rows = min(hv.shape[0], 512)
    r, rn = hv[:rows].cpu().numpy(), n2[:rows].cpu().numpy()
    t0 = time.perf_counter()
    orc.ani_matrix(r, rn, r, rn, KSIZE)
    t1 = time.perf_counter() - t0
    # grow the sub-block until it takes a few seconds (pairs scale with R x Q)
    q_rows = int(min(hv.shape[0], max(rows, rows * seconds / max(t1, 1e-4))))
    rows = min(hv.shape[0], 2048)
    r, rn = hv[:rows].cpu().numpy(), n2[:rows].cpu().numpy()
    q, qn = hv[:q_rows].cpu().numpy(), n2[:q_rows].cpu().numpy()
    t0 = time.perf_counter()
    block = orc.ani_matrix(r, rn, q, qn, KSIZE)
    dt = time.perf_counter() - t0
    log("cpu dist baseline: %d x %d in %.2f s" % (rows, q_rows, dt))
    return block, {"value": rows * q_rows / dt / 1e6, "unit": "M ANI-pairs/sec", "cores": cores, "kind": "port",
            "sample": "%d x %d sub-block of the step's HVs, oracle orc_ani_matrix (src/dist.rs:139-161, scalar "
                      "i16 dot per pair), OpenMP over rows on %d threads, %.2f s" % (rows, q_rows, cores, dt)}


DUMP_BYTES = 64 << 20  # --dump-outputs: the most all ranks together write


def dump_outputs(d, hv, n2, nh, rank, world):
    """--dump-outputs DIR: what a caller of the headline step (hg_sketch_batch_dev_packed) receives from its last timed
    step -- the HVs as float32 (i16 values, exact), the squared norms and hash counts as float64 (i32 values, exact).
    More genomes than fit this rank's share of DUMP_BYTES: a fixed, seeded sample of them (the same for the same
    arguments), whose genome indices go to hv_rows.npy.  With N > 1 ranks, rank r writes into DIR/rank<r>/."""
    if world > 1:
        d = os.path.join(d, "rank%d" % rank)
    os.makedirs(d, exist_ok=True)
    n = hv.shape[0]
    per_genome = hv.shape[1] * 4 + 2 * 8 + 8  # hv row, norm and count, row index
    limit = (DUMP_BYTES // world - 4 * 1024) // per_genome  # (1 KB for the header of each of the four files)
    rows = None
    if n > limit:
        rows = np.sort(np.random.default_rng(0x48470D).choice(n, limit, replace=False))
        sel = torch.from_numpy(rows).to(hv.device)
        hv, n2, nh = hv[sel], n2[sel], nh[sel]
        np.save(os.path.join(d, "hv_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(d, "hv.npy"), hv.cpu().numpy().astype(np.float32))
    np.save(os.path.join(d, "hv_norm_2.npy"), n2.cpu().numpy().astype(np.float64))
    np.save(os.path.join(d, "nhash.npy"), nh.cpu().numpy().astype(np.float64))
    return {"dir": d, "genomes": n if rows is None else int(rows.size), "of": n}


def self_launch(a):
    """`python bench.py --gpus N` with N > 1 and no torch.distributed environment: start the N ranks as CHILD
    processes (torch.distributed.run, one per GPU, rendezvous on 127.0.0.1), let rank 0's JSON line through on the
    inherited stdout and exit with the children's status.  Nothing in this parent has imported torch or the HIP
    library at this point."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("[bench] launching %d ranks: %s" % (a.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    sys.exit(subprocess.run(cmd, env=env).returncode)


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        self_launch(a)
    global np, torch, hg
    import numpy as np
    import torch
    import torch.distributed  # noqa: F401
    import hypergen_amd as hg
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    if a.share_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # tensors handed to collectives live on the GPU for RCCL; gloo (testing aid) gets host copies
    cdev = dev if a.backend == "nccl" else torch.device("cpu")
    coll = world > 1 or a.collectives  # run the exchange steps (always at N > 1; at N = 1 only on request)
    if coll:
        if "WORLD_SIZE" not in os.environ:  # bare one-rank run with --collectives: a private rendezvous
            import socket
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(s.getsockname()[1]), RANK="0", WORLD_SIZE="1")
            s.close()
        if a.backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=dev)
        else:
            torch.distributed.init_process_group(a.backend)

    def log(msg):
        if rank == 0:
            print("[bench] " + msg, file=sys.stderr, flush=True)

    def finish():
        """the end of every run, plain or --full: the process group goes, rank 0 prints the line, exit code 4 if an auxiliary leg failed"""
        if coll:
            out["collectives"] = {"backend": torch.distributed.get_backend(), "world": world,
                                  "steps": ("chunked all-gather of the prepared reference operands + control records (dist), query broadcast + hit "
                                            "gather (hamming), " if a.full else "") + "barrier / max-reduce around every timed region"}
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        if aux_failures:
            out["aux_failures"] = aux_failures
        if rank == 0:
            print(json.dumps(out), flush=True)
        ctx.close()
        if aux_failures:
            sys.exit(4)

    # No cyclic-GC passes inside the timed loops: with torch loaded a full collection takes ~10 ms, more than a step
    # (one run of round 3 showed exactly such a step: 20 steps at 8.73 ms of kernels averaged 9.34 ms).
    import gc
    gc.collect()
    gc.freeze()
    gc.disable()

    ctx = hg.Context(local)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    _CTX.append(ctx)
    aux_failures = []  # parity failures of legs the headline does not depend on: recorded in the line, exit code 4 after printing it

    # ---------------- sketch: genomes resident in HBM -------------------------------------------
    N = a.genomes
    stride = (L_GENOME + 1 + 15) // 16 * 16
    seq = torch.empty(N * stride + 64, dtype=torch.uint8, device=dev)
    ctx.synth_genomes_dev(rank * N, N, L_GENOME, stride, seq.data_ptr())
    offs = np.arange(N, dtype=np.uint64) * stride
    lens = np.full(N, L_GENOME + 1, np.uint64)
    p = hg.default_params(ksize=KSIZE, scaled=SCALED, hv_d=HV_D)
    hv = torch.empty((N, HV_D), dtype=torch.int16, device=dev)
    n2 = torch.empty(N, dtype=torch.int32, device=dev)
    nh = torch.empty(N, dtype=torch.int32, device=dev)

    # The headline runs on 2-bit PACKED bases (north_star: "coalesced HBM reads of packed bases"): the synthetic ASCII
    # genomes are packed once, on the device and outside every timed region (hg_pack2_batch_dev = the host's hg_pack2
    # byte for byte), and the step is hg_sketch_batch_dev_packed on the blobs.  The ASCII-resident form of the same step
    # is timed right after it in a --full run (`ascii_resident`) and must give identical sketches.
    blob_sz = hg.lib().hg_pack2_size(L_GENOME + 1)
    boffs = np.arange(N, dtype=np.uint64) * blob_sz
    blobs = torch.empty(N * blob_sz + 64, dtype=torch.uint8, device=dev)
    ctx.pack2_batch_dev(seq.data_ptr(), offs, lens, blobs.data_ptr(), boffs)

    def step():
        ctx.sketch_batch_dev_packed(blobs.data_ptr(), boffs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())

    def step_ascii():
        ctx.sketch_batch_dev(seq.data_ptr(), offs, lens, p, hv_a.data_ptr(), n2_a.data_ptr(), nh_a.data_ptr())

    # (disclosed beside the steady-state figures: what the very first call of the process costs -- workspaces, the code object,
    # an idle GPU's clock -- and the first timed-looking call after it)
    dev_sync()
    t0 = time.perf_counter()
    step()
    dev_sync()
    cold_first_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    step()
    dev_sync()
    cold_second_ms = (time.perf_counter() - t0) * 1e3
    settle(step, SETTLE["sketch"])
    for _ in range(a.warmup):
        step()
    ctx.enable_timing(True)
    ctx.timings()
    barrier_sync(world)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    barrier_sync(world)
    dt = max_over_ranks(time.perf_counter() - t0, world, dev)
    tm = ctx.timings()
    ctx.enable_timing(False)
    dumped = dump_outputs(a.dump_outputs, hv, n2, nh, rank, world) if a.dump_outputs else None
    kmer_ms, kmer_launches = tm["kmer"]
    kmer_avg_ms = kmer_ms / max(kmer_launches, 1)
    bytes_per_launch = N * (L_GENOME + 2 * HV_D)  # L + 2*D algorithmic bytes per genome
    achieved = bytes_per_launch / (kmer_avg_ms * 1e-3) / 1e9
    kmer_kernel = ctx.last_kernel("kmer")
    traffic, traffic_src = None, "not the profiled shape (1 000 genomes per launch)"
    if N == 1000:
        td, traffic_src = profiled("_kmer_traffic.json", kmer_kernel)
        traffic = td.get("hbm_bytes_per_launch") if td else None
    value = N * world * a.steps / dt
    log("sketch: %.1f genomes/s, kmer kernel %.3f ms/launch (%d launches), nhash mean %.1f" % (
        value, kmer_avg_ms, kmer_launches, nh.float().mean().item()))
    isa_path = newest_profile("_kmer_packed_isa.json")
    try:
        isa_valu = json.load(open(isa_path))["per_kmer"]["valu"]
    except Exception:
        isa_valu = None

    out = {
        "metric": "genomes/sec sketch (k=21,s=1500,D=4096)", "value": value, "unit": "genomes/sec",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "settle_steps": SETTLE, "ms_per_step": dt / a.steps * 1e3,
        "cold_start": {"first_step_ms": cold_first_ms, "second_step_ms": cold_second_ms,
                       "note": "the process's first two sketch steps, before the untimed clock settle (never part of `value`)"},
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u64",
        "data": "synthetic",
        "config": {"workload": "%d synthetic 5 Mbp genomes per GPU (BASELINE configs[1]), sketch k=21 "
                               "scaled=1500 seed=123 canonical D=4096 AVX2 layout, inputs resident in HBM as 2-bit packed "
                               "bases (hg_pack2 blobs: codes + not-a-base bitmap, 0.375 B per base)" % N,
                   "genomes_per_gpu": N, "genome_bp": L_GENOME, "parallelism": "genome-sharded x%d, no collective" % world},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                     "kernel": kmer_kernel, "launch_ms": kmer_avg_ms,
                     "algorithmic_bytes_per_launch": bytes_per_launch,
                     "input_bytes_per_launch": int(N * blob_sz),
                     "moved_bytes_per_launch": int(N * (blob_sz + 2 * HV_D)),
                     "frac_of_hbm_peak_moved": N * (blob_sz + 2 * HV_D) / (kmer_avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "note": "algorithmic bytes = SURVEY 8(d)'s L + 2 D per genome (one byte per base in, i16 HV out) whatever "
                             "the resident form; the packed blobs the kernel actually reads are input_bytes_per_launch, and frac_of_hbm_peak_moved prices "
                             "what really crosses HBM (blobs in, HVs out: 2.6x less than the algorithmic bytes). "
                             "Nominally a scan, so priced against HBM; the true binder is integer VALU issue (%s static VALU "
                             "instructions per k-mer, 25 of them the 64-bit multiply-adds of t1ha2; see valu_issue)" % (
                                 ("%.1f" % isa_valu) if isa_valu else "~65"),
                     "valu_issue": valu_issue(N, kmer_kernel),
                     "kmer_hashes_per_sec": N * (L_GENOME + 1 - KSIZE + 1) / (kmer_avg_ms * 1e-3)},
        "kernel_ms_per_step": {k: v[0] / max(a.steps, 1) for k, v in tm.items() if v[1]},
        "host_gap_ms": dt / a.steps * 1e3 - sum(v[0] for v in tm.values() if v[1]) / max(a.steps, 1),
        "host_gap_note": "ms_per_step minus the step's kernels (HIP events around the k-mer, sort and encode launches): what the "
                         "device spends outside every kernel of the step -- launch gaps, the counter memset, and any wait for the host. "
                         "The step queues k-mer -> sort -> encode without a host round trip (hg_sketch_step.hip); its check word is "
                         "read while the NEXT step is already queued",
        "sketch_steps": dict(zip(("sync_free", "synchronous", "rerun"), ctx.sketch_step_counts())),
    }
    if dumped:
        out["dump_outputs"] = dumped
    if not a.full:  # a plain run ends here: every leg below is one that the headline does not need
        finish()
        return

    # the same step on ASCII-resident genomes (1 byte per base in HBM), identical sketches required
    hv_a, n2_a, nh_a = torch.empty_like(hv), torch.empty_like(n2), torch.empty_like(nh)
    settle(step_ascii, 5)
    ctx.enable_timing(True)
    ctx.timings()
    steps_a = max(2, min(a.steps, 10))
    barrier_sync(world)
    t0 = time.perf_counter()
    for _ in range(steps_a):
        step_ascii()
    barrier_sync(world)
    dt_a = max_over_ranks(time.perf_counter() - t0, world, dev)
    tm_a = ctx.timings()
    ctx.enable_timing(False)
    ascii_kernel = ctx.last_kernel("kmer")
    if not (torch.equal(hv_a, hv) and torch.equal(n2_a, n2) and torch.equal(nh_a, nh)):
        raise SystemExit("PARITY GATE FAILED: sketches of the packed and of the ASCII-resident genomes differ")
    ascii_ms = tm_a["kmer"][0] / max(tm_a["kmer"][1], 1)
    log("sketch, ASCII-resident: %.1f genomes/s, kmer kernel %.3f ms/launch" % (N * world * steps_a / dt_a, ascii_ms))
    del hv_a, n2_a, nh_a
    out["ascii_resident"] = {"value": N * world * steps_a / dt_a, "unit": "genomes/sec", "steps": steps_a,
                             "ms_per_step": dt_a / steps_a * 1e3, "kernel": ascii_kernel, "launch_ms": ascii_ms,
                             "frac_of_hbm_peak": bytes_per_launch / (ascii_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             "config": {"workload": "the same %d genomes resident as ASCII (1 B per base, %.1f GB), "
                                                    "hg_sketch_batch_dev; sketches identical to the headline's" % (N, N * stride / 1e9)}}
    out["sketch_steps"] = dict(zip(("sync_free", "synchronous", "rerun"), ctx.sketch_step_counts()))  # (with this leg's steps)

    # ---------------- the inputs real users have (never `value`) ----------------------------------------------------
    # Every timed leg above runs on clean, single-contig, iid-uniform genomes.  (a) `draft_assemblies`: the SAME N genomes
    # rewritten as draft assemblies (draftify: 200 contigs, 30 % soft-masked, 0.05 % IUPAC codes, a 50 kbp tandem repeat) --
    # every tile that holds a non-base takes the kernel's validity-window path, the repeat's k-mers pile up in the hit
    # staging; (b) `many_small`: 100 000 genomes of 50 kbp in one batch (plasmids / viral genomes: the per-genome costs --
    # work-item table, one sort and one encode workgroup per genome -- instead of the per-base ones).  Both in the two
    # resident forms, identical sketches required, three sampled genomes against the CPU oracle.
    def realistic_legs():
        def time_leg(fn, n_gen, reps):
            settle(fn, 5)
            ctx.enable_timing(True)
            ctx.timings()
            dev_sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            dev_sync()
            dtl = time.perf_counter() - t0
            tml = ctx.timings()
            ctx.enable_timing(False)
            return {"value": n_gen * reps / dtl, "unit": "genomes/sec", "steps": reps, "ms_per_step": dtl / reps * 1e3,
                    "kernel": ctx.last_kernel("kmer"), "kernel_ms_per_step": {k: v[0] / reps for k, v in tml.items() if v[1]},
                    "host_gap_ms": dtl / reps * 1e3 - sum(v[0] for v in tml.values() if v[1]) / reps}

        def gate(name, buf, st_, length, hv_t, n2_t, nh_t, picks, scaled=SCALED):
            if a.no_cpu_baseline:
                return "skipped (--no-cpu-baseline)"
            from oracle import oracle as orc
            for g in picks:
                host = buf[g * st_: g * st_ + length + 1].cpu().numpy()
                w_hv, w_n2, w_nh = orc.sketch_genome(host, scaled=scaled)
                if not (int(nh_t[g]) == w_nh and int(n2_t[g]) == w_n2 and np.array_equal(hv_t[g].cpu().numpy(), w_hv)):
                    raise SystemExit("PARITY GATE FAILED: %s, genome %d differs from the CPU oracle" % (name, g))
            return "genomes %s == CPU oracle (hash count, HV, norm)" % (list(picks),)

        reps_r = max(2, min(a.steps, 10))
        seq_r = seq.clone()
        draftify(seq_r, N, stride, L_GENOME)
        blobs_r = torch.empty_like(blobs)
        ctx.pack2_batch_dev(seq_r.data_ptr(), offs, lens, blobs_r.data_ptr(), boffs)
        hv_r, n2_r, nh_r = torch.empty_like(hv), torch.empty_like(n2), torch.empty_like(nh)
        hv_q, n2_q, nh_q = torch.empty_like(hv), torch.empty_like(n2), torch.empty_like(nh)
        r_pk = time_leg(lambda: ctx.sketch_batch_dev_packed(blobs_r.data_ptr(), boffs, lens, p, hv_r.data_ptr(), n2_r.data_ptr(),
                                                            nh_r.data_ptr()), N, reps_r)
        r_as = time_leg(lambda: ctx.sketch_batch_dev(seq_r.data_ptr(), offs, lens, p, hv_q.data_ptr(), n2_q.data_ptr(),
                                                     nh_q.data_ptr()), N, reps_r)
        if not (torch.equal(hv_r, hv_q) and torch.equal(n2_r, n2_q) and torch.equal(nh_r, nh_q)):
            raise SystemExit("PARITY GATE FAILED: draft assemblies, packed and ASCII-resident sketches differ")
        r_pk["vs_clean"] = r_pk["value"] / value
        r_as["vs_clean"] = r_as["value"] / (N * world * steps_a / dt_a)
        out["realistic"] = {"draft_assemblies": dict(
            r_pk, ascii_resident=r_as, nhash_mean=float(nh_r.float().mean().item()),
            parity=gate("draft assemblies", seq_r, stride, L_GENOME, hv_r, n2_r, nh_r, (0, N // 2, N - 1)),
            config={"workload": "the headline's %d genomes as draft assemblies: 200 contigs each (an 'N' per record start, "
                                "src/fastx_reader.rs:6-29), ~30 %% soft-masked in 1 kbp runs, 0.05 %% IUPAC codes, one 50 kbp tandem "
                                "repeat of a 171-base unit; resident as hg_pack2 blobs (ascii_resident: as ASCII)" % N})}
        log("realistic, draft assemblies: %.0f genomes/s packed (%.2f of clean; kmer %.2f ms), %.0f ASCII (%.2f of clean; kmer %.2f ms)" % (
            r_pk["value"], r_pk["vs_clean"], r_pk["kernel_ms_per_step"].get("kmer", 0.0), r_as["value"], r_as["vs_clean"],
            r_as["kernel_ms_per_step"].get("kmer", 0.0)))
        del seq_r, blobs_r, hv_r, n2_r, nh_r, hv_q, n2_q, nh_q
        if a.small_genomes:
            NS, LS = a.small_genomes, 50_000
            st_s = (LS + 1 + 15) // 16 * 16
            seq_s = torch.empty(NS * st_s + 64, dtype=torch.uint8, device=dev)
            ctx.synth_genomes_dev(0, NS, LS, st_s, seq_s.data_ptr())
            offs_s, lens_s = np.arange(NS, dtype=np.uint64) * st_s, np.full(NS, LS + 1, np.uint64)
            bsz_s = hg.lib().hg_pack2_size(LS + 1)
            boffs_s = np.arange(NS, dtype=np.uint64) * bsz_s
            blobs_s = torch.empty(NS * bsz_s + 64, dtype=torch.uint8, device=dev)
            ctx.pack2_batch_dev(seq_s.data_ptr(), offs_s, lens_s, blobs_s.data_ptr(), boffs_s)
            hv_s = torch.empty((NS, HV_D), dtype=torch.int16, device=dev)
            n2_s, nh_s = torch.empty(NS, dtype=torch.int32, device=dev), torch.empty(NS, dtype=torch.int32, device=dev)
            hv_t, n2_t, nh_t = torch.empty_like(hv_s), torch.empty_like(n2_s), torch.empty_like(nh_s)
            s_pk = time_leg(lambda: ctx.sketch_batch_dev_packed(blobs_s.data_ptr(), boffs_s, lens_s, p, hv_s.data_ptr(), n2_s.data_ptr(),
                                                                nh_s.data_ptr()), NS, reps_r)
            s_as = time_leg(lambda: ctx.sketch_batch_dev(seq_s.data_ptr(), offs_s, lens_s, p, hv_t.data_ptr(), n2_t.data_ptr(),
                                                         nh_t.data_ptr()), NS, reps_r)
            if not (torch.equal(hv_s, hv_t) and torch.equal(n2_s, n2_t) and torch.equal(nh_s, nh_t)):
                raise SystemExit("PARITY GATE FAILED: many small genomes, packed and ASCII-resident sketches differ")
            for r_ in (s_pk, s_as):
                r_["mbases_per_sec"] = r_["value"] * LS / 1e6
            s_pk["vs_clean_per_base"] = s_pk["mbases_per_sec"] / (value * L_GENOME / 1e6)
            out["realistic"]["many_small"] = dict(
                s_pk, ascii_resident=s_as, nhash_mean=float(nh_s.float().mean().item()),
                parity=gate("many small genomes", seq_s, st_s, LS, hv_s, n2_s, nh_s, (0, NS // 2, NS - 1)),
                config={"workload": "%d synthetic genomes of %d bp in one batch (%.1f GB as ASCII), k=21 scaled=1500 D=4096; "
                                    "resident as hg_pack2 blobs (ascii_resident: as ASCII)" % (NS, LS, NS * st_s / 1e9)})
            log("realistic, %d x %d bp: %.0f genomes/s packed = %.0f Mbase/s (%.2f of the clean per-base rate), %.0f ASCII; kernels %s" % (
                NS, LS, s_pk["value"], s_pk["mbases_per_sec"], s_pk["vs_clean_per_base"], s_as["value"],
                {k: round(v, 2) for k, v in s_pk["kernel_ms_per_step"].items()}))
            del seq_s, blobs_s, hv_s, n2_s, nh_s, hv_t, n2_t, nh_t

    if not a.no_realistic and world == 1:
        try:
            realistic_legs()
        except SystemExit as e:  # an auxiliary leg: its failure is recorded, the line is still printed, the exit code says so
            if "PARITY GATE FAILED" not in str(e):
                raise
            out.setdefault("realistic", {})["parity"] = "FAILED: " + str(e)
            aux_failures.append(str(e))
            log("AUXILIARY LEG FAILED (line still printed, exit code 4): %s" % e)

    # ---------------- configs[2]: 10 000 genomes TOTAL, sharded over the ranks -------------------------------
    # (the headline above is weak-scaled at 1 000 genomes per GPU; this leg is the fixed-size job BASELINE.json
    # names: rank r sketches genomes shard_range(10 000, r, world), no collective -> "strong" scaling)
    if a.genomes_10k:
        from hypergen_amd import shard
        glo, ghi = shard.shard_range(a.genomes_10k, rank, world)
        M = ghi - glo
        # resident as packed blobs (18.75 GB for 10 000 genomes instead of 50 GB): generated and packed 1 000 at a time
        # through the headline's ASCII buffer
        seq2 = torch.empty(M * blob_sz + 64, dtype=torch.uint8, device=dev)
        boffs2 = np.arange(M, dtype=np.uint64) * blob_sz
        for g0 in range(0, M, N):
            m = min(N, M - g0)
            ctx.synth_genomes_dev(glo + g0, m, L_GENOME, stride, seq.data_ptr())
            ctx.pack2_batch_dev(seq.data_ptr(), offs[:m], lens[:m], seq2.data_ptr() + g0 * blob_sz, boffs[:m])
        ctx.synth_genomes_dev(rank * N, N, L_GENOME, stride, seq.data_ptr())  # (the later legs read the headline's genomes)
        lens2 = np.full(M, L_GENOME + 1, np.uint64)
        hv2 = torch.empty((M, HV_D), dtype=torch.int16, device=dev)
        n22 = torch.empty(M, dtype=torch.int32, device=dev)
        nh2 = torch.empty(M, dtype=torch.int32, device=dev)

        def step2():
            ctx.sketch_batch_dev_packed(seq2.data_ptr(), boffs2, lens2, p, hv2.data_ptr(), n22.data_ptr(), nh2.data_ptr())

        step2()
        steps2 = max(2, min(a.steps, 5))
        barrier_sync(world)
        t0 = time.perf_counter()
        for _ in range(steps2):
            step2()
        barrier_sync(world)
        dt2 = max_over_ranks(time.perf_counter() - t0, world, dev)
        # genomes [glo, ghi) here and genomes [rank*N, rank*N + N) above overlap on rank 0: same sketches expected
        same = min(N, M) if rank == 0 else 0
        if same and not (torch.equal(hv2[:same], hv[:same]) and torch.equal(n22[:same], n2[:same])):
            raise SystemExit("PARITY GATE FAILED: the 10k-genome leg disagrees with the headline leg on shared genomes")
        out["sketch_10k"] = {
            "metric": "genomes/sec sketch (k=21,s=1500,D=4096)", "value": a.genomes_10k * steps2 / dt2,
            "unit": "genomes/sec", "steps": steps2, "ms_per_step": dt2 / steps2 * 1e3, "scaling": "strong",
            "config": {"workload": "%d synthetic 5 Mbp genomes in total (BASELINE configs[2]), rank r sketches "
                                   "shard_range(%d, r, %d); inputs resident in HBM as 2-bit packed bases (%.2f GB per GPU)" % (
                                       a.genomes_10k, a.genomes_10k, world, M * blob_sz / 1e9),
                       "genomes_per_gpu": M, "parallelism": "genome-sharded x%d, no collective" % world}}
        log("sketch_10k: %.1f genomes/s (%d genomes on this rank, %.1f ms per pass)" % (
            out["sketch_10k"]["value"], M, dt2 / steps2 * 1e3))
        real_hv = (hv2, n22) if (world == 1 and a.dist_n and M == a.dist_n) else None  # the dist leg times these too
        del seq2, nh2

    else:
        real_hv = None

    # ---------------- host-fed: the same sketch path from pinned host memory (PCIe-inclusive, never `value`) ---
    if a.hostfed_genomes and rank == 0:
        HF = min(a.hostfed_genomes, N)
        host = torch.empty((HF, L_GENOME + 1), dtype=torch.uint8).pin_memory()
        for g in range(HF):
            host[g].copy_(seq[g * stride: g * stride + L_GENOME + 1])
        host_rows = [host[g].numpy() for g in range(HF)]
        own = hg.Context(local)  # its own stream and staging: hg_sketch_batch uploads while it computes
        h_hv, h_n2, h_nh = own.sketch_batch(host_rows, p)
        if not (np.array_equal(h_hv, hv[:HF].cpu().numpy()) and np.array_equal(h_n2, n2[:HF].cpu().numpy())):
            raise SystemExit("PARITY GATE FAILED: host-fed sketches differ from the HBM-resident ones")
        def median_pass(passes=5):
            """one hg_sketch_batch call over the HF genomes per pass; the median pass (the host is shared: a pass that meets
            another tenant's memory traffic takes up to twice as long)"""
            ts = []
            for _ in range(passes):
                t0 = time.perf_counter()
                own.sketch_batch(host_rows, p)
                ts.append(time.perf_counter() - t0)
            ts.sort()
            return ts[len(ts) // 2]

        reps = 1
        hdt_ = median_pass()
        link_form = "2-bit packed by the library's host threads (0.375 B/base)" if own.last_kernel("kmer").endswith("true>") else "ASCII"
        # the same call with the library told to send ASCII (debug hook "hostfed"): the link-bound rate of round 3
        own.set_debug("hostfed", "ascii")
        a_hv, a_n2, _ = own.sketch_batch(host_rows, p)
        if not (np.array_equal(a_hv, h_hv) and np.array_equal(a_n2, h_n2)):
            raise SystemExit("PARITY GATE FAILED: host-fed sketches depend on the form sent over the link")
        adt_ = median_pass(3)
        own.close()
        gbs = HF * reps * (L_GENOME + 1) / adt_ / 1e9
        out["host_fed"] = {"value": HF * reps / hdt_, "unit": "genomes/sec", "link_form": link_form,
                           "host_threads": min(16, len(os.sched_getaffinity(0))),
                           "ascii_link": {"value": HF * reps / adt_, "unit": "genomes/sec", "pcie_gbs": gbs, "pcie_peak_gbs": 63.0,
                                          "frac_of_pcie": gbs / 63.0},
                           "config": {"workload": "%d of the step's genomes from pinned host memory through "
                                                  "hg_sketch_batch (the library 2-bit packs each sub-batch on its host threads "
                                                  "while the previous one uploads; kernels overlap both), results "
                                                  "back on the host; the median of 5 calls; rank 0 only.  ascii_link: the same call with the bases "
                                                  "sent as ASCII (median of 3)" % HF}}
        log("host-fed: %.0f genomes/s (%s); %.0f genomes/s = %.1f GB/s of sequence over PCIe as ASCII" % (
            out["host_fed"]["value"], link_form, HF * reps / adt_, gbs))
        # the same genomes as hg_pack2 blobs (3 bits per base) through the streaming entry points: what the CLI's
        # readers do when the link is what limits.  Packing is host work of the caller's reader threads and is
        # reported beside the rate, not inside it.
        import threading
        blobs = [None] * HF
        T = min(16, len(os.sched_getaffinity(0)))

        def pack_some(t):
            for g in range(t, HF, T):
                blobs[g] = torch.from_numpy(hg.pack2(host_rows[g])).pin_memory().numpy()
                sp = hg.pack2s(host_rows[g])
                sblobs[g] = None if sp is None else torch.from_numpy(sp).pin_memory().numpy()
        sblobs = [None] * HF
        t0 = time.perf_counter()
        for g in range(min(HF, 2 * T)):  # timing of the packer alone, one thread
            hg.pack2s(host_rows[g])
        pack_ms = (time.perf_counter() - t0) / min(HF, 2 * T) * 1e3
        th = [threading.Thread(target=pack_some, args=(t,)) for t in range(T)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        ref_hv, ref_n2 = hv[:HF].cpu().numpy(), n2[:HF].cpu().numpy()

        stream_reps = 3

        def stream_pass(sparse):
            """the HF genomes through push_packed(_sparse) / pop, best of `stream_reps` passes; returns (seconds, bytes over the link)"""
            with hg.SketchStream((local,), p) as st:
                best = None
                for rep in range(stream_reps + 1):
                    t0 = time.perf_counter()
                    for g in range(HF):
                        if sparse and sblobs[g] is not None:
                            st.push_packed_sparse(sblobs[g], L_GENOME + 1, rep * HF + g)
                        else:
                            st.push_packed(blobs[g], L_GENOME + 1, rep * HF + g)
                    got = {}
                    for _ in range(HF):
                        r = st.pop()
                        got[r[0] - rep * HF] = r
                    dtp = time.perf_counter() - t0
                    if rep:
                        best = dtp if best is None else min(best, dtp)
                st.finish()
            if not all(np.array_equal(got[g][1], ref_hv[g]) and got[g][2] == ref_n2[g] for g in range(HF)):
                raise SystemExit("PARITY GATE FAILED: sketches of the 2-bit packed genomes differ from the HBM-resident ones")
            nbytes = sum((sblobs[g] if sparse and sblobs[g] is not None else blobs[g]).size for g in range(HF))
            return best, nbytes

        best_b, bytes_b = stream_pass(False)
        best, pk_bytes = stream_pass(True)
        out["host_fed"]["packed_stream"] = {
            "value": HF / best, "unit": "genomes/sec", "pcie_gbs": pk_bytes / best / 1e9,
            "bytes_per_base": pk_bytes / (HF * (L_GENOME + 1.0)), "host_pack_ms_per_genome_one_thread": pack_ms,
            "bitmap_form": {"value": HF / best_b, "unit": "genomes/sec", "pcie_gbs": bytes_b / best_b / 1e9,
                            "bytes_per_base": bytes_b / (HF * (L_GENOME + 1.0))},
            "config": {"workload": "the same %d genomes as hg_pack2s blobs (2-bit codes + a table of the not-a-base runs: "
                                   "0.25 B per base over the link) from pinned memory through "
                                   "hg_sketch_stream_push_packed_sparse / pop -- the device rebuilds the bitmap and the blobs go "
                                   "to the packed-input kernels as they arrive --, best of %d passes; packing time not "
                                   "included.  bitmap_form: the same through hg_pack2 blobs (0.375 B per base)" % (HF, stream_reps)}}
        log("host-fed, 2-bit packed stream: %.0f genomes/s sparse (%.1f GB/s over PCIe), %.0f genomes/s bitmap form (%.1f GB/s); "
            "host packing %.2f ms per genome and thread" % (HF / best, pk_bytes / best / 1e9, HF / best_b, bytes_b / best_b / 1e9, pack_ms))
        # ---- per_call: the literal drop-in of the reference's inner seam (src/sketch_cuda.rs:79-96,120-166) ------
        # T host threads (the reference's rayon workers), each with its OWN hg_ctx on this GPU, one synchronous
        # hg_kmer_hash_sample call per genome from pinned memory, the sampled hash list back on the host -- what a
        # Rust caller sees that only swaps `extract_kmer_t1ha2_cuda` for the C ABI (HV encode left where the
        # reference has it).  `sketch_one` is the same pattern through hg_sketch_batch with n = 1 (HV on the device).
        PT = min(16, len(os.sched_getaffinity(0)), HF)
        dev_node = hg.lib().hg_device_numa_node(local)
        pc_ctx = [hg.Context(local) for _ in range(PT)]
        thr = (2**64 - 1) // SCALED
        want_nh = nh[:HF].cpu().numpy()

        def run_threads(fn):
            bad = []

            def w(t):
                try:
                    hg.lib().hg_bind_thread_to_numa_node(dev_node, PT)  # (what the CLI does for its reader threads)
                    for g in range(t, HF, PT):
                        fn(pc_ctx[t], g)
                except Exception as e:  # pragma: no cover
                    bad.append(repr(e))
            ths = [threading.Thread(target=w, args=(t,)) for t in range(PT)]
            t0 = time.perf_counter()
            for x in ths:
                x.start()
            for x in ths:
                x.join()
            if bad:
                raise SystemExit("per_call leg failed: " + bad[0])
            return time.perf_counter() - t0

        got_n = np.zeros(HF, np.int64)
        outs = [np.zeros(8192, np.uint64) for _ in range(PT)]

        def call_sample(c, g):
            n = hg.C.c_size_t(0)
            c._ck(hg.lib().hg_kmer_hash_sample(c._h, hg._ptr(host_rows[g]), host_rows[g].size, KSIZE, hg.C.c_uint64(thr),
                                               hg.C.c_uint64(p.seed), 1, 0, hg._ptr(outs[g % PT]), 8192, hg.C.byref(n)))
            got_n[g] = n.value

        def call_sketch(c, g):
            c.sketch_batch([host_rows[g]], p)

        def timed(fn, passes=7):
            """median pass time after two untimed passes (workspaces, plan caches, page-locked staging; the first passes of
            a fresh pool of contexts also see 15 ms stalls in single calls that later ones do not)"""
            run_threads(fn)
            run_threads(fn)
            ts = sorted(run_threads(fn) for _ in range(passes))
            return ts[len(ts) // 2], ts[0]

        run_threads(call_sample)  # warm-up (workspaces, plan caches)
        if not np.array_equal(got_n, want_nh):
            raise SystemExit("PARITY GATE FAILED: per-call hash counts differ from the batch's")
        dt_s, dt_s_best = timed(call_sample)
        n_pk = sum(c.last_kernel("kmer").endswith("true>") for c in pc_ctx)
        pc_form = "the library's measured choice: %d of the %d threads' last calls went 2-bit packed by the calling thread, the others ASCII" % (n_pk, PT)
        dt_k, _ = timed(call_sketch, 5)
        for c in pc_ctx:
            c.set_debug("hostfed", "ascii")
        run_threads(call_sample)
        if not np.array_equal(got_n, want_nh):
            raise SystemExit("PARITY GATE FAILED: per-call hash counts differ from the batch's")
        dt_a, _ = timed(call_sample, 5)
        for c in pc_ctx:
            c.close()
        out["per_call"] = {"value": HF / dt_s, "unit": "genomes/sec", "best_pass": HF / dt_s_best, "passes": 7, "threads": PT, "link_form": pc_form,
                           "sketch_one": {"value": HF / dt_k, "unit": "genomes/sec"},
                           "ascii_link": {"value": HF / dt_a, "unit": "genomes/sec", "pcie_gbs": HF * (L_GENOME + 1) / dt_a / 1e9},
                           "config": {"workload": "%d of the step's genomes from pinned host memory, ONE synchronous "
                                                  "hg_kmer_hash_sample call per genome (hash list back on the host) "
                                                  "from %d host threads (bound to the device's NUMA node, "
                                                  "hg_bind_thread_to_numa_node) with one hg_ctx each on this GPU -- the "
                                                  "reference's rayon pattern, src/sketch_cuda.rs:79-96; sketch_one = "
                                                  "hg_sketch_batch with n = 1 in the same pattern; ascii_link = "
                                                  "hg_kmer_hash_sample with the bases sent as ASCII; every figure the median of "
                                                  "its timed passes over the %d genomes; rank 0 only" % (HF, PT, HF)}}
        log("per_call: %.0f genomes/s through hg_kmer_hash_sample on %d threads (%s), %.0f through hg_sketch_batch(n=1); %.0f as ASCII (%.1f GB/s)" % (
            HF / dt_s, PT, pc_form, HF / dt_k, HF / dt_a, out["per_call"]["ascii_link"]["pcie_gbs"]))
        del host, blobs

    # ---------------- dist: R x Q ANI matrix, thresholded ------------------------------------------
    if a.dist_n:
        R = a.dist_n
        rows = R // world
        mine = clustered_hvs(rows, rank * rows, dev)
        mine_n2 = (mine.int() ** 2).sum(1).int()
        cap = max(1 << 20, rows * R // 20)
        hits = torch.empty(cap * 3, dtype=torch.int32, device=dev)  # hg_ani_hit = 12 bytes
        R_all = rows * world
        if coll:
            ref_all = torch.empty((R_all, HV_D), dtype=torch.int16, device=dev)
            ref_n2 = torch.empty(R_all, dtype=torch.int32, device=dev)
            # The exchange moves PREPARED operands: every rank converts its own reference rows to centred byte operands +
            # control records once (hg_dist_prep_ops_dev) and all-gathers those -- 4.3 KB per row instead of 8 KB of i16, and
            # no rank repeats another rank's prepass.  The rows travel in `chunks` row blocks per rank; the GEMM of chunk c
            # (all ranks' block c x this rank's query rows, global reference indices through an index map) runs while
            # chunk c + 1 is in flight.  A veto on any rank (sketches that do not fit the byte scheme) falls back to the
            # all-gather of the i16 rows for that step.
            chunks = max(1, min(a.dist_chunks, rows))
            rb_, mb_ = hg.lib().hg_dist_ops_row_bytes(HV_D), hg.lib().hg_dist_ops_meta_bytes()
            my_ops = torch.empty((rows, rb_), dtype=torch.uint8, device=dev)
            my_meta = torch.empty((rows, mb_), dtype=torch.uint8, device=dev)
            my_flag = torch.zeros(4, dtype=torch.int32, device=dev)  # [0] the flag word (+ padding to 16 bytes)
            cb = [(c * rows // chunks, (c + 1) * rows // chunks) for c in range(chunks)]  # this rank's row range per chunk
            wbytes = [(hi - lo) * (4 + mb_) + 16 for lo, hi in cb]                         # norms | records | flag
            ops_all = [torch.zeros((hg.lib().hg_dist_ops_padded_rows((hi - lo) * world), rb_), dtype=torch.uint8, device=dev) for lo, hi in cb]
            words_all = [torch.empty(world * w, dtype=torch.uint8, device=dev) for w in wbytes]
            ref_index = [torch.cat([torch.arange(r * rows + lo, r * rows + hi, dtype=torch.int32) for r in range(world)]).to(dev)
                         for lo, hi in cb]
        found = 0
        fallbacks = 0

        def gather_bytes(dst, src):
            """all-gather of raw bytes (RCCL has no int16 datatype and the payloads are opaque); returns a work handle"""
            if a.backend == "nccl":
                return torch.distributed.all_gather_into_tensor(dst.view(-1), src.view(-1), async_op=True)
            h_dst = torch.empty(dst.numel(), dtype=torch.uint8)  # gloo (testing aid): the same collective on host copies
            torch.distributed.all_gather_into_tensor(h_dst, src.reshape(-1).cpu())
            dst.view(-1).copy_(h_dst)
            return None

        def gather_i16():
            for w in (gather_bytes(ref_all.view(torch.uint8), mine.view(torch.uint8)), gather_bytes(ref_n2.view(torch.uint8), mine_n2.view(torch.uint8))):
                if w is not None:
                    w.wait()

        def dstep():
            nonlocal found, fallbacks
            if not coll:
                found, _ = ctx.dist_dev(mine.data_ptr(), mine_n2.data_ptr(), rows, mine.data_ptr(), mine_n2.data_ptr(), rows,
                                        HV_D, KSIZE, False, 85.0, hits.data_ptr(), cap)
                return
            ctx.dist_prep_ops_dev(mine.data_ptr(), rows, HV_D, my_ops.data_ptr(), my_meta.data_ptr(), my_flag.data_ptr())
            works = []
            for c, (lo, hi) in enumerate(cb):  # every chunk's exchange is queued at once, in order
                words = torch.cat([mine_n2[lo:hi].view(torch.uint8).view(-1), my_meta[lo:hi].view(-1), my_flag.view(torch.uint8)])
                works.append((gather_bytes(ops_all[c][: (hi - lo) * world], my_ops[lo:hi]), gather_bytes(words_all[c], words)))
            total, vetoed = 0, False
            for c, (lo, hi) in enumerate(cb):
                for w in works[c]:
                    if w is not None:
                        w.wait()  # (the compute stream waits; the host does not)
                m = hi - lo
                wv = words_all[c].view(world, wbytes[c])
                n2_c = wv[:, : 4 * m].contiguous().view(torch.int32).view(-1)
                meta_c = wv[:, 4 * m: 4 * m + m * mb_].contiguous()
                flags_c = wv[:, 4 * m + m * mb_: 4 * m + m * mb_ + 4].contiguous().view(torch.int32).view(-1)
                n, st = ctx.dist_block_ops_dev(ops_all[c].data_ptr(), meta_c.data_ptr(), n2_c.data_ptr(), m * world, 0,
                                               ref_index[c].data_ptr(), flags_c.data_ptr(), world, mine.data_ptr(), mine_n2.data_ptr(),
                                               rows, rank * rows, HV_D, KSIZE, False, 85.0, hits.data_ptr() + 12 * total, cap - total)
                if st == hg.ERR_INEXACT:
                    vetoed = True
                    break
                if st != 0:
                    raise SystemExit("dist hit buffer too small")
                total += n
            if vetoed:  # every rank sees the same flags; a query-side veto is this rank's alone -- either way: the i16 rows
                fallbacks += 1
                gather_i16()
                total, st = ctx.dist_block_dev(ref_all.data_ptr(), ref_n2.data_ptr(), R_all, 0, mine.data_ptr(), mine_n2.data_ptr(), rows,
                                               rank * rows, HV_D, KSIZE, False, 85.0, hits.data_ptr(), cap)
            found = total

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dstep()
        torch.cuda.synchronize()
        dist_first_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        dstep()
        torch.cuda.synchronize()
        dist_second_ms = (time.perf_counter() - t0) * 1e3
        settle(dstep, SETTLE["dist"])
        for _ in range(max(a.warmup, 1)):
            dstep()
        ctx.enable_timing(True)
        ctx.timings()
        barrier_sync(world)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            dstep()
        barrier_sync(world)
        ddt = max_over_ranks(time.perf_counter() - t0, world, dev)
        dtm = ctx.timings()
        ctx.enable_timing(False)
        if coll:  # the prepared-operand exchange against the i16 exchange: same hit set (outside the timed region)
            got = hits[: 3 * found].view(-1, 3).clone()
            gather_i16()
            n16, st16 = ctx.dist_block_dev(ref_all.data_ptr(), ref_n2.data_ptr(), R_all, 0, mine.data_ptr(), mine_n2.data_ptr(), rows,
                                           rank * rows, HV_D, KSIZE, False, 85.0, hits.data_ptr(), cap)
            ref16 = hits[: 3 * n16].view(-1, 3)

            def canon(h):
                k = h[:, 0].long() * (1 << 32) + h[:, 1].long()
                return h[torch.argsort(k)]
            if st16 != 0 or n16 != found or not torch.equal(canon(got), canon(ref16)):
                raise SystemExit("PARITY GATE FAILED: prepared-operand exchange and i16 exchange disagree (%d vs %d hits)" % (found, n16))
            dstep()  # (the timed path's hits back in `hits` for the gates below)
        pairs = (rows * world) * rows * world  # all ranks together cover R x Q
        # GEMM time per step: the sum of the bracketed launches of the class (an i8 attempt queues its GEMM and, behind
        # it, the vetoed f16 kernels that return at once -- all of it is the price of one pass)
        gemm_ms = dtm["dist"][0] / max(a.steps, 1)
        flops_per_launch = 2.0 * HV_D * (rows * world) * rows  # 2*D ops per pair
        ach = flops_per_launch / (gemm_ms * 1e-3) / 1e12
        dist_kernel = ctx.last_kernel("dist")
        # bytes leaving the XCD L2s per launch (PMC, profiles/): 10 000 x 10 000 on one GPU only
        dist_traffic, dist_traffic_src = None, "not the profiled shape (10 000 x 10 000 on one GPU)"
        if rows * world == 10000 and world == 1:
            dd, dist_traffic_src = profiled("_dist_traffic.json", dist_kernel)
            dist_traffic = dd.get("hbm_bytes_per_launch") if dd else None
        path = ctx.last_dist_path()  # 1: centred i8 operands (v_mfma_i32_16x16x64_i8), 0: f16 operands; same integers
        peak = MFMA_F16_PEAK_TFLOPS * (2.0 if path == 1 else 1.0)  # dense i8 MFMA = 2x the f16 rate (MI355X_MICROARCH.md)
        out["dist"] = {
            "metric": "M ANI-pairs/sec (D=4096, ani_th=85)", "value": pairs * a.steps / ddt / 1e6,
            "unit": "M ANI-pairs/sec", "ms_per_step": ddt / a.steps * 1e3, "scaling": "strong",
            "cold_start": {"first_step_ms": dist_first_ms, "second_step_ms": dist_second_ms},
            "config": {"workload": "%d ref x %d query clustered synthetic HVs (BASELINE configs[3]), thresholded "
                                   "output" % (rows * world, rows * world), "hits_per_rank": int(found)},
            "exchange": ({"form": "prepared byte operands + control records, all-gathered in %d row chunks per rank, GEMM of chunk c "
                                  "under the exchange of chunk c + 1" % chunks,
                          "bytes_per_rank_per_step": int(rows * (rb_ + mb_ + 4) + 16 * chunks), "i16_form_bytes": int(rows * (2 * HV_D + 4)),
                          "fallbacks_to_i16": fallbacks, "checked_against_i16_exchange": True,
                          "note": "unmeasured on more than one physical GPU until an 8-GPU node runs it"} if coll else None),
            "roofline": {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                         "frac": ach / peak, "traffic": dist_traffic, "traffic_source": dist_traffic_src,
                         "kernel": dist_kernel, "operands": "i8" if path == 1 else "f16",
                         "peak_dtype": "i8 dense MFMA" if path == 1 else "f16 dense MFMA",
                         "frac_of_f16_peak": ach / MFMA_F16_PEAK_TFLOPS,
                         "launch_ms": gemm_ms, "algorithmic_flops_per_launch": flops_per_launch,
                         "note": "the peak is the nominal one (2.4 GHz); the kernel's loop shape sustains 0.63-0.78 of it on "
                                 "random operand bytes because the chip lowers the shader clock to 1.7-2.0 GHz "
                                 "(profiles/r03_mfma_ceiling.txt, tools/mfma_microbench.hip; DESIGN.md 4.3)"},
            "kernel_ms_per_step": {k: v[0] / max(a.steps, 1) for k, v in dtm.items() if v[1]},
        }
        log("dist: %.0f M pairs/s, gemm %.3f ms/launch = %.1f TFLOP/s, hits/rank %d" % (
            out["dist"]["value"], gemm_ms, ach, found))
        # ---- the same matrix size measured the two other ways a user reaches it (N = 1; never the dist `value`) -----------
        # `dist` above passes ONE buffer as references and queries (the same 10 000 HVs on both sides): the
        # library recognises that, prepares the operands once and both GEMM operands are one matrix.
        #   two_sets : R and Q are DIFFERENT members of the same clusters in different buffers (`hyper-gen dist -r A -q B`):
        #              both prepasses, two operand matrices, the same ~1.3 M hits;
        #   symmetric: one set with symmetric = 1, the reference's path_r == path_q case (src/dist.rs:13,243-265):
        #              R (R - 1) / 2 pairs, tiles below the diagonal never start.
        if not coll and world == 1 and not a.no_dist_variants:
            other = clustered_hvs(rows, 0, dev, salt=1)
            other_n2 = (other.int() ** 2).sum(1).int()

            def variant(qv, qn, sym, pairs_v, what):
                got = 0

                def vstep():
                    nonlocal got
                    got, _ = ctx.dist_dev(mine.data_ptr(), mine_n2.data_ptr(), rows, qv.data_ptr(), qn.data_ptr(), rows, HV_D, KSIZE,
                                          sym, 85.0, hits.data_ptr(), cap)
                settle(vstep, 100)
                ctx.enable_timing(True)
                ctx.timings()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    vstep()
                torch.cuda.synchronize()
                vdt = time.perf_counter() - t0
                vtm = ctx.timings()
                ctx.enable_timing(False)
                vg = vtm["dist"][0] / max(a.steps, 1)
                vpath = ctx.last_dist_path()
                vpeak = MFMA_F16_PEAK_TFLOPS * (2.0 if vpath == 1 else 1.0)
                vach = 2.0 * HV_D * pairs_v / (vg * 1e-3) / 1e12
                return {"value": pairs_v * a.steps / vdt / 1e6, "unit": "M ANI-pairs/sec", "ms_per_step": vdt / a.steps * 1e3,
                        "pairs": pairs_v, "hits": int(got), "gemm_ms": vg, "prep_ms": vtm["dist_prep"][0] / max(a.steps, 1),
                        "tflops": vach, "frac_of_peak": vach / vpeak, "operands": "i8" if vpath == 1 else "f16",
                        "kernel": ctx.last_kernel("dist"), "config": {"workload": what}}

            out["dist"]["two_sets"] = variant(other, other_n2, False, rows * rows,
                                              "%d refs x %d queries in DIFFERENT buffers: the queries are other members of the references' "
                                              "clusters (clustered_hvs(salt=1)), thresholded at 85" % (rows, rows))
            # (gate: the two-set hits against a CPU block, outside the timed region)
            two_hits = hits[: 3 * out["dist"]["two_sets"]["hits"]].clone()
            out["dist"]["symmetric"] = variant(mine, mine_n2, True, rows * (rows - 1) // 2,
                                               "the %d HVs against themselves with symmetric = 1 (i < j only; src/dist.rs:243-265)" % rows)
            out["dist"]["two_sets"]["vs_same_set_gemm"] = out["dist"]["two_sets"]["gemm_ms"] / gemm_ms
            log("dist two_sets: %.0f M pairs/s, gemm %.3f ms (%.2f x the same-set kernel), prep %.3f ms, hits %d; symmetric: %.0f M pairs/s, gemm %.3f ms, hits %d" % (
                out["dist"]["two_sets"]["value"], out["dist"]["two_sets"]["gemm_ms"], out["dist"]["two_sets"]["vs_same_set_gemm"],
                out["dist"]["two_sets"]["prep_ms"], out["dist"]["two_sets"]["hits"], out["dist"]["symmetric"]["value"],
                out["dist"]["symmetric"]["gemm_ms"], out["dist"]["symmetric"]["hits"]))
            if out["dist"]["symmetric"]["hits"] * 2 + rows != int(found):  # every i < j hit twice + the diagonal
                raise SystemExit("PARITY GATE FAILED: symmetric hits %d x 2 + %d != same-set hits %d" % (out["dist"]["symmetric"]["hits"], rows, found))
            dstep()  # the same-set leg's hits back in `hits` for the gates below
        else:
            other = None
        # the same call on the 10 000 REAL sketches of the sketch_10k leg (N = 1 only: they are all on this GPU): clusters
        # of 100 genomes at 0 - 9.9 % substitutions, so ani_th = 85 keeps about the within-cluster pairs
        if real_hv is not None:
            r_hv, r_n2 = real_hv
            rfound = 0

            def rstep():
                nonlocal rfound
                rfound, _ = ctx.dist_dev(r_hv.data_ptr(), r_n2.data_ptr(), R, r_hv.data_ptr(), r_n2.data_ptr(), R, HV_D, KSIZE,
                                         False, 85.0, hits.data_ptr(), cap)
            settle(rstep, 50)
            ctx.enable_timing(True)
            ctx.timings()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                rstep()
            torch.cuda.synchronize()
            rdt = time.perf_counter() - t0
            rtm = ctx.timings()
            ctx.enable_timing(False)
            rg_ms = rtm["dist"][0] / max(a.steps, 1)
            out["dist"]["dist_real"] = {
                "value": R * R * a.steps / rdt / 1e6, "unit": "M ANI-pairs/sec", "ms_per_step": rdt / a.steps * 1e3,
                "gemm_ms": rg_ms, "tflops": 2.0 * HV_D * R * R / (rg_ms * 1e-3) / 1e12, "hits": int(rfound),
                "kernel": ctx.last_kernel("dist"), "operands": "i8" if ctx.last_dist_path() == 1 else "f16",
                "config": {"workload": "the %d x %d ANI matrix of the sketch_10k leg's own sketches (synthetic 5 Mbp genomes, "
                                       "clusters of 100), thresholded at 85" % (R, R)}}
            real_hits = hits[: 3 * rfound].clone()
            log("dist_real: %.0f M pairs/s, gemm %.3f ms, hits %d" % (out["dist"]["dist_real"]["value"], rg_ms, rfound))
            dstep()  # the synthetic leg's hits back in `hits` for the parity gate below

    # ---------------- bit-packed D=16384 Hamming search (BASELINE configs[4], extension) -------------------
    # Sharded database search: the references are sharded by rows, ONE query set lives on rank 0
    # and is broadcast (RCCL) inside every step, every rank searches its shard, the hit lists (global
    # indices) are gathered and merged.  N = 1 runs the same code without the collectives.
    if a.hamming_refs:
        from hypergen_amd import shard
        HD, HQ, HMAX = 16384, a.hamming_queries, 2000
        words = HD // 32
        lo, hi = shard.shard_range(a.hamming_refs, rank, world)
        refs = hi - lo
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x48480000 + rank)
        rb = torch.randint(-2**31, 2**31 - 1, (refs, words), dtype=torch.int32, device=dev, generator=gen)
        qb = torch.zeros((HQ, words), dtype=torch.int32, device=dev)  # only rank 0 fills it
        src_rows = None
        if rank == 0:  # queries = rank 0's own rows with one flipped bit per word (512 of 16 384 bits)
            src_rows = torch.randint(0, refs, (HQ,), device=dev, generator=gen)
            qb = rb[src_rows] ^ (1 << torch.randint(0, 31, (HQ, words), device=dev, generator=gen)).int()
            qsrc = qb.clone()
        hcap = max(1 << 20, 4 * HQ)
        hh = torch.empty(hcap * 3, dtype=torch.int32, device=dev)
        merged = None

        def search_block(ref_local, ref_lo, queries):
            n, st = ctx.hamming_search_block_dev(ref_local.data_ptr(), ref_local.shape[0], ref_lo, queries.data_ptr(),
                                                 queries.shape[0], 0, HD, HMAX, hh.data_ptr(), hcap)
            if st != 0:
                raise SystemExit("hamming hit buffer too small")
            return hh[: 3 * n].cpu().numpy().view(hg.HAM_HIT_DTYPE)

        def hstep():
            nonlocal merged
            if coll and rank == 0:
                qb.copy_(qsrc)  # (the broadcast is in place; rank 0 re-publishes its query set every step)
            if a.backend == "nccl" or not coll:
                merged = shard.sharded_search(search_block, rb, lo, qb, world, dev, force=coll)
            else:  # gloo (testing aid): broadcast / gather on host copies
                hq = qb.cpu()
                shard.broadcast_rows(hq, world, 0, force=coll)
                qb.copy_(hq)
                merged = shard.gather_records(search_block(rb, lo, qb), world, cdev, force=coll)

        settle(hstep, SETTLE["hamming"])
        hstep()
        ctx.enable_timing(True)
        ctx.timings()
        barrier_sync(world)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            hstep()
        barrier_sync(world)
        hdt = max_over_ranks(time.perf_counter() - t0, world, dev)
        htm = ctx.timings()
        ctx.enable_timing(False)
        if rank == 0:  # in-run check: every query finds exactly its source row (global index), at distance 512
            order = np.argsort(merged["qry_idx"], kind="stable")
            ok = merged.size == HQ and np.array_equal(merged["qry_idx"][order], np.arange(HQ)) and \
                np.array_equal(merged["ref_idx"][order], src_rows.cpu().numpy() + lo) and bool((merged["dist"] == words).all())
            if not ok:
                raise SystemExit("PARITY GATE FAILED: merged Hamming hits != the queries' source rows")
        # roofline of the search.  The library runs large searches as an exact +-1 GEMM on the matrix pipe (G = D -
        # 2*distance): on e2m1 operands (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales; path 2) against the dense
        # FP4 MFMA peak, or on byte operands (v_mfma_i32_16x16x64_i8; path 1, test hook only) against the dense i8 peak
        # (MI355X_MICROARCH.md: ~10 / ~5 PFLOP/s); algorithmic flops = 2 * D per pair either way.  The xor + popcount
        # kernel (small searches) is priced in lane-ops: one v_xor_b32 + one v_bcnt_u32_b32 per 32 dims and pair against
        # the issue rate of that pair (3.1 ns per wave-instruction pair and SIMD, tools/gpu_microbench.hip).
        # Compulsory bytes: every packed row once.
        hpath = ctx.last_hamming_path()
        prep_ms = htm["dist_prep"][0] / max(a.steps, 1)
        hms = htm["dist"][0] / max(a.steps, 1)
        if hpath in (1, 2):
            flops = 2.0 * HD * refs * HQ
            hpeak = MFMA_F16_PEAK_TFLOPS * (4.0 if hpath == 2 else 2.0)
            hroof = {"bound": "mfma", "achieved": flops / (hms * 1e-3) / 1e12, "peak": hpeak,
                     "unit": "TFLOP/s", "frac": flops / (hms * 1e-3) / 1e12 / hpeak,
                     "peak_dtype": "FP4 dense MFMA" if hpath == 2 else "i8 dense MFMA",
                     "frac_of_i8_peak": flops / (hms * 1e-3) / 1e12 / (2 * MFMA_F16_PEAK_TFLOPS),
                     "kernel": "dist_mfma_kernel (+-1.0 e2m1 operands, Hamming epilogue)" if hpath == 2 else
                               "dist_mfma_kernel (+-1 byte operands, Hamming epilogue)",
                     "launch_ms": hms, "expand_ms": prep_ms, "algorithmic_flops_per_launch": flops}
        else:
            word_ops = 2.0 * refs * HQ * words
            pair_bound = 1024 * 128 / 3.1e-9
            hroof = {"bound": "valu", "achieved": word_ops / (hms * 1e-3) / 1e12, "peak": pair_bound / 1e12,
                     "unit": "T lane-ops/s (xor + popcount)", "frac": word_ops / (hms * 1e-3) / pair_bound,
                     "kernel": "hamming_kernel", "launch_ms": hms, "algorithmic_lane_ops_per_launch": word_ops}
        # HBM-side bytes per launch of the search kernel from the newest committed PMC pass of this command (only
        # for the shape that pass was taken on: all 50 000 refs x 10 000 queries on one GPU)
        ham_kernel = ctx.last_kernel("dist")
        ham_traffic, ham_traffic_src = None, "not the profiled shape (50 000 x 10 000 on one GPU)"
        if hpath in (1, 2) and world == 1 and a.hamming_refs == 50000 and HQ == 10000:
            hd, ham_traffic_src = profiled("_pmc.json", ham_kernel)
            ham_traffic = hd.get(ham_kernel, {}).get("hbm_bytes_per_launch") if hd else None
        hroof["kernel_symbol"] = ham_kernel
        hroof.update(compulsory_bytes_per_launch=(refs + HQ) * words * 4,
                     compulsory_gbs=(refs + HQ) * words * 4 / (hms * 1e-3) / 1e9, traffic=ham_traffic,
                     traffic_source=ham_traffic_src)
        out["hamming"] = {
            "metric": "M Hamming-pairs/sec (D=16384 bit-packed)", "value": a.hamming_refs * HQ * a.steps / hdt / 1e6,
            "unit": "M pairs/sec", "ms_per_step": hdt / a.steps * 1e3, "scaling": "strong",
            "config": {"workload": "%d ref x %d query sign-binarised D=16384 HVs, popcount(xor) <= %d (BASELINE "
                                   "configs[4]; extension, no reference counterpart); refs sharded x%d, one query "
                                   "set broadcast from rank 0, hits merged" % (a.hamming_refs, HQ, HMAX, world),
                       "hits_merged": int(merged.size), "refs_per_rank": refs},
            "roofline": hroof, "kernel_ms": hms,
        }
        log("hamming: %.0f M pairs/s, kernel %.3f ms (%s, %.0f %% of its bound), merged hits %d" % (
            out["hamming"]["value"], hms, {1: "matrix pipe, i8", 2: "matrix pipe, FP4"}.get(hpath, "xor+popcount"),
            100 * out["hamming"]["roofline"]["frac"], merged.size))
        del rb, qb, hh

    # ---------------- end to end through the CLI (--cli; rank 0, N = 1) ----------------------------------------------
    # `hyper-gen dist` / `search` as a user starts them (src/dist.rs:11-63, src/utils.rs:260-308): .sketch files in, TSV
    # out, process start and HIP bring-up included -- a child process (tools/cli_dist_bench.py), never a re-exec.
    if not a.no_cli and rank == 0 and world == 1 and a.dist_n:
        import subprocess
        torch.cuda.synchronize()
        try:  # (a measurement beside the line, never a reason to lose the line)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cli_dist_bench.py"), "--n", str(a.dist_n),
                                "--sketch-files", str(a.cli_sketch_files)],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(r.stderr.decode()[-1500:])
            out["cli"] = json.loads(r.stdout.decode().strip().splitlines()[-1])
            out["cli"]["source_sha"] = hg.cli_source_stamp()  # library sources + hg_cli.cpp: measured in THIS run on this tree
            log("cli: dist -r A -q A %.2f s, dist -r A -q B %.2f s, search %.2f s (wall, %d sketches)" % (
                out["cli"]["dist_symmetric"]["wall_s"], out["cli"]["dist_two_files"]["wall_s"],
                [v for k, v in out["cli"].items() if k.startswith("search")][0]["wall_s"], a.dist_n))
            if "sketch" in out["cli"]:
                log("cli: sketch -p DIR %.2f s wall for %d FASTA files of 5 Mbp = %.0f files/s (%.1f GB/s of FASTA, process start included)" % (
                    out["cli"]["sketch"]["wall_s"], out["cli"]["sketch"]["files"], out["cli"]["sketch"]["files_per_s"],
                    out["cli"]["sketch"]["fasta_gb_per_s"]))
        except Exception as e:  # pragma: no cover
            out["cli"] = {"error": repr(e)[:2000]}
            log("cli leg failed: %r" % (e,))

    # ---------------- CPU baseline (rank 0, single-GPU runs only) ----------------------------------
    # The same leg is the run's parity gate ("parity gates must pass before any number is
    # reported"): the oracle's outputs, which it produces anyway, are compared with this run's GPU results
    # outside every timed region; a mismatch aborts without printing the line.
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        from oracle import oracle as orc
        # ANI: EQUAL to the oracle's (the device evaluates glibc's logf, the oracle calls it) -- north_star would allow 1e-4
        gate = {"sketch_genomes": [], "tolerance_ani": 0.0}
        for g in (0, N // 2, N - 1):
            host = seq[g * stride: g * stride + L_GENOME + 1].cpu().numpy()
            w_hv, w_n2, w_nh = orc.sketch_genome(host)
            hs = ctx.kmer_hash_sample(host, KSIZE, SCALED)
            if not (np.array_equal(hs, orc.kmer_hash_sample(host, KSIZE, SCALED)) and int(nh[g]) == w_nh and
                    int(n2[g]) == w_n2 and np.array_equal(hv[g].cpu().numpy(), w_hv)):
                raise SystemExit("PARITY GATE FAILED: sketch of genome %d differs from the CPU oracle" % g)
            gate["sketch_genomes"].append(g)
        out["cpu_baseline"] = cpu_baseline_sketch(a.cpu_seconds, log)
        out["speedup_vs_cpu_baseline"] = value / out["cpu_baseline"]["value"]
        if a.dist_n:
            block, cb = cpu_baseline_dist(mine, mine_n2, min(a.cpu_seconds, 6.0), log)
            br, bq = block.shape
            gpu_block = torch.empty((br, bq), dtype=torch.float32, device=dev)
            ctx.dist_full_dev(mine.data_ptr(), mine_n2.data_ptr(), br, mine.data_ptr(), mine_n2.data_ptr(), bq, HV_D, KSIZE,
                              gpu_block.data_ptr())
            torch.cuda.synchronize()
            gb = gpu_block.cpu().numpy()
            err = float(np.abs(gb - block).max())
            # ... and the thresholded hits of the timed runs against the same CPU block
            hh_ = hits[: 3 * found].view(-1, 3)
            sel = (hh_[:, 0] < br) & (hh_[:, 1] < bq)
            hr, hq = hh_[sel, 0].long().cpu().numpy(), hh_[sel, 1].long().cpu().numpy()
            ha = hh_[sel, 2].contiguous().view(torch.float32).cpu().numpy()
            herr = float(np.abs(ha - block[hr, hq]).max()) if hr.size else 0.0
            n_cpu_hits = int((block >= np.float32(85.0)).sum())
            if err != 0.0 or herr != 0.0 or hr.size != n_cpu_hits:
                raise SystemExit("PARITY GATE FAILED: ANI block max |gpu - cpu| = %g, hits %g, %d < %d" % (err, herr, hr.size, n_cpu_hits))
            gate.update(ani_block="%d x %d" % (br, bq), ani_max_abs_err=err, ani_hits_checked=int(hr.size), ani_hits_max_abs_err=herr)
            if other is not None:  # ... and the two-set leg's hits against a 512 x 2 048 CPU block of (refs x other set)
                tb = orc.ani_matrix(mine[:512].cpu().numpy(), mine_n2[:512].cpu().numpy(), other[:2048].cpu().numpy(),
                                    other_n2[:2048].cpu().numpy(), KSIZE)
                th_ = two_hits.view(-1, 3)
                sel = (th_[:, 0] < 512) & (th_[:, 1] < 2048)
                hr, hq = th_[sel, 0].long().cpu().numpy(), th_[sel, 1].long().cpu().numpy()
                ha = th_[sel, 2].contiguous().view(torch.float32).cpu().numpy()
                terr = float(np.abs(ha - tb[hr, hq]).max()) if hr.size else 0.0
                if terr != 0.0 or hr.size != int((tb >= np.float32(85.0)).sum()):
                    aux_failures.append("PARITY GATE FAILED: two-set dist: max |gpu - cpu| = %g, %d hits" % (terr, hr.size))
                    out["dist"]["two_sets"]["parity"] = "FAILED: " + aux_failures[-1]
                gate.update(ani_two_sets_block="512 x 2048", ani_two_sets_hits_checked=int(hr.size), ani_two_sets_hits_max_abs_err=terr)
            if real_hv is not None:  # ... and the real sketches: a 512 x 2 048 CPU block against the timed run's hits
                r_hv, r_n2 = real_hv
                rb = orc.ani_matrix(r_hv[:512].cpu().numpy(), r_n2[:512].cpu().numpy(), r_hv[:2048].cpu().numpy(),
                                    r_n2[:2048].cpu().numpy(), KSIZE)
                rh = real_hits.view(-1, 3)
                sel = (rh[:, 0] < 512) & (rh[:, 1] < 2048)
                hr, hq = rh[sel, 0].long().cpu().numpy(), rh[sel, 1].long().cpu().numpy()
                ha = rh[sel, 2].contiguous().view(torch.float32).cpu().numpy()
                rerr = float(np.abs(ha - rb[hr, hq]).max()) if hr.size else 0.0
                n_cpu = int((rb >= np.float32(85.0)).sum())
                if rerr != 0.0 or hr.size != n_cpu:
                    aux_failures.append("PARITY GATE FAILED: dist on the real sketches: max |gpu - cpu| = %g, %d hits vs %d" % (rerr, hr.size, n_cpu))
                    out["dist"].setdefault("dist_real", {})["parity"] = "FAILED: " + aux_failures[-1]
                gate.update(ani_real_block="512 x 2048", ani_real_hits_checked=int(hr.size), ani_real_hits_max_abs_err=rerr)
            out["dist"]["cpu_baseline"] = cb
            out["dist"]["speedup_vs_cpu_baseline"] = out["dist"]["value"] / cb["value"]
        out["parity_gate"] = dict(gate, status="passed")
    elif rank == 0:
        out["parity_gate"] = {"status": "skipped (no CPU leg: N > 1 or --no-cpu-baseline); hamming / 10k / host-fed self-checks ran"}
    finish()


if __name__ == "__main__":
    main()
