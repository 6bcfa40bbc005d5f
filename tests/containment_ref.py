"""The containment ANI metrics restated for the tests (hg_ctx_set_ani_metric, include/hypergen.h), and seeded inputs for them.

* ani_ref: the three metrics in numpy float32, in the order the library evaluates them -- x = dot / nq (containment) or
  dot / min(nr, nq) (max containment), ani = 1 + logf(x) / k, NaN -> 0, clamp to [0, 1], x 100 -- with the host's logf
  (the oracle's logf_array, which tests/test_gpu_ani_exact.py proves equal to the device's).  The Mash-style metric is
  the oracle's own ani_from_dots.
* exact_dots: the integer dot products of two HV sets, wrapped to i32 like the reference's sum.
* fragment_hvs / stress_hvs: HVs built the way sketches are -- hv = sum over a hash set of +-1 vectors, so that
  dot ~ D * |A & B| and norm ~ D * |A| -- for members that keep a graded share (5 % .. 100 %) of a parent's hashes and
  replace a graded share with fresh ones: a wide spread of nr / nq.
* write_fasta / mutate / synth: seeded genomes for the command-line tests.
"""
import numpy as np

MASH, CONTAINMENT, MAX_CONTAINMENT = 0, 1, 2


def wrap_i32(x):
    return (np.asarray(x, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def ani_ref(orc, dot, nr, nq, k, metric):
    """float32 ANI of every (dot, nr, nq) under `metric` (arrays of one shape; i32 inputs)"""
    dot, nr, nq = (np.ascontiguousarray(v, np.int32) for v in (dot, nr, nq))
    shape = dot.shape
    dot, nr, nq = dot.ravel(), np.broadcast_to(nr, shape).ravel(), np.broadcast_to(nq, shape).ravel()
    if metric == MASH:
        return orc.ani_from_dots(dot, nr, nq, k).reshape(shape)
    den = nq if metric == CONTAINMENT else np.minimum(nr, nq)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = dot.astype(np.float32) / den.astype(np.float32)
        ani = np.float32(1.0) + orc.logf_array(x) / np.float32(k)
    ani = np.where(np.isnan(ani), np.float32(0.0), ani)
    ani = np.maximum(np.minimum(ani, np.float32(1.0)), np.float32(0.0))
    return (ani * np.float32(100.0)).astype(np.float32).reshape(shape)


def exact_dots(r_hv, q_hv):
    """R x Q i32 dot products: int64 products of the i16 HVs, summed exactly, wrapped.  Large sets take a float64 matmul on
    the GPU when torch has one -- exact as well: every partial sum stays far below 2^53."""
    r, q = np.asarray(r_hv), np.asarray(q_hv)
    if r.shape[0] * q.shape[0] > 1 << 20:
        try:
            import torch
            if torch.cuda.is_available():
                a = torch.from_numpy(r.astype(np.float64)).cuda()
                b = torch.from_numpy(q.astype(np.float64)).cuda()
                return wrap_i32((a @ b.T).cpu().numpy().astype(np.int64))
        except ImportError:
            pass
    return wrap_i32(r.astype(np.int64) @ q.astype(np.int64).T)


def norms(hv):
    return wrap_i32((np.asarray(hv, np.int64) ** 2).sum(1))


def _pm1_sum(rng, n, D):
    """the HV of n fresh hashes: a sum of n random +-1 per dimension, 2 * Binomial(n, 1/2) - n"""
    return (2 * rng.binomial(n, 0.5, D) - n).astype(np.int64)


def fragment_hvs(n, D=4096, seed=0, parents=4, blocks=40, block_hashes=80):
    """n HVs in `parents` families.  A family's parent is `blocks` blocks of `block_hashes` hashes; member i keeps a graded
    share of them (5 % .. 100 %, a seeded choice of blocks) and replaces a graded share (0 .. 30 %) of what it keeps with
    fresh hashes of its own.  Returns (hv int16, norm2 int32, completeness)."""
    rng = np.random.default_rng(seed)
    vb = [np.stack([_pm1_sum(rng, block_hashes, D) for _ in range(blocks)]) for _ in range(parents)]
    hv = np.zeros((n, D), np.int64)
    comp = np.zeros(n)
    for i in range(n):
        t = (i // parents) / max(1, (n - 1) // parents)
        keep = max(1, int(round(blocks * (0.05 + 0.95 * ((t * 7.3) % 1.0)))))
        repl = int(keep * 0.3 * ((t * 3.1) % 1.0))
        sel = rng.choice(blocks, keep, replace=False)
        hv[i] = vb[i % parents][sel[: keep - repl]].sum(0) + _pm1_sum(rng, repl * block_hashes, D)
        comp[i] = keep / blocks
    return hv.astype(np.int16), norms(hv), comp


def stress_hvs(R, Q, D=4096, seed=1, blocks=30, block_hashes=100):
    """References: one parent (blocks x block_hashes hashes) plus 0 .. 50 % fresh hashes; queries: 1 .. 5 of the parent's
    blocks (3 .. 17 %).  Nearly every query is contained in every reference (containment ANI ~ 100), while J = |q| / |r|
    stays below the Mash-style ANI of 95 (J >= 0.21 needed at k = 21)."""
    rng = np.random.default_rng(seed)
    vb = np.stack([_pm1_sum(rng, block_hashes, D) for _ in range(blocks)])
    parent = vb.sum(0)
    r = np.stack([parent + _pm1_sum(rng, int(blocks * block_hashes * 0.5 * i / max(1, R - 1)), D) for i in range(R)])
    q = np.stack([vb[rng.choice(blocks, 1 + i % 5, replace=False)].sum(0) for i in range(Q)])
    return r.astype(np.int16), norms(r), q.astype(np.int16), norms(q)


# ---- genomes for the command line ----------------------------------------------------------------------------------------
def synth(seed, L):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), L).tobytes()


def mutate(seq, rate, seed):
    """uniform substitutions at `rate` (every substituted base differs from the original)"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(seq, np.uint8).copy()
    pos = np.nonzero(rng.random(a.size) < rate)[0]
    lut = np.frombuffer(b"ACGT", np.uint8)
    code = np.searchsorted(lut, a[pos])
    a[pos] = lut[(code + rng.integers(1, 4, pos.size)) % 4]
    return a.tobytes()


def fragment(seq, frac, seed):
    """a contiguous stretch of `frac` of the sequence at a seeded offset"""
    n = int(len(seq) * frac)
    off = int(np.random.default_rng(seed).integers(0, len(seq) - n + 1))
    return seq[off: off + n]


def write_fasta(path, seq, name, width=80):
    with open(path, "wb") as f:
        f.write(b">" + name.encode() + b"\n")
        for i in range(0, len(seq), width):
            f.write(seq[i: i + width] + b"\n")
