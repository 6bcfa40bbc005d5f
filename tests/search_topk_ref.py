"""Numpy model of hg_search_topk*: from an ANI matrix (R x Q float32, row = reference), a threshold and k, per query the k
best references -- descending ANI, ties by ascending reference index, only entries with ani >= ani_th (float32 compare).
Returns (hits, counts) in the layout of the C entry points: hits of shape (Q, k) with fields ref_idx / qry_idx / ani, unused
slots {0xFFFFFFFF, 0xFFFFFFFF, 0}, counts[q] <= k.

The order does not depend on the threshold (it only cuts the descending list off), so the model has two steps: topk_sorted
orders the `depth` best entries of every column once, topk_from_sorted applies a threshold and a k <= depth to them -- a test
that sweeps thresholds and k over one large matrix orders it once."""
import numpy as np

HIT_DTYPE = np.dtype([("ref_idx", "<u4"), ("qry_idx", "<u4"), ("ani", "<f4")])
EMPTY = 0xFFFFFFFF


def topk_sorted(ani, depth, ref_off=0, chunk=256):
    """(min(depth, R), Q) uint64, every column descending: ani_bits << 32 | (0xFFFFFFFF - reference index).  ANI is never
    negative, so its bit pattern orders like its value and the key orders like (ANI descending, reference ascending)."""
    ani = np.ascontiguousarray(ani, np.float32)
    R, Q = ani.shape
    kk = min(depth, R)
    out = np.zeros((kk, Q), np.uint64)
    if kk == 0:
        return out
    low = (np.uint64(EMPTY) - (np.arange(R, dtype=np.uint64) + np.uint64(ref_off)))[:, None]
    for q0 in range(0, Q, chunk):
        a = ani[:, q0:q0 + chunk]
        keys = (a.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low
        top = np.partition(keys, R - kk, axis=0)[R - kk:] if kk < R else keys
        out[:, q0:q0 + chunk] = np.sort(top, axis=0)[::-1]
    return out


def topk_from_sorted(top, ani_th, k, qry_off=0):
    Q = top.shape[1]
    hits = np.zeros((Q, k), HIT_DTYPE)
    hits["ref_idx"] = EMPTY
    hits["qry_idx"] = EMPTY
    counts = np.zeros(Q, np.uint32)
    if Q == 0 or k == 0:
        return hits, counts
    top = top[:k]
    n = top.shape[0]
    ani = (top >> np.uint64(32)).astype(np.uint32).view(np.float32)
    ok = (ani >= np.float32(ani_th)).T  # (Q, n); a column is descending, so the entries that pass lead it
    hits["ref_idx"][:, :n][ok] = (np.uint64(EMPTY) - (top & np.uint64(EMPTY))).astype(np.uint32).T[ok]
    hits["qry_idx"][:, :n][ok] = np.broadcast_to((np.arange(Q, dtype=np.uint32) + np.uint32(qry_off))[:, None], (Q, n))[ok]
    hits["ani"][:, :n][ok] = ani.T[ok]
    counts[:] = ok.sum(axis=1)
    return hits, counts


def topk_model(ani, ani_th, k, ref_off=0, qry_off=0, chunk=256):
    ani = np.ascontiguousarray(ani, np.float32)
    return topk_from_sorted(topk_sorted(ani, k, ref_off, chunk), ani_th, k, qry_off)


def topk_loop(ani, ani_th, k):
    """the same by a plain Python loop (what the model is checked against)"""
    ani = np.asarray(ani, np.float32)
    R, Q = ani.shape
    hits = np.zeros((Q, k), HIT_DTYPE)
    hits["ref_idx"] = EMPTY
    hits["qry_idx"] = EMPTY
    counts = np.zeros(Q, np.uint32)
    for q in range(Q):
        cand = [(-float(ani[r, q]), r) for r in range(R) if ani[r, q] >= np.float32(ani_th)]
        cand.sort()
        for j, (neg, r) in enumerate(cand[:k]):
            hits[q, j] = (r, q, ani[r, q])
        counts[q] = min(k, len(cand))
    return hits, counts
