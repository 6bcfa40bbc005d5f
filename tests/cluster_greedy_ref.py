"""Greedy representative clustering restated for the tests (hg_cluster_greedy*, include/hypergen.h): the sequential
definition over an edge list with ANI values, in numpy float32.

Going through i = 0, 1, ...: i is a representative iff no representative j < i has ani(j, i) >= th; otherwise it is a
member of the representative j < i with the highest ani(j, i), ties to the smallest j.  A member covers nobody.  Edges
come in either orientation, duplicates count with each ANI (the highest wins), self-pairs and edges below th are ignored.
"""
import numpy as np


def greedy_model(n, a, b, ani, th):
    """-> (rep uint32[n], cluster uint32[n], ani float32[n], n_clusters)"""
    a = np.asarray(a, np.int64).ravel()
    b = np.asarray(b, np.int64).ravel()
    v = np.broadcast_to(np.asarray(ani, np.float32), a.shape).ravel()
    keep = (v >= np.float32(th)) & (a != b)
    lo, hi, v = np.minimum(a, b)[keep], np.maximum(a, b)[keep], v[keep]
    if lo.size and (lo.min() < 0 or hi.max() >= n):
        raise ValueError("index >= n")
    order = np.argsort(hi, kind="stable")
    lo, hi, v = lo[order], hi[order], v[order]
    first = np.searchsorted(hi, np.arange(n + 1))
    is_rep = np.zeros(n, bool)
    rep = np.arange(n, dtype=np.uint32)
    out = np.full(n, 100.0, np.float32)
    for i in range(n):
        s, e = first[i], first[i + 1]
        if s == e:
            is_rep[i] = True
            continue
        js, vs = lo[s:e], v[s:e]
        m = is_rep[js]
        if not m.any():
            is_rep[i] = True
            continue
        js, vs = js[m], vs[m]
        best = vs.max()
        rep[i] = js[vs == best].min()
        out[i] = best
    roots = np.flatnonzero(is_rep)
    return rep, np.searchsorted(roots, rep).astype(np.uint32), out, int(roots.size)


def greedy_model_matrix(ani, th):
    """the same on a full symmetric ANI matrix (the pairs i < j of its upper triangle)"""
    ani = np.asarray(ani, np.float32)
    i, j = np.nonzero(np.triu(ani >= np.float32(th), 1))
    return greedy_model(ani.shape[0], i, j, ani[i, j], th)
