"""Greedy set-cover clustering restated for the tests (hg_cluster_setcover*, include/hypergen.h): the sequential
definition over a list of hit records with ANI values, in numpy float32, and nothing cleverer.

A record counts iff ani >= th and its two indices differ; it is an edge in either orientation.  U = the undecided nodes,
at first all.  While U is not empty: deg(v) = the counting RECORDS with v at one end and the other end in U (a pair given
twice counts twice); the node of U with the largest deg, ties to the smallest index, becomes a representative; every node
of U with a counting record to it becomes its member, with the highest ANI among those records; all of them leave U.
"""
import numpy as np


def setcover_model(n, a, b, ani, th):
    """-> (rep uint32[n], cluster uint32[n], ani float32[n], n_clusters)"""
    a = np.asarray(a, np.int64).ravel()
    b = np.asarray(b, np.int64).ravel()
    v = np.broadcast_to(np.asarray(ani, np.float32), a.shape).ravel()
    if a.size and (min(a.min(), b.min()) < 0 or max(a.max(), b.max()) >= n):
        raise ValueError("index >= n")
    keep = (v >= np.float32(th)) & (a != b)
    a, b, v = a[keep], b[keep], v[keep]
    undecided = np.ones(n, bool)
    is_rep = np.zeros(n, bool)
    rep = np.arange(n, dtype=np.uint32)
    out = np.full(n, 100.0, np.float32)
    while undecided.any():
        live = undecided[a] & undecided[b]
        a, b, v = a[live], b[live], v[live]  # (a record with a decided end never counts again)
        deg = np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
        deg[~undecided] = -1
        if deg.max() == 0:  # what is left has no live record: every node is its own representative
            is_rep |= undecided
            break
        c = int(np.argmax(deg))  # the first of the largest
        is_rep[c] = True
        undecided[c] = False
        at_a, at_b = a == c, b == c
        others = np.concatenate([b[at_a], a[at_b]])
        values = np.concatenate([v[at_a], v[at_b]])
        best = np.full(n, -np.inf, np.float32)
        np.maximum.at(best, others, values)
        members = np.unique(others)
        rep[members] = c
        out[members] = best[members]
        undecided[members] = False
    roots = np.flatnonzero(is_rep)
    return rep, np.searchsorted(roots, rep).astype(np.uint32), out, int(roots.size)


def setcover_model_matrix(ani, th):
    """the same on a full symmetric ANI matrix (the pairs i < j of its upper triangle)"""
    ani = np.asarray(ani, np.float32)
    i, j = np.nonzero(np.triu(ani >= np.float32(th), 1))
    return setcover_model(ani.shape[0], i, j, ani[i, j], th)
