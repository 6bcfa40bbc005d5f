"""The single-linkage tree (hg_cluster_tree*) as its definition says it, in numpy / Python: Kruskal over the counting edges,
strongest first, under the strict order (ANI descending as floats, lo ascending, hi ascending).  Shared by the CPU tests
(the model itself) and the GPU tests (the device result must EQUAL it, indices and ANI bit patterns)."""
import numpy as np

TREE_DTYPE = np.dtype([("ref_idx", "<u4"), ("qry_idx", "<u4"), ("ani", "<f4")])  # hg_ani_hit


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def counting_edges(n, a, b, ani, th):
    """(lo, hi, ani) of the hits that count: ani >= th as floats (NaN never), a != b; -0 is +0; IndexError on an index >= n"""
    a = np.asarray(a, np.int64).ravel()
    b = np.asarray(b, np.int64).ravel()
    v = np.broadcast_to(np.asarray(ani, np.float32), a.shape).astype(np.float32) + np.float32(0.0)
    if a.size and (max(a.max(), b.max()) >= n or min(a.min(), b.min()) < 0):
        raise IndexError("a hit has an index >= n")
    keep = (v >= np.float32(th)) & (a != b)
    a, b, v = a[keep], b[keep], v[keep]
    return np.minimum(a, b), np.maximum(a, b), v


def tree_model(n, a, b, ani, th):
    """-> (tree, rep, cluster, n_clusters): tree as TREE_DTYPE records {lo, hi, ani}, strongest first; rep[i] = the smallest
    index of i's component at th, cluster[i] = its dense id in order of rep"""
    lo, hi, v = counting_edges(n, a, b, ani, th)
    order = np.lexsort((hi, lo, -v.astype(np.float64)))  # last key first: ANI descending, then lo, then hi
    parent = list(range(n))
    tree = []
    for k in order.tolist():
        x, y = _find(parent, int(lo[k])), _find(parent, int(hi[k]))
        if x != y:
            parent[max(x, y)] = min(x, y)
            tree.append((int(lo[k]), int(hi[k]), v[k]))
    rep = np.array([_find(parent, i) for i in range(n)], np.uint32)
    roots = np.flatnonzero(rep == np.arange(n, dtype=np.uint32))
    dense = np.zeros(max(n, 1), np.uint32)
    dense[roots] = np.arange(roots.size, dtype=np.uint32)
    out = np.zeros(len(tree), TREE_DTYPE)
    if tree:
        out["ref_idx"], out["qry_idx"], out["ani"] = zip(*tree)
    return out, rep, dense[rep] if n else np.zeros(0, np.uint32), int(roots.size)


def tree_model_matrix(ani, th):
    """the model on a full symmetric ANI matrix (the pairs i < j)"""
    ani = np.asarray(ani, np.float32)
    i, j = np.triu_indices(ani.shape[0], 1)
    return tree_model(ani.shape[0], i, j, ani[i, j], th)


def components(n, a, b, ani, th):
    """(rep, cluster, n_clusters) of the graph of the hits that count at th: what the step calls of hg_cluster give"""
    lo, hi, v = counting_edges(n, a, b, ani, th)
    parent = list(range(n))
    for x, y in zip(lo.tolist(), hi.tolist()):
        x, y = _find(parent, x), _find(parent, y)
        if x != y:
            parent[max(x, y)] = min(x, y)
    rep = np.array([_find(parent, i) for i in range(n)], np.uint32)
    roots = np.flatnonzero(rep == np.arange(n, dtype=np.uint32))
    dense = np.zeros(max(n, 1), np.uint32)
    dense[roots] = np.arange(roots.size, dtype=np.uint32)
    return rep, dense[rep] if n else np.zeros(0, np.uint32), int(roots.size)


def cut(n, tree, t):
    """the tree cut at t >= the floor it was built at: (rep, cluster, n_clusters)"""
    return components(n, tree["ref_idx"], tree["qry_idx"], tree["ani"], t)


def closure_count(n, a, b, ani, th):
    """the number of components by transitive closure of the adjacency matrix (small n): independent of union-find"""
    lo, hi, _ = counting_edges(n, a, b, ani, th)
    reach = np.eye(n, dtype=bool)
    reach[lo, hi] = reach[hi, lo] = True
    while True:
        nxt = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
        if np.array_equal(nxt, reach):
            return np.unique(reach, axis=0).shape[0]
        reach = nxt
