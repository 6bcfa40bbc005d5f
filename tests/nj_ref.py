"""CPU models of neighbour joining as hg_nj* define it (include/hypergen.h): the sequential rule on Python integers -- the
reference --, the same rule on numpy int64 for a few hundred to a thousand items, a generator of additive (tree)
matrices with integer branch lengths in thousandths, and a checker that rebuilds every leaf-to-leaf path length from a
join list.  Nothing here uses the library."""
import numpy as np

FRAC_BITS = 15
UNIT = 1 << FRAC_BITS  # one thousandth of an ANI percent
JOIN_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("len_a", "<i8"), ("len_b", "<i8")])


def milli_matrix(ani):
    """the integer `dist` prints for every entry, in thousandths: NaN and negative values 0, values above 100 100 000, else
    the product with 1000 in double precision, rounded to the nearest integer, ties to even"""
    a = np.asarray(ani, np.float32).astype(np.float64)
    a = np.where(a >= 0.0, a, 0.0)  # (NaN compares false)
    a = np.minimum(a, 100.0)
    return np.rint(a * 1000.0).astype(np.int64)


def dist_matrix(ani):
    """d(i, j) = (100 000 - m(i, j)) << 15 from the UPPER triangle of the float matrix, mirrored; d(i, i) = 0"""
    d = np.triu((100_000 - milli_matrix(ani)) << FRAC_BITS, 1)
    return d + d.T


def ani_of_milli(t):
    """a float32 ANI matrix whose distances in thousandths are the integers t (0 .. 100 000): exact through milli_matrix"""
    a = ((100_000 - np.asarray(t, np.int64)) / 1000.0).astype(np.float32)
    assert np.array_equal(100_000 - milli_matrix(a), t)
    return a


def floor_div(num, den):
    return num // den  # Python's // on ints IS the floor towards minus infinity


def nj_model(d, stats=None):
    """The sequential rule on Python integers.  d: a symmetric integer matrix (dist_matrix); returns the list of joins
    (a, b, len_a, len_b).  stats["clamped"], if given, counts the updates on which the clamp at 0 acted."""
    d = [[int(x) for x in row] for row in np.asarray(d).tolist()]
    n = len(d)
    live = list(range(n))
    joins = []
    while len(live) >= 3:
        c = len(live)
        r = {i: sum(d[i][k] for k in live if k != i) for i in live}
        best = None
        for x, i in enumerate(live):
            for j in live[x + 1:]:
                key = ((c - 2) * d[i][j] - r[i] - r[j], i, j)
                if best is None or key < best:
                    best = key
        _, a, b = best
        D = d[a][b]
        len_a = floor_div((c - 2) * D + r[a] - r[b], 2 * (c - 2))
        joins.append((a, b, len_a, D - len_a))
        for k in live:
            if k != a and k != b:
                if stats is not None and d[a][k] + d[b][k] < D:
                    stats["clamped"] += 1
                d[a][k] = d[k][a] = max(0, (d[a][k] + d[b][k] - D) >> 1)
        live.remove(b)
    if len(live) == 2:
        a, b = live
        joins.append((a, b, d[a][b], 0))
    return joins


def nj_model_np(d):
    """The same rule on numpy int64 (every quantity stays below 2^50).  The matrix is kept compact over the live names in
    ascending order, so the first minimum of Q masked to i < j and flattened row-major is the rule's tie-break."""
    d = np.array(d, np.int64)
    n = d.shape[0]
    names = np.arange(n)
    joins = []
    not_above = np.tril(np.full((n, n), 1 << 62, np.int64))  # added to a row's keys: columns j <= i never win
    key = np.empty((n, n), np.int64)
    r = d.sum(axis=1)  # (the diagonal is 0)
    while names.size >= 3:
        c = names.size
        # Q(i, j) = ((c - 2) d(i, j) - r(j)) - r(i): the first minimum over the rows of the rows' first minima is the first
        # minimum of Q in row-major order
        k = np.multiply(d, c - 2, out=key[:c, :c])
        k -= r[None, :]
        k += not_above[:c, :c]
        row_best = k.min(axis=1) - r
        x = int(np.argmin(row_best[:c - 1]))  # (the last row has no column above it)
        y = int(np.argmin(k[x]))
        D = int(d[x, y])
        len_a = ((c - 2) * D + int(r[x]) - int(r[y])) // (2 * (c - 2))
        joins.append((int(names[x]), int(names[y]), len_a, D - len_a))
        new = np.maximum(0, (d[x] + d[y] - D) >> 1)
        new[x] = 0
        r += new - d[x] - d[y]
        r[x] = new.sum() - new[y]
        d[x, :] = new
        d[:, x] = new
        # row and column y leave: the rows below and the columns behind close up (names stay ascending)
        d[y:c - 1, :] = d[y + 1:c, :]
        d[:, y:c - 1] = d[:, y + 1:c]
        d = d[:c - 1, :c - 1]
        r = np.delete(r, y)
        names = np.delete(names, y)
    if names.size == 2:
        joins.append((int(names[0]), int(names[1]), int(d[0, 1]), 0))
    return joins


def as_records(joins):
    out = np.zeros(len(joins), JOIN_DTYPE)
    for t, (a, b, la, lb) in enumerate(joins):
        out[t] = (a, b, la, lb)
    return out


def as_tuples(records):
    return [(int(x["a"]), int(x["b"]), int(x["len_a"]), int(x["len_b"])) for x in records]


def additive_matrix(rng, n):
    """A random binary (unrooted) tree on n >= 2 leaves with integer branch lengths >= 1 in thousandths, as the matrix of
    its leaf-to-leaf path lengths (int64, thousandths).  A path has at most n - 1 edges, every edge at most
    100 000 // (n - 1): every distance is <= 100 000."""
    longest = max(1, 100_000 // max(n - 1, 1))
    # grow the tree by hanging every new leaf into the middle of a random edge: nodes 0 .. n - 1 are the leaves
    edges = [(0, 1)]
    n_nodes = n
    for leaf in range(2, n):
        u, v = edges.pop(int(rng.integers(len(edges))))
        mid = n_nodes
        n_nodes += 1
        edges += [(u, mid), (mid, v), (mid, leaf)]
    length = rng.integers(1, longest + 1, len(edges))
    adj = [[] for _ in range(n_nodes)]
    for (u, v), w in zip(edges, length.tolist()):
        adj[u].append((v, w))
        adj[v].append((u, w))
    # rooted at leaf 0: the breadth-first order, every node's parent and the edge up to it
    order, parent, up = [0], {0: -1}, {0: 0}
    for u in order:
        for v, w in adj[u]:
            if v not in parent:
                parent[v], up[v] = u, w
                order.append(v)
    # to[u] = the distances from node u to every LEAF, filled from the root down: its parent's with the edge added for
    # the leaves outside u's subtree and taken off for the ones inside it
    inside = {u: np.zeros(n, bool) for u in order}
    for u in reversed(order):
        if u < n:
            inside[u][u] = True
        if parent[u] >= 0:
            inside[parent[u]] |= inside[u]
    depth = np.zeros(n_nodes, np.int64)
    for u in order[1:]:
        depth[u] = depth[parent[u]] + up[u]
    to = {0: depth[:n].copy()}
    t = np.zeros((n, n), np.int64)
    for u in order[1:]:
        to[u] = np.where(inside[u], to[parent[u]] - up[u], to[parent[u]] + up[u])
    for leaf in range(n):
        t[leaf] = to[leaf]
    assert np.array_equal(t, t.T) and not t.diagonal().any() and t.max() <= 100_000
    return t


def path_lengths(joins, n):
    """Every leaf-to-leaf path length of the tree a join list describes, in the joins' units (int64 n x n).  A join (a, b,
    len_a, len_b) puts the leaves under a and the leaves under b at depth + len_a and depth + len_b below the new node."""
    p = np.zeros((n, n), np.int64)
    leaves = {i: np.array([i]) for i in range(n)}
    depth = {i: np.zeros(1, np.int64) for i in range(n)}
    for a, b, la, lb in joins:
        da, db = depth[a] + la, depth.pop(b) + lb
        la_, lb_ = leaves[a], leaves.pop(b)
        cross = da[:, None] + db[None, :]
        p[np.ix_(la_, lb_)] = cross
        p[np.ix_(lb_, la_)] = cross.T
        leaves[a], depth[a] = np.concatenate([la_, lb_]), np.concatenate([da, db])
    return p


def newick_length(length):
    """a branch length as hg_nj_newick prints it"""
    t = (abs(length) * 1000 + 16384) >> 15
    return "%s%d.%08d" % ("-" if length < 0 and t else "", t // 10 ** 8, t % 10 ** 8)


def newick_model(joins, names):
    """hg_nj_newick in Python (valid join lists only)"""
    n = len(names)
    sub = {i: "'%s'" % str(names[i]).replace("'", "''") for i in range(n)}
    if n == 1:
        return sub[0] + ";"
    if n == 2:
        a, b, la, lb = joins[0]
        return "(%s:%s,%s:%s);" % (sub[a], newick_length(la), sub[b], newick_length(lb))
    for a, b, la, lb in joins[:-2]:
        sub[a] = "(%s:%s,%s:%s)" % (sub[a], newick_length(la), sub.pop(b), newick_length(lb))
    (pa, pb, pla, plb), (la_, lb_, ll, lr) = joins[-2], joins[-1]
    other = lb_ if la_ == pa else la_
    top = sorted([(pa, pla), (pb, plb), (other, ll + lr)])
    return "(%s);" % ",".join("%s:%s" % (sub[name], newick_length(length)) for name, length in top)
