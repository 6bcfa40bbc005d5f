"""CPU model of average linkage (hg_cluster_average*, `hyper-gen cluster --hclust average`; the rule: include/hypergen.h).

milli()               the integer `dist` prints for an ANI, in thousandths
average_model()       the sequential rule in Python integers, nothing clever: for n up to a few hundred
average_model_rounds() the round form -- every pair of mutual best partners merges at once -- for larger n: a float64
                      shortlist of the candidates of a row, then exact integer comparison among them
Both take the n x n float matrix, of which [i, j] with i < j is read, and return (rep, cluster, into, level, size,
n_clusters); average_model_rounds(..., with_rounds=True) also returns the rounds it ran, the one that merged nothing
included (0 when the threshold lets nothing merge)."""
import numpy as np


def milli(ani):
    """NaN and negative values 0, values above 100 100 000, else rint((double)ani * 1000), ties to even"""
    a = np.float32(ani)
    if not a >= np.float32(0):
        a = np.float32(0)
    if a > np.float32(100):
        a = np.float32(100)
    return int(np.rint(np.float64(a) * np.float64(1000.0)))


def milli_matrix(matrix):
    """milli() of every entry: int64"""
    a = np.asarray(matrix, np.float32).astype(np.float64)
    a = np.where(a >= 0, a, 0.0)  # NaN too
    a = np.minimum(a, 100.0)
    return np.rint(a * 1000.0).astype(np.int64)


def th_milli(th):
    """milli() of the threshold; None when nothing merges (NaN, above 100)"""
    t = np.float32(th)
    if np.isnan(t) or t > np.float32(100):
        return None
    return milli(t)


def level_of(s, pairs):
    return np.float32((np.float64(s) / np.float64(pairs)) / np.float64(1000.0))


def _finish(n, into, level, msize, cnt):
    into = np.asarray(into, np.uint32).reshape(n)
    rep = np.arange(n, dtype=np.uint32)
    for i in range(n):  # into[b] < b: the roots of the smaller indices are final
        if into[i] != i:
            rep[i] = rep[into[i]]
    roots = np.flatnonzero(rep == np.arange(n))
    ids = np.zeros(n, np.uint32)
    ids[roots] = np.arange(roots.size, dtype=np.uint32)
    size = np.array([cnt[i] if into[i] == i else msize[i] for i in range(n)], np.uint32).reshape(n)
    return rep, ids[rep].astype(np.uint32), into, np.asarray(level, np.float32).reshape(n), size, int(roots.size)


def _symmetric_sums(matrix):
    m = np.triu(milli_matrix(matrix), 1)
    return m + m.T


def average_model(matrix, th):
    n = np.asarray(matrix).shape[0]
    s = [[int(x) for x in row] for row in _symmetric_sums(matrix)] if n else []
    cnt, into, level, msize = [1] * n, list(range(n)), [0.0] * n, [1] * n
    live = list(range(n))
    t = th_milli(th)
    while t is not None:
        best = None
        for a in live:  # ascending (lower name, higher name): a strict improvement keeps the first of equals
            for b in live:
                if b <= a:
                    continue
                if best is None or s[a][b] * best[3] > best[2] * (cnt[a] * cnt[b]):
                    best = (a, b, s[a][b], cnt[a] * cnt[b])
        if best is None or best[2] < t * best[3]:
            break
        a, b, sab, pairs = best
        into[b], level[b], msize[b] = a, level_of(sab, pairs), cnt[a] + cnt[b]
        for k in live:
            s[a][k] += s[b][k]
            s[k][a] = s[a][k]
        cnt[a] += cnt[b]
        cnt[b] = 0
        live.remove(b)
    return _finish(n, into, level, msize, cnt)


def average_model_rounds(matrix, th, with_rounds=False):
    n = np.asarray(matrix).shape[0]
    s = _symmetric_sums(matrix) if n else np.zeros((0, 0), np.int64)  # (sums stay far below 2^53 for the n this is run at)
    cnt = np.ones(n, np.int64)
    into, level, msize = np.arange(n), np.zeros(n, np.float32), np.ones(n, np.int64)
    t = th_milli(th)
    rounds = 0
    while t is not None:
        rounds += 1
        live = np.flatnonzero(cnt > 0)
        k = live.size
        sub, c = s[np.ix_(live, live)], cnt[live]
        ok = sub >= t * c[:, None] * c[None, :]
        ok[np.arange(k), np.arange(k)] = False
        ratio = np.where(ok, sub / c[None, :].astype(np.float64), -1.0)  # within a row c(A) is common
        top = ratio.max(axis=1) if k else np.zeros(0)
        nn = np.full(n, -1)
        for r in range(k):
            if top[r] < 0:
                continue
            cand = np.flatnonzero(ratio[r] >= top[r] * (1.0 - 1e-12))
            b = cand[0]
            for x in cand[1:]:  # exact, ties to the smaller name (cand is ascending)
                if int(sub[r, x]) * int(c[b]) > int(sub[r, b]) * int(c[x]):
                    b = x
            nn[live[r]] = live[b]
        pairs = [(a, nn[a]) for a in live if nn[a] > a and nn[nn[a]] == a]
        if not pairs:
            break
        for a, b in pairs:
            into[b], level[b], msize[b] = a, level_of(int(s[a, b]), int(cnt[a] * cnt[b])), cnt[a] + cnt[b]
        for a, b in pairs:
            s[a, :] += s[b, :]
            s[:, a] += s[:, b]
            cnt[a] += cnt[b]
            cnt[b] = 0
    out = _finish(n, into, level, msize, cnt)
    return out + (rounds,) if with_rounds else out


def merge_order(into, level, size):
    """the absorbed names sorted by (level descending, size ascending, into, index): every child before its parent"""
    names = [i for i in range(len(into)) if into[i] != i]
    return sorted(names, key=lambda b: (-float(level[b]), int(size[b]), int(into[b]), b))
