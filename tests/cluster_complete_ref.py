"""CPU model of complete linkage (hg_cluster_complete*, `hyper-gen cluster --agglomerate complete`; the rule:
include/hypergen.h).

complete_model()        the sequential rule in Python integers, nothing clever: for n up to a few hundred
complete_model_rounds() the round form in vectorised numpy -- every pair of mutual best partners merges at once -- with the
                        two rules the device adds because values only fall: a row without a partner retires, and a row
                        is scanned again only when it or its partner took part in a merge of the previous round
                        (rescan="all" scans every live row every round: the same result, the same rounds)
Both take the n x n float matrix, of which [i, j] with i < j is read, and return (rep, cluster, into, level, size,
n_clusters); complete_model_rounds(..., with_rounds=True) also returns the rounds it ran, the one that merged nothing
included (0 when the threshold lets nothing merge), with_scans=True the number of row scans behind that.
milli, milli_matrix and th_milli are those of average linkage."""
import numpy as np

from cluster_average_ref import _finish, merge_order, milli, milli_matrix, th_milli  # noqa: F401  (re-exported)


def level_of(w):
    return np.float32(np.float64(w) / np.float64(1000.0))


def _symmetric(matrix):
    m = np.triu(milli_matrix(matrix), 1)
    return m + m.T


def complete_model(matrix, th):
    n = np.asarray(matrix).shape[0]
    w = [[int(x) for x in row] for row in _symmetric(matrix)] if n else []
    cnt, into, level, msize = [1] * n, list(range(n)), [0.0] * n, [1] * n
    live = list(range(n))
    t = th_milli(th)
    while t is not None:
        best = None
        for a in live:  # ascending (lower name, higher name): a strict improvement keeps the first of equals
            for b in live:
                if b > a and (best is None or w[a][b] > best[2]):
                    best = (a, b, w[a][b])
        if best is None or best[2] < t:
            break
        a, b, wab = best
        into[b], level[b], msize[b] = a, level_of(wab), cnt[a] + cnt[b]
        for k in live:
            w[a][k] = w[k][a] = min(w[a][k], w[b][k])
        cnt[a] += cnt[b]
        cnt[b] = 0
        live.remove(b)
    return _finish(n, into, level, msize, cnt)


def complete_model_rounds(matrix, th, with_rounds=False, with_scans=False, rescan="invalidated"):
    assert rescan in ("invalidated", "all")
    n = np.asarray(matrix).shape[0]
    w = _symmetric(matrix) if n else np.zeros((0, 0), np.int64)
    cnt = np.ones(n, np.int64)
    into, level, msize = np.arange(n), np.zeros(n, np.float32), np.ones(n, np.int64)
    none = -1
    nn = np.full(n, none)
    partner = np.full(n, none)  # the name absorbed into this one in the previous round
    t = th_milli(th)
    rounds = scans = 0
    col = np.arange(n)
    while t is not None:
        rounds += 1
        live = cnt > 0
        nn[~live] = none
        scan = live.copy()
        if rounds >= 2 and rescan == "invalidated":
            b = np.where(nn >= 0, nn, 0)
            keep = (nn == none) | ((partner == none) & (cnt[b] != 0) & (partner[b] == none))
            scan &= ~keep
        rows = np.flatnonzero(scan)
        scans += rows.size
        if rows.size:
            sub = w[rows]
            ok = live[None, :] & (col[None, :] != rows[:, None]) & (sub >= t)
            key = np.where(ok, sub * (1 << 32) + ((1 << 32) - 1 - col)[None, :], 0)  # m << 32 | 0xFFFFFFFF - j, under max
            top = key.max(axis=1)
            nn[rows] = np.where(top > 0, (1 << 32) - 1 - (top & 0xFFFFFFFF), none)
        a_all = np.flatnonzero(live & (nn > col))
        pairs = [(int(a), int(nn[a])) for a in a_all if nn[nn[a]] == a]
        partner[:] = none
        if not pairs:
            break
        for a, b in pairs:
            into[b], level[b], msize[b] = a, level_of(int(w[a, b])), cnt[a] + cnt[b]
            partner[a] = b
        for a, b in pairs:  # the rows pass, then the cols pass: two pairs of one round get the minimum of four
            w[a, :] = np.minimum(w[a, :], w[b, :])
        for a, b in pairs:
            w[:, a] = np.minimum(w[:, a], w[:, b])
        for a, b in pairs:
            cnt[a] += cnt[b]
            cnt[b] = 0
    out = _finish(n, into, level, msize, cnt)
    if with_rounds:
        out += (rounds,)
    if with_scans:
        out += (scans,)
    return out
