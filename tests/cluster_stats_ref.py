"""CPU model of the cluster statistics (hg_cluster_stats*, `hyper-gen cluster --stats`): the rule of include/hypergen.h on
integers.  m(i, j) = cluster_average_ref.milli_matrix (the ANI as `dist` prints it, in thousandths); the row of i uses row i
of the matrix only, the diagonal is never read, nothing assumes symmetry.  node_stats / cluster_stats return numpy record
arrays with the fields of hg_node_stat / hg_cluster_stat; stats_lines formats what the command line writes."""
import numpy as np

from cluster_average_ref import milli_matrix

NONE = 0xFFFFFFFF
NODE_DTYPE = np.dtype([("within_sum", np.uint64), ("within_min", np.uint32), ("within_min_idx", np.uint32),
                       ("outside_max", np.uint32), ("outside_max_idx", np.uint32)])
CLUSTER_DTYPE = np.dtype([("within_sum", np.uint64), ("size", np.uint32), ("first", np.uint32), ("medoid", np.uint32),
                          ("within_min", np.uint32), ("within_min_a", np.uint32), ("within_min_b", np.uint32),
                          ("outside_max", np.uint32), ("outside_member", np.uint32), ("outside_idx", np.uint32),
                          ("reserved", np.uint32)])


def node_stats(matrix, cluster):
    m = milli_matrix(matrix)
    cl = np.asarray(cluster, np.int64)
    n = cl.shape[0]
    out = np.zeros(n, NODE_DTYPE)
    big = np.int64(1) << 40
    for i in range(n):
        row = m[i] if n else None
        others = np.arange(n) != i
        inside = (cl == cl[i]) & others
        outside = cl != cl[i]
        out["within_sum"][i] = int(row[inside].sum())
        if inside.any():
            v = np.where(inside, row, big)
            j = int(np.argmin(v))  # (the first index of the minimum)
            out["within_min"][i], out["within_min_idx"][i] = int(v[j]), j
        else:
            out["within_min"][i] = out["within_min_idx"][i] = NONE
        if outside.any():
            v = np.where(outside, row, -1)
            j = int(np.argmax(v))  # (the first index of the maximum)
            out["outside_max"][i], out["outside_max_idx"][i] = int(v[j]), j
        else:
            out["outside_max"][i] = out["outside_max_idx"][i] = NONE
    return out


def cluster_stats(nodes, cluster, n_clusters):
    cl = np.asarray(cluster, np.int64)
    out = np.zeros(n_clusters, CLUSTER_DTYPE)
    for name in ("first", "medoid", "within_min", "within_min_a", "within_min_b", "outside_max", "outside_member", "outside_idx"):
        out[name] = NONE
    for c in range(n_clusters):
        mem = np.flatnonzero(cl == c)
        if mem.size == 0:
            continue
        r = out[c:c + 1]
        sums = nodes["within_sum"][mem]
        r["within_sum"], r["size"], r["first"] = int(sums.astype(object).sum()), mem.size, int(mem[0])
        r["medoid"] = int(mem[np.argmax(sums)])  # (members ascend: the first maximum is the smallest index)
        has = nodes["within_min_idx"][mem] != NONE
        if has.any():
            a = int(mem[has][np.argmin(nodes["within_min"][mem][has])])
            r["within_min"], r["within_min_a"], r["within_min_b"] = nodes["within_min"][a], a, nodes["within_min_idx"][a]
        has = nodes["outside_max_idx"][mem] != NONE
        if has.any():
            a = int(mem[has][np.argmax(nodes["outside_max"][mem][has])])
            r["outside_max"], r["outside_member"], r["outside_idx"] = nodes["outside_max"][a], a, nodes["outside_max_idx"][a]
    return out


def stats_model(matrix, cluster, n_clusters):
    nodes = node_stats(matrix, cluster)
    return nodes, cluster_stats(nodes, cluster, n_clusters)


def mean_within(within_sum, size):
    """the mean within-cluster ANI as the library's users compute it: two double divisions, one conversion"""
    return np.float32((np.float64(int(within_sum)) / np.float64(int(size) * (int(size) - 1))) / np.float64(1000.0))


def milli_text(v):
    return "%d.%03d" % (int(v) // 1000, int(v) % 1000)


def stats_lines(stats, cluster, names):
    """the lines of `cluster --stats`: names[i] = the file of item i (in the order the statistics were computed in)"""
    out = []
    for c, s in enumerate(stats):
        f = [str(c), str(int(s["size"])), names[int(s["medoid"])]]
        if s["size"] >= 2:
            f += ["%.3f" % float(mean_within(s["within_sum"], s["size"])), milli_text(s["within_min"]),
                  names[int(s["within_min_a"])], names[int(s["within_min_b"])]]
        else:
            f += ["NA"] * 4
        if s["outside_idx"] != NONE:
            f += [milli_text(s["outside_max"]), names[int(s["outside_member"])], names[int(s["outside_idx"])],
                  str(int(cluster[int(s["outside_idx"])]))]
        else:
            f += ["NA"] * 4
        out.append("\t".join(f) + "\n")
    return "".join(out)


def not_separated(stats):
    return int(sum(1 for s in stats if s["size"] >= 2 and s["outside_idx"] != NONE and s["outside_max"] >= s["within_min"]))
