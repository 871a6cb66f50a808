"""The random walks of include/pathpyg_amd.h ("random walks") restated in plain Python: the Philox word of cpu_ops_generative, Python floats
(IEEE float64, one rounded operation per statement) and Python loops.  No device, no torch.

A graph is ``(row_ptr, col)`` as lists (row-sorted CSR of n = len(row_ptr) - 1 nodes); ``weight`` a list of floats (float32 weights: their
exact float64 values) or ``None`` for all ones."""
from cpu_ops_generative import M64, word

TAG_WALK_START, TAG_WALK_STEP = 10, 11
BLOCK = 1024
MAX_ATTEMPTS = 4096


def uniform(w):
    """x(word) = (double)(word >> 11) * 2^-53"""
    return float(w >> 11) * 2.0 ** -53


def table(row_ptr, weight, m=None):
    """``(cum, total)``: cum[j] = the left-to-right running sum of j's row up to j; total[v] = T_v.  Raises ValueError on a weight that is
    negative or not finite, as the device flag makes the package do."""
    n = len(row_ptr) - 1
    m = row_ptr[n] if m is None else m
    cum, total = [0.0] * m, [0.0] * n
    for v in range(n):
        s = 0.0
        for j in range(row_ptr[v], row_ptr[v + 1]):
            w = 1.0 if weight is None else float(weight[j])
            if not (w >= 0.0) or w == float("inf"):
                raise ValueError("weight")
            s = s + w
            cum[j] = s
        total[v] = s
    return cum, total


def start_table(total):
    """``(bcum, B)``: running sums of T_v inside blocks of 1024 nodes; running sums of the block totals."""
    n = len(total)
    bcum, B = [0.0] * n, []
    run = 0.0
    for first in range(0, n, BLOCK):
        s = 0.0
        for i in range(first, min(first + BLOCK, n)):
            s = s + total[i]
            bcum[i] = s
        run = run + s
        B.append(run)
    return bcum, B


def positive_nodes(total):
    return [v for v, t in enumerate(total) if t > 0.0]


def below(N, seed, tag, index):
    """pp_rg_draws' rule: multiply-high, rejected while the low product word is under 2^64 mod N; attempt a reads stream a."""
    thr = (1 << 64) % N
    w = 0
    for a in range(MAX_ATTEMPTS):
        w = word(seed, tag, a, index)
        if (w * N) & M64 >= thr:
            break
    return (w * N) >> 64


def weighted_start(seed, w, total, bcum, B):
    n = len(total)
    target = uniform(word(seed, TAG_WALK_START, 0, w)) * B[-1]
    b = next((i for i, x in enumerate(B) if x > target), len(B) - 1)
    t2 = target - (B[b - 1] if b else 0.0)
    first, end = b * BLOCK, min(b * BLOCK + BLOCK, n)
    for v in range(first, end):
        if bcum[v] > t2:
            return v
    return max(v for v in range(first, end) if total[v] > 0.0)


def walks(row_ptr, col, weight, seed, steps, start, num_walks=None):
    """The node lists of the walks: ``start`` is ``"weighted"``, ``"uniform"`` (``num_walks`` of them) or a list of start nodes."""
    n = len(row_ptr) - 1
    cum, total = table(row_ptr, weight)
    if start == "weighted":
        bcum, B = start_table(total)
        starts = [weighted_start(seed, w, total, bcum, B) for w in range(num_walks)]
    elif start == "uniform":
        pos = positive_nodes(total)
        starts = [pos[below(len(pos), seed, TAG_WALK_START, w)] for w in range(num_walks)]
    else:
        starts = list(start)
    out = []
    for w, v in enumerate(starts):
        walk = [v]
        for t in range(steps):
            lo, hi = row_ptr[v], row_ptr[v + 1]
            T = total[v]
            if hi <= lo or not T > 0.0:
                break
            target = uniform(word(seed, TAG_WALK_STEP, t, w)) * T
            j = next((j for j in range(lo, hi) if cum[j] > target), None)
            if j is None or not 0 <= col[j] < n:
                break
            v = col[j]
            walk.append(v)
        out.append(walk)
    return out


def padded(walk_list, steps):
    """``(nodes [W][steps + 1] with -1 after the end, lengths [W])`` as the package's batch holds them."""
    return [w + [-1] * (steps + 1 - len(w)) for w in walk_list], [len(w) - 1 for w in walk_list]


def first_order(walk, node_sequence):
    """The first-order sequence of a walk on a graph whose node v stands for ``node_sequence[v]`` (k nodes): the k nodes of the first
    node, then the last node of every later one."""
    return list(node_sequence[walk[0]]) + [node_sequence[v][-1] for v in walk[1:]]


def path_data_fields(walk_list, node_sequence):
    """The PathData tensors as lists: walks without an edge are left out; the chain joins consecutive positions inside every walk."""
    seq, src, dst, num_nodes, num_edges, weights = [], [], [], [], [], []
    for walk in walk_list:
        if len(walk) < 2:
            continue
        fo = first_order(walk, node_sequence)
        base = len(seq)
        seq += fo
        src += range(base, base + len(fo) - 1)
        dst += range(base + 1, base + len(fo))
        num_nodes.append(len(fo))
        num_edges.append(len(fo) - 1)
        weights.append(1.0)
    return {"node_sequence": [[x] for x in seq], "edge_index": [src, dst], "dag_num_nodes": num_nodes, "dag_num_edges": num_edges,
            "dag_weight": weights}
