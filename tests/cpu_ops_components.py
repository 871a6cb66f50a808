"""Plain numpy / Python restatement of connected components and of the largest-component sub-graph, for the tests of
pathpyg_amd.algorithms.components.  Deliberately NOT the device's algorithms: weak components by a sequential union-find, strong ones by an
iterative Tarjan (the kernel colours and searches backwards), so that an error in the scheme itself cannot hide in a shared idea.
"""
from collections import Counter

import numpy as np


def _pairs(edge_index):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    return ei[0].tolist(), ei[1].tolist()


def by_smallest_member(raw) -> np.ndarray:
    """Renumber any labelling in the order of each class's first node (= its smallest member): int32."""
    raw = np.asarray(raw)
    seen, out = {}, np.empty(len(raw), dtype=np.int32)
    for v, x in enumerate(raw.tolist()):
        out[v] = seen.setdefault(x, len(seen))
    return out


def weak_labels(edge_index, n: int) -> np.ndarray:
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, w in zip(*_pairs(edge_index)):
        a, b = find(u), find(w)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return by_smallest_member([find(v) for v in range(n)])


def strong_labels(edge_index, n: int) -> np.ndarray:
    """Tarjan's algorithm with an explicit stack; labels renumbered by smallest member."""
    src, dst = _pairs(edge_index)
    succ = [[] for _ in range(n)]
    for u, w in zip(src, dst):
        succ[u].append(w)
    index, low, on_stack = [-1] * n, [0] * n, [False] * n
    comp, stack, counter, found = [-1] * n, [], 0, 0
    for s in range(n):
        if index[s] >= 0:
            continue
        work = [(s, 0)]
        while work:
            v, i = work.pop()
            if i == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on_stack[v] = True
            descended = False
            while i < len(succ[v]):
                w = succ[v][i]
                i += 1
                if index[w] < 0:
                    work.append((v, i))
                    work.append((w, 0))
                    descended = True
                    break
                if on_stack[w]:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                while True:
                    w = stack.pop()
                    on_stack[w] = False
                    comp[w] = found
                    if w == v:
                        break
                found += 1
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return by_smallest_member(comp)


def labels(edge_index, n: int, strong: bool = False, undirected: bool = False) -> np.ndarray:
    return strong_labels(edge_index, n) if strong and not undirected else weak_labels(edge_index, n)


def sizes(lab) -> np.ndarray:
    lab = np.asarray(lab)
    return np.bincount(lab, minlength=(int(lab.max()) + 1 if len(lab) else 0)).astype(np.int64)


def largest_label(lab) -> int:
    """The reference's choice: ``Counter(labels.tolist()).most_common(1)`` — among equal counts the label that appears first."""
    return Counter(np.asarray(lab).tolist()).most_common(1)[0][0]


def kept_edges(edge_index, lab, keep) -> np.ndarray:
    """The stored edges with both ends labelled ``keep``, in stored order: int64 [2, kept] of the ORIGINAL node indices."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    lab = np.asarray(lab)
    mask = (lab[ei[0]] == keep) & (lab[ei[1]] == keep)
    return ei[:, mask]
