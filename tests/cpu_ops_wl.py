"""Plain Python restatement of colour refinement and of the reference's Weisfeiler-Leman test, for the tests of
pathpyg_amd.algorithms.weisfeiler_leman.  Deliberately NOT the device's scheme: a node's signature is a tuple (own colour, sorted tuple of the
successors' colours) looked up in a dict — no hashes, no sort keys, no elections — so that an error in the scheme itself cannot hide in a
shared idea.
"""
import numpy as np


def successor_lists(edge_index, n: int) -> list:
    """Stored successors of every node index, parallel edges and self-loops included."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    succ = [[] for _ in range(n)]
    for u, w in zip(ei[0].tolist(), ei[1].tolist()):
        succ[u].append(w)
    return succ


def _by_rank(n: int, order) -> list:
    rank = list(range(n)) if order is None else [int(x) for x in order]
    assert sorted(rank) == list(range(n))
    nodes = [0] * n
    for v, r in enumerate(rank):
        nodes[r] = v
    return nodes


def refine(succ: list, initial=None, order=None, max_rounds=None):
    """``(colours, counts)``: classes 0 .. k-1 numbered by first occurrence in ``order`` (a rank per node); ``counts[0]`` the number of
    distinct initial colours, ``counts[r]`` the classes after round r.  ``max_rounds=None`` stops after the round that did not grow the count."""
    n = len(succ)
    walk = _by_rank(n, order)

    def number(signature):
        table = {}
        for v in walk:
            table.setdefault(signature[v], len(table))
        return [table[signature[v]] for v in range(n)], len(table)

    colours, k = number([0] * n if initial is None else [int(x) for x in initial])
    counts = [k]
    while max_rounds is None or len(counts) - 1 < max_rounds:
        colours, k = number([(colours[v], tuple(sorted(colours[w] for w in succ[v]))) for v in range(n)])
        counts.append(k)
        if counts[-1] == counts[-2]:
            break
    return colours, counts


def union_order(ids1: list, ids2: list) -> list:
    """Rank of every node of the union (g1's nodes, then g2's) in the sorted order of the IDs; tuples sort lexicographically."""
    ids = list(ids1) + list(ids2)
    assert len(set(ids)) == len(ids)
    rank = [0] * len(ids)
    for r, v in enumerate(sorted(range(len(ids)), key=lambda i: ids[i])):
        rank[v] = r
    return rank


def wl_test(ids1: list, succ1: list, ids2: list, succ2: list, features1=None, features2=None):
    """The reference's triple ``(result, fingerprint_1, fingerprint_2)``.  The label table persists over the rounds and is keyed by
    (``str`` of the own label, sorted tuple of the successors' labels): the own label enters the reference's key through ``str()``, the
    successors' through the ``repr`` of a list, which keeps ``'1'`` and ``1`` apart."""
    n1 = len(ids1)
    ids = list(ids1) + list(ids2)
    succ = [list(s) for s in succ1] + [[w + n1 for w in s] for s in succ2]
    walk = _by_rank(len(ids), union_order(ids1, ids2))
    if features1 is None or features2 is None:
        fingerprint = ["0"] * len(ids)
    else:
        merged = dict(features1)
        merged.update(features2)
        fingerprint = [merged[v] for v in ids]
    table, following = {}, 1
    while True:
        new = [None] * len(ids)
        for v in walk:
            key = (str(fingerprint[v]), tuple(sorted(fingerprint[w] for w in succ[v])))
            if key not in table:
                table[key] = following
                following += 1
            new[v] = table[key]
        if len(set(fingerprint)) == len(set(new)):
            break
        fingerprint = new
    fp1, fp2 = fingerprint[:n1], fingerprint[n1:]
    return sorted(fp1) == sorted(fp2), fp1, fp2


def fixture_case(golden, name: str) -> dict:
    """One case of tests/golden/wl_vectors.npz decoded to Python values (the layout: tests/golden/make_golden_wl.py)."""
    get = lambda key: golden[f"{name}/{key}"]  # noqa: E731
    case = {"result": bool(get("result"))}
    featured = f"{name}/feat_values" in golden.files
    values = []
    if featured:
        values = [int(x) if int(get("feat_int")) else str(x) for x in get("feat_values").tolist()]
    for g in ("1", "2"):
        ids = get("ids" + g)
        case["ids" + g] = [tuple(x) for x in ids.tolist()] if ids.ndim > 1 else [str(x) for x in ids.tolist()]
        case["edge_index" + g] = get("edge_index" + g)
        case["features" + g] = {v: values[c] for v, c in zip(case["ids" + g], get("feat" + g).tolist())} if featured else None
        fp = get("fp" + g).tolist()
        if int(get("fp_initial")):
            fp = [values[c] for c in fp] if featured else ["0"] * len(fp)
        case["fp" + g] = fp
    return case


def random_pairs(seed: int, count: int, max_n: int = 40):
    """``count`` random pairs ``(ids1, edge_index1, ids2, edge_index2, features1, features2)``: directed and symmetric graphs, parallel edges,
    self-loops and isolated nodes; on a third g2 is a relabelled copy of g1 (so that True occurs); string features on half.  The IDs of the
    two graphs interleave in sorted order and are not in index order; edge lists are row-sorted (stable)."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        n1 = int(rng.integers(1, max_n + 1))
        m1 = int(rng.integers(0, 3 * n1 + 1))
        ei1 = rng.integers(0, n1, (2, m1)).astype(np.int64)
        symmetric = i % 4 == 1
        if symmetric:
            ei1 = np.concatenate([ei1, ei1[::-1]], axis=1)
        perm = rng.permutation(n1)
        if i % 3 == 0:
            n2, ei2 = n1, perm[ei1]
        else:
            n2 = n1 if i % 3 == 1 else int(rng.integers(1, max_n + 1))
            ei2 = rng.integers(0, n2, (2, ei1.shape[1] // (2 if symmetric else 1))).astype(np.int64)
            if symmetric:
                ei2 = np.concatenate([ei2, ei2[::-1]], axis=1)
        ei1, ei2 = (e[:, np.argsort(e[0], kind="stable")] for e in (ei1, ei2))
        names = rng.permutation(n1 + n2)
        ids1, ids2 = [f"v{int(x):03d}" for x in names[:n1]], [f"v{int(x):03d}" for x in names[n1:]]
        f1 = f2 = None
        if i % 2 == 1:
            palette = ["red", "green", "0", "1x"][: int(rng.integers(1, 5))]
            colour1 = rng.integers(0, len(palette), n1)
            colour2 = np.empty(n2, dtype=np.int64)
            if i % 3 == 0:
                colour2[perm] = colour1
            else:
                colour2 = rng.integers(0, len(palette), n2)
            f1 = {v: palette[int(c)] for v, c in zip(ids1, colour1)}
            f2 = {v: palette[int(c)] for v, c in zip(ids2, colour2)}
        yield ids1, ei1, ids2, ei2, f1, f2
