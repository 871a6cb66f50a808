"""pathpyg_amd.statistics on the device (csrc/pp_graph_triads.hip) through the public functions, held to the fixtures made from the
reference's own functions (tests/golden/statistics_vectors.npz) and to the plain restatement (tests/cpu_ops_statistics.py: Python sets,
nothing sorted or bisected), at the smallest shapes at which each mechanism can fail: list lengths around every group width and the
workgroup threshold, a long list against short ones and against a long one, unsorted and parallel stored edges against their coalesced
twin, empty graphs, pair batches of many workgroups.

Integers, local clustering coefficients, the degree functions and the one-division similarities are compared exactly.  The Adamic-Adar sum
is held within (k - 1) 2**-53 sum|terms| for k common neighbours — the bound of ANY summation order of the same float64 terms — and the
average clustering coefficient within n 2**-24 mean|C_u| + 2**-24, the worst case of any float32 summation order; both must be bit-equal
on a second call."""
import math
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_statistics as ops
import pathpyg_amd as pp
from pathpyg_amd import _hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = pp.statistics
NS = pp.statistics.node_similarities
GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "statistics_vectors.npz", allow_pickle=False)
NAMES = [str(x) for x in GOLDEN["names"]]
MODES = ("in", "out", "total")
SCALAR = {"common_neighbors": NS.common_neighbors, "overlap": NS.overlap_coefficient, "jaccard": NS.jaccard_similarity,
          "adamic_adar": NS.adamic_adar_index, "cosine": NS.cosine_similarity}
FIXTURE_SLOT = {"common_neighbors": 0, "overlap": 1, "jaccard": 2, "adamic_adar": 3, "cosine": 4}
TOY = [("a", "b"), ("b", "c"), ("c", "a"), ("d", "e"), ("e", "f"), ("f", "g"), ("g", "d"), ("d", "f"), ("b", "d")]
REFERENCE_EXAMPLE = [("a", "b", 1), ("b", "c", 5), ("c", "d", 9), ("c", "e", 9), ("c", "f", 11), ("f", "a", 13), ("a", "g", 18), ("b", "f", 21),
                     ("a", "g", 26), ("c", "f", 27), ("h", "f", 27), ("g", "h", 28), ("a", "c", 30), ("a", "b", 31), ("c", "h", 32), ("f", "h", 33),
                     ("b", "i", 42), ("i", "b", 42), ("c", "i", 47), ("h", "i", 50)]


def graph_of(ei, n, device=DEV, ids=None, undirected=False):
    ei = torch.as_tensor(np.asarray(ei), dtype=torch.int64).reshape(2, -1).to(device)
    mapping = None if ids is None else pp.IndexMap(list(ids))
    g = pp.Graph(pp.Data(edge_index=ei, num_nodes=n), mapping=mapping)
    g.is_undirected_flag = undirected
    return g


def same(got, want):
    got, want = float(got), float(want)
    return (math.isnan(got) and math.isnan(want)) or got == want


def guarded(fn, *args, **kw):
    try:
        return fn(*args, **kw), 0
    except ZeroDivisionError:
        return float("nan"), 1


def aa_bound(terms):
    return max(len(terms) - 1, 0) * 2.0 ** -53 * sum(abs(t) for t in terms)


def check_aa(got, terms):
    if any(math.isinf(t) for t in terms):
        assert got == math.inf
    else:
        assert abs(float(got) - math.fsum(terms)) <= aa_bound(terms)


def stored(g):
    return g.data.edge_index.cpu().numpy(), g.n


def check_clustering(g, counts_only=False):
    """closed_triad_counts, the coefficients and the average of ``g`` against the restatement; returns the counts."""
    ei, n = stored(g)
    want = ops.triad_counts(ei, n)
    got = S.closed_triad_counts(g)
    assert got.dtype == torch.int64 and got.device == g.device and got.shape == (n,)
    assert np.array_equal(got.cpu().numpy(), want)
    if counts_only:
        return want
    coeff = S.local_clustering_coefficients(g)
    want_coeff = ops.local_coefficients(ei, n, g.is_undirected())
    assert coeff.dtype == torch.float64 and coeff.device == g.device and np.array_equal(coeff.cpu().numpy(), want_coeff)
    avg = S.avg_clustering_coefficient(g)
    assert isinstance(avg, float)
    if n == 0:
        assert math.isnan(avg)
    else:
        print(f"avg_clustering_coefficient: got {avg!r}, exact {ops.avg_coefficient(ei, n, g.is_undirected())!r}")
        assert abs(avg - ops.avg_coefficient(ei, n, g.is_undirected())) <= n * 2.0 ** -24 * float(np.abs(want_coeff).mean()) + 2.0 ** -24
        assert S.avg_clustering_coefficient(g) == avg
    return want


def check_pairs(g, pairs, measures=tuple(SCALAR)):
    """``pairwise`` on the index pairs [2, P] for every measure against the restatement's table."""
    ei, n = stored(g)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(2, -1)
    table = ops.pair_table(ei, n, pairs)
    dev_pairs = torch.from_numpy(pairs).to(g.device)
    for measure in measures:
        got = NS.pairwise(g, dev_pairs, measure)
        assert got.device == g.device and got.shape == (pairs.shape[1],)
        if measure == "common_neighbors":
            assert got.dtype == torch.int64 and got.cpu().tolist() == table["common"]
            continue
        assert got.dtype == torch.float64
        values = got.cpu().tolist()
        if measure == "adamic_adar":
            for value, terms in zip(values, table["terms"]):
                check_aa(value, terms)
            assert torch.equal(NS.pairwise(g, dev_pairs, measure).cpu().view(torch.int64), got.cpu().view(torch.int64))       # bit for bit
        else:
            bad = [(p, a, b) for p, (a, b) in enumerate(zip(values, table[measure])) if not same(a, b)]
            assert not bad, (measure, bad[:5])


# ------------------------------------------------------------------ 1. the fixtures
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(name):
    get = lambda key: GOLDEN[f"{name}/{key}"]  # noqa: E731
    ei, n, und = get("edge_index"), int(get("n")), bool(get("undirected"))
    ids = [f"v{i:03d}" for i in range(n)]
    g = graph_of(ei, n, ids=ids, undirected=und)
    assert np.array_equal(S.closed_triad_counts(g).cpu().numpy(), get("triads"))
    coeff = S.local_clustering_coefficients(g).cpu().numpy()
    assert coeff.dtype == np.float64 and np.array_equal(coeff, get("coeff"))
    avg = S.avg_clustering_coefficient(g)
    print(f"{name}: avg_clustering_coefficient {avg!r}, reference {float(get('avg'))!r}")
    assert abs(avg - float(get("avg"))) <= n * 2.0 ** -24 * float(np.abs(get("coeff")).mean()) + 2.0 ** -24
    assert S.avg_clustering_coefficient(g) == avg
    sets = ops.successor_sets(ei, n)
    for v in sorted({0, 1, 2, n // 2, n - 1} & set(range(n))):
        assert S.local_clustering_coefficient(g, ids[v]) == get("coeff")[v]
        triads = S.closed_triads(g, ids[v])
        assert len(triads) == get("triads")[v]
        assert triads == {(ids[x], ids[y]) for x, y in ops.closed_triads_of(ei, n, v, sets)}
    for mode in MODES:
        seq = S.degree_sequence(g, mode=mode)
        assert seq.device == g.device and np.array_equal(seq.cpu().numpy(), get(f"{mode}/sequence"))
        p = S.degree_distribution(g, mode=mode)
        assert p.dtype == torch.float32 and p.device == g.device and np.array_equal(p.cpu().numpy(), get(f"{mode}/distribution"))
        scalars, raised = get(f"{mode}/scalars"), get(f"{mode}/raised")
        for k in (1, 2, 3):
            assert S.degree_raw_moment(g, k=k, mode=mode) == scalars[k - 1]
            assert S.degree_central_moment(g, k=k, mode=mode) == scalars[2 + k]
        assert S.mean_degree(g, mode=mode) == scalars[6]
        for slot, flag in ((7, False), (8, True)):
            value, code = guarded(S.mean_neighbor_degree, g, mode=mode, exclude_backlink=flag)
            assert code == raised[slot] and same(value, scalars[slot])
        value, code = guarded(S.degree_assortativity, g, mode=mode)
        assert code == raised[9] and same(value, scalars[9])
        values = S.degree_generating_function(g, [0, 0.3, 1], mode=mode)
        assert values.dtype == torch.float32 and np.array_equal(values.numpy(), get(f"{mode}/genfun"))
        assert S.degree_generating_function(g, 0.3, mode=mode) == scalars[10]
    values, raised = get("pair/values"), get("pair/raised")
    k = min(n, 6)
    pairs = torch.tensor([[a for a in range(k) for _ in range(k)], [b for _ in range(k) for b in range(k)]], dtype=torch.int64, device=DEV)
    batch = {measure: NS.pairwise(g, pairs, measure).cpu().tolist() for measure in SCALAR}
    by_ids = NS.pairwise(g, [(ids[a], ids[b]) for a in range(k) for b in range(k)], "jaccard").cpu().tolist()
    assert all(same(x, y) for x, y in zip(by_ids, batch["jaccard"]))
    for a in range(k):
        for b in range(k):
            terms = ops.adamic_adar_terms(ei, n, a, b)
            for measure, fn in SCALAR.items():
                slot = FIXTURE_SLOT[measure]
                value, code = guarded(fn, g, ids[a], ids[b])
                assert code == raised[slot, a, b], (measure, a, b)
                if measure == "adamic_adar":
                    if math.isinf(values[slot, a, b]):
                        assert value == math.inf
                    else:
                        assert abs(float(value) - values[slot, a, b]) <= aa_bound(terms), (a, b, value, values[slot, a, b])
                    assert float(fn(g, ids[a], ids[b])) == float(value)                 # bit-equal on a second call
                else:
                    assert same(value, values[slot, a, b]), (measure, a, b, value, values[slot, a, b])
                paired = batch[measure][a * k + b]                                      # pairwise: the scalar's value, nan where it raises
                assert math.isnan(paired) if code else same(paired, value), (measure, a, b, paired, value)
            assert same(NS.inverse_path_length(g, ids[a], ids[b]), values[5, a, b])
    if name == "ref_toy_undirected":
        for slot, x in enumerate((0.02, 0.2)):
            assert np.isclose(NS.katz_index(g, ids[4], ids[6], beta=x), get("katz")[slot])
            assert np.isclose(NS.LeichtHolmeNewman_index(g, ids[4], ids[6], alpha=x), get("lhn")[slot])


# ------------------------------------------------------------------ 2. the reference's known answers
def test_reference_known_answers_undirected_toy():
    toy = pp.Graph.from_edge_list(TOY, device=DEV).to_undirected()
    assert toy.is_undirected()
    assert S.closed_triads(toy, "a") == {("b", "c"), ("c", "b")}
    assert S.closed_triads(toy, "d") == {("e", "f"), ("f", "e"), ("f", "g"), ("g", "f")}
    assert S.local_clustering_coefficient(toy, "a") == 1.0
    assert S.local_clustering_coefficient(toy, "b") == 1 / 3
    assert S.local_clustering_coefficient(toy, "f") == 2 / 3
    assert abs(S.avg_clustering_coefficient(toy) - 0.7619) <= 1e-4
    assert NS.common_neighbors(toy, "c", "a") == 1 and NS.common_neighbors(toy, "a", "g") == 0
    assert NS.common_neighbors(toy, "d", "d") == 4 and NS.common_neighbors(toy, "f", "d") == 2
    assert NS.jaccard_similarity(toy, "a", "b") == 1 / 4
    assert NS.overlap_coefficient(toy, "a", "a") == 1
    assert NS.adamic_adar_index(toy, "e", "g") == 1 / np.log(3) + 1 / np.log(4)
    assert np.isclose(NS.cosine_similarity(toy, "c", "a"), 0.5)
    assert NS.inverse_path_length(toy, "a", "a") == np.inf and NS.inverse_path_length(toy, "a", "g") == 1 / 3
    assert np.isclose(NS.katz_index(toy, "e", "g", beta=0.2), 0.12958435772871946)
    assert np.isclose(NS.LeichtHolmeNewman_index(toy, "e", "g", alpha=0.2), 0.14353902083713282)


def test_reference_known_answers_directed_toy():
    toy = pp.Graph.from_edge_list(TOY, device=DEV)
    assert S.closed_triads(toy, "a") == set()
    assert S.closed_triads(toy, "d") == {("e", "f")}
    assert S.closed_triad_counts(toy).tolist() == [len(S.closed_triads(toy, v)) for v in "abcdefg"]


def test_corner_return_types():
    g = pp.Graph.from_edge_list([("a", "b"), ("c", "b"), ("d", "e")], device=DEV)      # b and e have no successors
    assert NS.jaccard_similarity(g, "b", "e") == 1 and isinstance(NS.jaccard_similarity(g, "b", "e"), int)
    with pytest.raises(ZeroDivisionError):
        NS.overlap_coefficient(g, "a", "b")
    assert NS.cosine_similarity(g, "a", "c") == 0 and isinstance(NS.cosine_similarity(g, "a", "c"), int)      # in-degree 0
    assert math.isnan(NS.cosine_similarity(g, "b", "e"))                                # in-degree > 0, empty out-rows
    assert NS.adamic_adar_index(g, "a", "d") == 0 and isinstance(NS.adamic_adar_index(g, "a", "d"), int)
    assert float(NS.adamic_adar_index(g, "a", "c")) == 0.0                              # the common successor b has out-degree 0: 1 / log 0
    assert NS.inverse_path_length(g, "a", "e") == 0.0
    with pytest.raises(ZeroDivisionError):
        S.degree_assortativity(pp.Graph.from_edge_list([("a", "b"), ("b", "a")], device=DEV))
    with pytest.raises(KeyError):
        S.local_clustering_coefficient(g, "nobody")
    with pytest.raises(IndexError):
        NS.pairwise(g, torch.tensor([[0], [5]], device=DEV), "jaccard")


# ------------------------------------------------------------------ 3. where the kernel can go wrong
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
POOL = 1100


def lengths_graph():
    """Node i < len(LENGTHS) has LENGTHS[i] distinct successors drawn from all POOL nodes (the list nodes among them, so triads close);
    the other nodes have two successors each.  Columns sorted, no parallel edges: the stored list is its own simple structure."""
    rng = np.random.default_rng(11)
    edges = []
    for v in range(POOL):
        size = LENGTHS[v] if v < len(LENGTHS) else 2
        edges += [(v, int(w)) for w in np.sort(rng.choice(POOL, size=size, replace=False))]
    return np.array(edges, dtype=np.int64).T


LENGTHS_EI = lengths_graph()
LIST_PAIRS = np.array([[a for a in range(len(LENGTHS)) for _ in LENGTHS], [b for _ in LENGTHS for b in range(len(LENGTHS))]])
_EXPECTED = {}


def lengths_expected():
    if not _EXPECTED:
        _EXPECTED["triads"] = ops.triad_counts(LENGTHS_EI, POOL)
        _EXPECTED["pairs"] = ops.pair_table(LENGTHS_EI, POOL, LIST_PAIRS)
    return _EXPECTED


@pytest.mark.parametrize("heavy_min", [None, 8, 33])
@pytest.mark.parametrize("group", [None, 1, 2, 4, 8, 16, 32, 64])
def test_list_lengths_around_every_width_and_threshold(monkeypatch, group, heavy_min):
    """Lists of one less, exactly and one more than every group width (1 .. 64), the wave (63, 64, 65), the workgroup (255, 256, 257) and the
    default workgroup threshold (1023, 1024, 1025), with every width forced in turn and the threshold at its default, at 8 and at 33."""
    monkeypatch.setattr(_hip, "TRIAD_GROUP", group)
    monkeypatch.setattr(_hip, "TRIAD_HEAVY_MIN", heavy_min)
    want = lengths_expected()
    g = graph_of(LENGTHS_EI, POOL)
    assert np.array_equal(S.closed_triad_counts(g).cpu().numpy(), want["triads"])
    assert g._simple[3] is None                                                         # the fast path: nothing was coalesced
    pairs = torch.from_numpy(LIST_PAIRS).to(DEV)
    assert NS.pairwise(g, pairs, "common_neighbors").cpu().tolist() == want["pairs"]["common"]
    assert all(same(a, b) for a, b in zip(NS.pairwise(g, pairs, "jaccard").cpu().tolist(), want["pairs"]["jaccard"]))
    assert all(same(a, b) for a, b in zip(NS.pairwise(g, pairs, "cosine").cpu().tolist(), want["pairs"]["cosine"]))
    aa = NS.pairwise(g, pairs, "adamic_adar")
    for value, terms in zip(aa.cpu().tolist(), want["pairs"]["terms"]):
        check_aa(value, terms)
    assert torch.equal(NS.pairwise(g, pairs, "adamic_adar").view(torch.int64), aa.view(torch.int64))
    v = len(LENGTHS) - 1                                                                # the longest list through the fill
    assert S.closed_triads(g, v) == ops.closed_triads_of(LENGTHS_EI, POOL, v)


def test_hub_with_a_ring_of_leaves():
    """A long list against short ones: hub 0 joined to 4096 leaves that also form a ring, both directions stored."""
    leaves = 4096
    ring = [(1 + i, 1 + (i + 1) % leaves) for i in range(leaves)]
    spokes = [(0, 1 + i) for i in range(leaves)]
    both = sorted({(u, w) for u, w in ring + spokes} | {(w, u) for u, w in ring + spokes})
    g = graph_of(np.array(both, dtype=np.int64).T, leaves + 1, undirected=True)
    counts = check_clustering(g)
    assert counts[0] == 2 * leaves and (counts[1:] == 4).all()
    rng = np.random.default_rng(3)
    pairs = np.concatenate((rng.integers(0, leaves + 1, (2, 300)), [[0, 0, 5], [0, 7, 0]]), axis=1)
    check_pairs(g, pairs)
    assert len(S.closed_triads(g, 0)) == 2 * leaves


def test_two_hubs_sharing_most_neighbours():
    """A long list against a long one, through the workgroup launch: hubs 0 and 1 with 4000 successors each, 3000 of them shared, an
    edge between the hubs, parallel edges on some spokes; every leaf points back at both hubs and every third one at the next leaf."""
    first = 2
    edges = [(0, first + i) for i in range(4000)] + [(1, first + 1000 + i) for i in range(4000)] + [(0, 1), (1, 0)]
    edges += [(0, first + i) for i in range(0, 4000, 7)] + [(1, first + 1000 + i) for i in range(0, 4000, 5)]             # parallel spokes
    for i in range(5000):
        edges += [(first + i, 0), (first + i, 1)]
        if i % 3 == 0:
            edges.append((first + i, first + (i + 1) % 5000))
    ei = np.array(edges, dtype=np.int64).T
    g = graph_of(ei, first + 5000)
    assert g._simple is None
    counts = check_clustering(g)
    assert g._simple[3] is not None                                                     # parallel edges: the structure was coalesced
    assert counts[0] > 3000
    assert NS.common_neighbors(g, 0, 1) == 3000
    pairs = np.array([[0, 1, 0, 1, 2, 0, 4001], [1, 0, 0, 1, 3, 2, 1]])
    check_pairs(g, pairs)
    terms = ops.pair_table(stored(g)[0], g.n, [[0], [1]])["terms"][0]
    assert len(terms) == 3000 and all(math.isfinite(t) for t in terms)
    check_aa(NS.adamic_adar_index(g, 0, 1), terms)
    assert len(S.closed_triads(g, 0)) == counts[0]


def test_unsorted_parallel_and_looped_edges_against_the_coalesced_twin():
    rng = np.random.default_rng(17)
    n = 300
    simple = sorted({(int(u), int(w)) for u, w in rng.integers(0, n, (2500, 2))} | {(v, v) for v in range(0, n, 9)})
    messy = []
    for u, w in simple:
        messy += [(u, w)] * (3 if (u + w) % 4 == 0 else 1)
    order = rng.permutation(len(messy))                                                 # columns unsorted inside the rows after Graph's row sort
    twin, g = graph_of(np.array(simple, dtype=np.int64).T, n), graph_of(np.array(messy, dtype=np.int64)[order].T, n)
    assert any(u == w for u, w in simple) and len(messy) > len(simple)
    assert np.array_equal(check_clustering(g), check_clustering(twin))                  # the same sets: the same counts
    assert twin._simple[3] is None and g._simple[3] is not None
    assert torch.equal(g._simple[0], twin._simple[0]) and torch.equal(g._simple[2], twin._simple[2])
    deg_g, deg_t = ops.out_degrees(*stored(g)).astype(np.float64), ops.out_degrees(*stored(twin)).astype(np.float64)
    c_g, c_t = S.local_clustering_coefficients(g).cpu().numpy(), S.local_clustering_coefficients(twin).cpu().numpy()
    keep = (deg_t > 1) & (c_t > 0)
    assert keep.any() and (deg_g[keep] >= deg_t[keep]).all() and (deg_g > deg_t).any()
    np.testing.assert_allclose(c_g[keep] * deg_g[keep] * (deg_g[keep] - 1), c_t[keep] * deg_t[keep] * (deg_t[keep] - 1), rtol=4e-16)
    pairs = rng.integers(0, n, (2, 400))
    check_pairs(g, pairs)
    check_pairs(twin, pairs)
    for measure in ("common_neighbors", "jaccard", "overlap"):                          # set measures do not see the multiplicities
        a, b = NS.pairwise(g, torch.from_numpy(pairs).to(DEV), measure), NS.pairwise(twin, torch.from_numpy(pairs).to(DEV), measure)
        assert torch.equal(torch.nan_to_num(a.double(), nan=-1.0), torch.nan_to_num(b.double(), nan=-1.0))


def test_sorted_fast_path_and_coalesce_path_agree():
    rng = np.random.default_rng(23)
    n = 500
    simple = np.array(sorted({(int(u), int(w)) for u, w in rng.integers(0, n, (6000, 2))}), dtype=np.int64)
    fast = graph_of(simple.T, n)
    flipped = simple[np.lexsort((-simple[:, 1], simple[:, 0]))]                         # rows ascending, columns descending
    slow = graph_of(flipped.T, n)
    assert np.array_equal(check_clustering(fast), check_clustering(slow))
    assert fast._simple[3] is None and fast._simple[2].data_ptr() == fast.data.edge_index[1].data_ptr()
    assert slow._simple[3] is not None and bool((slow._simple[3] == 1).all())
    assert torch.equal(fast._simple[0], slow._simple[0]) and torch.equal(fast._simple[2], slow._simple[2])
    pairs = torch.from_numpy(rng.integers(0, n, (2, 500))).to(DEV)
    for measure in SCALAR:
        a, b = NS.pairwise(fast, pairs, measure), NS.pairwise(slow, pairs, measure)
        assert torch.equal(torch.nan_to_num(a.double(), nan=-1.0), torch.nan_to_num(b.double(), nan=-1.0)), measure
    und = fast.to_undirected()                                                          # a coalesce result: its own structure
    check_clustering(und)
    assert und._simple[3] is None


def test_empty_graphs_and_isolated_nodes():
    none = graph_of(np.zeros((2, 0), dtype=np.int64), 0)
    assert S.closed_triad_counts(none).shape == (0,) and S.closed_triad_counts(none).dtype == torch.int64
    assert S.local_clustering_coefficients(none).shape == (0,) and math.isnan(S.avg_clustering_coefficient(none))
    assert S.degree_distribution(none).shape == (0,) and math.isnan(S.mean_degree(none))
    assert NS.pairwise(none, torch.zeros((2, 0), dtype=torch.int64, device=DEV), "jaccard").shape == (0,)
    bare = graph_of(np.zeros((2, 0), dtype=np.int64), 5)
    assert S.closed_triad_counts(bare).tolist() == [0] * 5 and S.avg_clustering_coefficient(bare) == 0.0
    assert S.degree_distribution(bare).tolist() == [1.0] and S.mean_degree(bare) == 0.0
    assert NS.pairwise(bare, torch.tensor([[0, 4], [4, 4]], device=DEV), "jaccard").tolist() == [1.0, 1.0]
    assert math.isnan(NS.pairwise(bare, torch.tensor([[0], [4]], device=DEV), "overlap").item())
    with pytest.raises(ZeroDivisionError):
        S.mean_neighbor_degree(bare)
    ends = graph_of([[2, 2, 3, 3, 4, 4], [3, 4, 2, 4, 2, 3]], 8, undirected=True)      # nodes 0, 1 and 5, 6, 7 are isolated
    counts = check_clustering(ends)
    assert counts.tolist() == [0, 0, 2, 2, 2, 0, 0, 0]
    check_pairs(ends, [[0, 0, 7, 2, 7, 1], [0, 7, 7, 3, 2, 6]])
    assert S.closed_triads(ends, 0) == set() and S.closed_triads(ends, 7) == set()


def test_pair_batches():
    rng = np.random.default_rng(29)
    n = 400
    ei = rng.integers(0, n, (2, 5000)).astype(np.int64)
    g = graph_of(ei, n)
    for measure in SCALAR:
        empty = NS.pairwise(g, torch.zeros((2, 0), dtype=torch.int64, device=DEV), measure)
        assert empty.shape == (0,) and empty.dtype == (torch.int64 if measure == "common_neighbors" else torch.float64)
        assert NS.pairwise(g, [], measure).shape == (0,)
    check_pairs(g, [[7], [9]])                                                          # P = 1
    check_pairs(g, [[7, 9, 0], [7, 9, 0]])                                              # v == w
    few = rng.integers(0, n, (2, 500))
    many = few[:, rng.integers(0, 500, 70_000)]                                         # 70 000 pairs with repeats: many workgroups
    many[:, -1] = (n - 1, n - 1)
    check_pairs(g, many)


def test_second_order_layer_with_tuple_ids():
    t = pp.TemporalGraph.from_edge_list(REFERENCE_EXAMPLE, device=DEV)
    layer = pp.MultiOrderModel.from_temporal_graph(t, delta=15, max_order=2).layers[2]
    ei, n = stored(layer)
    assert n > 2 and ei.shape[1] > 2
    ids = [layer.mapping.to_id(i) for i in range(n)]
    assert all(isinstance(i, tuple) and len(i) == 2 for i in ids)
    counts = check_clustering(layer)
    coeff = ops.local_coefficients(ei, n, False)
    sets = ops.successor_sets(ei, n)
    table = ops.pair_table(ei, n, [[0] * n, list(range(n))])
    for v in range(n):
        triads = S.closed_triads(layer, ids[v])
        assert triads == {(ids[x], ids[y]) for x, y in ops.closed_triads_of(ei, n, v, sets)} and len(triads) == counts[v]
        assert S.local_clustering_coefficient(layer, ids[v]) == coeff[v]
        assert NS.common_neighbors(layer, ids[0], ids[v]) == table["common"][v]
        assert same(NS.jaccard_similarity(layer, ids[0], ids[v]), table["jaccard"][v])
        assert same(NS.cosine_similarity(layer, ids[0], ids[v]), table["cosine"][v])
        check_aa(NS.adamic_adar_index(layer, ids[0], ids[v]), table["terms"][v])
    got = NS.pairwise(layer, [(ids[0], ids[v]) for v in range(n)], "common_neighbors")
    assert got.tolist() == table["common"]


def test_cpu_resident_graph_is_staged():
    name = "ref_toy_directed"
    ei, n = GOLDEN[f"{name}/edge_index"], int(GOLDEN[f"{name}/n"])
    g = graph_of(ei, n, device="cpu")
    counts, coeff = S.closed_triad_counts(g), S.local_clustering_coefficients(g)
    assert counts.device.type == "cpu" and coeff.device.type == "cpu"
    assert np.array_equal(counts.numpy(), GOLDEN[f"{name}/triads"]) and np.array_equal(coeff.numpy(), GOLDEN[f"{name}/coeff"])
    assert all(t is None or t.device.type == "cpu" for t in g._simple)
    assert S.degree_distribution(g).device.type == "cpu"
    assert same(S.degree_assortativity(g), GOLDEN[f"{name}/total/scalars"][9])
    pairs = torch.tensor([[3, 0, 4], [4, 1, 6]])
    got = NS.pairwise(g, pairs, "jaccard")
    assert got.device.type == "cpu" and got.tolist() == [GOLDEN[f"{name}/pair/values"][2, 3, 4], GOLDEN[f"{name}/pair/values"][2, 0, 1],
                                                          ops.pair_table(ei, n, [[4], [6]])["jaccard"][0]]
    assert S.closed_triads(g, 3) == {(4, 5)}
    moved = g.to(DEV)
    assert all(t is None or t.device.type == "cuda" for t in moved._simple)
    assert np.array_equal(S.closed_triad_counts(moved).cpu().numpy(), GOLDEN[f"{name}/triads"])
