"""WeisfeilerLeman_test and color_refinement on the device (csrc/pp_graph_wl.hip) through the public functions, held to the fixtures made
from the reference's own function (tests/golden/wl_vectors.npz) and to the plain restatement (tests/cpu_ops_wl.py: dicts of tuples of sorted
colours, no hashes, no sort keys, no elections), at the smallest shapes at which each mechanism can fail: rows with equal colour sums, rows
longer than the heavy threshold that differ in one place, hundreds of rounds, first occurrences spread over workgroups, and the verify
passes that only run when row hashes collide (``HASH_MASK``).  Everything is an integer and every comparison is exact."""
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_wl as ops
import pathpyg_amd as pp
from pathpyg_amd import _hip
from pathpyg_amd.algorithms import WeisfeilerLeman_test, color_refinement, weisfeiler_leman

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "wl_vectors.npz", allow_pickle=False)
NAMES = [str(x) for x in GOLDEN["names"]]
PAIRS = list(ops.random_pairs(7, 300))
_unmasked: dict = {}                                                    # results of the unmasked runs, shared with the collision tests


def graph_of(ei, n, device=DEV, ids=None):
    """A Graph from a row-sorted edge list (the fixtures and generators sort)."""
    ei = torch.as_tensor(np.ascontiguousarray(ei), dtype=torch.int64).reshape(2, -1).to(device)
    return pp.Graph(pp.Data(edge_index=ei, num_nodes=n), mapping=None if ids is None else pp.IndexMap(list(ids)), _row_sorted=True)


def same_triple(got, expect):
    """Equal values AND equal element types ('1' is not 1)."""
    assert type(got) is tuple and type(got[0]) is bool and got[0] == expect[0]
    for a, b in zip(got[1:], expect[1:]):
        assert type(a) is list and a == b and [type(x) for x in a] == [type(x) for x in b]


@pytest.fixture
def mask(monkeypatch):
    def set_mask(value):
        monkeypatch.setattr(weisfeiler_leman, "HASH_MASK", value)
    return set_mask


# ------------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("device", [DEV, "cpu"])
@pytest.mark.parametrize("name", NAMES)
def test_fixture(name, device):
    case = ops.fixture_case(GOLDEN, name)
    g1 = graph_of(case["edge_index1"], len(case["ids1"]), device, case["ids1"])
    g2 = graph_of(case["edge_index2"], len(case["ids2"]), device, case["ids2"])
    same_triple(WeisfeilerLeman_test(g1, g2, case["features1"], case["features2"]), (case["result"], case["fp1"], case["fp2"]))


# ------------------------------------------------------------------ 2. random pairs
def run_pairs():
    """(triple, passes) of every random pair under the current HASH_MASK."""
    out = []
    for ids1, ei1, ids2, ei2, f1, f2 in PAIRS:
        got = WeisfeilerLeman_test(graph_of(ei1, len(ids1), ids=ids1), graph_of(ei2, len(ids2), ids=ids2), f1, f2)
        out.append((got, list(weisfeiler_leman.last_stats.passes)))
    return out


def restated_pairs():
    if "restated" not in _unmasked:
        _unmasked["restated"] = [ops.wl_test(ids1, ops.successor_lists(ei1, len(ids1)), ids2, ops.successor_lists(ei2, len(ids2)), f1, f2)
                                 for ids1, ei1, ids2, ei2, f1, f2 in PAIRS]
    return _unmasked["restated"]


def unmasked_pairs():
    if "pairs" not in _unmasked:
        assert weisfeiler_leman.HASH_MASK == 2 ** 64 - 1
        _unmasked["pairs"] = run_pairs()
    return _unmasked["pairs"]


def test_random_pairs_match_the_restatement():
    results = set()
    for (got, passes), expect in zip(unmasked_pairs(), restated_pairs()):
        same_triple(got, expect)
        assert passes[1:] == [1] * (len(passes) - 1)                    # a working hash: one verify pass in every round
        results.add(got[0])
    assert results == {True, False}


def refinement_inputs():
    """(succ, graph, initial, order, max_rounds) on the first graph of every random pair."""
    rng = np.random.default_rng(3)
    for i, (ids1, ei1, *_rest) in enumerate(PAIRS):
        n = len(ids1)
        initial = None if i % 3 == 0 else rng.choice(np.array([-5, 0, 7, 2 ** 40, -2 ** 50]), n)
        order = None if i % 4 == 0 else rng.permutation(n).astype(np.int64)
        yield ops.successor_lists(ei1, n), graph_of(ei1, n), initial, order, (0, 1, 2, None)[int(rng.integers(0, 4))]


def run_refinements():
    out = []
    for _, g, initial, order, max_rounds in refinement_inputs():
        tensors = [None if x is None else torch.from_numpy(x) for x in (initial, order)]
        if g.n % 2:                                                     # inputs on either side
            tensors = [None if t is None else t.to(DEV) for t in tensors]
        colours, counts, passes = color_refinement(g, initial=tensors[0], max_rounds=max_rounds, order=tensors[1], with_stats=True)
        assert colours.dtype == torch.int64 and colours.is_cuda and colours.shape == (g.n,)
        out.append((colours.cpu().tolist(), counts, passes))
    return out


def unmasked_refinements():
    if "refinements" not in _unmasked:
        assert weisfeiler_leman.HASH_MASK == 2 ** 64 - 1
        _unmasked["refinements"] = run_refinements()
    return _unmasked["refinements"]


def test_color_refinement_matches_the_restatement():
    for (colours, counts, passes), (succ, _, initial, order, max_rounds) in zip(unmasked_refinements(), refinement_inputs()):
        want_colours, want_counts = ops.refine(succ, initial, order, max_rounds)
        assert colours == want_colours and counts == want_counts
        assert len(passes) == len(counts) and passes[1:] == [1] * (len(counts) - 1)


# ------------------------------------------------------------------ 3. equal sum, different multiset
def equal_sum_graph():
    """Index order: S (a sink), X1 (out-degree 1), Y1 (2), X3 (3), Y2 (2), P -> X1, X3 and Q -> Y1, Y2.  After round 1 the colour is the
    rank of the out-degree by first occurrence: 0, 1, 2, 3; P and Q share colour 2 and degree 2, their successors' colours are (1, 3) and (2, 2)."""
    pairs = [(1, 0), (2, 0), (2, 0), (3, 0), (3, 0), (3, 0), (4, 0), (4, 0), (5, 1), (5, 3), (6, 2), (6, 4)]
    return np.array(pairs, dtype=np.int64).T, 7


def check_equal_sum():
    ei, n = equal_sum_graph()
    succ = ops.successor_lists(ei, n)
    assert ops.refine(succ, max_rounds=1)[0] == [0, 1, 2, 3, 2, 2, 2]
    after = ops.refine(succ, max_rounds=2)[0]
    assert after[5] != after[6]
    g = graph_of(ei, n)
    got = []
    for max_rounds in (1, 2, None):
        colours, counts, passes = color_refinement(g, max_rounds=max_rounds, with_stats=True)
        want = ops.refine(succ, max_rounds=max_rounds)
        assert (colours.cpu().tolist(), counts) == want
        got.append((colours.cpu().tolist(), counts, passes))
    assert got[1][0][5] != got[1][0][6] and got[2][0][5] != got[2][0][6]
    return got


def test_equal_sum_different_multiset():
    for _, _, passes in check_equal_sum():
        assert passes[1:] == [1] * (len(passes) - 1)


# ------------------------------------------------------------------ 4. long rows
HUB = 5000


def hub_graph(special1: int, special2: int, seed: int):
    """Six isolated palette nodes with the initial colours 0 .. 5 in index order (so that the numbering by first occurrence keeps the values),
    two hubs of colour 0 with HUB leaves each: HUB // 2 of colour 2, HUB // 2 - 1 of colour 4 and one of colour special1 / special2, stored
    in a shuffled order.  Returns (edge_index, n, initial)."""
    rng = np.random.default_rng(seed)
    n = 8 + 2 * HUB
    initial = np.zeros(n, dtype=np.int64)
    initial[:6] = np.arange(6)
    rows, cols = [], []
    for h, special in ((6, special1), (7, special2)):
        leaves = 8 + (h - 6) * HUB + np.arange(HUB)
        colours = np.array([2] * (HUB // 2) + [4] * (HUB // 2 - 1) + [special])
        shuffled = rng.permutation(HUB)
        initial[leaves[shuffled]] = colours
        rows.append(np.full(HUB, h))
        cols.append(leaves)
    return np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int64), n, initial


HUB_CASES = {"first": (1, 2), "last": (5, 4), "middle": (3, 4), "identical": (3, 3)}


def check_hubs(where):
    assert HUB >= _hip.wl_heavy_min()                                   # the rows take the workgroup-per-row kernels
    ei, n, initial = hub_graph(*HUB_CASES[where], seed=len(where))
    succ = ops.successor_lists(ei, n)
    g = graph_of(ei, n)
    out = []
    for max_rounds in (1, None):
        colours, counts, passes = color_refinement(g, initial=torch.from_numpy(initial), max_rounds=max_rounds, with_stats=True)
        colours = colours.cpu().tolist()
        assert (colours, counts) == ops.refine(succ, initial, None, max_rounds)
        assert (colours[6] == colours[7]) == (where == "identical")
        out.append((colours, counts, passes))
    return out


@pytest.mark.parametrize("where", list(HUB_CASES))
def test_long_rows(where):
    for _, _, passes in check_hubs(where):
        assert passes[1:] == [1] * (len(passes) - 1)


# ------------------------------------------------------------------ 5. many rounds
def path_pair(chord: bool):
    n = 600
    steps = np.stack([np.arange(n - 1), np.arange(1, n)])
    ei1 = np.concatenate([steps, steps[::-1]], axis=1)
    perm = np.random.default_rng(1).permutation(n)
    ei2 = perm[ei1]
    if chord:
        ei2 = np.concatenate([ei2, np.array([[perm[100], perm[400]], [perm[400], perm[100]]])], axis=1)
    ei1, ei2 = (e[:, np.argsort(e[0], kind="stable")].astype(np.int64) for e in (ei1, ei2))
    return [f"a{i:03d}" for i in range(n)], ei1, [f"b{i:03d}" for i in range(n)], ei2


def test_many_rounds():
    ids1, ei1, ids2, ei2 = path_pair(False)
    got = WeisfeilerLeman_test(graph_of(ei1, 600, ids=ids1), graph_of(ei2, 600, ids=ids2))
    stats = weisfeiler_leman.last_stats
    same_triple(got, ops.wl_test(ids1, ops.successor_lists(ei1, 600), ids2, ops.successor_lists(ei2, 600)))
    assert got[0] is True and len(stats.counts) - 1 == 300 and max(got[1] + got[2]) == 45149
    assert stats.counts[:4] == [1, 2, 3, 4] and stats.counts[-2:] == [300, 300] and stats.passes[1:] == [1] * 300


def test_many_rounds_with_a_chord():
    ids1, ei1, ids2, ei2 = path_pair(True)
    got = WeisfeilerLeman_test(graph_of(ei1, 600, ids=ids1), graph_of(ei2, 600, ids=ids2))
    same_triple(got, ops.wl_test(ids1, ops.successor_lists(ei1, 600), ids2, ops.successor_lists(ei2, 600)))
    assert got[0] is False


# ------------------------------------------------------------------ 6. numbering across workgroups
def test_numbering_across_workgroups():
    rng = np.random.default_rng(5)
    n = 70_000
    degree = rng.integers(0, 3, n)
    rows = np.repeat(np.arange(n), degree)
    ei = np.stack([rows, rng.integers(0, n, rows.size)]).astype(np.int64)
    initial = rng.choice(np.array([-7, 0, 3, 10 ** 12, 5]), n)
    order = rng.permutation(n).astype(np.int64)
    succ = ops.successor_lists(ei, n)
    g = graph_of(ei, n)
    first = [int(np.nonzero(initial == c)[0][np.argmin(order[initial == c])]) for c in np.unique(initial)]
    assert len({v // 256 for v in first}) == 5                          # the first occurrences lie in different workgroups
    for max_rounds, classes in ((0, 5), (1, None)):
        colours, counts = color_refinement(g, initial=torch.from_numpy(initial), max_rounds=max_rounds, order=torch.from_numpy(order).to(DEV))
        want_colours, want_counts = ops.refine(succ, initial, order, max_rounds)
        assert counts == want_counts and (classes is None or counts[-1] == classes) and counts[-1] < 200
        assert colours.cpu().tolist() == want_colours


# ------------------------------------------------------------------ 7. the collision path
@pytest.mark.parametrize("value", [0, 1])
def test_masked_hash_gives_the_same_pairs(mask, value):
    plain = unmasked_pairs()
    mask(value)
    masked = run_pairs()
    for (got, passes), (want, _) in zip(masked, plain):
        same_triple(got, want)
    if value == 0:
        assert any(max(passes[1:], default=0) >= 2 for _, passes in masked)


@pytest.mark.parametrize("value", [0, 1])
def test_masked_hash_gives_the_same_refinements(mask, value):
    plain = unmasked_refinements()
    mask(value)
    for (colours, counts, _), (want_colours, want_counts, _) in zip(run_refinements(), plain):
        assert colours == want_colours and counts == want_counts


@pytest.mark.parametrize("value", [0, 1])
def test_masked_hash_on_equal_sums_and_long_rows(mask, value):
    plain = [check_equal_sum()] + [check_hubs(where) for where in HUB_CASES]
    mask(value)
    masked = [check_equal_sum()] + [check_hubs(where) for where in HUB_CASES]
    for a, b in zip(plain, masked):
        assert [x[:2] for x in a] == [x[:2] for x in b]
    if value == 0:
        # by construction: P and Q (and Y1, Y2) share own colour 2 and degree 2 before round 2 and have distinct signatures, so without a
        # hash they share a group and the election takes one pass per signature; the two hubs likewise unless they are identical
        assert masked[0][1][2][2] >= 2
        for where, runs in zip(HUB_CASES, masked[1:]):
            assert (runs[0][2][1] >= 2) == (where != "identical")


# ------------------------------------------------------------------ 8. degenerate inputs
def test_degenerate_inputs():
    empty = graph_of(np.empty((2, 0), dtype=np.int64), 0)
    for max_rounds, want in ((None, [0, 0]), (0, [0]), (3, [0, 0])):
        colours, counts = color_refinement(empty, max_rounds=max_rounds)
        assert colours.shape == (0,) and colours.dtype == torch.int64 and counts == want
    edgeless = graph_of(np.empty((2, 0), dtype=np.int64), 5)
    colours, counts = color_refinement(edgeless)
    assert colours.cpu().tolist() == [0] * 5 and counts == [1, 1]
    colours, counts = color_refinement(edgeless, initial=torch.tensor([3, 3, 9, 3, 9]))
    assert colours.cpu().tolist() == [0, 0, 1, 0, 1] and counts == [2, 2]
    colours, counts = color_refinement(edgeless, initial=torch.tensor([3, 3, 9, 3, 9]), order=torch.tensor([4, 3, 0, 2, 1]), max_rounds=0)
    assert colours.cpu().tolist() == [1, 1, 0, 1, 0] and counts == [2]
    loop = graph_of(np.array([[0], [0]]), 1)
    colours, counts = color_refinement(loop)
    assert colours.cpu().tolist() == [0] and counts == [1, 1]
    ei = np.array([[0, 0, 1, 2], [1, 2, 2, 3]])
    wide = graph_of(ei, 10)                                             # nodes 4 .. 9 have no edge
    colours, counts = color_refinement(wide)
    assert (colours.cpu().tolist(), counts) == ops.refine(ops.successor_lists(ei, 10))
    same_triple(WeisfeilerLeman_test(graph_of(np.empty((2, 0), dtype=np.int64), 3, ids=["a", "b", "c"]),
                                     graph_of(np.empty((2, 0), dtype=np.int64), 3, ids=["x", "y", "z"])), (True, ["0"] * 3, ["0"] * 3))
    same_triple(WeisfeilerLeman_test(graph_of(np.empty((2, 0), dtype=np.int64), 3, ids=["a", "b", "c"]),
                                     graph_of(np.empty((2, 0), dtype=np.int64), 2, ids=["x", "y"])), (False, ["0"] * 3, ["0"] * 2))


def test_bad_arguments_are_refused():
    g = graph_of(np.array([[0, 1], [1, 2]]), 3)
    with pytest.raises(ValueError, match="order is not a permutation"):
        color_refinement(g, order=torch.tensor([0, 0, 2]))
    with pytest.raises(ValueError, match="order is not a permutation"):
        color_refinement(g, order=torch.tensor([0, 1, 3]))
    with pytest.raises(ValueError, match="one entry per node"):
        color_refinement(g, initial=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="one entry per node"):
        color_refinement(g, order=torch.tensor([0, 1, 2], dtype=torch.int32))
