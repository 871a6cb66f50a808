"""Host-side checks for connected components: the restatement (tests/cpu_ops_components.py) against the fixtures made from scipy and the
reference's own ``largest_connected_component`` (tests/golden/components_vectors.npz) and against scipy itself, and what the public
functions decide before any device is touched.  All comparisons are exact."""
import pathlib

import numpy as np
import pytest

import cpu_ops_components as ops

GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "components_vectors.npz", allow_pickle=False)
NAMES = [str(x) for x in GOLDEN["names"]]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_fixture(name):
    get = lambda key: GOLDEN[f"{name}/{key}"]  # noqa: E731
    ei, n = get("edge_index"), int(get("n"))
    weak, strong = ops.weak_labels(ei, n), ops.strong_labels(ei, n)
    assert weak.dtype == np.int32 and np.array_equal(weak, get("weak"))                 # scipy numbers weak components by first appearance
    assert np.array_equal(weak, get("undirected"))
    assert int(strong.max()) + 1 == int(get("strong").max()) + 1
    assert np.array_equal(strong, ops.by_smallest_member(get("strong")))                # the same partition
    for kind, lab, scipy_lab in (("weak", weak, get("weak")), ("strong", strong, get("strong")), ("undirected", weak, get("undirected"))):
        keep = ops.largest_label(lab)
        assert keep == ops.by_smallest_member(scipy_lab)[np.nonzero(scipy_lab == int(get(f"lcc_{kind}_label")))[0][0]]
        assert np.array_equal(ops.kept_edges(ei, lab, keep), get(f"lcc_{kind}"))
        size = ops.sizes(lab)
        assert size.sum() == n and size[keep] == size.max() and (size[:keep] < size[keep]).all()


def test_restatement_matches_scipy_on_random_graphs():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, 40))
        m = int(rng.integers(0, 3 * n + 1))
        ei = rng.integers(0, n, (2, m)).astype(np.int64)
        adj = coo_matrix((np.ones(m), (ei[0], ei[1])), shape=(n, n))
        count, weak = csgraph.connected_components(adj, directed=True, connection="weak")
        assert np.array_equal(ops.weak_labels(ei, n), weak)
        count, strong = csgraph.connected_components(adj, directed=True, connection="strong")
        mine = ops.strong_labels(ei, n)
        assert int(mine.max()) + 1 == count and np.array_equal(mine, ops.by_smallest_member(strong))
        assert np.array_equal(ops.weak_labels(ei, n), csgraph.connected_components(adj, directed=False, connection="strong")[1])


def test_names_are_exported():
    import pathpyg_amd as pp
    from pathpyg_amd.algorithms import components, connected_components, largest_connected_component
    assert components.connected_components is connected_components is pp.algorithms.connected_components
    assert components.largest_connected_component is largest_connected_component is pp.algorithms.largest_connected_component


class _NoDeviceGraph:
    """Stands where a Graph would: any access beyond the direction flag is an error."""

    def is_undirected(self):
        return False

    def __getattr__(self, name):
        raise AssertionError(f"the graph's {name} was read before `connection` was checked")


@pytest.mark.parametrize("bad", ["", "weakly", "both", None, 1])
def test_connection_is_validated_before_the_device(bad):
    from pathpyg_amd.algorithms import connected_components, largest_connected_component
    for fn in (connected_components, largest_connected_component):
        with pytest.raises(ValueError, match="connection must be 'weak' or 'strong'"):
            fn(_NoDeviceGraph(), connection=bad)


def test_connection_case_is_folded():
    from pathpyg_amd.algorithms import components

    class Flagged:
        def __init__(self, undirected):
            self.undirected = undirected

        def is_undirected(self):
            return self.undirected

    assert components._strong(Flagged(False), "STRONG") and components._strong(Flagged(False), "Strong")
    assert not components._strong(Flagged(False), "WEAK") and not components._strong(Flagged(False), "weak")
    assert not components._strong(Flagged(True), "strong")                              # undirected: the weak components, whatever is asked


def test_id_order_follows_from_edge_list():
    from pathpyg_amd.algorithms import components
    for ids in (["10", "9", "2", "b"], ["10", "9", "2"], [3, 11, 7], ["v1000", "v999"]):
        kept = np.array(ids)
        node_ids, rank = components._ordered_ids(kept)
        expect = np.unique(np.array(ids))                                               # Graph.from_edge_list's rule (core/graph.py), restated
        if np.issubdtype(expect.dtype, np.str_) and np.char.isnumeric(expect).all():
            expect = np.sort(expect.astype(int)).astype(str)
        assert node_ids.tolist() == expect.tolist() and node_ids[rank].tolist() == kept.tolist()
