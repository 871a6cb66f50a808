"""GPU parity tests of the level-by-level builder on OBSERVED WALKS (``pp_multiorder_prepare_paths`` / ``pp_multiorder_step`` /
``pp_multiorder_paths_inverse``: what ``MultiOrderModel.from_path_data(max_order >= 2, mode="propagation")`` runs on a device-resident walk
store) against the CPU oracle (reference src/pathpyG/core/multi_order_model.py:194-241, core/path_data.py:126-159), tensor by tensor, bit for
bit: merged weights are left-to-right fp32 sums in the reference's instance order, so fractional weights would show any other association.
Every test asserts the route it took (``"layers" in model.sizes`` = level by level)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("edge_index", "edge_weight", "node_sequence", "inverse_idx")


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


def _level_by_level(model) -> bool:
    return "layers" in getattr(model, "sizes", {})


def walks_of(shape: str) -> list:
    rng = np.random.default_rng(3)
    if shape == "random":            # 400 walks, 30 nodes, lengths 1..12 (every id 0..29 occurs)
        walks = [rng.integers(0, 30, int(rng.integers(1, 13))).tolist() for _ in range(400)]
    elif shape == "two_nodes":       # ~3150 edges on 4 node pairs: ~800 instances per type — k_mo_sums1_long and the workgroup children kernel
        walks = [rng.integers(0, 2, int(rng.integers(2, 9))).tolist() for _ in range(800)]
    elif shape == "boundaries":      # walk ends on and beside the wave (64) and workgroup (256) edges of the position kernels
        walks = [rng.integers(0, 50, n).tolist() for n in (1000, 256, 257, 255, 1, 2, 64, 65, 63)]
    elif shape == "cycles":
        walks = [[0, 1] * 6, [0, 0, 0, 0, 0], [1, 0, 1, 0], [1], [0], [1, 1], [0, 1]]
    else:
        raise ValueError(shape)
    return walks


def weights_of(walks: list, fractional: bool) -> list:
    rng = np.random.default_rng(17)
    if fractional:
        return (rng.random(len(walks)).astype(np.float32) + np.float32(0.25)).tolist()
    return rng.integers(1, 6, len(walks)).astype(np.float32).tolist()


_ORACLE = {}


def oracle_layers(shape: str, fractional: bool, K: int = 5):
    """The oracle's layers of a shape (cached=True), computed once per module run and left unchanged."""
    from oracle import model as om
    key = (shape, fractional, K)
    if key not in _ORACLE:
        walks = walks_of(shape)
        weights = weights_of(walks, fractional)
        _ORACLE[key] = (walks, weights, om.layers_from_paths(om.walks_to_path_tensors(walks, weights), max_order=K))
    return _ORACLE[key]


def _paths(pp, walks, weights, device=DEV, mapping=None):
    paths = pp.PathData(mapping, device=device)
    paths.append_walks(walks, weights)
    return paths


def _assert_layers(model, want: dict, keys=None):
    assert sorted(model.layers) == sorted(want if keys is None else keys)
    for k in model.layers:
        d = model.layers[k].data
        for key in KEYS:
            assert torch.equal(d[key].cpu(), want[k][key]), (k, key)
        assert d.num_nodes == want[k]["num_nodes"] and model.layers[k].order == k


# 1. levels equal the oracle
@pytest.mark.parametrize("fractional", [False, True])
@pytest.mark.parametrize("shape", ["random", "two_nodes", "boundaries", "cycles"])
def test_levels_equal_the_oracle(pp, shape, fractional):
    walks, weights, want = oracle_layers(shape, fractional)
    model = pp.MultiOrderModel.from_path_data(_paths(pp, walks, weights), max_order=5)
    assert _level_by_level(model), "from_path_data(max_order=5) did not take the level-by-level builder"
    _assert_layers(model, want)
    for k in range(1, 6):
        assert model.layers[k].data.inverse_idx.numel() == sum(max(len(w) - k + 1, 0) for w in walks), k
    sizes = model.sizes["layers"]
    assert sizes[0][2] == sum(len(w) - 1 for w in walks) and all(sizes[k][0] == sizes[k - 1][1] for k in range(1, len(sizes)))


# 2. cached=False: the reference (and the generic route) keeps layer 1 whatever `cached` says, and the top layer
@pytest.mark.parametrize("K", [2, 3, 5])
def test_top_layer_only(pp, K):
    walks, weights, want = oracle_layers("random", True)
    model = pp.MultiOrderModel.from_path_data(_paths(pp, walks, weights), max_order=K, cached=False)
    assert _level_by_level(model)
    _assert_layers(model, want, keys=[1, K])


# 3. the 4096-children limit from both sides
def _copies(count: int):
    return [[0, 1, 2, 3]] * count, [0.5 + (i % 7) for i in range(count)]


def test_a_type_with_4000_children_takes_the_fast_route(pp):
    from oracle import model as om
    walks, weights = _copies(4000)
    want = om.layers_from_paths(om.walks_to_path_tensors(walks, weights), max_order=3)
    model = pp.MultiOrderModel.from_path_data(_paths(pp, walks, weights), max_order=3)
    assert _level_by_level(model)
    _assert_layers(model, want)


def test_a_type_with_5000_children_falls_back(pp):
    from oracle import model as om
    walks, weights = _copies(5000)
    want = om.layers_from_paths(om.walks_to_path_tensors(walks, weights), max_order=3)
    model = pp.MultiOrderModel.from_path_data(_paths(pp, walks, weights), max_order=3)
    assert not _level_by_level(model), "a type with 5000 children cannot come out of the level-by-level builder (kMoBigMax = 4096)"
    _assert_layers(model, want)


# 4. fallbacks: the generic route, same layers
def test_diffusion_mode_takes_the_generic_route(pp):
    from oracle import model as om
    walks, weights, _ = oracle_layers("random", False)
    want = om.layers_from_paths(om.walks_to_path_tensors(walks, weights), max_order=3, mode="diffusion")
    model = pp.MultiOrderModel.from_path_data(_paths(pp, walks, weights), max_order=3, mode="diffusion")
    assert not _level_by_level(model)
    assert sorted(model.layers) == [1, 2, 3]
    for k in want:
        d = model.layers[k].data
        for key in ("edge_index", "node_sequence", "inverse_idx"):
            assert torch.equal(d[key].cpu(), want[k][key]), (k, key)
        # (diffusion weights are quotients and products: the generic kernels' own contract, tests/test_gpu_api.py)
        torch.testing.assert_close(d.edge_weight.cpu(), want[k]["edge_weight"], rtol=1e-6, atol=1e-7)


def test_host_resident_walks_take_the_generic_route(pp):
    walks, weights, want = oracle_layers("random", True)
    model = pp.MultiOrderModel.from_path_data(_paths(pp, walks, weights, device=None), max_order=5)
    assert not _level_by_level(model)
    _assert_layers(model, want)


def test_float64_walk_weights_take_the_generic_route(pp):
    from oracle import model as om
    walks, weights, _ = oracle_layers("random", False)
    ref = om.walks_to_path_tensors(walks, weights)
    ref["dag_weight"] = ref["dag_weight"].double()
    want = om.layers_from_paths(ref, max_order=3)
    paths = _paths(pp, walks, weights)
    paths.data.dag_weight = paths.data.dag_weight.double()
    model = pp.MultiOrderModel.from_path_data(paths, max_order=3)
    assert not _level_by_level(model)
    _assert_layers(model, want)


def test_node_ids_with_a_gap_take_the_generic_route(pp):
    from oracle import model as om
    walks, weights = [[0, 2, 3], [2, 3, 0, 2], [7]], [1.0, 2.0, 1.5]
    want = om.layers_from_paths(om.walks_to_path_tensors(walks, weights), max_order=3)
    model = pp.MultiOrderModel.from_path_data(_paths(pp, walks, weights), max_order=3)
    assert not _level_by_level(model)
    _assert_layers(model, want)


def test_a_foreign_edge_index_takes_the_generic_route(pp):
    from oracle import model as om
    walks, weights, _ = oracle_layers("random", True)
    ref = om.walks_to_path_tensors(walks, weights)
    # two columns swapped by hand: the same edges, no longer the chain in position order.  The line-graph lift (the reference's as the generic
    # kernels': lift_order.py:62-79) finds an edge's continuations at the column its head would have in a source-sorted edge_index, so the
    # columns are the edges of two two-node walks — nobody's continuation, continued by nobody: the walks stay what they are for every route,
    # only the instance order (and with it the summation order and inverse_idx of layers 1 and 2) follows the columns
    starts = np.cumsum([0] + [len(w) for w in walks])
    a, b = [int(starts[i]) - i for i, w in enumerate(walks) if len(w) == 2][:2]
    ei = ref["edge_index"].clone()
    ei[:, [a, b]] = ei[:, [b, a]]
    assert not torch.equal(ei, ref["edge_index"])
    ref["edge_index"] = ei
    want = om.layers_from_paths(ref, max_order=3)
    paths = _paths(pp, walks, weights)
    paths.data.edge_index = ei.to(DEV)
    model = pp.MultiOrderModel.from_path_data(paths, max_order=3)
    assert not _level_by_level(model)
    _assert_layers(model, want)


def test_an_order_beyond_the_longest_walk_takes_the_generic_route(pp):
    from oracle import model as om
    rng = np.random.default_rng(9)
    walks = [rng.integers(0, 5, int(rng.integers(1, 4))).tolist() for _ in range(60)] + [[0, 1, 2], [3, 4]]
    weights = weights_of(walks, True)
    want = om.layers_from_paths(om.walks_to_path_tensors(walks, weights), max_order=4)
    assert want[3]["num_nodes"] > 0 and want[3]["edge_index"].size(1) == 0 and want[4]["num_nodes"] == 0
    model = pp.MultiOrderModel.from_path_data(_paths(pp, walks, weights), max_order=4)
    assert not _level_by_level(model)
    _assert_layers(model, want)


# 5. the generic lift does not run
def test_the_generic_lift_does_not_run(pp, monkeypatch):
    from pathpyg_amd.core import multi_order_model as mom
    walks, weights, want = oracle_layers("random", True)
    paths = _paths(pp, walks, weights, mapping=pp.IndexMap(list(range(30))))       # (estimate_order compares the node ids of walks and model)

    def answers(model):
        out = [[model.layers[k].data[key].clone() for key in KEYS] for k in range(1, 5)]
        llh = [model.get_mon_log_likelihood(paths.data, k) for k in range(5)]
        return out, llh, model.estimate_order(paths, max_order=4)

    def boom(*a, **kw):
        raise AssertionError("the generic lift ran")

    with monkeypatch.context() as mp:
        mp.setattr(mom._LiftChain, "first_order", staticmethod(boom))
        mp.setattr(mom._LiftChain, "lift", boom)
        model = pp.MultiOrderModel.from_path_data(paths, max_order=4)
        assert _level_by_level(model)
        fast = answers(model)
    with monkeypatch.context() as mp:
        mp.setattr(mom, "FUSED_BUILDER", False)
        generic = pp.MultiOrderModel.from_path_data(paths, max_order=4)
        assert not _level_by_level(generic)
        slow = answers(generic)
    for a, b in zip(fast[0], slow[0]):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x, y)
    assert fast[1] == slow[1] and fast[2] == slow[2]
    _assert_layers(model, want, keys=[1, 2, 3, 4])


# 6. the device function called directly
def test_multi_order_paths_directly(pp):
    from pathpyg_amd import _hip
    from oracle import aggregate as oa
    walks, weights, want = oracle_layers("random", True)
    d = _paths(pp, walks, weights).data
    built = _hip.multi_order_paths(d.node_sequence, d.dag_num_nodes, d.dag_weight, d.edge_index, 30, 5)
    assert built is not None
    layers, inverses = built
    assert len(layers) == 5 and sorted(inverses) == [2, 3, 4, 5]
    for k, b in enumerate(layers, start=1):
        csr = oa.csr_csc(want[k]["edge_index"], want[k]["num_nodes"])
        assert b.n_nodes == want[k]["num_nodes"] and b.n_edges == want[k]["edge_index"].size(1)
        assert b.row_ptr.dtype == torch.int32 and torch.equal(b.row_ptr.cpu().long(), csr["row_ptr"])
        assert b.col.dtype == torch.int32 and torch.equal(b.col.cpu().long(), csr["col"])
        assert torch.equal(b.weight.cpu(), want[k]["edge_weight"])
        if k >= 2:
            assert inverses[k].dtype == torch.int32 and torch.equal(inverses[k].cpu().long(), want[k]["inverse_idx"])
            # the instances of level k - 1 (= the children of level k - 2, kept as layer k - 1's n_instances) are what layer k's inverse lists
            assert layers[k - 2].n_instances == inverses[k].numel()
    # status bits 3 / 5: ids that are not 0 .. n - 1, walk lengths that do not fit the store
    assert _hip.multi_order_paths(d.node_sequence, d.dag_num_nodes, d.dag_weight, d.edge_index, 31, 3) is None
    lengths = d.dag_num_nodes.clone()
    lengths[0] += 1
    lengths[1] -= 1
    assert _hip.multi_order_paths(d.node_sequence, lengths, d.dag_weight, d.edge_index, 30, 3) is None
