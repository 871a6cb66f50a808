"""The host half of the level-by-level builder on observed walks, without a GPU: ``_path_csr_layers`` turns int32 CSR layers and int32
inverse maps (what ``_hip.multi_order_paths`` returns) into the reference's layer tensors and mappings.  The CSR arrays are made here on the
CPU from the oracle's layers; the kernels themselves are checked on the GPU (``tests/test_gpu_path_builder.py``)."""
import numpy as np
import pytest
import torch

from oracle import aggregate as oa
from oracle import model as om
from pathpyg_amd._hip import MultiOrderLayer
from pathpyg_amd.core.index_map import IndexMap
from pathpyg_amd.core.multi_order_model import _path_csr_layers
from tests.cpu_ops_multiorder import CpuOpsMultiOrder

K = 5


@pytest.fixture(scope="module")
def built():
    """The *random* shape of tests/test_gpu_path_builder.py: walk store, oracle layers, and the builder's outputs restated on the CPU."""
    rng = np.random.default_rng(3)
    walks = [rng.integers(0, 30, int(rng.integers(1, 13))).tolist() for _ in range(400)]
    weights = (np.random.default_rng(17).random(len(walks)).astype(np.float32) + np.float32(0.25)).tolist()
    store = om.walks_to_path_tensors(walks, weights)
    want = om.layers_from_paths(store, max_order=K)
    csr, inverses = [], {}
    for k in range(1, K + 1):
        layer = want[k]
        n, edges = layer["num_nodes"], layer["edge_index"]
        parts = oa.csr_csc(edges, n)
        # the last first-order node of every edge of layer k = of every node of layer k + 1 (None for the top layer of a build)
        last = None if k == K else layer["node_sequence"][edges[1], -1].to(torch.int32)
        csr.append(MultiOrderLayer(n_nodes=n, n_edges=edges.size(1), n_instances=want[k + 1]["inverse_idx"].numel() if k < K else 0,
                                   row_ptr=parts["row_ptr"].to(torch.int32), col=parts["col"].to(torch.int32), weight=layer["edge_weight"].clone(),
                                   last=last))
        if k >= 2:
            inverses[k] = layer["inverse_idx"].to(torch.int32)
    return store, want, csr, inverses


@pytest.mark.parametrize("cached", [True, False])
def test_path_layers_from_csr_equal_the_oracle(built, cached):
    store, want, csr, inverses = built
    names = np.array([f"n{i}" for i in range(30)])
    mapping = IndexMap(names.tolist())
    kept = inverses if cached else {K: inverses[K]}
    layers = _path_csr_layers(mapping, store["node_sequence"], csr, kept, cached, gather_concat=CpuOpsMultiOrder.gather_concat)
    assert sorted(layers) == (list(range(1, K + 1)) if cached else [1, K])      # (layer 1 stays whatever `cached` says, as in the reference)
    assert layers[1].mapping is mapping
    for k, g in layers.items():
        d = g.data
        assert d.num_nodes == want[k]["num_nodes"] and g.order == k
        for key in ("edge_index", "edge_weight", "node_sequence", "inverse_idx"):
            assert d[key].dtype == want[k][key].dtype and torch.equal(d[key], want[k][key]), (k, key)
        if k >= 2:
            ids = g.mapping.node_ids
            assert ids.shape == (want[k]["num_nodes"], k) and (ids == names[want[k]["node_sequence"].numpy()]).all()
            first = tuple(names[want[k]["node_sequence"][0].numpy()].tolist())
            assert g.mapping.to_id(0) == first and g.mapping.to_idx(first) == 0
