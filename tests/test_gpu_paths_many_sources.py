"""pp_paths.hip with more source nodes than workgroups: k_temporal_bfs runs at most 2048 workgroups and k_temporal_betweenness at most
1024, each walks ``for (s = blockIdx.x; s < n; s += gridDim.x)`` and re-initialises its per-workgroup state (levels, queues, sigma, credit)
for the next source.  The random tests of tests/test_gpu_api.py stay below 60 and 40 nodes: no workgroup there takes a second source."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


def _stream(seed, n, m, span):
    rng = np.random.default_rng(seed)
    ei = torch.from_numpy(rng.integers(0, n, (2, m)))
    t = torch.from_numpy(np.sort(rng.integers(0, span, m)))
    return ei, t


def test_shortest_paths_with_more_sources_than_workgroups(pp):
    """2100 nodes: the sources 2048 .. 2099 are second sources of workgroups 0 .. 51.  Distances equal scipy's Dijkstra and the
    level-synchronous oracle, predecessors the latter (latest tight event)."""
    from oracle import temporal_paths as tp
    from pathpyg_amd import _hip
    n, m, delta = 2100, 20_000, 25
    ei, t = _stream(17, n, m, 300)
    # one workgroup per source up to the kernel's cap of 2048 (12 m bytes of state each): 52 workgroups take a second source
    ws_bytes = _hip.lib().pp_temporal_bfs_ws_bytes(m, n)
    assert 2048 * 12 * m <= ws_bytes < 2049 * 12 * m
    d_ref, _ = tp.temporal_shortest_paths_reference(ei, t, n, delta)
    d_bfs, p_bfs = tp.temporal_shortest_paths_bfs(ei, t, n, delta)
    far = [s for s in range(2048, n) if np.where(np.isfinite(d_bfs[s]), d_bfs[s], 0).max() >= 3]
    assert 2 * len(far) >= n - 2048, "the second-round sources must reach beyond their neighbours"
    g = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=n))
    dist, pred = pp.algorithms.temporal.temporal_shortest_paths(g, delta)
    assert np.array_equal(np.nan_to_num(dist, posinf=-1), np.nan_to_num(d_ref, posinf=-1))
    assert np.array_equal(np.nan_to_num(dist, posinf=-1), np.nan_to_num(d_bfs, posinf=-1))
    assert np.array_equal(pred, p_bfs)


def test_betweenness_with_more_sources_than_workgroups(pp):
    """1100 nodes: the sources 1024 .. 1099 are second sources of workgroups 0 .. 75; one of them has no out-going event (the kernel's
    ``continue`` in a second round)."""
    from oracle import temporal_paths as tp
    from pathpyg_amd import _dispatch, _hip
    n, m, delta = 1100, 9000, 25
    ei, t = _stream(19, n, m, 200)
    silent = 1060
    ei[0][ei[0] == silent] = 3                                         # node 1060 keeps its in-coming events and loses the out-going ones
    assert _hip.lib().pp_temporal_betweenness_parts(m, n) == 1024
    want = tp.temporal_betweenness_reference(ei, t, n, delta)
    assert 2 * int(np.count_nonzero(want[1024:])) >= n - 1024, "the second-round sources must carry weight"
    assert not bool((ei[0] == silent).any()) and bool((ei[1] == silent).any())
    got = _dispatch.temporal_betweenness(ei.to(DEV), t.to(DEV), n, delta).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-9)
