"""GPU tests of the native order selection (``csrc/pp_selection.hip``: ``pp_walk_counts_i64``, ``pp_mon_layer_llh_f64``,
``pp_mon_zeroth_llh_f64`` and their routing in ``MultiOrderModel``; reference src/pathpyG/core/multi_order_model.py:243-509).

Expected values are computed here: walk counts in exact Python ints, likelihood terms in float64 (``math.fsum`` of float64 summands, so the
expectation's own error is one rounding) from the CPU oracle's layers.

The likelihood bound: a term's result must lie within ``1e-12 * B`` of the float64 formula, ``B = sum |w| (1 + |log p|)`` over its summands.
Each summand takes fewer than ten roundings of 2^-53 and a tree sum adds at most log2(count) * 2^-53 of sum |summand|; 1e-12 is about
9000 * 2^-53, two orders of magnitude above that, and four orders below what a float32 intermediate costs."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-12


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


@pytest.fixture(scope="module")
def hip(pp):
    from pathpyg_amd import _hip
    return _hip


@pytest.fixture()
def mom(pp):
    from pathpyg_amd.core import multi_order_model
    return multi_order_model


# ------------------------------------------------------------------ walk stores (the shapes of tests/test_gpu_path_builder.py)
def walks_of(shape: str) -> list:
    rng = np.random.default_rng(3)
    if shape == "random":            # 400 walks, 30 nodes, lengths 1..12 (every id 0..29 occurs)
        return [rng.integers(0, 30, int(rng.integers(1, 13))).tolist() for _ in range(400)]
    if shape == "two_nodes":         # 800 walks on two nodes: about 800 instances per row
        return [rng.integers(0, 2, int(rng.integers(2, 9))).tolist() for _ in range(800)]
    if shape == "boundaries":        # one-node walks, walks kept / dropped at every order, ends beside the wave and workgroup sizes
        return [rng.integers(0, 50, n).tolist() for n in (1000, 256, 257, 255, 1, 2, 64, 65, 63)]
    raise ValueError(shape)


def weights_of(walks: list) -> list:
    rng = np.random.default_rng(17)
    return (rng.random(len(walks)).astype(np.float32) + np.float32(0.25)).tolist()


_ORACLE = {}


def oracle_layers(shape: str, K: int = 4):
    """(walks, weights, oracle layers 1..K), computed once per module run and left unchanged."""
    from oracle import model as om
    if shape not in _ORACLE:
        walks = walks_of(shape)
        weights = weights_of(walks)
        _ORACLE[shape] = (walks, weights, om.layers_from_paths(om.walks_to_path_tensors(walks, weights), max_order=K))
    return _ORACLE[shape]


def _paths(pp, walks, weights, mapping=None, device=DEV):
    paths = pp.PathData(mapping, device=device)
    paths.append_walks(walks, weights)
    return paths


# ------------------------------------------------------------------ float64 expectations
def _term(weight, p):
    """(sum w log p, B) of one term, float64 summands added exactly."""
    weight, p = np.asarray(weight, dtype=np.float64), np.asarray(p, dtype=np.float64)
    logp = np.log(p)
    return math.fsum((weight * logp).tolist()), math.fsum((np.abs(weight) * (1 + np.abs(logp))).tolist())


def _segment_fsum(values, segment, count):
    buckets = [[] for _ in range(count)]
    for v, s in zip(np.asarray(values, dtype=np.float64).tolist(), np.asarray(segment).tolist()):
        buckets[s].append(v)
    return np.array([math.fsum(b) for b in buckets], dtype=np.float64)


def expect_top(layer):
    rows = layer["edge_index"][0].numpy()
    w = layer["edge_weight"].numpy().astype(np.float64)
    s = _segment_fsum(w, rows, layer["num_nodes"])
    return _term(w, w / s[rows])


def expect_intermediate(layers, walks, weights, order):
    lengths = np.array([len(w) for w in walks]) - order
    keep = lengths > 0
    kept = lengths[keep]
    first = np.cumsum(kept) - kept
    sel = layers[order + 1]["inverse_idx"].numpy()[first]
    rows = layers[order]["edge_index"][0].numpy()
    deg = np.bincount(rows, minlength=layers[order]["num_nodes"])
    return _term(np.asarray(weights, dtype=np.float32)[keep], 1.0 / deg[rows[sel]])


def expect_zeroth(walks, weights):
    flat = np.array([v for w in walks for v in w])
    f = np.asarray(weights, dtype=np.float32).astype(np.float64)
    counts = np.bincount(flat)
    z = _term(f, counts[[w[0] for w in walks]] / flat.size)
    c = _segment_fsum(np.repeat(f, [len(w) for w in walks]), flat, counts.size)
    z0 = _term(c, c / math.fsum(c.tolist()))
    return z, z0


def _check(name, got, want):
    value, b = want
    err = abs(got - value)
    print(f"{name}: got {got!r} want {value!r} err/B {err / b if b else err:.3e}")
    assert err <= BOUND * b, (name, got, value, err / b if b else err)


# ------------------------------------------------------------------ exact walk counts
def exact_walk_counts(succ: list, K: int):
    c = [len(s) for s in succ]
    totals, starts = [], []
    for k in range(K):
        if k:
            c = [sum(c[u] for u in s) for s in succ]
        totals.append(sum(c))
        starts.append(sum(1 for x in c if x > 0))
    return totals, starts


def _csr(succ: list, dtype):
    ptr = np.concatenate(([0], np.cumsum([len(s) for s in succ])))
    col = np.array([u for s in succ for u in s], dtype=np.int64)
    return torch.tensor(ptr, dtype=dtype, device=DEV), torch.tensor(col, dtype=dtype, device=DEV)


def _dense_succ(adj) -> list:
    return [np.nonzero(row)[0].tolist() for row in adj]


def _walk_count_graphs():
    rng = np.random.default_rng(5)
    out = {"random": (_dense_succ(rng.random((40, 40)) < 0.3), 5),
           # (K = 40: a walk of a 40-node DAG has at most 39 edges, so the totals reach 0; the first five orders are the K = 5 answer)
           "dag": (_dense_succ(np.triu(rng.random((40, 40)) < 0.2, 1)), 40),
           # rows 0, 3, 7 empty, 5 and 6 isolated, a loop, a two-cycle
           "empty_rows": ([[], [2, 4], [1], [], [4, 0], [], [], []], 5),
           "self_loop": ([[0]], 5)}
    hub = [[] for _ in range(10001)]
    hub[0] = list(range(1, 5001))                       # 5000 out-edges of node 0 ...
    for i in range(1, 5001):
        hub[i] = [i + 5000]
        hub[i + 5000] = [0]                             # ... and 5000 in-edges
    out["hub"] = (hub, 3)
    return out


@pytest.mark.parametrize("name", ["random", "dag", "empty_rows", "self_loop", "hub"])
def test_walk_counts(hip, name):
    succ, K = _walk_count_graphs()[name]
    want = exact_walk_counts(succ, K)
    got = {}
    for dtype in (torch.int32, torch.int64):
        ptr, col = _csr(succ, dtype)
        got[dtype] = hip.walk_counts(ptr, col, len(succ), K)
        assert got[dtype] == want, (name, dtype, got[dtype], want)
    assert got[torch.int32] == got[torch.int64]
    assert all(type(x) is int for x in got[torch.int64][0] + got[torch.int64][1])
    if name == "dag":
        assert want[1][4] < want[1][0] and want[0][4] > 0 and want[0][-1] == 0 and want[1][-1] == 0      # sinks: starts shrink, totals reach 0
    if name == "hub":
        assert want[0][0] == 15000
    # mixed widths, and a column outside [0, n) is reported, not read
    ptr, col = _csr(succ, torch.int64)
    assert hip.walk_counts(ptr.int(), col, len(succ), K) == want
    bad = col.clone()
    bad[-1] = len(succ)
    with pytest.raises(IndexError):
        hip.walk_counts(ptr, bad, len(succ), 1)                 # (order 1 reads no column: they are checked whatever K)
    with pytest.raises(ValueError):
        hip.walk_counts(ptr, torch.cat((col, col[-1:])), len(succ), K)      # row_ptr does not end at the entry count


# ------------------------------------------------------------------ beyond 2^31
@pytest.fixture(scope="module")
def complete216(pp):
    """The complete digraph with loops on 216 nodes as 46 656 two-node walks plus one five-node walk (the store as ``append_walks`` lays it
    out, made in one piece: 46 657 ``append_walk`` calls would take seconds)."""
    from oracle import model as om
    n = 216
    walks = [[a, b] for a in range(n) for b in range(n)] + [[0, 1, 2, 3, 4]]
    paths = pp.PathData(pp.IndexMap(list(range(n))), device=DEV)
    store = om.walks_to_path_tensors(walks, [1.0] * len(walks))
    paths.data = pp.Data(**{key: value.to(DEV) for key, value in store.items()})
    paths.data.num_nodes = int(store["node_sequence"].size(0))
    return paths


def test_dof_beyond_int32_instances(pp, hip, complete216):
    n = 216
    model = pp.MultiOrderModel.from_path_data(complete216, max_order=3)
    want = n - 1 + sum(n ** (k + 1) - n for k in (1, 2, 3))
    assert n ** 4 >= 2 ** 31
    assert model.get_mon_dof(3) == want
    assert [model.get_mon_dof(k) for k in range(3)] == [n - 1 + sum(n ** (j + 1) - n for j in range(1, k + 1)) for k in range(3)]
    succ = [list(range(n))] * n
    ptr, col = _csr(succ, torch.int32)
    totals, starts = hip.walk_counts(ptr, col, n, 7)
    assert totals == [n ** (k + 1) for k in range(1, 8)] and starts == [n] * 7 and n ** 8 < 2 ** 63
    with pytest.raises(OverflowError) as err:
        hip.walk_counts(ptr, col, n, 9)
    assert "length 8" in str(err.value)                 # 216^9 >= 2^63 is the first count that leaves int64
    assert err.value.starts == [n] * 9
    assert err.value.totals[:7] == totals and err.value.totals[7:] == [2 ** 63 - 1] * 2


# ------------------------------------------------------------------ no lift
def test_selection_runs_no_lift(pp, mom, monkeypatch):
    walks, weights, _ = oracle_layers("random")
    paths = _paths(pp, walks, weights, mapping=pp.IndexMap(list(range(30))))
    model = pp.MultiOrderModel.from_path_data(paths, max_order=4)
    with monkeypatch.context() as off:
        off.setattr(mom, "NATIVE_SELECTION", False)
        dof_off = [model.get_mon_dof(k) for k in range(5)]
        order_off = model.estimate_order(paths, max_order=4)

    def boom(*a, **kw):
        raise AssertionError("a line-graph lift ran")

    monkeypatch.setattr(mom, "lift_order_edge_index", boom)
    assert [model.get_mon_dof(k) for k in range(5)] == dof_off
    assert model.estimate_order(paths, max_order=4) == order_off


# ------------------------------------------------------------------ likelihood accuracy
@pytest.mark.parametrize("shape", ["random", "two_nodes", "boundaries"])
def test_likelihood_terms_are_float64(pp, hip, mom, monkeypatch, shape):
    walks, weights, layers = oracle_layers(shape)
    n = layers[1]["num_nodes"]
    paths = _paths(pp, walks, weights, mapping=pp.IndexMap(list(range(n))))
    model = pp.MultiOrderModel.from_path_data(paths, max_order=4)
    d = paths.data
    want_z, want_z0 = expect_zeroth(walks, weights)
    z, z0 = model.get_zeroth_order_log_likelihood(d), model.get_mon_log_likelihood(d, 0)
    _check("Z", z, want_z)
    _check("Z0", z0, want_z0)
    inter, top = {}, {}
    for k in range(1, 5):
        if k < 4:
            inter[k] = model.get_intermediate_order_log_likelihood(d, k)
            _check(f"I{k}", inter[k], expect_intermediate(layers, walks, weights, k))
        # T_k from the oracle's layer, uploaded: a pure function of the values, so it is the model's own T_k bit for bit (checked below)
        rows = layers[k]["edge_index"][0]
        ptr = torch.zeros(layers[k]["num_nodes"] + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=layers[k]["num_nodes"]), 0)
        top[k] = hip.mon_layer_llh(ptr.to(DEV), layers[k]["edge_weight"].to(DEV))[0]
        _check(f"T{k}", top[k], expect_top(layers[k]))
    llh = [model.get_mon_log_likelihood(d, k) for k in range(5)]
    assert llh[0] == z0
    for k in range(1, 5):
        total = z
        for j in range(1, k):
            total += inter[j]
        assert llh[k] == total + top[k], (k, llh[k], total + top[k])
    monkeypatch.setattr(mom, "NATIVE_SELECTION", False)
    for k in range(5):
        assert np.isclose(llh[k], model.get_mon_log_likelihood(d, k)), k


# ------------------------------------------------------------------ one layer directly
def test_layer_terms_directly(hip):
    rng = np.random.default_rng(11)
    lengths = [0, 0, 70000, 0]
    for i in range(3000):
        lengths += [1] if i % 3 else [1, 0]              # empty rows between the one-edge rows
    lengths += [0, 0]
    lengths = np.array(lengths)
    ptr = np.concatenate(([0], np.cumsum(lengths)))
    A = int(ptr[-1])
    w = np.exp2(rng.uniform(-20, 20, A)).astype(np.float32)
    rows = np.repeat(np.arange(lengths.size), lengths)
    # first / last edge of the long row (edge 0 is its first), edges next to empty rows, the last edge, repeats
    sel = np.array([0, 69999, 70000, 70001, 70002, 0, 69999, A - 1, A - 2, A - 1, 35000, 70000] + rng.integers(0, A, 5000).tolist())
    freq = (rng.random(sel.size) * 3 + 0.1).astype(np.float32)
    s = _segment_fsum(w, rows, lengths.size)
    want_t = _term(w, w.astype(np.float64) / s[rows])
    want_i = _term(freq, 1.0 / lengths[rows[sel]])
    got = {}
    for pt in (torch.int32, torch.int64):
        for st in (torch.int32, torch.int64):
            args = (torch.tensor(ptr, dtype=pt, device=DEV), torch.tensor(w, device=DEV), torch.tensor(sel, dtype=st, device=DEV), torch.tensor(freq, device=DEV))
            got[pt, st] = hip.mon_layer_llh(*args)
            assert hip.mon_layer_llh(*args) == got[pt, st]                  # two consecutive calls: bit-equal
    first = got[torch.int32, torch.int32]
    assert all(v == first for v in got.values()), got
    _check("T", first[0], want_t)
    _check("I", first[1], want_i)
    assert hip.mon_layer_llh(args[0], args[1]) == (first[0], 0.0)
    for bad in (A, -1):
        outside = args[2].clone()
        outside[7] = bad
        with pytest.raises(IndexError):
            hip.mon_layer_llh(args[0], args[1], outside, args[3])


# ------------------------------------------------------------------ fallbacks
def test_ids_with_a_gap_take_the_torch_route(pp, hip, mom, monkeypatch):
    # The model: the 400-walk shape (a walk store with a gap cannot build one: layer 1 uses the ids as given).  The walks that are scored:
    # the same walks with id 17 unused, so the lengths - and with them every first-of-walk offset into the model's inverse_idx - stay valid.
    full, weights, _ = oracle_layers("random")
    walks = [[16 if v == 17 else v for v in w] for w in full]                # id 17 is mapped but unused
    # (the torch route indexes the counts of the 29 ids that occur by node id: a walk that STARTS at id 29 would read past them)
    walks = [[28 if w[0] == 29 else w[0]] + w[1:] for w in walks]
    assert {v for w in walks for v in w} == set(range(30)) - {17} and all(w[0] != 29 for w in walks)
    mapping = pp.IndexMap(list(range(30)))
    model = pp.MultiOrderModel.from_path_data(_paths(pp, full, weights, mapping=mapping), max_order=3)
    paths = _paths(pp, walks, weights, mapping=mapping)
    seen = []
    real = hip.mon_zeroth_llh

    def spy(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]

    monkeypatch.setattr(hip, "mon_zeroth_llh", spy)
    z_on = model.get_zeroth_order_log_likelihood(paths.data)
    llh0_on = model.get_mon_log_likelihood(paths.data, 0)
    order_on = model.estimate_order(paths, max_order=3)
    assert seen and all(s is None for s in seen), "a native zeroth-order value was used for ids with a gap"
    monkeypatch.setattr(mom, "NATIVE_SELECTION", False)
    count = len(seen)
    assert model.get_zeroth_order_log_likelihood(paths.data) == z_on
    llh0_off = model.get_mon_log_likelihood(paths.data, 0)
    assert llh0_off == llh0_on or (math.isnan(llh0_off) and math.isnan(llh0_on))
    assert model.estimate_order(paths, max_order=3) == order_on
    assert len(seen) == count


# ------------------------------------------------------------------ one pass
def _toy(pp, weights):
    paths = pp.PathData(pp.IndexMap(list("abcde")), device=DEV)
    for walk, weight in zip([("a", "c", "d"), ("b", "c", "e")], weights):
        paths.append_walk(walk, weight=weight)
    return paths


@pytest.mark.parametrize("case", ["weak", "strong", "random"])
def test_estimate_order_is_one_pass(pp, hip, case, monkeypatch):
    if case == "random":
        walks, weights, _ = oracle_layers("random")
        paths, top = _paths(pp, walks, weights, mapping=pp.IndexMap(list(range(30)))), 4
    else:
        paths, top = _toy(pp, [3, 3] if case == "weak" else [4, 4]), 2
    model = pp.MultiOrderModel.from_path_data(paths, max_order=top)
    assert "layers" in getattr(model, "sizes", {}), "not the level-by-level builder"
    calls = {"walk_counts": 0, "mon_zeroth_llh": 0, "mon_layer_llh": 0}
    for name in calls:
        def counted(*a, _name=name, _real=getattr(hip, name), **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(hip, name, counted)
    order = model.estimate_order(paths, max_order=top)
    assert calls["walk_counts"] <= 1 and calls["mon_zeroth_llh"] <= 1 and calls["mon_layer_llh"] <= top, calls
    assert calls["walk_counts"] == 1 and calls["mon_layer_llh"] == top, calls
    for k in range(2, top + 1):
        lazy = model.layers[k].data.peek("edge_index")
        assert not isinstance(lazy, torch.Tensor) and lazy.value is None, f"estimate_order resolved layer {k}'s edge_index"
    rejected = [k for k in range(2, top + 1) if model.likelihood_ratio_test(paths.data, max_order_null=k - 1, max_order=k)[0]]
    assert order == (rejected[-1] if rejected else 1)
    if case != "random":
        assert order == (1 if case == "weak" else 2)
