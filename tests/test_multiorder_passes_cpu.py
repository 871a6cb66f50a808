"""The De Bruijn layers of a level-by-level build whose levels are taken in PASSES over ranges of types
(``core/multi_order_passes.continue_in_passes``): the PROTOCOL — the greedy cuts, the rebased part arrays, parts without children, the
concatenation of the pieces, the fallbacks, the 64-bit counts behind a wrapped int32 prefix — with the numpy stand-in of the device
contracts (``tests/cpu_ops_passes.py``), against the CPU oracle, bit for bit.  The kernels are checked on the GPU
(``tests/test_gpu_multiorder_passes.py``)."""
import functools

import numpy as np
import pytest
import torch

from tests.test_multiorder_sharded_cpu import K, KINDS, case, check_model, fallback_streams

I32 = 0x7ffffff0


def _ops():
    from tests.cpu_ops_passes import CpuOpsPasses
    return CpuOpsPasses()


def _prime_at_or_below(x):
    x = max(int(x), 2)
    while any(x % d == 0 for d in range(2, int(x ** 0.5) + 1)):
        x -= 1
    return x


@functools.lru_cache(maxsize=None)
def oracle_levels(kind):
    """Per level k = 1 .. K - 1 of the stream, from the unit-weight oracle: ``(children of every type, new types of every type)`` — the
    instances of order k + 1 whose first k nodes are the type (the merged unit weights of layer k + 1's rows) and that layer's row lengths."""
    _, _, want = case(kind, "unit")
    out = {}
    for k in range(1, K):
        nxt = want[k + 1]
        rows, types = nxt["edge_index"][0].numpy(), int(nxt["num_nodes"])
        assert types == want[k]["edge_index"].size(1)
        children = np.bincount(rows, weights=nxt["edge_weight"].double().numpy(), minlength=types).astype(np.int64)
        out[k] = (children, np.bincount(rows, minlength=types).astype(np.int64))
    return out


def budgets_of(kind):
    most = max(int(children.sum()) for children, _ in oracle_levels(kind).values())
    return [-(-most // 3), -(-most // 10), _prime_at_or_below(most // 10)] + ([1] if kind == "loops" else [])


def expected_cuts(kind, budget):
    """The parts of every level by the rule of the issue, worked out from the oracle alone: a part that starts at type t0 ends before the
    first type t with more than ``budget`` children in [t0, t], holds at least one type; the parts of the next level are the (non-empty)
    type ranges the parts' children fall into, cut again where they exceed the budget."""
    levels = oracle_levels(kind)
    parts = [(0, levels[1][0].size)]
    out = []
    for k in range(1, K):
        children, new_types = levels[k]
        split = []
        for a, b in parts:
            if int(children[a:b].sum()) <= budget:
                split.append((a, b))
                continue
            t0 = a
            while t0 < b:
                t, acc = t0, 0
                while t < b and acc + int(children[t]) <= budget:
                    acc += int(children[t])
                    t += 1
                t = max(t, t0 + 1)
                split.append((t0, t))
                t0 = t
        out.append((split, children))
        first = np.concatenate(([0], np.cumsum(new_types)))
        parts = [(int(first[a]), int(first[b])) for a, b in split if first[b] > first[a]]
    return out


def build(kind, mode, budget, max_order=K, graph=None):
    """The model of a test stream: level 1 over the whole node range, every further level in passes of ``budget`` instances."""
    from pathpyg_amd import _hip
    from pathpyg_amd.core import multi_order_model as mm
    from pathpyg_amd.core.multi_order_passes import continue_in_passes
    g, delta, _ = case(kind, mode) if graph is None else graph
    ops = _ops()
    ei, n = g.data.edge_index, int(g.data.num_nodes)
    w = g.data["edge_weight"] if "edge_weight" in g.data else None
    started = ops.multi_order_node_loads(ei, g.data.time, n, delta, w)
    assert started is not None
    windows, loads = started
    m = int(loads[0][n])
    level, tab = ops.multi_order_prepare_range(windows, 0, n, 0, m)
    assert level.status == 0
    layer1 = _hip.MultiOrderLayer(n_nodes=n, n_edges=level.types, n_instances=m, row_ptr=level.row_ptr, col=level.col[:level.types],
                                  weight=level.weight[:level.types], last=level.tlast[:level.types])
    built = continue_in_passes(ops, level, level.row_ptr, level.tlast, tab, [layer1], max_order, w is not None, budget)
    if built is None:
        return None
    layers, passes, cuts = built
    model = mm.MultiOrderModel()
    model.sizes = {"m": m, "N": n, "layers": [(b.n_nodes, b.n_edges, b.n_instances) for b in layers], "passes": [1] + passes}
    model.layers = mm._csr_layers(g, ei, layers, True, gather_concat=ops.gather_concat)
    return model, cuts


CASES = [(kind, mode, which) for kind in KINDS for mode in ("unit", "dyadic") for which in range(4 if kind == "loops" else 3)]


@pytest.mark.parametrize("kind,mode,which", CASES)
def test_passes_equal_the_oracle(kind, mode, which):
    budget = budgets_of(kind)[which]
    _, _, want = case(kind, mode)
    model, cuts = build(kind, mode, budget)
    check_model(model, want)
    passes = model.sizes["passes"]
    assert len(passes) == K and passes[0] == 1 and max(passes) > 1, passes
    # true instance counts: order k + 1 has as many instances as level k has children
    levels = oracle_levels(kind)
    assert [x[2] for x in model.sizes["layers"]][1:] == [int(levels[k][0].sum()) for k in range(1, K)]
    expected = expected_cuts(kind, budget)
    assert len(cuts) == K - 1
    for j, (split, children) in enumerate(expected):
        assert cuts[j] == [a for a, _ in split] + [children.size], (j, budget)
        assert passes[j + 1] == len(split)
        largest_type = int(children.max())
        for a, b in split:
            assert int(children[a:b].sum()) <= max(budget, largest_type), (j, a, b)
            assert b - a == 1 or int(children[a:b].sum()) <= budget, (j, a, b)


def test_a_budget_nobody_reaches_is_one_part_per_level():
    _, _, want = case("hubs", "unit")
    model, cuts = build("hubs", "unit", I32)
    check_model(model, want)
    assert model.sizes["passes"] == [1] * K and all(len(c) == 2 for c in cuts)


@pytest.mark.parametrize("budget", [1, 50, I32])
@pytest.mark.parametrize("which", ["many_children", "no_edges"])
def test_fallback_streams_are_handed_back(which, budget):
    g, delta, max_order = fallback_streams()[which]
    assert build(None, None, budget, max_order, graph=(g, delta, None)) is None


def _wrapped_level(counts):
    """A level of one-instance types whose int32 ``ibase`` is the low 32 bits of the int64 prefix of ``counts`` — pure arithmetic."""
    from pathpyg_amd._hip import MultiOrderLevel
    counts = np.asarray(counts, dtype=np.int64)
    prefix = np.concatenate(([0], np.cumsum(counts)))
    ibase = (prefix & 0xffffffff).astype(np.uint32).view(np.int32)
    t = counts.size
    inst = (np.arange(t), counts.copy(), np.ones(t, dtype=np.float32))
    ids = torch.arange(t, dtype=torch.int32)
    return MultiOrderLevel(types=t, children=int(prefix[-1]), status=0, tptr=np.arange(t + 1), ibase=ibase, inst=inst, row_ptr=None, col=ids,
                           weight=torch.ones(t), tlast=ids), prefix


WRAP_COUNTS = [(1 << 30) - 3, (1 << 30) + 5, 7, 1 << 30, (1 << 30) - 1, 0, (1 << 30) + 11]


@pytest.mark.parametrize("budget,cuts", [(I32 - 1, [0, 1, 3, 4, 6, 7]), (1 << 30, [0, 1, 2, 3, 4, 6, 7]), (3 << 30, [0, 3, 7])])
def test_split_recovers_the_counts_behind_a_wrapped_prefix(budget, cuts):
    from tests.cpu_ops_passes import counts_from_ibase
    level, prefix = _wrapped_level(WRAP_COUNTS)
    assert level.children > 1 << 32 and (level.ibase[1:] < level.ibase[:-1]).any(), "the prefix was meant to wrap"
    assert counts_from_ibase(level.ibase).tolist() == WRAP_COUNTS
    if budget > I32 - 1:
        # a part of 2^31 or more children is no input of a step: the stand-in refuses it as the device wrapper does
        assert _ops().multi_order_split(level, budget) is None
        return
    parts = _ops().multi_order_split(level, budget)
    assert [0] + list(np.cumsum([p.types for p in parts])) == cuts
    for p, (a, b) in zip(parts, zip(cuts, cuts[1:])):
        assert p.children == int(prefix[b] - prefix[a]) == sum(WRAP_COUNTS[a:b])
        assert p.children <= budget or b - a == 1
        assert np.asarray(p.ibase).tolist() == (prefix[a: b + 1] - prefix[a]).tolist()
        assert np.asarray(p.tptr).tolist() == list(range(b - a + 1))
        assert p.col.tolist() == list(range(a, b)) and p.inst[1].tolist() == WRAP_COUNTS[a:b]


def test_greedy_cuts_rule():
    from pathpyg_amd.core.multi_order_passes import greedy_cuts
    assert greedy_cuts([0], 5) == [0]
    assert greedy_cuts([0, 0, 0, 0], 1) == [0, 3]
    assert greedy_cuts([0, 9], 5) == [0, 1]
    assert greedy_cuts([0, 2, 4, 6, 8], 4) == [0, 2, 4]
    assert greedy_cuts([0, 2, 4, 6, 8], 5) == [0, 2, 4]
    assert greedy_cuts([0, 2, 9, 9, 10, 12], 3) == [0, 1, 2, 5]
