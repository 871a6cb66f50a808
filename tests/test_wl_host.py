"""Host-side checks for the Weisfeiler-Leman test: the restatement (tests/cpu_ops_wl.py) against the fixtures made from the reference's own
function (tests/golden/wl_vectors.npz) and against the reference-free properties of its numbering and stop rule, what the public function
decides before any device is touched, and the host loop that keeps the features the device does not take.  All comparisons are exact."""
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_wl as ops

GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "wl_vectors.npz", allow_pickle=False)
NAMES = [str(x) for x in GOLDEN["names"]]


def same_triple(got, expect):
    """Equal values AND equal element types ('1' is not 1)."""
    assert got[0] is expect[0] or got[0] == expect[0] and type(got[0]) is bool
    for a, b in zip(got[1:], expect[1:]):
        assert a == b and [type(x) for x in a] == [type(x) for x in b]


def restated(case):
    return ops.wl_test(case["ids1"], ops.successor_lists(case["edge_index1"], len(case["ids1"])), case["ids2"],
                       ops.successor_lists(case["edge_index2"], len(case["ids2"])), case["features1"], case["features2"])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_fixture(name):
    case = ops.fixture_case(GOLDEN, name)
    same_triple(restated(case), (case["result"], case["fp1"], case["fp2"]))


def test_fixtures_cover_the_pinned_cases():
    cases = {name: ops.fixture_case(GOLDEN, name) for name in NAMES}
    assert cases["triangles_hexagon"]["result"] and set(cases["triangles_hexagon"]["fp1"]) == {"0"}      # regular: the initial fingerprint
    assert cases["string_features_stable"]["fp1"] == ["p", "q"]                                          # the feature values themselves
    assert len(cases["unequal_sizes"]["fp1"]) != len(cases["unequal_sizes"]["fp2"])
    assert isinstance(cases["tuple_ids"]["ids1"][0], tuple)
    assert all(type(x) is int for x in cases["integer_features"]["fp1"])
    both = sorted(cases["interleaved_ids"]["ids1"] + cases["interleaved_ids"]["ids2"])
    assert [v in cases["interleaved_ids"]["ids1"] for v in both] == [False, True] * 4
    assert {cases[n]["result"] for n in NAMES} == {True, False}


def test_label_reuse_changes_the_reference_result():
    """Point 7: with '1' on a sink the dict hands a round-1 number out again; a numbering without reuse (the rule of points 4 and 5) differs."""
    case = ops.fixture_case(GOLDEN, "feature_one_on_sink")
    n1 = len(case["ids1"])
    succ = ops.successor_lists(case["edge_index1"], n1) + [[w + n1 for w in s] for s in ops.successor_lists(case["edge_index2"], len(case["ids2"]))]
    merged = {**case["features1"], **case["features2"]}
    values = sorted(set(merged.values()))
    colours, counts = ops.refine(succ, [values.index(merged[v]) for v in case["ids1"] + case["ids2"]], ops.union_order(case["ids1"], case["ids2"]))
    rounds = len(counts) - 1
    assert rounds > 1
    without_reuse = [1 + sum(counts[1:rounds - 1]) + c for c in colours]
    assert without_reuse != case["fp1"] + case["fp2"]


def test_numbering_and_stop_rule_on_random_pairs():
    """Points 4 and 5 without the reference: the triple is the stable partition of colour refinement on the union, numbered by first occurrence
    in the sorted ID order, offset by 1 + k_1 + ... + k_(R-2); the initial fingerprint when the first round adds no class."""
    seen = set()
    for ids1, ei1, ids2, ei2, f1, f2 in ops.random_pairs(11, 300):
        n1, n2 = len(ids1), len(ids2)
        s1, s2 = ops.successor_lists(ei1, n1), ops.successor_lists(ei2, n2)
        result, fp1, fp2 = ops.wl_test(ids1, s1, ids2, s2, f1, f2)
        succ = s1 + [[w + n1 for w in s] for s in s2]
        initial = None
        if f1 is not None:
            merged = {**f1, **f2}
            values = sorted(set(merged.values()))
            initial = [values.index(merged[v]) for v in ids1 + ids2]
        colours, counts = ops.refine(succ, initial, ops.union_order(ids1, ids2))
        rounds = len(counts) - 1
        assert counts[-1] == counts[-2] and all(a < b for a, b in zip(counts[:-2], counts[1:-1]))
        if rounds == 1:
            expect = [merged[v] for v in ids1 + ids2] if f1 is not None else ["0"] * (n1 + n2)
        else:
            expect = [1 + sum(counts[1:rounds - 1]) + c for c in colours]
            assert ops.refine(succ, initial, ops.union_order(ids1, ids2), max_rounds=rounds - 1)[0] == colours
        assert fp1 + fp2 == expect and result == (sorted(fp1) == sorted(fp2))
        seen.add((result, rounds == 1, f1 is not None))
    assert {(True, False, False), (False, False, False), (True, False, True), (False, False, True)} <= seen


def test_names_are_exported():
    import pathpyg_amd as pp
    from pathpyg_amd.algorithms import WeisfeilerLeman_test, color_refinement, weisfeiler_leman
    assert weisfeiler_leman.WeisfeilerLeman_test is WeisfeilerLeman_test is pp.algorithms.WeisfeilerLeman_test
    assert weisfeiler_leman.color_refinement is color_refinement is pp.algorithms.color_refinement
    assert weisfeiler_leman.NATIVE is True and weisfeiler_leman.HASH_MASK == 2 ** 64 - 1


class _NoDeviceGraph:
    """Stands where a Graph would: it has a size and a mapping; any other access (the edge list, the CSR) is an error."""

    def __init__(self, ids):
        from pathpyg_amd import IndexMap
        self.mapping = None if ids is None else IndexMap(ids)
        self.n = 0 if ids is None else len(ids)

    def __getattr__(self, name):
        raise AssertionError(f"the graph's {name} was read before the IDs were checked")


def test_refusals_come_before_the_device():
    from pathpyg_amd import IndexMap
    from pathpyg_amd.algorithms import WeisfeilerLeman_test
    for g1, g2 in ((_NoDeviceGraph(None), _NoDeviceGraph(["a"])), (_NoDeviceGraph(["a"]), _NoDeviceGraph(None))):
        with pytest.raises(Exception, match="^Graphs must contain IndexMap that assigns node IDs$") as info:
            WeisfeilerLeman_test(g1, g2)
        assert type(info.value) is Exception
    unmapped = _NoDeviceGraph(["a"])
    unmapped.mapping = IndexMap()
    with pytest.raises(Exception, match="^Graphs must contain IndexMap that assigns node IDs$"):
        WeisfeilerLeman_test(unmapped, _NoDeviceGraph(["b"]))
    for ids1, ids2 in ((["a", "b", "c"], ["x", "b"]), ([("a", "b"), ("b", "c")], [("b", "c")]), (["a"], ["a"])):
        with pytest.raises(Exception, match="^node identifiers of graphs must not overlap$") as info:
            WeisfeilerLeman_test(_NoDeviceGraph(ids1), _NoDeviceGraph(ids2), {"a": "x"}, {"b": "y"})
        assert type(info.value) is Exception


def test_which_features_the_device_takes():
    from pathpyg_amd.algorithms.weisfeiler_leman import _device_features
    nodes = ["a", "b", "c"]
    assert _device_features({"a": "red", "b": "blue", "c": "red"}, nodes)
    assert _device_features({"a": "0", "b": "01", "c": "-1"}, nodes)                    # not the decimal form of a positive integer
    assert _device_features({"a": "1x", "b": "x1", "c": " 1"}, nodes)
    assert _device_features({"a": "", "b": "1.0", "c": "١"}, nodes)                # (str(int) is ASCII)
    assert _device_features({("a", "b"): "x"}, [("a", "b")])
    assert not _device_features({"a": "1", "b": "blue", "c": "red"}, nodes)             # "1[]" is a later round's label
    assert not _device_features({"a": "red", "b": "45149", "c": "red"}, nodes)
    assert not _device_features({"a": 1, "b": 2, "c": 1}, nodes)                        # integers
    assert not _device_features({"a": "red", "b": 2, "c": "red"}, nodes)                # mixed types
    assert not _device_features({"a": "red", "b": None, "c": "red"}, nodes)
    assert not _device_features({"a": "red", "b": "blue"}, nodes)                       # a node is missing: the host loop's KeyError
    assert not _device_features({"a": "red", "b": "blue", "c": "red", "d": "green"}, nodes)      # an extra value counts in the stop rule
    assert not _device_features({"a": "red", "b": "blue", "d": "red"}, nodes)


def cpu_graph(ids, edge_index):
    """A CPU-resident Graph from a row-sorted edge list, built without any device."""
    import pathpyg_amd as pp
    from pathpyg_amd.data import Data
    return pp.Graph._from_parts(Data(edge_index=torch.from_numpy(np.ascontiguousarray(edge_index)), num_nodes=len(ids),
                                     node_sequence=torch.arange(len(ids)).reshape(-1, 1)), pp.IndexMap(ids))


@pytest.fixture
def host_loop(monkeypatch):
    from pathpyg_amd import _dispatch
    from pathpyg_amd.algorithms import weisfeiler_leman
    monkeypatch.setattr(weisfeiler_leman, "NATIVE", False)

    def no_device(*a, **k):
        raise AssertionError("the host loop reached for the device")

    monkeypatch.setattr(_dispatch, "graph_pair_color_refinement", no_device)
    return weisfeiler_leman.WeisfeilerLeman_test


@pytest.mark.parametrize("name", NAMES)
def test_host_loop_matches_fixture(host_loop, name):
    case = ops.fixture_case(GOLDEN, name)
    got = host_loop(cpu_graph(case["ids1"], case["edge_index1"]), cpu_graph(case["ids2"], case["edge_index2"]), case["features1"], case["features2"])
    same_triple(got, (case["result"], case["fp1"], case["fp2"]))


@pytest.mark.parametrize("name", ["integer_features", "integer_features_reuse", "feature_one_on_sink", "feature_one_everywhere"])
def test_ineligible_features_take_the_host_loop(monkeypatch, name):
    """NATIVE stays True: the feature rule alone sends these to the host loop, and no device is touched."""
    from pathpyg_amd import _dispatch
    from pathpyg_amd.algorithms import WeisfeilerLeman_test
    monkeypatch.setattr(_dispatch, "graph_pair_color_refinement", lambda *a, **k: pytest.fail("the device was asked"))
    case = ops.fixture_case(GOLDEN, name)
    got = WeisfeilerLeman_test(cpu_graph(case["ids1"], case["edge_index1"]), cpu_graph(case["ids2"], case["edge_index2"]), case["features1"],
                               case["features2"])
    same_triple(got, (case["result"], case["fp1"], case["fp2"]))


def test_host_loop_raises_what_the_reference_raises(host_loop):
    case = ops.fixture_case(GOLDEN, "string_features")
    g1, g2 = cpu_graph(case["ids1"], case["edge_index1"]), cpu_graph(case["ids2"], case["edge_index2"])
    missing = dict(case["features2"])
    del missing["z"]
    with pytest.raises(KeyError):
        host_loop(g1, g2, case["features1"], missing)
    mixed = dict(case["features1"], b=1, c="x", d=2)                                    # a's successor list is fine; b's holds 'x' ... sorted with ints
    g3 = cpu_graph(case["ids1"], np.array([[0, 0, 1], [2, 3, 2]], dtype=np.int64))
    with pytest.raises(TypeError):
        host_loop(g3, g2, mixed, case["features2"])
