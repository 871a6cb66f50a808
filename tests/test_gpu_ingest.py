"""Native ingest of integer temporal edge lists (csrc/pp_ingest.hip + io/pandas.py): with a CUDA device,
read_csv_temporal_graph indexes and parses a qualifying `v<sep>w<sep>t` file on the GPU and must return the very graph the pandas path
(the same call with ``io.pandas.NATIVE_CSV = False``) returns; a file that does not qualify silently takes the pandas path."""
import numpy as np
import pandas as pd
import pytest
import torch

import pathpyg_amd as pp
from pathpyg_amd.io import pandas as ppio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")


def make_rows(m: int, seed: int = 0):
    """m events over about 300 ids drawn from [0, 10^17) (non-contiguous, wider than 32 bits; 0 and a 17-digit one always among them),
    timestamps that tie (a small range around 0, negative ones included) or have 18 digits of either sign, and exact duplicate rows."""
    rng = np.random.default_rng(seed)
    ids = np.unique(np.concatenate([rng.integers(0, 10 ** 17, 298), [0, 10 ** 17 - 1]]))
    v = ids[rng.integers(0, len(ids), m)]
    w = ids[rng.integers(0, len(ids), m)]
    t = rng.integers(-50, 50, m)
    wide = rng.random(m) < 0.05
    t[wide] = rng.integers(10 ** 17, 10 ** 18, int(wide.sum())) * rng.choice([-1, 1], int(wide.sum()))
    if m >= 4:                                                # exact duplicates of earlier rows, at a distance and side by side
        dup = rng.integers(m // 2, m, m // 20 + 1)
        src = rng.integers(0, m // 2, len(dup))
        v[dup], w[dup], t[dup] = v[src], w[src], t[src]
        v[1], w[1], t[1] = v[0], w[0], t[0]
    return v, w, t


def write_file(path, rows, sep=",", header=True, crlf=False, blanks=False, final_newline=True, zeros=False, seed=1):
    v, w, t = rows
    rng = np.random.default_rng(seed)
    eol = "\r\n" if crlf else "\n"
    lines = [f"v{sep}w{sep}t"] if header else []
    for i in range(len(v)):
        a, b, c = str(int(v[i])), str(int(w[i])), str(abs(int(t[i])))
        if zeros and i % 3 == 0:                              # leading zeros, up to the 18 digits a token may have
            a, b, c = a.zfill(18), b.zfill(int(rng.integers(len(b), 19))), c.zfill(int(rng.integers(len(c), 19)))
        lines.append(f"{a}{sep}{b}{sep}{'-' if t[i] < 0 else ''}{c}")
        if blanks and i % 97 == 5:
            lines.extend([""] * int(rng.integers(1, 4)))      # blank lines in the middle
    text = eol.join(lines)
    if blanks:
        text += eol * 3                                       # ... and at the end
    elif final_newline:
        text += eol
    path.write_bytes(text.encode())
    return path


def load_pandas(monkeypatch, path, **kw):
    with monkeypatch.context() as mp:
        mp.setattr(ppio, "NATIVE_CSV", False)
        return pp.io.read_csv_temporal_graph(str(path), device="cuda", **kw)


def load_native(monkeypatch, path, **kw):
    """The same call with pandas.read_csv out of reach: only the native path can answer."""
    def refuse(*args, **kwargs):
        raise AssertionError("pandas.read_csv was called: the native path did not run")

    with monkeypatch.context() as mp:
        mp.setattr(pd, "read_csv", refuse)
        return pp.io.read_csv_temporal_graph(str(path), device="cuda", **kw)


def assert_same_graph(got, want):
    for key in ("edge_index", "time"):
        a, b = got.data[key], want.data[key]
        assert a.dtype == b.dtype and a.device == b.device and a.is_cuda, key
        if a.dtype.is_floating_point:                         # (a pandas-path time column may hold NaN)
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True), key
        else:
            assert torch.equal(a, b), key
    assert got.data.num_nodes == want.data.num_nodes
    assert got.mapping.node_ids.dtype == want.mapping.node_ids.dtype
    assert np.array_equal(got.mapping.node_ids, want.mapping.node_ids)
    assert sorted(got.data.edge_attrs()) == sorted(want.data.edge_attrs())


def assert_native_equals_pandas(monkeypatch, path, **kw):
    got = load_native(monkeypatch, path, **kw)
    want = load_pandas(monkeypatch, path, **kw)
    assert_same_graph(got, want)
    assert got.data.edge_index.dtype == torch.int64 and got.data.time.dtype == torch.int64
    assert got.mapping.node_ids.dtype == np.int64 and bool((np.diff(got.mapping.node_ids) > 0).all())
    assert [k for k in got.data.edge_attrs() if k.startswith("edge_") and k != "edge_index"] == []
    return got, want


@pytest.fixture(scope="module")
def rows5000():
    return make_rows(5000)


def test_native_path_ran(tmp_path, monkeypatch, rows5000):
    g = load_native(monkeypatch, write_file(tmp_path / "g.csv", rows5000))
    v, w, t = rows5000
    assert g.data.edge_index.is_cuda and g.data.time.is_cuda
    assert g.n == len(np.unique(np.concatenate([v, w])))
    assert g.data.num_edges == len(set(zip(v.tolist(), w.tolist(), t.tolist())))
    assert g.data.time.cpu().tolist() == sorted(x[2] for x in set(zip(v.tolist(), w.tolist(), t.tolist())))


PARITY = {
    "defaults": dict(),
    "no-header,semicolon,multiedges": dict(file=dict(header=False, sep=";"), call=dict(header=False, sep=";", multiedges=True)),
    "tab,crlf,rescale7": dict(file=dict(sep="\t", crlf=True), call=dict(sep="\t", time_rescale=7)),
    "space,blank-lines": dict(file=dict(sep=" ", blanks=True), call=dict(sep=" ")),
    "no-final-newline,zeros,multiedges,rescale7": dict(file=dict(final_newline=False, zeros=True), call=dict(multiedges=True, time_rescale=7)),
    "crlf,blank-lines,no-header,num_nodes": dict(file=dict(crlf=True, blanks=True, header=False), call=dict(header=False, num_nodes=400)),
    "crlf,no-final-newline,multiedges": dict(file=dict(crlf=True, final_newline=False), call=dict(multiedges=True)),
    "zeros,rescale7,num_nodes": dict(file=dict(zeros=True), call=dict(time_rescale=7, num_nodes=300)),
}


@pytest.mark.parametrize("case", list(PARITY))
def test_parity_with_the_pandas_path(tmp_path, monkeypatch, rows5000, case):
    spec = PARITY[case]
    path = write_file(tmp_path / "g.csv", rows5000, **spec.get("file", {}))
    got, _ = assert_native_equals_pandas(monkeypatch, path, **spec.get("call", {}))
    v, w, t = rows5000
    t = t // spec.get("call", {}).get("time_rescale", 1)      # (floor division, before the duplicates are dropped)
    events = len(v) if spec.get("call", {}).get("multiedges") else len(set(zip(v.tolist(), w.tolist(), t.tolist())))
    assert got.data.num_edges == events
    assert got.data.time.cpu().tolist() == sorted(t.tolist() if spec.get("call", {}).get("multiedges") else
                                                  [x[2] for x in set(zip(v.tolist(), w.tolist(), t.tolist()))])
    assert got.data.num_nodes == spec.get("call", {}).get("num_nodes", len(np.unique(np.concatenate([v, w]))))


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_launch_boundaries(tmp_path, monkeypatch, m):
    path = write_file(tmp_path / "g.csv", make_rows(m, seed=m), final_newline=m != 1)
    assert path.read_bytes().endswith(b"\n") == (m != 1)
    got, _ = assert_native_equals_pandas(monkeypatch, path, multiedges=True)
    assert got.data.num_edges == m


@pytest.mark.parametrize("chunk_bytes", [48, 1000, 4096])
def test_chunk_seams(tmp_path, monkeypatch, rows5000, chunk_bytes):
    path = write_file(tmp_path / "g.csv", rows5000, crlf=True, blanks=True)
    one = load_native(monkeypatch, path)
    with monkeypatch.context() as mp:
        mp.setattr(ppio, "CHUNK_BYTES", chunk_bytes)
        assert len(ppio._cut_chunks(path.read_bytes(), ppio.CHUNK_BYTES, 7)) > 40
        cut = load_native(mp, path)
    assert_same_graph(cut, one)
    assert_same_graph(cut, load_pandas(monkeypatch, path))


FALLBACKS = {
    "string id": dict(text="v,w,t\na,b,1\nb,c,2\n"),
    "1.5 as time": dict(text="v,w,t\n1,2,1.5\n2,3,2.5\n"),
    "19-digit token": dict(text="v,w,t\n1,2,1234567890123456789\n2,3,4\n"),
    "+1": dict(text="v,w,t\n1,2,+1\n3,4,5\n"),
    "' 1'": dict(text="v,w,t\n1, 2,3\n3,4,5\n"),
    "quoted field": dict(text='v,w,t\n"1",2,3\n3,4,5\n'),
    "lone CR": dict(text="v,w,t\r1,2,3\r4,5,6\r"),
    "lone CR between data lines": dict(text="v,w,t\n1,2,3\r4,5,6\n7,8,9\n"),
    "2-field row": dict(text="v,w,t\n1,2,3\n4,5\n6,7,8\n"),
    "4-field row": dict(text="v,w,t\n1,2,3\n4,5,6,7\n"),
    "header a,b,c": dict(text="a,b,c\n1,2,3\n4,5,6\n"),
    "attribute column": dict(text="v,w,t,weight\n1,2,3,0.5\n2,3,4,1.5\n"),
    "negative node id": dict(text="v,w,t\n-1,2,3\n2,3,4\n"),
    "sep='::'": dict(text="v::w::t\n1::2::3\n2::3::4\n", call=dict(sep="::")),
    "empty file": dict(text=""),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks(tmp_path, monkeypatch, case):
    spec = FALLBACKS[case]
    path = tmp_path / "g.csv"
    path.write_bytes(spec["text"].encode())
    kw = spec.get("call", {})
    try:
        want, error = load_pandas(monkeypatch, path, **kw), None
    except Exception as exc:                                  # noqa: BLE001 - whatever pandas raises for this file
        want, error = None, exc
    calls = []
    real = pd.read_csv

    def counting(*args, **kwargs):
        calls.append(args)
        return real(*args, **kwargs)

    with monkeypatch.context() as mp:
        mp.setattr(pd, "read_csv", counting)
        assert ppio.NATIVE_CSV is True
        if error is not None:
            with pytest.raises(type(error)):
                pp.io.read_csv_temporal_graph(str(path), device="cuda", **kw)
        else:
            assert_same_graph(pp.io.read_csv_temporal_graph(str(path), device="cuda", **kw), want)
    assert len(calls) == 1, "a file that does not qualify is read by pandas.read_csv"


def test_downstream_multi_order_model(tmp_path, monkeypatch, rows5000):
    path = write_file(tmp_path / "g.csv", rows5000)
    native = pp.MultiOrderModel.from_temporal_graph(load_native(monkeypatch, path), delta=5, max_order=3)
    host = pp.MultiOrderModel.from_temporal_graph(load_pandas(monkeypatch, path), delta=5, max_order=3)
    for k in (1, 2, 3):
        a, b = native.layers[k].data, host.layers[k].data
        assert a.edge_index.numel() > 0
        assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_weight, b.edge_weight), f"layer {k}"
