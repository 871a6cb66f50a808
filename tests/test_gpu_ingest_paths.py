"""Native ingest of integer n-gram path files (csrc/pp_ingest.hip, the pp_ingest_tokens_* half, + io/pandas.py): with a
CUDA device, read_csv_path_data indexes and parses the TOKENS of a qualifying file on the GPU and must return the very walk store the
host code (the same call with ``io.pandas.NATIVE_CSV = False``: csv.reader, ast.literal_eval, PathData.append_walks) returns, bit for
bit; a file that does not qualify silently takes the host code."""
import types

import numpy as np
import pytest
import torch

import pathpyg_amd as pp
from pathpyg_amd.io import pandas as ppio

pytestmark = pytest.mark.gpu

TILE = 4096                                                   # bytes per workgroup of the token index; a lane takes 16
WALK_KEYS = ("edge_index", "node_sequence", "dag_weight", "dag_num_edges", "dag_num_nodes")
WALK_DTYPES = (torch.int64, torch.int64, torch.float32, torch.int64, torch.int64)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")


def id_pool(seed: int = 0) -> list:
    """About 300 distinct ids of 1 to 18 digits, 0 and a 17-digit one always among them."""
    rng = np.random.default_rng(seed)
    ids = {0, 10 ** 17 - 1, 10 ** 16, 7, 10, 100, 999999999999999999}
    while len(ids) < 300:
        d = int(rng.integers(1, 19))
        ids.add(int(rng.integers(10 ** (d - 1), 10 ** d)))
    return sorted(ids)


def weight_token(rng) -> str:
    """Integers, d.ddd decimals of up to 15 digits in total, and the fixed 0, 0.5, 2.0."""
    kind = int(rng.integers(0, 6))
    if kind == 0:
        return ["0", "0.5", "2.0", "1", "0." + "0" * 13 + "1", "999999999999999"][int(rng.integers(0, 6))]
    if kind <= 2:
        return str(int(rng.integers(0, 10 ** int(rng.integers(1, 16)))))
    total = int(rng.integers(2, 16))
    whole = int(rng.integers(1, total))
    head = str(int(rng.integers(10 ** (whole - 1), 10 ** whole))) if whole > 1 else str(int(rng.integers(0, 10)))
    return head + "." + "".join(str(int(x)) for x in rng.integers(0, 10, total - whole))


def make_walks(count: int = 400, longest: int = 40, seed: int = 0):
    rng = np.random.default_rng(seed)
    pool = id_pool(seed)
    walks = [[pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(1, longest + 1)))] for _ in range(count)]
    return walks, [weight_token(rng) for _ in range(count)]


def ngram_text(walks, weights, sep=",", weight=True, crlf=False, blanks=False, final_newline=True, seed=1) -> bytes:
    rng = np.random.default_rng(seed)
    eol = "\r\n" if crlf else "\n"
    lines = []
    for i, walk in enumerate(walks):
        fields = [str(v) for v in walk] + ([weights[i]] if weight else [])
        lines.append(sep.join(fields))
        if blanks and i % 37 == 5:
            lines.extend([""] * int(rng.integers(1, 4)))      # blank lines in the middle
    text = eol.join(lines)
    if blanks:
        text += eol * 3                                       # ... and at the end
    elif final_newline:
        text += eol
    return text.encode()


def load_host(monkeypatch, path, **kw):
    with monkeypatch.context() as mp:
        mp.setattr(ppio, "NATIVE_CSV", False)
        return pp.io.read_csv_path_data(str(path), device="cuda", **kw)


def load_native(monkeypatch, path, **kw):
    """The same call with csv.reader and ast.literal_eval out of io.pandas' reach: only the native path can answer."""
    def refuse(*args, **kwargs):
        raise AssertionError("the host code of read_csv_path_data was reached: the native path did not run")

    with monkeypatch.context() as mp:
        mp.setattr(ppio, "csv", types.SimpleNamespace(reader=refuse))
        mp.setattr(ppio, "ast", types.SimpleNamespace(literal_eval=refuse))
        return pp.io.read_csv_path_data(str(path), device="cuda", **kw)


def assert_same_paths(got, want, stock_dtypes=True):
    """Equal walk stores, bit for bit.  ``stock_dtypes``: the tensors also have the dtypes the native builders demand (what the host code makes
    of a file that does not qualify may not: a line without a node turns its node indices into floats)."""
    assert got.mapping.node_ids.dtype == want.mapping.node_ids.dtype, (got.mapping.node_ids.dtype, want.mapping.node_ids.dtype)
    assert np.array_equal(got.mapping.node_ids, want.mapping.node_ids)
    for key, dtype in zip(WALK_KEYS, WALK_DTYPES):
        a, b = got.data[key], want.data[key]
        assert a.dtype == b.dtype and a.device == b.device and a.is_cuda, key
        assert a.dtype == dtype or not stock_dtypes, key
        assert a.shape == b.shape and torch.equal(a, b), key
    assert got.data.num_nodes == want.data.num_nodes and got.num_paths == want.num_paths


def assert_native_equals_host(monkeypatch, path, **kw):
    got = load_native(monkeypatch, path, **kw)
    want = load_host(monkeypatch, path, **kw)
    assert_same_paths(got, want)
    p, w = got.data.node_sequence.size(0), got.num_paths
    assert tuple(got.data.edge_index.shape) == (2, p - w) and tuple(got.data.node_sequence.shape) == (p, 1)
    assert got.mapping.node_ids.dtype.kind == "U"
    return got, want


@pytest.fixture(scope="module")
def walks400():
    return make_walks()


PARITY = {
    "defaults": dict(),
    "semicolon": dict(file=dict(sep=";"), call=dict(sep=";")),
    "tab,crlf": dict(file=dict(sep="\t", crlf=True), call=dict(sep="\t")),
    "space,blank-lines": dict(file=dict(sep=" ", blanks=True), call=dict(sep=" ")),
    "no-final-newline": dict(file=dict(final_newline=False)),
    "crlf,blank-lines": dict(file=dict(crlf=True, blanks=True)),
    "crlf,no-final-newline,semicolon": dict(file=dict(crlf=True, final_newline=False, sep=";"), call=dict(sep=";")),
    "no-weight": dict(file=dict(weight=False), call=dict(weight=False)),
    "no-weight,tab,crlf,blank-lines": dict(file=dict(weight=False, sep="\t", crlf=True, blanks=True), call=dict(weight=False, sep="\t")),
    "no-weight,space,no-final-newline": dict(file=dict(weight=False, sep=" ", final_newline=False), call=dict(weight=False, sep=" ")),
}


@pytest.mark.parametrize("case", list(PARITY))
def test_parity_with_the_host_code(tmp_path, monkeypatch, walks400, case):
    spec = PARITY[case]
    walks, weights = walks400
    path = tmp_path / "p.ngram"
    path.write_bytes(ngram_text(walks, weights, **spec.get("file", {})))
    got, _ = assert_native_equals_host(monkeypatch, path, **spec.get("call", {}))
    assert got.num_paths == len(walks)
    assert got.data.dag_num_nodes.cpu().tolist() == [len(w) for w in walks]
    assert got.data.node_sequence.size(0) == sum(len(w) for w in walks)
    distinct = sorted({str(v) for w in walks for v in w})
    assert got.mapping.node_ids.tolist() == distinct and got.mapping.node_ids.dtype == np.dtype("<U18")
    assert [got.get_walk(i) for i in (0, 1, len(walks) - 1)] == [tuple(str(v) for v in walks[i]) for i in (0, 1, len(walks) - 1)]
    if spec.get("call", {}).get("weight", True):
        assert got.data.dag_weight.cpu().tolist() == torch.tensor([float(w) for w in weights], dtype=torch.float64).float().tolist()
    else:
        assert got.data.dag_weight.cpu().tolist() == [1.0] * len(walks)


def filler(nbytes: int) -> str:
    """Exactly ``nbytes`` bytes of whole 2-node walks (8 bytes each, the last one 8 to 15)."""
    assert nbytes >= 8
    full = nbytes // 8 - 1
    rest = nbytes - 8 * full
    return "10,20,1\n" * full + "3" * (rest - 5) + ",4,1\n"


def border_texts() -> dict:
    out = {}
    text = filler(TILE - 2) + "5,66,3\n7,8,2\n"
    assert text[TILE - 1] == "," and text[TILE:TILE + 2] == "66"
    out["separator ends tile 0, a token starts tile 1"] = text
    text = filler(TILE) + "77,8,2\n9,7,1\n"
    assert text[TILE - 1] == "\n" and text[TILE:TILE + 2] == "77"
    out["line start at byte 4096"] = text
    text = filler(TILE - 2) + "123456,9,1\n9,123456,1\n"
    assert text[TILE - 2:TILE + 4] == "123456"
    out["token straddling bytes 4095/4096"] = text
    text = filler(TILE - 4) + "12,5\r\n\r\n6,7,1\r\n"
    assert text[TILE - 1] == "5" and text[TILE:TILE + 2] == "\r\n"
    out["CR LF at bytes 4096/4097"] = text
    text = filler(TILE - 1) + "\n\n8,9,4\n"
    assert text[TILE - 1] == "\n" and text[TILE] == "\n"
    out["blank lines across the tile border"] = text
    text = filler(16 - 2) + "5,66,3\n"
    assert text[15] == "," and text[16] == "6"
    out["separator ends lane 0, a token starts lane 1"] = text
    out["shorter than 16 bytes"] = "1,2,3\n"
    out["one line, no newline"] = "12,34,5"
    out["one byte and its weight, no newline"] = "7,1"
    out["two bytes, no weight"] = dict(text="4\n", call=dict(weight=False))
    out["one byte, no weight"] = dict(text="4", call=dict(weight=False))
    return out


BORDERS = border_texts()


@pytest.mark.parametrize("case", list(BORDERS))
def test_constructed_borders(tmp_path, monkeypatch, case):
    spec = BORDERS[case] if isinstance(BORDERS[case], dict) else dict(text=BORDERS[case])
    path = tmp_path / "p.ngram"
    path.write_bytes(spec["text"].encode())
    got, _ = assert_native_equals_host(monkeypatch, path, **spec.get("call", {}))
    assert got.num_paths == sum(1 for line in spec["text"].splitlines() if line)


def test_one_long_walk_among_short_ones(tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    pool = [0, 3, 12, 45, 678, 9012, 5]
    long_walk = [pool[int(i)] for i in rng.integers(0, len(pool), 3000)]
    walks = [[5], [3, 12], long_walk, [5], [45, 0, 3], long_walk[:700], [678]]
    weights = ["3", "1", "2.5", "0.25", "7", "1", "12"]
    text = ngram_text(walks, weights)
    assert text.startswith(b"5,3\n") and len(text) > 2 * TILE + 1000
    path = tmp_path / "p.ngram"
    path.write_bytes(text)
    got, _ = assert_native_equals_host(monkeypatch, path)
    assert got.data.dag_num_nodes.cpu().tolist() == [1, 2, 3000, 1, 3, 700, 1]
    assert got.data.dag_num_edges.cpu().tolist() == [0, 1, 2999, 0, 2, 699, 0]
    assert got.get_walk(0) == ("5",) and got.data.dag_weight.cpu().tolist() == [3.0, 1.0, 2.5, 0.25, 7.0, 1.0, 12.0]
    assert got.get_walk(2) == tuple(str(v) for v in long_walk)


@pytest.mark.parametrize("chunk_bytes", [64, 4096])
def test_chunk_seams(tmp_path, monkeypatch, walks400, chunk_bytes):
    walks, weights = walks400
    path = tmp_path / "p.ngram"
    path.write_bytes(ngram_text(walks, weights, crlf=True, blanks=True))
    one = load_native(monkeypatch, path)
    with monkeypatch.context() as mp:
        mp.setattr(ppio, "CHUNK_BYTES", chunk_bytes)
        assert len(ppio._cut_chunks(path.read_bytes(), ppio.CHUNK_BYTES)) > (100 if chunk_bytes == 64 else 15)
        cut = load_native(mp, path)
    assert_same_paths(cut, one)
    assert_same_paths(cut, load_host(monkeypatch, path))


FALLBACKS = {
    "string ids": dict(text="a,b,1\nb,c,2\n"),
    "007": dict(text="007,7,1\n7,8,2\n"),
    "a space after a separator": dict(text="1, 2,1\n2,3,1\n"),
    "a quoted field": dict(text='"1",2,3\n3,4,5\n'),
    "a trailing separator": dict(text="1,2,3,\n4,5,6,\n"),
    "a trailing separator, no weight": dict(text="1,2,3,\n4,5,6,\n", call=dict(weight=False)),
    "a trailing separator ends the file": dict(text="1,2,3\n4,5,6,"),
    "an empty field": dict(text="1,,2,1\n3,4,1\n"),
    "a 19-digit id": dict(text="1,1234567890123456789,1\n2,3,4\n"),
    "a 16-digit weight": dict(text="1,2,1234567890.123456\n2,3,4\n"),
    "weight 1e3": dict(text="1,2,1e3\n2,3,4\n"),
    "weight -2": dict(text="1,2,-2\n2,3,4\n"),
    "weight .5": dict(text="1,2,.5\n2,3,4\n"),
    "weight 5.": dict(text="1,2,5.\n2,3,4\n"),
    "weight 00.5": dict(text="1,2,00.5\n2,3,4\n"),
    "a decimal point in a node": dict(text="1,2.5,3\n2,3,4\n"),
    "a lone CR": dict(text="1,2,1\r3,4,1\n5,6,1\n"),
    "lone CRs only": dict(text="1,2,1\r3,4,1\r"),
    "a weight-only line": dict(text="1,2,1\n5\n3,4,1\n"),
    "sep='::'": dict(text="1::2::3\n", call=dict(sep="::")),
    "no data line": dict(text="\n\r\n\n"),
    "empty file": dict(text=""),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks(tmp_path, monkeypatch, case):
    spec = FALLBACKS[case]
    path = tmp_path / "p.ngram"
    path.write_bytes(spec["text"].encode())
    kw = spec.get("call", {})
    try:
        want, error = load_host(monkeypatch, path, **kw), None
    except Exception as exc:                                  # noqa: BLE001 - whatever the host code raises for this file
        want, error = None, exc
    answers = []
    real = ppio._read_csv_paths_native

    def spying(*args, **kwargs):
        answers.append(real(*args, **kwargs))
        return answers[-1]

    with monkeypatch.context() as mp:
        mp.setattr(ppio, "_read_csv_paths_native", spying)
        assert ppio.NATIVE_CSV is True
        if error is not None:
            with pytest.raises(type(error)):
                pp.io.read_csv_path_data(str(path), device="cuda", **kw)
        else:
            assert_same_paths(pp.io.read_csv_path_data(str(path), device="cuda", **kw), want, stock_dtypes=False)
    assert answers == [None], "the native reader is asked once and declines: the host code reads this file"


def test_walk_indices_follow_string_order(tmp_path, monkeypatch):
    path = tmp_path / "p.ngram"
    path.write_bytes(b"2,10,1\n100,7,2,1\n")
    got, _ = assert_native_equals_host(monkeypatch, path)
    assert got.mapping.node_ids.tolist() == ["10", "100", "2", "7"] and got.mapping.node_ids.dtype == np.dtype("<U3")
    assert got.data.node_sequence.view(-1).cpu().tolist() == [2, 0, 1, 3, 2]
    assert got.data.edge_index.cpu().tolist() == [[0, 2, 3], [1, 3, 4]]


def test_downstream_multi_order_model(tmp_path, monkeypatch):
    rng = np.random.default_rng(11)
    pool = [0, 2, 10, 100, 7, 31, 10 ** 17 - 1, 4, 55, 6]
    walks = [[pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(1, 9)))] for _ in range(500)]
    weights = [str(int(rng.integers(1, 6))) for _ in walks]
    path = tmp_path / "p.ngram"
    path.write_bytes(ngram_text(walks, weights))
    native_paths, host_paths = load_native(monkeypatch, path), load_host(monkeypatch, path)
    native = pp.MultiOrderModel.from_path_data(native_paths, max_order=3)
    host = pp.MultiOrderModel.from_path_data(host_paths, max_order=3)
    assert "layers" in getattr(native, "sizes", {}) and "layers" in getattr(host, "sizes", {}), "the level-by-level builder was not taken"
    assert native.sizes == host.sizes
    for k in (1, 2, 3):
        a, b = native.layers[k].data, host.layers[k].data
        assert a.edge_index.numel() > 0
        for key in ("edge_index", "edge_weight", "node_sequence"):
            assert torch.equal(a[key], b[key]), (k, key)
    assert native.estimate_order(native_paths) == host.estimate_order(host_paths)
