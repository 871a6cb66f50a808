"""Ingest of time-stamped edge lists and n-gram path files, reference ``pathpyG.io.pandas``:
``df_to_temporal_graph`` (:318-397), ``temporal_graph_to_df`` (:431-470), ``read_csv_temporal_graph`` (:511-546),
``write_csv`` (:548-570), ``read_csv_path_data`` (:572-599), and their static-graph counterparts ``df_to_graph`` (:109-181),
``add_node_attributes`` (:183-235), ``add_edge_attributes`` (:237-316), ``graph_to_df`` (:399-429), ``read_csv_graph`` (:472-509).

Same column conventions as the reference (``v``, ``w``, ``t`` + edge attributes; header-less frames take the first three
columns).  Node IDs are mapped to indices with ONE vectorised ``np.unique(..., return_inverse=True)`` instead of a Python
dictionary lookup per endpoint, and the event sort happens on the GPU inside :class:`TemporalGraph`.
"""
from __future__ import annotations

import ast
import csv
import logging
import os
from typing import Any, Optional

import numpy as np
import pandas as pd
import torch

from .. import _hip
from ..core.graph import Graph
from ..core.index_map import IndexMap
from ..core.path_data import PathData
from ..core.temporal_graph import TemporalGraph
from ..data import Data

_log = logging.getLogger(__name__)


def _parse_timestamps(df: pd.DataFrame, timestamp_format: str, time_rescale: int) -> pd.Series:
    t = df["t"]
    if pd.api.types.is_string_dtype(t) or pd.api.types.is_datetime64_any_dtype(t):
        if not pd.api.types.is_datetime64_any_dtype(t):
            t = pd.to_datetime(t, format=timestamp_format)
        t = t.astype("int64") // time_rescale
        return t - t.min()                                   # seconds (or ns / rescale) since the first event
    if t.dtype == "int64" or t.dtype == "float64":
        return t // time_rescale
    raise ValueError(f"Column `t` must be of type `object`, `int64`, `float64`, or a datetime type. Found {t.dtype} instead.")


def _column_to_attribute(values: np.ndarray, device):
    """Numeric columns -> tensors, strings holding numbers / literals -> tensors, other strings -> NumPy string arrays."""
    if values.dtype.kind in "iufb":
        return torch.tensor(values, device=device)
    first = values[0]
    if isinstance(first, str):
        try:
            parsed = [ast.literal_eval(x) for x in values]
            return torch.tensor(parsed, device=device)
        except (ValueError, SyntaxError, TypeError):
            return np.asarray(values).astype(str)
    if isinstance(first, (list, tuple, np.ndarray)):
        return torch.tensor(np.asarray([np.asarray(x) for x in values]), device=device)
    raise ValueError(f"Unsupported data type for attribute column: {type(first)}")


def df_to_temporal_graph(df: pd.DataFrame, multiedges: bool = False, timestamp_format="%Y-%m-%d %H:%M:%S", time_rescale=1,
                         num_nodes: int | None = None, device: Optional[torch.device] = None) -> TemporalGraph:
    """Temporal graph from a DataFrame with columns ``v``, ``w``, ``t`` (+ edge attributes); one row = one event."""
    df = df.copy()
    if all(isinstance(c, (int, np.integer)) for c in df.columns.values.tolist()):
        df.columns = ["v", "w", "t"] + [f"edge_attr_{i - 2}" for i in range(3, len(df.columns))]
    df["t"] = _parse_timestamps(df, timestamp_format, time_rescale)
    if not multiedges:
        df = df.drop_duplicates(subset=["v", "w", "t"])
    endpoints = df[["v", "w"]].values
    ids, inverse = np.unique(endpoints, return_inverse=True)
    mapping = IndexMap(ids)
    edge_index = torch.from_numpy(inverse.reshape(endpoints.shape).T.astype(np.int64)).contiguous()
    data = Data(edge_index=edge_index if device is None else edge_index.to(device),
                time=torch.tensor(df["t"].values, device=device),
                num_nodes=num_nodes if num_nodes is not None else len(ids))
    for col in df.columns:
        if col not in ("v", "w", "t"):
            data[col if col.startswith("edge_") else "edge_" + col] = _column_to_attribute(df[col].values, device)
    return TemporalGraph(data=data, mapping=mapping)


def df_to_graph(df: pd.DataFrame, is_undirected: bool = False, multiedges: bool = False, num_nodes: int | None = None,
                device: Optional[torch.device] = None) -> Graph:
    """Graph from a DataFrame with columns ``v``, ``w`` (+ edge attributes; header-less frames: the first two columns); duplicate
    (v, w) rows are dropped unless ``multiedges``; ``is_undirected`` adds every edge in the opposite direction."""
    df = df.copy()
    if all(isinstance(c, (int, np.integer)) for c in df.columns.values.tolist()):
        df.columns = ["v", "w"] + [f"edge_attr_{i - 2}" for i in range(2, len(df.columns))]
    if not multiedges and df[["v", "w"]].duplicated().any():
        df = df.drop_duplicates(subset=["v", "w"])
    endpoints = df[["v", "w"]].values
    ids, inverse = np.unique(endpoints, return_inverse=True)
    mapping = IndexMap(ids)
    edge_index = torch.from_numpy(inverse.reshape(endpoints.shape).T.astype(np.int64)).contiguous()
    data = Data(edge_index=edge_index if device is None else edge_index.to(device),
                num_nodes=num_nodes if num_nodes is not None else len(ids))
    for col in df.columns:
        if col not in ("v", "w"):
            data[col if col.startswith("edge_") else "edge_" + col] = _column_to_attribute(df[col].values, device)
    g = Graph(data=data, mapping=mapping)
    return g.to_undirected() if is_undirected else g


def _store_column(data: Data, name: str, values: np.ndarray) -> None:
    value = _column_to_attribute(values, None)
    data[name] = value.to(data.edge_index.device) if isinstance(value, torch.Tensor) else value


def add_node_attributes(df: pd.DataFrame, g: Graph) -> None:
    """Node attributes from a DataFrame: nodes in column ``v`` (IDs) or ``index`` (indices), every other column ``x`` becomes
    ``node_x`` ordered by node index; the frame must cover every node exactly once."""
    if "v" in df:
        attributed = list(df["v"])
    elif "index" in df:
        attributed = list(df["index"])
    else:
        raise ValueError("DataFrame must either have `index` or `v` column")
    if len(set(attributed)) < len(attributed):
        raise ValueError("DataFrame cannot contain multiple attribute values for single node")
    if "v" in df:
        if set(attributed) != set(g.nodes):
            raise ValueError("Mismatch between nodes in DataFrame and nodes in graph")
        node_idx = np.asarray(g.mapping.to_idxs(attributed).tolist())
    else:
        if set(attributed) != set(range(g.n)):
            raise ValueError("Mismatch between nodes in DataFrame and nodes in graph")
        node_idx = np.asarray(attributed)
    order = np.argsort(node_idx, kind="stable")               # row of the frame that describes node 0, 1, ...
    for attr in df.columns:
        if attr not in ("v", "index"):
            _store_column(g.data, attr if attr.startswith("node_") else "node_" + attr, df[attr].values[order])


def add_edge_attributes(df: pd.DataFrame, g: Graph, time_attr: str | None = None) -> None:
    """Edge attributes from a DataFrame with columns ``v``, ``w`` (and ``time_attr`` for temporal graphs): every other column ``x``
    becomes ``edge_x`` in the graph's edge order; the frame must describe every edge of the graph."""
    if "v" not in df or "w" not in df:
        raise ValueError("Data frame must have columns `v` and `w` for source and target nodes")
    node_ids = set(df["v"]).union(set(df["w"]))
    if not node_ids.issubset(set(g.nodes)):
        raise ValueError(f"DataFrame contains nodes {node_ids - set(g.nodes)} that do not exist in the graph. "
                         "Please ensure all nodes in the DataFrame are present in the graph.")
    if g.m != len(df):
        raise ValueError(f"DataFrame contains {len(df)} edges, but the graph has {g.m} edges. "
                         "Please ensure the DataFrame matches the number of edges in the graph.")
    src = g.mapping.to_idxs(df["v"].tolist()).tolist()
    tgt = g.mapping.to_idxs(df["w"].tolist()).tolist()
    attrs = [a for a in df.columns if a not in ("v", "w")]
    position = np.empty(len(df), dtype=np.int64)             # position[k] = index of the graph edge that row k describes
    if time_attr is not None:
        if time_attr not in df:
            raise ValueError(f"Data frame must have column {time_attr} for time stamps")
        attrs.remove(time_attr)
        lookup = g.tedge_to_index
        for k, (s_, t_, ts) in enumerate(zip(src, tgt, df[time_attr].values.tolist())):
            if (s_, t_, ts) not in lookup:
                raise ValueError(f"Edge ({s_}, {t_}) does not exist at time {ts} in the graph.")
            position[k] = lookup[s_, t_, ts]
    else:
        lookup = g.edge_to_index
        for k, (s_, t_) in enumerate(zip(src, tgt)):
            if (s_, t_) not in lookup:
                raise ValueError(f"Edge ({s_}, {t_}) does not exist in the graph.")
            position[k] = lookup[s_, t_]
    # like the reference (pandas.py:308-315: ``df.iloc[edge_idx]``) the rows are taken in the order of the positions found
    for attr in attrs:
        _store_column(g.data, attr if attr.startswith("edge_") else "edge_" + attr, df[attr].values[position])


def graph_to_df(graph: Graph, node_indices: Optional[bool] = False) -> pd.DataFrame:
    """One row per edge: ``v``, ``w`` and every ``edge_*`` attribute."""
    ei = graph.data.edge_index.cpu()
    if node_indices or not graph.mapping.has_ids:
        v, w = ei[0].numpy(), ei[1].numpy()
    else:
        v, w = graph.mapping.to_ids(ei[0]), graph.mapping.to_ids(ei[1])
    frame = pd.DataFrame({"v": v, "w": w})
    for attr in graph.edge_attrs():
        value = graph.data[attr]
        value = value.cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
        frame[attr] = list(value) if value.ndim > 1 else value
    return frame


def read_csv_graph(filename: str, sep: str = ",", header: bool = True, is_undirected: bool = False, multiedges: bool = False,
                   **kwargs: Any) -> Graph:
    df = pd.read_csv(filename, header=0 if header else None, sep=sep)
    return df_to_graph(df, is_undirected=is_undirected, multiedges=multiedges, **kwargs)


def temporal_graph_to_df(graph: TemporalGraph, node_indices: Optional[bool] = False) -> pd.DataFrame:
    """One row per event: ``v``, ``w``, ``t`` and every ``edge_*`` attribute, in time order."""
    ei = graph.data.edge_index.cpu()
    if node_indices or not graph.mapping.has_ids:
        v, w = ei[0].numpy(), ei[1].numpy()
    else:
        v, w = graph.mapping.to_ids(ei[0]), graph.mapping.to_ids(ei[1])
    frame = pd.DataFrame({"v": v, "w": w, "t": graph.data.time.cpu().numpy()})
    for attr in graph.edge_attrs():
        value = graph.data[attr]
        value = value.cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
        frame[attr] = list(value) if value.ndim > 1 else value
    return frame


# ---------------------------------------------------------------------------------------------------------------------------------
# Native ingest of integer edge lists (csrc/pp_ingest.hip): with a CUDA ``device``, a file whose every non-blank line is exactly
# ``[0-9]{1,18} sep [0-9]{1,18} sep -?[0-9]{1,18}`` is indexed, parsed, de-duplicated and mapped to node indices on the device; only the
# sorted node IDs come back to the host.  Every other file (and every other call) takes the pandas code below, unchanged: the kernels
# report what disqualifies a file in a status word, nothing is raised, and pandas decides what such a file means.
#
# read_csv_path_data has the same arrangement for n-gram files of integer node IDs (the pp_ingest_tokens_* half of that file): tokens, not
# lines, are indexed and parsed on the device, and every other file takes the csv.reader code of that function, unchanged.
NATIVE_CSV = True          # False: read_csv_temporal_graph always takes the pandas path, read_csv_path_data always its csv.reader code
CHUNK_BYTES = 1 << 30      # the file goes to the device in pieces of at most this many bytes, each ending at a '\n' (always below 2^31)

_NO_LINES = 64             # PP_INGEST_NO_LINES: a piece of blank lines only disqualifies nothing, a file without any data line does
_SEARCH_WINDOW = 1 << 16


def _native_sep(sep) -> int | None:
    """The separator as a byte value when the kernels take it: one ASCII byte, no digit, ``-``, ``\\r`` or ``\\n`` (nor ``"``, which
    pandas treats as a quote)."""
    if not isinstance(sep, str) or len(sep) != 1 or ord(sep) >= 128 or ord(sep) == 0:
        return None
    if sep.isdigit() or sep in '-\r\n"':
        return None
    return ord(sep)


def _header_length(head: bytes, sep: str) -> int | None:
    """Bytes the header line takes (terminator included) when the file starts with exactly ``v<sep>w<sep>t`` + ``\\n`` / ``\\r\\n`` /
    end of file; ``None`` for any other first line."""
    want = f"v{sep}w{sep}t".encode()
    if not head.startswith(want):
        return None
    rest = head[len(want):len(want) + 2]
    if rest == b"":
        return len(want)
    if rest[:1] == b"\n":
        return len(want) + 1
    if rest == b"\r\n":
        return len(want) + 2
    return None


def _newline_end_before(raw: np.ndarray, lo: int, hi: int) -> int:
    """Index just behind the last ``\\n`` of ``raw[lo:hi]``, -1 if there is none (searched backwards, a window at a time)."""
    b = hi
    while b > lo:
        a = max(lo, b - _SEARCH_WINDOW)
        at = raw[a:b].tobytes().rfind(b"\n")
        if at >= 0:
            return a + at + 1
        b = a
    return -1


def _newline_end_from(raw: np.ndarray, lo: int) -> int:
    """Index just behind the first ``\\n`` of ``raw[lo:]``, ``len(raw)`` if there is none."""
    n = len(raw)
    a = lo
    while a < n:
        b = min(n, a + _SEARCH_WINDOW)
        at = raw[a:b].tobytes().find(b"\n")
        if at >= 0:
            return a + at + 1
        a = b
    return n


def _cut_chunks(raw, chunk_bytes: int, start: int = 0) -> list[tuple[int, int]]:
    """``[(lo, hi), ...]`` covering ``raw[start:]`` in order: every piece has at most ``chunk_bytes`` bytes and ends behind a ``\\n``
    (or at the end of the input: a last line without ``\\n`` is kept); a piece that would hold no ``\\n`` grows to the next one."""
    if isinstance(raw, (bytes, bytearray)):
        raw = np.frombuffer(raw, dtype=np.uint8)
    chunk_bytes = max(1, min(int(chunk_bytes), _hip.INGEST_MAX_CHUNK))
    n, lo, out = len(raw), start, []
    while lo < n:
        hi = min(lo + chunk_bytes, n)
        if hi < n:
            cut = _newline_end_before(raw, lo, hi)
            hi = cut if cut > lo else _newline_end_from(raw, hi)
        out.append((lo, hi))
        lo = hi
    return out


def _first_occurrences(rows: torch.Tensor) -> torch.Tensor | None:
    """Mask of the rows of ``rows`` [n, k] that no earlier row equals (``DataFrame.drop_duplicates`` keeps those, in order); ``None`` when
    every row is distinct."""
    n = rows.size(0)
    uniq, inverse = _hip.unique_rows(rows)
    if uniq.size(0) == n:
        return None
    order = _hip.argsort(inverse, (0, uniq.size(0) - 1))                    # stable: inside a group of equal rows the file order stays
    grouped = inverse[order]
    head = torch.ones(n, dtype=torch.bool, device=rows.device)
    head[1:] = grouped[1:] != grouped[:-1]
    keep = torch.zeros(n, dtype=torch.bool, device=rows.device)
    keep[order[head]] = True
    return keep


def _read_csv_temporal_native(filename, sep: str, header: bool, time_rescale, multiedges: bool, num_nodes, device: torch.device):
    """The TemporalGraph of a qualifying file, ``None`` for a file (or arguments) the native path does not take."""
    sep_byte = _native_sep(sep)
    if sep_byte is None or not isinstance(filename, (str, os.PathLike)) or not os.path.isfile(filename):
        return None
    if isinstance(time_rescale, bool) or not isinstance(time_rescale, (int, np.integer)) or time_rescale < 1:
        return None
    raw = np.fromfile(filename, dtype=np.uint8)
    start = 0
    if header:
        start = _header_length(raw[:8].tobytes(), sep)
        if start is None:
            return None
    with torch.cuda.device(device):
        dev = torch.device("cuda", torch.cuda.current_device())
        parts = []
        for lo, hi in _cut_chunks(raw, CHUNK_BYTES, start):
            if hi - lo > _hip.INGEST_MAX_CHUNK:
                return None
            chunk = torch.from_numpy(raw[lo:hi]).to(dev)
            ws = _hip.ingest_workspace(hi - lo, dev)
            line_start = _hip.ingest_index(chunk, sep_byte, ws)
            cols = _hip.ingest_parse(chunk, sep_byte, line_start, ws)
            n_lines, status, bad_at = _hip.ingest_result(ws)                 # the chunk's one read-back
            if status & ~_NO_LINES:
                _log.debug("native ingest: %s does not qualify (status %#x, byte %d): pandas reads it", filename, status, lo + bad_at)
                return None
            if n_lines:
                parts.append(cols[:, :n_lines].clone())                     # (cols has the capacity of the worst case: let it go)
            del chunk, line_start, cols, ws
        if not parts:
            _log.debug("native ingest: %s has no data line: pandas reads it", filename)
            return None
        cols = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        del parts
        if cols.size(1) >= 1 << 30:                                         # (the 2 n endpoints are indexed with 32 bits)
            return None
        v, w, t = cols[0], cols[1], cols[2]
        if time_rescale != 1:
            t = torch.div(t, int(time_rescale), rounding_mode="floor")
        if not multiedges:
            keep = _first_occurrences(torch.stack([v, w, t], dim=1))
            if keep is not None:
                v, w, t = v[keep], w[keep], t[keep]
        # np.unique(df[["v", "w"]].values, return_inverse=True): sorted IDs, inverse in row-major (v0, w0, v1, w1, ...) order
        ids, inverse = _hip.unique_rows(torch.stack([v, w], dim=1).reshape(-1, 1))
        edge_index = inverse.view(-1, 2).t().contiguous()
        ids = ids.view(-1).cpu().numpy()
        data = Data(edge_index=edge_index, time=t.contiguous(), num_nodes=num_nodes if num_nodes is not None else len(ids))
        return TemporalGraph(data=data, mapping=IndexMap(ids))


def read_csv_temporal_graph(filename: str, sep: str = ",", header: bool = True, timestamp_format: str = "%Y-%m-%d %H:%M:%S",
                            time_rescale: int = 1, **kwargs: Any) -> TemporalGraph:
    """Temporal graph from a ``v, w, t`` (+ edge attributes) text file.  With a CUDA ``device`` an all-integer three-column file is
    parsed on the device (see ``NATIVE_CSV`` above); everything else goes through ``pandas.read_csv``.  Both give the same graph."""
    if NATIVE_CSV and set(kwargs) <= {"multiedges", "num_nodes", "device"} and kwargs.get("device") is not None:
        try:
            device = torch.device(kwargs["device"])
        except (RuntimeError, TypeError, ValueError):
            device = None
        if device is not None and device.type == "cuda":
            g = _read_csv_temporal_native(filename, sep, header, time_rescale, bool(kwargs.get("multiedges", False)),
                                          kwargs.get("num_nodes"), device)
            if g is not None:
                return g
    df = pd.read_csv(filename, header=0 if header else None, sep=sep)
    return df_to_temporal_graph(df, timestamp_format=timestamp_format, time_rescale=time_rescale, **kwargs)


def write_csv(graph, node_indices: bool = False, path_or_buf: Any = None, **pdargs: Any) -> None:
    frame = temporal_graph_to_df(graph, node_indices) if isinstance(graph, TemporalGraph) else graph_to_df(graph, node_indices)
    frame.to_csv(index=False, path_or_buf=path_or_buf, **pdargs)


def _string_order(ids: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Distinct non-negative integer IDs -> ``(node_ids, rank)``: the IDs as the strings the file held (no leading zeros, dtype
    ``<U{longest}``), sorted as ``np.unique`` sorts strings (code points: ``'10' < '2'``), and ``rank[j]`` = index of ``ids[j]`` in it."""
    ids = np.asarray(ids, dtype=np.int64)
    width = max(len(str(int(ids.max()))), 1) if ids.size else 1
    strings = ids.astype(f"<U{width}")
    order = np.argsort(strings, kind="stable")
    rank = np.empty(len(ids), dtype=np.int64)
    rank[order] = np.arange(len(ids), dtype=np.int64)
    return strings[order], rank


def _read_csv_paths_native(path_or_buf, weight: bool, sep, device: torch.device) -> PathData | None:
    """The PathData of a qualifying integer n-gram file (csrc/pp_ingest.hip, the pp_ingest_tokens_* half), ``None`` for a file (or
    arguments) the native path does not take: the caller's host code then reads it.  Node IDs come out as the host code makes them:
    strings in ``np.unique`` order."""
    sep_byte = _native_sep(sep)
    if sep_byte is None or device.type != "cuda" or not isinstance(path_or_buf, (str, os.PathLike)) or not os.path.isfile(path_or_buf):
        return None
    weight = bool(weight)
    raw = np.fromfile(path_or_buf, dtype=np.uint8)
    with torch.cuda.device(device):
        dev = torch.device("cuda", torch.cuda.current_device())
        parts = []
        for lo, hi in _cut_chunks(raw, CHUNK_BYTES):
            if hi - lo > _hip.INGEST_MAX_CHUNK:
                return None
            chunk = torch.from_numpy(raw[lo:hi]).to(dev)
            ws = _hip.ingest_tokens_workspace(hi - lo, dev)
            index = _hip.ingest_tokens_index(chunk, sep_byte, ws)
            nodes, lengths, weights = _hip.ingest_tokens_parse(chunk, sep_byte, weight, index, ws)
            n_lines, n_tokens, status, bad_at = _hip.ingest_tokens_result(ws)          # the chunk's one read-back
            if status & ~_NO_LINES:
                _log.debug("native ingest: %s does not qualify (status %#x, byte %d): the host code reads it", path_or_buf, status, lo + bad_at)
                return None
            if n_lines:                                                     # (the outputs have the capacity of the worst case: let them go)
                parts.append((nodes[:n_tokens - n_lines if weight else n_tokens].clone(), lengths[:n_lines].clone(),
                              weights[:n_lines].clone() if weight else None))
            del chunk, ws, index, nodes, lengths, weights
        if not parts:
            _log.debug("native ingest: %s has no data line: the host code reads it", path_or_buf)
            return None
        nodes = parts[0][0] if len(parts) == 1 else torch.cat([p[0] for p in parts])
        lengths = parts[0][1] if len(parts) == 1 else torch.cat([p[1] for p in parts])
        if weight:
            weights = parts[0][2] if len(parts) == 1 else torch.cat([p[2] for p in parts])
        else:
            weights = torch.ones(lengths.numel(), dtype=torch.float32, device=dev)
        del parts
        positions = nodes.numel()
        if positions >= 1 << 31:
            return None
        # np.unique(np.hstack(paths)) of the host code: the distinct IDs AS STRINGS, in string order
        ids, inverse = _hip.unique_rows(nodes.view(-1, 1))
        node_ids, rank = _string_order(ids.view(-1).cpu().numpy())
        node_idx = torch.from_numpy(rank).to(dev)[inverse]
        # PathData.append_walks from here on, on device tensors: every position but a walk's last one starts an edge
        pos = torch.arange(positions, device=dev)
        last_of_walk = torch.zeros(positions, dtype=torch.bool, device=dev)
        last_of_walk[torch.cumsum(lengths, 0) - 1] = True
        tails = pos[~last_of_walk]
        out = PathData(IndexMap(node_ids), dev)
        out._append(torch.stack((tails, tails + 1)), node_idx.unsqueeze(1), weights, lengths)
        return out


def read_csv_path_data(path_or_buf: Any = None, weight: bool = True, sep=",", device: Optional[torch.device] = None) -> PathData:
    """Walks from an n-gram file: one walk per line, node IDs separated by ``sep``, optionally a trailing weight.  With a CUDA
    ``device`` a file of integer IDs (and plain decimal weights) is indexed and parsed on the device (see ``NATIVE_CSV`` above);
    everything else is read by the host code below.  Both give the same walk store."""
    if NATIVE_CSV and device is not None:
        try:
            dev = torch.device(device)
        except (RuntimeError, TypeError, ValueError):
            dev = None
        if dev is not None and dev.type == "cuda":
            paths_native = _read_csv_paths_native(path_or_buf, weight, sep, dev)
            if paths_native is not None:
                return paths_native
    with open(path_or_buf, "r") as fh:
        rows = [r for r in csv.reader(fh, delimiter=sep) if r]
    if weight:
        paths = [r[:-1] for r in rows]
        weights = [ast.literal_eval(r[-1]) for r in rows]
    else:
        paths, weights = rows, [1.0] * len(rows)
    mapping = IndexMap()
    mapping.add_ids(np.unique(np.hstack(paths)))
    out = PathData(mapping, device)
    out.append_walks(node_seqs=paths, weights=weights)
    return out
