#!/usr/bin/env python3
"""Generate tests/golden/generative_vectors.npz from the REFERENCE's own ``max_edges`` and G(n,p) likelihood functions.

Run where a checkout of the reference exists; no test needs it for the fixtures.  The four functions are loaded from their source file by
name with ``ast`` (the route make_golden_wl.py takes) and run on duck-typed graphs that offer what they read: ``n``, ``m`` and
``is_directed()``.  Nothing of the reference's text is written to the repository: only inputs and the outputs its code produced for them.

    python tests/golden/make_golden_generative.py <path to the reference's src/pathpyG>

``max_edges/in`` int64 [k, 4] holds (n, directed, multi_edges, self_loops), ``max_edges/out`` float64 [k] the values (inf for multi-edges)
and ``max_edges/is_int`` whether the function returned a Python int.  ``llh/in_p`` float64 [c], ``llh/in_graph`` int64 [c, 3] = (n, m,
directed); ``llh/likelihood``, ``llh/log_likelihood``, ``llh/mle`` float64 [c] (nan where the function raised) and ``llh/raised`` int64 [c]:
1 where all three raised NotImplementedError (directed graphs).
"""
from __future__ import annotations

import ast
import logging
import pathlib
import sys
import warnings

import numpy as np
import scipy.special

OUT = pathlib.Path(__file__).resolve().parent
NAMES = ("max_edges", "erdos_renyi_gnp_likelihood", "erdos_renyi_gnp_log_likelihood", "erdos_renyi_gnp_mle")


def load_reference(ref: pathlib.Path) -> dict:
    logger = logging.getLogger("golden")
    logger.disabled = True
    ns = {"_np": np, "scipy": scipy, "logger": logger}
    path = ref / "algorithms" / "generative_models.py"
    for node in ast.parse(path.read_text()).body:
        if isinstance(node, ast.FunctionDef) and node.name in NAMES:
            node.returns = None
            for arg in node.args.args:
                arg.annotation = None
            exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), str(path), "exec"), ns)  # noqa: S102 - the reference's own function
    return ns


class DuckGraph:
    def __init__(self, n, m, directed):
        self.n, self.m, self._directed = n, m, directed

    def is_directed(self):
        return self._directed


def max_edges_cases():
    for n in (0, 1, 2, 3, 7, 100, 4097, 100000):
        for directed in (False, True):
            for multi in (False, True):
                for loops in (False, True):
                    yield n, directed, multi, loops


def llh_cases():
    """(p, n, m, directed)"""
    for n, m in ((0, 0), (1, 0), (2, 0), (2, 1), (5, 4), (10, 45), (10, 0), (40, 200)):
        for p in (0.0, 0.25, 0.5, 1.0):
            yield p, n, m, False
    yield 0.1, 300, 4000, False
    yield 1e-3, 2000, 1900, False
    for p, n, m in ((0.5, 5, 4), (0.0, 2, 1), (1.0, 0, 0)):
        yield p, n, m, True


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    ref = load_reference(pathlib.Path(sys.argv[1]))
    store = {}
    cases = list(max_edges_cases())
    values = [ref["max_edges"](n, directed=d, multi_edges=mu, self_loops=lo) for n, d, mu, lo in cases]
    store["max_edges/in"] = np.array(cases, dtype=np.int64)
    store["max_edges/out"] = np.array(values, dtype=np.float64)
    store["max_edges/is_int"] = np.array([type(v) is int for v in values], dtype=np.int64)
    cases = list(llh_cases())
    out = {name: [] for name in NAMES[1:]}
    raised = []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for p, n, m, directed in cases:
            g = DuckGraph(n, m, directed)
            count = 0
            for name in NAMES[1:]:
                try:
                    out[name].append(float(ref[name](p, g) if name != "erdos_renyi_gnp_mle" else ref[name](g)))
                except NotImplementedError:
                    out[name].append(float("nan"))
                    count += 1
            assert count in (0, 3), (p, n, m, directed)
            raised.append(count == 3)
    store["llh/in_p"] = np.array([c[0] for c in cases], dtype=np.float64)
    store["llh/in_graph"] = np.array([[c[1], c[2], c[3]] for c in cases], dtype=np.int64)
    store["llh/likelihood"] = np.array(out[NAMES[1]], dtype=np.float64)
    store["llh/log_likelihood"] = np.array(out[NAMES[2]], dtype=np.float64)
    store["llh/mle"] = np.array(out[NAMES[3]], dtype=np.float64)
    store["llh/raised"] = np.array(raised, dtype=np.int64)
    np.savez_compressed(OUT / "generative_vectors.npz", **store)
    print(f"{len(store['max_edges/in'])} max_edges cases, {len(cases)} likelihood cases -> {OUT / 'generative_vectors.npz'}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
