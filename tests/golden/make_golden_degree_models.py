#!/usr/bin/env python3
"""Generate tests/golden/degree_models_vectors.npz from the REFERENCE's own ``is_graphic_erdos_gallai``.

Run where a checkout of the reference exists; no test needs it for the fixtures.  The function is loaded from its source file by name with
``ast`` (the route make_golden_generative.py takes).  Nothing of the reference's text is written to the repository: only the degree
sequences and the booleans its code returned for them.

    python tests/golden/make_golden_degree_models.py <path to the reference's src/pathpyG>

``eg/values`` int64 [total] holds the sequences back to back, ``eg/ptr`` int64 [k + 1] where each begins, ``eg/graphic`` int64 [k] what the
reference answered.  The cases: the six sequences of the reference's own test, the tutorial's two, the empty sequence, 2000 seeded
sequences with 2 <= n <= 12 and entries in 0 .. n (half of them uniform, half the degrees of a random graph with, every other time, one
entry redrawn — so that both answers are well represented), and eight with n = 200.
"""
from __future__ import annotations

import ast
import pathlib
import sys

import numpy as np

OUT = pathlib.Path(__file__).resolve().parent
NAME = "is_graphic_erdos_gallai"


def load_reference(ref: pathlib.Path):
    ns = {"_np": np}
    path = ref / "algorithms" / "generative_models.py"
    for node in ast.parse(path.read_text()).body:
        if isinstance(node, ast.FunctionDef) and node.name == NAME:
            node.returns = None
            for arg in node.args.args:
                arg.annotation = None
            exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), str(path), "exec"), ns)  # noqa: S102 - the reference's own function
    return ns[NAME]


def graph_degrees(rng, n: int, p: float) -> list:
    upper = np.triu(rng.random((n, n)) < p, 1)
    return (upper.sum(0) + upper.sum(1)).astype(int).tolist()


def cases() -> list:
    out = [[1, 0], [1, 3], [1, 1], [1, 3, 1, 1], [1, 3, 0, 2], [3, 2, 2, 1], [2, 2, 3, 2, 3], [2, 2, 6, 2, 3], []]
    rng = np.random.default_rng(20240611)
    for i in range(2000):
        n = int(rng.integers(2, 13))
        if i % 2 == 0:
            seq = rng.integers(0, n + 1, size=n).tolist()
        else:
            seq = graph_degrees(rng, n, float(rng.random()))
            if i % 4 == 1:
                seq[int(rng.integers(n))] = int(rng.integers(0, n + 1))
        out.append(seq)
    for i in range(8):
        seq = graph_degrees(rng, 200, (0.02, 0.3, 0.9, 0.5)[i % 4])
        if i >= 4:                                                      # raise the largest degrees: the condition fails at a middle r, if at all
            order = np.argsort(seq)[::-1]
            for v in order[:25 * (i - 3)]:
                seq[v] = min(199, seq[v] + 2 * int(rng.integers(1, 40)))
        out.append(seq)
    return out


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    graphic = load_reference(pathlib.Path(sys.argv[1]))
    seqs = cases()
    answers = [bool(graphic(list(s))) for s in seqs]
    store = {
        "eg/values": np.array([d for s in seqs for d in s], dtype=np.int64),
        "eg/ptr": np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64),
        "eg/graphic": np.array(answers, dtype=np.int64),
    }
    np.savez_compressed(OUT / "degree_models_vectors.npz", **store)
    print(f"{len(seqs)} sequences, {sum(answers)} graphic -> {OUT / 'degree_models_vectors.npz'}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
