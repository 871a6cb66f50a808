"""Descriptive statistics of a static graph: clustering coefficients, the degree distribution with its moments and assortativity, and
neighbourhood similarities between nodes (reference ``pathpyG.statistics``).

    g = pp.Graph.from_edge_list([("b", "c"), ("a", "b"), ("c", "d"), ("d", "a"), ("b", "d")])
    pp.statistics.degree_distribution(g)
    pp.statistics.avg_clustering_coefficient(g)
    pp.statistics.node_similarities.jaccard_similarity(g, "a", "b")

The names of the reference are here with its results; ``closed_triad_counts``, ``local_clustering_coefficients`` and
``node_similarities.pairwise`` are the all-node / many-pair forms that one device pass answers.
"""
from . import node_similarities  # noqa: F401
from .clustering import (  # noqa: F401
    avg_clustering_coefficient,
    closed_triad_counts,
    closed_triads,
    local_clustering_coefficient,
    local_clustering_coefficients,
)
from .degrees import (  # noqa: F401
    degree_assortativity,
    degree_central_moment,
    degree_distribution,
    degree_generating_function,
    degree_raw_moment,
    degree_sequence,
    mean_degree,
    mean_neighbor_degree,
)

__all__ = [
    "avg_clustering_coefficient",
    "closed_triads",
    "local_clustering_coefficient",
    "degree_assortativity",
    "degree_central_moment",
    "degree_distribution",
    "degree_generating_function",
    "degree_raw_moment",
    "degree_sequence",
    "mean_degree",
    "mean_neighbor_degree",
    "node_similarities",
    "closed_triad_counts",
    "local_clustering_coefficients",
]
