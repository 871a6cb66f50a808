"""Algorithms on the hot path of pathpyG: order lifts, De Bruijn aggregation, shortest paths and centralities."""
from . import centrality, components, generative_models, ranking, shortest_paths, weisfeiler_leman  # noqa: F401
from .components import connected_components, largest_connected_component  # noqa: F401
from .weisfeiler_leman import WeisfeilerLeman_test, color_refinement  # noqa: F401
from .centrality import (  # noqa: F401
    betweenness_centrality,
    closeness_centrality,
    eigenvector_centrality,
    katz_centrality,
    map_to_nodes,
    path_node_traversals,
    path_visitation_probabilities,
)
from .ranking import pagerank, personalized_pagerank  # noqa: F401
from .lift_order import (  # noqa: F401
    aggregate_edge_index,
    aggregate_node_attributes,
    lift_order_edge_index,
    lift_order_edge_index_weighted,
)
from .rolling_time_window import RollingTimeWindow, RollingWindows, rolling_static_graphs  # noqa: F401
from .shortest_paths import avg_path_length, diameter, shortest_paths_dijkstra  # noqa: F401
from .temporal import (  # noqa: F401
    lift_order_temporal,
    temporal_betweenness_centrality,
    temporal_closeness_centrality,
    temporal_shortest_paths,
)
