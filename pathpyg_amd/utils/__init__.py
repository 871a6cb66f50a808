from .dbgnn import generate_bipartite_edge_index  # noqa: F401
from .split import random_node_split  # noqa: F401
