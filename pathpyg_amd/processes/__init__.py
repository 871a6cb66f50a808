"""Processes on graphs and on the layers of a :class:`~pathpyg_amd.MultiOrderModel`, on the GPU: ``pp.processes.RandomWalk`` samples walks and
evolves distributions (``evolve``, ``stationary_distribution``)."""
from . import random_walk  # noqa: F401
from .random_walk import Evolution, RandomWalk, WalkBatch  # noqa: F401


def __getattr__(name):
    if name == "last_seed":          # the seed of the most recent :meth:`RandomWalk.run` (``None`` before the first)
        return random_walk.last_seed
    raise AttributeError(name)
