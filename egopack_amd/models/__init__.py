from .graph import Graph  # noqa: F401
from .task_weighting import TaskLogVariance  # noqa: F401
