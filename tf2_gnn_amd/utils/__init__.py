from .constants import LAYER_NORM_EPSILON, LEAKY_RELU_ALPHA, SEGMENT_SOFTMAX_EPSILON, SMALL_NUMBER
from .param_helpers import get_activation_function, get_aggregation_function

__all__ = [
    "LAYER_NORM_EPSILON",
    "LEAKY_RELU_ALPHA",
    "SEGMENT_SOFTMAX_EPSILON",
    "SMALL_NUMBER",
    "get_activation_function",
    "get_aggregation_function",
    "TaskInfo",
    "register_task",
    "clear_known_tasks",
    "get_known_tasks",
    "task_name_to_dataset_class",
    "task_name_to_model_class",
]

_TASK_UTILS = ("TaskInfo", "register_task", "clear_known_tasks", "get_known_tasks", "task_name_to_dataset_class",
               "task_name_to_model_class")


def __getattr__(name):
    # the task registry names the task models, and tasks.py imports this package: resolved at first use, not at import
    if name in _TASK_UTILS:
        import importlib

        return getattr(importlib.import_module(".task_utils", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
