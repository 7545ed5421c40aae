"""Task registry - mirror of tf2_gnn/cli_utils/task_utils.py:13-98: a task name resolves to a dataset class and a model
class, each with the hyper-parameters that task overrides."""
from __future__ import annotations

from typing import Any, Dict, Iterable, NamedTuple, Tuple, Type

from ..data import (GraphDataset, JsonLGraphPropertyDataset, LinkPredictionDataset, NodeClassificationDataset, PPIDataset,
                    QM9Dataset)
from ..tasks import (GraphBinaryClassificationTask, GraphRegressionTask, GraphTaskModel, LinkPredictionTask, NodeClassificationTask,
                     NodeMulticlassTask, QM9RegressionTask)


class TaskInfo(NamedTuple):
    """A named tuple to hold information about a task."""

    name: str
    dataset_class: Type[GraphDataset]
    dataset_default_hypers: Dict[str, Any]
    model_class: Type[GraphTaskModel]
    model_default_hypers: Dict[str, Any]


TASK_NAME_TO_DATASET_AND_MODEL_INFO: Dict[str, TaskInfo] = {}


def register_task(task_name, dataset_class, dataset_default_hypers, model_class, model_default_hypers):
    TASK_NAME_TO_DATASET_AND_MODEL_INFO[task_name.lower()] = TaskInfo(
        name=task_name,
        dataset_class=dataset_class,
        dataset_default_hypers=dataset_default_hypers,
        model_class=model_class,
        model_default_hypers=model_default_hypers,
    )


def clear_known_tasks() -> None:
    TASK_NAME_TO_DATASET_AND_MODEL_INFO.clear()


def get_known_tasks() -> Iterable[str]:
    for task_info in TASK_NAME_TO_DATASET_AND_MODEL_INFO.values():
        yield task_info.name


def _task_info(name: str) -> TaskInfo:
    task_info = TASK_NAME_TO_DATASET_AND_MODEL_INFO.get(name.lower())
    if task_info is None:
        raise ValueError("Unknown task type '%s'" % name)
    return task_info


def task_name_to_dataset_class(name: str) -> Tuple[Type[GraphDataset], Dict[str, Any]]:
    """Map task name to a dataset class and default hyperparameters for that class."""
    task_info = _task_info(name)
    return task_info.dataset_class, task_info.dataset_default_hypers


def task_name_to_model_class(name: str) -> Tuple[Type[GraphTaskModel], Dict[str, Any]]:
    """Map task name to a model class and default hyperparameters for that class."""
    task_info = _task_info(name)
    return task_info.model_class, task_info.model_default_hypers


def register_default_tasks() -> None:
    """The reference's four default tasks (task_utils.py:67-98)."""
    register_task("PPI", PPIDataset, {}, NodeMulticlassTask, {})
    register_task("QM9", QM9Dataset, {}, QM9RegressionTask, {})
    register_task("GraphRegression", JsonLGraphPropertyDataset, {"threshold_for_classification": None}, GraphRegressionTask, {})
    register_task("GraphBinaryClassification", JsonLGraphPropertyDataset, {"threshold_for_classification": 23.0},
                  GraphBinaryClassificationTask, {})


def register_node_classification_task() -> None:
    """One class per node with fold masks over one graph.  The reference has no such task, so it is not among the
    defaults: whoever wants it by name registers it."""
    register_task("NodeClassification", NodeClassificationDataset, {}, NodeClassificationTask, {})


def register_link_prediction_task() -> None:
    """Typed-edge scoring with a DistMult decoder over one graph.  The reference has no such task, so it is not among the
    defaults: whoever wants it by name registers it."""
    register_task("LinkPrediction", LinkPredictionDataset, {}, LinkPredictionTask, {})


register_default_tasks()
