from .synthetic import make_ppi_shaped_batch, make_qm9_shaped_batch, make_synthetic_batch, make_zipf_typed_batch, rmat_edges
from .utils import compute_number_of_edge_types, get_tied_edge_types, process_adjacency_lists
from .batching import GraphSample, batch_adjacency_lists, check_batch, graph_batch_iterator_from_graph_iterator
from .graph_dataset import (DataFold, EpochPlan, FoldStore, GraphDataset, PackedFold, assemble_batch, batch_assemble_launch_counts,
                            plan_batches)
from .jsonl_graph_dataset import JsonLGraphDataset
from .jsonl_graph_property_dataset import GraphWithPropertySample, JsonLGraphPropertyDataset
from .ppi_dataset import PPIDataset, PPIGraphSample
from .qm9_dataset import QM9Dataset, QM9GraphSample
from .neighbor_sampling import NeighborStore, batch_key, build_in_csr, plan_seed_chunks, sampled_batch
from .node_classification_dataset import NodeClassificationDataset
from .link_prediction_dataset import LinkPredictionDataset
