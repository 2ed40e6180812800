"""MI355X-native GAT message passing for the PlotPointe user-item recommender.

Drop-in for the GAT layer of Axionis47/PlotPointe-GAT-Recommendation
(scripts/train_gat_pyg.py:77 GATConv, scripts/train_gat_custom.py:63 SimpleGATLayer).
The directory name is not a Python identifier; import it with
``importlib.import_module("plotpointe-gat-recommendation_amd")`` -- after the first
import it is also registered as ``ppgat_amd``.
"""
import sys as _sys

from . import _lib, data, dist, evaluation, fusion, knn, lightgcn, neighbors, optim, sampler, torch_ops  # noqa: F401
from .conv import GATConv, GATv2Conv, SimpleGATLayer  # noqa: F401
from .evaluation import eval_full, eval_topk, full_rank, recommend_topk, topk_metrics  # noqa: F401
from .hip_ops import CSRGraph, csr_build, gat_aggregate, gatv2_aggregate, graph_cache  # noqa: F401
from .lightgcn import LightGCN  # noqa: F401
from .neighbors import NeighborSampler, Subgraph, SubgraphSampler, sample_neighbors, sample_subgraph  # noqa: F401
from .model import (CustomGAT, PyGGAT, PyGGATv2, bpr_loss, forward_subgraph, shared_softmax_loss,  # noqa: F401
                    softmax_loss)

_sys.modules.setdefault("ppgat_amd", _sys.modules[__name__])

__all__ = ["GATConv", "GATv2Conv", "SimpleGATLayer", "PyGGAT", "PyGGATv2", "CustomGAT", "LightGCN", "lightgcn", "bpr_loss", "softmax_loss", "shared_softmax_loss", "CSRGraph", "csr_build",
           "gat_aggregate", "gatv2_aggregate", "graph_cache", "data", "eval_full", "full_rank", "recommend_topk",
           "topk_metrics", "eval_topk", "NeighborSampler", "sample_neighbors", "Subgraph", "SubgraphSampler",
           "sample_subgraph", "forward_subgraph"]
