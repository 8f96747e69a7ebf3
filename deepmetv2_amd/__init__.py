"""deepmetv2_amd -- MI355X-native operators for the DeepMETv2 DynamicEdgeConv -> MET hot path.

Drop-in names (same spelling and argument meaning as the third-party operators the reference imports at
/root/reference/model/graph_met_network.py:7,9, model/net.py:8, train.py:10):

    from deepmetv2_amd import EdgeConv, DynamicEdgeConv      # torch_geometric.nn
    from deepmetv2_amd import knn_graph, radius_graph, knn, radius   # torch_cluster
    from deepmetv2_amd import scatter_add, scatter_max       # torch_scatter
    from deepmetv2_amd import graclus                        # torch_cluster
    from deepmetv2_amd import fps, nearest                   # torch_cluster
    from deepmetv2_amd import normalized_cut, max_pool, max_pool_x, global_max_pool   # torch_geometric
    from deepmetv2_amd import GravNetConv                    # torch_geometric.nn
    from deepmetv2_amd import TransformerConv                # torch_geometric.nn (attention_aggregate: utils.softmax + sum)
    from deepmetv2_amd import knn_interpolate                # torch_geometric.nn.unpool (interpolate_aggregate: its sums)
    from deepmetv2_amd import PointNetConv, PointConv        # torch_geometric.nn (pointnet_aggregate: message + max)
    from deepmetv2_amd import GATConv, GATv2Conv             # torch_geometric.nn (gat_v1_aggregate / gat_aggregate)
    from deepmetv2_amd import scatter, scatter_sum, scatter_mean, scatter_min, segment_csr      # torch_scatter
    from deepmetv2_amd import scatter_softmax, scatter_log_softmax, scatter_logsumexp           # torch_scatter.composite
    from deepmetv2_amd import softmax                        # torch_geometric.utils
    from deepmetv2_amd import AttentionalAggregation         # torch_geometric.nn.aggr (GlobalAttention)
    from deepmetv2_amd import PNAConv, DegreeScalerAggregation   # torch_geometric.nn (multi_aggregate: its statistics)
    from deepmetv2_amd import scatter_std                    # torch_scatter.composite
    from deepmetv2_amd import GCNConv, GraphConv, SAGEConv, GINConv   # torch_geometric.nn (weighted_aggregate: propagate)
    from deepmetv2_amd import gcn_norm                       # torch_geometric.nn.conv.gcn_conv
    from deepmetv2_amd import spmm                           # torch_sparse
    from deepmetv2_amd import GraphNorm, InstanceNorm, LayerNorm, PairNorm, GraphSizeNorm, MeanSubtractionNorm   # torch_geometric.nn
                                                             # (event_moments / event_normalize: their statistics and pass)
    from deepmetv2_amd import TopKPooling, SAGPooling        # torch_geometric.nn
    from deepmetv2_amd import topk, filter_adj               # torch_geometric.nn.pool.select / .connect (filter_table: tables)
    from deepmetv2_amd import SortAggregation, global_sort_pool   # torch_geometric.nn.aggr / torch_geometric.nn
    from deepmetv2_amd import grid_cluster                   # torch_cluster
    from deepmetv2_amd import voxel_grid, consecutive_cluster   # torch_geometric.nn / torch_geometric.nn.pool.consecutive
    from deepmetv2_amd import EdgePooling                    # torch_geometric.nn (edge_matching: its _merge_edges)
    from deepmetv2_amd import connected_components, largest_connected_components   # scipy.sparse.csgraph / PyG's
                                                             # LargestConnectedComponents, per event on the device
    from deepmetv2_amd import dbscan, dbscan_graph           # sklearn.cluster.DBSCAN (dbscan_graph: over a given graph)
    from deepmetv2_amd import condensation_cluster, condensation_points   # object-condensation inference (Kieseler 2020):
                                                             # upstream's host loop over the condensation points

All of them run hand-written HIP kernels for gfx950 through the C ABI in include/dmet.h
(deepmetv2_amd/libdmet_hip.so, built by `python -m deepmetv2_amd.build`).  There is no CPU implementation:
calling an operator without the library or with non-GPU tensors raises.
"""
from .cluster import (fps, knn, knn_graph, knn_table, knn_xy_table, nearest, radius, radius_graph, radius_table,
                      radius_xy_table)
from .conv import DynamicEdgeConv, EdgeConv
from .data import Batch, DeviceLoader, EventLoader, collate, events_from_padded
from .graph import BipartiteTable, GraphFuture, NeighborTable, build_async, raise_deferred_errors, register_batch, to_undirected
from .metrics import metrics, resolution, u_perp_par_loss
from . import scatter        # the module, callable as torch_scatter.scatter (see its last lines)
from .scatter import (met_reduce, scatter_add, scatter_log_softmax, scatter_logsumexp, scatter_max, scatter_mean,
                      scatter_min, scatter_softmax, scatter_std, scatter_sum, segment_csr, softmax)
from .aggr import AttentionalAggregation
from .nn import accelerate
from .pool import (avg_pool, avg_pool_x, consecutive_cluster, global_add_pool, global_max_pool, global_mean_pool, graclus,
                   grid_cluster, max_pool, max_pool_x, normalized_cut, normalized_cut_2d, voxel_grid)
from .drn import DynamicReductionNetwork
from .gravnet import GravNetConv, gravnet_aggregate
from .attention import TransformerConv, attention_aggregate
from .interpolate import interpolate_aggregate, knn_interpolate
from .pointnet import PointConv, PointNetConv, pointnet_aggregate
from .gat import GATConv, GATv2Conv, gat_aggregate, gat_v1_aggregate
from .pna import DegreeScalerAggregation, PNAConv, multi_aggregate
from .propagate import spmm, weighted_aggregate
from .gcn import GCNConv, GINConv, GraphConv, SAGEConv, gcn_norm
from .event_norm import (GraphNorm, GraphSizeNorm, InstanceNorm, LayerNorm, MeanSubtractionNorm, PairNorm, event_moments,
                         event_normalize)
from .select import SAGPooling, SortAggregation, TopKPooling, filter_adj, filter_table, global_sort_pool, topk
from .edge_pool import EdgePooling, edge_matching
from .components import connected_components, dbscan, dbscan_graph, largest_connected_components
from .condense import condensation_cluster, condensation_points

__all__ = [
    "EdgeConv", "DynamicEdgeConv", "knn", "knn_graph", "knn_table", "knn_xy_table", "radius", "radius_graph", "radius_table",
    "radius_xy_table", "BipartiteTable",
    "scatter_add", "scatter_max", "met_reduce", "NeighborTable", "register_batch", "metrics", "resolution",
    "u_perp_par_loss", "to_undirected", "raise_deferred_errors", "accelerate", "build_async", "GraphFuture", "Batch", "EventLoader", "DeviceLoader", "collate", "events_from_padded",
    "graclus", "normalized_cut", "normalized_cut_2d", "max_pool", "max_pool_x", "avg_pool", "avg_pool_x",
    "global_max_pool", "global_mean_pool", "global_add_pool", "DynamicReductionNetwork",
    "grid_cluster", "voxel_grid", "consecutive_cluster",
    "GravNetConv", "gravnet_aggregate", "TransformerConv", "attention_aggregate", "fps", "nearest",
    "knn_interpolate", "interpolate_aggregate", "PointNetConv", "PointConv", "pointnet_aggregate",
    "GATConv", "GATv2Conv", "gat_aggregate", "gat_v1_aggregate",
    "scatter", "scatter_sum", "scatter_mean", "scatter_min", "scatter_softmax", "scatter_log_softmax", "scatter_logsumexp",
    "segment_csr", "softmax", "AttentionalAggregation",
    "PNAConv", "DegreeScalerAggregation", "multi_aggregate", "scatter_std",
    "GCNConv", "GraphConv", "SAGEConv", "GINConv", "gcn_norm", "weighted_aggregate", "spmm",
    "GraphNorm", "InstanceNorm", "LayerNorm", "PairNorm", "GraphSizeNorm", "MeanSubtractionNorm", "event_moments",
    "event_normalize",
    "TopKPooling", "SAGPooling", "SortAggregation", "global_sort_pool", "topk", "filter_adj", "filter_table",
    "EdgePooling", "edge_matching",
    "connected_components", "largest_connected_components", "dbscan_graph", "dbscan",
    "condensation_cluster", "condensation_points",
]
__version__ = "0.1.0"
