"""DynamicReductionNetwork: the reference's second model (model/dynamic_reduction_network.py:32-103),
composed from this package's operators.

    x = datanorm * x -> inputnet (3 x Linear + ELU)
    -> edge_index = to_undirected(knn_graph(x, k, batch, loop=False)) -> edgeconv1 (EdgeConv over
       Linear(2H, 3H/2) - ELU - Linear(3H/2, H) - ELU - BatchNorm1d(H), aggr)
    -> normalized_cut_2d -> graclus -> max pool                                  (:86-92)
    -> the same again with edgeconv2 and max_pool_x                              (:94-99)
    -> global_max_pool -> output MLP                                             (:101-103)

The attribute names (datanorm, inputnet, edgeconv1, edgeconv2, output) and the defaults k=16, aggr='add' are the
reference's.  The reference file is not part of this repository, so state-dict compatibility with it is UNPINNED: layer
widths and the default `norm` follow SURVEY §3.3 / row N4, not a checked copy of the file.

Differences in mechanics, not in results: the first pooling skips PyG's pool_edge (max_pool's edge coarsening), because
the next knn_graph replaces the edge index; graclus is given the batch vector so that it matches one event per workgroup
(the same bits as the whole-graph call, include/dmet.h); `data` is read, not modified.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .cluster import knn_graph
from .conv import EdgeConv
from .graph import to_undirected
from .pool import global_max_pool, graclus, max_pool_x, normalized_cut_2d


def _edge_nn(hidden_dim: int) -> nn.Sequential:
    middle = 3 * hidden_dim // 2
    return nn.Sequential(nn.Linear(2 * hidden_dim, middle), nn.ELU(), nn.Linear(middle, hidden_dim), nn.ELU(),
                         nn.BatchNorm1d(hidden_dim))


class DynamicReductionNetwork(nn.Module):
    def __init__(self, input_dim: int = 5, hidden_dim: int = 64, output_dim: int = 1, k: int = 16, aggr: str = "add",
                 norm: Optional[torch.Tensor] = None):
        super().__init__()
        if norm is None:
            norm = torch.ones(input_dim)
        self.datanorm = nn.Parameter(torch.as_tensor(norm, dtype=torch.float32).clone())
        self.k = k
        self.inputnet = nn.Sequential(
            nn.Linear(input_dim, hidden_dim // 2), nn.ELU(),
            nn.Linear(hidden_dim // 2, hidden_dim), nn.ELU(),
            nn.Linear(hidden_dim, hidden_dim), nn.ELU(),
        )
        self.edgeconv1 = EdgeConv(nn=_edge_nn(hidden_dim), aggr=aggr)
        self.edgeconv2 = EdgeConv(nn=_edge_nn(hidden_dim), aggr=aggr)
        self.output = nn.Sequential(
            nn.Linear(hidden_dim, hidden_dim), nn.ELU(),
            nn.Linear(hidden_dim, hidden_dim // 2), nn.ELU(),
            nn.Linear(hidden_dim // 2, output_dim),
        )

    def _reduce(self, conv: EdgeConv, x: torch.Tensor, batch: torch.Tensor, seed: Optional[int]):
        N = x.shape[0]
        edge_index = to_undirected(knn_graph(x, self.k, batch, loop=False, flow=conv.flow), num_nodes=N)
        x = conv(x, edge_index)
        weight = normalized_cut_2d(edge_index, x)
        cluster = graclus(edge_index, weight, N, batch=batch, seed=seed)
        return max_pool_x(cluster, x, batch)

    def forward(self, data, seeds: Optional[tuple] = None) -> torch.Tensor:
        """data.x [N, input_dim], data.batch [N] (sorted) -> [B] (output_dim 1) or [B, output_dim].  `seeds`: optional
        (seed1, seed2) for the two graclus calls (default: drawn from torch's CPU generator)."""
        s1, s2 = seeds if seeds is not None else (None, None)
        x = self.datanorm * data.x
        x = self.inputnet(x)
        x, batch = self._reduce(self.edgeconv1, x, data.batch, s1)
        x, batch = self._reduce(self.edgeconv2, x, batch, s2)
        x = global_max_pool(x, batch)
        return self.output(x).squeeze(-1)
