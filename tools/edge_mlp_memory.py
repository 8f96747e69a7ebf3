"""Peak-memory growth of one EdgeConv forward + backward for the DRN's edge MLP, fused fp32 route against the generic
route (DMET_EDGE_MLP_F32=0): the graph of tests/test_gpu_edge_mlp_f32.py's memory test (8 x 4 000 nodes, Hin 64, H1 96,
k 32, symmetrised), inputs and module allocated before the measurement.

    python tools/edge_mlp_memory.py [--json OUT]
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deepmetv2_amd as dm  # noqa: E402


def growth(conv, x, ei, g, dev):
    xx = x.detach().clone().requires_grad_(True)
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.max_memory_allocated(dev)
    conv(xx, ei).backward(g)
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(33)
    x = torch.randn(8 * 4000, 64, generator=gen).to(dev)
    batch = torch.repeat_interleave(torch.arange(8), 4000).to(dev)
    ei = dm.to_undirected(dm.knn_graph(x[:, :32].contiguous(), 32, batch, loop=False), num_nodes=x.shape[0])
    E = int(ei.shape[1])
    torch.manual_seed(34)
    nn = torch.nn.Sequential(torch.nn.Linear(128, 96), torch.nn.ELU(), torch.nn.Linear(96, 64), torch.nn.ELU(),
                             torch.nn.BatchNorm1d(64))
    g = torch.randn(x.shape[0], 64, device=dev)
    res = {"E": E, "bound_bytes": E * 64 * 2}
    for route, flag in (("fused", "1"), ("generic", "0")):
        os.environ["DMET_EDGE_MLP_F32"] = flag
        conv = dm.EdgeConv(copy.deepcopy(nn), aggr="add")
        conv.nn.load_state_dict(nn.state_dict())
        conv = conv.to(dev)
        res[route + "_bytes"] = growth(conv, x, ei, g, dev)
        res[route + "_over_bound"] = round(res[route + "_bytes"] / res["bound_bytes"], 3)
        del conv
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
