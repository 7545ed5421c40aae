"""Cost of the optimizer step (tfgnn_optimizer_apply) against torch's foreach Adam, on the variables of two models:
the bench stack (configs[2]: RGCN H=320, 4 layers, 4 edge types, ~1.6 M parameters) and the PPI model (bench.py --workload ppi:
RGCN H=320, 4 layers, 3 edge types + the 121-label head).

Per model and mode: HIP-event time per step of an eager loop, host enqueue time per step (the loop without a sync), and for
the library's entry the event time of the same steps replayed from one captured graph (device time without host gaps).
Modes: the library's Adam with global-norm clipping; torch.optim.Adam(foreach=True) after
torch.nn.utils.clip_grad_norm_(foreach=True) on the same tensors.  (The two do not compute the same numbers - Keras and torch
Adam differ in where epsilon enters - the comparison is of cost only.)

    python tools/optim_probe.py [--steps 50]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def bench_stack_variables():
    from tf2_gnn_amd.layers import GNN, GNNInput
    from bench import model_params

    params = model_params("rgcn", 320, 4)
    gnn = GNN(params)
    gnn.build(GNNInput(node_features=(None, 320), adjacency_lists=tuple((None, 2) for _ in range(4)), node_to_graph_map=(None,),
                       num_graphs=()))
    return gnn.trainable_variables


def ppi_variables():
    from bench import ppi_rgcn_params
    from tf2_gnn_amd.tasks import NodeMulticlassTask

    p = NodeMulticlassTask.get_default_hyperparameters("rgcn")
    p.update({f"gnn_{k}": v for k, v in ppi_rgcn_params(320, 4).items()})
    model = NodeMulticlassTask(p, num_edge_types=3, num_node_target_labels=121)
    model.build({"node_features": (None, 50)})
    return model.trainable_variables


def timed(fn, steps):
    """(event ms per step, host enqueue us per step)"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    host = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, host / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    from tf2_gnn_amd import _lib
    from tf2_gnn_amd.optim import Optimizer

    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(dev)}; {args.steps} steps per measurement")
    for name, make in (("bench stack (configs[2])", bench_stack_variables), ("ppi model", ppi_variables)):
        vars_ = make()
        gen = torch.Generator().manual_seed(0)
        grads = [(torch.randn(v.shape, generator=gen) * 1e-3).to(dev) for v in vars_]
        n = sum(v.value.numel() for v in vars_)
        mb = n * 4 * 7 / 1e6  # Adam: reads w, g, m, v and writes w, m, v
        print(f"\n{name}: {len(vars_)} tensors, {n} parameters, Adam moves {mb:.1f} MB per step")

        opt = Optimizer("adam", learning_rate=1e-4)
        pairs = list(zip(vars_, grads))
        c0 = _lib.load().tfgnn_optimizer_launch_count()
        opt.apply_gradients(pairs, clip=("global_norm", 1.0))
        launches = _lib.load().tfgnn_optimizer_launch_count() - c0
        ms, us = timed(lambda: opt.apply_gradients(pairs, clip=("global_norm", 1.0)), args.steps)
        print(f"  tfgnn_optimizer_apply  Adam + global norm: {launches} launches; eager {ms * 1e3:8.1f} us/step (events), "
              f"host enqueue {us:7.1f} us/step")
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for _ in range(args.steps):
                    opt.apply_gradients(pairs, clip=("global_norm", 1.0))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        dms = a.elapsed_time(b) / args.steps
        print(f"  tfgnn_optimizer_apply  replayed from one graph: {dms * 1e3:8.1f} us/step  ({mb / 1e6 / (dms / 1e3):.2f} TB/s)")

        params = [v.value for v in vars_]
        for p, gr in zip(params, grads):
            p.grad = gr
        topt = torch.optim.Adam(params, lr=1e-4, foreach=True)

        def torch_step():
            torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
            topt.step()

        ms_t, us_t = timed(torch_step, args.steps)
        print(f"  torch foreach Adam + clip_grad_norm_:        eager {ms_t * 1e3:8.1f} us/step (events), host enqueue {us_t:7.1f} us/step")
        for p in params:
            p.grad = None


if __name__ == "__main__":
    main()
