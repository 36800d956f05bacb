"""Writes tests/golden/edge_predictor_reference.npz: what the reference's EdgePredictor(12)
(gnnflow/models/modules/layers.py, loaded by file path) computes on the CPU with a fixed seed.

    state.<name>   its state_dict
    h              the input, [21, 12] = 7 source, 7 positive and 7 negative rows
    pos, neg       its two outputs
    grad.h, grad.<name>   the gradients of pos.sum() - 2 * neg.sum()

    python tests/golden/make_edge_predictor_fixture.py /path/to/GNNFlow
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

DIM, ROWS, SEED = 12, 21, 1234


def main(ref_root):
    from gnnflow_amd import dgl_compat
    dgl_compat.install()
    spec = importlib.util.spec_from_file_location(
        "_ref_layers", os.path.join(ref_root, "gnnflow", "models", "modules", "layers.py"))
    layers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(layers)
    torch.manual_seed(SEED)
    model = layers.EdgePredictor(DIM)
    h = torch.randn(ROWS, DIM, requires_grad=True)
    pos, neg = model(h)
    (pos.sum() - 2 * neg.sum()).backward()
    out = {"h": h.detach().numpy(), "pos": pos.detach().numpy(), "neg": neg.detach().numpy(),
           "grad.h": h.grad.numpy()}
    for k, v in model.state_dict().items():
        out["state." + k] = v.numpy()
    for k, v in model.named_parameters():
        out["grad." + k] = v.grad.numpy()
    np.savez(os.path.join(HERE, "edge_predictor_reference.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
