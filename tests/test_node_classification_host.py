"""Host-side checks of the node-classification experiment (no GPU): the new entry points are declared, exported and bound; the
split-bits byte is what its numpy restatement says; CPU tensors are refused with the package's message instead of computed on."""
import os
import re

import numpy as np
import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, harness, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kagnn_node_eval_workspace_bytes", "kagnn_node_eval", "kagnn_early_stop_update", "kagnn_copy_if")
NO_CPU = "There is no CPU fallback in this package"


def test_new_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kagnn_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/kagnn_hip.h"
        assert name in _lib.EXPORTED and name in _lib._SIGNATURES
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.kagnn_version() >= 265
    assert "nodeclass.hip" in __import__("kagnn_amd._build", fromlist=["SOURCES"]).SOURCES
    for name in ("split_bits", "node_eval", "EarlyStop", "copy_if"):
        assert hasattr(ops, name)
    for name in ("train_node_classification", "node_classification_splits", "NodeClassificationResult"):
        assert hasattr(harness, name)


def test_split_bits_equals_the_numpy_restatement():
    rng = np.random.default_rng(0)
    for n, k in ((1, 1), (37, 3), (1000, 8), (0, 2)):
        masks = rng.random((k, n)) < 0.4
        if k >= 3 and n:
            masks[2] = masks[0] | masks[1]                                  # overlapping on purpose
        want = np.zeros(n, dtype=np.uint8)
        for s in range(k):
            want |= (masks[s].astype(np.uint8) << s).astype(np.uint8)
        got = ops.split_bits(*[torch.from_numpy(m) for m in masks])
        assert got.dtype == torch.uint8 and got.shape == (n,) and np.array_equal(got.numpy(), want)
        buf = torch.full((n,), 255, dtype=torch.uint8)
        assert ops.split_bits(*[torch.from_numpy(m) for m in masks], out=buf) is buf and np.array_equal(buf.numpy(), want)
    m = torch.tensor([True, False, True])
    assert ops.split_bits(m, m).tolist() == [3, 0, 3]                        # test_mask=None: the validation mask twice


def test_split_bits_refuses_too_many_masks_and_mismatched_lengths():
    m = torch.zeros(5, dtype=torch.bool)
    with pytest.raises(ValueError, match="1 to 8"):
        ops.split_bits(*([m] * 9))
    with pytest.raises(ValueError, match="1 to 8"):
        ops.split_bits()
    with pytest.raises(ValueError, match="one length"):
        ops.split_bits(m, torch.zeros(6, dtype=torch.bool))
    with pytest.raises(TypeError):
        ops.split_bits(m, torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.split_bits(m, out=torch.zeros(4, dtype=torch.uint8))


def test_cpu_tensors_are_refused():
    z, y, bits = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=NO_CPU):
        ops.node_eval(z, y, bits, 3)
    with pytest.raises(RuntimeError, match=NO_CPU):
        ops.EarlyStop(5, device="cpu")
    with pytest.raises(RuntimeError, match=NO_CPU):
        ops.copy_if(torch.ones(1, dtype=torch.int32), [torch.zeros(4)], [torch.ones(4)])
    model = kagnn_amd.GKAN_Nodes("gin", 1, 3, 4, 2)
    mask = torch.ones(4, dtype=torch.bool)
    with pytest.raises(RuntimeError, match=NO_CPU):
        harness.train_node_classification(model, z, torch.zeros(2, 0, dtype=torch.int64), y, mask, mask, epochs=1)
    with pytest.raises(RuntimeError, match=NO_CPU):
        harness.node_classification_splits({}, z, torch.zeros(2, 0, dtype=torch.int64), y, mask[None], mask[None], mask[None])
    with pytest.raises(ValueError, match="metrics_at"):
        harness.train_node_classification(model, z, torch.zeros(2, 0, dtype=torch.int64), y, mask, mask, metrics_at="final")
