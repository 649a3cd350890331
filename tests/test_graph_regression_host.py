"""Host-side checks of the graph-regression experiment (no GPU): ``random_split_ids`` draws what ``torch.utils.data.random_split``
draws; the new entry points are declared, exported and bound; CPU tensors are refused with the package's message instead of
computed on."""
import os
import re
import warnings

import pytest
import torch
from torch.utils.data import random_split

import kagnn_amd
from kagnn_amd import _lib, data, harness, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kagnn_l1_loss_meter_fwd", "kagnn_regression_epoch_update")
NO_CPU = "There is no CPU fallback in this package"


@pytest.mark.parametrize("n", [1, 10, 133885])
def test_random_split_ids_equals_torch_random_split_for_fractions(n):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (n = 1: torch warns about its two empty splits)
        want = random_split(range(n), [0.8, 0.1, 0.1], torch.Generator().manual_seed(n))
    got = data.random_split_ids(n, [0.8, 0.1, 0.1], torch.Generator().manual_seed(n))
    assert len(got) == 3 and sum(g.numel() for g in got) == n
    for w, g in zip(want, got):
        assert g.dtype == torch.int64 and not g.is_cuda and g.tolist() == list(w.indices)
    if n == 133885:                                                      # floors 107108 / 13388 / 13388; the one graph left over goes to split 0
        assert [g.numel() for g in got] == [107109, 13388, 13388]


def test_random_split_ids_equals_torch_random_split_for_lengths_and_the_default_generator():
    for n, lengths in ((10, [3, 7]), (133885, [110000, 10000, 13885]), (5, [5]), (6, [0, 6])):
        want = random_split(range(n), lengths, torch.Generator().manual_seed(7))
        got = data.random_split_ids(n, lengths, torch.Generator().manual_seed(7))
        assert [g.tolist() for g in got] == [list(w.indices) for w in want]
    torch.manual_seed(11)
    want = random_split(range(40), [0.5, 0.5])
    torch.manual_seed(11)
    got = data.random_split_ids(40, [0.5, 0.5])
    assert [g.tolist() for g in got] == [list(w.indices) for w in want]
    # the generator is advanced exactly as random_split advances it: the next draw agrees too
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    random_split(range(9), [4, 5], ga)
    data.random_split_ids(9, [4, 5], gb)
    assert torch.equal(torch.randperm(9, generator=ga), torch.randperm(9, generator=gb))
    with pytest.raises(ValueError, match="add up"):
        data.random_split_ids(10, [3, 6])
    with pytest.raises(ValueError):
        data.random_split_ids(10, [1.5, -0.5])


def test_new_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kagnn_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/kagnn_hip.h"
        assert name in _lib.EXPORTED and name in _lib._SIGNATURES
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert re.search(r"#define\s+KAGNN_REGRESSION_MAX_TARGETS\s+32\b", header) and _lib.REGRESSION_MAX_TARGETS == 32
    assert lib.kagnn_version() >= 266
    assert "regress.hip" in __import__("kagnn_amd._build", fromlist=["SOURCES"]).SOURCES
    for name in ("RegressionMeter", "RegressionStop", "RegressionStopState", "l1_loss"):
        assert hasattr(ops, name)
    for name in ("train_graph_regression", "evaluate_graph_regression", "GraphRegressionResult"):
        assert hasattr(harness, name)
    assert hasattr(data, "random_split_ids") and hasattr(data.DeviceGraphDataset, "standardize_targets")


def test_argument_checks_need_no_gpu():
    """the entry points validate before they launch: a 33rd target, a missing record, a misaligned record"""
    lib = _lib.load()
    buf = (torch.zeros(64, dtype=torch.int64)).data_ptr()                # (never dereferenced: every call below is refused)
    assert lib.kagnn_l1_loss_meter_fwd(buf, 33, buf, 33, 4, 33, None, buf, None, None) != 0
    assert b"targets" in lib.kagnn_last_error()
    assert lib.kagnn_l1_loss_meter_fwd(buf, 0, buf, 0, 4, 0, None, buf, None, None) != 0
    assert lib.kagnn_l1_loss_meter_fwd(buf, 2, buf, 4, 4, 4, None, buf, None, None) != 0      # ldp < targets
    assert lib.kagnn_l1_loss_meter_fwd(buf, 4, buf, 4, 4, 4, None, None, None, None) != 0      # neither a loss nor a record
    assert lib.kagnn_l1_loss_meter_fwd(buf, 4, buf, 4, 4, 4, None, buf, buf + 4, None) != 0    # record not 8-byte aligned
    assert lib.kagnn_regression_epoch_update(None, buf, None, 1, 1, 1, buf, None, 4, None) != 0
    assert lib.kagnn_regression_epoch_update(buf, buf, None, 1, 1, 1, None, None, 4, None) != 0
    assert lib.kagnn_regression_epoch_update(buf, buf + 4, None, 1, 1, 1, buf, None, 4, None) != 0
    assert lib.kagnn_regression_epoch_update(buf, buf, None, 1, 1, 1, buf, None, -1, None) != 0


def test_cpu_tensors_are_refused():
    p, t = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(RuntimeError, match=NO_CPU):
        ops.RegressionMeter(3, device="cpu")
    with pytest.raises(RuntimeError, match=NO_CPU):
        ops.RegressionStop(5, device="cpu")
    with pytest.raises(RuntimeError, match=NO_CPU):
        ops.l1_loss(p, t, scale=torch.ones(3))
    with pytest.raises(RuntimeError, match=NO_CPU):
        ops.l1_loss(p, t)                                                # (the plain path, as before)
    with pytest.raises(ValueError, match="same shape"):
        ops.l1_loss(p, t[:, :2], scale=torch.ones(3))
    model = kagnn_amd.KAGCNRegression(2, 1, 4, 4, 3, 1, 0.0)
    with pytest.raises(RuntimeError, match=NO_CPU):
        harness.train_graph_regression(model, [], [], epochs=1)
    with pytest.raises(RuntimeError, match=NO_CPU):
        harness.evaluate_graph_regression(model, [])
