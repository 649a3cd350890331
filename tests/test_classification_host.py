"""The host side of the graph-classification workflow (no GPU): ``kagnn_amd.data.read_splits`` on the reference's split-file format
(``graph_classification/graph_classification_utils.py:88-91,103-124``), and the refusals -- ``ops.nll_loss``, ``ops.degree_one_hot``,
``ops.ClassificationMeter`` and a degree-featured ``DeviceGraphDataset`` raise the package's "no CPU fallback" error on CPU tensors and
emulate nothing."""
import json

import pytest
import torch

import kagnn_amd
from kagnn_amd import data, harness, ops

FOLDS = [
    {"test": [0, 5, 9], "model_selection": [{"train": [1, 2, 3, 4, 5], "validation": [5, 6]}]},          # 5 in all three lists
    {"test": [], "model_selection": [{"train": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9], "validation": []}]},       # empty lists
    {"test": [3], "model_selection": [{"train": [9, 9, 0], "validation": [3, 4, 3]}, {"train": [7], "validation": [8]}]},
]


def test_read_splits_round_trips_the_reference_format(tmp_path):
    path = tmp_path / "IMDB-BINARY_splits.json"
    path.write_text(json.dumps(FOLDS))                      # one line, as the reference's files are
    got = data.read_splits(str(path))
    assert isinstance(got, list) and len(got) == 3
    for fold, (train, val, test) in zip(FOLDS, got):
        for t, want in ((train, fold["model_selection"][0]["train"]), (val, fold["model_selection"][0]["validation"]), (test, fold["test"])):
            assert t.dtype == torch.int64 and t.dim() == 1 and not t.is_cuda
            assert t.tolist() == want
    # what comes back serialises to the file's own content (the first model_selection entry is the one the reference uses)
    again = [{"test": te.tolist(), "model_selection": [{"train": tr.tolist(), "validation": va.tolist()}]} for tr, va, te in got]
    assert again == [{"test": f["test"], "model_selection": f["model_selection"][:1]} for f in FOLDS]
    # a trailing newline and a pathlib path are fine; the tensors index a dataset view's positions
    path.write_text(json.dumps(FOLDS) + "\n")
    assert [t.tolist() for t in data.read_splits(path)[2]] == [[9, 9, 0], [3, 4, 3], [3]]
    assert data._normalise_index(got[0][0], 10).tolist() == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("content,what", [
    ("", "empty file"),
    ("this is not json", "not JSON"),
    (json.dumps({"test": [1]}), "a dict, not a list of folds"),
    (json.dumps([]), "no folds"),
    (json.dumps([{"test": [1]}]), "no model_selection"),
    (json.dumps([{"test": [1], "model_selection": []}]), "empty model_selection"),
    (json.dumps([{"test": [1], "model_selection": [{"train": [0]}]}]), "no validation"),
    (json.dumps([{"test": [1.5], "model_selection": [{"train": [0], "validation": [2]}]}]), "a fractional index"),
    (json.dumps([{"test": [-1], "model_selection": [{"train": [0], "validation": [2]}]}]), "a negative index"),
    (json.dumps([{"test": "1,2", "model_selection": [{"train": [0], "validation": [2]}]}]), "a string for a list"),
])
def test_read_splits_says_what_is_wrong(tmp_path, content, what):
    path = tmp_path / "bad.json"
    path.write_text(content)
    with pytest.raises(ValueError, match="bad.json"):
        data.read_splits(str(path))
    with pytest.raises(OSError):
        data.read_splits(str(tmp_path / "missing.json"))


def test_nll_loss_refuses_cpu_tensors():
    logp = torch.log_softmax(torch.randn(4, 3), 1)
    y = torch.tensor([0, 2, 1, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nll_loss(logp, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nll_loss(logp, y, reduction="sum")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ClassificationMeter("cpu")


def test_nll_loss_reduction_none_is_a_value_error():
    logp = torch.log_softmax(torch.randn(4, 3), 1)
    with pytest.raises(ValueError, match="reduction"):
        ops.nll_loss(logp, torch.tensor([0, 2, 1, 1]), reduction="none")


def test_degree_one_hot_refuses_cpu_tensors():
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.degree_one_hot(ei, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.degree_one_hot(ei[:, :0], 3, num_classes=5)


def test_degree_featured_dataset_refuses_the_cpu():
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.DeviceGraphDataset(None, ei, [0, 3], y=torch.tensor([1]), device="cpu", degree_features=36)
    from types import SimpleNamespace
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.DeviceGraphDataset.from_graphs([SimpleNamespace(x=None, num_nodes=3, edge_index=ei, y=torch.tensor([1]))], device="cpu",
                                                 degree_features=36)


def test_the_classification_loops_refuse_a_cpu_model():
    m = torch.nn.Linear(3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        harness.evaluate_graph_classification(m, [])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        harness.train_graph_classification(m, [])
