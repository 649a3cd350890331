"""The MLP baselines of the reference -- the GNNs every KAN-GNN table is set beside -- on this package's kernels.

Mirrors ``node_classification_clean/models.py`` (``make_mlp`` :8-17, ``GNN_Nodes`` :94-148),
``graph_classification/models.py`` (``make_mlp`` :9-24, ``GIN`` :26-45, ``GCN`` :47-67, ``GAT`` :69-89) and
``graph_regression/models.py`` (``make_mlp`` :9-24, ``GIN`` :26-54, ``GCN`` :56-80): same constructor arguments, attribute names
and state_dict keys, so a state_dict saved by the reference's baseline loads.  The reference builds them from torch_geometric's
``GINConv`` / ``GINEConv`` / ``GCNConv`` / ``GATConv`` (2.5.3); here the same message-passing shells as the KAN models
(``models._SumAggregateConv`` / ``_NormalisedConv`` / ``_AttentionConv``, ``graph_models.GINEKANLayer``) wrap a dense transform, and the
dense transform is ``ops.linear`` (``csrc/linear.hip``: exact fp32, Linear + ReLU as one call each way).  A KAN row and its MLP row
are therefore measured through the same CSR, aggregation, BatchNorm, loss and loops.

``make_mlp`` is restated quirk for quirk: the last block of a chain of two or more layers is
``nn.Sequential(nn.Linear(hidden_dim, out_dim, nn.ReLU()))`` in the reference -- the module lands in the ``bias`` argument, so that
layer HAS a bias and NO activation -- while a one-layer chain is ``Linear -> ReLU``.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .graph_models import AtomEncoder, BondEncoder, GINEKANLayer, _segment_ptr
from .models import _AttentionConv, _NodeModel, _NormalisedConv, _SumAggregateConv
from .norm import BatchNorm1d


class Linear(nn.Linear):
    """``torch.nn.Linear`` (same parameters, same initialisation, same state_dict keys) computed by ``ops.linear``."""

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return ops.linear(input, self.weight, self.bias)


class LinearReLU(nn.Sequential):
    """The ``nn.Sequential(nn.Linear, nn.ReLU[, nn.BatchNorm1d])`` block of ``make_mlp`` (keys ``0.weight``, ``0.bias``, ``2.*``).  Linear and
    ReLU run as ONE call each way while the first two children still are that pair and carry no hooks (a hook must see the
    tensor between them); anything else runs the plain sequential."""

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if len(self) >= 2 and type(self[0]) is Linear and type(self[1]) is nn.ReLU and ops._hook_free((self[0], self[1])):
            x = ops.linear(input, self[0].weight, self[0].bias, relu=True)
            for m in list(self)[2:]:
                x = m(x)
            return x
        return super().forward(input)


def _make_mlp(num_features, hidden_dim, out_dim, hidden_layers, batch_norm):
    def block(fin, fout):
        if batch_norm:
            return LinearReLU(Linear(fin, fout), nn.ReLU(), BatchNorm1d(fout))
        return LinearReLU(Linear(fin, fout), nn.ReLU())

    if hidden_layers >= 2:
        blocks = [block(num_features, hidden_dim)]
        for _ in range(hidden_layers - 2):
            blocks.append(block(hidden_dim, hidden_dim))
        # the reference: nn.Sequential(nn.Linear(hidden_dim, out_dim, nn.ReLU())) -- the ReLU is the `bias` argument (truthy)
        blocks.append(nn.Sequential(Linear(hidden_dim, out_dim, bias=True)))
    else:
        blocks = [LinearReLU(Linear(num_features, out_dim), nn.ReLU())]     # never a BatchNorm1d here, whatever batch_norm says
    return nn.Sequential(*blocks)


def make_mlp_nodes(num_features, hidden_dim, out_dim, hidden_layers):
    """``make_mlp`` of ``node_classification_clean/models.py:8-17``."""
    return _make_mlp(num_features, hidden_dim, out_dim, hidden_layers, False)


def make_mlp(num_features, hidden_dim, out_dim, hidden_layers, batch_norm=True):
    """``make_mlp`` of the two graph-level files (``graph_classification/models.py:9-24``): ``BatchNorm1d`` after the ReLU of every block
    but the last."""
    return _make_mlp(num_features, hidden_dim, out_dim, hidden_layers, batch_norm)


# ---------------------------------------------------------------------------------- convolutions
class GINConv(_SumAggregateConv):
    """torch_geometric ``GINConv(nn, eps=0., train_eps=False)``: keys ``nn.*``, ``eps``."""

    def __init__(self, nn: nn.Module, eps: float = 0.0):
        super().__init__(nn, eps)


class GINEConv(GINEKANLayer):
    """torch_geometric ``GINEConv(nn, eps=0., train_eps=False)`` without an edge projection (the reference's bond encoder already has
    the node width): ``nn((1 + eps) x_i + sum_j relu(x_j + e_ij))``.  ``GINEKANLayer`` asks the fused KAN node first, which declines
    any net that is not a KAN chain, and then composes ``ops.aggregate_gine`` with the net."""

    def __init__(self, nn: nn.Module, eps: float = 0.0):
        super().__init__(nn, eps)


def _glorot_linear(fin, fout):
    lin = Linear(fin, fout, bias=False)
    nn.init.xavier_uniform_(lin.weight)       # torch_geometric's Linear(weight_initializer='glorot')
    return lin


class GCNConv(_NormalisedConv):
    """torch_geometric ``GCNConv(in_channels, out_channels)`` at its defaults: keys ``lin.weight``, ``bias``."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__(_glorot_linear(in_channels, out_channels), out_channels)
        self.in_channels, self.out_channels = in_channels, out_channels


class GATConv(_AttentionConv):
    """torch_geometric ``GATConv(in_channels, out_channels, heads)`` at its defaults: keys ``lin.weight``, ``att_src``, ``att_dst``,
    ``bias``."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1):
        super().__init__(_glorot_linear(in_channels, heads * out_channels), out_channels, heads)
        self.in_channels = in_channels


# ---------------------------------------------------------------------------------- node classification
class GNN_Nodes(_NodeModel):
    """``node_classification_clean/models.py:94-148``."""

    def __init__(self, conv_type: str, mp_layers: int, num_features: int, hidden_channels: int, num_classes: int,
                 skip: bool = True, hidden_layers: int = 2, dropout: float = 0., heads=4):
        super().__init__()

        def make_conv(width):
            if conv_type == "gcn":
                return GCNConv(width, hidden_channels)
            if conv_type == "gat":
                return GATConv(width, hidden_channels, heads)
            return GINConv(make_mlp_nodes(width, hidden_channels, hidden_channels, hidden_layers))

        dim = self._build(conv_type, mp_layers, num_features, hidden_channels, skip, dropout, make_conv, heads)
        self.lay_out = Linear(dim, num_classes)


# ---------------------------------------------------------------------------------- graph classification
class _Baseline(nn.Module):
    @staticmethod
    def _graph(data, n):
        return ops.batch_graph_index(data, n)

    @staticmethod
    def _pool(x, data, mean=False):
        return ops.segment_pool(x, _segment_ptr(data), mean=mean)


class GIN(_Baseline):
    """``graph_classification/models.py:26-45``: ``dropout(conv(x))`` per layer, add-pool, ``mlp``, ``log_softmax``."""

    def __init__(self, gnn_layers, num_features, hidden_dim, hidden_layers, num_classes, dropout):
        super().__init__()
        self.n_layers = gnn_layers
        self.conv = nn.ModuleList(
            GINConv(make_mlp(num_features if i == 0 else hidden_dim, hidden_dim, hidden_dim, hidden_layers, batch_norm=True))
            for i in range(gnn_layers))
        self.mlp = make_mlp(hidden_dim, hidden_dim, num_classes, hidden_layers, batch_norm=False)
        self.dropout = nn.Dropout(p=dropout)

    def forward(self, data):
        x = data.x
        g = self._graph(data, x.size(0))
        for conv in self.conv:
            x = self.dropout(conv(x, g))
        return F.log_softmax(self.mlp(self._pool(x, data)), dim=1)


class GCN(_Baseline):
    """``graph_classification/models.py:47-67``: ``conv -> SiLU -> dropout``, MEAN pool, ``readout``."""

    def __init__(self, gnn_layers, num_features, hidden_dim, num_classes, dropout):
        super().__init__()
        self.n_layers = gnn_layers
        self.conv = nn.ModuleList(GCNConv(num_features if i == 0 else hidden_dim, hidden_dim) for i in range(gnn_layers))
        self.readout = make_mlp(hidden_dim, hidden_dim, num_classes, 1, batch_norm=False)
        self.dropout = nn.Dropout(p=dropout)

    def forward(self, data):
        x = data.x
        g = self._graph(data, x.size(0))
        for conv in self.conv:
            x = self.dropout(F.silu(conv(x, g)))
        return F.log_softmax(self.readout(self._pool(x, data, mean=True)), dim=1)


class GAT(_Baseline):
    """``graph_classification/models.py:69-89``: the same with add-pool, widths ``hidden_dim * heads``."""

    def __init__(self, gnn_layers, num_features, hidden_dim, num_classes, dropout, heads):
        super().__init__()
        self.n_layers = gnn_layers
        self.conv = nn.ModuleList(GATConv(num_features if i == 0 else hidden_dim * heads, hidden_dim, heads) for i in range(gnn_layers))
        self.readout = make_mlp(hidden_dim * heads, hidden_dim, num_classes, 1, batch_norm=False)
        self.dropout = nn.Dropout(p=dropout)

    def forward(self, data):
        x = data.x
        g = self._graph(data, x.size(0))
        for conv in self.conv:
            x = self.dropout(F.silu(conv(x, g)))
        return F.log_softmax(self.readout(self._pool(x, data)), dim=1)


# ---------------------------------------------------------------------------------- graph regression
class GINRegression(_Baseline):
    """``graph_regression/models.py:26-54`` (class ``GIN`` there): encoders, GINE messages, add-pool, ``mlp``; no ``log_softmax``."""

    def __init__(self, num_node_features, num_edge_features, gnn_layers, hidden_dim, hidden_layers, num_classes, dropout, ogb_encoders):
        super().__init__()
        self.n_layers = gnn_layers
        self.atom_encoder = AtomEncoder(hidden_dim) if ogb_encoders else Linear(num_node_features, hidden_dim)
        self.bond_encoder = BondEncoder(hidden_dim) if ogb_encoders else Linear(num_edge_features, hidden_dim)
        self.conv = nn.ModuleList(GINEConv(make_mlp(hidden_dim, hidden_dim, hidden_dim, hidden_layers, batch_norm=True))
                                  for _ in range(gnn_layers))
        self.mlp = make_mlp(hidden_dim, hidden_dim, num_classes, hidden_layers, batch_norm=False)
        self.dropout = nn.Dropout(p=dropout)

    def forward(self, data):
        x, edge_attr = data.x, data.edge_attr
        if edge_attr.dim() == 1:
            edge_attr = edge_attr.unsqueeze(1)
        x = self.atom_encoder(x)
        edge_attr = self.bond_encoder(edge_attr)
        g = self._graph(data, x.size(0))
        for conv in self.conv:
            x = self.dropout(conv(x, g, edge_attr))
        return self.mlp(self._pool(x, data))


class GCNRegression(_Baseline):
    """``graph_regression/models.py:56-80`` (class ``GCN`` there): encoder, ``conv -> SiLU -> dropout``, ADD pool, ``readout``."""

    def __init__(self, num_node_features, gnn_layers, hidden_dim, num_classes, dropout, ogb_encoders):
        super().__init__()
        self.n_layers = gnn_layers
        self.atom_encoder = AtomEncoder(hidden_dim) if ogb_encoders else Linear(num_node_features, hidden_dim)
        self.conv = nn.ModuleList(GCNConv(hidden_dim, hidden_dim) for _ in range(gnn_layers))
        self.readout = make_mlp(hidden_dim, hidden_dim, num_classes, 1, batch_norm=False)
        self.dropout = nn.Dropout(p=dropout)

    def forward(self, data):
        x = self.atom_encoder(data.x)
        g = self._graph(data, x.size(0))
        for conv in self.conv:
            x = self.dropout(F.silu(conv(x, g)))
        return self.readout(self._pool(x, data))
