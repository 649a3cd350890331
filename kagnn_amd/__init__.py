"""kagnn_amd -- MI355X-native KAN-GNN layer hot path (drop-in for RomanBresson/KAGNN's layers).

Host side: Python mirrors of the reference's ``nn.Module`` surface (``ekan``, ``fastkan``,
``models``, ``graph_models``).  Compute: ``libkagnn_hip.so`` (hand-written HIP for gfx950) behind the
C ABI of ``include/kagnn_hip.h``, reached through ``kagnn_amd.ops``.
"""
from . import _lib, ops                                                          # noqa: F401
from .ekan import (KAN, KANLinear, Attribution, EdgeStats, PruneReport, apply_pruning, attribute, collect_edge_l1, prune,   # noqa: F401
                   refine_grids)                             # noqa: F401
from .fastkan import (AttentionWithFastKANTransform, FastKAN, FastKANLayer, RadialBasisFunction,   # noqa: F401
                      SplineLinear)
from .models import (FASTKAGATConv, FASTKAGCNConv, FKANLayer, GFASTKAN_Nodes,        # noqa: F401
                     GIFASTKANLayer, GIKANLayer, GKAN_Nodes, KAGATConv, KAGCNConv, KANLayer, LinkPredictor)

from .norm import BatchNorm1d                                                    # noqa: F401
from .graph_models import (AtomEncoder, BondEncoder, FASTKAGAT, FASTKAGCN, FASTKAGCNRegression, FASTKAGIN, GINEKANLayer,   # noqa: F401
                           KAGAT, KAGCN, KAGCNRegression, KAGIN, KAGINRegression, FASTKAGINRegression,
                           KAGCN_Layer, KAGAT_Layer, FASTKAGCN_Layer, FASTKAGAT_Layer)
from . import baselines                                                          # noqa: F401
from .baselines import (GAT, GCN, GIN, GATConv, GCNConv, GCNRegression, GINConv, GINEConv, GINRegression, GNN_Nodes,   # noqa: F401
                        Linear, LinearReLU, make_mlp, make_mlp_nodes)
from .explain import edge_mask, explain_edges, receptive_hops                    # noqa: F401
from .data import (DeviceBatch, DeviceBatchLoader, DeviceGraphDataset, LinkSplit, NeighborLoader, NodeBatch,   # noqa: F401
                   random_link_split)
from . import symbolic                                                           # noqa: F401
from .symbolic import SYMBOLIC_LIB, SymbolicSuggestion, auto_symbolic, suggest_symbolic         # noqa: F401

__version__ = "0.1.0"
