"""Mirrors of the RecBole pieces the project serves (third_party/recbole): ``layers`` (``AttLayer``, ``MLPLayers``,
``activation_layer``, ``Dice``, ``SequenceAttLayer``); in ``context_aware`` the interaction part of AFM over ``ops.afm_pool``,
that of AutoInt (``AutoIntInteraction``, also exported here) over ``ops.field_attn`` and that of FiGNN (``GraphLayer``,
``FiGNNInteraction``, also exported here) over ``ops.field_attn`` and ``ops.fignn_step``; in ``sequential`` the layers of DIEN
(``AGRUCell``, ``AUGRUCell``, ``DynamicRNN``, ``InterestExtractorNetwork``, ``InterestEvolvingLayer``) over ``ops.att_gru`` /
``ops.gru``, and SR-GNN's ``GNN`` and ``SRGNNEncoder`` (also exported here) over ``ops.session_graph_torch`` and
``ops.session_gnn_step_torch``, and Caser's ``CaserEncoder`` (also exported here, with ``RegLoss``) over ``ops.caser_conv``;
``rechub.models.matching.Caser`` is the trainable Caser.  RecBole's ``(config, dataset)`` constructors, its recommender base classes, ``ContextSeqEmbLayer``, trainer and
``calculate_loss`` are not mirrored, and ``compat.install()`` registers nothing under ``recbole.*``: the trainable models
(``AFM``, ``AutoInt``, ``FiGNN``, ``DIEN``) are registered with the rechub ranking zoo; ``rechub.models.matching.SRGNN`` is the trainable SR-GNN.
In ``general`` the graph collaborative-filtering networks over ``ops.graph_prop`` / ``ops.graph_prop_mean``: ``norm_adj``,
``LightGCNEncoder``, ``BiGNNLayer``, ``NGCFEncoder``, ``BPRLoss`` and ``EmbLoss`` (also exported here);
``rechub.models.matching.LightGCN`` is the trainable LightGCN."""
from . import context_aware, general, layers, sequential  # noqa: F401
from .context_aware import AutoIntInteraction, FiGNNInteraction, GraphLayer  # noqa: F401
from .general import BiGNNLayer, BPRLoss, EmbLoss, LightGCNEncoder, NGCFEncoder, RegLoss, norm_adj  # noqa: F401
from .sequential import GNN, CaserEncoder, SRGNNEncoder  # noqa: F401
