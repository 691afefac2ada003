"""Mirrors of the RecBole pieces the project serves (third_party/recbole): ``layers.AttLayer`` and, in ``context_aware``, the
interaction part of AFM over ``ops.afm_pool``.  RecBole's ``(config, dataset)`` constructors, its ``ContextRecommender`` base
class, trainer and ``calculate_loss`` are not mirrored, and ``compat.install()`` registers nothing under ``recbole.*``."""
from . import context_aware, layers  # noqa: F401
