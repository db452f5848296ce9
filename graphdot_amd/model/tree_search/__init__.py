"""Monte Carlo tree search over graphs (or sequences that a kernel turns into
graphs) towards a target value of the property a surrogate model predicts;
mirrors ``graphdot.model.tree_search`` of the reference."""
from ._rewriter import AbstractRewriter, LookAheadSequenceRewriter
from .graph_transformer import MCTSGraphTransformer

__all__ = ['MCTSGraphTransformer', 'AbstractRewriter',
           'LookAheadSequenceRewriter']
