"""Rewrite rules for the tree search.

`LookAheadSequenceRewriter` has the interface and the behaviour of the
reference's class of that name; how it gets there is this module's own.  The
n-gram statistics are a table ``gram (tuple of symbols) -> count`` filled in
one pass over the training sequences; `NGramTree` presents that table as a
tree whose node identifiers ARE the grams, so that looking a context up is a
dictionary access and the parent of a node is its gram without the last
symbol.  It offers the part of treelib's interface that users of the
reference touch: ``root``, ``nodes``, ``tree[id]``, ``children(id)`` in
order of first occurrence, ``parent(id)``, ``show()``, nodes with ``tag``,
``identifier``, ``data.count`` and ``data.freq``.
"""
from abc import ABC, abstractmethod
from types import SimpleNamespace
import numpy as np


class AbstractRewriter(ABC):
    """What the tree search expects of a rewriter: a callable that turns one
    graph into a list of derived graphs."""

    @abstractmethod
    def __call__(self, g, random_state=None):
        """Derive new graphs from `g`.

        g: the graph, or the node of a search tree that holds it as ``g.g``.
        random_state: the `np.random.Generator` to draw from, if any.
        Returns a list of graphs.
        """


class NGramNode:
    __slots__ = ('tag', 'identifier', 'data')

    def __init__(self, gram, count):
        self.identifier = gram
        self.tag = gram[-1] if gram else '$'
        self.data = SimpleNamespace(count=count, freq=0)

    def __repr__(self):
        return (f'NGramNode({self.identifier!r}, count={self.data.count}, '
                f'freq={self.data.freq:.4g})')


class NGramTree:
    """The counted grams of a training set as a tree.  The identifier of a
    node is its gram, the root is the empty gram ``()``."""

    root = ()

    def __init__(self, counts):
        """counts: {gram: count} in which every gram comes after its prefix
        (`LookAheadSequenceRewriter.fit` counts them in that order)."""
        self.nodes = {(): NGramNode((), 0)}
        self._kids = {(): []}
        for gram, count in counts.items():
            self.nodes[gram] = NGramNode(gram, count)
            self._kids[gram] = []
            self._kids[gram[:-1]].append(gram)
        for kids in self._kids.values():
            total = sum(counts[g] for g in kids)
            for g in kids:
                self.nodes[g].data.freq = counts[g] / total

    def __getitem__(self, identifier):
        return self.nodes[identifier]

    def __contains__(self, identifier):
        return identifier in self.nodes

    def __len__(self):
        return len(self.nodes)

    def children(self, identifier):
        return [self.nodes[g] for g in self._kids[identifier]]

    def parent(self, identifier):
        return self.nodes[identifier[:-1]] if identifier else None

    def depth(self, identifier):
        return len(identifier)

    def show(self, file=None):
        """Print one line per node, children under their parent."""
        lines, todo = [], [()]
        while todo:
            gram = todo.pop()
            node = self.nodes[gram]
            lines.append(f'{"    " * len(gram)}{node.tag} '
                         f'[count={node.data.count} '
                         f'freq={node.data.freq:.4g}]')
            todo.extend(reversed(self._kids[gram]))
        text = '\n'.join(lines)
        print(text, file=file)
        return text


def _generator(random_state):
    # (an int seeds PCG64, a Generator is passed through, None is entropy)
    return np.random.default_rng(random_state)


class LookAheadSequenceRewriter(AbstractRewriter):
    """Random edits of a symbol sequence that respect the n-gram statistics
    of a training set.

    An edit is an insertion, a mutation or a deletion at a uniformly drawn
    position.  Inserted and substituted symbols are drawn from the symbols
    that followed, in the training set, the up to `n` symbols in front of the
    position; if that context never occurred (or has no successor) the
    longest suffix of it that did is used, down to the empty context, i.e.
    the plain symbol frequencies.  Deletions ignore the context.

    Parameters
    ----------
    n: int
        Length of the longest context.
    b: int
        Branching factor: offspring to attempt per call.
    min_edits, max_edits: int
        An offspring is accepted after at least `min_edits` edits, as soon
        as it is new; it is given up after `max_edits` edits.
    p_insert, p_mutate, p_delete: float
        Relative frequencies of the three kinds of edit.
    random_state: np.random.Generator or int
        The internal generator (or its seed).
    """

    def __init__(self, n=1, b=3, min_edits=1, max_edits=5, p_insert=1,
                 p_mutate=1, p_delete=1, random_state=None):
        self.n, self.b = n, b
        self.min_edits, self.max_edits = min_edits, max_edits
        weights = np.asarray((p_insert, p_mutate, p_delete), dtype=float)
        self.edit_probabilities = weights / weights.sum()
        self.rng = _generator(random_state)

    # -- the statistics --------------------------------------------------------
    def fit(self, X):
        """Count the 1- to (n+1)-grams of the sequences in `X`."""
        counts = {}
        for seq in X:
            seq = tuple(seq)
            for end in range(1, len(seq) + 1):
                # shortest first: every gram is counted after its prefix,
                # which ended one symbol earlier
                for length in range(1, min(self.n + 1, end) + 1):
                    gram = seq[end - length:end]
                    counts[gram] = counts.get(gram, 0) + 1
        self._tree = NGramTree(counts)
        return self

    @property
    def tree(self):
        """The n-gram statistics as an `NGramTree`: the children of the node
        of a context are the symbols seen after it."""
        if not hasattr(self, '_tree'):
            raise RuntimeError('No n-gram statistics yet: call fit() with a '
                               'collection of sequences first.')
        return self._tree

    @staticmethod
    def _match_context(tree, s, k, n):
        """The node of the longest context of at most `n` symbols in front of
        position `k` of `s` that occurred in training and has successors;
        None if not even the root has any."""
        for length in range(min(n, k), -1, -1):
            gram = tuple(s[k - length:k])
            if gram in tree and tree.children(gram):
                return tree[gram]
        return None

    def _propose(self, s, k, rng=None):
        """A symbol for position `k` of `s`, drawn by its context."""
        rng = self.rng if rng is None else rng
        successors = self.tree.children(
            self._match_context(self.tree, s, k, self.n).identifier)
        pick = rng.choice(len(successors),
                          p=[c.data.freq for c in successors])
        return successors[pick].tag

    # -- edits ------------------------------------------------------------------
    @staticmethod
    def _spliced(s, k, removed, symbols):
        """`s` with `removed` items from position `k` on replaced by
        `symbols`, as a sequence of the type of `s`."""
        middle = ''.join(map(str, symbols)) if isinstance(s, str) \
            else type(s)(symbols)
        return s[:k] + middle + s[k + removed:]

    def _insert(self, s, k, rng=None):
        return self._spliced(s, k, 0, [self._propose(s, k, rng)])

    def _mutate(self, s, k, rng=None):
        return self._spliced(s, k, 1, [self._propose(s, k, rng)])

    def _delete(self, s, k, rng=None):
        return self._spliced(s, k, 1, [])

    def _rewrite(self, s, rng=None):
        """`s` after one random edit."""
        rng = self.rng if rng is None else rng
        edit = (self._insert, self._mutate, self._delete)[
            rng.choice(3, p=self.edit_probabilities)]
        return edit(s, int(rng.integers(len(s))), rng)

    def __call__(self, s, random_state=None):
        """Up to `b` distinct offspring of `s`, none equal to `s`, in the
        order they were made.

        s: a sequence, or a node of a search tree (then ``s.g`` is edited).
        random_state: a generator to draw from instead of the internal one.
        """
        from ._tree import NodeView
        if isinstance(s, NodeView):
            s = s.g
        rng = self.rng if random_state is None else random_state
        taken, offspring = {s}, []
        for _ in range(self.b):
            candidate = s
            for done in range(1, self.max_edits + 1):
                candidate = self._rewrite(candidate, rng)
                if done >= self.min_edits and candidate not in taken:
                    taken.add(candidate)
                    offspring.append(candidate)
                    break
        return offspring
