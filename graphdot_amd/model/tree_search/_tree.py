"""The search tree of `MCTSGraphTransformer`.

A `Tree` is one table of siblings (a `minipandas.DataFrame` with the columns
``parent``, ``children``, ``g``, ``visits`` and whatever the evaluation of the
nodes adds).  The cell ``children[i]`` holds the `Tree` of the offspring of
row `i`, or None for a leaf; ``parent[i]`` holds a view of the row the
siblings hang from, None at the root.  Interface as in the reference
(`iternodes`, `flat`, `str`)."""
from ...minipandas import DataFrame

_LINKS = ('parent', 'children')


class NodeView:
    """Row `i` of `tree` as an object: reading an attribute reads the cell of
    that column, assigning to it writes the cell."""

    def __init__(self, tree, i):
        object.__setattr__(self, 'tree', tree)
        object.__setattr__(self, 'i', i)

    def __getattr__(self, column):
        # (only reached for names that are no instance attributes.  A name
        # that is no column is an AttributeError, so that protocol probes --
        # numpy asks the objects it stores for `__array_struct__` and the
        # like -- get the answer they expect)
        if column in ('tree', 'i') or column not in self.tree:
            raise AttributeError(f'The tree has no column {column!r}.')
        return self.tree[column][self.i]

    def __setattr__(self, column, value):
        self.tree[column][self.i] = value

    def __repr__(self):
        cells = ', '.join(f'{c}={self.tree[c][self.i]!r}'
                          for c in self.tree.columns if c not in _LINKS)
        return f'NodeView({cells})'


class Tree(DataFrame):

    NodeView = NodeView

    def __init__(self, data=None, **columns):
        super().__init__({**(data or {}), **columns})

    def iternodes(self):
        """Views of the rows of this table (not of their offspring)."""
        return (NodeView(self, i) for i in range(len(self)))

    def walk(self):
        """``(level, table, row)`` of every node below and including this
        table's rows, depth first, siblings in order."""
        todo = [(0, self, i) for i in reversed(range(len(self)))]
        while todo:
            level, table, i = todo.pop()
            yield level, table, i
            below = table.children[i]
            if below is not None:
                todo.extend((level + 1, below, j)
                            for j in reversed(range(len(below))))

    @property
    def flat(self):
        """The whole tree as one `DataFrame` in depth-first order: a `level`
        column, then every column but the `parent` / `children` links."""
        payload = [c for c in self.columns if c not in _LINKS]
        cells = {c: [] for c in ['level'] + payload}
        for level, table, i in self.walk():
            cells['level'].append(level)
            for c in payload:
                cells[c].append(table[c][i])
        return DataFrame(cells)

    def __str__(self):
        payload = [c for c in self.columns if c not in _LINKS]
        return '\n'.join(
            '  ' * level + ' '.join(f'{c}:{table[c][i]}' for c in payload)
            for level, table, i in self.walk())
