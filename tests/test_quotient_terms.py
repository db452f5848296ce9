"""The `terms` section of quotient arenas (GraphArena):
one 16-byte record per directed nonzero of a quotient image -- what the
quotient solver needs of a half-term of a slot (mgk_oc.h RECS) -- written by
`gdh_assemble_arena` and restated in numpy; arenas of full images keep their
layout."""
import networkx as nx
import numpy as np
import pytest

import cases
from graphdot_amd.graph import Graph
from graphdot_amd.kernel.marginalized._devicegraph import (
    _ALIGN, HEADER_DTYPE, SECTIONS, TERM_DTYPE, GraphArena, class_bytes,
    pack_many, quotient_graph, term_bytes)
from test_quotient import _atom, _bond, hand_built, molecule


def weighted_tree():
    """A small weighted tree: two leaves of equal weight on one node (a twin
    group), weights that float32 holds exactly and one that it does not."""
    g = nx.Graph()
    for v in range(6):
        g.add_node(v, category=1 + int(v in (0, 3)))
    for u, v, w, length in ((0, 1, 0.75, 1.0), (0, 2, 0.75, 1.0),
                            (0, 3, 2.0, 2.0), (3, 4, 0.1, 1.0),
                            (3, 5, 1.5, 2.0)):
        g.add_edge(u, v, w=w, length=length)
    return [Graph.from_networkx(g, weight='w')]


def graph_sets():
    """name -> graphs of one type"""
    hand = [Graph.from_networkx(g) for g, _, _ in hand_built().values()]
    atom = nx.Graph()
    _atom(atom, 0, 6)
    _bond(atom, 0, 0)      # (a graph needs an edge: the node's self loop)
    extra = [Graph.from_networkx(g) for g in (
        molecule([6], [], [4]),                                   # methane
        molecule([6, 8, 6, 7], [(0, 1, 2), (0, 2, 1), (2, 3, 3)], [0] * 4),
        atom,                                                     # one node
        hand_built()['h2'][0])]
    return {
        'molecules': Graph.unify_datatype(
            hand + cases.config3_graphs(30) + extra),
        'weighted': weighted_tree(),
    }


@pytest.fixture(scope='module', params=['molecules', 'weighted'])
def images(request):
    """(full images, quotient images) in double"""
    dgs = pack_many(graph_sets()[request.param], real=np.float64)
    return dgs, [quotient_graph(dg) for dg in dgs]


def test_record_layout():
    assert TERM_DTYPE.itemsize == 16 == _ALIGN
    assert [TERM_DTYPE.fields[f][1] for f in ('qw', 'w', 'j', 'cls', 'pad')] \
        == [0, 8, 12, 14, 15]
    assert term_bytes(np.array([0, 5])).tolist() == [0, 80]


def test_native_arena_is_the_numpy_one(images):
    for dgs in images:
        a = GraphArena(dgs, classes=True, native=True)
        b = GraphArena(dgs, classes=True, native=False)
        assert a.nbytes == b.nbytes
        assert np.array_equal(a.blob_start, b.blob_start)
        assert np.array_equal(a.term_bytes, b.term_bytes)
        assert np.array_equal(a._hdr, b._hdr)
        assert np.array_equal(a.host, b.host)


def test_every_record_is_its_definition(images):
    dgs, qs = images
    arena = GraphArena(qs, classes=True)
    assert np.array_equal(arena.term_bytes, 16 * arena.n_nz)
    assert sum(q.n_merged for q in qs) > 0
    edge_t = np.dtype(qs[0].edge_t)
    at = arena.blob_start - arena.class_bytes - arena.term_bytes
    assert np.all(at % 16 == 0)
    # the sections tile the arena: [terms][classes][blob] graph after graph
    assert np.array_equal(
        at[1:], (arena.blob_start + [len(q.blob) for q in qs])[:-1])
    for k, q in enumerate(qs):
        rec = arena.host[at[k]:at[k] + 16 * q.n_nz].view(TERM_DTYPE)
        zi, zj = q.nz['i'].astype(np.int64), q.nz['j'].astype(np.int64)
        want = q.scale[zi] * q.scale[zj]
        assert want.dtype == np.float64
        assert np.array_equal(rec['qw'].view(np.uint64), want.view(np.uint64))
        assert np.array_equal(rec['j'], q.nz['j'])
        assert not rec['pad'].any()
        # the class ids are those of the class section behind the records
        c0 = arena.blob_start[k] - arena.class_bytes[k]
        ecls = arena.host[c0 + (q.n_node + 3) // 4 * 4:][:q.n_nz]
        assert np.array_equal(rec['cls'], ecls)
        if q.weighted:
            o = q.offsets['edge']
            w = q.blob[o:o + q.n_nz * edge_t.itemsize].view(edge_t)['weight']
            assert np.array_equal(rec['w'], w.astype(np.float32))
            assert len(set(w.tolist())) > 1
        else:
            assert np.all(rec['w'] == 1)


def test_edge_classes_of_the_records_tell_the_labels_apart(images):
    _, qs = images
    arena = GraphArena(qs, classes=True)
    at = arena.blob_start - arena.class_bytes - arena.term_bytes
    cls = np.concatenate([
        arena.host[at[k]:at[k] + 16 * q.n_nz].view(TERM_DTYPE)['cls']
        for k, q in enumerate(qs)])
    assert cls.max() == arena.classes['ne'] - 1 and arena.classes['ne'] > 1


def test_terms_only_with_quotient_images_and_numbered_labels(images):
    dgs, qs = images
    for arena in (GraphArena(qs, classes=False), GraphArena(qs, terms=False),
                  GraphArena(dgs, classes=True)):
        assert not arena.term_bytes.any()


@pytest.mark.parametrize('native', [True, False])
@pytest.mark.parametrize('classes', [True, False])
def test_arenas_of_full_images_keep_their_layout(images, native, classes):
    """[headers][class representatives]([classes g][blob g])...: sizes and
    section offsets restated from the blobs and `class_bytes` alone."""
    dgs, _ = images
    arena = GraphArena(dgs, classes=classes, native=native)

    def pad(n):
        return (n + 15) // 16 * 16
    cursor = pad(len(dgs) * HEADER_DTYPE.itemsize)
    if classes:
        c = arena.classes
        assert c['vrep'] == cursor
        cursor = c['erep'] + pad(c['ne'] * np.dtype(dgs[0].edge_t).itemsize)
    for k, g in enumerate(dgs):
        cursor += int(class_bytes(g.n_node, g.n_nz))
        assert arena.blob_start[k] == cursor
        for name in SECTIONS:
            assert arena._hdr[name][k] == cursor + g.offsets[name]
        assert np.array_equal(arena.host[cursor:cursor + len(g.blob)], g.blob)
        cursor += len(g.blob)
    assert arena.nbytes == cursor
    assert np.array_equal(arena.host,
                          GraphArena(dgs, classes=classes, native=native,
                                     terms=False).host)
