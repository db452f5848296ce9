// Device image of one graph, as packed by kernel/marginalized/_devicegraph.py.
//
// The reference stores adjacency as compact 8x8 "octiles" + 64-bit masks
// (graphdot/cpp/graph.h:8-33) because its solver walks tile pairs with
// 32-lane half-tiles and scatters with float atomics.  The MI355X solver is
// atomic-free: it needs, per graph, plain CSR of the *directed* nonzeros with
// the nodes renumbered by descending adjacency count, so that any run of
// consecutive rows (tasks) handled by one wave instruction has near-equal
// trip counts and the wave-uniform maximum is known from its first row.
//
// The solver copies the packed image of each graph of a pair into LDS (the
// image [degree .. perm] is contiguous) and builds its view on that copy.
// All graphs of a call live in one arena allocation; a header stores byte
// offsets from the arena base (which is a kernel argument, so the compiler
// knows every derived pointer is in global memory and emits global_load /
// s_load rather than flat_load).
#ifndef GRAPHDOT_HIP_GRAPH_H_
#define GRAPHDOT_HIP_GRAPH_H_
#include <cstdint>

namespace graphdot {

struct nz_t {            // one directed nonzero of the adjacency matrix
    std::uint16_t i, j;  // row (source), column (target), new numbering
};

struct graph_header_t {  // 64 bytes, see _devicegraph.HEADER_DTYPE
    // (quotient images, _devicegraph.quotient_graph: the node count of the
    // quotient in the low half, that of the full graph in the high half --
    // both fit 16 bits; full images leave the high half 0)
    std::int32_t n_node;
    std::int32_t n_nz;   // directed nonzeros (self loop counted once)
    std::uint32_t degree, node, rowptr, nz, edge, perm;  // byte offsets
    // nodes per adjacency count 0..14 (hist[15]: 15 and above).  Nodes are
    // stored by descending count, so this is all the owner-computes solver
    // needs to lay out its degree-pair rectangles (mgk_oc.h) -- read with the
    // header into scalar registers instead of counted per pair with ballots.
    std::uint16_t hist[16];
};

template<class Node, class Edge> struct graph_t {
    using node_t = Node;
    using edge_t = Edge;
    int n_node, n_nz;
    float const *degree;           // [n_node] sum of incident weights, 0 -> 1
    node_t const *node;            // [n_node] AoS node labels
    std::uint16_t const *rowptr;   // [n_node + 1] CSR row starts
    nz_t const *nz;                // [n_nz] CSR order
    edge_t const *edge;            // [n_nz] AoS edge labels (incl. weight)
    std::uint16_t const *perm;     // [n_node] new id -> caller's node id
    // Quotient images only: the twin leaves of a node (equal records, one
    // shared neighbour) are merged into one representative of multiplicity m.
    // `scale` = sqrt(m) per node, a section of doubles between the degrees
    // and the node records (a float sqrt(2) would cap a double solve at
    // 6e-8); `n_orig` = nodes of the full graph.  `degree` keeps the degrees
    // of the full graph.
    double const *scale = nullptr; // [n_node]
    int n_orig = 0;

    __device__ __forceinline__ graph_t(char const *arena, graph_header_t const &h)
        : n_node(h.n_node), n_nz(h.n_nz),
          degree(reinterpret_cast<float const *>(arena + h.degree)),
          node(reinterpret_cast<node_t const *>(arena + h.node)),
          rowptr(reinterpret_cast<std::uint16_t const *>(arena + h.rowptr)),
          nz(reinterpret_cast<nz_t const *>(arena + h.nz)),
          edge(reinterpret_cast<edge_t const *>(arena + h.edge)),
          perm(reinterpret_cast<std::uint16_t const *>(arena + h.perm)) {}

    // the view of a quotient image (`h`: its header with the plain node count)
    __device__ static __forceinline__ graph_t quotient(char const *arena, graph_header_t const &h, int n_orig_) {
        graph_t g(arena, h);
        g.scale = reinterpret_cast<double const *>(arena + h.degree + ((4u * (unsigned)h.n_node + 15u) & ~15u));
        g.n_orig = n_orig_;
        return g;
    }
};

}  // namespace graphdot
#endif
