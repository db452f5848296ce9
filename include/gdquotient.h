/*
 * gdquotient.h -- C ABI of the twin-leaf quotient packer of libgdhost.so
 * (csrc/gdhost.cpp; bound by graphdot_amd/hip/hostlib.py like the entry
 * points of gdhost.h, same return codes).  The numpy statement it is held to
 * byte for byte is _devicegraph._quotient_blob_numpy.
 */
#ifndef GDQUOTIENT_H_
#define GDQUOTIENT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The twin-leaf quotient image of ONE packed graph (sections of its image as
 * gdh_pack_graphs wrote them: degree f32[n], node records, rowptr u16[n+1],
 * nz u16x2[nnz], edge records, perm u16[n]).  A twin group is a maximal set
 * of m >= 2 nodes with exactly one neighbour each and no self loop, the same
 * neighbour -- which has at least two neighbours itself --, bytewise equal
 * node records and bytewise equal edge records to that neighbour; its first
 * node stays, with multiplicity m.  The nodes that stay are renumbered by
 * descending adjacency count of the quotient (stable), the nonzeros between
 * them put in CSR order.  Sections of the result, each 16-byte aligned:
 *   degree f32[nq] (of the FULL graph) | scale f64[nq] (sqrt(m)) | node_t[nq]
 *   | rowptr u16[nq+1] | nz u16x2[nnzq] | edge_t[nnzq] | perm u16[nq]
 * Outputs: blob (capacity bytes, zero padded), sec_off [7], counts [3] = nq,
 * nnzq, bytes used. */
int gdh_quotient_graph(int32_t n, int32_t nnz, const float *degree,
                       const uint8_t *node, int32_t node_size, const uint16_t *rowptr,
                       const uint16_t *nz, const uint8_t *edge, int32_t edge_size,
                       const uint16_t *perm, uint8_t *blob, int64_t capacity,
                       int64_t *sec_off, int64_t *counts);

#ifdef __cplusplus
}
#endif
#endif
