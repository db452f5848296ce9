// The minimum spanning tree of the mutual-reachability graph of a
// device-resident kernel matrix, by Boruvka rounds on the implicit graph
// (model/clustering; the host side is model/clustering/_mst.py; DESIGN.md
// section 40).  This file is a translation unit by itself --
// MODEL_UNITS['mst'] of hip/source_module.py compiles its text -- although it
// is no .hip file: the stages and, at the end, the extern "C" kernels that
// name them.  IEEE arithmetic, no square root, and every result a function of
// the data alone: a repeat gives the same bits.
//
// K is the (n, n) matrix of k(sample i, sample j), float or double, read as it
// lies: element (i, j) at K[i s_row + j s_col].  With the self-similarities
// diag (n,) and the squared core distances c2 (n,),
//
//   d2(i, j) = (diag[i] + diag[j]) - 2.0 * (double)K[i][j];  d2 < 0 ? 0 : d2
//   s(i, j)  = min(d2(i, j), d2(j, i))
//   w2(i, j) = max(c2[i], c2[j], s(i, j))
//
// (2 K is exact, so a contraction into one fma rounds the same number once).
// Edges are compared in the strict total order (w2, min(i, j), max(i, j)):
// the spanning tree that is minimal in it is unique, Boruvka's rounds find
// exactly its edges, and since the order is strict the edges that the
// components choose in a round form no cycle but the pair of two components
// that choose the same edge.  For a fixed row i the order of its edges is the
// order (w2, j) of their columns.  Neither d2 nor w2 is written as a matrix.
//
// mst_rows_*: gridDim.x = strips * parts.  A workgroup owns a strip of 32
// rows and part p of the column tiles (tiles of 64 columns; part p has the
// tiles p tpp ... (p + 1) tpp - 1, tpp = ceil(tiles / parts): possibly none).
// A 32 x 64 tile of d2(i, j) is staged in LDS, loaded along whichever axis has
// the smaller stride; then the same tile of d2(j, i) is read from the
// transposed place in K, again along the axis of the smaller stride -- the
// threads change their mapping, not the matrix its layout -- and the minimum
// of the two stays in LDS.  Rows are 65 doubles apart, so that either mapping
// spreads over the banks: 16 640 bytes.  Wave w serves the rows 8 w ... 8 w +
// 7; lane l takes column l of every tile and keeps, per row, the first
// (w2, j) it has seen among the columns of another component (columns ascend,
// so a strict comparison keeps the smaller j).  A __shfl_xor butterfly of
// (value, index) pairs in that order ends the row: part p of row i writes
// (w2, j) to out[i parts + p], (+inf, -1) where it has no candidate.  A d2
// that is not finite before the clamp sets *flag (a plain store of 1) and is
// staged as +inf.
//   comp == nullptr is the rectangular mode: K is a (b, n) cross matrix, dq
//   and cq belong to its rows and dt and ct to its columns, nothing is
//   symmetrised and every column is a candidate: the nearest training sample
//   of a query in mutual reachability.
//
// mst_combine: one thread per row, the parts in their order.
//
// mst_best_w, mst_best_e: the minimum of a component, in two launches of one
// thread per row, with integer atomic minima on keys that carry the order: the
// bits of a non-negative double order as unsigned integers the way the
// doubles do (-0 is keyed as 0), so best_w[root] = min key(w2) over the
// component's rows; then the rows that hold that minimum offer (min(i, j) <<
// 32 | max(i, j)) to best_e[root].  A minimum of integers does not depend on
// the order of its operands: nothing here depends on scheduling.
//
// mst_hook: one thread per sample; a root r (comp[r] == r) with the edge (a,
// b) points to the root of the other end, unless that root chose the same
// edge and is the larger one: of a mutual pair the smaller root stays.  A root
// that vanishes writes (w2, a, b) at its own slot r of the edge buffers: every
// sample vanishes as a root exactly once, but the last one, so the n - 1 edges
// need no compaction.  Whoever is no root points to itself.
//
// mst_jump: parent'[i] = parent^8[i], from one buffer into another: every
// dependency is a launch boundary.  ceil(log8(components)) launches flatten
// the forest.
//
// mst_relabel: comp'[i] = parent[comp[i]], and count[workgroup] = its samples
// that are their own label, in total the number of components.
//
// An index that is out of range -- a label or a candidate the host did not
// make -- is never followed: such a row is skipped.
#ifndef GRAPHDOT_HIP_MST_H_
#define GRAPHDOT_HIP_MST_H_
#include "dense_reduce.h"

#define MST_ROWS 32             // rows per strip
#define MST_TILE 64             // columns per tile: one per lane
#define MST_LT 65               // doubles per staged row
#define MST_OWN (MST_ROWS / NWAVE)      // rows per wave
#define MST_JUMP 8              // steps of a pointer jump
#define MST_NONE 0x7fffffff     // the column of no candidate

namespace mst {

typedef unsigned long long key_t;
#define MST_NO_KEY (~0ull)

// (w, j) precedes (v, c) in the total order
__device__ __forceinline__ bool precedes(double w, int j, double v, int c) {
    return w < v || (w == v && j < c);
}

// d2 of one entry; not finite before the clamp: +inf, and `bad` is raised
__device__ __forceinline__ double entry(double s, double k, bool &bad) {
    double d2 = s - 2.0 * k;
    if (!is_finite(d2)) { bad = true; return __builtin_inf(); }
    return d2 < 0.0 ? 0.0 : d2;
}

// -- the row pass ----------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void rows_stage(
    const T *__restrict__ K, int64_t b, int64_t n, int64_t s_row,
    int64_t s_col, const double *__restrict__ dq,
    const double *__restrict__ dt, const double *__restrict__ cq,
    const double *__restrict__ ct, const int *__restrict__ comp,
    int64_t parts, double *__restrict__ out_w2, int *__restrict__ out_j,
    int *__restrict__ flag)
{
    __shared__ double tile[MST_ROWS][MST_LT];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t strip = blockIdx.x / parts, part = blockIdx.x % parts;
    const int64_t row0 = strip * MST_ROWS;
    const int64_t tiles = (n + MST_TILE - 1) / MST_TILE;
    const int64_t tpp = (tiles + parts - 1) / parts;
    const int64_t t0 = part * tpp;
    const int64_t t1 = t0 + tpp < tiles ? t0 + tpp : tiles;
    const double inf = __builtin_inf();
    const bool along_cols = s_col <= s_row;
    const bool square = comp != nullptr;

    double ci[MST_OWN], bw[MST_OWN];
    int li[MST_OWN], bj[MST_OWN];
#pragma unroll
    for (int r = 0; r < MST_OWN; ++r) {
        const int64_t i = row0 + wid * MST_OWN + r;
        ci[r] = i < b ? cq[i] : 0.0;
        li[r] = (square && i < b) ? comp[i] : -1;
        bw[r] = inf;
        bj[r] = MST_NONE;
    }

    bool bad = false;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t col0 = t * MST_TILE;
#pragma unroll
        for (int e = 0; e < MST_ROWS * MST_TILE / BLOCK; ++e) {
            // consecutive threads along the axis of the smaller stride
            const int x = threadIdx.x + e * BLOCK;
            const int r = along_cols ? x / MST_TILE : x % MST_ROWS;
            const int c = along_cols ? x % MST_TILE : x / MST_ROWS;
            const int64_t i = row0 + r, j = col0 + c;
            double d2 = inf;
            if (i < b && j < n)
                d2 = entry(dq[i] + dt[j], (double)K[i * s_row + j * s_col],
                           bad);
            tile[r][c] = d2;
        }
        if (square) {
            // K[j][i]: the same axis of the matrix is the other axis of the
            // tile (b == n here, dq == dt)
            __syncthreads();
#pragma unroll
            for (int e = 0; e < MST_ROWS * MST_TILE / BLOCK; ++e) {
                const int x = threadIdx.x + e * BLOCK;
                const int r = along_cols ? x % MST_ROWS : x / MST_TILE;
                const int c = along_cols ? x / MST_ROWS : x % MST_TILE;
                const int64_t i = row0 + r, j = col0 + c;
                if (i < b && j < n) {
                    const double d2 = entry(
                        dq[i] + dt[j], (double)K[j * s_row + i * s_col], bad);
                    if (d2 < tile[r][c]) tile[r][c] = d2;
                }
            }
        }
        __syncthreads();
        const int64_t j = col0 + lane;
        const bool valid = j < n;
        const double cj = valid ? ct[j] : 0.0;
        const int lj = (square && valid) ? comp[j] : -2;
#pragma unroll
        for (int r = 0; r < MST_OWN; ++r) {
            double w = tile[wid * MST_OWN + r][lane];
            w = ci[r] > w ? ci[r] : w;
            w = cj > w ? cj : w;
            if (valid && lj != li[r] && precedes(w, (int)j, bw[r], bj[r])) {
                bw[r] = w;
                bj[r] = (int)j;
            }
        }
        __syncthreads();
    }
    if (bad) *flag = 1;
#pragma unroll
    for (int r = 0; r < MST_OWN; ++r) {
        double w = bw[r];
        int j = bj[r];
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const double ow = __shfl_xor(w, off, WAVE);
            const int oj = __shfl_xor(j, off, WAVE);
            if (precedes(ow, oj, w, j)) { w = ow; j = oj; }
        }
        const int64_t i = row0 + wid * MST_OWN + r;
        if (i < b && lane == 0) {
            out_w2[i * parts + part] = w;
            out_j[i * parts + part] = j == MST_NONE ? -1 : j;
        }
    }
}

// gridDim.x = ceil(b / BLOCK)
__device__ __forceinline__ void combine_stage(
    const double *__restrict__ ws_w2, const int *__restrict__ ws_j, int64_t b,
    int64_t parts, double *__restrict__ out_w2, int *__restrict__ out_j)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= b) return;
    double w = __builtin_inf();
    int j = MST_NONE;
    for (int64_t p = 0; p < parts; ++p) {
        const double ow = ws_w2[i * parts + p];
        const int oj = ws_j[i * parts + p];
        if (oj >= 0 && precedes(ow, oj, w, j)) { w = ow; j = oj; }
    }
    out_w2[i] = w;
    out_j[i] = j == MST_NONE ? -1 : j;
}

// -- the minimum of a component --------------------------------------------------------
__device__ __forceinline__ key_t weight_key(double w) {
    return w == 0.0 ? 0ull : (key_t)__double_as_longlong(w);
}

__device__ __forceinline__ bool within(int64_t x, int64_t n) {
    return x >= 0 && x < n;
}

// gridDim.x = ceil(n / BLOCK)
__device__ __forceinline__ void best_w_stage(
    const double *__restrict__ w2, const int *__restrict__ cand,
    const int *__restrict__ comp, int64_t n, key_t *__restrict__ best_w)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int root = comp[i];
    if (!within(cand[i], n) || !within(root, n) || !(w2[i] >= 0.0)) return;
    atomicMin(&best_w[root], weight_key(w2[i]));
}

__device__ __forceinline__ void best_e_stage(
    const double *__restrict__ w2, const int *__restrict__ cand,
    const int *__restrict__ comp, int64_t n,
    const key_t *__restrict__ best_w, key_t *__restrict__ best_e)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int root = comp[i], j = cand[i];
    if (!within(j, n) || !within(root, n) || !(w2[i] >= 0.0)) return;
    if (weight_key(w2[i]) != best_w[root]) return;
    const key_t lo = (key_t)(i < j ? i : j), hi = (key_t)(i < j ? j : i);
    atomicMin(&best_e[root], (lo << 32) | hi);
}

// -- hooking, flattening, relabelling ----------------------------------------------------
__device__ __forceinline__ void hook_stage(
    const int *__restrict__ comp, int64_t n, const key_t *__restrict__ best_w,
    const key_t *__restrict__ best_e, int *__restrict__ parent,
    double *__restrict__ edge_w, int *__restrict__ edge_a,
    int *__restrict__ edge_b)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    int p = (int)i;
    const key_t e = best_e[i];
    if (comp[i] == (int)i && e != MST_NO_KEY) {
        const int64_t a = (int64_t)(e >> 32), b = (int64_t)(e & 0xffffffffull);
        if (within(a, n) && within(b, n)) {
            const int ca = comp[a], cb = comp[b];
            const int other = ca == (int)i ? cb : ca;
            if (within(other, n) && other != (int)i
                    && !(best_e[other] == e && (int)i < other)) {
                p = other;
                edge_w[i] = __longlong_as_double((long long)best_w[i]);
                edge_a[i] = (int)a;
                edge_b[i] = (int)b;
            }
        }
    }
    parent[i] = p;
}

__device__ __forceinline__ void jump_stage(const int *__restrict__ parent,
                                           int64_t n, int *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    int p = (int)i;
    for (int s = 0; s < MST_JUMP; ++s)
        if (within(p, n)) p = parent[p];
    out[i] = p;
}

__device__ __forceinline__ void relabel_stage(
    const int *__restrict__ comp, const int *__restrict__ parent, int64_t n,
    int *__restrict__ out, int *__restrict__ count)
{
    __shared__ int own[NWAVE];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool mine = false;
    if (i < n) {
        int c = comp[i];
        if (within(c, n)) c = parent[c];
        out[i] = c;
        mine = c == (int)i;
    }
    const int total = __popcll(__ballot(mine));
    if (lane == 0) own[wid] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < NWAVE; ++w) t += own[w];
        count[blockIdx.x] = t;
    }
}

}  // namespace mst

#define MST_ROWS_PARAMS                                                        \
    int64_t b, int64_t n, int64_t s_row, int64_t s_col, const double *dq,      \
    const double *dt, const double *cq, const double *ct, const int *comp,     \
    int64_t parts, double *out_w2, int *out_j, int *flag
#define MST_ROWS_ARGS                                                          \
    b, n, s_row, s_col, dq, dt, cq, ct, comp, parts, out_w2, out_j, flag

extern "C" __global__ __launch_bounds__(BLOCK) void
mst_rows_f32(const float *K, MST_ROWS_PARAMS)
{
    mst::rows_stage<float>(K, MST_ROWS_ARGS);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mst_rows_f64(const double *K, MST_ROWS_PARAMS)
{
    mst::rows_stage<double>(K, MST_ROWS_ARGS);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mst_combine(const double *ws_w2, const int *ws_j, int64_t b, int64_t parts,
            double *out_w2, int *out_j)
{
    mst::combine_stage(ws_w2, ws_j, b, parts, out_w2, out_j);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mst_best_w(const double *w2, const int *cand, const int *comp, int64_t n,
           unsigned long long *best_w)
{
    mst::best_w_stage(w2, cand, comp, n, best_w);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mst_best_e(const double *w2, const int *cand, const int *comp, int64_t n,
           const unsigned long long *best_w, unsigned long long *best_e)
{
    mst::best_e_stage(w2, cand, comp, n, best_w, best_e);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mst_hook(const int *comp, int64_t n, const unsigned long long *best_w,
         const unsigned long long *best_e, int *parent, double *edge_w,
         int *edge_a, int *edge_b)
{
    mst::hook_stage(comp, n, best_w, best_e, parent, edge_w, edge_a, edge_b);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mst_jump(const int *parent, int64_t n, int *out)
{
    mst::jump_stage(parent, n, out);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mst_relabel(const int *comp, const int *parent, int64_t n, int *out,
            int *count)
{
    mst::relabel_stage(comp, parent, n, out, count);
}

#endif
