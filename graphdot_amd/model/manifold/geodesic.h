// Geodesic distances on the neighbourhood graph of a device-resident kernel
// matrix (model/manifold; the host side is model/manifold/_geodesic.py;
// DESIGN.md section 39).  This file is a translation unit by itself --
// MODEL_UNITS['geodesic'] of hip/source_module.py compiles its text --
// although it is no .hip file: the stages and, at the end, the extern "C"
// kernels that name them.  IEEE arithmetic, no atomics, and every result a
// function of the data alone: a repeat gives the same bits.
//
// K is the (n, n) matrix of k(sample i, sample j), float or double, read as it
// lies: element (i, j) at K[i s_row + j s_col].  With the self-similarities
// diag (n,) and the neighbour lists idx (n, k) of knn.h (each row without
// itself),
//
//   d2(i, j) = (diag[i] + diag[j]) - 2.0 * (double)K[i][j];  d2 < 0 ? 0 : d2
//   W[i][j] = sqrt(min(d2(i, j), d2(j, i)))  if j is in the list of i or i in
//             the list of j;  0 if i == j;  +inf otherwise
//
// (2 K is exact, so a contraction into one fma rounds the same number once).
// The min makes W symmetric to the bit whether the stored K is or not, and
// everything below relies on that.
//
// geo_graph_*: gridDim.x = R^2, R = ceil(n / GEO_T).  Owner computes: a
// workgroup owns a GEO_T x GEO_T tile of W, stages the lists of its rows and of
// its columns in LDS as int (row stride k | 1: lanes along the columns walk
// the lists of 64 different columns, an odd stride spreads them over the
// banks), and each thread decides for its own elements whether they are edges
// and reads K[i][j] and K[j][i] for those that are.  There is no scatter: an
// edge that is in one list only is found by the owner of (i, j) and by the
// owner of (j, i) alike, so no two workgroups write one element and every
// element -- the inf fill and the zero diagonal included -- is written once.
//
// geo_fw_diag, geo_fw_cross, geo_fw_rest: round p of the blocked
// Floyd-Warshall algorithm on G (n, n) double, in place; the host launches the
// three for p = 0 .. R - 1 in this order.  Tiles are GEO_T x GEO_T, a ragged
// edge is padded with +inf in LDS and never stored.  There is no subtraction
// and inf + inf = inf: a graph that is not connected yields inf, never NaN.
//   diag   one workgroup: the pivot tile (p, p) in LDS, GEO_T dependent steps
//          x[i][j] = min(x[i][j], x[i][m] + x[m][j]).
//   cross  2 (R - 1) workgroups: the tiles (p, J) of the pivot row against
//          the finished pivot tile P, x[i][j] = min(x[i][j], P[i][m] +
//          x[m][j]), and the tiles (I, p) of the pivot column, which are
//          loaded transposed, run through the same steps and stored transposed:
//          the mirror of a tile sees the same operations on the same bits.
//   rest   (R - 1)^2 workgroups, one per tile (I, J) with I, J != p: C =
//          min(C, A (+) B) with A = (I, p) and B = (p, J) fixed -- the min-plus
//          tile product, the hot loop.  A is needed by columns, A[:, m]; G is
//          symmetric, so A[i][m] is element [m][i] of the row tile (p, I) and
//          both operands are tiles of the pivot row, loaded as they lie:
//          2 x 32 KiB of LDS.
// `steps` and `rest_stage` share one mapping: 256 threads as 16 x 16, a
// thread holds a 4 x 4 register tile of rows {2 ty, 2 ty + 1, 32 + 2 ty, 33 +
// 2 ty} and columns {2 tx, 2 tx + 1, 32 + 2 tx, 33 + 2 tx}.  Per m it reads
// four double2 (ds_read_b128) of row m of the two LDS tiles; the 16 lanes that
// differ in tx read 256 consecutive bytes, one bank row, and the lanes that
// differ in ty alone read one address.  In `steps` the tile stays in registers
// and step m reads row m of it alone (and of P): after step m the 16 threads
// that own row m + 1 put it into LDS, and one barrier ends the step.  The pivot
// tile is read by rows where the algorithm says columns, P[i][m] as P[m][i]:
// it is symmetric at every step.
// Symmetry: the mirror of every update adds the same two numbers in the other
// order, which rounds the same, and min is exact: G stays symmetric to the
// bit.
//
// geo_finish: gridDim.x = ceil(n / GEO_FIN_ROWS), a wave per row, four rows
// per wave.  B[i][j] = -0.5 * (g * g); label[i] = the smallest j that i
// reaches (the label of its component); count[workgroup] = its rows that are
// their own label, in total the number of components.
//
// geo_extend: gridDim.x = ceil(b / GEO_EXT_ROWS) * ceil(n / BLOCK).  A
// workgroup takes a strip of query rows, whose lists (sqrt(d2), column) it
// keeps in LDS, and BLOCK columns, one per thread: Gq[q][j] = min_r (sqrt(d2[q][r])
// + G[idx[q][r]][j]), read along j, and Bq = -0.5 * (Gq * Gq).  An entry of a
// list that names no training sample is no term.
#ifndef GRAPHDOT_HIP_GEODESIC_H_
#define GRAPHDOT_HIP_GEODESIC_H_
#include "dense_reduce.h"

#define GEO_T 64                // rows and columns per tile
#define GEO_K_MOST 64           // most neighbours per list
#define GEO_FIN_ROWS 16         // rows per workgroup of geo_finish
#define GEO_EXT_ROWS 16         // query rows per workgroup of geo_extend

namespace geo {

typedef double tile_t[GEO_T][GEO_T];

// -- the graph -------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void graph_stage(
    const T *__restrict__ K, int64_t n, int64_t s_row, int64_t s_col,
    const double *__restrict__ diag, const int64_t *__restrict__ idx, int k,
    double *__restrict__ W)
{
    __shared__ int rows[GEO_T * (GEO_K_MOST + 1)];
    __shared__ int cols[GEO_T * (GEO_K_MOST + 1)];
    const int kp = k | 1;
    const int64_t R = (n + GEO_T - 1) / GEO_T;
    const int64_t i0 = ((int64_t)blockIdx.x / R) * GEO_T;
    const int64_t j0 = ((int64_t)blockIdx.x % R) * GEO_T;
    for (int e = threadIdx.x; e < GEO_T * k; e += BLOCK) {
        const int r = e / k, c = e % k;
        rows[r * kp + c] = i0 + r < n ? (int)idx[(i0 + r) * k + c] : -1;
        cols[r * kp + c] = j0 + r < n ? (int)idx[(j0 + r) * k + c] : -1;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < GEO_T * GEO_T; e += BLOCK) {
        const int li = e / GEO_T, lj = e % GEO_T;
        const int64_t i = i0 + li, j = j0 + lj;
        if (i >= n || j >= n) continue;
        double w = 0.0;
        if (i != j) {
            bool edge = false;
            for (int r = 0; r < k; ++r)
                edge |= (rows[li * kp + r] == (int)j)
                        | (cols[lj * kp + r] == (int)i);
            w = __builtin_inf();
            if (edge) {
                const double s = diag[i] + diag[j];
                double a = s - 2.0 * (double)K[i * s_row + j * s_col];
                double b = s - 2.0 * (double)K[j * s_row + i * s_col];
                a = a < 0.0 ? 0.0 : a;
                b = b < 0.0 ? 0.0 : b;
                w = sqrt(b < a ? b : a);
            }
        }
        W[i * n + j] = w;
    }
}

// -- Floyd-Warshall --------------------------------------------------------------------
// Tile (ti, tj) of G into S, +inf beyond n.  tr: S takes the transpose, and
// the lanes go down the rows of G so that they stay consecutive in LDS.
__device__ __forceinline__ void load_tile(
    const double *__restrict__ G, int64_t n, int64_t ti, int64_t tj,
    tile_t &S, bool tr)
{
    for (int e = threadIdx.x; e < GEO_T * GEO_T; e += BLOCK) {
        const int hi = e / GEO_T, lo = e % GEO_T;
        const int64_t i = ti * GEO_T + (tr ? lo : hi);
        const int64_t j = tj * GEO_T + (tr ? hi : lo);
        S[hi][lo] = (i < n && j < n) ? G[i * n + j] : __builtin_inf();
    }
}

__device__ __forceinline__ void store_tile(
    double *__restrict__ G, int64_t n, int64_t ti, int64_t tj,
    const tile_t &S, bool tr)
{
    for (int e = threadIdx.x; e < GEO_T * GEO_T; e += BLOCK) {
        const int hi = e / GEO_T, lo = e % GEO_T;
        const int64_t i = ti * GEO_T + (tr ? lo : hi);
        const int64_t j = tj * GEO_T + (tr ? hi : lo);
        if (i < n && j < n) G[i * n + j] = S[hi][lo];
    }
}

// row / column r = 0 .. 3 of the register tile of thread coordinate t
__device__ __forceinline__ int own(int t, int r) {
    return (r & 2) * (GEO_T / 4) + 2 * t + (r & 1);
}

// four numbers of row m of S for thread coordinate t: two double2
__device__ __forceinline__ void read4(const tile_t &S, int m, int t,
                                      double (&out)[4]) {
    const double2 lo = *reinterpret_cast<const double2 *>(&S[m][2 * t]);
    const double2 hi =
        *reinterpret_cast<const double2 *>(&S[m][GEO_T / 2 + 2 * t]);
    out[0] = lo.x; out[1] = lo.y; out[2] = hi.x; out[3] = hi.y;
}

// x[r][q] = min(x[r][q], a[r] + b[q])
__device__ __forceinline__ void relax(double (&x)[4][4], const double (&a)[4],
                                      const double (&b)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) x[r][q] = fmin(x[r][q], a[r] + b[q]);
}

// x[r][.] of a thread into its place in row `row` of X
__device__ __forceinline__ void put4(tile_t &X, int row, int t,
                                     const double (&x)[4]) {
    *reinterpret_cast<double2 *>(&X[row][2 * t]) = make_double2(x[0], x[1]);
    *reinterpret_cast<double2 *>(&X[row][GEO_T / 2 + 2 * t]) =
        make_double2(x[2], x[3]);
}

// The GEO_T dependent steps on the tile X in LDS against the finished,
// symmetric pivot tile P (&P == &X: the pivot tile itself).  X is kept in
// registers; step m reads row m of it from LDS, so after step m the owners of
// row m + 1 put it there, and everything at the end.  Barriers inside: every
// thread of the workgroup comes here.
__device__ __forceinline__ void steps(const tile_t &P, tile_t &X)
{
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    double x[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) read4(X, own(ty, r), tx, x[r]);
    for (int m = 0; m < GEO_T; ++m) {
        double a[4], b[4];
        read4(P, m, ty, a);
        read4(X, m, tx, b);
        relax(x, a, b);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (own(ty, r) == m + 1) put4(X, m + 1, tx, x[r]);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) put4(X, own(ty, r), tx, x[r]);
    __syncthreads();
}

__device__ __forceinline__ void fw_diag_stage(double *__restrict__ G,
                                              int64_t n, int64_t p)
{
    __shared__ __attribute__((aligned(16))) tile_t X;
    load_tile(G, n, p, p, X, false);
    __syncthreads();
    steps(X, X);
    store_tile(G, n, p, p, X, false);
}

__device__ __forceinline__ void fw_cross_stage(double *__restrict__ G,
                                               int64_t n, int64_t p)
{
    __shared__ __attribute__((aligned(16))) tile_t P, X;
    const int64_t R = (n + GEO_T - 1) / GEO_T;
    const bool column = (int64_t)blockIdx.x >= R - 1;
    int64_t t = (int64_t)blockIdx.x - (column ? R - 1 : 0);
    t += t >= p;
    load_tile(G, n, p, p, P, false);
    load_tile(G, n, column ? t : p, column ? p : t, X, column);
    __syncthreads();
    steps(P, X);
    store_tile(G, n, column ? t : p, column ? p : t, X, column);
}

__device__ __forceinline__ void fw_rest_stage(double *__restrict__ G,
                                              int64_t n, int64_t p)
{
    __shared__ __attribute__((aligned(16))) tile_t A, B;
    const int64_t R = (n + GEO_T - 1) / GEO_T;
    int64_t I = (int64_t)blockIdx.x / (R - 1), J = (int64_t)blockIdx.x % (R - 1);
    I += I >= p;
    J += J >= p;
    load_tile(G, n, p, I, A, false);          // A[m][i] = G[i][m]: symmetric
    load_tile(G, n, p, J, B, false);
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    double x[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = I * GEO_T + own(ty, r), j = J * GEO_T + own(tx, q);
            x[r][q] = (i < n && j < n) ? G[i * n + j] : __builtin_inf();
        }
    __syncthreads();
#pragma unroll 4
    for (int m = 0; m < GEO_T; ++m) {
        double a[4], b[4];
        read4(A, m, ty, a);
        read4(B, m, tx, b);
        relax(x, a, b);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = I * GEO_T + own(ty, r), j = J * GEO_T + own(tx, q);
            if (i < n && j < n) G[i * n + j] = x[r][q];
        }
}

// -- B and the components --------------------------------------------------------------
__device__ __forceinline__ void finish_stage(
    const double *__restrict__ G, int64_t n, double *__restrict__ B,
    int *__restrict__ label, int *__restrict__ count)
{
    __shared__ int own_label[NWAVE];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    int mine = 0;
    for (int s = 0; s < GEO_FIN_ROWS / NWAVE; ++s) {
        const int64_t i = (int64_t)blockIdx.x * GEO_FIN_ROWS
                          + wid * (GEO_FIN_ROWS / NWAVE) + s;
        if (i >= n) break;                    // (whole waves)
        int64_t first = n;
        for (int64_t j = lane; j < n; j += WAVE) {
            const double g = G[i * n + j];
            B[i * n + j] = -0.5 * (g * g);
            if (g < __builtin_inf() && j < first) first = j;
        }
        int f = (int)first;
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const int o = __shfl_xor(f, off, WAVE);
            f = o < f ? o : f;
        }
        if (lane == 0) label[i] = f;
        mine += f == (int)i;
    }
    if (lane == 0) own_label[wid] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < NWAVE; ++w) t += own_label[w];
        count[blockIdx.x] = t;
    }
}

// -- out of sample ---------------------------------------------------------------------
__device__ __forceinline__ void extend_stage(
    const double *__restrict__ d2, const int64_t *__restrict__ idx, int64_t b,
    int k, const double *__restrict__ G, int64_t n, double *__restrict__ Bq,
    double *__restrict__ Gq)
{
    __shared__ double dist[GEO_EXT_ROWS * GEO_K_MOST];
    __shared__ int at[GEO_EXT_ROWS * GEO_K_MOST];
    const int64_t tiles = (n + BLOCK - 1) / BLOCK;
    const int64_t q0 = ((int64_t)blockIdx.x / tiles) * GEO_EXT_ROWS;
    const int64_t j = ((int64_t)blockIdx.x % tiles) * BLOCK + threadIdx.x;
    for (int e = threadIdx.x; e < GEO_EXT_ROWS * k; e += BLOCK) {
        const int64_t q = q0 + e / k;
        int64_t c = -1;
        double d = __builtin_inf();
        if (q < b) {
            c = idx[q * k + e % k];
            d = sqrt(d2[q * k + e % k]);
        }
        dist[e] = d;
        at[e] = (c >= 0 && c < n) ? (int)c : -1;
    }
    __syncthreads();
    if (j >= n) return;                       // (no barrier below)
    for (int s = 0; s < GEO_EXT_ROWS; ++s) {
        const int64_t q = q0 + s;
        if (q >= b) break;
        double g = __builtin_inf();
        for (int r = 0; r < k; ++r) {
            const int c = at[s * k + r];
            if (c >= 0) g = fmin(g, dist[s * k + r] + G[(int64_t)c * n + j]);
        }
        Bq[q * n + j] = -0.5 * (g * g);
        if (Gq) Gq[q * n + j] = g;
    }
}

}  // namespace geo

extern "C" __global__ __launch_bounds__(BLOCK) void
geo_graph_f32(const float *K, int64_t n, int64_t s_row, int64_t s_col,
              const double *diag, const int64_t *idx, int k, double *W)
{
    geo::graph_stage<float>(K, n, s_row, s_col, diag, idx, k, W);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
geo_graph_f64(const double *K, int64_t n, int64_t s_row, int64_t s_col,
              const double *diag, const int64_t *idx, int k, double *W)
{
    geo::graph_stage<double>(K, n, s_row, s_col, diag, idx, k, W);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
geo_fw_diag(double *G, int64_t n, int64_t p)
{
    geo::fw_diag_stage(G, n, p);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
geo_fw_cross(double *G, int64_t n, int64_t p)
{
    geo::fw_cross_stage(G, n, p);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
geo_fw_rest(double *G, int64_t n, int64_t p)
{
    geo::fw_rest_stage(G, n, p);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
geo_finish(const double *G, int64_t n, double *B, int *label, int *count)
{
    geo::finish_stage(G, n, B, label, count);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
geo_extend(const double *d2, const int64_t *idx, int64_t b, int k,
           const double *G, int64_t n, double *Bq, double *Gq)
{
    geo::extend_stage(d2, idx, b, k, G, n, Bq, Gq);
}

#endif
