// Row-wise k-nearest-neighbour selection over a device-resident kernel matrix
// and what the neighbour models make of the lists (model/neighbors; the host
// side is model/neighbors/_knn.py).  Its translation
// unit is the text TEXT_UNITS['knn'] of hip/source_module.py: this header and
// thin extern "C" wrappers around the templates below.
//
// K is the (b, n) matrix of k(query i, candidate j), float or double, read as
// it lies: element (i, j) at K[i s_row + j s_col], any positive strides.  With
// the self-similarities dq (b,) and dt (n,),
//
//   s = dq[i] + dt[j];  d2 = s - 2.0 * (double)K[i][j];  d2 = d2 < 0 ? 0 : d2
//
// (2 K is exact, so a contraction into one fma rounds the same number once:
// the same bits).  The neighbours of row i are its k smallest candidates in
// the total order (d2, j).  Because the order is total, the k smallest of a
// set are one well-defined list whichever way the set is walked or split:
// the lists depend on the row's data alone, not on the layout, the strip, the
// number of rows or the split of the columns.
//
// knn_topk_*: gridDim.x = strips * parts.  A workgroup owns a strip of 32
// rows and part p of the column tiles (tiles of 64 columns; part p has the
// tiles p tpp ... (p + 1) tpp - 1, tpp = ceil(tiles / parts): possibly none).
// Each 32 x 64 tile is staged in LDS as d2 (+inf for what is no candidate:
// beyond b or n, or column i of row i with exclude_self), loaded along
// whichever axis has the smaller stride; rows are 65 doubles apart, so that
// the stores of either loading order spread over the banks: 16 640 bytes.
// Wave w serves the rows 8 w ... 8 w + 7 of the strip and keeps their lists in
// registers: lane l holds entry l of the sorted list of each of its rows (a
// double and an int: 24 registers), (+inf, INT_MAX) where there is none yet.
// For a row, lane l takes candidate l of the tile and compares it with the
// row's k-th entry; __ballot gives the 64-bit mask of the survivors, which are
// inserted one after the other, lowest column first: the rank of the newcomer
// is the number of lanes whose entry precedes it (a second ballot), and the
// lanes from there on take their left neighbour's entry (__shfl_up).  After
// the first tiles survivors are rare.  A d2 that is not finite before the
// clamp sets *flag (a plain store of 1 by whoever sees one) and is staged as
// +inf: the host raises, whatever the lists say.  Part p of row i writes its
// k entries to out[(i parts + p) k ...], (+inf, -1) where it has fewer: with
// parts = 1 that is the final list.
//
// knn_merge: gridDim.x = ceil(b / NWAVE), one wave per row: the same
// selection over the parts' k entries each; the (+inf, -1) entries of short
// parts are no candidates.
//
// knn_average, knn_lrd, knn_ratio: one thread per output, neighbours summed in
// rank order.  No atomics anywhere, and nothing of size b x n is written.
#ifndef GRAPHDOT_HIP_KNN_H_
#define GRAPHDOT_HIP_KNN_H_
#include "dense_reduce.h"

#define K_MOST 64               // entries per list: one per lane
#define KNN_ROWS 32             // rows per strip
#define KNN_TILE 64             // columns per tile: one per lane
#define KNN_LT 65               // doubles per staged row
#define KNN_OWN (KNN_ROWS / NWAVE)      // rows per wave
#define KNN_NONE 0x7fffffff     // the column of an empty entry

namespace knn {

// (d2, j) precedes (e2, c) in the total order
__device__ __forceinline__ bool precedes(double d2, int j, double e2, int c) {
    return d2 < e2 || (d2 == e2 && j < c);
}

// Offer the wave's 64 candidates (cd, cj), one per lane, to the sorted list
// (ld, li), one entry per lane, of which the first k count.
__device__ __forceinline__ void offer(double &ld, int &li, double cd, int cj,
                                      int k)
{
    const int lane = threadIdx.x % WAVE;
    double kd = __shfl(ld, k - 1, WAVE);
    int ki = __shfl(li, k - 1, WAVE);
    unsigned long long mask = __ballot(precedes(cd, cj, kd, ki));
    while (mask) {
        const int s = __builtin_ctzll(mask);
        mask &= mask - 1;
        const double nd = __shfl(cd, s, WAVE);
        const int ni = __shfl(cj, s, WAVE);
        if (!precedes(nd, ni, kd, ki)) continue;    // (the list has moved on)
        const int pos = __popcll(__ballot(precedes(ld, li, nd, ni)));
        const double pd = __shfl_up(ld, 1, WAVE);
        const int pi = __shfl_up(li, 1, WAVE);
        if (lane == pos) { ld = nd; li = ni; }
        else if (lane > pos) { ld = pd; li = pi; }
        kd = __shfl(ld, k - 1, WAVE);
        ki = __shfl(li, k - 1, WAVE);
    }
}

template <typename T>
__device__ __forceinline__ void topk_stage(
    const T *__restrict__ K, int64_t b, int64_t n, int64_t s_row,
    int64_t s_col, const double *__restrict__ dq,
    const double *__restrict__ dt, int k, int exclude_self, int64_t parts,
    double *__restrict__ out_d2, int64_t *__restrict__ out_idx,
    int *__restrict__ flag)
{
    __shared__ double tile[KNN_ROWS][KNN_LT];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t strip = blockIdx.x / parts, part = blockIdx.x % parts;
    const int64_t row0 = strip * KNN_ROWS;
    const int64_t tiles = (n + KNN_TILE - 1) / KNN_TILE;
    const int64_t tpp = (tiles + parts - 1) / parts;
    const int64_t t0 = part * tpp;
    const int64_t t1 = t0 + tpp < tiles ? t0 + tpp : tiles;
    const double inf = __builtin_inf();
    const bool along_cols = s_col <= s_row;

    double ld[KNN_OWN];
    int li[KNN_OWN];
#pragma unroll
    for (int r = 0; r < KNN_OWN; ++r) { ld[r] = inf; li[r] = KNN_NONE; }

    bool bad = false;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t col0 = t * KNN_TILE;
#pragma unroll
        for (int e = 0; e < KNN_ROWS * KNN_TILE / BLOCK; ++e) {
            // consecutive threads along the axis of the smaller stride
            const int x = threadIdx.x + e * BLOCK;
            const int r = along_cols ? x / KNN_TILE : x % KNN_ROWS;
            const int c = along_cols ? x % KNN_TILE : x / KNN_ROWS;
            const int64_t i = row0 + r, j = col0 + c;
            double d2 = inf;
            if (i < b && j < n && !(exclude_self && i == j)) {
                const double s = dq[i] + dt[j];
                d2 = s - 2.0 * (double)K[i * s_row + j * s_col];
                // (before the clamp, which would turn -inf into 0)
                if (!is_finite(d2)) { bad = true; d2 = inf; }
                d2 = d2 < 0.0 ? 0.0 : d2;
            }
            tile[r][c] = d2;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < KNN_OWN; ++r)
            offer(ld[r], li[r], tile[wid * KNN_OWN + r][lane],
                  (int)(col0 + lane), k);
        __syncthreads();
    }
    if (bad) *flag = 1;
#pragma unroll
    for (int r = 0; r < KNN_OWN; ++r) {
        const int64_t i = row0 + wid * KNN_OWN + r;
        if (i < b && lane < k) {
            const int64_t o = (i * parts + part) * k + lane;
            out_d2[o] = ld[r];
            out_idx[o] = li[r] == KNN_NONE ? (int64_t)-1 : (int64_t)li[r];
        }
    }
}

// gridDim.x = ceil(b / NWAVE)
__device__ __forceinline__ void merge_stage(
    const double *__restrict__ ws_d2, const int64_t *__restrict__ ws_idx,
    int64_t b, int64_t parts, int k, double *__restrict__ out_d2,
    int64_t *__restrict__ out_idx)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= b) return;                       // (whole waves only)
    const int64_t m = parts * k;
    const double *wd = ws_d2 + i * m;
    const int64_t *wi = ws_idx + i * m;
    double ld = __builtin_inf();
    int li = KNN_NONE;
    for (int64_t c0 = 0; c0 < m; c0 += WAVE) {
        const int64_t c = c0 + lane;
        double cd = __builtin_inf();
        int cj = KNN_NONE;
        if (c < m && wi[c] >= 0) { cd = wd[c]; cj = (int)wi[c]; }
        offer(ld, li, cd, cj, k);
    }
    if (lane < k) {
        out_d2[i * k + lane] = ld;
        out_idx[i * k + lane] = li == KNN_NONE ? (int64_t)-1 : (int64_t)li;
    }
}

// The weight of neighbour r of a list: 1 (mode 0), or 1 / d (mode 1) --
// unless some neighbour of the list is at d == 0: then 1 for those, 0 for the
// rest.
__device__ __forceinline__ double weight(double d, int mode, bool zeros) {
    if (mode == 0) return 1.0;
    if (zeros) return d == 0.0 ? 1.0 : 0.0;
    return 1.0 / d;
}

// Row j of a table of n rows of m doubles, column c -- NaN for the -1 of a
// list that matrix entries which are not finite left short (the flag is up,
// the host raises; nothing is read out of bounds meanwhile)
__device__ __forceinline__ double at(const double *__restrict__ T, int64_t j,
                                     int64_t n, int64_t m, int64_t c) {
    return j >= 0 && j < n ? T[j * m + c] : __builtin_nan("");
}

// gridDim.x = ceil(b m / BLOCK): out[i][c] = sum_r w_r T[idx[i][r]][c] / sum_r
// w_r, r in rank order
__device__ __forceinline__ void average_stage(
    const double *__restrict__ d2, const int64_t *__restrict__ idx, int64_t b,
    int k, const double *__restrict__ T, int64_t n, int64_t m, int mode,
    double *__restrict__ out)
{
    const int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= b * m) return;
    const int64_t i = x / m, c = x % m;
    bool zeros = false;
    if (mode != 0)
        for (int r = 0; r < k; ++r) zeros |= d2[i * k + r] == 0.0;
    double num = 0.0, den = 0.0;
    for (int r = 0; r < k; ++r) {
        const double w = weight(sqrt(d2[i * k + r]), mode, zeros);
        num += w * at(T, idx[i * k + r], n, m, c);
        den += w;
    }
    out[x] = num / den;
}

// gridDim.x = ceil(b / BLOCK): lrd[i] = 1 / (mean_r max(kdist[idx[i][r]],
// d[i][r]) + 1e-10)
__device__ __forceinline__ void lrd_stage(
    const double *__restrict__ d2, const int64_t *__restrict__ idx, int64_t b,
    int k, const double *__restrict__ kdist, int64_t n,
    double *__restrict__ lrd)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= b) return;
    double s = 0.0;
    for (int r = 0; r < k; ++r) {
        const double d = sqrt(d2[i * k + r]);
        const double kd = at(kdist, idx[i * k + r], n, 1, 0);
        s += nanmax(kd, d);
    }
    lrd[i] = 1.0 / (s / (double)k + 1e-10);
}

// gridDim.x = ceil(b / BLOCK): lof[i] = mean_r (lrd_train[idx[i][r]] / lrd[i])
__device__ __forceinline__ void ratio_stage(
    const int64_t *__restrict__ idx, int64_t b, int k,
    const double *__restrict__ lrd_train, int64_t n,
    const double *__restrict__ lrd, double *__restrict__ lof)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= b) return;
    double s = 0.0;
    for (int r = 0; r < k; ++r)
        s += at(lrd_train, idx[i * k + r], n, 1, 0) / lrd[i];
    lof[i] = s / (double)k;
}

}  // namespace knn
#endif
