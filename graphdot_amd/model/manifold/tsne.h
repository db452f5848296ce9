// Exact t-SNE on a device-resident kernel matrix (model/manifold; the host
// side is model/manifold/_tsne.py).  This file is a
// translation unit by itself -- FILE_UNITS['tsne'] of hip/source_module.py
// compiles its text -- although it is no .hip file: the templates and, at the
// end, the extern "C" kernels that name them.
//
// K is the symmetric (n, n) matrix of k(sample i, sample j), float or double,
// read as it lies: element (i, j) at K[j k_lane + i k_col], the lane axis being
// the index of the smaller stride.  With the self-similarities diag (n,),
//
//   d2 = (diag[i] + diag[j]) - 2.0 * (double)K[i][j];  d2 = d2 < 0 ? 0 : d2
//
// (2 K is exact, so a contraction into one fma rounds the same number once).
// Per row i the calibration leaves three numbers, beta_i, m_i = min_{j != i}
// d2 and 1 / Z_i, Z_i = sum_{j != i} exp(-beta_i (d2 - m_i)), and the joint
// probability of a pair is recomputed from those of both rows wherever it is
// needed,
//
//   p_ij = max((exp(-beta_i (d2 - m_i)) / Z_i
//               + exp(-beta_j (d2 - m_j)) / Z_j) / (2 n), eps):
//
// nothing of size n x n is written.  All sums are double, in an order that the
// shape alone decides, without atomics.
//
// tsne_calibrate_*: gridDim.x = ceil(n / NWAVE), a wave per row.  The row's d2
// - m_i is kept in LDS for the up to 100 passes of the bisection where n <=
// TS_CAL_COLS (four rows of 2048 doubles: 64 KiB) and recomputed from K in
// every pass beyond; each lane reads back what it wrote itself, so no barrier.
// The terms at d2 == m_i are counted, not added (their e is exactly 1): then
// the sums of two samples whose data are the same -- duplicates, at d2 == 0 of
// each other -- hold the same numbers at the same places and come out bit for
// bit equal.  A d2 that is not finite before its clamp sets *flag and is no
// term.
//
// tsne_forces_*: gridDim.x = strips * parts.  A workgroup owns a strip of 32
// rows, whose tables (diag, beta, m, 1/Z, y) it stages in LDS, and part p of
// the column tiles (64 columns, the split of knn_topk).  Lanes go across the
// columns: a lane keeps the tables of its column of the tile in registers and
// walks the 8 rows of its wave, so a wave reads 64 consecutive elements of K
// along the lane axis.  Per row it adds A = sum p w (y_i - y_j), R = sum w^2
// (y_i - y_j) over the pairs with w >= tau, z = sum w and the number of pairs
// with w < tau, w = 1 / (1 + |y_i - y_j|^2); the wave's butterfly ends the
// part, and part p of row i goes to F[(p n + i) (2 D + 2) ...].
//
// tau = 2 eps n (n - 1) >= eps Zq, so q_ij = max(w / Zq, eps) = w / Zq for
// every pair that R takes, and sum q w (y_i - y_j) = R / Zq.  The other pairs
// -- far outliers: |y_i - y_j| beyond 1 / sqrt(tau) -- need Zq, which this pass
// is still summing: tsne_update_* walks Y once more for the rows that counted
// any, with the same w from the same instructions (`weight`).
//
// tsne_update_*: a thread per row.  Zq = sum z in a fixed order (every
// workgroup for itself: the same bits), the parts in order, grad = 4 (a A - R /
// Zq - tail), then the gains, the momentum and the new Y, which goes to a
// second buffer: the tail walk of another row may still read the old one.  With
// grad_out the gradient is written and nothing else.  With g2 the squared norm
// of the row's gains-scaled gradient.
//
// tsne_zq, tsne_kl_*, tsne_look: what a look needs.  Zq to a word; the pass
// over the pairs again, a p log(max(a p, eps) / max(w / Zq, eps)) per row and
// part; and the two totals, with the flag word, for one download.
#ifndef GRAPHDOT_HIP_TSNE_H_
#define GRAPHDOT_HIP_TSNE_H_
#include "dense_reduce.h"

#define TS_ROWS 32              // rows per strip
#define TS_TILE 64              // columns per tile: one per lane
#define TS_OWN (TS_ROWS / NWAVE)        // rows per wave
#define TS_CAL_COLS 2048        // columns of a row that tsne_calibrate stages
#define TS_STEPS 100            // most steps of the bisection
#define TS_TOL 1e-5             // its tolerance on the entropy
#define TS_EPS 2.220446049250313e-16    // np.finfo(float).eps

namespace tsne {

__device__ __forceinline__ double wave_min(double v) {
    for (int off = WAVE / 2; off > 0; off >>= 1)
        v = fmin(v, __shfl_xor(v, off, WAVE));
    return v;
}

// d2 of a pair; +inf, and bad, if it is not finite before the clamp
__device__ __forceinline__ double dist2(double di, double dj, double k,
                                        bool &bad) {
    double d2 = (di + dj) - 2.0 * k;
    if (!is_finite(d2)) { bad = true; return __builtin_inf(); }
    return d2 < 0.0 ? 0.0 : d2;
}

// w = 1 / (1 + |yi - yj|^2) and dy = yi - yj.  The fmas are spelled out: the
// same bits wherever this is inlined (forces_stage and update_stage must agree
// on which pairs are below tau).
template <int D>
__device__ __forceinline__ double weight(const double *yi, const double *yj,
                                         double (&dy)[D]) {
    double s = 1.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        dy[c] = yi[c] - yj[c];
        s = fma(dy[c], dy[c], s);
    }
    return 1.0 / s;
}

// The sum of the 256 threads' v, to every thread: the butterfly, then the four
// waves in order.
__device__ __forceinline__ double block_total(double v) {
    __shared__ double red[NWAVE];
    v = wave_sum(v);
    __syncthreads();                          // (red may still be read)
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < NWAVE; ++w) t += red[w];
    return t;
}

// sum_b p[b], b strided over the threads
__device__ __forceinline__ double block_sum(const double *__restrict__ p,
                                            int64_t len) {
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < len; b += BLOCK) s += p[b];
    return block_total(s);
}

// Zq = sum_i sum_p z of F (parts, n, C): rows strided over the threads, the
// parts of a row in order
__device__ __forceinline__ double zq_total(const double *__restrict__ F,
                                           int64_t parts, int64_t n, int C) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += BLOCK) {
        double z = 0.0;
        for (int64_t p = 0; p < parts; ++p) z += F[(p * n + i) * C + C - 2];
        s += z;
    }
    return block_total(s);
}

// -- the calibration ---------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void calibrate_stage(
    const T *__restrict__ K, int64_t n, int64_t k_lane, int64_t k_col,
    const double *__restrict__ diag, double log_perplexity,
    double *__restrict__ beta_out, double *__restrict__ m_out,
    double *__restrict__ rz_out, int *__restrict__ steps_out,
    int *__restrict__ flag)
{
    __shared__ double rows[NWAVE][TS_CAL_COLS];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= n) return;                       // (whole waves; no barrier below)
    double *row = rows[wid];
    const bool staged = n <= TS_CAL_COLS;
    const double inf = __builtin_inf();
    const double di = diag[i];
    const T *Ki = K + i * k_col;
    bool bad = false;

    double mn = inf;
    for (int64_t j = lane; j < n; j += WAVE) {
        double d2 = inf;
        if (j != i) d2 = dist2(di, diag[j], (double)Ki[j * k_lane], bad);
        if (staged) row[j] = d2;
        mn = fmin(mn, d2);
    }
    mn = wave_min(mn);
    if (staged)
        for (int64_t j = lane; j < n; j += WAVE) row[j] -= mn;

    double beta = 1.0, lo = -inf, hi = inf, Z = 0.0;
    int steps = 0;
    for (;;) {
        double z = 0.0, s = 0.0, c0 = 0.0;
        for (int64_t j = lane; j < n; j += WAVE) {
            double r = inf;
            if (staged) {
                r = row[j];
            } else if (j != i) {
                bool again = false;
                r = dist2(di, diag[j], (double)Ki[j * k_lane], again) - mn;
            }
            if (r == 0.0) {
                c0 += 1.0;
            } else if (r < inf) {
                const double e = exp(-beta * r);
                z += e;
                s += r * e;
            }
        }
        // (every lane gets the same bits: the loop below is uniform)
        Z = wave_sum(c0) + wave_sum(z);
        const double H = log(Z) + beta * wave_sum(s) / Z;
        const double diff = H - log_perplexity;
        if (fabs(diff) <= TS_TOL) break;
        if (++steps == TS_STEPS) break;
        if (diff > 0.0) {
            lo = beta;
            beta = hi == inf ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = lo == -inf ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    if (lane == 0) {
        beta_out[i] = beta;
        m_out[i] = mn;
        rz_out[i] = 1.0 / Z;
        steps_out[i] = steps;
    }
    if (bad) *flag = 1;
}

// -- the pass over the pairs -------------------------------------------------------
#define TS_RT (4 + D)           // doubles per row of the staged tables

// One pass of a workgroup over its strip and its part of the tiles: `pair(r,
// p, w, dy)` for every pair (row0 + wid TS_OWN + r, j != i) with j in the
// part, lane l at the columns l mod 64.
template <typename T, int D, typename Pair>
__device__ __forceinline__ void walk(
    const T *__restrict__ K, int64_t n, int64_t k_lane, int64_t k_col,
    const double *__restrict__ diag, const double *__restrict__ beta,
    const double *__restrict__ m, const double *__restrict__ rz,
    const double *__restrict__ Y, int64_t parts, Pair pair)
{
    __shared__ double rt[TS_ROWS][TS_RT];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t strip = blockIdx.x / parts, part = blockIdx.x % parts;
    const int64_t row0 = strip * TS_ROWS;
    const int64_t tiles = (n + TS_TILE - 1) / TS_TILE;
    const int64_t tpp = (tiles + parts - 1) / parts;
    const int64_t t0 = part * tpp;
    const int64_t t1 = t0 + tpp < tiles ? t0 + tpp : tiles;
    const double two_n = 2.0 * (double)n;

    for (int x = threadIdx.x; x < TS_ROWS * TS_RT; x += BLOCK) {
        const int r = x / TS_RT, c = x % TS_RT;
        const int64_t i = row0 + r;
        double v = 0.0;
        if (i < n)
            v = c == 0 ? diag[i] : c == 1 ? beta[i] : c == 2 ? m[i]
                : c == 3 ? rz[i] : Y[i * D + (c - 4)];
        rt[r][c] = v;
    }
    __syncthreads();

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j = t * TS_TILE + lane;
        if (j >= n) continue;
        const double dj = diag[j], bj = beta[j], mj = m[j], zj = rz[j];
        double yj[D];
#pragma unroll
        for (int c = 0; c < D; ++c) yj[c] = Y[j * D + c];
#pragma unroll
        for (int r = 0; r < TS_OWN; ++r) {
            const double *ri = rt[wid * TS_OWN + r];
            const int64_t i = row0 + wid * TS_OWN + r;
            if (i >= n || i == j) continue;
            bool bad = false;
            const double d2 = dist2(ri[0], dj, (double)K[j * k_lane + i * k_col],
                                    bad);
            const double ei = exp(-ri[1] * (d2 - ri[2])) * ri[3];
            const double ej = exp(-bj * (d2 - mj)) * zj;
            const double p = fmax((ei + ej) / two_n, TS_EPS);
            double dy[D];
            const double w = weight<D>(ri + 4, yj, dy);
            pair(r, p, w, dy);
        }
    }
}

template <typename T, int D>
__device__ __forceinline__ void forces_stage(
    const T *__restrict__ K, int64_t n, int64_t k_lane, int64_t k_col,
    const double *__restrict__ diag, const double *__restrict__ beta,
    const double *__restrict__ m, const double *__restrict__ rz,
    const double *__restrict__ Y, int64_t parts, double tau,
    double *__restrict__ F)
{
    constexpr int C = 2 * D + 2;
    double acc[TS_OWN][C];
#pragma unroll
    for (int r = 0; r < TS_OWN; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[r][c] = 0.0;
    walk<T, D>(K, n, k_lane, k_col, diag, beta, m, rz, Y, parts,
               [&](int r, double p, double w, const double (&dy)[D]) {
        const double pw = p * w, ww = w >= tau ? w * w : 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            acc[r][c] += pw * dy[c];
            acc[r][D + c] += ww * dy[c];
        }
        acc[r][2 * D] += w;
        acc[r][2 * D + 1] += w >= tau ? 0.0 : 1.0;
    });
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t strip = blockIdx.x / parts, part = blockIdx.x % parts;
#pragma unroll
    for (int r = 0; r < TS_OWN; ++r) {
        const int64_t i = strip * TS_ROWS + wid * TS_OWN + r;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double v = wave_sum(acc[r][c]);
            if (lane == 0 && i < n) F[(part * n + i) * C + c] = v;
        }
    }
}

template <typename T, int D>
__device__ __forceinline__ void kl_stage(
    const T *__restrict__ K, int64_t n, int64_t k_lane, int64_t k_col,
    const double *__restrict__ diag, const double *__restrict__ beta,
    const double *__restrict__ m, const double *__restrict__ rz,
    const double *__restrict__ Y, int64_t parts, double a,
    const double *__restrict__ zq, double *__restrict__ klp)
{
    const double Zq = *zq;
    double acc[TS_OWN];
#pragma unroll
    for (int r = 0; r < TS_OWN; ++r) acc[r] = 0.0;
    walk<T, D>(K, n, k_lane, k_col, diag, beta, m, rz, Y, parts,
               [&](int r, double p, double w, const double (&dy)[D]) {
        const double ap = a * p;
        acc[r] += ap * log(fmax(ap, TS_EPS) / fmax(w / Zq, TS_EPS));
    });
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t strip = blockIdx.x / parts, part = blockIdx.x % parts;
#pragma unroll
    for (int r = 0; r < TS_OWN; ++r) {
        const int64_t i = strip * TS_ROWS + wid * TS_OWN + r;
        const double v = wave_sum(acc[r]);
        if (lane == 0 && i < n) klp[part * n + i] = v;
    }
}

// -- the step ----------------------------------------------------------------------
// gridDim.x = ceil(n / BLOCK)
template <int D>
__device__ __forceinline__ void update_stage(
    const double *__restrict__ F, int64_t parts, int64_t n,
    const double *__restrict__ Y, double *__restrict__ Y_new,
    double *__restrict__ update, double *__restrict__ gains, double a,
    double momentum, double learning_rate, double tau,
    double *__restrict__ grad_out, double *__restrict__ g2)
{
    constexpr int C = 2 * D + 2;
    const double Zq = zq_total(F, parts, n, C);
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double A[D], R[D], tail = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) A[c] = R[c] = 0.0;
    for (int64_t p = 0; p < parts; ++p) {
        const double *f = F + (p * n + i) * C;
#pragma unroll
        for (int c = 0; c < D; ++c) { A[c] += f[c]; R[c] += f[D + c]; }
        tail += f[2 * D + 1];
    }
    double yi[D], corr[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { yi[c] = Y[i * D + c]; corr[c] = 0.0; }
    if (tail > 0.0) {
        // the pairs of this row that forces_stage left out of R: those whose
        // q may be the clamp
        for (int64_t j = 0; j < n; ++j) {
            if (j == i) continue;
            double yj[D], dy[D];
#pragma unroll
            for (int c = 0; c < D; ++c) yj[c] = Y[j * D + c];
            const double w = weight<D>(yi, yj, dy);
            if (w >= tau) continue;
            const double qw = fmax(w / Zq, TS_EPS) * w;
#pragma unroll
            for (int c = 0; c < D; ++c) corr[c] += qw * dy[c];
        }
    }
    double sq = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const double g = 4.0 * ((a * A[c] - R[c] / Zq) - corr[c]);
        if (grad_out) { grad_out[i * D + c] = g; continue; }
        const double u = update[i * D + c];
        double gain = gains[i * D + c];
        gain = u * g < 0.0 ? gain + 0.2 : gain * 0.8;
        gain = gain < 0.01 ? 0.01 : gain;
        const double gg = gain * g;
        const double nu = momentum * u - learning_rate * gg;
        gains[i * D + c] = gain;
        update[i * D + c] = nu;
        Y_new[i * D + c] = yi[c] + nu;
        sq += gg * gg;
    }
    if (g2) g2[i] = sq;
}

}  // namespace tsne

// -- the kernels -------------------------------------------------------------------
#define TS_CAL_PARAMS(T)                                                       \
    const T *K, int64_t n, int64_t k_lane, int64_t k_col, const double *diag,  \
    double log_perplexity, double *beta, double *m, double *rz, int *steps,    \
    int *flag
#define TS_CAL_ARGS K, n, k_lane, k_col, diag, log_perplexity, beta, m, rz,    \
    steps, flag
#define TS_PASS_PARAMS(T)                                                      \
    const T *K, int64_t n, int64_t k_lane, int64_t k_col, const double *diag,  \
    const double *beta, const double *m, const double *rz, const double *Y,    \
    int64_t parts
#define TS_PASS_ARGS K, n, k_lane, k_col, diag, beta, m, rz, Y, parts
#define TS_UPDATE_PARAMS                                                       \
    const double *F, int64_t parts, int64_t n, const double *Y, double *Y_new, \
    double *update, double *gains, double a, double momentum,                  \
    double learning_rate, double tau, double *grad_out, double *g2
#define TS_UPDATE_ARGS F, parts, n, Y, Y_new, update, gains, a, momentum,      \
    learning_rate, tau, grad_out, g2

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_calibrate_f32(TS_CAL_PARAMS(float))
{
    tsne::calibrate_stage<float>(TS_CAL_ARGS);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_calibrate_f64(TS_CAL_PARAMS(double))
{
    tsne::calibrate_stage<double>(TS_CAL_ARGS);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_forces_f32_d2(TS_PASS_PARAMS(float), double tau, double *F)
{
    tsne::forces_stage<float, 2>(TS_PASS_ARGS, tau, F);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_forces_f64_d2(TS_PASS_PARAMS(double), double tau, double *F)
{
    tsne::forces_stage<double, 2>(TS_PASS_ARGS, tau, F);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_forces_f32_d3(TS_PASS_PARAMS(float), double tau, double *F)
{
    tsne::forces_stage<float, 3>(TS_PASS_ARGS, tau, F);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_forces_f64_d3(TS_PASS_PARAMS(double), double tau, double *F)
{
    tsne::forces_stage<double, 3>(TS_PASS_ARGS, tau, F);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_kl_f32_d2(TS_PASS_PARAMS(float), double a, const double *zq, double *klp)
{
    tsne::kl_stage<float, 2>(TS_PASS_ARGS, a, zq, klp);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_kl_f64_d2(TS_PASS_PARAMS(double), double a, const double *zq, double *klp)
{
    tsne::kl_stage<double, 2>(TS_PASS_ARGS, a, zq, klp);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_kl_f32_d3(TS_PASS_PARAMS(float), double a, const double *zq, double *klp)
{
    tsne::kl_stage<float, 3>(TS_PASS_ARGS, a, zq, klp);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_kl_f64_d3(TS_PASS_PARAMS(double), double a, const double *zq, double *klp)
{
    tsne::kl_stage<double, 3>(TS_PASS_ARGS, a, zq, klp);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_update_d2(TS_UPDATE_PARAMS)
{
    tsne::update_stage<2>(TS_UPDATE_ARGS);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_update_d3(TS_UPDATE_PARAMS)
{
    tsne::update_stage<3>(TS_UPDATE_ARGS);
}

// gridDim.x = 1: Zq of the partial sums F (parts, n, C) to *zq
extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_zq(const double *F, int64_t parts, int64_t n, int C, double *zq)
{
    const double t = tsne::zq_total(F, parts, n, C);
    if (threadIdx.x == 0) *zq = t;
}

// gridDim.x = 1: out[0] = sum klp, out[1] = sum g2 (0 of them: 0), out[2] =
// the flag word
extern "C" __global__ __launch_bounds__(BLOCK) void
tsne_look(const double *klp, int64_t n_kl, const double *g2, int64_t n_g2,
          const int *flag, double *out)
{
    const double kl = tsne::block_sum(klp, n_kl);
    const double sq = tsne::block_sum(g2, n_g2);
    if (threadIdx.x == 0) {
        out[0] = kl;
        out[1] = sq;
        out[2] = (double)*flag;
    }
}

#endif
