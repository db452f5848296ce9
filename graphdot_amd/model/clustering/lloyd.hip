// Kernel k-means (Lloyd's iteration in the feature space of a kernel) on the
// Gram matrix alone (kkmeans.py; the host side is _lloyd.py; DESIGN.md section
// 28).  K is n x n, symmetric, float or double, contiguous along either index
// (symmetric: read as it lies).  All R restarts advance in the same launches:
// labels are (R, n) int32 in {0..k-1}, k <= 64.  With n_c the size of cluster c,
//
//   S[i, c] = sum_{j: lab[j] = c} K[i, j]        T[c] = sum_{i: lab[i] = c} S[i, c]
//   d2(i, c) = K[i, i] - 2 S[i, c] / n_c + T[c] / n_c^2
//
// and one round is
//
//   kkm_accumulate_* -> kkm_assign_* -> kkm_reduce
//
// kkm_seed_{f32,f64}: one workgroup per restart chooses k seed samples and
// labels every sample with its nearest seed (the lowest cluster on a tie).
// mind[i] is the squared distance of sample i to its nearest seed so far,
// (K_ii + K_jj) - 2 K_ij clamped at 0.  Seed 0 is floor(u_0 n).  Mode 0
// (k-means++): seed t is the smallest i whose inclusive prefix sum of mind
// exceeds u_t total; the prefix of i is off[w] + (the sum of the thread's
// span up to i), off[w] the sum of the spans of the threads before w, in
// order; total is the prefix of n - 1.  If total is not positive: the lowest
// index not chosen yet.  Mode 1 (farthest): argmax mind, the lowest index on a
// tie.  Mode 2: the seeds are given.
// kkm_accumulate_{f32,f64}_k{KC}: S for ROWS = 16 rows of K and one chunk of KC
// clusters per workgroup; each of the four waves keeps RW = 4 rows x KC double
// accumulators in registers and adds an entry of K to the accumulator whose
// cluster is the label of its column by a compare and select per accumulator:
// no one-hot matrix, no indexed registers (float4 / double2 loads of K when n
// is a multiple of the vector, single elements otherwise: `n % VEC` decides,
// nothing else).  Per row block rb it writes
//   part[r][rb] = [share of T (k) | share of the counts (k)]
// restricted to its rows (its chunk of the clusters of each).
// kkm_assign_{f32,f64}: a thread per sample.  Adds the shares of T and of the
// counts up in order, forms d2 and its argmin (the lowest cluster on a tie; an
// empty cluster never attracts a sample) and writes the next labels; per
// workgroup the shares apart[r] = [changed labels | inertia of the labels used
// | a K_ii or S that is not finite] (each nab).
// kkm_reduce: info[r] = [changed, inertia, status (sticky), the first round in
// which nothing changed].
// kkm_predict_{f32,f64}_k{KC}: -2 S_zc / n_c + T_c / n_c^2 and its argmin for the
// rows of a (b, n) cross matrix with any strides, a lane per row, the n terms
// split over the four waves in order, KC clusters per pass.
//
// Every grid is a function of the shapes alone, every sum runs in a fixed order
// (wave_sum of dense_reduce.h where a wave adds its lanes) and there are no
// atomics: the same bits on every call.
#include "dense_reduce.h"

#define KMAX 64                  // most clusters
#define ROWS 16                  // rows of K per workgroup of kkm_accumulate
#define RW (ROWS / NWAVE)        // rows per wave, all at once
#define EPS 2.220446049250313e-16

// gridDim.x = R
template <typename T>
__device__ __forceinline__ void seed_stage(
    const T *__restrict__ K, int64_t n, int k, int mode,
    const double *__restrict__ u, int *__restrict__ seeds,
    int *__restrict__ lab, double *__restrict__ mind)
{
    __shared__ double part[BLOCK], off[BLOCK];
    __shared__ int64_t cand[BLOCK];
    __shared__ int64_t chosen[KMAX];
    __shared__ double target;
    __shared__ int64_t cur;
    const int t = threadIdx.x;
    u += (int64_t)blockIdx.x * k;
    seeds += (int64_t)blockIdx.x * k;
    lab += (int64_t)blockIdx.x * n;
    mind += (int64_t)blockIdx.x * n;
    const int64_t span = (n + BLOCK - 1) / BLOCK;
    const int64_t i0 = min(n, t * span), i1 = min(n, i0 + span);

    for (int s = 0; s < k; ++s) {
        if (mode == 2 || s == 0) {
            if (t == 0) {
                int64_t j = mode == 2 ? (int64_t)seeds[s]
                                      : (int64_t)(u[0] * (double)n);
                cur = j < 0 ? 0 : (j < n ? j : n - 1);
            }
        } else if (mode == 1) {
            double bm = -1.0;
            int64_t bi = 0;
            for (int64_t i = i0; i < i1; ++i) {
                const double m = mind[i];
                if (m > bm) { bm = m; bi = i; }
            }
            part[t] = bm;
            cand[t] = bi;
            __syncthreads();
            if (t == 0) {
                bm = -1.0;
                bi = 0;
                for (int w = 0; w < BLOCK; ++w)
                    if (part[w] > bm) { bm = part[w]; bi = cand[w]; }
                cur = bi;
            }
        } else {
            double loc = 0.0;
            for (int64_t i = i0; i < i1; ++i) loc += mind[i];
            part[t] = loc;
            __syncthreads();
            if (t == 0) {
                double run = 0.0;
                for (int w = 0; w < BLOCK; ++w) {
                    off[w] = run;
                    run += part[w];
                }
                double x = u[s] * run;
                if (!(x < run)) x = run * (1.0 - EPS);
                // (no prefix exceeds a NaN: the lowest index not chosen)
                target = run > 0.0 ? x : __builtin_nan("");
            }
            __syncthreads();
            const double x = target, base = off[t];
            int64_t c = n;
            loc = 0.0;
            for (int64_t i = i0; i < i1; ++i) {
                loc += mind[i];
                if (base + loc > x) { c = i; break; }
            }
            cand[t] = c;
            __syncthreads();
            if (t == 0) {
                int64_t j = n;
                for (int w = 0; w < BLOCK && j == n; ++w) j = cand[w];
                if (j == n) {
                    for (j = 0; j < n - 1; ++j) {
                        bool used = false;
                        for (int a = 0; a < s; ++a) used |= chosen[a] == j;
                        if (!used) break;
                    }
                }
                cur = j;
            }
        }
        __syncthreads();
        const int64_t j = cur;
        if (t == 0) {
            chosen[s] = j;
            seeds[s] = (int)j;
        }
        const double djj = (double)K[j * n + j];
        const T *kj = K + j * n;
        for (int64_t i = t; i < n; i += BLOCK) {
            double d = ((double)K[i * n + i] + djj) - 2.0 * (double)kj[i];
            d = d > 0.0 ? d : 0.0;
            if (s == 0 || d < mind[i]) {
                mind[i] = d;
                lab[i] = s;
            }
        }
        __syncthreads();
    }
}

extern "C" __global__ __launch_bounds__(BLOCK) void
kkm_seed_f32(const float *K, int64_t n, int k, int mode, const double *u,
             int *seeds, int *lab, double *mind) {
    seed_stage<float>(K, n, k, mode, u, seeds, lab, mind);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
kkm_seed_f64(const double *K, int64_t n, int k, int mode, const double *u,
             int *seeds, int *lab, double *mind) {
    seed_stage<double>(K, n, k, mode, u, seeds, lab, mind);
}

// lane l takes columns j = VEC (l + 64 t) + v
template <typename T, int KC, int VEC>
__device__ __forceinline__ void accumulate_rows(
    const T *(&row)[RW], const int *__restrict__ lab, int64_t n, int c0,
    double (&acc)[RW][KC])
{
    const int lane = threadIdx.x % WAVE;
    for (int64_t j = (int64_t)lane * VEC; j < n; j += WAVE * VEC) {
        double kv[RW][VEC];          // (n % VEC == 0: whole vectors)
        int l[VEC];
#pragma unroll
        for (int r = 0; r < RW; ++r) load_k<T, VEC>(row[r] + j, kv[r]);
#pragma unroll
        for (int v = 0; v < VEC; ++v) l[v] = lab[j + v] - c0;
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const bool hit = l[v] == kk;
#pragma unroll
                for (int r = 0; r < RW; ++r)
                    acc[r][kk] += hit ? kv[r][v] : 0.0;
            }
        }
    }
}

// gridDim.x = R * ceil(k / KC) * nrb, nrb = ceil(n / ROWS)
template <typename T, int KC>
__device__ __forceinline__ void accumulate_stage(
    const T *__restrict__ K, int64_t n, int k, const int *__restrict__ lab,
    double *__restrict__ S, double *__restrict__ part)
{
    constexpr int VEC = 16 / sizeof(T);
    __shared__ double Zs[ROWS][KC];
    __shared__ int lrow[ROWS];
    const int64_t nrb = (n + ROWS - 1) / ROWS;
    const int nch = (k + KC - 1) / KC;
    const int64_t rb = blockIdx.x % nrb, q = blockIdx.x / nrb;
    const int c0 = (int)(q % nch) * KC;
    const int64_t rs = q / nch;
    const int nk = min(KC, k - c0);
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    lab += rs * n;
    S += rs * n * k;
    part += (rs * nrb + rb) * 2 * k;

    const T *row[RW];
    bool valid[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int64_t i = rb * ROWS + wid * RW + r;
        valid[r] = i < n;
        row[r] = K + (valid[r] ? i : 0) * n;     // (in bounds either way)
    }
    double acc[RW][KC];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) acc[r][kk] = 0.0;
    if (VEC > 1 && n % VEC == 0)
        accumulate_rows<T, KC, VEC>(row, lab, n, c0, acc);
    else
        accumulate_rows<T, KC, 1>(row, lab, n, c0, acc);
#pragma unroll
    for (int r = 0; r < RW; ++r) {
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            const double z = wave_sum(acc[r][kk]);
            if (lane == 0 && kk < nk) {
                Zs[wid * RW + r][kk] = valid[r] ? z : 0.0;
                if (valid[r])
                    S[(rb * ROWS + wid * RW + r) * k + c0 + kk] = z;
            }
        }
    }
    if (threadIdx.x < ROWS) {
        const int64_t i = rb * ROWS + threadIdx.x;
        lrow[threadIdx.x] = i < n ? lab[i] : -1;
    }
    __syncthreads();
    if ((int)threadIdx.x < nk) {
        const int c = c0 + threadIdx.x;
        double t = 0.0, cnt = 0.0;
        for (int r = 0; r < ROWS; ++r) {
            const bool hit = lrow[r] == c;
            t += hit ? Zs[r][threadIdx.x] : 0.0;
            cnt += hit ? 1.0 : 0.0;
        }
        part[c] = t;
        part[k + c] = cnt;
    }
}

#define ACCUMULATE(T, SFX, KC)                                                 \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    kkm_accumulate_##SFX##_k##KC(const T *K, int64_t n, int k, const int *lab, \
                                 double *S, double *part) {                    \
        accumulate_stage<T, KC>(K, n, k, lab, S, part);                        \
    }

ACCUMULATE(float, f32, 1)
ACCUMULATE(float, f32, 2)
ACCUMULATE(float, f32, 4)
ACCUMULATE(float, f32, 8)
ACCUMULATE(float, f32, 16)
ACCUMULATE(double, f64, 1)
ACCUMULATE(double, f64, 2)
ACCUMULATE(double, f64, 4)
ACCUMULATE(double, f64, 8)
ACCUMULATE(double, f64, 16)

// sum over the workgroup in thread 0 (the butterfly, then the four waves in
// order); `red` is one row of NWAVE
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < NWAVE; ++w) t += red[w];
    return t;
}

// gridDim.x = R * nab, nab = ceil(n / BLOCK)
template <typename T>
__device__ __forceinline__ void assign_stage(
    const T *__restrict__ K, int64_t n, int k, const int *__restrict__ lab,
    const double *__restrict__ S, const double *__restrict__ part,
    int64_t nrb, int *__restrict__ next, double *__restrict__ apart)
{
    __shared__ double Tq[KMAX], cnt[KMAX], red[3][NWAVE];
    const int64_t nab = (n + BLOCK - 1) / BLOCK;
    const int64_t rs = blockIdx.x / nab, b = blockIdx.x % nab;
    if ((int)threadIdx.x < k) {
        const double *p = part + rs * nrb * 2 * k + threadIdx.x;
        double t = 0.0, c = 0.0;
        for (int64_t rb = 0; rb < nrb; ++rb) {
            t += p[rb * 2 * k];
            c += p[rb * 2 * k + k];
        }
        cnt[threadIdx.x] = c;
        Tq[threadIdx.x] = c > 0.0 ? t / (c * c) : 0.0;
    }
    __syncthreads();
    const int64_t i = b * BLOCK + threadIdx.x;
    double changed = 0.0, share = 0.0, bad = 0.0;
    if (i < n) {
        const double dii = (double)K[i * n + i];
        const int li = lab[rs * n + i];
        const double *s = S + (rs * n + i) * k;
        double best = __builtin_inf(), own = 0.0;
        int bc = 0;
        bool ok = is_finite(dii);
        for (int c = 0; c < k; ++c) {
            const double sc = s[c], nc = cnt[c];
            ok &= is_finite(sc);
            if (nc > 0.0) {
                const double q = sc / nc;
                const double d = dii - 2.0 * q + Tq[c];
                if (c == li) own = q;
                if (d < best) { best = d; bc = c; }
            }
        }
        next[rs * n + i] = bc;
        changed = bc != li ? 1.0 : 0.0;
        share = dii - own;
        bad = ok ? 0.0 : 1.0;
    }
    changed = block_sum(changed, red[0]);
    share = block_sum(share, red[1]);
    bad = block_sum(bad, red[2]);
    if (threadIdx.x == 0) {
        apart[(rs * 3 + 0) * nab + b] = changed;
        apart[(rs * 3 + 1) * nab + b] = share;
        apart[(rs * 3 + 2) * nab + b] = bad;
    }
}

extern "C" __global__ __launch_bounds__(BLOCK) void
kkm_assign_f32(const float *K, int64_t n, int k, const int *lab,
               const double *S, const double *part, int64_t nrb, int *next,
               double *apart) {
    assign_stage<float>(K, n, k, lab, S, part, nrb, next, apart);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
kkm_assign_f64(const double *K, int64_t n, int k, const int *lab,
               const double *S, const double *part, int64_t nrb, int *next,
               double *apart) {
    assign_stage<double>(K, n, k, lab, S, part, nrb, next, apart);
}

// info[r] = [changed, inertia, status, stamp]; gridDim.x = R
extern "C" __global__ __launch_bounds__(BLOCK) void
kkm_reduce(const double *__restrict__ apart, int64_t nab, int round,
           double *__restrict__ info)
{
    __shared__ double red[NWAVE];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    double s = 0.0;
    if (wid < 3) {
        const double *p = apart + ((int64_t)blockIdx.x * 3 + wid) * nab;
        for (int64_t b = lane; b < nab; b += WAVE) s += p[b];
    }
    s = wave_sum(s);
    if (lane == 0) red[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double *out = info + (int64_t)blockIdx.x * 4;
        const bool status = out[2] != 0.0 || red[2] != 0.0;
        out[0] = red[0];
        out[1] = red[1];
        out[2] = status ? 1.0 : 0.0;
        if (out[3] == 0.0 && red[0] == 0.0 && !status) out[3] = (double)round;
    }
}

// Ks[z s_z + i s_i]; out (b, k) row-major; gridDim.x = ceil(b / WAVE)
template <typename T, int KC>
__device__ __forceinline__ void predict_stage(
    const T *__restrict__ Ks, int64_t b, int64_t n, int64_t s_z, int64_t s_i,
    const int *__restrict__ lab, const double *__restrict__ Tc,
    const double *__restrict__ cnt, int k, double *__restrict__ out,
    int *__restrict__ arg)
{
    __shared__ double sh[NWAVE][KC][WAVE];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t z = (int64_t)blockIdx.x * WAVE + lane;
    const int64_t span = (n + NWAVE - 1) / NWAVE;
    const int64_t i0 = min(n, wid * span), i1 = min(n, i0 + span);
    const T *p = Ks + (z < b ? z : 0) * s_z;
    double best = __builtin_inf();
    int bc = 0;
    for (int c0 = 0; c0 < k; c0 += KC) {
        double acc[KC];
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;
        for (int64_t i = i0; i < i1; ++i) {
            const double ks = (double)p[i * s_i];
            const int l = lab[i] - c0;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) acc[kk] += l == kk ? ks : 0.0;
        }
        __syncthreads();                 // (the pass before is used up)
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) sh[wid][kk][lane] = acc[kk];
        __syncthreads();
        if (wid == 0 && z < b) {
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) {
                if (c0 + kk < k) {
                    double s = 0.0;
                    for (int w = 0; w < NWAVE; ++w) s += sh[w][kk][lane];
                    const double nc = cnt[c0 + kk];
                    const double d = nc > 0.0
                        ? -2.0 * (s / nc) + Tc[c0 + kk] / (nc * nc)
                        : __builtin_inf();
                    out[z * k + c0 + kk] = d;
                    if (d < best) { best = d; bc = c0 + kk; }
                }
            }
        }
    }
    if (wid == 0 && z < b) arg[z] = bc;
}

#define PREDICT(T, SFX, KC)                                                    \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    kkm_predict_##SFX##_k##KC(const T *Ks, int64_t b, int64_t n, int64_t s_z,  \
                              int64_t s_i, const int *lab, const double *Tc,   \
                              const double *cnt, int k, double *out,           \
                              int *arg) {                                      \
        predict_stage<T, KC>(Ks, b, n, s_z, s_i, lab, Tc, cnt, k, out, arg);   \
    }

PREDICT(float, f32, 1)
PREDICT(float, f32, 2)
PREDICT(float, f32, 4)
PREDICT(float, f32, 8)
PREDICT(float, f32, 16)
PREDICT(double, f64, 1)
PREDICT(double, f64, 2)
PREDICT(double, f64, 4)
PREDICT(double, f64, 8)
PREDICT(double, f64, 16)
