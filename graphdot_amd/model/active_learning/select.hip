// Greedy subset selection on a symmetric kernel matrix K (N x N, column-major,
// float or double, read as it is stored; every sum in double) for the active
// learning selectors of model/active_learning (_select.py drives the loop).
//
// DeterminantMaximizer -- implicit row Gram-Schmidt.  The reference's update
// K -= (K v) v^T projects every row of K off the chosen row; here K is never
// written.  Orthonormal directions Q (N x n), coefficients C = Q^T K (n x N,
// row t at C + t N) and residual norms rho_a = |K_a|^2 - sum_t C_ta^2.  Step s
// (pivot i = picks[s]):
//   al_dm_direction   w = K_i - Q C_:,i into Q_:,s, |w| from w itself
//   al_colreduce      C_s,: = K w / |w|                   (the one N^2 read)
//   al_update_argmax  Q_:,s /= |w|, rho -= C_s,:^2, masked argmax -> picks[s+1]
//
// VarianceMinimizer -- partial pivoted Cholesky of K + alpha I with the row
// sums of the posterior over the unchosen set U as the criterion s_a.  Step s
// (pivot j = picks[s]):
//   al_vm_column      p = K_:,j + alpha e_j - L L_j,:^T,  l = p / sqrt(p_j)
//                     into L_:,s, sum of l over U \ {j} in per-block partials
//   al_update_argmax  s_a -= p_a + l_a sum_{U\{j}} l, masked argmax
//
// The pivot stays in device memory (picks[]); no kernel needs the host.  The
// argmax keeps the largest criterion and, among equal values, the smallest
// index.  A sample whose criterion is NaN is passed over like a chosen one --
// never picked, and hiding no other, whichever lane holds it -- and when only
// such samples are left the status word says so (the rule of
// _greedy._argmax).  A pivot whose residual is not above `tol` times its own
// size sets the status word and every later launch returns at once.
#include "dense_reduce.h"

#define CHUNK 1024   // coefficients staged in LDS per pass

enum { ST_OK = 0, ST_DM_RESIDUAL = 1, ST_VM_RESIDUAL = 2, ST_NO_CANDIDATE = 3 };

__device__ __forceinline__ double ld_agent(const double *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_agent(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int *p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sum over the block (every thread gets it); `red` holds BLOCK / WAVE doubles
__device__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < BLOCK / WAVE; ++k) t += red[k];
    return t;
}

// (value, index) order of the argmax: larger value first, then smaller index.
// idx < 0 is "none"; a NaN candidate never wins, and a NaN incumbent (a lane
// starts from its own criterion) loses to every candidate that is not NaN
__device__ __forceinline__ bool better(double v, int i, double bv, int bi) {
    if (i < 0 || v != v) return false;
    if (bi < 0 || bv != bv) return true;
    return v > bv || (v == bv && i < bi);
}

__device__ __forceinline__ void wave_argmax(double &v, int &i) {
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, WAVE);
        const int oi = __shfl_xor(i, off, WAVE);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

__device__ void block_argmax(double &v, int &i, double *rv, int *ri) {
    wave_argmax(v, i);
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    __syncthreads();
    if (lane == 0) { rv[wid] = v; ri[wid] = i; }
    __syncthreads();
    v = rv[0]; i = ri[0];
    for (int k = 1; k < BLOCK / WAVE; ++k)
        if (better(rv[k], ri[k], v, i)) { v = rv[k]; i = ri[k]; }
}

// One wave per column a of K (= row a, K symmetric):
//   mode 0: out[a] = scal[0] * sum_b K_ba w_b    (GEMV, w = Q_:,s unscaled)
//   mode 1: out[a] = sum_b K_ba^2
//   mode 2: out[a] = sum_b K_ba + alpha
template <typename T>
__device__ void colreduce(const T *__restrict__ K, int N, int mode, double alpha,
                          const double *__restrict__ w, const double *scal,
                          const int *status, double *__restrict__ out) {
    if (*status != ST_OK) return;
    const int a = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (a >= N) return;
    const T *col = K + (size_t)a * N;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int b = lane;
    if (mode == 0) {
        for (; b + 3 * WAVE < N; b += 4 * WAVE) {
            s0 += (double)col[b] * w[b];
            s1 += (double)col[b + WAVE] * w[b + WAVE];
            s2 += (double)col[b + 2 * WAVE] * w[b + 2 * WAVE];
            s3 += (double)col[b + 3 * WAVE] * w[b + 3 * WAVE];
        }
        for (; b < N; b += WAVE) s0 += (double)col[b] * w[b];
    } else if (mode == 1) {
        for (; b + 3 * WAVE < N; b += 4 * WAVE) {
            const double k0 = col[b], k1 = col[b + WAVE],
                         k2 = col[b + 2 * WAVE], k3 = col[b + 3 * WAVE];
            s0 += k0 * k0; s1 += k1 * k1; s2 += k2 * k2; s3 += k3 * k3;
        }
        for (; b < N; b += WAVE) { const double k0 = col[b]; s0 += k0 * k0; }
    } else {
        for (; b + 3 * WAVE < N; b += 4 * WAVE) {
            s0 += (double)col[b]; s1 += (double)col[b + WAVE];
            s2 += (double)col[b + 2 * WAVE]; s3 += (double)col[b + 3 * WAVE];
        }
        for (; b < N; b += WAVE) s0 += (double)col[b];
    }
    const double s = wave_sum((s0 + s1) + (s2 + s3));
    if (lane == 0)
        out[a] = mode == 0 ? s * scal[0] : (mode == 2 ? s + alpha : s);
}

// DeterminantMaximizer, first kernel of step s (grid: ceil(N / BLOCK)).
// Q_a,s = K_a,i - sum_{t<s} Q_a,t C_t,i; the last block to finish reduces the
// per-block sums of w^2 and K_i^2 and writes scal[0] = 1 / |w|, or the status.
template <typename T>
__device__ void dm_direction(const T *__restrict__ K, int N, int s, double tol,
                             double *__restrict__ Q, const double *__restrict__ C,
                             const int *picks, int *status, double *partials,
                             int *counter, double *scal) {
    __shared__ double coef[CHUNK];
    __shared__ double red[BLOCK / WAVE];
    __shared__ bool last;
    if (*status != ST_OK) return;
    const int i = picks[s];
    const int a = blockIdx.x * BLOCK + threadIdx.x;
    double w = (a < N) ? (double)K[(size_t)i * N + a] : 0.0;
    const double k = w;
    for (int t0 = 0; t0 < s; t0 += CHUNK) {
        const int m = min(CHUNK, s - t0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += BLOCK)
            coef[t] = C[(size_t)(t0 + t) * N + i];
        __syncthreads();
        if (a < N)
            for (int t = 0; t < m; ++t)
                w -= Q[(size_t)(t0 + t) * N + a] * coef[t];
    }
    if (a < N) Q[(size_t)s * N + a] = w;
    const double w2 = block_sum(w * w, red);
    const double k2 = block_sum(k * k, red);
    if (threadIdx.x == 0) {
        st_agent(partials + 2 * blockIdx.x, w2);
        st_agent(partials + 2 * blockIdx.x + 1, k2);
        __threadfence();
        last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    double sw = 0.0, sk = 0.0;
    for (int g = 0; g < (int)gridDim.x; ++g) {
        sw += ld_agent(partials + 2 * g);
        sk += ld_agent(partials + 2 * g + 1);
    }
    if (sw > tol * sk && sw <= 1.7e308) scal[0] = 1.0 / sqrt(sw);
    else *status = ST_DM_RESIDUAL;
    *counter = 0;
}

// VarianceMinimizer, first kernel of step s (grid: ceil(N / BLOCK)).  Every
// block forms p_j itself (the same sum in the same order: the same value).
template <typename T>
__device__ void vm_column(const T *__restrict__ K, int N, int s, double alpha,
                          double tol, double *__restrict__ L,
                          double *__restrict__ p, const int *picks,
                          const unsigned char *chosen, int *status,
                          double *partials) {
    __shared__ double coef[CHUNK];
    __shared__ double red[BLOCK / WAVE];
    if (*status != ST_OK) return;
    const int j = picks[s];
    const int a = blockIdx.x * BLOCK + threadIdx.x;
    double d = 0.0;
    for (int t = threadIdx.x; t < s; t += BLOCK) {
        const double l = L[(size_t)t * N + j];
        d += l * l;
    }
    const double kjj = (double)K[(size_t)j * N + j] + alpha;
    const double pj = kjj - block_sum(d, red);
    if (!(pj > tol * kjj) || !(pj <= 1.7e308)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *status = ST_VM_RESIDUAL;
        return;
    }
    double v = (a < N) ? (double)K[(size_t)j * N + a] + (a == j ? alpha : 0.0)
                       : 0.0;
    for (int t0 = 0; t0 < s; t0 += CHUNK) {
        const int m = min(CHUNK, s - t0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += BLOCK)
            coef[t] = L[(size_t)(t0 + t) * N + j];
        __syncthreads();
        if (a < N)
            for (int t = 0; t < m; ++t)
                v -= L[(size_t)(t0 + t) * N + a] * coef[t];
    }
    const double l = v / sqrt(pj);
    if (a < N) {
        L[(size_t)s * N + a] = l;
        p[a] = v;
    }
    // j is already marked chosen: this is the sum over U \ {j}
    const double u = block_sum((a < N && !chosen[a]) ? l : 0.0, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = u;
}

// Criterion update of step s and the masked argmax that picks picks[next]
// (grid: ceil(N / BLOCK)).  op 0: none (the first pick), 1: DeterminantMaximizer
// (V = Q, W = C), 2: VarianceMinimizer (V = L, W = p, partials of al_vm_column).
__device__ void update_argmax(int N, int s, int op, int next, double *crit,
                              double *V, const double *W, const double *scal,
                              const double *upart, int nupart,
                              unsigned char *chosen, int *picks, int *status,
                              double *bval, int *bidx, int *counter) {
    __shared__ double rv[BLOCK / WAVE];
    __shared__ int ri[BLOCK / WAVE];
    __shared__ double red[BLOCK / WAVE];
    __shared__ bool last;
    if (*status != ST_OK) return;
    const int a = blockIdx.x * BLOCK + threadIdx.x;
    double sum_u = 0.0;
    if (op == 2) {
        double t = 0.0;
        for (int g = threadIdx.x; g < nupart; g += BLOCK) t += upart[g];
        sum_u = block_sum(t, red);
    }
    double v = 0.0;
    int idx = -1;
    if (a < N) {
        double c = crit[a];
        if (op == 1) {
            const double q = V[(size_t)s * N + a] * scal[0];
            V[(size_t)s * N + a] = q;
            const double cs = W[(size_t)s * N + a];
            c -= cs * cs;
            crit[a] = c;
        } else if (op == 2) {
            c -= W[a] + V[(size_t)s * N + a] * sum_u;
            crit[a] = c;
        }
        if (!chosen[a]) { v = c; idx = a; }
    }
    block_argmax(v, idx, rv, ri);
    if (threadIdx.x == 0) {
        st_agent(bval + blockIdx.x, v);
        st_agent(bidx + blockIdx.x, idx);
        __threadfence();
        last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    double best = 0.0;
    int bi = -1;
    for (int g = 0; g < (int)gridDim.x; ++g) {
        const double gv = ld_agent(bval + g);
        const int gi = ld_agent(bidx + g);
        if (better(gv, gi, best, bi)) { best = gv; bi = gi; }
    }
    if (bi < 0) {
        *status = ST_NO_CANDIDATE;
    } else {
        picks[next] = bi;
        chosen[bi] = 1;
    }
    *counter = 0;
}

#define INSTANTIATE(T, SFX)                                                    \
extern "C" __global__ __launch_bounds__(BLOCK) void al_colreduce_##SFX(       \
        const T *K, int N, int mode, double alpha, const double *w,           \
        const double *scal, const int *status, double *out) {                 \
    colreduce<T>(K, N, mode, alpha, w, scal, status, out);                    \
}                                                                              \
extern "C" __global__ __launch_bounds__(BLOCK) void al_dm_direction_##SFX(    \
        const T *K, int N, int s, double tol, double *Q, const double *C,     \
        const int *picks, int *status, double *partials, int *counter,        \
        double *scal) {                                                        \
    dm_direction<T>(K, N, s, tol, Q, C, picks, status, partials, counter,     \
                    scal);                                                     \
}                                                                              \
extern "C" __global__ __launch_bounds__(BLOCK) void al_vm_column_##SFX(       \
        const T *K, int N, int s, double alpha, double tol, double *L,        \
        double *p, const int *picks, const unsigned char *chosen,             \
        int *status, double *partials) {                                       \
    vm_column<T>(K, N, s, alpha, tol, L, p, picks, chosen, status, partials); \
}

INSTANTIATE(float, f32)
INSTANTIATE(double, f64)

extern "C" __global__ __launch_bounds__(BLOCK) void al_update_argmax(
        int N, int s, int op, int next, double *crit, double *V,
        const double *W, const double *scal, const double *upart, int nupart,
        unsigned char *chosen, int *picks, int *status, double *bval,
        int *bidx, int *counter) {
    update_argmax(N, s, op, next, crit, V, W, scal, upart, nupart, chosen,
                  picks, status, bval, bidx, counter);
}
