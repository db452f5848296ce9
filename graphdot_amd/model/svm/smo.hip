// Support vector classification on the Gram matrix alone (svc.py; the host side
// is _smo.py).  K is n x n, symmetric, float or double,
// contiguous along either index (symmetric: K[i n + t] is row i as it lies).
// A batch of P problems shares K; problem p is y[p] (n int8 in {+1, -1}) and
// the upper bounds U[p] (n doubles, >= 0; U = 0: the sample is not part of the
// problem) and minimises
//
//   f(alpha) = 1/2 sum_ij alpha_i alpha_j y_i y_j K_ij - sum_i alpha_i
//   subject to 0 <= alpha <= U, y^T alpha = 0
//
// by SMO with the second-order working-set rule of Fan, Chen and Lin.  With
// G = Q alpha - 1, v_t = -y_t G_t, I_up = {y > 0, alpha < U} + {y < 0, alpha >
// 0} and I_low = {y > 0, alpha > 0} + {y < 0, alpha < U}, one step is
//
//   i = argmax_{I_up} v, m = v_i;  M = min_{I_low} v;  stop when m - M < tol
//   j = argmin over t in I_low with v_t < m of -(m - v_t)^2 / a_t,
//       a_t = K_ii + K_tt - 2 K_it (1e-12 where that is not positive)
//   (alpha_i, alpha_j) move along the constraint, clipped to their box
//   G_t += y_t (y_i K_ti d alpha_i + y_j K_tj d alpha_j)
//
// every argmax and argmin taking the lowest index on a tie, all of it in
// double whatever the type of K.
//
// svm_smo_{f32,f64}: one workgroup per problem, at most `steps` steps per
// launch.  G and alpha of the problem live in LDS (16 bytes per sample of the
// 64 KB, less 512 bytes for the exchange of the reductions: NMAX = 4064); y, U
// and the diagonal of K in registers, sample t = thread + 256 k with thread
// `t % 256`.  A launch loads (alpha, G) from state[p] = [alpha (n) | G (n)] and
// stores them back; info[p] = [steps so far, m, M, status] describes the state
// stored, and a problem that has stopped by it (m - M < tol, steps >= max_iter
// or a status) returns at once.  Status 1: a diagonal entry or a G that is not
// finite, or no second sample to be found (a NaN in the row).
// The two reductions of a step are (value, index) reductions: strided over
// the threads in ascending index, the __shfl_xor butterfly, then the four
// waves in order.  The thread that owns the winner hands its alpha, U, y (and
// G, a) on with it, so that nothing of another thread's is read while it may
// be written (G and alpha in LDS are touched by their owner alone): two
// barriers per step and two dependent row reads, K[i, :] and K[j, :].
//
// svm_decide_{f32,f64}_k{KC}: out[p, r] = sum_j Ks[r, j] coef[p, j] + b[p] for
// the rows of a (nb, n) matrix with any strides, a lane per row, the n terms
// split over the four waves in order, KC problems per pass in registers;
// gridDim.x = ceil(nb / 64) * ceil(P / KC).
//
// Every grid is a function of the shapes alone, every sum and every choice runs
// in a fixed order and there are no atomics: the same bits on every call.
#include "dense_reduce.h"

#define NMAX 4064                // (65536 - 512) / 16
#define TAU 1e-12
#define NONE 0x7fffffff          // the index of an empty choice

// what the waves exchange: stage 1 [m, M, alpha_i, U_i, K_ii], [i, y_i];
// stage 2 [objective, G_j, alpha_j, U_j, a_j], [j, y_j]
struct Exchange {
    double r1[NWAVE][5], r2[NWAVE][5];
    int q1[NWAVE][2], q2[NWAVE][2];
    int bad;
};

template <typename T, int PT>
__device__ __forceinline__ void smo_slice(
    const T *__restrict__ K, int n, const int8_t *__restrict__ y,
    const double *__restrict__ U, double *__restrict__ state,
    double *__restrict__ info, double tol, int64_t done, int64_t limit,
    double *G, double *A, Exchange &x)
{
    const int tid = threadIdx.x, lane = tid % WAVE, wid = tid / WAVE;
    const double inf = __builtin_inf();
    int yk[PT];
    double Uk[PT], dk[PT], ki[PT];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < PT; ++k) {
        const int t = tid + k * BLOCK;
        yk[k] = 0;
        Uk[k] = dk[k] = ki[k] = 0.0;
        if (t < n) {
            A[t] = state[t];
            G[t] = state[n + t];
            yk[k] = y[t];
            Uk[k] = U[t];
            dk[k] = (double)K[(int64_t)t * n + t];
            bad |= !is_finite(dk[k]) || !is_finite(G[t]);
        }
    }
    if (tid == 0) x.bad = 0;
    __syncthreads();
    if (bad) x.bad = 1;

    double m, M;
    int status;
    for (;;) {
        // -- i = argmax of v over I_up, M = min of v over I_low
        double bv = -inf, bM = inf, pa = 0.0, pu = 0.0, pd = 0.0;
        int bi = NONE, py = 0;
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const int t = tid + k * BLOCK;
            if (t < n) {
                const double g = G[t], a = A[t];
                const bool pos = yk[k] > 0;
                const double v = pos ? -g : g;
                const bool up = pos ? a < Uk[k] : a > 0.0;
                const bool low = pos ? a > 0.0 : a < Uk[k];
                if (up && v > bv) {
                    bv = v; bi = t; pa = a; pu = Uk[k]; pd = dk[k]; py = yk[k];
                }
                if (low && v < bM) bM = v;
            }
        }
        const int mine = bi;
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, WAVE);
            const int oi = __shfl_xor(bi, off, WAVE);
            const double oM = __shfl_xor(bM, off, WAVE);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            bM = oM < bM ? oM : bM;
        }
        if (bi == NONE ? lane == 0 : mine == bi) {
            x.r1[wid][0] = bv; x.r1[wid][1] = bM; x.r1[wid][2] = pa;
            x.r1[wid][3] = pu; x.r1[wid][4] = pd;
            x.q1[wid][0] = bi; x.q1[wid][1] = py;
        }
        __syncthreads();
        int i = NONE, w1 = 0;
        m = -inf;
        M = inf;
        for (int w = 0; w < NWAVE; ++w) {
            const double ov = x.r1[w][0], oM = x.r1[w][1];
            const int oi = x.q1[w][0];
            if (ov > m || (ov == m && oi < i)) { m = ov; i = oi; w1 = w; }
            M = oM < M ? oM : M;
        }
        status = x.bad;
        if (status != 0 || m - M < tol || done >= limit) break;
        const double a_i = x.r1[w1][2], U_i = x.r1[w1][3], d_i = x.r1[w1][4];
        const int y_i = x.q1[w1][1];

        // -- j = argmin of -(m - v_t)^2 / a_t over the t in I_low with v_t < m
        const T *row = K + (int64_t)i * n;
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const int t = tid + k * BLOCK;
            if (t < n) ki[k] = (double)row[t];
        }
        double bo = inf, pg = 0.0, pq = 0.0;
        int bj = NONE;
        pa = pu = 0.0;
        py = 0;
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const int t = tid + k * BLOCK;
            if (t < n) {
                const double g = G[t], a = A[t];
                const bool pos = yk[k] > 0;
                const double v = pos ? -g : g;
                const bool low = pos ? a > 0.0 : a < Uk[k];
                if (low && v < m) {
                    const double b = m - v;
                    double q = (d_i + dk[k]) - 2.0 * ki[k];
                    q = q <= 0.0 ? TAU : q;
                    const double o = -(b * b) / q;
                    if (o < bo) {
                        bo = o; bj = t; pg = g; pa = a; pu = Uk[k]; pq = q;
                        py = yk[k];
                    }
                }
            }
        }
        const int mine2 = bj;
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const double oo = __shfl_xor(bo, off, WAVE);
            const int oj = __shfl_xor(bj, off, WAVE);
            if (oo < bo || (oo == bo && oj < bj)) { bo = oo; bj = oj; }
        }
        if (bj == NONE ? lane == 0 : mine2 == bj) {
            x.r2[wid][0] = bo; x.r2[wid][1] = pg; x.r2[wid][2] = pa;
            x.r2[wid][3] = pu; x.r2[wid][4] = pq;
            x.q2[wid][0] = bj; x.q2[wid][1] = py;
        }
        __syncthreads();
        int j = NONE, w2 = 0;
        double o = inf;
        for (int w = 0; w < NWAVE; ++w) {
            const double oo = x.r2[w][0];
            const int oj = x.q2[w][0];
            if (oo < o || (oo == o && oj < j)) { o = oo; j = oj; w2 = w; }
        }
        if (j == NONE) {                 // (a NaN in row i: nothing compares)
            status = 1;
            break;
        }
        const double G_j = x.r2[w2][1], a_j = x.r2[w2][2], U_j = x.r2[w2][3],
                     q = x.r2[w2][4];
        const int y_j = x.q2[w2][1];
        const double G_i = y_i > 0 ? -m : m;
        const T *rowj = K + (int64_t)j * n;
        double kj[PT];
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const int t = tid + k * BLOCK;
            kj[k] = t < n ? (double)rowj[t] : 0.0;
        }

        // -- the pair along the constraint, clipped to its box: ni, nj
        SMO_PAIR_UPDATE(y_i != y_j, a_i, a_j, G_i, G_j, U_i, U_j, q);
        const double s_i = (double)y_i * (ni - a_i),
                     s_j = (double)y_j * (nj - a_j);
        if (tid == i % BLOCK) A[i] = ni;
        if (tid == j % BLOCK) A[j] = nj;
        bad = false;
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const int t = tid + k * BLOCK;
            if (t < n) {
                const double d = ki[k] * s_i + kj[k] * s_j;
                const double g = G[t] + (yk[k] > 0 ? d : -d);
                G[t] = g;
                bad |= !is_finite(g);
            }
        }
        if (bad) x.bad = 1;
        ++done;
    }

#pragma unroll
    for (int k = 0; k < PT; ++k) {
        const int t = tid + k * BLOCK;
        if (t < n) {
            state[t] = A[t];
            state[n + t] = G[t];
        }
    }
    if (tid == 0) {
        info[0] = (double)done;
        info[1] = m;
        info[2] = M;
        info[3] = status ? 1.0 : 0.0;
    }
}

// gridDim.x = P
template <typename T>
__device__ __forceinline__ void smo_stage(
    const T *__restrict__ K, int n, const int8_t *__restrict__ y,
    const double *__restrict__ U, double *__restrict__ state,
    double *__restrict__ info, double tol, int64_t steps, int64_t max_iter)
{
    __shared__ double G[NMAX], A[NMAX];
    __shared__ Exchange x;
    if (n < 1 || n > NMAX) return;
    const int64_t p = blockIdx.x;
    info += p * 4;
    if (info[3] != 0.0 || info[1] - info[2] < tol
            || info[0] >= (double)max_iter)
        return;
    const int64_t done = (int64_t)info[0];
    const int64_t limit = steps < max_iter - done ? done + steps : max_iter;
    y += p * n;
    U += p * n;
    state += p * 2 * n;
    if (n <= 4 * BLOCK)
        smo_slice<T, 4>(K, n, y, U, state, info, tol, done, limit, G, A, x);
    else if (n <= 8 * BLOCK)
        smo_slice<T, 8>(K, n, y, U, state, info, tol, done, limit, G, A, x);
    else
        smo_slice<T, 16>(K, n, y, U, state, info, tol, done, limit, G, A, x);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
svm_smo_f32(const float *K, int n, const int8_t *y, const double *U,
            double *state, double *info, double tol, int64_t steps,
            int64_t max_iter) {
    smo_stage<float>(K, n, y, U, state, info, tol, steps, max_iter);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
svm_smo_f64(const double *K, int n, const int8_t *y, const double *U,
            double *state, double *info, double tol, int64_t steps,
            int64_t max_iter) {
    smo_stage<double>(K, n, y, U, state, info, tol, steps, max_iter);
}

// Ks[r s_r + j s_j]; coef (P, n), b (P), out (P, nb) row-major;
// gridDim.x = ceil(nb / WAVE) * ceil(P / KC)
template <typename T, int KC>
__device__ __forceinline__ void decide_stage(
    const T *__restrict__ Ks, int64_t nb, int64_t n, int64_t s_r, int64_t s_j,
    const double *__restrict__ coef, const double *__restrict__ b, int P,
    double *__restrict__ out)
{
    __shared__ double sh[NWAVE][KC][WAVE];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t nrb = (nb + WAVE - 1) / WAVE;
    const int64_t r = (blockIdx.x % nrb) * WAVE + lane;
    const int p0 = (int)(blockIdx.x / nrb) * KC;
    const int64_t span = (n + NWAVE - 1) / NWAVE;
    const int64_t j0 = min(n, wid * span), j1 = min(n, j0 + span);
    const T *row = Ks + (r < nb ? r : 0) * s_r;
    const double *c[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)              // (in bounds either way)
        c[kk] = coef + (int64_t)(p0 + kk < P ? p0 + kk : 0) * n;
    double acc[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;
    for (int64_t j = j0; j < j1; ++j) {
        const double ks = (double)row[j * s_j];
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) acc[kk] += ks * c[kk][j];
    }
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) sh[wid][kk][lane] = acc[kk];
    __syncthreads();
    if (wid == 0 && r < nb) {
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            if (p0 + kk < P) {
                double s = 0.0;
                for (int w = 0; w < NWAVE; ++w) s += sh[w][kk][lane];
                out[(int64_t)(p0 + kk) * nb + r] = s + b[p0 + kk];
            }
        }
    }
}

#define DECIDE(T, SFX, KC)                                                     \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    svm_decide_##SFX##_k##KC(const T *Ks, int64_t nb, int64_t n, int64_t s_r,  \
                             int64_t s_j, const double *coef, const double *b, \
                             int P, double *out) {                             \
        decide_stage<T, KC>(Ks, nb, n, s_r, s_j, coef, b, P, out);             \
    }

DECIDE(float, f32, 1)
DECIDE(float, f32, 2)
DECIDE(float, f32, 4)
DECIDE(float, f32, 8)
DECIDE(float, f32, 16)
DECIDE(double, f64, 1)
DECIDE(double, f64, 2)
DECIDE(double, f64, 4)
DECIDE(double, f64, 8)
DECIDE(double, f64, 16)
