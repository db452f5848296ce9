// Epsilon support vector regression on the Gram matrix alone (svr.py; the host
// side is _smo.py).  K is n x n, symmetric, float or
// double, contiguous along either index (symmetric: K[i n + r] is row i as it
// lies).  The dual has 2n variables over the n samples: a_t for t < n and
// a*_{t - n} for t >= n, with the sign s_t = +1 on the first half and -1 on
// the second and Q_st = s_s s_t K[s mod n, t mod n].  A batch of P problems
// shares K; problem p is the upper bounds U[p] (n doubles, >= 0, the bound of
// both variables of a sample; U = 0: the sample is not part of the problem)
// and minimises
//
//   f(alpha) = 1/2 sum_st alpha_s alpha_t Q_st + sum_t p_t alpha_t
//   subject to 0 <= alpha_t <= U[t mod n], s^T alpha = 0
//
// where the linear term p (eps - z on the first half, eps + z on the second)
// enters only through the G = Q alpha + p that the host writes into `state`
// before the first step: the kernel sees neither z nor eps.  One step is the
// step of smo.hip with y_t = s_t, K_ti = K[t mod n, i mod n] and the diagonal
// K[t mod n, t mod n]:
//
//   i = argmax_{I_up} v, m = v_i;  M = min_{I_low} v;  stop when m - M < tol
//   j = argmin over t in I_low with v_t < m of -(m - v_t)^2 / a_t,
//       a_t = K_ii + K_tt - 2 K_it (1e-12 where that is not positive)
//   (alpha_i, alpha_j) move along the constraint, clipped to their box
//   G_t += s_t (s_i K_ti d alpha_i + s_j K_tj d alpha_j)
//
// with v_t = -s_t G_t, I_up = {s > 0, alpha < U} + {s < 0, alpha > 0} and
// I_low = {s > 0, alpha > 0} + {s < 0, alpha < U}; every argmax and argmin
// runs over the variable index 0 .. 2n - 1 and takes the lowest on a tie (a_t
// before a*_t), all of it in double whatever the type of K.
//
// svm_smo2_{f32,f64}: one workgroup per problem, at most `steps` steps per
// launch.  G and alpha of the 2n variables live in LDS (32 bytes per sample
// of the 64 KB, less 512 bytes for the exchange of the reductions: NMAX2 =
// 2032).  Thread `r % 256` owns sample r and both of its variables, r and n +
// r; it keeps U_r, K_rr and its slices of the two rows in registers, so a row
// of n entries is read once and serves both halves.  A launch loads (alpha,
// G) from state[p] = [alpha (2n) | G (2n)] and stores them back; info[p] =
// [steps so far, m, M, status] describes the state stored, and a problem that
// has stopped by it (m - M < tol, steps >= max_iter or a status) returns at
// once.  Status 1: a diagonal entry or a G that is not finite, or no second
// variable to be found (a NaN in the row).
// The two reductions of a step are (value, index) reductions: strided over
// the threads in ascending variable index (the first half of a thread's
// samples, then the second), the __shfl_xor butterfly, then the four waves in
// order.  The thread that owns the winner hands its alpha, U (and G, a) on
// with it; the sign of a winner is its index (>= n or not).  G and alpha in
// LDS are touched by their owner alone: two barriers per step and two
// dependent row reads, K[i mod n, :] and K[j mod n, :].
//
// The grid is a function of the shapes alone, every choice runs in a fixed
// order and there are no atomics: the same bits on every call.
#include "dense_reduce.h"

#define NMAX2 2032               // (65536 - 512) / 32
#define TAU 1e-12
#define NONE 0x7fffffff          // the index of an empty choice

// what the waves exchange: stage 1 [m, M, alpha_i, U_i, K_ii], i;
// stage 2 [objective, G_j, alpha_j, U_j, a_j], j
struct Exchange {
    double r1[NWAVE][5], r2[NWAVE][5];
    int q1[NWAVE], q2[NWAVE];
    int bad;
};

template <typename T, int PT>
__device__ __forceinline__ void smo2_slice(
    const T *__restrict__ K, int n, const double *__restrict__ U,
    double *__restrict__ state, double *__restrict__ info, double tol,
    int64_t done, int64_t limit, double *G, double *A, Exchange &x)
{
    const int tid = threadIdx.x, lane = tid % WAVE, wid = tid / WAVE;
    const double inf = __builtin_inf();
    double Uk[PT], dk[PT], ki[PT];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < PT; ++k) {
        const int r = tid + k * BLOCK;
        Uk[k] = dk[k] = ki[k] = 0.0;
        if (r < n) {
            A[r] = state[r];
            A[n + r] = state[n + r];
            G[r] = state[2 * n + r];
            G[n + r] = state[3 * n + r];
            Uk[k] = U[r];
            dk[k] = (double)K[(int64_t)r * n + r];
            bad |= !is_finite(dk[k]) || !is_finite(G[r])
                || !is_finite(G[n + r]);
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
        int bi = NONE;
#pragma unroll
        for (int k = 0; k < PT; ++k) {           // s = +1: v = -G
            const int r = tid + k * BLOCK;
            if (r < n) {
                const double v = -G[r], a = A[r];
                if (a < Uk[k] && v > bv) {
                    bv = v; bi = r; pa = a; pu = Uk[k]; pd = dk[k];
                }
                if (a > 0.0 && v < bM) bM = v;
            }
        }
#pragma unroll
        for (int k = 0; k < PT; ++k) {           // s = -1: v = G
            const int r = tid + k * BLOCK;
            if (r < n) {
                const double v = G[n + r], a = A[n + r];
                if (a > 0.0 && v > bv) {
                    bv = v; bi = n + r; pa = a; pu = Uk[k]; pd = dk[k];
                }
                if (a < Uk[k] && v < bM) bM = v;
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
            x.q1[wid] = bi;
        }
        __syncthreads();
        int i = NONE, w1 = 0;
        m = -inf;
        M = inf;
        for (int w = 0; w < NWAVE; ++w) {
            const double ov = x.r1[w][0], oM = x.r1[w][1];
            const int oi = x.q1[w];
            if (ov > m || (ov == m && oi < i)) { m = ov; i = oi; w1 = w; }
            M = oM < M ? oM : M;
        }
        status = x.bad;
        if (status != 0 || m - M < tol || done >= limit) break;
        const double a_i = x.r1[w1][2], U_i = x.r1[w1][3], d_i = x.r1[w1][4];
        const bool pos_i = i < n;
        const int ri = pos_i ? i : i - n;

        // -- j = argmin of -(m - v_t)^2 / a_t over the t in I_low with v_t < m
        const T *row = K + (int64_t)ri * n;
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const int r = tid + k * BLOCK;
            if (r < n) ki[k] = (double)row[r];
        }
        double bo = inf, pg = 0.0, pq = 0.0;
        int bj = NONE;
        pa = pu = 0.0;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int k = 0; k < PT; ++k) {
                const int r = tid + k * BLOCK;
                if (r < n) {
                    const int t = half ? n + r : r;
                    const double g = G[t], a = A[t];
                    const double v = half ? g : -g;
                    const bool low = half ? a < Uk[k] : a > 0.0;
                    if (low && v < m) {
                        const double b = m - v;
                        double q = (d_i + dk[k]) - 2.0 * ki[k];
                        q = q <= 0.0 ? TAU : q;
                        const double o = -(b * b) / q;
                        if (o < bo) {
                            bo = o; bj = t; pg = g; pa = a; pu = Uk[k]; pq = q;
                        }
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
            x.q2[wid] = bj;
        }
        __syncthreads();
        int j = NONE, w2 = 0;
        double o = inf;
        for (int w = 0; w < NWAVE; ++w) {
            const double oo = x.r2[w][0];
            const int oj = x.q2[w];
            if (oo < o || (oo == o && oj < j)) { o = oo; j = oj; w2 = w; }
        }
        if (j == NONE) {                 // (a NaN in row i: nothing compares)
            status = 1;
            break;
        }
        const double G_j = x.r2[w2][1], a_j = x.r2[w2][2], U_j = x.r2[w2][3],
                     q = x.r2[w2][4];
        const bool pos_j = j < n;
        const int rj = pos_j ? j : j - n;
        const double G_i = pos_i ? -m : m;
        const T *rowj = K + (int64_t)rj * n;
        double kj[PT];
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const int r = tid + k * BLOCK;
            kj[k] = r < n ? (double)rowj[r] : 0.0;
        }

        // -- the pair along the constraint, clipped to its box: ni, nj
        SMO_PAIR_UPDATE(pos_i != pos_j, a_i, a_j, G_i, G_j, U_i, U_j, q);
        const double s_i = pos_i ? ni - a_i : -(ni - a_i),
                     s_j = pos_j ? nj - a_j : -(nj - a_j);
        if (tid == ri % BLOCK) A[i] = ni;
        if (tid == rj % BLOCK) A[j] = nj;
        bad = false;
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const int r = tid + k * BLOCK;
            if (r < n) {
                const double d = ki[k] * s_i + kj[k] * s_j;
                const double g = G[r] + d, h = G[n + r] - d;
                G[r] = g;
                G[n + r] = h;
                bad |= !is_finite(g) || !is_finite(h);
            }
        }
        if (bad) x.bad = 1;
        ++done;
    }

#pragma unroll
    for (int k = 0; k < PT; ++k) {
        const int r = tid + k * BLOCK;
        if (r < n) {
            state[r] = A[r];
            state[n + r] = A[n + r];
            state[2 * n + r] = G[r];
            state[3 * n + r] = G[n + r];
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
__device__ __forceinline__ void smo2_stage(
    const T *__restrict__ K, int n, const double *__restrict__ U,
    double *__restrict__ state, double *__restrict__ info, double tol,
    int64_t steps, int64_t max_iter)
{
    __shared__ double G[2 * NMAX2], A[2 * NMAX2];
    __shared__ Exchange x;
    if (n < 1 || n > NMAX2) return;
    const int64_t p = blockIdx.x;
    info += p * 4;
    if (info[3] != 0.0 || info[1] - info[2] < tol
            || info[0] >= (double)max_iter)
        return;
    const int64_t done = (int64_t)info[0];
    const int64_t limit = steps < max_iter - done ? done + steps : max_iter;
    U += p * n;
    state += p * 4 * n;
    if (n <= 4 * BLOCK)
        smo2_slice<T, 4>(K, n, U, state, info, tol, done, limit, G, A, x);
    else
        smo2_slice<T, 8>(K, n, U, state, info, tol, done, limit, G, A, x);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
svm_smo2_f32(const float *K, int n, const double *U, double *state,
             double *info, double tol, int64_t steps, int64_t max_iter) {
    smo2_stage<float>(K, n, U, state, info, tol, steps, max_iter);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
svm_smo2_f64(const double *K, int n, const double *U, double *state,
             double *info, double tol, int64_t steps, int64_t max_iter) {
    smo2_stage<double>(K, n, U, state, info, tol, steps, max_iter);
}
