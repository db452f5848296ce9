// Element-wise map of KernelOverMetric (host side _kom_map.py; DESIGN.md
// section 21): K = f(D) and, on request, the gradient of K by the chain rule,
// for a distance matrix D (nr x nc, element (r, c) at D[r sd0 + c sd1],
// float or double, read as it lies).  The expressions come from the user's
// formula through the sympy printer of graphdot_amd.codegen; the
// hyperparameter values are a kernel argument (H), so this source -- and the
// JIT cache key -- depends on the formula alone.  All arithmetic double.
//   value: K[e] = f(d)
//   dense: K[e], G[e + N k] = df/dh_k (d)                    k < NH
//                G[e + N (NH + k)] = df/dx (d) P[r, c, planes[k]]   k < np
//   lazy:  K[e], G[e + N k] = df/dh_k (d) (k < NH), S[e] = df/dx (d)
// with e = r + nr c and N = nr nc: every output column-major, float64.  P are
// the distance's gradient planes (element (r, c, q) at P[r sp0 + c sp1 +
// q sp2], float or double); `planes` picks the active ones without a copy.
// One element per thread, the rows of one column over a workgroup: D, each
// selected plane and every output are read or written once, coalesced when
// the row stride is 1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fmath.h"

#define BLOCK 256
#define NH ${n_hyper}

struct kom_hyper {
    double h[NH > 0 ? NH : 1];
};

enum { KOM_VALUE = 0, KOM_DENSE = 1, KOM_LAZY = 2 };

__device__ __forceinline__ double kom_f(const double d, const kom_hyper &H) {
    return ${fun};
}

__device__ __forceinline__ double kom_dfdx(const double d,
                                           const kom_hyper &H) {
    return ${dfdx};
}

__device__ __forceinline__ void kom_own(const double d, const kom_hyper &H,
                                        double *__restrict__ G, int64_t e,
                                        int64_t N) {
${own}
}

template <typename TD, typename TP, int MODE>
__device__ __forceinline__ void kom_body(
    const TD *__restrict__ D, int64_t sd0, int64_t sd1, int64_t nr,
    int64_t nc, int64_t gx, const TP *__restrict__ P, int64_t sp0,
    int64_t sp1, int64_t sp2, const int64_t *__restrict__ planes, int64_t np,
    double *__restrict__ K, double *__restrict__ G, double *__restrict__ S,
    const kom_hyper &H)
{
    const int64_t c = (int64_t)blockIdx.x / gx;
    const int64_t r = ((int64_t)blockIdx.x % gx) * BLOCK + threadIdx.x;
    if (r >= nr || c >= nc) return;
    const int64_t e = r + nr * c;
    const int64_t N = nr * nc;
    const double d = (double)D[r * sd0 + c * sd1];
    K[e] = kom_f(d, H);
    if (MODE == KOM_VALUE) return;
    kom_own(d, H, G, e, N);
    if (MODE == KOM_LAZY) {
        S[e] = kom_dfdx(d, H);
        return;
    }
    if (np > 0) {
        const double s = kom_dfdx(d, H);
        const TP *__restrict__ p = P + r * sp0 + c * sp1;
        double *__restrict__ g = G + e + N * NH;
        for (int64_t k = 0; k < np; ++k)
            g[N * k] = s * (double)p[planes[k] * sp2];
    }
}

#define KOM_ENTRY(MODE_NAME, MODE, TD, TP, SD, SP)                            \
    extern "C" __global__ __launch_bounds__(BLOCK) void                       \
    kom_##MODE_NAME##_##SD##_##SP(                                           \
        const TD *__restrict__ D, int64_t sd0, int64_t sd1, int64_t nr,       \
        int64_t nc, int64_t gx, const TP *__restrict__ P, int64_t sp0,        \
        int64_t sp1, int64_t sp2, const int64_t *__restrict__ planes,         \
        int64_t np, double *__restrict__ K, double *__restrict__ G,           \
        double *__restrict__ S, const kom_hyper H)                           \
    {                                                                         \
        kom_body<TD, TP, MODE>(D, sd0, sd1, nr, nc, gx, P, sp0, sp1, sp2,     \
                               planes, np, K, G, S, H);                      \
    }

#define KOM_MODES(TD, TP, SD, SP)                                             \
    KOM_ENTRY(value, KOM_VALUE, TD, TP, SD, SP)                               \
    KOM_ENTRY(dense, KOM_DENSE, TD, TP, SD, SP)                               \
    KOM_ENTRY(lazy, KOM_LAZY, TD, TP, SD, SP)

KOM_MODES(float, float, f32, f32)
KOM_MODES(float, double, f32, f64)
KOM_MODES(double, float, f64, f32)
KOM_MODES(double, double, f64, f64)
