// ba_calib.hip — K3''' with intrinsics: global bundle adjustment with shared intrinsics and radial
// distortion as unknowns (DESIGN.md "K3''' with intrinsics", tests/ba_calib_ref.py restates every step).
//
// ba_global.hip's solver (Schur-complement Levenberg-Marquardt, matrix-free block-Jacobi PCG, the
// same step rule, gate and status codes) over the camera-side unknown x~ = (x_c [6C], x_k [5G]):
// every camera belongs to one of G intrinsics groups with theta = (f, cx, cy, k1, k2) and a fixed
// aspect asp = fy / fx; a byte mask of length 5 says which components of theta are free.
//
//   (x, y, z) = R X + t,  xn = x / z,  yn = y / z,  r2 = xn^2 + yn^2,  d = 1 + k1 r2 + k2 r2^2
//   u = f (d xn) + cx,  v = (f asp) (d yn) + cy          (OpenCV's radial model, p1 = p2 = k3 = 0)
//
// Per observation r (2), Jc (2x6), Jp (2x3) and Jk (2x5, columns of masked components 0) are
// stored: 30 doubles.  At k1 = k2 = 0 the operations give the values of ba_global.hip's
// k_linearize (a term that is exactly 0 is added where the pinhole form has none).
//
// Sums, none with a floating-point atomic, all in an order fixed by the structure alone:
//   * per point, per camera chunk, per camera, CG vectors and the cost: as in ba_global.hip;
//   * per group: one workgroup per group; lane l of 256 adds the per-camera values of the group's
//     l-th, (l + 256)-th, ... camera (ascending camera index) in sequence, then the pairwise tree.
// The CG vectors have length 6C + 5G, the intrinsics entries after the cameras.
#include "common.h"
#include "geom_dev.h"
#include "ba_dev.h"
#include <climits>
#include <cmath>
#include <algorithm>

namespace sfmhip {
namespace {

constexpr int kMaxGroups = 1 << 20;

struct Ctl {
    double lambda, cost, cost_trial, rel, rz, bb, gtol, ftol, eta;
    unsigned long long gmax_bits;      // max |g| over free cameras, free intrinsics and points (bits of a double)
    int bad;                           // structure / index / mask error found by kc_validate
    int depth_flag, depth_bad;         // as in ba_global.hip
    int done, status, cg_done, cg_iters, cg_total, accepted, n_accept;
};

struct Ws {                            // device pointers of one solve
    Ctl* ctl;
    const double* asp;                 // [G] fy / fx
    const int32_t* grp;                // [C] group of a camera
    const uint8_t* mask;               // [5] 1: the component of theta is free
    const int32_t *oc, *op;
    const double* uv;
    const int64_t *pt_off, *cam_perm, *cam_off;
    const uint8_t* fixed;              // nullable: no camera fixed
    int C, N, G;
    int64_t M;
    int nb, tmax;
    int *chunk_base, *chunk_cam;
    int *grp_off, *grp_cams;           // cameras of a group, ascending: grp_cams[grp_off[g] .. grp_off[g + 1])
    double *R, *t, *X, *th, *Rt, *tt, *Xt, *tht;   // accepted and trial state
    double *r, *Jc, *Jk, *Jp, *cpart;
    double *U, *gc, *B, *H, *gk, *V, *gp;
    double *Us, *Ui, *Hs, *Hi, *Vi;
    double *part27, *part30, *part20, *part11, *camH, *gq, *y;
    double *b, *x, *rr, *z, *p, *q;    // CG vectors (6C + 5G each)
    double f2;
    double* wout;
};

__device__ __forceinline__ void gmax_update(Ctl* ctl, double g) {
    atomicMax(&ctl->gmax_bits, (unsigned long long)__double_as_longlong(fabs(g)));
}

// ---------------------------------------------------------------------------
// Structure check (ba_dev.h) plus the group of every camera and the mask bytes.
__global__ __launch_bounds__(kWg) void kc_validate(Ws w) {
    const int64_t i = (int64_t)blockIdx.x * kWg + threadIdx.x;
    bool bad = structure_bad(i, w.oc, w.op, w.pt_off, w.cam_perm, w.cam_off, w.C, w.N, w.M);
    if (i < w.C) bad |= w.grp[i] < 0 || w.grp[i] >= w.G;
    if (i < 5) bad |= w.mask[i] > 1;
    if (bad) atomicOr(&w.ctl->bad, 1);
}

// Chunk numbering (ba_dev.h) and the cameras of every group in ascending order (a counting sort
// by one lane: C + G steps, once per call; C, G <= 2^20).
__global__ void kc_layout(Ws w) {
    if (w.ctl->bad) return;
    chunk_numbering(w);
    for (int g = 0; g <= w.G; ++g) w.grp_off[g] = 0;
    for (int c = 0; c < w.C; ++c) w.grp_off[w.grp[c] + 1] += 1;
    for (int g = 0; g < w.G; ++g) w.grp_off[g + 1] += w.grp_off[g];
    for (int c = w.C - 1; c >= 0; --c) {            // back to front, then the offsets are the starts again
        const int g = w.grp[c];
        w.grp_cams[w.grp_off[g + 1] - 1] = c;
        w.grp_off[g + 1] -= 1;
    }
    // grp_off[g + 1] now holds the start of group g: shift back into place
    for (int g = 0; g < w.G; ++g) w.grp_off[g] = w.grp_off[g + 1];
    w.grp_off[w.G] = w.C;
}

__global__ __launch_bounds__(kWg) void kc_init(Ws w, const double* cam, const double* X, const double* theta) {
    if (w.ctl->bad) return;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.C) {
        rodrigues(cam + 6 * i, w.R + 9 * i);
        for (int k = 0; k < 3; ++k) w.t[3 * i + k] = cam[6 * i + 3 + k];
    }
    if (i < w.N)
        for (int k = 0; k < 3; ++k) w.X[3 * i + k] = X[3 * i + k];
    if (i < w.G)
        for (int k = 0; k < 5; ++k) w.th[5 * i + k] = theta[5 * i + k];
}

// The distorted projection of one observation.
struct Proj {
    double px, py, pz, z, iz, xn, yn, r2, d, fx, fy, r0, r1;
};

__device__ __forceinline__ Proj project(const Ws& w, int64_t m, const double* Rs, const double* ts, const double* Xs,
                                        const double* ths, const double*& R, const double*& th) {
    const int c = w.oc[m], p = w.op[m];
    const int g = w.grp[c];
    R = Rs + 9 * (int64_t)c;
    th = ths + 5 * (int64_t)g;
    const double* t = ts + 3 * (int64_t)c;
    const double* X = Xs + 3 * (int64_t)p;
    Proj o;
    o.fx = th[0];
    o.fy = th[0] * w.asp[g];
    o.px = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2];
    o.py = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2];
    o.pz = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
    const double x = o.px + t[0], y = o.py + t[1];
    o.z = o.pz + t[2];
    o.iz = 1.0 / o.z;
    o.xn = x * o.iz;
    o.yn = y * o.iz;
    o.r2 = o.xn * o.xn + o.yn * o.yn;
    o.d = (1.0 + th[3] * o.r2) + th[4] * (o.r2 * o.r2);
    o.r0 = ((o.d * o.xn) * o.fx + th[1]) - w.uv[2 * m];
    o.r1 = ((o.d * o.yn) * o.fy + th[2]) - w.uv[2 * m + 1];
    return o;
}

// Residual, Jacobians (JAC) and the workgroup's partial cost, one lane per sorted observation; the
// robust loss as in ba_global.hip (sqrt(w) on r, Jc, Jk, Jp; the cost term f^2 rho).
template <bool JAC, int LOSS>
__global__ __launch_bounds__(kWg) void kc_linearize(Ws w, const double* Rs, const double* ts, const double* Xs,
                                                    const double* ths, bool trial) {
    if (w.ctl->bad || (trial && w.ctl->done)) return;
    __shared__ double sm[kWg];
    const int64_t m = (int64_t)blockIdx.x * kWg + threadIdx.x;
    double sq = 0.0;
    if (m < w.M) {
        const double *R, *th;
        const Proj o = project(w, m, Rs, ts, Xs, ths, R, th);
        if (!(o.z > 0.0)) atomicOr(&w.ctl->depth_flag, 1);
        sq = o.r0 * o.r0 + o.r1 * o.r1;
        double sw = 1.0;
        if (LOSS != kLinear) {
            const double zr = sq / w.f2;
            sq = w.f2 * loss_rho<LOSS>(zr);
            if (JAC) {
                const double wt = loss_weight<LOSS>(zr);
                if (w.wout != nullptr) w.wout[m] = wt;
                sw = sqrt(wt);
            }
        }
        if (JAC) {
            const double xn = o.xn, yn = o.yn, px = o.px, py = o.py, pz = o.pz;
            const double e = 2.0 * (th[3] + (2.0 * th[4]) * o.r2);
            const double D00 = o.d + e * (xn * xn), D01 = e * (xn * yn), D11 = o.d + e * (yn * yn);
            const double a = o.fx * o.iz, b = o.fy * o.iz;
            const double a00 = a * D00, a01 = a * D01, a10 = b * D01, a11 = b * D11;
            const double d02 = -(a00 * xn + a01 * yn), d12 = -(a10 * xn + a11 * yn);
            double jp[6], jc[12], jk[10];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                jp[j] = (a00 * R[j] + a01 * R[3 + j]) + d02 * R[6 + j];
                jp[3 + j] = (a10 * R[j] + a11 * R[3 + j]) + d12 * R[6 + j];
            }
            jc[0] = d02 * py - a01 * pz;
            jc[1] = a00 * pz - d02 * px;
            jc[2] = -(a00 * py) + a01 * px;
            jc[3] = a00;
            jc[4] = a01;
            jc[5] = d02;
            jc[6] = -(a11 * pz) + d12 * py;
            jc[7] = a10 * pz - d12 * px;
            jc[8] = a11 * px - a10 * py;
            jc[9] = a10;
            jc[10] = a11;
            jc[11] = d12;
            const double asp = w.asp[w.grp[w.oc[m]]];
            const double fxn = o.fx * xn, fyn = o.fy * yn, r4 = o.r2 * o.r2;
            jk[0] = o.d * xn;
            jk[5] = asp * (o.d * yn);
            jk[1] = 1.0; jk[6] = 0.0;
            jk[2] = 0.0; jk[7] = 1.0;
            jk[3] = fxn * o.r2;
            jk[8] = fyn * o.r2;
            jk[4] = fxn * r4;
            jk[9] = fyn * r4;
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (!w.mask[j]) {
                    jk[j] = 0.0;
                    jk[5 + j] = 0.0;
                }
            double* Jp = w.Jp + 6 * m;
            double* Jc = w.Jc + 12 * m;
            double* Jk = w.Jk + 10 * m;
            if (LOSS == kLinear) {
                w.r[2 * m] = o.r0;
                w.r[2 * m + 1] = o.r1;
#pragma unroll
                for (int j = 0; j < 6; ++j) Jp[j] = jp[j];
#pragma unroll
                for (int j = 0; j < 12; ++j) Jc[j] = jc[j];
#pragma unroll
                for (int j = 0; j < 10; ++j) Jk[j] = jk[j];
            } else {
                w.r[2 * m] = sw * o.r0;
                w.r[2 * m + 1] = sw * o.r1;
#pragma unroll
                for (int j = 0; j < 6; ++j) Jp[j] = sw * jp[j];
#pragma unroll
                for (int j = 0; j < 12; ++j) Jc[j] = sw * jc[j];
#pragma unroll
                for (int j = 0; j < 10; ++j) Jk[j] = sw * jk[j];
            }
        }
    }
    const double s = block_sum(sq, sm);
    if (threadIdx.x == 0) w.cpart[blockIdx.x] = s;
}

// The unweighted |r|^2 of every sorted observation under the distorted model, once after the solve.
__global__ __launch_bounds__(kWg) void kc_obs_res2(Ws w, const double* Rs, const double* ts, const double* Xs,
                                                   const double* ths, double* res2) {
    if (w.ctl->bad) return;
    const int64_t m = (int64_t)blockIdx.x * kWg + threadIdx.x;
    if (m >= w.M) return;
    const double *R, *th;
    const Proj o = project(w, m, Rs, ts, Xs, ths, R, th);
    res2[m] = o.r0 * o.r0 + o.r1 * o.r1;
}

__global__ __launch_bounds__(kWg) void kc_fill(double* out, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * kWg + threadIdx.x;
    if (i < n) out[i] = v;
}

__global__ __launch_bounds__(kWg) void kc_cost_final(Ws w, bool trial) {
    Ctl* ctl = w.ctl;
    if (ctl->bad || (trial && ctl->done)) return;
    __shared__ double sm[kWg];
    double acc = 0.0;
    for (int i = threadIdx.x; i < w.nb; i += kWg) acc = acc + w.cpart[i];
    const double s = 0.5 * block_sum(acc, sm);
    if (threadIdx.x == 0) {
        const int flag = ctl->depth_flag;
        ctl->depth_flag = 0;
        ctl->depth_bad = flag;
        const double cost = flag ? INFINITY : s;
        if (trial) {
            ctl->cost_trial = cost;
        } else {
            ctl->cost = cost;
            ctl->gmax_bits = 0ull;
        }
    }
}

// V = sum Jp^T Jp, g_p = sum Jp^T r over the point's segment, in sequence; one lane per point.
__global__ __launch_bounds__(kWg) void kc_point_blocks(Ws w, bool solver) {
    if (w.ctl->bad) return;
    const int p = blockIdx.x * kWg + threadIdx.x;
    if (p >= w.N) return;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int64_t m = w.pt_off[p]; m < w.pt_off[p + 1]; ++m) {
        const double* J = w.Jp + 6 * m;
        const double r0 = w.r[2 * m], r1 = w.r[2 * m + 1];
        int k = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b) {
                acc[k] = acc[k] + (J[a] * J[b] + J[3 + a] * J[3 + b]);
                ++k;
            }
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[6 + a] = acc[6 + a] + (J[a] * r0 + J[3 + a] * r1);
    }
    double* V = w.V + 9 * (int64_t)p;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            V[a * 3 + b] = acc[k];
            V[b * 3 + a] = acc[k];
            ++k;
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w.gp[3 * (int64_t)p + a] = acc[6 + a];
        if (solver) gmax_update(w.ctl, acc[6 + a]);
    }
}

// Stage 1, three launches (chunk_reduce holds NV * 256 doubles of LDS): U upper triangle + g_c (27),
// B = Jc^T Jk (30), H upper triangle + g_k (20).
__global__ __launch_bounds__(kWg) void kc_cam_partial_u(Ws w) {
    if (w.ctl->bad) return;
    chunk_reduce<27>(w, w.part27, [&](int64_t m, double* v) {
        const double* J = w.Jc + 12 * m;
        const double r0 = w.r[2 * m], r1 = w.r[2 * m + 1];
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) v[k++] = J[a] * J[b] + J[6 + a] * J[6 + b];
#pragma unroll
        for (int a = 0; a < 6; ++a) v[21 + a] = J[a] * r0 + J[6 + a] * r1;
    });
}

__global__ __launch_bounds__(kWg) void kc_cam_partial_b(Ws w) {
    if (w.ctl->bad) return;
    chunk_reduce<30>(w, w.part30, [&](int64_t m, double* v) {
        const double* J = w.Jc + 12 * m;
        const double* Q = w.Jk + 10 * m;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int j = 0; j < 5; ++j) v[a * 5 + j] = J[a] * Q[j] + J[6 + a] * Q[5 + j];
    });
}

__global__ __launch_bounds__(kWg) void kc_cam_partial_h(Ws w) {
    if (w.ctl->bad) return;
    chunk_reduce<20>(w, w.part20, [&](int64_t m, double* v) {
        const double* Q = w.Jk + 10 * m;
        const double r0 = w.r[2 * m], r1 = w.r[2 * m + 1];
        int k = 0;
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = a; b < 5; ++b) v[k++] = Q[a] * Q[b] + Q[5 + a] * Q[5 + b];
#pragma unroll
        for (int a = 0; a < 5; ++a) v[15 + a] = Q[a] * r0 + Q[5 + a] * r1;
    });
}

// Stage 2: the chunks of a camera in sequence; one lane per camera.  U, g_c and B are final, the
// 20 values of H and g_k go to camH for the group sum.
__global__ __launch_bounds__(kWg) void kc_cam_blocks(Ws w, bool solver) {
    if (w.ctl->bad) return;
    const int c = blockIdx.x * kWg + threadIdx.x;
    if (c >= w.C) return;
    const int b0 = w.chunk_base[c], b1 = w.chunk_base[c + 1];
    {
        double acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0.0;
        for (int b = b0; b < b1; ++b)
#pragma unroll
            for (int k = 0; k < 27; ++k) acc[k] = acc[k] + w.part27[(int64_t)b * 27 + k];
        double* U = w.U + 36 * (int64_t)c;
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) {
                U[a * 6 + b] = acc[k];
                U[b * 6 + a] = acc[k];
                ++k;
            }
        const bool fx = is_fixed(w.fixed, c);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            w.gc[6 * (int64_t)c + a] = acc[21 + a];
            if (solver && !fx) gmax_update(w.ctl, acc[21 + a]);
        }
    }
    {
        double acc[30];
#pragma unroll
        for (int k = 0; k < 30; ++k) acc[k] = 0.0;
        for (int b = b0; b < b1; ++b)
#pragma unroll
            for (int k = 0; k < 30; ++k) acc[k] = acc[k] + w.part30[(int64_t)b * 30 + k];
#pragma unroll
        for (int k = 0; k < 30; ++k) w.B[30 * (int64_t)c + k] = acc[k];
    }
    {
        double acc[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) acc[k] = 0.0;
        for (int b = b0; b < b1; ++b)
#pragma unroll
            for (int k = 0; k < 20; ++k) acc[k] = acc[k] + w.part20[(int64_t)b * 20 + k];
#pragma unroll
        for (int k = 0; k < 20; ++k) w.camH[20 * (int64_t)c + k] = acc[k];
    }
}

// Stage 3: H (5x5) and g_k of a group from its cameras; one workgroup per group.
__global__ __launch_bounds__(kWg) void kc_group_blocks(Ws w, bool solver) {
    if (w.ctl->bad) return;
    __shared__ double sm[kWg];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int lo = w.grp_off[g], hi = w.grp_off[g + 1];
    double tot[20];
    for (int k = 0; k < 20; ++k) {
        double acc = 0.0;
        for (int j = lo + tid; j < hi; j += kWg) acc = acc + w.camH[20 * (int64_t)w.grp_cams[j] + k];
        tot[k] = block_sum(acc, sm);
    }
    if (tid == 0) {
        double* H = w.H + 25 * (int64_t)g;
        int k = 0;
        for (int a = 0; a < 5; ++a)
            for (int b = a; b < 5; ++b) {
                H[a * 5 + b] = tot[k];
                H[b * 5 + a] = tot[k];
                ++k;
            }
        for (int a = 0; a < 5; ++a) {
            w.gk[5 * (int64_t)g + a] = tot[15 + a];
            if (solver && w.mask[a]) gmax_update(w.ctl, tot[15 + a]);
        }
    }
}

__global__ void kc_gate(Ws w) {
    Ctl* ctl = w.ctl;
    if (ctl->bad || ctl->done) return;
    const double gmax = __longlong_as_double((long long)ctl->gmax_bits);
    if (gmax <= ctl->gtol) {
        ctl->status = 1;
        ctl->done = 1;
    } else if (ctl->rel <= ctl->ftol) {
        ctl->status = 2;
        ctl->done = 1;
    }
}

// V*^-1 per point, U* and U*^-1 per camera (zero for a fixed camera), H* and H*^-1 per group.
__global__ __launch_bounds__(kWg) void kc_damp(Ws w, double lam_arg, bool from_ctl) {
    if (w.ctl->bad || w.ctl->done) return;
    const double lam = from_ctl ? w.ctl->lambda : lam_arg;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.N) damp_invert<3>(w.V + 9 * (int64_t)i, lam, nullptr, w.Vi + 9 * (int64_t)i);
    if (i < w.C) {
        damp_invert<6>(w.U + 36 * (int64_t)i, lam, w.Us + 36 * (int64_t)i, w.Ui + 36 * (int64_t)i);
        if (is_fixed(w.fixed, i))
            for (int k = 0; k < 36; ++k) w.Ui[36 * (int64_t)i + k] = 0.0;
    }
    if (i < w.G) damp_invert<5>(w.H + 25 * (int64_t)i, lam, w.Hs + 25 * (int64_t)i, w.Hi + 25 * (int64_t)i);
}

// By point: s = sum Jp^T ((fixed ? 0 : Jc x_c) + Jk x_k) in sequence (entries of x_k at masked
// components are not read); y as in ba_global.hip.  x = (x_c, x_k).  One lane per point.
__global__ __launch_bounds__(kWg) void kc_point_pass(Ws w, int mode, const double* x, bool cg) {
    if (w.ctl->bad || w.ctl->done || (cg && w.ctl->cg_done)) return;
    const int p = blockIdx.x * kWg + threadIdx.x;
    if (p >= w.N) return;
    double s[3] = {0.0, 0.0, 0.0};
    if (mode != kRhs) {
        const double* xk0 = x + 6 * (int64_t)w.C;
        for (int64_t m = w.pt_off[p]; m < w.pt_off[p + 1]; ++m) {
            const int c = w.oc[m];
            double t0 = 0.0, t1 = 0.0;
            if (!is_fixed(w.fixed, c)) {
                const double* J = w.Jc + 12 * m;
                const double* xc = x + 6 * (int64_t)c;
                t0 = J[0] * xc[0];
                t1 = J[6] * xc[0];
#pragma unroll
                for (int j = 1; j < 6; ++j) {
                    t0 = t0 + J[j] * xc[j];
                    t1 = t1 + J[6 + j] * xc[j];
                }
            }
            const double* Q = w.Jk + 10 * m;
            const double* xk = xk0 + 5 * (int64_t)w.grp[c];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const double xj = w.mask[j] ? xk[j] : 0.0;
                t0 = t0 + Q[j] * xj;
                t1 = t1 + Q[5 + j] * xj;
            }
            const double* Jp = w.Jp + 6 * m;
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = s[k] + (Jp[k] * t0 + Jp[3 + k] * t1);
        }
    }
    const double* g = w.gp + 3 * (int64_t)p;
    if (mode == kRhs) {
        s[0] = g[0]; s[1] = g[1]; s[2] = g[2];
    } else if (mode == kBacksub) {
        s[0] = g[0] + s[0]; s[1] = g[1] + s[1]; s[2] = g[2] + s[2];
    }
    const double* Vi = w.Vi + 9 * (int64_t)p;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double yi = (Vi[3 * i] * s[0] + Vi[3 * i + 1] * s[1]) + Vi[3 * i + 2] * s[2];
        w.y[3 * (int64_t)p + i] = mode == kBacksub ? -yi : yi;
    }
}

// By camera, stage 1: (Jc^T w, Jk^T w), w = Jp y_p, 11 values per observation through the chunk tree.
__global__ __launch_bounds__(kWg) void kc_cam_pass(Ws w, bool cg) {
    if (w.ctl->bad || w.ctl->done || (cg && w.ctl->cg_done)) return;
    chunk_reduce<11>(w, w.part11, [&](int64_t m, double* v) {
        const double* Jp = w.Jp + 6 * m;
        const double* y = w.y + 3 * (int64_t)w.op[m];
        const double w0 = (Jp[0] * y[0] + Jp[1] * y[1]) + Jp[2] * y[2];
        const double w1 = (Jp[3] * y[0] + Jp[4] * y[1]) + Jp[5] * y[2];
        const double* J = w.Jc + 12 * m;
        const double* Q = w.Jk + 10 * m;
#pragma unroll
        for (int a = 0; a < 6; ++a) v[a] = J[a] * w0 + J[6 + a] * w1;
#pragma unroll
        for (int j = 0; j < 5; ++j) v[6 + j] = Q[j] * w0 + Q[5 + j] * w1;
    });
}

__device__ __forceinline__ double cam_chunks_sum(const Ws& w, int c, int a) {
    double o = 0.0;
    for (int b = w.chunk_base[c]; b < w.chunk_base[c + 1]; ++b) o = o + w.part11[(int64_t)b * 11 + a];
    return o;
}

// By group: gq[g][j] = sum over the group's cameras of ((fixed or no x) ? 0 : (B^T x_c)[j]) minus the
// camera's chunk sum of (Jk^T w)[j]; one workgroup per group, the group order of the file header.
__global__ __launch_bounds__(kWg) void kc_group_pass(Ws w, const double* x, bool cg) {
    if (w.ctl->bad || w.ctl->done || (cg && w.ctl->cg_done)) return;
    __shared__ double sm[kWg];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int lo = w.grp_off[g], hi = w.grp_off[g + 1];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lo + tid; i < hi; i += kWg) {
        const int c = w.grp_cams[i];
        const bool use = x != nullptr && !is_fixed(w.fixed, c);
        const double* B = w.B + 30 * (int64_t)c;
        const double* xc = use ? x + 6 * (int64_t)c : nullptr;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            double bt = 0.0;
            if (use) {
                bt = B[j] * xc[0];
#pragma unroll
                for (int a = 1; a < 6; ++a) bt = bt + B[a * 5 + j] * xc[a];
            }
            acc[j] = acc[j] + (bt - cam_chunks_sum(w, c, 6 + j));
        }
    }
    for (int j = 0; j < 5; ++j) {
        const double s = block_sum(acc[j], sm);
        if (tid == 0) w.gq[5 * (int64_t)g + j] = s;
    }
}

__device__ __forceinline__ double block_row(const double* A, const double* v, int c, int a) {
    const double* row = A + 36 * (int64_t)c + 6 * a;
    const double* vc = v + 6 * (int64_t)c;
    double acc = row[0] * vc[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) acc = acc + row[j] * vc[j];
    return acc;
}

__device__ __forceinline__ double group_row(const double* A, const double* vk, int g, int a) {
    const double* row = A + 25 * (int64_t)g + 5 * a;
    const double* vg = vk + 5 * (int64_t)g;
    double acc = row[0] * vg[0];
#pragma unroll
    for (int j = 1; j < 5; ++j) acc = acc + row[j] * vg[j];
    return acc;
}

// Entry i of S~ x~ from the stage-1 partials and gq: rows of fixed cameras and of masked
// components are exactly 0.
__device__ __forceinline__ double matvec_entry(const Ws& w, const double* x, int i) {
    const int n6 = 6 * w.C;
    const double* xk = x + n6;
    if (i < n6) {
        const int c = i / 6, a = i % 6;
        if (is_fixed(w.fixed, c)) return 0.0;
        const double* B = w.B + 30 * (int64_t)c + 5 * a;
        const double* xg = xk + 5 * (int64_t)w.grp[c];
        double bx = B[0] * (w.mask[0] ? xg[0] : 0.0);
#pragma unroll
        for (int j = 1; j < 5; ++j) bx = bx + B[j] * (w.mask[j] ? xg[j] : 0.0);
        return (block_row(w.Us, x, c, a) + bx) - cam_chunks_sum(w, c, a);
    }
    const int g = (i - n6) / 5, a = (i - n6) % 5;
    if (!w.mask[a]) return 0.0;
    const double* row = w.Hs + 25 * (int64_t)g + 5 * a;
    const double* xg = xk + 5 * (int64_t)g;
    double acc = row[0] * (w.mask[0] ? xg[0] : 0.0);
#pragma unroll
    for (int j = 1; j < 5; ++j) acc = acc + row[j] * (w.mask[j] ? xg[j] : 0.0);
    return acc + w.gq[5 * (int64_t)g + a];
}

__device__ __forceinline__ double precond_entry(const Ws& w, const double* v, int i) {
    const int n6 = 6 * w.C;
    if (i < n6) return block_row(w.Ui, v, i / 6, i % 6);
    return group_row(w.Hi, v + n6, (i - n6) / 5, (i - n6) % 5);
}

__global__ __launch_bounds__(kWg) void kc_matvec_out(Ws w, const double* x, double* out) {
    if (w.ctl->bad) return;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i >= 6 * w.C + 5 * w.G) return;
    out[i] = matvec_entry(w, x, i);
}

// b = -(g~ - A~^T Jp V*^-1 g_p) (gq holds minus the group sums), x = 0, r = b, z = M^-1 r, p = z.
__global__ __launch_bounds__(kWg) void kc_cg_init(Ws w) {
    Ctl* ctl = w.ctl;
    if (ctl->bad || ctl->done) return;
    __shared__ double sm[kWg];
    const int n6 = 6 * w.C, n = n6 + 5 * w.G, tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n; i += kWg) {
        double b;
        if (i < n6) {
            const int c = i / 6, a = i % 6;
            b = is_fixed(w.fixed, c) ? 0.0 : -(w.gc[i] - cam_chunks_sum(w, c, a));
        } else {
            b = w.mask[(i - n6) % 5] ? -(w.gk[i - n6] + w.gq[i - n6]) : 0.0;
        }
        w.b[i] = b;
        w.x[i] = 0.0;
        w.rr[i] = b;
        acc = acc + b * b;
    }
    const double bb = block_sum(acc, sm);   // also makes rr visible to the workgroup
    acc = 0.0;
    for (int i = tid; i < n; i += kWg) {
        const double z = precond_entry(w, w.rr, i);
        w.z[i] = z;
        w.p[i] = z;
        acc = acc + w.rr[i] * z;
    }
    const double rz = block_sum(acc, sm);
    if (tid == 0) {
        ctl->bb = bb;
        ctl->rz = rz;
        ctl->cg_iters = 0;
        ctl->cg_done = bb > 0.0 ? 0 : 1;
    }
}

// One PCG iteration, as ba_global.hip's k_cg_step over 6C + 5G entries.
__global__ __launch_bounds__(kWg) void kc_cg_step(Ws w) {
    Ctl* ctl = w.ctl;
    if (ctl->bad || ctl->done || ctl->cg_done) return;
    __shared__ double sm[kWg];
    const int n = 6 * w.C + 5 * w.G, tid = threadIdx.x;
    const double rz = ctl->rz, bb = ctl->bb, eta = ctl->eta;
    const int iters = ctl->cg_iters + 1;
    double acc = 0.0;
    for (int i = tid; i < n; i += kWg) {
        const double q = matvec_entry(w, w.p, i);
        w.q[i] = q;
        acc = acc + w.p[i] * q;
    }
    const double pq = block_sum(acc, sm);
    if (!(pq > 0.0)) {
        if (tid == 0) ctl->cg_done = 1;
        return;
    }
    const double alpha = rz / pq;
    acc = 0.0;
    for (int i = tid; i < n; i += kWg) {
        w.x[i] = w.x[i] + alpha * w.p[i];
        const double ri = w.rr[i] - alpha * w.q[i];
        w.rr[i] = ri;
        acc = acc + ri * ri;
    }
    const double r2 = block_sum(acc, sm);
    if (sqrt(r2) <= eta * sqrt(bb)) {
        if (tid == 0) {
            ctl->cg_done = 1;
            ctl->cg_iters = iters;
        }
        return;
    }
    acc = 0.0;
    for (int i = tid; i < n; i += kWg) {
        const double z = precond_entry(w, w.rr, i);
        w.z[i] = z;
        acc = acc + w.rr[i] * z;
    }
    const double rzn = block_sum(acc, sm);
    const double beta = rzn / rz;
    for (int i = tid; i < n; i += kWg) w.p[i] = w.z[i] + beta * w.p[i];
    if (tid == 0) {
        ctl->rz = rzn;
        ctl->cg_iters = iters;
    }
}

// Trial state: cameras and points as in ba_global.hip, theta <- theta + x_k at free components.
__global__ __launch_bounds__(kWg) void kc_trial(Ws w) {
    if (w.ctl->bad || w.ctl->done) return;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.C) {
        const double* R = w.R + 9 * (int64_t)i;
        double* Rn = w.Rt + 9 * (int64_t)i;
        if (is_fixed(w.fixed, i)) {
            for (int k = 0; k < 9; ++k) Rn[k] = R[k];
            for (int k = 0; k < 3; ++k) w.tt[3 * (int64_t)i + k] = w.t[3 * (int64_t)i + k];
        } else {
            const double* d = w.x + 6 * (int64_t)i;
            double E[9];
            rodrigues(d, E);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    Rn[3 * a + j] = (E[3 * a] * R[j] + E[3 * a + 1] * R[3 + j]) + E[3 * a + 2] * R[6 + j];
            for (int k = 0; k < 3; ++k) w.tt[3 * (int64_t)i + k] = w.t[3 * (int64_t)i + k] + d[3 + k];
        }
    }
    if (i < w.N)
        for (int k = 0; k < 3; ++k) w.Xt[3 * (int64_t)i + k] = w.X[3 * (int64_t)i + k] + w.y[3 * (int64_t)i + k];
    if (i < w.G) {
        const double* xk = w.x + 6 * (int64_t)w.C + 5 * (int64_t)i;
        for (int k = 0; k < 5; ++k)
            w.tht[5 * (int64_t)i + k] = w.mask[k] ? w.th[5 * (int64_t)i + k] + xk[k] : w.th[5 * (int64_t)i + k];
    }
}

__global__ void kc_step(Ws w) {
    Ctl* ctl = w.ctl;
    if (ctl->bad || ctl->done) return;
    ctl->cg_total += ctl->cg_iters;
    if (ctl->cost_trial < ctl->cost) {
        ctl->rel = (ctl->cost - ctl->cost_trial) / ctl->cost;
        ctl->cost = ctl->cost_trial;
        ctl->lambda = fmax(ctl->lambda / 3.0, kLambdaMin);
        ctl->accepted = 1;
        ctl->n_accept += 1;
    } else {
        ctl->accepted = 0;
        ctl->lambda = ctl->lambda * 4.0;
        if (ctl->lambda > kLambdaMax) {
            ctl->status = 3;
            ctl->done = 1;
        }
    }
}

__global__ __launch_bounds__(kWg) void kc_accept(Ws w) {
    if (w.ctl->bad || w.ctl->done || !w.ctl->accepted) return;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.C) {
        for (int k = 0; k < 9; ++k) w.R[9 * (int64_t)i + k] = w.Rt[9 * (int64_t)i + k];
        for (int k = 0; k < 3; ++k) w.t[3 * (int64_t)i + k] = w.tt[3 * (int64_t)i + k];
    }
    if (i < w.N)
        for (int k = 0; k < 3; ++k) w.X[3 * (int64_t)i + k] = w.Xt[3 * (int64_t)i + k];
    if (i < w.G)
        for (int k = 0; k < 5; ++k) w.th[5 * (int64_t)i + k] = w.tht[5 * (int64_t)i + k];
}

// Write the accepted state back: free cameras that have observations, every point, and the free
// components of a group that has a camera.
__global__ __launch_bounds__(kWg) void kc_finish(Ws w, double* cam, double* X, double* theta) {
    if (w.ctl->bad || w.ctl->n_accept == 0) return;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.C && !is_fixed(w.fixed, i) && w.cam_off[i + 1] > w.cam_off[i]) {
        rodrigues_inverse(w.R + 9 * (int64_t)i, cam + 6 * (int64_t)i);
        for (int k = 0; k < 3; ++k) cam[6 * (int64_t)i + 3 + k] = w.t[3 * (int64_t)i + k];
    }
    if (i < w.N)
        for (int k = 0; k < 3; ++k) X[3 * (int64_t)i + k] = w.X[3 * (int64_t)i + k];
    if (i < w.G && w.grp_off[i + 1] > w.grp_off[i])
        for (int k = 0; k < 5; ++k)
            if (w.mask[k]) theta[5 * (int64_t)i + k] = w.th[5 * (int64_t)i + k];
}

// ---------------------------------------------------------------------------
// Host side.  Carve (base == nullptr: size only); the flags as in ba_global.hip.
void carve(Arena& a, Ws& w, bool solver, bool own_lin, bool own_damp) {
    const size_t C = (size_t)w.C, N = (size_t)w.N, M = (size_t)w.M, G = (size_t)w.G, n = 6 * C + 5 * G;
    w.ctl = a.take<Ctl>(1);
    w.chunk_base = a.take<int>(C + 1);
    w.chunk_cam = a.take<int>((size_t)w.tmax);
    w.grp_off = a.take<int>(G + 2);
    w.grp_cams = a.take<int>(C);
    w.cpart = a.take<double>((size_t)w.nb);
    w.part27 = a.take<double>((size_t)w.tmax * 27);
    w.part30 = a.take<double>((size_t)w.tmax * 30);
    w.part20 = a.take<double>((size_t)w.tmax * 20);
    w.part11 = a.take<double>((size_t)w.tmax * 11);
    w.camH = a.take<double>(20 * C);
    w.gq = a.take<double>(5 * G);
    w.R = a.take<double>(9 * C);
    w.t = a.take<double>(3 * C);
    w.X = a.take<double>(3 * N);
    w.th = a.take<double>(5 * G);
    if (own_lin) {
        w.r = a.take<double>(2 * M);
        w.Jc = a.take<double>(12 * M);
        w.Jk = a.take<double>(10 * M);
        w.Jp = a.take<double>(6 * M);
        w.U = a.take<double>(36 * C);
        w.gc = a.take<double>(6 * C);
        w.B = a.take<double>(30 * C);
        w.H = a.take<double>(25 * G);
        w.gk = a.take<double>(5 * G);
        w.V = a.take<double>(9 * N);
        w.gp = a.take<double>(3 * N);
    }
    if (own_damp) {
        w.Us = a.take<double>(36 * C);
        w.Ui = a.take<double>(36 * C);
        w.Hs = a.take<double>(25 * G);
        w.Hi = a.take<double>(25 * G);
        w.Vi = a.take<double>(9 * N);
        w.y = a.take<double>(3 * N);
    }
    if (solver) {
        w.Rt = a.take<double>(9 * C);
        w.tt = a.take<double>(3 * C);
        w.Xt = a.take<double>(3 * N);
        w.tht = a.take<double>(5 * G);
        w.b = a.take<double>(n);
        w.x = a.take<double>(n);
        w.rr = a.take<double>(n);
        w.z = a.take<double>(n);
        w.p = a.take<double>(n);
        w.q = a.take<double>(n);
    }
}

int alloc_ws(const char* who, Ws& w, bool solver, bool own_lin, bool own_damp, hipStream_t st, void** scratch) {
    w.nb = grid_of(w.M);
    w.tmax = (int)(w.M / kChunk) + w.C + 1;
    Arena size;
    carve(size, w, solver, own_lin, own_damp);
    if (scratch_alloc(scratch, size.used, st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: scratch allocation failed", who);
        return SFMHIP_E_HIP;
    }
    Arena a;
    a.base = static_cast<char*>(*scratch);
    carve(a, w, solver, own_lin, own_damp);
    if (hipMemsetAsync(w.ctl, 0, sizeof(Ctl), st) != hipSuccess) {
        scratch_free(*scratch, st);
        set_error("%s: %s", who, hipGetErrorString(hipGetLastError()));
        return SFMHIP_E_HIP;
    }
    return SFMHIP_OK;
}

int read_ctl(const char* who, const Ws& w, Ctl* host, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(host, w.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e));
        return SFMHIP_E_HIP;
    }
    return SFMHIP_OK;
}

void launch_validate(const Ws& w, hipStream_t st) {
    const int64_t n = std::max<int64_t>(std::max<int64_t>(w.M, 5), std::max(w.C, w.N) + 1);
    hipLaunchKernelGGL(kc_validate, dim3(grid_of(n)), dim3(kWg), 0, st, w);
    hipLaunchKernelGGL(kc_layout, dim3(1), dim3(1), 0, st, w);
}

template <bool JAC>
void launch_residuals(const Ws& w, int loss, const double* R, const double* t, const double* X, const double* th,
                      bool trial, hipStream_t st) {
    const dim3 g(w.nb), b(kWg);
    switch (loss) {
    case kHuber: hipLaunchKernelGGL((kc_linearize<JAC, kHuber>), g, b, 0, st, w, R, t, X, th, trial); break;
    case kSoftL1: hipLaunchKernelGGL((kc_linearize<JAC, kSoftL1>), g, b, 0, st, w, R, t, X, th, trial); break;
    case kCauchy: hipLaunchKernelGGL((kc_linearize<JAC, kCauchy>), g, b, 0, st, w, R, t, X, th, trial); break;
    default: hipLaunchKernelGGL((kc_linearize<JAC, kLinear>), g, b, 0, st, w, R, t, X, th, trial); break;
    }
}

// Linearise at (R, t, X, theta) of the workspace: 8 launches.
void launch_linearize(const Ws& w, int loss, bool solver, hipStream_t st) {
    launch_residuals<true>(w, loss, w.R, w.t, w.X, w.th, false, st);
    hipLaunchKernelGGL(kc_cost_final, dim3(1), dim3(kWg), 0, st, w, false);
    hipLaunchKernelGGL(kc_point_blocks, dim3(grid_of(w.N)), dim3(kWg), 0, st, w, solver);
    hipLaunchKernelGGL(kc_cam_partial_u, dim3(w.tmax), dim3(kWg), 0, st, w);
    hipLaunchKernelGGL(kc_cam_partial_b, dim3(w.tmax), dim3(kWg), 0, st, w);
    hipLaunchKernelGGL(kc_cam_partial_h, dim3(w.tmax), dim3(kWg), 0, st, w);
    hipLaunchKernelGGL(kc_cam_blocks, dim3(grid_of(w.C)), dim3(kWg), 0, st, w, solver);
    if (w.G > 0) hipLaunchKernelGGL(kc_group_blocks, dim3(w.G), dim3(kWg), 0, st, w, solver);
}

// The by-point pass, the by-camera chunk pass and the group pass of one product / right-hand side.
void launch_passes(const Ws& w, int mode, const double* x, bool cg, hipStream_t st) {
    hipLaunchKernelGGL(kc_point_pass, dim3(grid_of(w.N)), dim3(kWg), 0, st, w, mode, x, cg);
    hipLaunchKernelGGL(kc_cam_pass, dim3(w.tmax), dim3(kWg), 0, st, w, cg);
    if (w.G > 0)
        hipLaunchKernelGGL(kc_group_pass, dim3(w.G), dim3(kWg), 0, st, w, mode == kRhs ? (const double*)nullptr : x,
                           cg);
}

bool common_args_ok(const char* who, const void* oc, const void* op, const void* pt_off, const void* cam_perm,
                    const void* cam_off, const void* grp, const void* mask, int C, int N, int G, int64_t M) {
    if (C < 0 || N < 0 || M < 0 || G < 0) {
        set_error("%s: negative size", who);
        return false;
    }
    if (M > INT32_MAX || C > (1 << 20) || N > INT32_MAX / 16 || G > kMaxGroups) {
        set_error("%s: size out of range", who);
        return false;
    }
    if (C > 0 && G == 0) {
        set_error("%s: cameras need at least one intrinsics group", who);
        return false;
    }
    if (!pt_off || !cam_off || !mask || (M > 0 && (!oc || !op || !cam_perm)) || (C > 0 && !grp)) {
        set_error("%s: null pointer", who);
        return false;
    }
    return true;
}

bool loss_args_ok(const char* who, int loss, double f_scale) {
    if (loss < kLinear || loss > kCauchy) {
        set_error("%s: unknown loss code %d (0 linear, 1 huber, 2 soft_l1, 3 cauchy)", who, loss);
        return false;
    }
    if (!(f_scale > 0.0) || !std::isfinite(f_scale)) {
        set_error("%s: f_scale must be positive and finite", who);
        return false;
    }
    return true;
}

const char* kBadStructure = "index or group out of range, mask byte not 0 / 1, offsets not monotone or orders inconsistent";

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_ba_calib_linearize(const double* cam, const double* theta, const double* asp,
                                         const int32_t* cam_group, const uint8_t* mask, const double* X,
                                         const int32_t* obs_cam, const int32_t* obs_pt, const double* pts2d,
                                         const int64_t* pt_off, const int64_t* cam_perm, const int64_t* cam_off, int C,
                                         int N, int G, int64_t M, double* r, double* Jc, double* Jk, double* Jp,
                                         double* U, double* g_c, double* B, double* H, double* g_k, double* V,
                                         double* g_p, double* cost, void* stream, int loss, double f_scale,
                                         double* weight) {
    const char* who = "sfmhip_ba_calib_linearize";
    if (!loss_args_ok(who, loss, f_scale)) return SFMHIP_E_ARG;
    if (!common_args_ok(who, obs_cam, obs_pt, pt_off, cam_perm, cam_off, cam_group, mask, C, N, G, M))
        return SFMHIP_E_ARG;
    SFMHIP_REQUIRE(cost && (C == 0 || (cam && U && g_c && B)) && (G == 0 || (theta && asp && H && g_k)) &&
                       (N == 0 || (X && V && g_p)) && (M == 0 || (pts2d && r && Jc && Jk && Jp)),
                   "%s: null pointer", who);
    hipStream_t st = as_stream(stream);
    Ws w = {};
    w.asp = asp; w.grp = cam_group; w.mask = mask; w.oc = obs_cam; w.op = obs_pt; w.uv = pts2d;
    w.pt_off = pt_off; w.cam_perm = cam_perm; w.cam_off = cam_off;
    w.C = C; w.N = N; w.G = G; w.M = M;
    w.r = r; w.Jc = Jc; w.Jk = Jk; w.Jp = Jp; w.U = U; w.gc = g_c; w.B = B; w.H = H; w.gk = g_k; w.V = V; w.gp = g_p;
    w.f2 = f_scale * f_scale; w.wout = weight;
    void* scratch = nullptr;
    int rc = alloc_ws(who, w, false, false, false, st, &scratch);
    if (rc != SFMHIP_OK) return rc;
    launch_validate(w, st);
    Ctl h;
    rc = read_ctl(who, w, &h, st);    // nothing is written before the structure is known to be sound
    if (rc == SFMHIP_OK && h.bad) {
        set_error("%s: %s", who, kBadStructure);
        rc = SFMHIP_E_ARG;
    }
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(kc_init, dim3(grid_of(std::max(std::max(C, N), G))), dim3(kWg), 0, st, w, cam, X, theta);
        launch_linearize(w, loss, false, st);
        if (loss == kLinear && weight != nullptr && M > 0)
            hipLaunchKernelGGL(kc_fill, dim3(grid_of(M)), dim3(kWg), 0, st, weight, M, 1.0);
        rc = check_launch("ba_calib linearize");
        if (rc == SFMHIP_OK) rc = read_ctl(who, w, &h, st);
        if (rc == SFMHIP_OK) *cost = h.cost;
    }
    scratch_free(scratch, st);
    return rc;
}

extern "C" int sfmhip_ba_calib_matvec(const double* Jc, const double* Jk, const double* Jp, const double* U,
                                      const double* B, const double* H, const double* V, const int32_t* cam_group,
                                      const uint8_t* mask, const int32_t* obs_cam, const int32_t* obs_pt,
                                      const int64_t* pt_off, const int64_t* cam_perm, const int64_t* cam_off,
                                      const uint8_t* cam_fixed, int C, int N, int G, int64_t M, double lambda,
                                      const double* x, double* out, void* stream) {
    const char* who = "sfmhip_ba_calib_matvec";
    if (!common_args_ok(who, obs_cam, obs_pt, pt_off, cam_perm, cam_off, cam_group, mask, C, N, G, M))
        return SFMHIP_E_ARG;
    SFMHIP_REQUIRE((C == 0 || (U && B)) && (G == 0 || H) && (C + G == 0 || (x && out)) && (N == 0 || V) &&
                       (M == 0 || (Jc && Jk && Jp)), "%s: null pointer", who);
    SFMHIP_REQUIRE(lambda >= 0.0, "%s: lambda must be non-negative", who);
    hipStream_t st = as_stream(stream);
    Ws w = {};
    w.grp = cam_group; w.mask = mask; w.oc = obs_cam; w.op = obs_pt; w.pt_off = pt_off; w.cam_perm = cam_perm;
    w.cam_off = cam_off; w.fixed = cam_fixed;
    w.C = C; w.N = N; w.G = G; w.M = M;
    w.Jc = const_cast<double*>(Jc); w.Jk = const_cast<double*>(Jk); w.Jp = const_cast<double*>(Jp);
    w.U = const_cast<double*>(U); w.B = const_cast<double*>(B); w.H = const_cast<double*>(H);
    w.V = const_cast<double*>(V);
    void* scratch = nullptr;
    int rc = alloc_ws(who, w, false, false, true, st, &scratch);
    if (rc != SFMHIP_OK) return rc;
    launch_validate(w, st);
    Ctl h;
    rc = read_ctl(who, w, &h, st);
    if (rc == SFMHIP_OK && h.bad) {
        set_error("%s: %s", who, kBadStructure);
        rc = SFMHIP_E_ARG;
    }
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(kc_damp, dim3(grid_of(std::max(std::max(C, N), G))), dim3(kWg), 0, st, w, lambda, false);
        launch_passes(w, kMatvec, x, false, st);
        hipLaunchKernelGGL(kc_matvec_out, dim3(grid_of(6 * (int64_t)C + 5 * (int64_t)G)), dim3(kWg), 0, st, w, x, out);
        rc = check_launch("ba_calib matvec");
    }
    scratch_free(scratch, st);
    return rc;
}

extern "C" int sfmhip_ba_calib(double* cam, double* theta, const double* asp, const int32_t* cam_group,
                               const uint8_t* mask, double* X, const int32_t* obs_cam, const int32_t* obs_pt,
                               const double* pts2d, const int64_t* pt_off, const int64_t* cam_perm,
                               const int64_t* cam_off, const uint8_t* cam_fixed, int C, int N, int G, int64_t M,
                               double gtol, double ftol, double eta, int max_iter, int max_cg, double* cost,
                               int32_t* info, void* stream, int loss, double f_scale, double* obs_res2) {
    const char* who = "sfmhip_ba_calib";
    if (!loss_args_ok(who, loss, f_scale)) return SFMHIP_E_ARG;
    if (!common_args_ok(who, obs_cam, obs_pt, pt_off, cam_perm, cam_off, cam_group, mask, C, N, G, M))
        return SFMHIP_E_ARG;
    SFMHIP_REQUIRE(cost && info && (C == 0 || cam) && (G == 0 || (theta && asp)) && (N == 0 || X) && (M == 0 || pts2d),
                   "%s: null pointer", who);
    SFMHIP_REQUIRE(max_iter >= 1 && max_cg >= 0 && max_cg <= 4096, "%s: max_iter >= 1 and 0 <= max_cg <= 4096", who);
    SFMHIP_REQUIRE(gtol >= 0.0 && ftol >= 0.0 && eta >= 0.0, "%s: negative tolerance", who);
    hipStream_t st = as_stream(stream);
    Ws w = {};
    w.asp = asp; w.grp = cam_group; w.mask = mask; w.oc = obs_cam; w.op = obs_pt; w.uv = pts2d;
    w.pt_off = pt_off; w.cam_perm = cam_perm; w.cam_off = cam_off; w.fixed = cam_fixed;
    w.C = C; w.N = N; w.G = G; w.M = M;
    w.f2 = f_scale * f_scale;
    void* scratch = nullptr;
    int rc = alloc_ws(who, w, true, true, true, st, &scratch);
    if (rc != SFMHIP_OK) return rc;
    cost[0] = cost[1] = 0.0;
    info[0] = -1; info[1] = info[2] = info[3] = 0;
    Ctl h;
    {   // tolerances and the start of the step control
        Ctl init = {};
        init.lambda = kLambda0;
        init.rel = INFINITY;
        init.gtol = gtol; init.ftol = ftol; init.eta = eta;
        if (hipMemcpyAsync(w.ctl, &init, sizeof(Ctl), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {   // `init` leaves scope
            scratch_free(scratch, st);
            set_error("%s: %s", who, hipGetErrorString(hipGetLastError()));
            return SFMHIP_E_HIP;
        }
    }
    const int gcn = grid_of(std::max(std::max(C, N), G));
    launch_validate(w, st);
    hipLaunchKernelGGL(kc_init, dim3(gcn), dim3(kWg), 0, st, w, (const double*)cam, (const double*)X,
                       (const double*)theta);
    launch_linearize(w, loss, true, st);
    hipLaunchKernelGGL(kc_gate, dim3(1), dim3(1), 0, st, w);
    rc = check_launch("ba_calib linearize");
    if (rc == SFMHIP_OK) rc = read_ctl(who, w, &h, st);
    if (rc != SFMHIP_OK || h.bad || h.depth_bad) {
        if (rc == SFMHIP_OK) info[0] = h.bad ? -1 : -2;
        scratch_free(scratch, st);
        return rc;
    }
    cost[0] = h.cost;
    int nit = 1, status = 0;
    while (!h.done) {
        // one trial, the schedule of ba_global.hip with the group pass after every by-camera pass
        hipLaunchKernelGGL(kc_damp, dim3(gcn), dim3(kWg), 0, st, w, 0.0, true);
        launch_passes(w, kRhs, w.x, false, st);
        hipLaunchKernelGGL(kc_cg_init, dim3(1), dim3(kWg), 0, st, w);
        for (int it = 0; it < max_cg; ++it) {
            launch_passes(w, kMatvec, w.p, true, st);
            hipLaunchKernelGGL(kc_cg_step, dim3(1), dim3(kWg), 0, st, w);
        }
        hipLaunchKernelGGL(kc_point_pass, dim3(grid_of(N)), dim3(kWg), 0, st, w, (int)kBacksub, (const double*)w.x,
                           false);
        hipLaunchKernelGGL(kc_trial, dim3(gcn), dim3(kWg), 0, st, w);
        launch_residuals<false>(w, loss, w.Rt, w.tt, w.Xt, w.tht, true, st);
        hipLaunchKernelGGL(kc_cost_final, dim3(1), dim3(kWg), 0, st, w, true);
        hipLaunchKernelGGL(kc_step, dim3(1), dim3(1), 0, st, w);
        hipLaunchKernelGGL(kc_accept, dim3(gcn), dim3(kWg), 0, st, w);
        rc = check_launch("ba_calib trial");
        if (rc == SFMHIP_OK) rc = read_ctl(who, w, &h, st);
        if (rc != SFMHIP_OK) break;
        if (h.done || !h.accepted) continue;
        if (nit == max_iter) break;          // status 0
        launch_linearize(w, loss, true, st);
        hipLaunchKernelGGL(kc_gate, dim3(1), dim3(1), 0, st, w);
        ++nit;
    }
    if (rc == SFMHIP_OK) {
        status = h.done ? h.status : 0;
        hipLaunchKernelGGL(kc_finish, dim3(gcn), dim3(kWg), 0, st, w, cam, X, theta);
        if (obs_res2 != nullptr && M > 0)
            hipLaunchKernelGGL(kc_obs_res2, dim3(w.nb), dim3(kWg), 0, st, w, (const double*)w.R, (const double*)w.t,
                               (const double*)w.X, (const double*)w.th, obs_res2);
        rc = check_launch("ba_calib finish");
        if (rc == SFMHIP_OK && hipStreamSynchronize(st) != hipSuccess) {
            set_error("%s: %s", who, hipGetErrorString(hipGetLastError()));
            rc = SFMHIP_E_HIP;
        }
    }
    if (rc == SFMHIP_OK) {
        cost[1] = h.cost;
        info[0] = status; info[1] = nit; info[2] = h.n_accept; info[3] = h.cg_total;
    }
    scratch_free(scratch, st);
    return rc;
}
