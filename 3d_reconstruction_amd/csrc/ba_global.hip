// ba_global.hip — K3''': global bundle adjustment over all cameras and points.
// Levenberg-Marquardt with Marquardt scaling; the reduced camera system (implicit Schur
// complement) is solved matrix-free by block-Jacobi preconditioned conjugate gradients
// (DESIGN.md K3''', tests/ba_global_ref.py restates every step in numpy).
//
// Observations are held sorted by (point, camera) with CSR offsets by point (pt_off) and a
// permutation + CSR offsets by camera (cam_perm, cam_off).  Every sum has a fixed order that
// depends only on that structure, and there is no floating-point atomic:
//   * per point: one lane walks the point's segment in sequence;
//   * per camera: the camera's observations in cam_perm order, cut into chunks of kChunk; one
//     workgroup per chunk sums through a pairwise LDS tree, a second stage adds the chunks of a
//     camera in sequence;
//   * vectors of the CG iteration and the cost: lane l of one 256-lane workgroup sums elements
//     l, l + 256, ... in sequence, then the same tree.
// The host enqueues one LM trial (damping, right-hand side, max_cg CG iterations, back
// substitution, trial cost, step control) and reads one control record back; kernels return at
// once when the record says `done` / `cg_done`.
// A robust loss (huber, soft_l1, cauchy; tests/ba_robust_ref.py) lives in k_linearize alone: plain
// IRLS, the stored r, Jc, Jp carry sqrt(w) and the cost sums f^2 rho, nothing downstream changes.
#include "common.h"
#include "geom_dev.h"
#include "ba_dev.h"                    // constants, tree sum, LDL inverse, losses, rodrigues_inverse, Arena
#include <climits>
#include <cmath>
#include <algorithm>

namespace sfmhip {
namespace {

struct Ctl {
    double lambda, cost, cost_trial, rel, rz, bb, gtol, ftol, eta;
    unsigned long long gmax_bits;      // max |g| over free cameras and points, as the bits of a double
    int bad;                           // structure / index error found by k_validate
    int depth_flag;                    // raised by the running linearisation / cost pass
    int depth_bad;                     // the last finished pass saw a non-positive depth
    int done, status, cg_done, cg_iters, cg_total, accepted, n_accept;
};

struct Ws {                            // device pointers of one solve
    Ctl* ctl;
    const double* K;
    const int32_t *oc, *op;
    const double* uv;
    const int64_t *pt_off, *cam_perm, *cam_off;
    const uint8_t* fixed;              // nullable: no camera fixed
    int C, N;
    int64_t M;
    int nb, tmax;                      // cost blocks, upper bound of the camera chunks
    int *chunk_base, *chunk_cam;
    double *R, *t, *X, *Rt, *tt, *Xt;  // accepted and trial state
    double *r, *Jc, *Jp, *cpart;
    double *U, *gc, *V, *gp, *Us, *Ui, *Vi;
    double *part27, *part6, *y;
    double *b, *x, *rr, *z, *p, *q;    // CG vectors (6C each)
    double f2;                         // robust loss: f_scale^2
    double* wout;                      // nullable: the IRLS weight per sorted observation
};

// ---------------------------------------------------------------------------
// Structure check: every read below is guarded by the checks before it.
__global__ __launch_bounds__(kWg) void k_validate(const int32_t* oc, const int32_t* op, const int64_t* pt_off,
                                                  const int64_t* cam_perm, const int64_t* cam_off, int C, int N,
                                                  int64_t M, Ctl* ctl) {
    const int64_t i = (int64_t)blockIdx.x * kWg + threadIdx.x;
    if (structure_bad(i, oc, op, pt_off, cam_perm, cam_off, C, N, M)) atomicOr(&ctl->bad, 1);
}

// chunk_base[c] = first chunk of camera c (chunk_base[C] = number of chunks), chunk_cam = the
// owner of every chunk.  Once per call; one lane walks the C cameras and writes the M / kChunk + C
// entries in sequence: ~9 k steps for the 0.77 M observations of the timing scene, and at most
// 2^20 + 2^23 at the sizes common_args_ok admits (C <= 2^20, M < 2^31), tens of milliseconds once
// per call; a problem near those limits wants a scan here.
__global__ void k_chunks(Ws w) {
    if (w.ctl->bad) return;
    chunk_numbering(w);
}

__global__ __launch_bounds__(kWg) void k_init(Ws w, const double* cam, const double* X) {
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.C) {
        rodrigues(cam + 6 * i, w.R + 9 * i);
        for (int k = 0; k < 3; ++k) w.t[3 * i + k] = cam[6 * i + 3 + k];
    }
    if (i < w.N)
        for (int k = 0; k < 3; ++k) w.X[3 * i + k] = X[3 * i + k];
}

// Residual, Jacobians (JAC) and the workgroup's partial cost, one lane per sorted observation.
// LOSS = kLinear: r, Jc, Jp and |r|^2 as they are.  A robust LOSS (plain IRLS): with z = |r|^2 / f^2
// and w = rho'(z) the stored arrays are sqrt(w) r, sqrt(w) Jc, sqrt(w) Jp and the cost term is
// f^2 rho(z), so everything downstream reads the robust Gauss-Newton quantities unchanged.
template <bool JAC, int LOSS>
__global__ __launch_bounds__(kWg) void k_linearize(Ws w, const double* Rs, const double* ts, const double* Xs,
                                                   bool trial) {
    if (w.ctl->bad || (trial && w.ctl->done)) return;
    __shared__ double sm[kWg];
    const int64_t m = (int64_t)blockIdx.x * kWg + threadIdx.x;
    double sq = 0.0;
    if (m < w.M) {
        const int c = w.oc[m], p = w.op[m];
        const double* R = Rs + 9 * (int64_t)c;
        const double* t = ts + 3 * (int64_t)c;
        const double* X = Xs + 3 * (int64_t)p;
        const double* K = w.K + 9 * (int64_t)c;
        const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
        const double px = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2];
        const double py = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2];
        const double pz = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
        const double x = px + t[0], y = py + t[1], z = pz + t[2];
        if (!(z > 0.0)) atomicOr(&w.ctl->depth_flag, 1);
        const double iz = 1.0 / z;
        const double xn = x * iz, yn = y * iz;
        const double r0 = (xn * fx + cx) - w.uv[2 * m], r1 = (yn * fy + cy) - w.uv[2 * m + 1];
        sq = r0 * r0 + r1 * r1;
        double sw = 1.0;                   // sqrt(w); not read when LOSS == kLinear
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
            const double a = fx * iz, b = fy * iz;
            const double d02 = -(a * xn), d12 = -(b * yn);
            double* Jp = w.Jp + 6 * m;
            double* Jc = w.Jc + 12 * m;
            double jp[6], jc[12];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                jp[j] = a * R[j] + d02 * R[6 + j];
                jp[3 + j] = b * R[3 + j] + d12 * R[6 + j];
            }
            jc[0] = d02 * py;
            jc[1] = a * pz - d02 * px;
            jc[2] = -(a * py);
            jc[3] = a;
            jc[4] = 0.0;
            jc[5] = d02;
            jc[6] = -(b * pz) + d12 * py;
            jc[7] = -(d12 * px);
            jc[8] = b * px;
            jc[9] = 0.0;
            jc[10] = b;
            jc[11] = d12;
            if (LOSS == kLinear) {
                w.r[2 * m] = r0;
                w.r[2 * m + 1] = r1;
#pragma unroll
                for (int j = 0; j < 6; ++j) Jp[j] = jp[j];
#pragma unroll
                for (int j = 0; j < 12; ++j) Jc[j] = jc[j];
            } else {
                w.r[2 * m] = sw * r0;
                w.r[2 * m + 1] = sw * r1;
#pragma unroll
                for (int j = 0; j < 6; ++j) Jp[j] = sw * jp[j];
#pragma unroll
                for (int j = 0; j < 12; ++j) Jc[j] = sw * jc[j];
            }
        }
    }
    const double s = block_sum(sq, sm);
    if (threadIdx.x == 0) w.cpart[blockIdx.x] = s;
}

// The unweighted |r|^2 of every sorted observation at (Rs, ts, Xs): k_linearize's residual, once
// after the solve.
__global__ __launch_bounds__(kWg) void k_obs_res2(Ws w, const double* Rs, const double* ts, const double* Xs,
                                                  double* res2) {
    if (w.ctl->bad) return;
    const int64_t m = (int64_t)blockIdx.x * kWg + threadIdx.x;
    if (m >= w.M) return;
    const int c = w.oc[m], p = w.op[m];
    const double* R = Rs + 9 * (int64_t)c;
    const double* t = ts + 3 * (int64_t)c;
    const double* X = Xs + 3 * (int64_t)p;
    const double* K = w.K + 9 * (int64_t)c;
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double px = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2];
    const double py = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2];
    const double pz = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
    const double x = px + t[0], y = py + t[1], z = pz + t[2];
    const double iz = 1.0 / z;
    const double xn = x * iz, yn = y * iz;
    const double r0 = (xn * fx + cx) - w.uv[2 * m], r1 = (yn * fy + cy) - w.uv[2 * m + 1];
    res2[m] = r0 * r0 + r1 * r1;
}

__global__ __launch_bounds__(kWg) void k_fill(double* out, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * kWg + threadIdx.x;
    if (i < n) out[i] = v;
}

// cost = 0.5 sum of the partial costs (infinite after a non-positive depth); one workgroup.
__global__ __launch_bounds__(kWg) void k_cost_final(Ws w, bool trial) {
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

__device__ __forceinline__ void gmax_update(Ctl* ctl, double g) {
    atomicMax(&ctl->gmax_bits, (unsigned long long)__double_as_longlong(fabs(g)));
}

// V = sum Jp^T Jp, g_p = sum Jp^T r over the point's segment, in sequence; one lane per point.
__global__ __launch_bounds__(kWg) void k_point_blocks(Ws w, bool solver) {
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

// Stage 1 (ba_dev.h chunk_reduce: one workgroup per camera chunk through the tree) of U = sum Jc^T Jc (upper triangle, 21) and g_c = sum Jc^T r (6).
__global__ __launch_bounds__(kWg) void k_cam_partial(Ws w) {
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

// Stage 2: the chunks of a camera in sequence; one lane per camera.
__global__ __launch_bounds__(kWg) void k_cam_blocks(Ws w, bool solver) {
    if (w.ctl->bad) return;
    const int c = blockIdx.x * kWg + threadIdx.x;
    if (c >= w.C) return;
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int b = w.chunk_base[c]; b < w.chunk_base[c + 1]; ++b)
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

// Convergence gate at a fresh linearisation: gtol on the gradient, ftol on the last accepted step.
__global__ void k_gate(Ws w) {
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

// V*^-1 per point, U* and U*^-1 per camera (zero for a fixed camera) at lambda.
__global__ __launch_bounds__(kWg) void k_damp(Ws w, double lam_arg, bool from_ctl) {
    if (w.ctl->bad || w.ctl->done) return;
    const double lam = from_ctl ? w.ctl->lambda : lam_arg;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.N) damp_invert<3>(w.V + 9 * (int64_t)i, lam, nullptr, w.Vi + 9 * (int64_t)i);
    if (i < w.C) {
        damp_invert<6>(w.U + 36 * (int64_t)i, lam, w.Us + 36 * (int64_t)i, w.Ui + 36 * (int64_t)i);
        if (is_fixed(w.fixed, i))
            for (int k = 0; k < 36; ++k) w.Ui[36 * (int64_t)i + k] = 0.0;
    }
}

// By point: s = sum Jp^T (Jc x_c) in sequence; y = V*^-1 s (kMatvec), V*^-1 g_p (kRhs),
// -V*^-1 (g_p + s) (kBacksub).  One lane per point.
__global__ __launch_bounds__(kWg) void k_point_pass(Ws w, int mode, const double* x, bool cg) {
    if (w.ctl->bad || w.ctl->done || (cg && w.ctl->cg_done)) return;
    const int p = blockIdx.x * kWg + threadIdx.x;
    if (p >= w.N) return;
    double s[3] = {0.0, 0.0, 0.0};
    if (mode != kRhs) {
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

// By camera, stage 1: Jc^T (Jp y_p) per observation through the chunk tree.
__global__ __launch_bounds__(kWg) void k_cam_pass(Ws w, bool cg) {
    if (w.ctl->bad || w.ctl->done || (cg && w.ctl->cg_done)) return;
    chunk_reduce<6>(w, w.part6, [&](int64_t m, double* v) {
        const double* Jp = w.Jp + 6 * m;
        const double* y = w.y + 3 * (int64_t)w.op[m];
        const double w0 = (Jp[0] * y[0] + Jp[1] * y[1]) + Jp[2] * y[2];
        const double w1 = (Jp[3] * y[0] + Jp[4] * y[1]) + Jp[5] * y[2];
        const double* J = w.Jc + 12 * m;
#pragma unroll
        for (int a = 0; a < 6; ++a) v[a] = J[a] * w0 + J[6 + a] * w1;
    });
}

__device__ __forceinline__ double cam_chunks_sum(const Ws& w, int c, int a) {
    double o = 0.0;
    for (int b = w.chunk_base[c]; b < w.chunk_base[c + 1]; ++b) o = o + w.part6[(int64_t)b * 6 + a];
    return o;
}

__device__ __forceinline__ double block_row(const double* A, const double* v, int c, int a) {
    const double* row = A + 36 * (int64_t)c + 6 * a;
    const double* vc = v + 6 * (int64_t)c;
    double acc = row[0] * vc[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) acc = acc + row[j] * vc[j];
    return acc;
}

// out = U* x - W V*^-1 W^T x from the stage-1 partials (rows of fixed cameras exactly 0).
__global__ __launch_bounds__(kWg) void k_matvec_out(Ws w, const double* x, double* out) {
    if (w.ctl->bad) return;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i >= 6 * w.C) return;
    const int c = i / 6, a = i % 6;
    out[i] = is_fixed(w.fixed, c) ? 0.0 : block_row(w.Us, x, c, a) - cam_chunks_sum(w, c, a);
}

// b = -(g_c - W V*^-1 g_p), x = 0, r = b, z = M^-1 r, p = z; one workgroup.
__global__ __launch_bounds__(kWg) void k_cg_init(Ws w) {
    Ctl* ctl = w.ctl;
    if (ctl->bad || ctl->done) return;
    __shared__ double sm[kWg];
    const int n6 = 6 * w.C, tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n6; i += kWg) {
        const int c = i / 6, a = i % 6;
        const double b = is_fixed(w.fixed, c) ? 0.0 : -(w.gc[i] - cam_chunks_sum(w, c, a));
        w.b[i] = b;
        w.x[i] = 0.0;
        w.rr[i] = b;
        acc = acc + b * b;
    }
    const double bb = block_sum(acc, sm);   // also makes rr visible to the workgroup
    acc = 0.0;
    for (int i = tid; i < n6; i += kWg) {
        const double z = block_row(w.Ui, w.rr, i / 6, i % 6);
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

// One PCG iteration: q = S p from the stage-1 partials, the three dot products, x, r, z, p.
__global__ __launch_bounds__(kWg) void k_cg_step(Ws w) {
    Ctl* ctl = w.ctl;
    if (ctl->bad || ctl->done || ctl->cg_done) return;
    __shared__ double sm[kWg];
    const int n6 = 6 * w.C, tid = threadIdx.x;
    const double rz = ctl->rz, bb = ctl->bb, eta = ctl->eta;
    const int iters = ctl->cg_iters + 1;
    double acc = 0.0;
    for (int i = tid; i < n6; i += kWg) {
        const int c = i / 6, a = i % 6;
        const double q = is_fixed(w.fixed, c) ? 0.0 : block_row(w.Us, w.p, c, a) - cam_chunks_sum(w, c, a);
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
    for (int i = tid; i < n6; i += kWg) {
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
    for (int i = tid; i < n6; i += kWg) {
        const double z = block_row(w.Ui, w.rr, i / 6, i % 6);
        w.z[i] = z;
        acc = acc + w.rr[i] * z;
    }
    const double rzn = block_sum(acc, sm);
    const double beta = rzn / rz;
    for (int i = tid; i < n6; i += kWg) w.p[i] = w.z[i] + beta * w.p[i];
    if (tid == 0) {
        ctl->rz = rzn;
        ctl->cg_iters = iters;
    }
}

// Trial state: R <- exp(dw) R, t <- t + dt for free cameras, X <- X + dX (dX in y).
__global__ __launch_bounds__(kWg) void k_trial(Ws w) {
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
}

// Step control: accept iff the cost decreased.
__global__ void k_step(Ws w) {
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

__global__ __launch_bounds__(kWg) void k_accept(Ws w) {
    if (w.ctl->bad || w.ctl->done || !w.ctl->accepted) return;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.C) {
        for (int k = 0; k < 9; ++k) w.R[9 * (int64_t)i + k] = w.Rt[9 * (int64_t)i + k];
        for (int k = 0; k < 3; ++k) w.t[3 * (int64_t)i + k] = w.tt[3 * (int64_t)i + k];
    }
    if (i < w.N)
        for (int k = 0; k < 3; ++k) w.X[3 * (int64_t)i + k] = w.Xt[3 * (int64_t)i + k];
}

// Write the accepted state back: free cameras that have observations, and every point.
__global__ __launch_bounds__(kWg) void k_finish(Ws w, double* cam, double* X) {
    if (w.ctl->bad || w.ctl->n_accept == 0) return;
    const int i = blockIdx.x * kWg + threadIdx.x;
    if (i < w.C && !is_fixed(w.fixed, i) && w.cam_off[i + 1] > w.cam_off[i]) {
        rodrigues_inverse(w.R + 9 * (int64_t)i, cam + 6 * (int64_t)i);
        for (int k = 0; k < 3; ++k) cam[6 * (int64_t)i + 3 + k] = w.t[3 * (int64_t)i + k];
    }
    if (i < w.N)
        for (int k = 0; k < 3; ++k) X[3 * (int64_t)i + k] = w.X[3 * (int64_t)i + k];
}

// ---------------------------------------------------------------------------
// Host side: one scratch allocation (ba_dev.h Arena) carved into the arrays a call needs.
// Carve (base == nullptr: size only).  solver: the state, trial and CG arrays as well;
// own_lin: r / Jc / Jp / blocks live in the scratch (the solver) or are the caller's.
void carve(Arena& a, Ws& w, bool solver, bool own_lin, bool own_damp) {
    const size_t C = (size_t)w.C, N = (size_t)w.N, M = (size_t)w.M;
    w.ctl = a.take<Ctl>(1);
    w.chunk_base = a.take<int>(C + 1);
    w.chunk_cam = a.take<int>((size_t)w.tmax);
    w.cpart = a.take<double>((size_t)w.nb);
    w.part27 = a.take<double>((size_t)w.tmax * 27);
    w.part6 = a.take<double>((size_t)w.tmax * 6);
    w.R = a.take<double>(9 * C);
    w.t = a.take<double>(3 * C);
    w.X = a.take<double>(3 * N);
    if (own_lin) {
        w.r = a.take<double>(2 * M);
        w.Jc = a.take<double>(12 * M);
        w.Jp = a.take<double>(6 * M);
        w.U = a.take<double>(36 * C);
        w.gc = a.take<double>(6 * C);
        w.V = a.take<double>(9 * N);
        w.gp = a.take<double>(3 * N);
    }
    if (own_damp) {
        w.Us = a.take<double>(36 * C);
        w.Ui = a.take<double>(36 * C);
        w.Vi = a.take<double>(9 * N);
        w.y = a.take<double>(3 * N);
    }
    if (solver) {
        w.Rt = a.take<double>(9 * C);
        w.tt = a.take<double>(3 * C);
        w.Xt = a.take<double>(3 * N);
        w.b = a.take<double>(6 * C);
        w.x = a.take<double>(6 * C);
        w.rr = a.take<double>(6 * C);
        w.z = a.take<double>(6 * C);
        w.p = a.take<double>(6 * C);
        w.q = a.take<double>(6 * C);
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
    const int64_t n = std::max<int64_t>(w.M, std::max(w.C, w.N) + 1);
    hipLaunchKernelGGL(k_validate, dim3(grid_of(n)), dim3(kWg), 0, st, w.oc, w.op, w.pt_off, w.cam_perm, w.cam_off,
                       w.C, w.N, w.M, w.ctl);
    hipLaunchKernelGGL(k_chunks, dim3(1), dim3(1), 0, st, w);
}

// k_linearize<JAC, loss>; the linear loss is its own instantiation with today's operations only.
template <bool JAC>
void launch_residuals(const Ws& w, int loss, const double* R, const double* t, const double* X, bool trial,
                      hipStream_t st) {
    switch (loss) {
    case kHuber: hipLaunchKernelGGL((k_linearize<JAC, kHuber>), dim3(w.nb), dim3(kWg), 0, st, w, R, t, X, trial); break;
    case kSoftL1: hipLaunchKernelGGL((k_linearize<JAC, kSoftL1>), dim3(w.nb), dim3(kWg), 0, st, w, R, t, X, trial); break;
    case kCauchy: hipLaunchKernelGGL((k_linearize<JAC, kCauchy>), dim3(w.nb), dim3(kWg), 0, st, w, R, t, X, trial); break;
    default: hipLaunchKernelGGL((k_linearize<JAC, kLinear>), dim3(w.nb), dim3(kWg), 0, st, w, R, t, X, trial); break;
    }
}

// Linearise at (R, t, X) of the workspace: r, Jc, Jp, the cost and the blocks.
void launch_linearize(const Ws& w, int loss, bool solver, hipStream_t st) {
    launch_residuals<true>(w, loss, w.R, w.t, w.X, false, st);
    hipLaunchKernelGGL(k_cost_final, dim3(1), dim3(kWg), 0, st, w, false);
    hipLaunchKernelGGL(k_point_blocks, dim3(grid_of(w.N)), dim3(kWg), 0, st, w, solver);
    hipLaunchKernelGGL(k_cam_partial, dim3(w.tmax), dim3(kWg), 0, st, w);
    hipLaunchKernelGGL(k_cam_blocks, dim3(grid_of(w.C)), dim3(kWg), 0, st, w, solver);
}

bool common_args_ok(const char* who, const void* oc, const void* op, const void* pt_off, const void* cam_perm,
                    const void* cam_off, int C, int N, int64_t M) {
    if (C < 0 || N < 0 || M < 0) {
        set_error("%s: negative size", who);
        return false;
    }
    if (M > INT32_MAX || C > (1 << 20) || N > INT32_MAX / 16) {
        set_error("%s: size out of range", who);
        return false;
    }
    if (!pt_off || !cam_off || (M > 0 && (!oc || !op || !cam_perm))) {
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

int linearize_impl(const char* who, const double* cam, const double* K, const double* X, const int32_t* obs_cam,
                   const int32_t* obs_pt, const double* pts2d, const int64_t* pt_off, const int64_t* cam_perm,
                   const int64_t* cam_off, int C, int N, int64_t M, double* r, double* Jc, double* Jp, double* U,
                   double* g_c, double* V, double* g_p, double* cost, int loss, double f_scale, double* weight,
                   void* stream) {
    if (!loss_args_ok(who, loss, f_scale)) return SFMHIP_E_ARG;
    if (!common_args_ok(who, obs_cam, obs_pt, pt_off, cam_perm, cam_off, C, N, M)) return SFMHIP_E_ARG;
    SFMHIP_REQUIRE(cost && (C == 0 || (cam && K && U && g_c)) && (N == 0 || (X && V && g_p)) &&
                       (M == 0 || (pts2d && r && Jc && Jp)), "%s: null pointer", who);
    hipStream_t st = as_stream(stream);
    Ws w = {};
    w.K = K; w.oc = obs_cam; w.op = obs_pt; w.uv = pts2d; w.pt_off = pt_off; w.cam_perm = cam_perm; w.cam_off = cam_off;
    w.C = C; w.N = N; w.M = M;
    w.r = r; w.Jc = Jc; w.Jp = Jp; w.U = U; w.gc = g_c; w.V = V; w.gp = g_p;
    w.f2 = f_scale * f_scale; w.wout = weight;
    void* scratch = nullptr;
    int rc = alloc_ws(who, w, false, false, false, st, &scratch);
    if (rc != SFMHIP_OK) return rc;
    launch_validate(w, st);
    Ctl h;
    rc = read_ctl(who, w, &h, st);    // nothing is written before the structure is known to be sound
    if (rc == SFMHIP_OK && h.bad) {
        set_error("%s: index out of range, offsets not monotone or orders inconsistent", who);
        rc = SFMHIP_E_ARG;
    }
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(k_init, dim3(grid_of(std::max(C, N))), dim3(kWg), 0, st, w, cam, X);
        launch_linearize(w, loss, false, st);
        if (loss == kLinear && weight != nullptr && M > 0)
            hipLaunchKernelGGL(k_fill, dim3(grid_of(M)), dim3(kWg), 0, st, weight, M, 1.0);
        rc = check_launch("ba_global linearize");
        if (rc == SFMHIP_OK) rc = read_ctl(who, w, &h, st);
        if (rc == SFMHIP_OK) *cost = h.cost;
    }
    scratch_free(scratch, st);
    return rc;
}

}  // namespace
}  // namespace sfmhip

using namespace sfmhip;

extern "C" int sfmhip_ba_global_linearize(const double* cam, const double* K, const double* X, const int32_t* obs_cam,
                                          const int32_t* obs_pt, const double* pts2d, const int64_t* pt_off,
                                          const int64_t* cam_perm, const int64_t* cam_off, int C, int N, int64_t M,
                                          double* r, double* Jc, double* Jp, double* U, double* g_c, double* V,
                                          double* g_p, double* cost, void* stream) {
    return linearize_impl("sfmhip_ba_global_linearize", cam, K, X, obs_cam, obs_pt, pts2d, pt_off, cam_perm, cam_off, C,
                          N, M, r, Jc, Jp, U, g_c, V, g_p, cost, kLinear, 1.0, nullptr, stream);
}

extern "C" int sfmhip_ba_global_linearize_robust(const double* cam, const double* K, const double* X,
                                                 const int32_t* obs_cam, const int32_t* obs_pt, const double* pts2d,
                                                 const int64_t* pt_off, const int64_t* cam_perm,
                                                 const int64_t* cam_off, int C, int N, int64_t M, double* r, double* Jc,
                                                 double* Jp, double* U, double* g_c, double* V, double* g_p,
                                                 double* cost, void* stream, int loss, double f_scale, double* weight) {
    const char* who = "sfmhip_ba_global_linearize_robust";
    if (!loss_args_ok(who, loss, f_scale)) return SFMHIP_E_ARG;
    SFMHIP_REQUIRE(M <= 0 || weight, "%s: null pointer", who);
    return linearize_impl(who, cam, K, X, obs_cam, obs_pt, pts2d, pt_off, cam_perm, cam_off, C, N, M, r, Jc, Jp, U, g_c,
                          V, g_p, cost, loss, f_scale, weight, stream);
}

extern "C" int sfmhip_ba_global_schur_matvec(const double* Jc, const double* Jp, const double* U, const double* V,
                                             const int32_t* obs_cam, const int32_t* obs_pt, const int64_t* pt_off,
                                             const int64_t* cam_perm, const int64_t* cam_off,
                                             const uint8_t* cam_fixed, int C, int N, int64_t M, double lambda,
                                             const double* x, double* out, void* stream) {
    const char* who = "sfmhip_ba_global_schur_matvec";
    if (!common_args_ok(who, obs_cam, obs_pt, pt_off, cam_perm, cam_off, C, N, M)) return SFMHIP_E_ARG;
    SFMHIP_REQUIRE((C == 0 || (U && x && out)) && (N == 0 || V) && (M == 0 || (Jc && Jp)), "%s: null pointer", who);
    SFMHIP_REQUIRE(lambda >= 0.0, "%s: lambda must be non-negative", who);
    hipStream_t st = as_stream(stream);
    Ws w = {};
    w.oc = obs_cam; w.op = obs_pt; w.pt_off = pt_off; w.cam_perm = cam_perm; w.cam_off = cam_off; w.fixed = cam_fixed;
    w.C = C; w.N = N; w.M = M;
    w.Jc = const_cast<double*>(Jc); w.Jp = const_cast<double*>(Jp);
    w.U = const_cast<double*>(U); w.V = const_cast<double*>(V);
    void* scratch = nullptr;
    int rc = alloc_ws(who, w, false, false, true, st, &scratch);
    if (rc != SFMHIP_OK) return rc;
    launch_validate(w, st);
    Ctl h;
    rc = read_ctl(who, w, &h, st);
    if (rc == SFMHIP_OK && h.bad) {
        set_error("%s: index out of range, offsets not monotone or orders inconsistent", who);
        rc = SFMHIP_E_ARG;
    }
    if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(k_damp, dim3(grid_of(std::max(C, N))), dim3(kWg), 0, st, w, lambda, false);
        hipLaunchKernelGGL(k_point_pass, dim3(grid_of(N)), dim3(kWg), 0, st, w, (int)kMatvec, x, false);
        hipLaunchKernelGGL(k_cam_pass, dim3(w.tmax), dim3(kWg), 0, st, w, false);
        hipLaunchKernelGGL(k_matvec_out, dim3(grid_of(6 * (int64_t)C)), dim3(kWg), 0, st, w, x, out);
        rc = check_launch("ba_global schur_matvec");
    }
    scratch_free(scratch, st);
    return rc;
}

namespace sfmhip {
namespace {

int solve_impl(const char* who, double* cam, const double* K, double* X, const int32_t* obs_cam, const int32_t* obs_pt,
               const double* pts2d, const int64_t* pt_off, const int64_t* cam_perm, const int64_t* cam_off,
               const uint8_t* cam_fixed, int C, int N, int64_t M, double gtol, double ftol, double eta, int max_iter,
               int max_cg, double* cost, int32_t* info, int loss, double f_scale, double* obs_res2, void* stream) {
    if (!loss_args_ok(who, loss, f_scale)) return SFMHIP_E_ARG;
    if (!common_args_ok(who, obs_cam, obs_pt, pt_off, cam_perm, cam_off, C, N, M)) return SFMHIP_E_ARG;
    SFMHIP_REQUIRE(cost && info && (C == 0 || (cam && K)) && (N == 0 || X) && (M == 0 || pts2d), "%s: null pointer",
                   who);
    SFMHIP_REQUIRE(max_iter >= 1 && max_cg >= 0 && max_cg <= 4096, "%s: max_iter >= 1 and 0 <= max_cg <= 4096", who);
    SFMHIP_REQUIRE(gtol >= 0.0 && ftol >= 0.0 && eta >= 0.0, "%s: negative tolerance", who);
    hipStream_t st = as_stream(stream);
    Ws w = {};
    w.K = K; w.oc = obs_cam; w.op = obs_pt; w.uv = pts2d; w.pt_off = pt_off; w.cam_perm = cam_perm; w.cam_off = cam_off;
    w.fixed = cam_fixed; w.C = C; w.N = N; w.M = M;
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
    const int gcn = grid_of(std::max(C, N));
    launch_validate(w, st);
    hipLaunchKernelGGL(k_init, dim3(gcn), dim3(kWg), 0, st, w, (const double*)cam, (const double*)X);
    launch_linearize(w, loss, true, st);
    hipLaunchKernelGGL(k_gate, dim3(1), dim3(1), 0, st, w);
    rc = check_launch("ba_global linearize");
    if (rc == SFMHIP_OK) rc = read_ctl(who, w, &h, st);
    if (rc != SFMHIP_OK || h.bad || h.depth_bad) {
        if (rc == SFMHIP_OK) info[0] = h.bad ? -1 : -2;
        scratch_free(scratch, st);
        return rc;
    }
    cost[0] = h.cost;
    int nit = 1, status = 0;
    while (!h.done) {
        // one trial: damp, right-hand side, CG batch (fixed launch count), back-substitution, trial cost, step control
        hipLaunchKernelGGL(k_damp, dim3(gcn), dim3(kWg), 0, st, w, 0.0, true);
        hipLaunchKernelGGL(k_point_pass, dim3(grid_of(N)), dim3(kWg), 0, st, w, (int)kRhs, (const double*)w.x, false);
        hipLaunchKernelGGL(k_cam_pass, dim3(w.tmax), dim3(kWg), 0, st, w, false);
        hipLaunchKernelGGL(k_cg_init, dim3(1), dim3(kWg), 0, st, w);
        for (int it = 0; it < max_cg; ++it) {
            hipLaunchKernelGGL(k_point_pass, dim3(grid_of(N)), dim3(kWg), 0, st, w, (int)kMatvec, (const double*)w.p,
                               true);
            hipLaunchKernelGGL(k_cam_pass, dim3(w.tmax), dim3(kWg), 0, st, w, true);
            hipLaunchKernelGGL(k_cg_step, dim3(1), dim3(kWg), 0, st, w);
        }
        hipLaunchKernelGGL(k_point_pass, dim3(grid_of(N)), dim3(kWg), 0, st, w, (int)kBacksub, (const double*)w.x,
                           false);
        hipLaunchKernelGGL(k_trial, dim3(gcn), dim3(kWg), 0, st, w);
        launch_residuals<false>(w, loss, w.Rt, w.tt, w.Xt, true, st);
        hipLaunchKernelGGL(k_cost_final, dim3(1), dim3(kWg), 0, st, w, true);
        hipLaunchKernelGGL(k_step, dim3(1), dim3(1), 0, st, w);
        hipLaunchKernelGGL(k_accept, dim3(gcn), dim3(kWg), 0, st, w);
        rc = check_launch("ba_global trial");
        if (rc == SFMHIP_OK) rc = read_ctl(who, w, &h, st);
        if (rc != SFMHIP_OK) break;
        if (h.done || !h.accepted) continue;
        if (nit == max_iter) break;          // status 0
        // the next linearisation goes in front of the next trial's batch: when the gate ends the
        // solve there, that batch returns at once and the record read after it says so
        launch_linearize(w, loss, true, st);
        hipLaunchKernelGGL(k_gate, dim3(1), dim3(1), 0, st, w);
        ++nit;
    }
    if (rc == SFMHIP_OK) {
        status = h.done ? h.status : 0;
        hipLaunchKernelGGL(k_finish, dim3(gcn), dim3(kWg), 0, st, w, cam, X);
        if (obs_res2 != nullptr && M > 0)   // the final unweighted |r|^2, at the accepted state
            hipLaunchKernelGGL(k_obs_res2, dim3(w.nb), dim3(kWg), 0, st, w, (const double*)w.R, (const double*)w.t,
                               (const double*)w.X, obs_res2);
        rc = check_launch("ba_global finish");
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

}  // namespace
}  // namespace sfmhip

extern "C" int sfmhip_ba_global(double* cam, const double* K, double* X, const int32_t* obs_cam, const int32_t* obs_pt,
                                const double* pts2d, const int64_t* pt_off, const int64_t* cam_perm,
                                const int64_t* cam_off, const uint8_t* cam_fixed, int C, int N, int64_t M, double gtol,
                                double ftol, double eta, int max_iter, int max_cg, double* cost, int32_t* info,
                                void* stream) {
    return solve_impl("sfmhip_ba_global", cam, K, X, obs_cam, obs_pt, pts2d, pt_off, cam_perm, cam_off, cam_fixed, C, N,
                      M, gtol, ftol, eta, max_iter, max_cg, cost, info, kLinear, 1.0, nullptr, stream);
}

extern "C" int sfmhip_ba_global_robust(double* cam, const double* K, double* X, const int32_t* obs_cam,
                                       const int32_t* obs_pt, const double* pts2d, const int64_t* pt_off,
                                       const int64_t* cam_perm, const int64_t* cam_off, const uint8_t* cam_fixed, int C,
                                       int N, int64_t M, double gtol, double ftol, double eta, int max_iter, int max_cg,
                                       double* cost, int32_t* info, void* stream, int loss, double f_scale,
                                       double* obs_res2) {
    return solve_impl("sfmhip_ba_global_robust", cam, K, X, obs_cam, obs_pt, pts2d, pt_off, cam_perm, cam_off, cam_fixed,
                      C, N, M, gtol, ftol, eta, max_iter, max_cg, cost, info, loss, f_scale, obs_res2, stream);
}
