"""numpy restatement of the global bundle adjustment with shared intrinsics and radial
distortion as unknowns (ba_calib.hip, DESIGN.md "K3‴ with intrinsics"), built on
tests/ba_global_ref.py and tests/ba_robust_ref.py, which it imports and does not change.
Dtype-generic like them: ``dt=np.float64`` is the kernels' arithmetic, ``dt=np.longdouble``
the reference.  Imports nothing from the product.

Camera model of intrinsics group g, theta[g] = (f, cx, cy, k1, k2), asp[g] = fy / fx:

    (x, y, z) = R X + t;  xn = x / z, yn = y / z;  r2 = xn xn + yn yn
    d  = (1 + k1 r2) + k2 (r2 r2)
    r0 = ((d xn) fx + cx) - u,  r1 = ((d yn) fy + cy) - v,   fx = f, fy = f asp

Jacobians, in the kernel's order (at k1 = k2 = 0: D00 = D11 = 1, D01 = 0, e = 0, every value
equals ba_global_ref.linearize's):

    e = 2 (k1 + (2 k2) r2);  D00 = d + e (xn xn), D01 = e (xn yn), D11 = d + e (yn yn)
    a = fx / z, b = fy / z;  a00 = a D00, a01 = a D01, a10 = b D01, a11 = b D11
    d02 = -(a00 xn + a01 yn), d12 = -(a10 xn + a11 yn)
    Jp row 0: (a00 R0j + a01 R1j) + d02 R2j        row 1: (a10 R0j + a11 R1j) + d12 R2j
    Jc row 0: d02 py - a01 pz, a00 pz - d02 px, -(a00 py) + a01 px, a00, a01, d02
    Jc row 1: -(a11 pz) + d12 py, a10 pz - d12 px, a11 px - a10 py, a10, a11, d12
    Jk row 0: d xn, 1, 0, (fx xn) r2, (fx xn) (r2 r2)
    Jk row 1: asp (d yn), 0, 1, (fy yn) r2, (fy yn) (r2 r2)       (masked columns 0)

Orders beyond ba_global_ref's: a per-group sum adds the per-camera values of the group's
cameras in ascending camera index by ``ref.wg_sum`` (lane l takes the l-th, (l+256)-th, ...
camera in sequence, then the tree).  The CG vectors are (x_c.ravel(), x_k.ravel()).
"""
import numpy as np

import ba_global_ref as ref
import ba_robust_ref as rob

PARTS = {"f": (0,), "pp": (1, 2), "k1": (3,), "k2": (4,)}
UNDISTORT_ITERS = 20


def mask_of(refine):
    m = np.zeros(5, np.uint8)
    for name in refine:
        m[list(PARTS[name])] = 1
    return m


def theta_of(K, grp, dist, G):
    """theta (G,5) and asp (G,) from per-camera K (C,3,3), as the wrapper builds them (float64)."""
    K = np.asarray(K, np.float64)
    theta = np.zeros((G, 5))
    theta[:, 0] = 1.0
    asp = np.ones(G)
    for g in np.unique(grp):
        Kg = K[np.nonzero(grp == g)[0][0]]
        theta[g, :3] = Kg[0, 0], Kg[0, 2], Kg[1, 2]
        asp[g] = Kg[1, 1] / Kg[0, 0]
    theta[:, 3:] = np.broadcast_to(np.asarray(dist, np.float64).reshape(-1, 2), (G, 2))
    return theta, asp


def _cost(term, bad):
    dt = term.dtype.type
    M = len(term)
    nb = max(1, -(-M // 256))
    pad = np.zeros((nb * 256, 1), term.dtype)
    pad[:M, 0] = term
    cost = dt(0.5) * ref.wg_sum(ref._tree(pad.reshape(nb, 256, 1)))[0]
    return dt(np.inf) if bad else cost


def project(R, t, theta, asp, grp, X, oc, op):
    """The distorted projection: dict of per-observation arrays."""
    dt = X.dtype.type
    g = grp[oc]
    Ro, to, Xo, th = R[oc], t[oc], X[op], theta[g]
    fx = th[:, 0]
    fy = th[:, 0] * asp[g]
    px = (Ro[:, 0, 0] * Xo[:, 0] + Ro[:, 0, 1] * Xo[:, 1]) + Ro[:, 0, 2] * Xo[:, 2]
    py = (Ro[:, 1, 0] * Xo[:, 0] + Ro[:, 1, 1] * Xo[:, 1]) + Ro[:, 1, 2] * Xo[:, 2]
    pz = (Ro[:, 2, 0] * Xo[:, 0] + Ro[:, 2, 1] * Xo[:, 1]) + Ro[:, 2, 2] * Xo[:, 2]
    x, y, z = px + to[:, 0], py + to[:, 1], pz + to[:, 2]
    iz = dt(1) / z
    xn, yn = x * iz, y * iz
    r2 = xn * xn + yn * yn
    d = (dt(1) + th[:, 3] * r2) + th[:, 4] * (r2 * r2)
    return dict(Ro=Ro, th=th, asp=asp[g], fx=fx, fy=fy, px=px, py=py, pz=pz, z=z, iz=iz, xn=xn, yn=yn, r2=r2, d=d,
                u=(d * xn) * fx + th[:, 1], v=(d * yn) * fy + th[:, 2])


def linearize(R, t, theta, asp, grp, mask, X, oc, op, uv, loss="linear", f_scale=1.0, jac=True):
    """-> (r (M,2), Jc (M,2,6), Jk (M,2,5), Jp (M,2,3), cost, bad, w); under a robust loss the
    arrays carry sqrt(w) (jac=False: the UNWEIGHTED r, the rest None, the cost the loss's)."""
    dt = X.dtype.type
    M = len(oc)
    with np.errstate(all="ignore"):
        o = project(R, t, theta, asp, grp, X, oc, op)
        bad = bool(np.any(~(o["z"] > 0)))
        r = np.stack([o["u"] - uv[:, 0], o["v"] - uv[:, 1]], 1)
        sq = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        w = np.ones(M, X.dtype)
        if loss != "linear":
            f2 = dt(f_scale) * dt(f_scale)
            z = sq / f2
            sq = f2 * rob.rho_of_z(z, loss)
            w = rob.weight_of_z(z, loss)
        cost = _cost(sq, bad)
        if not jac:
            return r, None, None, None, cost, bad, None
        xn, yn, px, py, pz, Ro, th = o["xn"], o["yn"], o["px"], o["py"], o["pz"], o["Ro"], o["th"]
        e = dt(2) * (th[:, 3] + (dt(2) * th[:, 4]) * o["r2"])
        D00, D01, D11 = o["d"] + e * (xn * xn), e * (xn * yn), o["d"] + e * (yn * yn)
        a, b = o["fx"] * o["iz"], o["fy"] * o["iz"]
        a00, a01, a10, a11 = a * D00, a * D01, b * D01, b * D11
        d02, d12 = -(a00 * xn + a01 * yn), -(a10 * xn + a11 * yn)
        Jp = np.stack([np.stack([(a00 * Ro[:, 0, j] + a01 * Ro[:, 1, j]) + d02 * Ro[:, 2, j] for j in range(3)], 1),
                       np.stack([(a10 * Ro[:, 0, j] + a11 * Ro[:, 1, j]) + d12 * Ro[:, 2, j] for j in range(3)], 1)], 1)
        Jc = np.stack([np.stack([d02 * py - a01 * pz, a00 * pz - d02 * px, -(a00 * py) + a01 * px, a00, a01, d02], 1),
                       np.stack([-(a11 * pz) + d12 * py, a10 * pz - d12 * px, a11 * px - a10 * py, a10, a11, d12], 1)], 1)
        fxn, fyn, r4 = o["fx"] * xn, o["fy"] * yn, o["r2"] * o["r2"]
        one, zero = np.ones(M, X.dtype), np.zeros(M, X.dtype)
        Jk = np.stack([np.stack([o["d"] * xn, one, zero, fxn * o["r2"], fxn * r4], 1),
                       np.stack([o["asp"] * (o["d"] * yn), zero, one, fyn * o["r2"], fyn * r4], 1)], 1)
        Jk[:, :, np.asarray(mask) == 0] = 0
        if loss != "linear":
            sw = np.sqrt(w)
            r, Jc, Jk, Jp = sw[:, None] * r, sw[:, None, None] * Jc, sw[:, None, None] * Jk, sw[:, None, None] * Jp
    return r, Jc, Jk, Jp, cost, bad, w


def group_sum(v, grp, G):
    """(C, k) per-camera values -> (G, k): the group order of the module docstring."""
    out = np.zeros((G, v.shape[1]), v.dtype)
    for g in range(G):
        out[g] = ref.wg_sum(v[np.nonzero(grp == g)[0]])
    return out


def blocks(r, Jc, Jk, Jp, pt_off, cam_perm, cam_off, grp, G):
    """-> U (C,6,6), gc (C,6), B (C,6,5), H (G,5,5), gk (G,5), V (N,3,3), gp (N,3)."""
    U, gc, V, gp = ref.blocks(r, Jc, Jp, pt_off, cam_perm, cam_off)
    rows = np.stack([Jc[:, 0, a] * Jk[:, 0, j] + Jc[:, 1, a] * Jk[:, 1, j] for a in range(6) for j in range(5)], 1)
    B = ref.cam_sum(rows, cam_perm, cam_off).reshape(-1, 6, 5)
    H, gk = ref._unpack(group_sum(ref.cam_sum(ref._outer_rows(Jk, r), cam_perm, cam_off), grp, G), 5)
    return U, gc, B, H, gk, V, gp


def damped(U, H, V, lam, fixed):
    Us, Ui, Vi = ref.damped(U, V, lam, fixed)
    Hs = ref.damp(H, lam)
    return Us, Ui, Hs, ref.ldl_inverse(Hs), Vi


def _masked(xk, mask):
    return np.where((np.asarray(mask) != 0)[None, :], xk, 0)


def point_pass(mode, xc, xk, gp, Vi, Jc, Jk, Jp, oc, grp, mask, pt_off, fixed):
    if mode == ref.RHS:
        s = gp
    else:
        xo = np.where((fixed[oc] != 0)[:, None], 0, xc[oc])
        t0, t1 = ref._dot(Jc[:, 0], xo), ref._dot(Jc[:, 1], xo)
        xg = _masked(xk, mask)[grp[oc]]
        for j in range(5):
            t0 = t0 + Jk[:, 0, j] * xg[:, j]
            t1 = t1 + Jk[:, 1, j] * xg[:, j]
        s = ref.seg_sum_seq(Jp[:, 0] * t0[:, None] + Jp[:, 1] * t1[:, None], pt_off)
        if mode == ref.BACKSUB:
            s = gp + s
    y = np.stack([ref._dot(Vi[:, i], s) for i in range(3)], 1)
    return -y if mode == ref.BACKSUB else y


def cam_pass(y, Jc, Jk, Jp, op, cam_perm, cam_off):
    """-> (C, 11): the camera's chunk sums of (Jc^T w, Jk^T w), w = Jp y_p."""
    yo = y[op]
    w0, w1 = ref._dot(Jp[:, 0], yo), ref._dot(Jp[:, 1], yo)
    v = np.concatenate([Jc[:, 0] * w0[:, None] + Jc[:, 1] * w1[:, None],
                        Jk[:, 0] * w0[:, None] + Jk[:, 1] * w1[:, None]], 1)
    return ref.cam_sum(v, cam_perm, cam_off)


def group_pass(xc, s, B, grp, G, fixed):
    """gq (G,5): per camera ((fixed or xc None) ? 0 : B^T x_c) - s[:, 6:], summed per group."""
    bt = np.zeros((len(grp), 5), s.dtype)
    if xc is not None:
        xo = np.where((fixed != 0)[:, None], 0, xc)
        bt = np.stack([ref._dot(B[:, :, j], xo) for j in range(5)], 1)
        bt[fixed != 0] = 0
    return group_sum(bt - s[:, 6:], grp, G)


def matvec(xc, xk, Us, Hs, Vi, B, Jc, Jk, Jp, oc, op, grp, mask, pt_off, cam_perm, cam_off, fixed):
    """-> (out_c (C,6), out_k (G,5)) = S~ x~ from damped blocks."""
    G = Hs.shape[0]
    free = (fixed == 0)[:, None]
    y = point_pass(ref.MATVEC, xc, xk, None, Vi, Jc, Jk, Jp, oc, grp, mask, pt_off, fixed)
    s = cam_pass(y, Jc, Jk, Jp, op, cam_perm, cam_off)
    gq = group_pass(xc, s, B, grp, G, fixed)
    xm = _masked(xk, mask)
    bx = np.stack([ref._dot(B[:, a], xm[grp]) for a in range(6)], 1)
    out_c = np.where(free, (ref._blockmul(Us, np.where(free, xc, 0)) + bx) - s[:, :6], 0)
    out_k = _masked(ref._blockmul(Hs, xm) + gq, mask)
    return out_c, out_k


def schur_matvec(x, lam, U, B, H, V, Jc, Jk, Jp, oc, op, grp, mask, pt_off, cam_perm, cam_off, fixed):
    """out (6C + 5G,) = S~(lam) x for the flat x~."""
    C, G = U.shape[0], H.shape[0]
    Us, _, Hs, _, Vi = damped(U, H, V, lam, fixed)
    oc_, ok_ = matvec(x[:6 * C].reshape(C, 6), x[6 * C:].reshape(G, 5), Us, Hs, Vi, B, Jc, Jk, Jp, oc, op, grp, mask,
                      pt_off, cam_perm, cam_off, fixed)
    return np.concatenate([oc_.ravel(), ok_.ravel()])


def dense_system(lam, U, gc, B, H, gk, V, gp, r, Jc, Jk, Jp, oc, op, grp, mask, fixed):
    """Dense S~ (n, n), b (n,), n = 6C + 5G, from dense Jacobians (tests; longdouble).  Rows and
    columns of fixed cameras and masked components are 0."""
    C, G, N, M = U.shape[0], H.shape[0], V.shape[0], len(oc)
    dt = U.dtype
    n = 6 * C + 5 * G
    A = np.zeros((2 * M, n), dt)
    P = np.zeros((2 * M, 3 * N), dt)
    for m in range(M):
        A[2 * m:2 * m + 2, 6 * oc[m]:6 * oc[m] + 6] = Jc[m]
        A[2 * m:2 * m + 2, 6 * C + 5 * grp[oc[m]]:6 * C + 5 * grp[oc[m]] + 5] = Jk[m]
        P[2 * m:2 * m + 2, 3 * op[m]:3 * op[m] + 3] = Jp[m]
    dead = np.zeros(n, bool)
    dead[:6 * C] = np.repeat(fixed != 0, 6)
    dead[6 * C:] = np.tile(np.asarray(mask) == 0, G)
    A[:, dead] = 0
    Us, _, Hs, _, Vi = damped(U, H, V, lam, fixed)
    Vd = np.zeros((3 * N, 3 * N), dt)
    for p in range(N):
        Vd[3 * p:3 * p + 3, 3 * p:3 * p + 3] = Vi[p]
    W = A.T @ P
    S = A.T @ A - W @ Vd @ W.T
    for c in range(C):
        S[6 * c:6 * c + 6, 6 * c:6 * c + 6] += Us[c] - U[c]
    for g in range(G):
        S[6 * C + 5 * g:6 * C + 5 * g + 5, 6 * C + 5 * g:6 * C + 5 * g + 5] += Hs[g] - H[g]
    S[dead] = 0
    S[:, dead] = 0
    b = -(A.T @ r.ravel() - W @ Vd @ (P.T @ r.ravel()))
    b[dead] = 0
    return S, b


def dense_magnitude(lam, q, fixed):
    """|A^T A| + |W V*^-1 W^T| (n, n) of a linearisation dict q (keys as ba_calib_scenes.ref_linearize):
    the size of the terms whose difference S~ is, for rounding bounds of a product S~ x."""
    C, G, N, M = q["U"].shape[0], q["H"].shape[0], q["V"].shape[0], len(q["oc"])
    n = 6 * C + 5 * G
    A = np.zeros((2 * M, n), q["U"].dtype)
    P = np.zeros((2 * M, 3 * N), q["U"].dtype)
    for m in range(M):
        c = q["oc"][m]
        if not fixed[c]:
            A[2 * m:2 * m + 2, 6 * c:6 * c + 6] = q["Jc"][m]
        A[2 * m:2 * m + 2, 6 * C + 5 * q["grp"][c]:6 * C + 5 * q["grp"][c] + 5] = q["Jk"][m]
        P[2 * m:2 * m + 2, 3 * q["op"][m]:3 * q["op"][m] + 3] = q["Jp"][m]
    Vi = ref.ldl_inverse(ref.damp(q["V"], lam))
    Vd = np.zeros((3 * N, 3 * N), q["U"].dtype)
    for p in range(N):
        Vd[3 * p:3 * p + 3, 3 * p:3 * p + 3] = Vi[p]
    W = A.T @ P
    return (1 + lam) * np.abs(A.T @ A) + np.abs(W) @ np.abs(Vd) @ np.abs(W.T)


def _vsum(a, b):
    return ref.wg_sum((a * b).reshape(-1, 1))[0]


def pcg(lam, U, gc, B, H, gk, V, gp, Jc, Jk, Jp, oc, op, grp, mask, pt_off, cam_perm, cam_off, fixed, eta, max_cg):
    """Block-Jacobi PCG on S~ x~ = b from 0 -> (x_c, x_k, iterations, Vi)."""
    dt = U.dtype.type
    C, G = U.shape[0], H.shape[0]
    Us, Ui, Hs, Hi, Vi = damped(U, H, V, lam, fixed)
    free = (fixed == 0)[:, None]
    cat = lambda c, k: np.concatenate([c.ravel(), k.ravel()])
    split = lambda v: (v[:6 * C].reshape(C, 6), v[6 * C:].reshape(G, 5))
    s = cam_pass(point_pass(ref.RHS, None, None, gp, Vi, Jc, Jk, Jp, oc, grp, mask, pt_off, fixed), Jc, Jk, Jp, op,
                 cam_perm, cam_off)
    gq = group_pass(None, s, B, grp, G, fixed)
    b = cat(np.where(free, -(gc - s[:, :6]), 0), _masked(-(gk + gq), mask))
    x = np.zeros_like(b)
    r = b.copy()
    precond = lambda v: cat(ref._blockmul(Ui, split(v)[0]), ref._blockmul(Hi, split(v)[1]))
    z = precond(r)
    p = z.copy()
    rz = _vsum(r, z)
    bb = _vsum(b, b)
    it = 0
    if not bb > 0:
        return (*split(x), it, Vi)
    while it < max_cg:
        q = cat(*matvec(*split(p), Us, Hs, Vi, B, Jc, Jk, Jp, oc, op, grp, mask, pt_off, cam_perm, cam_off, fixed))
        pq = _vsum(p, q)
        if not pq > 0:
            break
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        rr = _vsum(r, r)
        it += 1
        if np.sqrt(rr) <= dt(eta) * np.sqrt(bb):
            break
        z = precond(r)
        rz_new = _vsum(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return (*split(x), it, Vi)


def setup(cam, theta, asp, grp, X, obs_cam, obs_pt, pts2d, dt):
    """Sorted layout and the state in dt."""
    cam = np.array(cam, dt).reshape(-1, 6)
    X = np.array(X, dt).reshape(-1, 3)
    C, N = len(cam), len(X)
    obs_cam, obs_pt = np.asarray(obs_cam, np.int64), np.asarray(obs_pt, np.int64)
    order, pt_off, cam_perm, cam_off = ref.structure(obs_cam, obs_pt, C, N)
    R = np.stack([ref.rodrigues(c[:3], dt) for c in cam]) if C else np.zeros((0, 3, 3), dt)
    return dict(cam=cam, X=X, C=C, N=N, order=order, pt_off=pt_off, cam_perm=cam_perm, cam_off=cam_off,
                oc=obs_cam[order], op=obs_pt[order], uv=np.asarray(pts2d, dt).reshape(-1, 2)[order], R=R,
                t=cam[:, 3:].copy(), theta=np.array(theta, dt).reshape(-1, 5), asp=np.asarray(asp, dt),
                grp=np.asarray(grp, np.int64))


def solve(cam, theta, asp, grp, mask, X, obs_cam, obs_pt, pts2d, fixed=None, gtol=1e-8, ftol=1e-10, eta=1e-2,
          max_iter=50, max_cg=64, dt=np.float64, loss="linear", f_scale=1.0, trace=None):
    """The whole solve -> dict(cam, theta, X, cost0, cost, status, nit, n_accept, n_cg, residual, weight)."""
    s = setup(cam, theta, asp, grp, X, obs_cam, obs_pt, pts2d, dt)
    cam, X, theta, asp, grp = s["cam"], s["X"], s["theta"], s["asp"], s["grp"]
    C, N, G, M = s["C"], s["N"], len(theta), len(s["oc"])
    mask = np.asarray(mask, np.uint8)
    fixed = np.zeros(C, np.uint8) if fixed is None else np.asarray(fixed, np.uint8)
    oc, op, uv, pt_off, cam_perm, cam_off = s["oc"], s["op"], s["uv"], s["pt_off"], s["cam_perm"], s["cam_off"]
    res = dict(cam=cam.copy(), theta=theta.copy(), X=X.copy(), cost0=dt(0), cost=dt(0), status=-1, nit=0, n_accept=0,
               n_cg=0, residual=np.full(M, np.nan, dt), weight=np.full(M, np.nan, dt))
    R, t = s["R"], s["t"]
    free = (fixed == 0)[:, None]
    lin = lambda R, t, th, X, jac=True: linearize(R, t, th, asp, grp, mask, X, oc, op, uv, loss, f_scale, jac)
    r, Jc, Jk, Jp, cost, bad, _ = lin(R, t, theta, X)
    if bad:
        res["status"] = -2
        return res
    res["cost0"] = cost
    lam, nit, n_accept, n_cg, rel = dt(ref.LAMBDA0), 1, 0, 0, dt(np.inf)
    while True:
        U, gc, B, H, gk, V, gp = blocks(r, Jc, Jk, Jp, pt_off, cam_perm, cam_off, grp, G)
        gmax = max(np.abs(np.where(free, gc, 0)).max(initial=0), np.abs(gp).max(initial=0),
                   np.abs(_masked(gk, mask)).max(initial=0))
        if gmax <= gtol:
            status = 1
            break
        if rel <= ftol:
            status = 2
            break
        accepted = False
        while True:
            dc, dk, it, Vi = pcg(lam, U, gc, B, H, gk, V, gp, Jc, Jk, Jp, oc, op, grp, mask, pt_off, cam_perm, cam_off,
                                 fixed, eta, max_cg)
            n_cg += it
            dp = point_pass(ref.BACKSUB, dc, dk, gp, Vi, Jc, Jk, Jp, oc, grp, mask, pt_off, fixed)
            Rt, tt = R.copy(), t.copy()
            for c in range(C):
                if not fixed[c]:
                    Rt[c], tt[c] = ref.left_update(R[c], t[c], dc[c])
            Xt = X + dp
            tht = np.where((mask != 0)[None, :], theta + dk, theta)
            cost_t = lin(Rt, tt, tht, Xt, jac=False)[4]
            if trace is not None:
                trace.append((float(lam), float(cost), float(cost_t), it))
            if cost_t < cost:
                rel = (cost - cost_t) / cost
                R, t, X, theta, cost = Rt, tt, Xt, tht, cost_t
                lam = max(lam / dt(3), dt(ref.LAMBDA_MIN))
                n_accept += 1
                accepted = True
                break
            lam = lam * dt(4)
            if lam > ref.LAMBDA_MAX:
                break
        if not accepted:
            status = 3
            break
        if nit == max_iter:
            status = 0
            break
        r, Jc, Jk, Jp, cost, _, _ = lin(R, t, theta, X)
        nit += 1
    if n_accept:
        touched = (fixed == 0) & (cam_off[1:] > cam_off[:-1])
        for c in np.nonzero(touched)[0]:
            cam[c, :3] = ref.rodrigues_inverse(R[c])
            cam[c, 3:] = t[c]
    rf = linearize(R, t, theta, asp, grp, mask, X, oc, op, uv, jac=False)[0] if M else np.zeros((0, 2), dt)
    e2 = np.zeros(M, dt)
    e2[s["order"]] = rf[:, 0] * rf[:, 0] + rf[:, 1] * rf[:, 1]
    res.update(cam=cam, theta=theta, X=X, cost=cost, status=status, nit=nit, n_accept=n_accept, n_cg=n_cg,
               residual=np.sqrt(e2), weight=rob.weights(e2, loss, f_scale, dt)[1])
    return res


# ---------------------------------------------------------------------------
# undistortion (geometry.hip undistort_kernel)
def distort_points(p, K, dist, dt=np.float64):
    """Undistorted pixels (n,2) -> the pixels the radial model gives under the same K."""
    p, K = np.asarray(p, dt), np.asarray(K, dt)
    k1, k2 = (dt(v) for v in dist)
    xn, yn = (p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]
    r2 = xn * xn + yn * yn
    d = (dt(1) + k1 * r2) + k2 * (r2 * r2)
    return np.stack([(d * xn) * K[0, 0] + K[0, 2], (d * yn) * K[1, 1] + K[1, 2]], 1)


def undistort_points(p, K, dist, dt=np.float64, iters=UNDISTORT_ITERS):
    """The kernel op for op: ``iters`` steps xn <- xd / d(xn) from xn = xd, no early exit."""
    p, K = np.asarray(p, dt), np.asarray(K, dt)
    k1, k2 = (dt(v) for v in dist)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xd, yd = (p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy
    xn, yn = xd.copy(), yd.copy()
    for _ in range(iters):
        r2 = xn * xn + yn * yn
        d = (dt(1) + k1 * r2) + k2 * (r2 * r2)
        xn = xd / d
        yn = yd / d
    return np.stack([xn * fx + cx, yn * fy + cy], 1)


# ---------------------------------------------------------------------------
# scipy's dense optimum over cameras, free intrinsics and points (tests only)
_OPTIMA = {}


def scipy_optimum(cam, theta, asp, grp, mask, X, obs_cam, obs_pt, pts2d, fixed):
    """As ba_global_ref.scipy_optimum with the free components of theta among the unknowns:
    dict(cost, g2, lmin, bound, theta); bound = g2 / (2 lmin)."""
    from scipy.optimize import least_squares
    ld = np.longdouble
    cam, X, pts2d = np.asarray(cam, np.float64), np.asarray(X, np.float64), np.asarray(pts2d, np.float64)
    theta0 = np.asarray(theta, np.float64).reshape(-1, 5)
    mask, fixed = np.asarray(mask, np.uint8), np.asarray(fixed)
    key = hash((cam.tobytes(), X.tobytes(), pts2d.tobytes(), fixed.tobytes(), theta0.tobytes(), mask.tobytes()))
    if key in _OPTIMA:
        return _OPTIMA[key]
    s = setup(cam, theta0, asp, grp, X, obs_cam, obs_pt, pts2d, np.float64)
    C, N, G = s["C"], s["N"], len(theta0)
    free = np.nonzero(fixed == 0)[0]
    fk = np.nonzero(mask)[0]
    nc, nk = 6 * len(free), len(fk) * G

    def unpack(x, dt):
        R, t = s["R"].astype(dt), s["t"].astype(dt)
        for k, c in enumerate(free):
            R[c], t[c] = ref.left_update(R[c], t[c], x[6 * k:6 * k + 6].astype(dt))
        th = theta0.astype(dt)
        th[:, fk] = th[:, fk] + x[nc:nc + nk].reshape(G, len(fk)).astype(dt)
        return R, t, th, x[nc + nk:].reshape(N, 3).astype(dt)

    def fun(x):
        R, t, th, Xx = unpack(x, np.float64)
        o = project(R, t, th, s["asp"], s["grp"], Xx, s["oc"], s["op"])
        return np.stack([o["u"] - s["uv"][:, 0], o["v"] - s["uv"][:, 1]], 1).ravel()

    x_scale = np.concatenate([np.ones(nc), np.tile(np.array([1e3, 1e1, 1e1, 1e-1, 1e-1])[fk], G), np.ones(3 * N)])
    sol = least_squares(fun, np.concatenate([np.zeros(nc + nk), X.ravel()]), jac="2-point", ftol=1e-14, xtol=1e-14,
                        gtol=1e-14, x_scale=x_scale)
    R, t, th, Xs = unpack(sol.x, ld)
    r, Jc, Jk, Jp, cost, _, _ = linearize(R, t, th, s["asp"].astype(ld), s["grp"], mask, Xs, s["oc"], s["op"],
                                          s["uv"].astype(ld))
    M = len(s["oc"])
    J = np.zeros((2 * M, nc + nk + 3 * N))
    pos = {c: k for k, c in enumerate(free)}
    for m in range(M):
        c = s["oc"][m]
        if c in pos:
            J[2 * m:2 * m + 2, 6 * pos[c]:6 * pos[c] + 6] = Jc[m]
        g = s["grp"][c]
        J[2 * m:2 * m + 2, nc + len(fk) * g:nc + len(fk) * (g + 1)] = Jk[m][:, fk]
        J[2 * m:2 * m + 2, nc + nk + 3 * s["op"][m]:nc + nk + 3 * s["op"][m] + 3] = Jp[m]
    g = J.T.astype(ld) @ r.ravel()
    g2 = float((g * g).sum())
    lmin = float(np.linalg.eigvalsh(J.T @ J)[0])
    out = dict(cost=cost, g2=g2, lmin=lmin, bound=g2 / (2 * lmin), theta=th)
    _OPTIMA[key] = out
    return out
