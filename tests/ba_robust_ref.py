"""numpy restatement of the robust loss of the global bundle adjustment
(``k_linearize<JAC, LOSS>`` in ba_global.hip, DESIGN.md K3‴ "Robust loss"), on top of
tests/ba_global_ref.py, which it imports and does not change.  Dtype-generic like it:
``dt=np.float64`` is the kernels' arithmetic, ``dt=np.longdouble`` the reference.

The loss acts on the 2-vector of an observation (as Ceres does, not per scalar component
as scipy's ``least_squares`` does).  Per observation, in the kernel's order:

    e2 = r0 r0 + r1 r1            (the unweighted residual of ba_global_ref.linearize)
    f2 = f_scale f_scale
    z  = e2 / f2
    cost term = f2 rho(z)         (summed like |r|^2 of the linear loss, then halved)
    w  = rho'(z),  sw = sqrt(w)
    stored: sw r, sw Jc, sw Jp

with scipy's rho: huber z if z <= 1 else 2 sqrt(z) - 1 (rho' = 1 / sqrt(z) there), soft_l1
2 (sqrt(1 + z) - 1) (rho' = 1 / sqrt(1 + z)), cauchy log1p(z) (rho' = 1 / (1 + z)).  Plain
IRLS: everything after the linearisation (blocks, damping, CG, back-substitution, the
trial cost through the same cost term, the step rule) is ba_global_ref's, unchanged.
"""
import numpy as np

import ba_global_ref as ref

LOSSES = ("linear", "huber", "soft_l1", "cauchy")


def rho_of_z(z, loss):
    """rho(z) in z's dtype."""
    z = np.asarray(z)
    one = z.dtype.type(1)
    two = z.dtype.type(2)
    if loss == "huber":
        return np.where(z <= one, z, two * np.sqrt(z) - one)
    if loss == "soft_l1":
        return two * (np.sqrt(one + z) - one)
    if loss == "cauchy":
        return np.log1p(z)
    if loss == "linear":
        return z.copy()
    raise ValueError(loss)


def weight_of_z(z, loss):
    """rho'(z) in z's dtype."""
    z = np.asarray(z)
    one = z.dtype.type(1)
    with np.errstate(divide="ignore"):
        if loss == "huber":
            return np.where(z <= one, one, one / np.sqrt(z))
        if loss == "soft_l1":
            return one / np.sqrt(one + z)
        if loss == "cauchy":
            return one / (one + z)
    if loss == "linear":
        return np.ones_like(z)
    raise ValueError(loss)


def weights(e2, loss, f_scale, dt=np.float64):
    """(z, w) of squared residual norms e2 at scale f_scale."""
    e2 = np.asarray(e2, dt)
    f2 = dt(f_scale) * dt(f_scale)
    z = e2 / f2
    return z, weight_of_z(z, loss)


def linearize(R, t, K, X, oc, op, uv, loss="linear", f_scale=1.0, jac=True):
    """ba_global_ref.linearize under the loss -> (r, Jc, Jp, cost, bad, w): the weighted
    arrays, the robust cost and the weight per sorted observation (jac=False: r is the
    UNWEIGHTED residual, Jc = Jp = w = None, only the cost is the loss's)."""
    r, Jc, Jp, cost, bad = ref.linearize(R, t, K, X, oc, op, uv, jac=jac)
    if loss == "linear":
        return r, Jc, Jp, cost, bad, (np.ones(len(oc), X.dtype) if jac else None)
    dt = X.dtype.type
    M = len(oc)
    with np.errstate(all="ignore"):
        e2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        f2 = dt(f_scale) * dt(f_scale)
        z = e2 / f2
        term = (f2 * rho_of_z(z, loss))[:, None]
        nb = max(1, -(-M // 256))
        pad = np.zeros((nb * 256, 1), term.dtype)
        pad[:M] = term
        cost = dt(0.5) * ref.wg_sum(ref._tree(pad.reshape(nb, 256, 1)))[0]
        if bad:
            cost = dt(np.inf)
        if not jac:
            return r, None, None, cost, bad, None
        w = weight_of_z(z, loss)
        sw = np.sqrt(w)
        return sw[:, None] * r, sw[:, None, None] * Jc, sw[:, None, None] * Jp, cost, bad, w


def solve(cam, K, X, obs_cam, obs_pt, pts2d, fixed=None, gtol=1e-8, ftol=1e-10, eta=1e-2, max_iter=50,
          max_cg=64, dt=np.float64, trace=None, loss="linear", f_scale=1.0):
    """ba_global_ref.solve with the loss's linearisation and trial cost -> its dict plus
    ``residual`` (M,), the final unweighted |r| in the caller's order, and ``weight`` (M,).
    With loss="linear" every operation is ba_global_ref.solve's."""
    if loss not in LOSSES:
        raise ValueError(loss)
    cam = np.array(cam, dt).reshape(-1, 6)
    X = np.array(X, dt).reshape(-1, 3)
    K = np.asarray(K, dt)
    C, N = len(cam), len(X)
    fixed = np.zeros(C, np.uint8) if fixed is None else np.asarray(fixed, np.uint8)
    obs_cam, obs_pt = np.asarray(obs_cam, np.int64), np.asarray(obs_pt, np.int64)
    M = len(obs_cam)
    res = dict(cam=cam.copy(), X=X.copy(), cost0=dt(0), cost=dt(0), status=-1, nit=0, n_accept=0, n_cg=0,
               residual=np.full(M, np.nan, dt), weight=np.full(M, np.nan, dt))
    if M and (obs_cam.min() < 0 or obs_cam.max() >= C or obs_pt.min() < 0 or obs_pt.max() >= N):
        return res
    order, pt_off, cam_perm, cam_off = ref.structure(obs_cam, obs_pt, C, N)
    oc, op, uv = obs_cam[order], obs_pt[order], np.asarray(pts2d, dt).reshape(-1, 2)[order]
    R = np.stack([ref.rodrigues(c[:3], dt) for c in cam]) if C else np.zeros((0, 3, 3), dt)
    t = cam[:, 3:].copy()
    free = (fixed == 0)[:, None]
    r, Jc, Jp, cost, bad, _ = linearize(R, t, K, X, oc, op, uv, loss, f_scale)
    if bad:
        res["status"] = -2
        return res
    res["cost0"] = cost
    lam, nit, n_accept, n_cg, rel = dt(ref.LAMBDA0), 1, 0, 0, dt(np.inf)
    while True:
        U, gc, V, gp = ref.blocks(r, Jc, Jp, pt_off, cam_perm, cam_off)
        gmax = max(np.abs(np.where(free, gc, 0)).max(initial=0), np.abs(gp).max(initial=0))
        if gmax <= gtol:
            status = 1
            break
        if rel <= ftol:
            status = 2
            break
        accepted = False
        while True:
            dc, it, Vi = ref.pcg(lam, U, gc, V, gp, Jc, Jp, oc, op, pt_off, cam_perm, cam_off, fixed, eta, max_cg)
            n_cg += it
            dp = ref.point_pass(ref.BACKSUB, dc, gp, Vi, Jc, Jp, oc, pt_off, fixed)
            Rt, tt = R.copy(), t.copy()
            for c in range(C):
                if not fixed[c]:
                    Rt[c], tt[c] = ref.left_update(R[c], t[c], dc[c])
            Xt = X + dp
            _, _, _, cost_t, _, _ = linearize(Rt, tt, K, Xt, oc, op, uv, loss, f_scale, jac=False)
            if trace is not None:
                trace.append((float(lam), float(cost), float(cost_t), it))
            if cost_t < cost:
                rel = (cost - cost_t) / cost
                R, t, X, cost = Rt, tt, Xt, cost_t
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
        r, Jc, Jp, cost, _, _ = linearize(R, t, K, X, oc, op, uv, loss, f_scale)
        nit += 1
    if n_accept:
        touched = (fixed == 0) & (cam_off[1:] > cam_off[:-1])
        for c in np.nonzero(touched)[0]:
            cam[c, :3] = ref.rodrigues_inverse(R[c])
            cam[c, 3:] = t[c]
    rf = ref.linearize(R, t, K, X, oc, op, uv, jac=False)[0] if M else np.zeros((0, 2), dt)
    e2 = np.zeros(M, dt)
    e2[order] = rf[:, 0] * rf[:, 0] + rf[:, 1] * rf[:, 1]
    res.update(cam=cam, X=X, cost=cost, status=status, nit=nit, n_accept=n_accept, n_cg=n_cg, residual=np.sqrt(e2),
               weight=weights(e2, loss, f_scale, dt)[1])
    return res
