"""numpy restatement of V11, the SIFT of include/sfmhip.h (sift.hip), written from
the header text: every f32 step in the order given there, vectorised over pixels / keypoints.
The tables (taps, radii, sig, wo, wd, cw, cs) are arguments, as they are for the kernels.
One view at a time; records are (N, 8) int32 with the floats as their bits.
detect, orient and describe take an optional dict `census` and count in it the branches they take
(tests/test_sift_census_cpu.py); it changes nothing they return."""
import numpy as np

f32 = np.float32
S, L = 3, 6
C = [f32(float.fromhex(h)) for h in ("0x1.45e8e8p-3", "-0x1.aec82ap-5", "0x1.d67172p-6", "-0x1.bd6ba4p-7",
                                     "0x1.b4a748p-9")]


def layout(H, W, O):
    dims, off = [], 0
    for o in range(O):
        h, w = ((H - 1) >> o) + 1, ((W - 1) >> o) + 1
        dims.append((h, w, off))
        off += L * h * w
    return dims, off


def blur(src, taps, r):
    """rows first, then columns; acc = 0, then acc = acc + tap[k] src[clamp(i + k - r)] for ascending k."""
    H, W = src.shape
    nt = 2 * r + 1
    xi = np.clip(np.arange(W)[None, :] + np.arange(nt)[:, None] - r, 0, W - 1)
    yi = np.clip(np.arange(H)[None, :] + np.arange(nt)[:, None] - r, 0, H - 1)
    acc = np.zeros((H, W), f32)
    for k in range(nt):
        acc = acc + f32(taps[k]) * src[:, xi[k]]
    tmp = acc
    acc = np.zeros((H, W), f32)
    for k in range(nt):
        acc = acc + f32(taps[k]) * tmp[yi[k], :]
    return acc


def pyramid(img, O, tb):
    """img (H,W) u8 -> list of O arrays (6, H_o, W_o) f32."""
    octs = []
    for o in range(O):
        base = img.astype(f32) if o == 0 else octs[-1][S][::2, ::2]
        lv = [blur(base, tb["taps"][0], int(tb["radii"][0])) if o == 0 else np.ascontiguousarray(base)]
        for s in range(1, L):
            lv.append(blur(lv[-1], tb["taps"][s], int(tb["radii"][s])))
        octs.append(np.stack(lv))
    return octs


def flat(octs):
    """One view's pyramid as the buffer of the header: octaves, then levels, row-major."""
    return np.concatenate([g.ravel() for g in octs])


def _count(census, key, n=1):
    if census is not None:
        census[key] = census.get(key, 0) + int(n)


def in_contract(rec, O):
    """The record contract of the header: octave and level in range, x, y and the scale finite and
    at most 2^20 in magnitude, the scale positive.  A record outside it reads nothing."""
    o, l, _, x, y, sc = _fields(rec)
    big = f32(1048576)
    with np.errstate(invalid="ignore"):
        return (o >= 0) & (o < O) & (l >= 1) & (l <= S) & (np.abs(x) <= big) & (np.abs(y) <= big) & (sc > 0) & \
            (sc <= big)


def detect(octs, tb, border=5, contrast=0.04, edge=10.0, census=None):
    """census (a dict, optional) counts the branches taken: it changes nothing that is returned."""
    pre = f32(0.5 * contrast / S * 255.0)
    cthr = f32(contrast * 255.0)
    er = f32(edge)
    sig = tb["sig"].astype(f32)
    out = []
    for o, G in enumerate(octs):
        _, H, W = G.shape
        if H < 2 * border + 1 or W < 2 * border + 1:
            continue
        D = G[1:] - G[:-1]
        ys, xs = slice(border, H - border), slice(border, W - border)
        v = D[1:S + 1, ys, xs]
        gt = np.abs(v) > pre
        lt = gt.copy()
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl == dy == dx == 0:
                        continue
                    n = D[1 + dl:S + 1 + dl, border + dy:H - border + dy, border + dx:W - border + dx]
                    gt &= v > n
                    lt &= v < n
        cand = np.argwhere(gt | lt)   # ascending (level, row, column)
        _count(census, "start", cand.shape[0])
        if cand.shape[0] == 0:
            continue
        l, y, x = cand[:, 0] + 1, cand[:, 1] + border, cand[:, 2] + border
        N = l.shape[0]
        alive = np.ones(N, bool)
        conv = np.zeros(N, bool)
        fin = {k: np.zeros(N, f32) for k in ("c", "gx", "gy", "gl", "hxx", "hyy", "hxy", "ox", "oy", "ol")}
        with np.errstate(all="ignore"):
            for it in range(5):
                act = alive & ~conv
                c = D[l, y, x]
                xp, xm, yp, ym, lp, lm = D[l, y, x + 1], D[l, y, x - 1], D[l, y + 1, x], D[l, y - 1, x], D[l + 1, y, x], \
                    D[l - 1, y, x]
                gx, gy, gl = (xp - xm) * f32(0.5), (yp - ym) * f32(0.5), (lp - lm) * f32(0.5)
                c2 = f32(2) * c
                hxx, hyy, hll = (xp + xm) - c2, (yp + ym) - c2, (lp + lm) - c2
                hxy = ((D[l, y + 1, x + 1] - D[l, y + 1, x - 1]) - (D[l, y - 1, x + 1] - D[l, y - 1, x - 1])) * f32(0.25)
                hxl = ((D[l + 1, y, x + 1] - D[l + 1, y, x - 1]) - (D[l - 1, y, x + 1] - D[l - 1, y, x - 1])) * f32(0.25)
                hyl = ((D[l + 1, y + 1, x] - D[l + 1, y - 1, x]) - (D[l - 1, y + 1, x] - D[l - 1, y - 1, x])) * f32(0.25)
                A00, A01, A02 = hyy * hll - hyl * hyl, hxl * hyl - hxy * hll, hxy * hyl - hxl * hyy
                A11, A12, A22 = hxx * hll - hxl * hxl, hxy * hxl - hxx * hyl, hxx * hyy - hxy * hxy
                det = (hxx * A00 + hxy * A01) + hxl * A02
                okdet = np.abs(det) > 0
                ox = -(((A00 * gx + A01 * gy) + A02 * gl) / det)
                oy = -(((A01 * gx + A11 * gy) + A12 * gl) / det)
                ol = -(((A02 * gx + A12 * gy) + A22 * gl) / det)
                cv = (np.abs(ox) < f32(0.5)) & (np.abs(oy) < f32(0.5)) & (np.abs(ol) < f32(0.5))
                small = (np.abs(ox) <= f32(1048576)) & (np.abs(oy) <= f32(1048576)) & (np.abs(ol) <= f32(1048576))
                now = act & okdet & cv
                for k, a in (("c", c), ("gx", gx), ("gy", gy), ("gl", gl), ("hxx", hxx), ("hyy", hyy), ("hxy", hxy),
                             ("ox", ox), ("oy", oy), ("ol", ol)):
                    fin[k][now] = a[now]
                conv |= now
                alive &= ~(act & (~okdet | (~cv & ~small)))
                mv = act & okdet & ~cv & small
                nl = l + np.where(mv, np.rint(ol), 0).astype(np.int64)
                ny = y + np.where(mv, np.rint(oy), 0).astype(np.int64)
                nx = x + np.where(mv, np.rint(ox), 0).astype(np.int64)
                inb = (nl >= 1) & (nl <= S) & (ny >= border) & (ny <= H - 1 - border) & (nx >= border) & \
                    (nx <= W - 1 - border)
                alive &= ~(mv & ~inb)
                ok = mv & inb
                l0 = l
                l, y, x = np.where(ok, nl, l), np.where(ok, ny, y), np.where(ok, nx, x)
                if census is not None:
                    lev = (nl >= 1) & (nl <= S)
                    _count(census, "det0", (act & ~okdet).sum())
                    _count(census, "offset_above_2^20", (act & okdet & ~cv & ~small).sum())
                    _count(census, "conv_solve_%d" % (it + 1), now.sum())
                    _count(census, "move", ok.sum())
                    _count(census, "move_level", (ok & (nl != l0)).sum())
                    _count(census, "leave_level", (mv & ~lev).sum())
                    _count(census, "leave_rowcol", (mv & lev & ~inb).sum())
            keep = alive & conv
            _count(census, "no_conv_after_5", (alive & ~conv).sum())
            ox, oy, ol = fin["ox"], fin["oy"], fin["ol"]
            resp = fin["c"] + f32(0.5) * ((fin["gx"] * ox + fin["gy"] * oy) + fin["gl"] * ol)
            strong = np.abs(resp) * f32(3) >= cthr
            tr = fin["hxx"] + fin["hyy"]
            d2 = fin["hxx"] * fin["hyy"] - fin["hxy"] * fin["hxy"]
            e1 = er + f32(1)
            round_ = (tr * tr) * er < (e1 * e1) * d2
            _count(census, "contrast", (keep & ~strong).sum())
            _count(census, "d2", (keep & strong & ~(d2 > 0)).sum())
            _count(census, "edge", (keep & strong & (d2 > 0) & ~round_).sum())
            _count(census, "edge_both_sides_equal", (keep & strong & (d2 > 0) & ((tr * tr) * er == (e1 * e1) * d2)).sum())
            keep &= strong & (d2 > 0) & round_
        l, y, x, ox, oy, ol, resp = (a[keep] for a in (l, y, x, ox, oy, ol, resp))
        if census is not None:
            _count(census, "scale_ol>=0", (ol >= 0).sum())
            _count(census, "scale_ol<0", (ol < 0).sum())
            for ll in range(1, S + 1):
                _count(census, "kept_level_%d" % ll, (l == ll).sum())
            _count(census, "records", l.shape[0])
        s0 = sig[l]
        sc = np.where(ol >= 0, s0 + ol * (sig[l + 1] - s0), s0 + ol * (s0 - sig[l - 1])).astype(f32)
        fx, fy, po = x.astype(f32) + ox, y.astype(f32) + oy, f32(1 << o)
        rec = np.zeros((l.shape[0], 8), np.int32)
        rec[:, 0], rec[:, 1] = o, l
        for j, a in enumerate((fx, fy, sc, np.abs(resp), fx * po, fy * po)):
            rec[:, 2 + j] = a.astype(f32).view(np.int32)
        out.append(rec)
    return np.concatenate(out) if out else np.zeros((0, 8), np.int32)


def turn(y, x):
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    a, b = np.abs(x), np.abs(y)
    m, mn = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(all="ignore"):
        t = np.where(m == 0, f32(0), mn / m).astype(f32)
    u = t * t
    p = C[4] * u + C[3]
    p = p * u + C[2]
    p = p * u + C[1]
    p = p * u + C[0]
    p = p * t
    p = np.where(b > a, f32(0.25) - p, p)
    p = np.where(np.signbit(x), f32(0.5) - p, p)
    p = np.where(np.signbit(y), f32(1) - p, p)
    return np.where(p >= f32(1), f32(0), p).astype(f32)


def sample(G, px, py):
    H, W = G.shape
    x0, y0 = np.floor(px), np.floor(py)
    fx, fy = px - x0, py - y0
    xi = np.fmin(np.fmax(x0, f32(-1)), f32(W)).astype(np.int64)
    yi = np.fmin(np.fmax(y0, f32(-1)), f32(H)).astype(np.int64)
    i0, i1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
    j0, j1 = np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
    one = f32(1)
    top = G[j0, i0] * (one - fx) + G[j0, i1] * fx
    bot = G[j1, i0] * (one - fx) + G[j1, i1] * fx
    return top * (one - fy) + bot * fy


def _fields(rec):
    fl = rec.view(f32)
    return rec[:, 0], rec[:, 1] & 0xff, (rec[:, 1] >> 8) & 1023, fl[:, 2], fl[:, 3], fl[:, 4]


def _patches(octs, rec, n, pos):
    """P (N, n, n): pos(record fields, i, j) -> (px, py), sampled on the level of each record."""
    o, l, _, _, _, _ = _fields(rec)
    P = np.zeros((rec.shape[0], n, n), f32)
    for oo in np.unique(o):
        for ll in np.unique(l[o == oo]):
            sel = np.nonzero((o == oo) & (l == ll))[0]
            px, py = pos(sel)
            P[sel] = sample(octs[oo][ll], px, py)
    return P


def orient(octs, rec, tb, census=None):
    """(N, 8) records -> (M, 8) oriented records (word 1 = level | q << 8).  A record outside the
    contract gives none."""
    good = in_contract(rec, len(octs))
    _count(census, "orient_records", rec.shape[0])
    _count(census, "orient_out_of_contract", (~good).sum())
    rec = rec[good]
    N = rec.shape[0]
    if N == 0:
        return np.zeros((0, 8), np.int32)
    _, _, _, x, y, sc = _fields(rec)
    h = (sc * f32(4.5)) * f32(0.125)
    off = (np.arange(19) - 9).astype(f32)

    def pos(sel):
        px = x[sel, None, None] + off[None, None, :] * h[sel, None, None]
        py = y[sel, None, None] + off[None, :, None] * h[sel, None, None]
        return np.broadcast_arrays(px, py)

    P = _patches(octs, rec, 19, pos)
    gx = P[:, 1:18, 2:19] - P[:, 1:18, 0:17]
    gy = P[:, 2:19, 1:18] - P[:, 0:17, 1:18]
    w = np.sqrt(gx * gx + gy * gy) * tb["wo"][None]
    b = np.minimum(np.floor(turn(gy, gx) * f32(36)).astype(np.int64), 35)
    iw = np.rint(np.fmin(w * f32(1024), f32(4194304))).astype(np.int64)
    hist = np.bincount((np.arange(N)[:, None, None] * 36 + b).ravel(), weights=iw.ravel().astype(np.float64),
                       minlength=N * 36).reshape(N, 36)
    assert hist.max() < 2 ** 31
    hs = hist.astype(np.int32).astype(f32)
    for _ in range(2):
        hs = (np.roll(hs, 1, 1) + np.roll(hs, -1, 1)) * f32(0.25) + hs * f32(0.5)
    lf, rt = np.roll(hs, 1, 1), np.roll(hs, -1, 1)
    M = hs.max(1, keepdims=True)
    peak = (hs > lf) & (hs > rt) & (hs >= f32(0.8) * M)
    with np.errstate(all="ignore"):
        bf = (np.arange(36).astype(f32)[None] + f32(0.5)) + f32(0.5) * (lf - rt) / ((lf - f32(2) * hs) + rt)
        qr = np.where(peak, np.rint((bf * f32(1024)) / f32(36)), 0).astype(np.int64)
        q = qr % 1024
    if census is not None:
        npk = peak.sum(1)
        for k in range(5):
            _count(census, "peaks_%d" % k, (npk == k).sum())
        _count(census, "peaks_above_4", (npk > 4).sum())
        _count(census, "peak_in_bin_0", peak[:, 0].sum())
        _count(census, "peak_in_bin_35", peak[:, 35].sum())
        _count(census, "q_wrap", (peak & (qr != q)).sum())
        _count(census, "hist_term_at_bound", (w * f32(1024) >= f32(4194304)).sum())
        _count(census, "oriented", np.minimum(npk, 4).sum())
    sel = np.argwhere(peak & (np.cumsum(peak, 1) <= 4))   # input order, then ascending bin
    out = rec[sel[:, 0]].copy()
    out[:, 1] = (out[:, 1] & 0xff) | (q[sel[:, 0], sel[:, 1]] << 8).astype(np.int32)
    return out


def describe(octs, orec, tb, census=None):
    """(M, 8) oriented records -> (M, 128) u8.  The row of a record outside the contract is zero."""
    good = in_contract(orec, len(octs))
    if not good.all():
        _count(census, "describe_out_of_contract", (~good).sum())
        out = np.zeros((orec.shape[0], 128), np.uint8)
        out[good] = describe(octs, orec[good], tb, census)
        return out
    M = orec.shape[0]
    _count(census, "describe_rows", M)
    if M == 0:
        return np.zeros((0, 128), np.uint8)
    _, _, q, x, y, sc = _fields(orec)
    c, s = tb["cs"][q, 0], tb["cs"][q, 1]
    h = (sc * f32(12)) * f32(0.0625)
    uv = np.arange(18).astype(f32) - f32(8.5)

    def pos(sel):
        u, v = uv[None, None, :], uv[None, :, None]
        cc, ss, hh = c[sel, None, None], s[sel, None, None], h[sel, None, None]
        px = x[sel, None, None] + ((u * cc) - (v * ss)) * hh
        py = y[sel, None, None] + ((u * ss) + (v * cc)) * hh
        return px, py

    P = _patches(octs, orec, 18, pos)
    gx = P[:, 1:17, 2:18] - P[:, 1:17, 0:16]
    gy = P[:, 2:18, 1:17] - P[:, 0:16, 1:17]
    m = np.sqrt(gx * gx + gy * gy) * tb["wd"][None]
    ob = turn(gy, gx) * f32(8)
    f0 = np.floor(ob)
    fo = ob - f0
    o0 = f0.astype(np.int64) & 7
    cw = tb["cw"]
    d = np.zeros((M, 4, 4, 8), f32)
    rows = np.arange(M)
    for a in range(16):
        for b in range(16):
            wgt = np.zeros((M, 8), f32)
            wgt[rows, o0[:, a, b]] = f32(1) - fo[:, a, b]
            wgt[rows, (o0[:, a, b] + 1) & 7] = fo[:, a, b]
            t = (m[:, a, b, None] * cw[None, :, a])[:, :, None] * cw[None, None, :, b]
            d = d + t[:, :, :, None] * wgt[:, None, None, :]
    d = d.reshape(M, 128)

    def norm(e):
        acc = np.zeros(M, f32)
        for k in range(128):
            acc = acc + e[:, k] * e[:, k]
        return np.sqrt(acc)

    n = norm(d)
    ok = n > 0
    with np.errstate(all="ignore"):
        e = np.minimum(d / n[:, None], f32(0.2))
        e = np.where(ok[:, None], e, f32(0))
        n2 = norm(e)
        r = np.rint(f32(512) * (e / n2[:, None]))
        _count(census, "zero_norm", (~ok).sum())
        _count(census, "entry_clamped_255", (ok[:, None] & (r > f32(255))).sum())
        r = np.minimum(r, f32(255))
    return np.where(ok[:, None], r, 0).astype(np.uint8)


def sift(img, tb, O, border=5, contrast=0.04, edge=10.0):
    """All four stages of one view: pyramid (list), rec, orec, desc."""
    octs = pyramid(img, O, tb)
    rec = detect(octs, tb, border, contrast, edge)
    orec = orient(octs, rec, tb)
    return octs, rec, orec, describe(octs, orec, tb)
