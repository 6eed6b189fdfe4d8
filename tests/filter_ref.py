"""numpy restatement of the denoise chain (lighthouse2_amd/csrc/lh2_filter.hip): the checker of the filter tests.

Every function takes dt, the float type it computes in: np.float64 (the reference the kernels are compared with) or
np.float32 (the same operations in the kernels' precision, whose distance from float64 sets the tolerances).  The
operations and their order follow the kernels (fminf / fmaxf are np.fmin / np.fmax: a NaN operand loses), which follow
Lighthouse 2's prepareFilterKernel / applyFilterKernel.
Buffers are (h, w, words) arrays; packed ones (features, shading, the pass outputs) are uint32 words."""
from __future__ import annotations

import numpy as np

MISS_T = np.float32(1e34)
STEP = 1.0 / 2048.0          # one unit of the 5:11 fixed point the shading buffers are stored in


# ---- packed formats -------------------------------------------------------------------------
def f2u(x):
    """float -> uint32 as the kernels convert: truncation, NaN and negatives to 0."""
    return np.clip(np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=4294967040.0), 0.0, 4294967040.0).astype(np.uint32)


def pack_normal(n):
    n = np.asarray(n, np.float32)
    q = np.fmin(f2u((n + np.float32(1)) * np.float32(511)), 1023).astype(np.uint32)
    return (q[..., 0] << 2) + (q[..., 1] << 12) + (q[..., 2] << 22)


def unpack_normal(p, dt):
    p = np.asarray(p, np.uint32)
    k = dt(1) / dt(511)
    return np.stack([((p >> 2) & 1023).astype(dt) * k - dt(1), ((p >> 12) & 1023).astype(dt) * k - dt(1),
                     (p >> 22).astype(dt) * k - dt(1)], -1)


def pack_rgb(c):
    c = np.asarray(c, np.float32)
    one = np.float32(1)
    return (f2u(np.float32(1023) * np.fmin(one, c[..., 0])) << 22) + (f2u(np.float32(2047) * np.fmin(one, c[..., 1])) << 11) + \
        f2u(np.float32(2047) * np.fmin(one, c[..., 2]))


def unpack_rgb(c, dt, min1=False):
    c = np.asarray(c, np.uint32)
    r, g, b = c >> 22, (c >> 11) & 2047, c & 2047
    if min1:
        r, g, b = np.fmax(r, 1), np.fmax(g, 1), np.fmax(b, 1)
    return np.stack([r.astype(dt) * (dt(1) / dt(1023)), g.astype(dt) * (dt(1) / dt(2047)), b.astype(dt) * (dt(1) / dt(2047))], -1)


def combine(a, b, dt):
    """Two rgb triples -> (.., 4) uint32 words, 5:11 fixed point."""
    q = lambda v: f2u(np.fmin(v, dt(31.999)) * dt(2048))
    qa, qb = q(a), q(b)
    return np.stack([(qa[..., 0] << 16) + qa[..., 1], qa[..., 2], (qb[..., 0] << 16) + qb[..., 1], qb[..., 2]], -1).astype(np.uint32)


def direct_of(c, dt):
    c = np.asarray(c, np.uint32)
    k = dt(1) / dt(2048)
    return np.stack([(c[..., 0] >> 16).astype(dt) * k, (c[..., 0] & 65535).astype(dt) * k, c[..., 1].astype(dt) * k], -1)


def indirect_of(c, dt):
    c = np.asarray(c, np.uint32)
    k = dt(1) / dt(2048)
    return np.stack([(c[..., 2] >> 16).astype(dt) * k, (c[..., 2] & 65535).astype(dt) * k, c[..., 3].astype(dt) * k], -1)


def lum(c, dt):
    ten = dt(10)
    return dt(0.299) * np.fmin(c[..., 0], ten) + dt(0.587) * np.fmin(c[..., 1], ten) + dt(0.114) * np.fmin(c[..., 2], ten)


def rgb_to_ycocg(c, dt):
    r = np.fmin(dt(4), c)
    k = dt(0.5) * dt(256) / dt(255)
    q = dt(0.25)
    return np.stack([(r[..., 0] * dt(1) + r[..., 1] * dt(2) + r[..., 2] * dt(1)) * q,
                     (r[..., 0] * dt(2) + r[..., 1] * dt(0) + r[..., 2] * dt(-2)) * q + k,
                     (r[..., 0] * dt(-1) + r[..., 1] * dt(2) + r[..., 2] * dt(-1)) * q + k], -1)


def ycocg_to_rgb(c, dt):
    k = dt(0.5) * dt(256) / dt(255)
    Y, Co, Cg = c[..., 0], c[..., 1] - k, c[..., 2] - k
    return np.stack([Y + Co - Cg, Y + Cg, Y - Co - Cg], -1)


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the previous view ------------------------------------------------------------------------
def prev_view(view, h, dt=np.float32):
    """The reprojection constants of a view (pos, p1, p2, p3 as 3-vectors): computed in float32 on the host, as
    lh2_filter_prev_view does, whatever dt is; returned in dt."""
    f = np.float32
    pos, p1, p2, p3 = (np.asarray(v, f) for v in view)
    norm = lambda a: a * (f(1) / np.sqrt(dot(a, a), dtype=f))
    centre = f(0.5) * (p2 + p3)
    direction, right, up = norm(centre - pos), norm(p2 - p1), norm(p3 - p1)
    len_reci = f(h) / np.sqrt(dot(p3 - p1, p3 - p1), dtype=f)
    out = dict(pos=np.append(pos, -(dot(pos, direction) - dot(centre, direction))), E=np.append(direction, f(0)),
               right=np.append(right * len_reci, dot(p1, right) * len_reci), up=np.append(up * len_reci, dot(p1, up) * len_reci))
    return {k: np.asarray(v, f).astype(dt) for k, v in out.items()}


def view_tuple(v):
    """(pos, p1, p2, p3) of an abi.ViewPyramid."""
    g = lambda a: np.array([a.x, a.y, a.z], np.float32)
    return g(v.pos), g(v.p1), g(v.p2), g(v.p3)


# ---- history lookup ------------------------------------------------------------------------------
def history_taps(prevWorldPos, local_bits, local_normal, min_dot, u, v, dt):
    """Indices (4, h, w) and weights (4, h, w) of the bilinear taps around (u, v), and the mask of pixels inside."""
    h, w = u.shape
    fu, fv = np.floor(u), np.floor(v)
    with np.errstate(invalid="ignore"):
        iu1 = np.nan_to_num(fu, nan=-1.0).clip(-2, 1 << 20).astype(np.int64)
        iv1 = np.nan_to_num(fv, nan=-1.0).clip(-2, 1 << 20).astype(np.int64)
    inside = (iu1 < w) & (iv1 < h) & (iu1 >= 0) & (iv1 >= 0)
    iu1c, iv1c = np.clip(iu1, 0, w - 1), np.clip(iv1, 0, h - 1)
    iu0, iv0 = np.fmax(0, iu1c - 1), np.fmax(0, iv1c - 1)
    fx, fy = u - fu, v - fv
    one = dt(1)
    w0, w1, w2 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy
    w3 = one - (w0 + w1 + w2)
    idx = np.stack([iu0 + iv0 * w, iu1c + iv0 * w, iu0 + iv1c * w, iu1c + iv1c * w])
    wts = np.stack([w0, w1, w2, w3])
    nbits = fbits(prevWorldPos[..., 3]).reshape(-1)
    spec = local_bits & 3
    for k in range(4):
        nb = nbits[idx[k]]
        bad = (dot(unpack_normal(nb, dt), local_normal) < dt(min_dot)) | ((nb & 3) != spec)
        wts[k] = np.where(bad, dt(0), wts[k])
    return idx, wts, inside


def _world_distance(px, py, cur, prevWorldPos, dt):
    h, w = prevWorldPos.shape[:2]
    if 0 <= px < w and 0 <= py < h:
        p = prevWorldPos[py, px, :3].astype(dt)
        pb = int(fbits(prevWorldPos[py, px, 3:4])[0])
    else:
        p, pb = np.array([1e20, 1e20, 1e20], dt), 0
    if (pb & 3) != 1:
        return dt(1e21)
    if dot(unpack_normal(np.uint32(cur[4]), dt), unpack_normal(np.uint32(pb), dt)) < dt(0.85):
        return dt(1e21)
    d = cur[:3] - p[:3]
    return np.sqrt(dot(d, d))


def _fine_world_distance(px, py, cur, prevWorldPos, dt):
    x0, y0 = int(px), int(py)
    fx, fy = px - np.floor(px), py - np.floor(py)
    one = dt(1)
    ws = [(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy]
    ds = [_world_distance(x0 + dx, y0 + dy, cur, prevWorldPos, dt) for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))]
    tw, td = dt(0), dt(0)
    for d, wt in zip(ds, ws):
        if d < dt(1e20):
            td, tw = td + d * wt, tw + wt
    return dt(1e20) if tw == 0 else td / tw


def _diamond_search(x, y, cur, prevWorldPos, dt):
    """The specular pixels' search for their previous position (one pixel, scalar)."""
    ppx, ppy = dt(x), dt(y)
    d0 = cur[:3] - prevWorldPos[y, x, :3].astype(dt)
    best, step = np.sqrt(dot(d0, d0)), dt(5)
    for _ in range(25):
        cx, cy, tap = ppx, ppy, 0
        for k, (ox, oy) in enumerate(((-step, 0), (step, 0), (0, -step), (0, step))):
            d = _fine_world_distance(cx + dt(ox), cy + dt(oy), cur, prevWorldPos, dt)
            if d < best:
                best, ppx, ppy, tap = d, cx + dt(ox), cy + dt(oy), k + 1
        if tap == 0:
            step = step * dt(0.45)
            if step < dt(0.05):
                break
    return ppx, ppy


# ---- prepare ---------------------------------------------------------------------------------------
def view_project(v, wp, dt):
    """World positions (h, w, 3) on the screen of a view (prev_view(..)), in pixels from its top-left corner."""
    pos, E, R, U = (v[k].astype(dt) for k in ("pos", "E", "right", "up"))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = wp - pos[:3]
        D = d * (dt(1) / np.sqrt(dot(d, d)))[..., None]
        t = pos[3] / dot(E[None, None, :3], D)
        S = pos[:3] + D * t[..., None]
        return dot(S, R[None, None, :3]) - R[3], dot(S, U[None, None, :3]) - U[3]


def prepare(acc, features, worldPos, prevWorldPos, deltaDepth, prevMoments, pview, cview, dt=np.float64, scale=1.0, clamp_direct=2.5,
            clamp_indirect=15.0, cam_stationary=True, history_valid=True):
    """k_filter_prepare.  acc: (2, h, w, 4); pview, cview: prev_view(..) of the previous and the current view.  Returns shading (packed), direct / indirect (before
    packing), motion, moments, features (history count updated) and found (the pixel has history)."""
    features = np.asarray(features, np.uint32)
    h, w = features.shape[:2]
    wp = np.asarray(worldPos, np.float32)
    albedo = unpack_rgb(features[..., 0], dt, min1=True)
    direct = acc[0][..., :3].astype(dt) * dt(scale)
    indirect = acc[1][..., :3].astype(dt) * dt(scale)
    reci = dt(1) / albedo
    dl = np.fmin(direct * reci, dt(clamp_direct))
    il = np.fmin(indirect * reci, dt(clamp_indirect))
    shading = combine(dl, il, dt)
    l_d, l_i = lum(dl, dt), lum(il, dt)
    l_d2, l_i2 = l_d * l_d, l_i * l_i
    # reprojection
    ys, xs = np.mgrid[0:h, 0:w]
    px0, py0 = view_project(pview, wp[..., :3].astype(dt), dt)
    px1, py1 = view_project(cview, wp[..., :3].astype(dt), dt)
    ppx, ppy = xs.astype(dt) + (px0 - px1), ys.astype(dt) + (py0 - py1)
    specular = ((features[..., 3] >> 4) & 3) != 0
    ppx = np.where(specular, xs.astype(dt), ppx)
    ppy = np.where(specular, ys.astype(dt), ppy)
    if not cam_stationary and history_valid:
        pw = np.asarray(prevWorldPos, np.float32)
        wbits = fbits(wp[..., 3])
        for y, x in zip(*np.nonzero(specular)):
            ppx[y, x], ppy[y, x] = _diamond_search(int(x), int(y), _Cur(wp[y, x, :3].astype(dt), int(wbits[y, x])), pw, dt)
    ppx, ppy = ppx + dt(0.5), ppy + dt(0.5)
    # history
    found = np.zeros((h, w), bool)
    if history_valid:
        with np.errstate(invalid="ignore"):
            ok = (ppx >= 0) & (ppx < w) & (ppy >= 0) & (ppy < h)
        idx, wts, inside = history_taps(np.asarray(prevWorldPos, np.float32), fbits(wp[..., 3]), unpack_normal(features[..., 1], dt), 0.95,
                                        np.where(ok, ppx, dt(0)), np.where(ok, ppy, dt(0)), dt)
        s = wts[0] + wts[1] + wts[2] + wts[3]
        pm = np.asarray(prevMoments, np.float32).reshape(-1, 4).astype(dt)
        with np.errstate(invalid="ignore", divide="ignore"):
            rs = dt(1) / s
            hist = (wts[0][..., None] * pm[idx[0]] + wts[1][..., None] * pm[idx[1]] + wts[2][..., None] * pm[idx[2]] +
                    wts[3][..., None] * pm[idx[3]]) * rs[..., None]
            found = ok & inside & (s != 0) & (hist[..., 0] > -1)
        a, b = dt(0.2), dt(0.8)
        l_d = np.where(found, a * l_d + b * hist[..., 0], l_d)
        l_d2 = np.where(found, a * l_d2 + b * hist[..., 1], l_d2)
        l_i = np.where(found, a * l_i + b * hist[..., 2], l_i)
        l_i2 = np.where(found, a * l_i2 + b * hist[..., 3], l_i2)
    fw = features[..., 3].copy()
    cnt = fw & 15
    fw = np.where(found, np.where(cnt < 15, fw + 1, fw), fw & 0xfffffff0).astype(np.uint32)
    out_features = features.copy()
    out_features[..., 3] = fw
    return dict(shading=shading, direct=dl, indirect=il, motion=np.stack([ppx, ppy], -1), moments=np.stack([l_d, l_d2, l_i, l_i2], -1),
                features=out_features, found=found)


class _Cur:
    """A pixel's world position and packed-normal bits for the diamond search (indexable like the scalar helpers expect)."""
    def __init__(self, p, bits):
        self.p, self.bits = p, bits

    def __getitem__(self, k):
        if isinstance(k, slice):
            return self.p[k]
        return self.bits if k == 4 else self.p[k]


# ---- the a-trous passes --------------------------------------------------------------------------------
TAPS = [(uu, vv) for vv in range(-2, 3) for uu in range(-(1 if abs(vv) == 2 else 2), (1 if abs(vv) == 2 else 2) + 1) if uu or vv]


def pow128(x):
    for _ in range(7):
        x = x * x
    return x


def atrous(phase, features, worldPos, prevWorldPos, deltaDepth, motion, moments, A, B=None, dt=np.float64, history_valid=True):
    """k_filter_atrous<phase>.  Returns out (packed words for phases 1 and 2, radiance (h, w, 4) for phase 3), direct /
    indirect (the filtered light before packing or remodulation) and finite (h, w, 20, 2): which tap weights were finite."""
    features = np.asarray(features, np.uint32)
    A = np.asarray(A, np.uint32)
    h, w = features.shape[:2]
    step = 1 << (phase - 1)
    ys, xs = np.mgrid[0:h, 0:w]
    l_normal = unpack_normal(features[..., 1], dt)
    l_color = unpack_rgb(features[..., 0], dt)
    l_mat = features[..., 3] >> 4
    d_sum, i_sum = direct_of(A, dt), indirect_of(A, dt)
    d_w, i_w = np.ones((h, w), dt), np.ones((h, w), dt)
    l_dir, l_ind = lum(d_sum, dt), lum(i_sum, dt)
    l_depth = features[..., 2].view(np.float32).astype(dt)
    dd = np.asarray(deltaDepth, np.float32)
    ddx, ddy = dd[..., 2].astype(dt), dd[..., 3].astype(dt)
    m = np.asarray(moments, np.float32).astype(dt)
    sigma = dt(10) * dt(2.0 ** -(phase - 1))
    factor = np.where((features[..., 3] & 15) == 0, dt(400), dt(1))
    eps = dt(0.00001)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        var_d, var_i = m[..., 1] - m[..., 0] * m[..., 0], m[..., 3] - m[..., 2] * m[..., 2]
        reci_d = dt(-1) / (sigma * factor * np.sqrt(var_d + eps) + eps)
        reci_i = dt(-1) / (sigma * factor * np.sqrt(var_i + eps) + eps)
        depth_scale = dt(0.5) + dt(phase) * dt(0.5)
        finite = np.ones((h, w, len(TAPS), 2), bool)
        for k, (uu, vv) in enumerate(TAPS):
            v = vv * step + ys
            valid = (v >= 0) & (v < h)
            u = np.clip(uu * step + xs, 0, w - 1)
            vc = np.clip(v, 0, h - 1)
            nc, nf = A[vc, u], features[vc, u]
            w_dist = dt(uu * uu + vv * vv) * (dt(-1) / dt(7.5))
            n_d, n_i = direct_of(nc, dt), indirect_of(nc, dt)
            w_n = pow128(np.fmax(dt(0), dot(unpack_normal(nf[..., 1], dt), l_normal)))
            expected = l_depth + ddx * dt(uu * step) + ddy * dt(vv * step)
            depth_err = np.abs(expected - nf[..., 2].view(np.float32).astype(dt))
            expected_diff = np.abs(expected - l_depth)
            w_depth = depth_err / np.fmax(eps, depth_scale * expected_diff)
            w_n = w_n * np.where((nf[..., 3] >> 4) != l_mat, dt(0.0001), dot(l_color, unpack_rgb(nf[..., 0], dt)))
            w_d = w_n * np.exp(np.abs(l_dir - lum(n_d, dt)) * reci_d + w_dist - w_depth)
            w_i = w_n * np.exp(np.abs(l_ind - lum(n_i, dt)) * reci_i + w_dist - w_depth)
            fd, fi = np.isfinite(w_d), np.isfinite(w_i)
            finite[..., k, 0], finite[..., k, 1] = fd | ~valid, fi | ~valid
            w_d = np.where(fd & valid, w_d, dt(0))
            w_i = np.where(fi & valid, w_i, dt(0))
            d_sum, d_w = d_sum + n_d * w_d[..., None], d_w + w_d
            i_sum, i_w = i_sum + n_i * w_i[..., None], i_w + w_i
        d_f = d_sum * (dt(1) / np.fmax(dt(0.0001), d_w))[..., None]
        i_f = i_sum * (dt(1) / np.fmax(dt(0.0001), i_w))[..., None]
        if phase == 1 and history_valid:
            mo = np.asarray(motion, np.float32)
            mx, my = mo[..., 0].astype(dt), mo[..., 1].astype(dt)
            px = np.trunc(np.nan_to_num(mx, nan=0.0)).astype(np.int64)
            py = np.trunc(np.nan_to_num(my, nan=0.0)).astype(np.int64)
            ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            wp = np.asarray(worldPos, np.float32)
            idx, wts, inside = history_taps(np.asarray(prevWorldPos, np.float32), fbits(wp[..., 3]), l_normal, 0.975,
                                            np.where(ok, mx, dt(0)), np.where(ok, my, dt(0)), dt)
            s = wts[0] + wts[1] + wts[2] + wts[3]
            Bf = np.asarray(B, np.uint32).reshape(-1, 4)
            rs = dt(1) / s
            p_d = (wts[0][..., None] * direct_of(Bf[idx[0]], dt) + wts[1][..., None] * direct_of(Bf[idx[1]], dt) +
                   wts[2][..., None] * direct_of(Bf[idx[2]], dt) + wts[3][..., None] * direct_of(Bf[idx[3]], dt)) * rs[..., None]
            p_i = (wts[0][..., None] * indirect_of(Bf[idx[0]], dt) + wts[1][..., None] * indirect_of(Bf[idx[1]], dt) +
                   wts[2][..., None] * indirect_of(Bf[idx[2]], dt) + wts[3][..., None] * indirect_of(Bf[idx[3]], dt)) * rs[..., None]
            use = ok & inside & (s != 0) & (p_d[..., 0] != -1)
            p_d, p_i = rgb_to_ycocg(p_d, dt), rgb_to_ycocg(p_i, dt)
            d_avg, i_avg = rgb_to_ycocg(d_f, dt), rgb_to_ycocg(i_f, dt)
            d_var, i_var = d_avg * d_avg, i_avg * i_avg
            Ad, Ai = rgb_to_ycocg(direct_of(A, dt), dt), rgb_to_ycocg(indirect_of(A, dt), dt)
            xl, xh, yl, yh = xs > 1, xs < w - 1, ys > 1, ys < h - 1      # the reference's bounds
            order = [(-1, -1, xl & yl), (-1, 0, xl), (-1, 1, xl & yh), (0, -1, yl), (0, 1, yh), (1, -1, xh & yl), (1, 0, xh), (1, 1, xh & yh)]
            for dx, dy, cond in order:
                f = Ad[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]
                g = Ai[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]
                c = cond[..., None]
                d_avg, d_var = np.where(c, d_avg + f, d_avg), np.where(c, d_var + f * f, d_var)
                i_avg, i_var = np.where(c, i_avg + g, i_avg), np.where(c, i_var + g * g, i_var)
            k9 = dt(1) / dt(9)
            d_avg, d_var, i_avg, i_var = d_avg * k9, d_var * k9, i_avg * k9, i_var * k9
            s_d = np.sqrt(np.fmax(dt(0), d_var - d_avg * d_avg))
            s_i = np.sqrt(np.fmax(dt(0), i_var - i_avg * i_avg))
            q = dt(0.75)
            p_d = np.fmin(np.fmax(p_d, d_avg - q * s_d), d_avg + q * s_d)
            p_i = np.fmin(np.fmax(p_i, i_avg - q * s_i), i_avg + q * s_i)
            d_b = d_f * dt(0.1) + ycocg_to_rgb(p_d, dt) * dt(0.9)
            i_b = i_f * dt(0.1) + ycocg_to_rgb(p_i, dt) * dt(0.9)
            d_f, i_f = np.where(use[..., None], d_b, d_f), np.where(use[..., None], i_b, i_f)
        if phase == 3:
            rgb = (d_f + i_f) * l_color
            out = np.concatenate([rgb, np.ones((h, w, 1), dt)], -1)
        else:
            out = combine(d_f, i_f, dt)
    return dict(out=out, direct=d_f, indirect=i_f, finite=finite)


def unpacked(words, dt=np.float64):
    """A packed shading buffer as (h, w, 6) floats: direct rgb, indirect rgb."""
    return np.concatenate([direct_of(words, dt), indirect_of(words, dt)], -1)


def rel_max(a, b):
    """The largest difference of a from b, relative to b's largest magnitude (nan where both are nan)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    return float(np.max(d) / max(float(np.nanmax(np.abs(b))), 1e-30))
