"""numpy restatement of the TAA stage (lighthouse2_amd/csrc/lh2_filter.hip: k_filter_taa, k_filter_unsharpen): the checker
of the TAA tests.

As in tests/filter_ref.py every function takes dt, the float type it computes in: np.float64 (the reference) or
np.float32 (the same operations in the kernels' precision, whose distance from float64 sets the tolerances).  The
operations and their order follow the kernels, which follow Lighthouse 2's TAApassKernel / unsharpenTAAKernel
(finalize_shared.h) with ReadTexelBmitchellNetravali / mitchellNetravali (sampling_shared.h), but for four things:
  1. the pass writes a buffer of its own (the reference works in place, reading neighbours other threads overwrite);
  2. the bicubic footprint is the kernel's support, floor(u) - 1 .. floor(u) + 2 per axis, taps outside the frame skipped
     and the weights renormalised (the reference starts at (int)(u - 2) and skips row 0);
  3. a frame without history passes through (the reference reads whatever its history buffer holds);
  4. the frame's border pixels get their TAA pixel squared, without the sharpening (the reference leaves them unwritten);
and a fifth the kernel needs for the reference's NaN fallback to do its work: the history's own sum is tested for NaN as
well as the blend's, because rgb_to_ycocg's fmin( 4, . ) turns a NaN history into 4 before the blend could show it.
Buffers are (h, w, words) arrays."""
from __future__ import annotations

import numpy as np

from filter_ref import rgb_to_ycocg, ycocg_to_rgb


def mitchell_netravali(v, dt):
    """mitchellNetravali with B = C = 1/3."""
    B = C = dt(1) / dt(3)
    x = np.abs(v)
    x2 = x * x
    x3 = x2 * x
    near = (dt(1) / dt(6)) * ((dt(12) - dt(9) * B - dt(6) * C) * x3 + (dt(-18) + dt(12) * B + dt(6) * C) * x2 + (dt(6) - dt(2) * B))
    far = (dt(1) / dt(6)) * ((-B - dt(6) * C) * x3 + (dt(6) * B + dt(30) * C) * x2 + (dt(-12) * B - dt(48) * C) * x + (dt(8) * B + dt(24) * C))
    return np.where(x < 1, near, np.where(x < 2, far, dt(0)))


def taa_pass(linear, prev, motion, history_valid=True, dt=np.float64):
    """k_filter_taa.  linear: the last a-trous pass's output (h, w, 4); prev: the previous frame's TAA pixels; motion
    (h, w, 2).  Returns out (h, w, 4) in dt (w = 0) and the decisions: inside (the pixel blends with its history; the others
    pass through) and fallback (its blend summed to NaN, so it took ycocg_to_rgb( rgb_to_ycocg( g ) ))."""
    lin = np.asarray(linear, np.float32).astype(dt)
    pv = np.asarray(prev, np.float32).astype(dt)
    mo = np.asarray(motion, np.float32).astype(dt)
    h, w = lin.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = np.sqrt(lin[..., :3])
        new = rgb_to_ycocg(g, dt)
        u, v = mo[..., 0] - dt(0.5), mo[..., 1] - dt(0.5)
        inside = (u >= 0) & (u < dt(w)) & (v >= 0) & (v < dt(h)) & bool(history_valid)
        us, vs = np.where(inside, u, dt(0)), np.where(inside, v, dt(0))
        # the history: Mitchell-Netravali over the kernel's support, rows outermost
        x1, y1 = np.floor(us).astype(np.int64) - 1, np.floor(vs).astype(np.int64) - 1
        wx = [mitchell_netravali((x1 + i).astype(dt) - us, dt) for i in range(4)]
        wy = [mitchell_netravali((y1 + j).astype(dt) - vs, dt) for j in range(4)]
        total, total_w = np.zeros((h, w, 3), dt), np.zeros((h, w), dt)
        for j in range(4):
            ty = y1 + j
            for i in range(4):
                tx = x1 + i
                ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                weight = wx[i] * wy[j]
                tap = pv[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1), :3]
                total = np.where(ok[..., None], total + tap * weight[..., None], total)
                total_w = np.where(ok, total_w + weight, total_w)
        history_rgb = total * (dt(1) / total_w)[..., None]
        history = rgb_to_ycocg(history_rgb, dt)
        # this frame's 3 x 3 neighbourhood in YCoCg (the reference's bounds; / 9 whatever the count)
        avg, var = new, new * new
        xl, xh, yl, yh = xs > 1, xs < w - 1, ys > 1, ys < h - 1
        order = [(-1, -1, xl & yl), (-1, 0, xl), (-1, 1, xl & yh), (0, -1, yl), (0, 1, yh), (1, -1, xh & yl), (1, 0, xh), (1, 1, xh & yh)]
        for dx, dy, cond in order:
            f = new[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]
            c = cond[..., None]
            avg, var = np.where(c, avg + f, avg), np.where(c, var + f * f, var)
        k9 = dt(1) / dt(9)
        avg, var = avg * k9, var * k9
        sigma = np.sqrt(np.fmax(dt(0), var - avg * avg))
        q = dt(1.25)
        history = np.fmin(np.fmax(history, avg - q * sigma), avg + q * sigma)
        blend = ycocg_to_rgb(new * dt(0.1) + history * dt(0.9), dt)
        s = blend[..., 0] + blend[..., 1] + blend[..., 2]
        hs = history_rgb[..., 0] + history_rgb[..., 1] + history_rgb[..., 2]
        fallback = inside & (np.isnan(s) | np.isnan(hs))
        blend = np.where(fallback[..., None], ycocg_to_rgb(new, dt), blend)
        pixel = np.where(inside[..., None], blend, g)
        out = np.concatenate([np.fmin(dt(10), pixel), np.zeros((h, w, 1), dt)], -1)
    return dict(out=out, inside=inside, fallback=fallback)


def unsharpen(taa, dt=np.float64):
    """k_filter_unsharpen: the frame (h, w, 4) in dt (linear radiance, w = 1) from the TAA pass's pixels."""
    p = np.asarray(taa, np.float32).astype(dt)[..., :3]
    h, w = p.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    interior = (xs > 0) & (ys > 0) & (xs < w - 1) & (ys < h - 1)
    at = lambda dx, dy: p[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = dt(0.35), dt(0.5)
        ring = a * at(-1, -1) + b * at(0, -1)
        for k, (dx, dy) in ((a, (1, -1)), (b, (1, 0)), (a, (1, 1)), (b, (0, 1)), (a, (-1, 1)), (b, (-1, 0))):
            ring = ring + k * at(dx, dy)
        sharp = np.fmax(p, p * dt(2.7) - dt(0.5) * ring)
        pixel = np.where(interior[..., None], sharp, p)
        out = np.concatenate([pixel * pixel, np.ones((h, w, 1), dt)], -1)
    return out
