"""torch-fp64 CPU restatement of scipy.ndimage.rotate(a, angle, axes=(-2, -1), reshape=False) (order 3, mode
'constant', cval 0, prefilter on) and of the reference's field / mask / error compositions
(src/equivariance_error_calculator.py), with no scipy.  tests/test_equivariance_host.py pins it to stored scipy
outputs; the GPU tests use it at sizes too large for a fixture."""
import math

import numpy as np
import torch

R = 27
_Z = math.sqrt(3.0) - 2.0


def fir_taps():
    h, out = -6.0 * _Z / (1.0 - _Z * _Z), []
    for _ in range(R + 1):
        out.append(h)
        h *= _Z
    return out


def mirror_index(i, n):
    """whole-sample symmetric extension a[-i] = a[i], period 2(n - 1); works on int tensors"""
    if n == 1:
        return torch.zeros_like(i)
    p = 2 * (n - 1)
    i = i.abs() % p
    return torch.where(i > n - 1, p - i, i)


def _filter_axis(a, dim):
    n = a.shape[dim]
    if n == 1:
        return a.clone()
    h = fir_taps()
    idx = torch.arange(n)
    out = h[0] * a
    for j in range(1, R + 1):
        out = out + h[j] * (a.index_select(dim, mirror_index(idx - j, n)) + a.index_select(dim, mirror_index(idx + j, n)))
    return out


def spline_coefficients(a):
    """cubic B-spline coefficients of every (y, x) plane (mirror boundary), fp64"""
    a = torch.as_tensor(a).double()
    return _filter_axis(_filter_axis(a, a.dim() - 2), a.dim() - 1)


def cos_sin_deg(angle):
    a = math.fmod(float(angle), 360.0)
    if a < 0:
        a += 360.0
    exact = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
    if a in exact:
        return exact[a]
    r = a * (math.pi / 180.0)
    return math.cos(r), math.sin(r)


def source_coords(angle, Y, X):
    """fp64 (cy, cx) of every output (oy, ox), (Y, X) each"""
    c, s = cos_sin_deg(angle)
    hy, hx = (Y - 1) / 2.0, (X - 1) / 2.0
    off_y, off_x = hy - (c * hy + s * hx), hx - (-s * hy + c * hx)
    oy = torch.arange(Y, dtype=torch.float64).view(Y, 1)
    ox = torch.arange(X, dtype=torch.float64).view(1, X)
    cy = (c * oy + s * ox) + off_y
    cx = (-s * oy + c * ox) + off_x
    return cy.expand(Y, X), cx.expand(Y, X)


def _weights(c):
    f = torch.floor(c)
    t = c - f
    u = 1.0 - t
    w = torch.stack([u * u * u / 6.0, (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0, (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0,
                     t * t * t / 6.0], -1)
    return f.long() - 1, w


def rotate_coefficients(coef, angle):
    """the spline of every (y, x) plane of ``coef`` sampled at the rotated grid; cval 0 outside"""
    Y, X = coef.shape[-2:]
    cy, cx = source_coords(angle, Y, X)
    inside = (cy >= 0) & (cy <= Y - 1) & (cx >= 0) & (cx <= X - 1)
    cyc, cxc = cy.clamp(0, Y - 1), cx.clamp(0, X - 1)
    sy, wy = _weights(cyc)
    sx, wx = _weights(cxc)
    flat = coef.reshape(-1, Y * X)
    out = torch.zeros(flat.shape[0], Y, X, dtype=torch.float64)
    for i in range(4):
        iy = mirror_index(sy + i, Y)
        for j in range(4):
            ix = mirror_index(sx + j, X)
            out += (wy[..., i] * wx[..., j]) * flat[:, (iy * X + ix).reshape(-1)].reshape(-1, Y, X)
    out = torch.where(inside, out, torch.zeros((), dtype=torch.float64))
    return out.reshape(coef.shape)


def rotate(a, angle):
    """scipy.ndimage.rotate(a, angle, axes=(-2, -1), reshape=False) in fp64"""
    return rotate_coefficients(spline_coefficients(a), angle)


def _ms(means, scales):
    m = torch.tensor(means, dtype=torch.float64).view(1, 4, 1, 1, 1)
    s = torch.tensor(scales, dtype=torch.float64).view(1, 4, 1, 1, 1)
    return m, s


def mix_velocity(v, angle):
    """the reference's channel matrix (cosdg / sindg here; np.cos(np.deg2rad) differs by ~1e-16)"""
    c, s = cos_sin_deg(angle)
    out = v.clone()
    out[:, 1] = c * v[:, 1] + s * v[:, 2]
    out[:, 2] = -s * v[:, 1] + c * v[:, 2]
    return out


def rotate_fields(x, means, scales, angle, rescaled=True):
    """rotate_temperature_velocity of the reference, fp64"""
    m, s = _ms(means, scales)
    v = mix_velocity(rotate(torch.as_tensor(x).double() * s + m, angle), angle)
    return ((v - m) / s).clamp(0.0, 1.0) if rescaled else v


def rotate_building(b, angle, th=0.1):
    v = rotate(b, angle).float()
    return (v > np.float32(th)).float()


def equivariance_errors(preds, preds_after_rot, means, scales, angle, sx, ex, sy, ey):
    """(tm, vr, vl_vp) of calc_equivariance_errors given the two predictions, fp64"""
    m, s = _ms(means, scales)
    rot = s * rotate_fields(preds, means, scales, angle) + m
    par = s * torch.as_tensor(preds_after_rot).double() + m
    d = (rot - par)[..., sy:ey, sx:ex]
    return (float(d[:, 0].abs().mean()), float(d[:, 3].abs().mean()),
            float(torch.sqrt(d[:, 1] ** 2 + d[:, 2] ** 2).mean()))
