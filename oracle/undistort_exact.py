"""The undistorted pixel of one raw-image pixel in 50-digit arithmetic (mpmath): what oracle/undistort.py and k_undistort are held to.

TEST INFRASTRUCTURE ONLY (see oracle/snowtri_oracle.c header for the rules).

Written from the model in the header of oracle/undistort.py (OpenCV's 5-coefficient Brown-Conrady), formed in mpmath from the fp64
VALUES of K, D and the pixel:

    forward:  y = (v - cy) / fy,  x = (u - cx - s y) / fx,  (x_d, y_d) = distort(x, y),  (u_d, v_d) = (fx x_d + s y_d + cx, fy y_d + cy)
    inverse:  (x_d, y_d) from the raw pixel the same way, Newton on distort(x, y) = (x_d, y_d) from (x, y) = (x_d, y_d) until the
              step is below 1e-40 (quadratic convergence: the error left is ~1e-80, below the 50 digits carried), then K.

`forward_exact(exact_inverse(p))` = p to ~1e-45 px is what makes this an inverse, not a second iteration that agrees with the first;
tests/test_undistort_host.py asserts it on every case.
"""
import mpmath as mp
import numpy as np

DIGITS = 50
STEP = mp.mpf(10) ** -40
MAX_STEPS = 200


def _lens(K, D):
    K = np.asarray(K, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    assert K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1 and D.size >= 5
    return [mp.mpf(float(v)) for v in (K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2])], [mp.mpf(float(v)) for v in D[:5]]


def _distort(x, y, D):
    """-> (x_d, y_d, a, b, d): the distorted point and its Jacobian [[a, b], [b, d]] (symmetric)."""
    k1, k2, p1, p2, k3 = D
    r2 = x * x + y * y
    rho = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    drho = k1 + r2 * (2 * k2 + 3 * r2 * k3)                     # d rho / d r2
    xd = x * rho + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rho + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    a = rho + 2 * x * x * drho + 2 * p1 * y + 6 * p2 * x
    b = 2 * x * y * drho + 2 * p1 * x + 2 * p2 * y
    d = rho + 2 * y * y * drho + 6 * p1 * y + 2 * p2 * x
    return xd, yd, a, b, d


def forward_exact_mp(K, D, u, v):
    """Undistorted pixel (u, v: anything mp.mpf takes) -> the raw-image pixel as two mpf."""
    with mp.workdps(DIGITS):
        (fx, s, cx, fy, cy), Dm = _lens(K, D)
        y = (mp.mpf(v) - cy) / fy
        x = (mp.mpf(u) - cx - s * y) / fx
        xd, yd, _, _, _ = _distort(x, y, Dm)
        return fx * xd + s * yd + cx, fy * yd + cy


def exact_inverse_mp(K, D, u, v):
    """Raw-image pixel -> the undistorted pixel as two mpf.  A non-finite pixel, or one no Newton sequence from the raw point
    reaches (outside the lens's invertible region), raises ValueError."""
    with mp.workdps(DIGITS):
        (fx, s, cx, fy, cy), Dm = _lens(K, D)
        u, v = mp.mpf(u), mp.mpf(v)
        if not (mp.isfinite(u) and mp.isfinite(v)):
            raise ValueError("non-finite pixel")
        yd = (v - cy) / fy
        xd = (u - cx - s * yd) / fx
        x, y = xd, yd
        for _ in range(MAX_STEPS):
            gx, gy, a, b, d = _distort(x, y, Dm)
            f1, f2 = gx - xd, gy - yd
            det = a * d - b * b
            dx, dy = (d * f1 - b * f2) / det, (a * f2 - b * f1) / det
            x, y = x - dx, y - dy
            if max(abs(dx), abs(dy)) < STEP:
                return fx * x + s * y + cx, fy * y + cy
        raise ValueError(f"Newton did not converge from the raw pixel ({u}, {v})")


def _map(fn, K, D, uv):
    uv = np.asarray(uv, dtype=np.float64)
    flat = uv.reshape(-1, 2)
    out = np.empty_like(flat)
    for i, (u, v) in enumerate(flat):
        a, b = fn(K, D, float(u), float(v))
        out[i] = float(a), float(b)
    return out.reshape(uv.shape)


def forward_exact(K, D, uv):
    """uv [..., 2] fp64 undistorted pixels -> raw pixels, each the exact value rounded once to fp64."""
    return _map(forward_exact_mp, K, D, uv)


def exact_inverse(K, D, uv):
    """uv [..., 2] fp64 raw pixels -> undistorted pixels, each the exact value rounded once to fp64."""
    return _map(exact_inverse_mp, K, D, uv)


def jacobian_min_eig(K, D, uv):
    """Smallest eigenvalue of the forward model's Jacobian in normalised coordinates at the undistorted pixels uv [..., 2]
    (fp64 is plenty: a conditioning figure).  Newton inverts where it stays positive."""
    K = np.asarray(K, dtype=np.float64)
    k1, k2, p1, p2, k3 = [float(v) for v in np.asarray(D, dtype=np.float64).reshape(-1)[:5]]
    uv = np.asarray(uv, dtype=np.float64)
    y = (uv[..., 1] - K[1, 2]) / K[1, 1]
    x = (uv[..., 0] - K[0, 2] - K[0, 1] * y) / K[0, 0]
    r2 = x * x + y * y
    rho = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    drho = k1 + r2 * (2 * k2 + 3 * r2 * k3)
    a = rho + 2 * x * x * drho + 2 * p1 * y + 6 * p2 * x
    b = 2 * x * y * drho + 2 * p1 * x + 2 * p2 * y
    d = rho + 2 * y * y * drho + 6 * p1 * y + 2 * p2 * x
    return 0.5 * (a + d) - np.sqrt(0.25 * (a - d) ** 2 + b * b)
