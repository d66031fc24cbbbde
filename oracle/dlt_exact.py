"""The DLT point of one set of observations in 50-digit arithmetic (mpmath): what oracle/dlt.py and the kernels are held to.

TEST INFRASTRUCTURE ONLY (see oracle/snowtri_oracle.c header for the rules).

Everything is formed in mpmath from the fp64 VALUES of K, R, t and the pixels: the rig frame (c, s) of oracle/dlt.py's
definition, P'_c = K_c [R_c^T | -R_c^T (t_c - c) / s], the rows u P'[2] - P'[0], v P'[2] - P'[1], A^T A, its eigenvectors
(mp.eigsy), X = c + s e[:3] / e[3] of the smallest.  An ulp of difference between this c, s and the fp64 ones moves the answer
by ~1e-21 s, so they need not be rounded the way the library rounds them.

frame="world" solves the OLD definition (P = K [R^T | -R^T t], no centring) exactly: tests use it to record how far the
exact answer itself moves with the world's origin and unit, and how far fp64 A^T A in world coordinates is from it.
"""
import mpmath as mp
import numpy as np

DIGITS = 50


def _m(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a.reshape(a.shape[0], -1)])


def rig_frame_exact(t):
    """-> (c [3 mpf], s mpf) of the definition, in mpmath."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    C = t.shape[0]
    c = [mp.fsum(mp.mpf(float(t[k, a])) for k in range(C)) / C for a in range(3)]
    s = max(abs(mp.mpf(float(t[k, a])) - c[a]) for k in range(C) for a in range(3))
    return c, (s if s > 0 else mp.mpf(1))


def projection_matrices_exact(K, R, t, frame="rig"):
    """-> (list of 3x4 mp.matrix, c, s); frame="world": c = 0, s = 1."""
    K, R = np.asarray(K, dtype=np.float64), np.asarray(R, dtype=np.float64)
    C = K.shape[0]
    t = np.asarray(t, dtype=np.float64).reshape(C, 3)
    with mp.workdps(DIGITS):
        if frame == "rig":
            c, s = rig_frame_exact(t)
        else:
            c, s = [mp.mpf(0)] * 3, mp.mpf(1)
        Ps = []
        for k in range(C):
            Rt = _m(R[k]).T
            tc = mp.matrix([(mp.mpf(float(t[k, a])) - c[a]) / s for a in range(3)])
            Rt4 = mp.matrix(3, 4)
            Rt4[:, 0:3] = Rt
            Rt4[:, 3] = -(Rt * tc)
            Ps.append(_m(K[k]) * Rt4)
    return Ps, c, s


def dlt_point_exact(Ps, c, s, obs):
    """Ps, c, s of projection_matrices_exact; obs: list of (camera, u, v) (fp64 values; the caller has applied the gates).
    -> xyz as three mpf (world coordinates)."""
    with mp.workdps(DIGITS):
        A = mp.matrix(2 * len(obs), 4)
        for i, (k, u, v) in enumerate(obs):
            P = Ps[k]
            u, v = mp.mpf(float(u)), mp.mpf(float(v))
            for a in range(4):
                A[2 * i, a] = u * P[2, a] - P[0, a]
                A[2 * i + 1, a] = v * P[2, a] - P[1, a]
        E, Q = mp.eigsy(A.T * A)
        k0 = min(range(4), key=lambda i: E[i])
        e = [Q[a, k0] for a in range(4)]
        return [c[a] + s * e[a] / e[3] for a in range(3)]


def dlt_point(K, R, t, obs, frame="rig"):
    """One point -> np.float64 [3] (the exact answer rounded once)."""
    Ps, c, s = projection_matrices_exact(K, R, t, frame)
    return np.array([float(x) for x in dlt_point_exact(Ps, c, s, obs)])


def reproject_exact(Ps, c, s, X, k):
    """pixel (u, v) as mpf of the world point X (three mpf) in camera k."""
    with mp.workdps(DIGITS):
        x = mp.matrix([(X[a] - c[a]) / s for a in range(3)] + [mp.mpf(1)])
        p = Ps[k] * x
        return p[0] / p[2], p[1] / p[2]


def robust_point_exact(Ps, c, s, obs, tau, max_drops):
    """The rule of method = DLT_ROBUST (snowmocap_amd/robust.py, steps 2-4) for one joint in 50-digit arithmetic.
    obs: list of (camera, u, v) of the views that pass the gates (two or more, increasing camera).
    -> (xyz [3 mpf], views bit mask, resid mpf in pixels, margin: the smallest relative gap over the decisions taken, inf if none)."""
    with mp.workdps(DIGITS):
        tau2 = mp.mpf(tau) ** 2

        def solve(sub):
            X = dlt_point_exact(Ps, c, s, sub)
            r2 = []
            for k, u, v in sub:
                pu, pv = reproject_exact(Ps, c, s, X, k)
                r2.append((pu - mp.mpf(float(u))) ** 2 + (pv - mp.mpf(float(v))) ** 2)
            return X, r2

        S = list(obs)
        X, r2 = solve(S)
        d = 0
        margin = mp.inf
        while len(S) >= 3 and d < max_drops:
            m = max(r2)
            if tau2 != mp.inf and tau2 > 0:
                margin = min(margin, abs(m - tau2) / tau2)
            if not m > tau2:
                break
            cands = [solve(S[:i] + S[i + 1:]) for i in range(len(S))]
            ms = [max(cr2) for _, cr2 in cands]
            best = min(range(len(S)), key=lambda i: (ms[i], i))
            rest = sorted(ms[i] for i in range(len(S)) if i != best)
            if rest and rest[0] > 0:
                margin = min(margin, (rest[0] - ms[best]) / rest[0])
            S = S[:best] + S[best + 1:]
            X, r2 = cands[best]
            d += 1
        views = 0
        for k, _, _ in S:
            views |= 1 << k
        return X, views, mp.sqrt(mp.fsum(r2) / len(r2)), margin
