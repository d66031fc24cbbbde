"""Row N4 on the CPU: what the references of tests/test_gpu_undistort.py are worth, before any kernel runs.

  * oracle/undistort_exact.py is an inverse of the forward model, not a second iteration: forward_exact(exact_inverse(p)) = p to
    1e-30 px in 50-digit arithmetic on every pixel of every pool (tests/undistort_cases.py), and the exact inverse of the
    float64-rounded raw pixel is the true pixel to that rounding divided by the Jacobian's smallest eigenvalue;
  * every lens is invertible over the pixel box: the smallest eigenvalue of the forward Jacobian (normalised coordinates) is >= 0.3;
  * oracle/undistort.py::undistort_pixels (fp64 Newton) is within 1e-12 px of the exact inverse on every pixel of every pool, both
    dtypes -- which is what pins that file;
  * the premise of the GPU wave tests: under the wave-uniform exit rule the kernel used to have, the bits of >= 1 % of the
    observations of the (40, 1, 133) float64 case depend on how they are aligned to their waves, with and without a NaN per 64 lanes.
"""
import numpy as np
import pytest

import undistort_cases as uc

CAMERAS = [(r, c) for r in uc.RIGS for c in range(uc.RIGS[r][0])]
MIN_EIG = 0.3


def _grid(n=61, m=37):
    u, v = np.meshgrid(np.linspace(*uc.BOX[0], n), np.linspace(*uc.BOX[1], m), indexing="ij")
    return np.stack([u, v], axis=-1)


def test_lenses_are_invertible_over_the_pixel_box():
    from oracle import undistort_exact as ue
    worst = {}
    for r, c in CAMERAS:
        K, _, _, D, names = uc.rig(r)
        lam = min(ue.jacobian_min_eig(K[c], D[c], _grid()).min(), ue.jacobian_min_eig(K[c], D[c], uc.pool(r, c)["true"]).min())
        worst[names[c]] = min(worst.get(names[c], np.inf), lam)
        assert np.abs((_grid()[..., 0] - K[c, 0, 2]) / K[c, 0, 0]).max() <= 1.2          # (the |x| the GPU bound assumes)
    print("    smallest eigenvalue of the forward Jacobian over the box, per lens:", {k: round(float(v), 3) for k, v in worst.items()})
    assert set(worst) == set(uc.LENSES)
    for name, lam in worst.items():
        assert lam >= MIN_EIG, (name, lam)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_exact_inverse_round_trip(dtype_name):
    from oracle import undistort_exact as ue
    worst = 0.0
    for r, c in CAMERAS:
        p = uc.pool(r, c, dtype_name)
        assert np.isfinite(p["inv"]).all()
        worst = max(worst, p["roundtrip"].max())
        assert p["roundtrip"].max() < 1e-30, (r, c, p["roundtrip"].max())
        if dtype_name == "float32":
            assert np.array_equal(p["raw"], p["raw"].astype(np.float32).astype(np.float64))
            continue
        # raw = forward(true) rounded to float64: |d raw| <= half a spacing per coordinate.  In pixels the forward Jacobian is
        # A Jn A^-1 (A = [[fx, s], [0, fy]]), so its inverse amplifies by at most cond(A) / lambda_min(Jn); then one rounding of inv.
        K, _, _, D, _ = uc.rig(r)
        A = K[c][:2, :2]
        lam = ue.jacobian_min_eig(K[c], D[c], p["true"])
        draw = 0.5 * np.linalg.norm(np.spacing(np.abs(p["raw"])), axis=-1)
        bound = 1.01 * np.linalg.cond(A) * draw / lam + 0.5 * np.linalg.norm(np.spacing(np.abs(p["inv"])), axis=-1)
        err = np.linalg.norm(p["inv"] - p["true"], axis=-1)
        assert (err <= bound).all(), (r, c, (err / bound).max())
    print(f"    {dtype_name}: max |forward_exact(exact_inverse(p)) - p| = {worst:.2e} px over {len(CAMERAS) * uc.POOL} pixels")


def test_exact_inverse_rejects_what_it_cannot_invert():
    from oracle import undistort_exact as ue
    K, _, _, D, _ = uc.rig("floor")
    with pytest.raises(ValueError):
        ue.exact_inverse(K[0], D[0], [[np.nan, 3.0]])
    with pytest.raises(ValueError):
        ue.exact_inverse(K[0], D[0], [[np.inf, 3.0]])
    # zero coefficients: the inverse is the identity, exactly
    uv = uc.pool("floor", 0)["raw"][:5]
    assert np.array_equal(ue.exact_inverse(K[0], np.zeros(5), uv), uv) and np.array_equal(ue.forward_exact(K[0], np.zeros(5), uv), uv)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_oracle_newton_against_the_exact_inverse(dtype_name):
    """What pins oracle/undistort.py: <= 1e-12 px from the exact inverse (one ulp of a 1300 px coordinate is 2.3e-13)."""
    from oracle import undistort as ou
    worst = {}
    for r, c in CAMERAS:
        K, _, _, D, names = uc.rig(r)
        p = uc.pool(r, c, dtype_name)
        err = np.abs(ou.undistort_pixels(K[c], D[c], p["raw"]) - p["inv"]).max()
        worst[names[c]] = max(worst.get(names[c], 0.0), err)
        assert err <= 1e-12, (r, c, names[c], err)
        # and the forward restatement against the exact forward model
        if dtype_name == "float64":
            assert np.abs(ou.distort_pixels(K[c], D[c], p["true"]) - p["raw"]).max() <= 1e-12
    print(f"    {dtype_name}: max |undistort_pixels - exact inverse| per lens (px):", {k: f"{v:.2e}" for k, v in worst.items()})


def test_cases_are_deterministic_and_draw_from_the_pools():
    for r in uc.RIGS:
        assert len(uc.shapes_of(r)) == len(uc.SHAPES) + (uc.RIGS[r][0] == 4)
    a = uc.case("ring5", (3, 1, 17))
    uc.case.cache_clear()
    b = uc.case("ring5", (3, 1, 17))
    assert all(np.array_equal(a[k], b[k]) for k in ("kpts", "want", "true"))
    assert a["kpts"].shape == (3, 5, 1, 17, 3) and not a["kpts"].flags.writeable
    assert len(set(a["lenses"])) == 5 and all(len(set(uc.rig(r)[4])) == uc.RIGS[r][0] for r in uc.DISTINCT_LENS_RIGS)
    K, _, _, D, _ = uc.rig("ring5")
    assert (K[:, 0, 1] >= 0.5).all() and (K[:, 0, 1] <= 4.0).all() and not uc.rig("floor-s0")[0][:, 0, 1].any()
    f32 = uc.case("ring5", (3, 1, 17), "float32")
    assert f32["kpts"].dtype == np.float32 and np.abs(f32["want"] - a["want"]).max() < 1e-3
    kp, hit = uc.poison(a["kpts"], np.nan)
    assert hit.sum() == -(-(a["kpts"].size // 3 - 37) // 64) and np.isnan(kp[hit][:, :2]).all() and np.array_equal(kp[~hit], a["kpts"][~hit])


def test_the_recording_can_show_the_fault_too():
    """The premise of the BatchTriangulator wave test: in uc.recording() a person's joints sit within ~300 px, so most lenses need
    the same step count across a wave; under the strong barrel lens (camera 2 of the floor rig) they do not."""
    rec = uc.recording()
    assert uc.rig(uc.WAVE_RIG)[4][2] == "strong-barrel"
    raw = rec["kpts"][:, 2, 0, :, :2].reshape(-1, 2)
    a = uc.emulate_wave_uniform(rec["K"][2], rec["D"][2], raw, first_wave=64)
    b = uc.emulate_wave_uniform(rec["K"][2], rec["D"][2], raw, first_wave=20)
    differ = (a.view(np.uint64) != b.view(np.uint64)).any(axis=-1)
    print(f"    recording, camera 2: {int(differ.sum())} of {differ.size} observations change bits with the wave alignment")
    assert differ.sum() >= 0.01 * differ.size


@pytest.mark.parametrize("how", ["alignment", "nan-per-64"])
def test_wave_uniform_exit_makes_bits_depend_on_the_wave(how):
    """The premise of test_gpu_undistort.py's wave tests, on the reference alone: the data can show the fault.
    alignment: the same observations with a first wave of 64 and of 20 lanes (a 17 + 23 frame split shifts them by 20 mod 64).
    nan-per-64: one observation in each 64 set to NaN against the clean run at the same alignment, which is what the GPU test
    compares.  (Two ALIGNMENTS of the poisoned data cannot differ: a NaN in every wave holds every wave to the bound of 8 steps, and
    then every lane takes the same number of steps whichever wave it sits in.)"""
    cs = uc.case(uc.WAVE_RIG, uc.WAVE_SHAPE)
    assert cs["lenses"][0] == "shipped"
    raw = cs["kpts"][:, 0, 0, :, :2].reshape(-1, 2).copy()               # camera 0: 40 x 133 observations in lane order
    keep = np.ones(raw.shape[0], dtype=bool)
    a = uc.emulate_wave_uniform(cs["K"][0], cs["D"][0], raw, first_wave=64)
    if how == "alignment":
        b = uc.emulate_wave_uniform(cs["K"][0], cs["D"][0], raw, first_wave=20)
    else:
        keep[37::64] = False
        raw[~keep] = np.nan
        b = uc.emulate_wave_uniform(cs["K"][0], cs["D"][0], raw, first_wave=64)
        assert np.isnan(b[~keep]).all()
    want = cs["want"][:, 0, 0].reshape(-1, 2)
    assert np.abs(a - want)[keep].max() < 1e-11 and np.abs(b - want)[keep].max() < 1e-11     # both ARE the answer, to rounding
    differ = (a.view(np.uint64) != b.view(np.uint64)).any(axis=-1) & keep
    print(f"    {how}: {int(differ.sum())} of {int(keep.sum())} observations change bits, by up to {np.abs(a - b)[keep].max():.2e} px")
    assert differ.sum() >= 0.01 * keep.sum()
